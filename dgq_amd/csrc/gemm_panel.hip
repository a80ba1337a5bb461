// gemm_panel.hip — the quantise-on-load member of the W4A8 GEMM family (round 5): Linear / 1x1 layers whose whole padded K fits an LDS
// panel (SD1.4: K = 320 ... 1280, after DGQ padding Kp = 384 ... 1664) run their activation quantiser (UniformAffineQuantizer.forward on
// the layer input, quant/quant_layer.py:295-299, with the LayerNorm / GroupNorm / SiLU in front of it folded in) INSIDE the GEMM launch:
// no int8 code matrix, no row-sum vector, no second launch (QuantLayer.forward, quant_layer.py:626-661, as one kernel).  Same tables,
// epilogue (gemm_tile.h) and results as dgq_quant_act + gemm_wxa8_kernel.
//
// Why (profiles/r05_small_launch_timeline.txt, s_memtime stamps of the 32x64 tile kernel on 8192 x 320 x 320 per-K): the K loop was
// 62 % of a workgroup's life at 1681 cycles per K tile for TWO MFMAs per wave — five co-resident waves per SIMD, each paying per K
// tile two LDS-DMA pieces (60-100 issue cycles each), a barrier, a counted wait, fragment reads for both operands and the ring
// bookkeeping; and in front of every such launch sits a quantise-on-load launch of about the same length that exists only to turn
// the fp32 rows into int8 codes in HBM.  The weights of a 32-row tile are read by ONE wave (no reuse), so LDS staging buys nothing.
//   * A (activation codes): the workgroup's 32 rows x the WHOLE K sit in LDS (the "panel"), written by the workgroup quantising its
//     rows itself; ONE barrier, no ring.  Image per K tile as in gemm_wxa8_kernel (128-byte rows, 16-byte pieces XOR-swizzled).
//   * W (int4): never touches LDS.  dgq_pack_w4 layout 2 stores the weights FRAGMENT-MAJOR: for every 32-column tile and every pair
//     of 32-wide K chunks one 1-KiB block in which lane l finds, at l·16, the 8 bytes of its column (l & 31) and K half (l >> 5) of
//     both chunks — one perfectly coalesced global_load_dwordx4 per two MFMA B operands, prefetched DT K tiles ahead in registers.
//   * a wave owns a 32 x 32 output tile; NW waves side by side (BN = 32·NW columns) x KW waves along K (each a contiguous
//     range of the K tiles; their partial tiles meet in LDS behind the loop, in a fixed order).
// Grid = column blocks x row blocks x problems.  (The round-5 form that took a materialised code matrix lost to the tile family inside
// the step — profiles/r05_panel_plan_in_step_ab.txt — and was removed in round 6.)
#include "gemm_wfrag.h"
#include "quant_common.h"

DGQ_DIAG_BUFFER(panel)

namespace {

template <int NW, int KW>
struct PanelCfg {
    static constexpr int BM = 32, BN = 32 * NW, NWT = NW * KW, NT = 64 * NWT;
    static constexpr int EP_BYTES = NW * BM * (32 + 4) * 4;          // the store epilogue's transposition scratch (gemm_store_tile)
    static constexpr int RED_BYTES = (KW - 1) * NW * BM * 32 * 4;    // partial tiles of the K waves 1 .. KW-1
    static constexpr int VEC_BYTES = (3 * BM + 4 * BN) * 4;
};

__host__ __device__ constexpr int align16(int v) { return (v + 15) & ~15; }
// LDS map: region 0 (the A panel; once it is idle the epilogue's scratch + the K waves' partial tiles) | vtab | vcol | ctab |
// (per-K) the chunks' δ and z
template <int NW, int KW>
__host__ __device__ constexpr int panel_region0(int nk) {
    using C = PanelCfg<NW, KW>;
    const int a = nk * C::BM * BK, e = C::EP_BYTES + C::RED_BYTES;
    return align16(a > e ? a : e);
}
__host__ __device__ constexpr int panel_ctab_bytes(bool per_m, int nk) { return per_m ? 0 : align16((NCH + 1) * nk * 4); }
template <int NW, int KW>
constexpr int panel_lds(bool per_m, int nk) {
    return panel_region0<NW, KW>(nk) + PanelCfg<NW, KW>::VEC_BYTES + panel_ctab_bytes(per_m, nk) +
           (!per_m ? nk * NCH * 16 + nk * BK * 4 : 0);      // (δ, z, 1/δ, ·) per chunk | decoded destination per source channel
}

template <bool PER_M, typename TIO, int NW, int KW>
__global__ __launch_bounds__(64 * NW * KW) void gemm_panel_kernel(GemmBatch bt, int n_major) {
    using Cfg = PanelCfg<NW, KW>;
    constexpr int BM = Cfg::BM, BN = Cfg::BN, NT = Cfg::NT, NWT = Cfg::NWT;
    constexpr int ACCS = PER_M ? 1 : 2;                      // two accumulator sets: a chunk's flush issues behind the next chunk's MFMA
    const GemmParams& p = bt.p[bt.n > 1 ? blockIdx.z : 0];
    const int zsplit = bt.n > 1 ? 0 : blockIdx.z;
    gemm_prefetch_params(p);
    // XCD-aware tile order (as gemm_wxa8_kernel): XCD k owns a contiguous range of tiles — row-block major when the activations are
    // the larger operand, column-block major (n_major) when the weights are: the big operand is then fetched by one XCD's L2 only.
    int tile_n, tile_m;
    {
        const int gx = gridDim.x, gy = gridDim.y;
        const int logical = dgq_xcd_logical(blockIdx.x + gx * blockIdx.y, gx * gy);
        if (n_major) { tile_n = logical / gy; tile_m = logical - tile_n * gy; }
        else { tile_m = logical / gx; tile_n = logical - tile_m * gx; }
    }
    if (tile_n * BN >= p.N || tile_m * BM >= p.M) return;   // batch: a narrower problem than the grid (whole block)
    DGQ_DIAG_DECL
    DGQ_STAMP(0); DGQ_STAMP_REAL(1); DGQ_STAMP_WHERE(2);
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nq = wid % NW, kq = wid / NW;                  // column tile / K range of this wave
    const int n0 = tile_n * BN, m0 = tile_m * BM;
    const int nk_total = p.Kp / BK;
    const int kt_begin = zsplit * p.tiles_per_split;
    const int kt_end = min(nk_total, kt_begin + p.tiles_per_split);
    const int nk = kt_end - kt_begin;
    // K range of this wave inside the slice: tiles [w_t0, w_t0 + w_nk)
    const int per_kw = (nk + KW - 1) / KW;
    const int w_t0 = kq * per_kw;
    const int w_nk = max(0, min(nk - w_t0, per_kw));

    // ---- W stream (gemm_wfrag.h): this wave's 32 columns of its K range, fragment-major
    const int ntile32 = (p.N + 31) >> 5;
    const int jt = min(tile_n * NW + nq, ntile32 - 1);      // a wave past N recomputes the last column tile and stores nothing
    const uint4* wsrc = reinterpret_cast<const uint4*>(p.wfrag) + ((int64_t)jt * (nk_total * 2) + (kt_begin + w_t0) * 2) * 64 + lane;
    v4i wr[WF_NS][2];
    wfrag_start(wsrc, w_nk, wr);

    // ---- tables (as gemm_wxa8_kernel: asm loads at clamped indices, retired by one wait)
    const int region0 = panel_region0<NW, KW>(nk);
    float* vtab = reinterpret_cast<float*>(smem + region0);  // [3][BM]: R0 R1 R2 | [4][BN]: alpha zw gamma vn
    float* vcol = vtab + 3 * BM;
    float* ctab = vcol + 4 * BN;                              // [nk·4] flush coefficients | [nk] clear flags
    // per-K: [nk·NCH] float4 (δ, z, 1/δ, ·) of the chunks | [<= nk·BK] per source channel: panel offset of its code byte at row 0 with
    // swizzle 0 (bits 0-19) and its chunk (bits 20-31) — the per-element work of the scatter is then one xor-add and one table read
    float4* tq = reinterpret_cast<float4*>(reinterpret_cast<uint8_t*>(ctab) + panel_ctab_bytes(PER_M, nk));
    uint32_t* tdst = reinterpret_cast<uint32_t*>(tq + nk * NCH);
    static_assert(BM <= NT && BN <= NT, "one row / column of the epilogue vectors per thread");
    // flush table: linear over the slice's chunks; a chunk belongs to the K wave whose tile range holds it and, inside that wave, to
    // sequence (chunk mod ACCS)
    const int n_coef = PER_M ? 0 : nk * NCH, n_tab = PER_M ? 0 : n_coef + nk;
    const FlushGeom fg = {ACCS, kt_begin, nk, nk_total, per_kw};
    auto tab_ref = [&](int e) { return flush_ref(fg, e < n_coef, kt_begin * NCH + (e < n_coef ? e : 0), e - n_coef); };
    const bool final_ep = (p.splits == 1);
    const bool has_col = final_ep && tid < BN;
    GemmColRegs cr = gemm_cols_issue<PER_M>(p, min(n0 + tid, p.N - 1));
    GemmFlushRegs fr = {};
    if constexpr (!PER_M) fr = gemm_flush_issue(p, n_tab, tid, tab_ref);
    DGQ_STAMP(3);

    // ---- the activation quantiser of the layer (dgq_quant_act's arithmetic) on this workgroup's BM rows, written into the
    // panel image.  QL lanes share a row (64 / QL rows per wave at a time); per-M / scalar scales: natural K order, four codes per
    // dword store; per-K: each source channel's code byte goes to its packed position kdst[c] (padding stays zero).
    // (every load below is an ordinary one: the asm loads above are all OLDER, so hipcc's counted waits for these stay correct)
    {
        const dgq_gemm_act_t& act = p.act;
        const TIO* x = reinterpret_cast<const TIO*>(act.x);
        const int K = act.K;
        const float qmax = (float)((1 << act.bits) - 1), aoff = (float)(1 << (act.bits - 1));
        if constexpr (!PER_M) {
            for (int i = tid; i < nk * NCH; i += NT) {
                const float dl = p.cdelta[kt_begin * NCH + i];
                tq[i] = make_float4(dl, act.czp[kt_begin * NCH + i], dgq_rcp(dl), 0.0f);
            }
            for (int c = tid; c < K; c += NT) {
                const int kp = act.kdst[c];
                tdst[c] = (uint32_t)((kp >> 7) * (BM * BK) + (kp & 127)) | ((uint32_t)(kp >> 5) << 20);
            }
            for (int i = tid * 16; i < nk * BM * BK; i += NT * 16) *reinterpret_cast<uint4*>(smem + i) = make_uint4(0, 0, 0, 0);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
        DGQ_STAMP(14);
        constexpr int QL = (NWT >= 8) ? 16 : 8;              // lanes per row
        constexpr int RPWV = 64 / QL, RP = NWT * RPWV;       // rows per wave / per pass of the workgroup
        constexpr int SEG = 4;                               // 16-byte loads per lane in flight per round (5 spills: 168 VGPRs + scratch)
        const int sl = lane % QL, rw = lane / QL;
        auto panel_addr = [&](int row, int kp) {
            return (kp >> 7) * (BM * BK) + row * BK + ((((kp & 127) >> 4) ^ ((row >> 1) & 7)) << 4) + (kp & 15);
        };
        for (int r0 = 0; r0 < BM; r0 += RP) {
            const int row = r0 + wid * RPWV + rw;
            const bool rv = row < BM;
            const int m = min(m0 + min(row, BM - 1), p.M - 1);
            const TIO* xr = x + (int64_t)m * act.ldx;
            float mu = 0.0f, rstd = 1.0f;
            // (every load of a round goes out unconditionally at a clamped address — a load under `if (c < K)` makes hipcc branch around
            // it and wait for each one before the next is issued: five dependent round trips per pass of a 320-wide row)
            if (act.ln_gamma) {
                // LayerNorm statistics of the row: two passes (mean, then Σ(x − mean)²) in the summation order of quant_act.hip's
                // row_layernorm_stats — that kernel gives a row to 64 lanes, lane v owning columns 4v + 256i; here a row's QL lanes
                // each stand for the 64/QL lanes v = sl + QL·u of it and merge them in the order of its xor-shuffle tree (offsets 32,
                // 16, (8)), then finish the tree among themselves: mean and rstd — and with them the codes — equal the two-launch
                // form's bit for bit (the second pass re-reads the row from L1)
                constexpr int NU = 64 / QL;
                float sv[NU];
#pragma unroll
                for (int u = 0; u < NU; ++u) sv[u] = 0.0f;
                for (int i0 = 0; i0 < K; i0 += 256) {
                    float v[NU][4];
#pragma unroll
                    for (int u = 0; u < NU; ++u) load4<TIO>(xr + min(i0 + (sl + QL * u) * 4, K - 4), v[u]);
#pragma unroll
                    for (int u = 0; u < NU; ++u) {
                        const float t4 = (v[u][0] + v[u][1]) + (v[u][2] + v[u][3]);
                        sv[u] += (i0 + (sl + QL * u) * 4 < K) ? t4 : 0.0f;
                    }
                }
                auto tree = [&](float (&a)[NU]) {
#pragma unroll
                    for (int h = NU / 2; h > 0; h >>= 1)
#pragma unroll
                        for (int u = 0; u < h; ++u) a[u] += a[u + h];
                    float r = a[0];
#pragma unroll
                    for (int o = QL / 2; o > 0; o >>= 1) r += __shfl_xor(r, o, 64);
                    return r;
                };
                mu = tree(sv) / (float)K;
#pragma unroll
                for (int u = 0; u < NU; ++u) sv[u] = 0.0f;
                for (int i0 = 0; i0 < K; i0 += 256) {
                    float v[NU][4];
#pragma unroll
                    for (int u = 0; u < NU; ++u) load4<TIO>(xr + min(i0 + (sl + QL * u) * 4, K - 4), v[u]);
#pragma unroll
                    for (int u = 0; u < NU; ++u) {
                        float q4 = sv[u];
#pragma unroll
                        for (int e = 0; e < 4; ++e) q4 += (v[u][e] - mu) * (v[u][e] - mu);
                        sv[u] = (i0 + (sl + QL * u) * 4 < K) ? q4 : sv[u];
                    }
                }
                rstd = 1.0f / sqrtf(tree(sv) / (float)K + act.ln_eps);
            }
            DGQ_STAMP(15);
            const int img = act.pre_scale ? m / act.rows_per_image : 0;
            const float* psc = act.pre_scale ? act.pre_scale + (int64_t)img * K : nullptr;
            const float* psh = act.pre_scale ? act.pre_shift + (int64_t)img * K : nullptr;
            float rmd = 1.0f, rmz = 0.0f, rinv = 1.0f;
            if constexpr (PER_M) {
                const int li = m % p.L;
                rmd = p.mdelta[li]; rmz = p.mzp[li]; rinv = dgq_rcp(rmd);
            }
            const float bias = 128.0f - aoff;
            float partial = 0.0f;
            const uint32_t row_base = (uint32_t)(row * BK), row_swz = (uint32_t)(((row >> 1) & 7) << 4);
            const int kend = PER_M ? nk * BK : K;            // per-M also writes the zero codes of the K padding
            for (int c0 = sl * 4; c0 < kend; c0 += 4 * QL * SEG) {
                float v[SEG][4];
                int4 kd[SEG];
                float4 f0[SEG], f1[SEG];                     // folded norm: scale / shift (GroupNorm) or gamma / beta (LayerNorm)
#pragma unroll
                for (int j = 0; j < SEG; ++j) {
                    const int cc = min(c0 + j * 4 * QL, K - 4);
                    load4<TIO>(xr + cc, v[j]);
                    if constexpr (!PER_M) kd[j] = *reinterpret_cast<const int4*>(tdst + cc);
                }
                DGQ_STAMP_NOW(dg_q0);
                if (psc) {
#pragma unroll
                    for (int j = 0; j < SEG; ++j) {
                        const int cc = min(c0 + j * 4 * QL, K - 4);
                        f0[j] = *reinterpret_cast<const float4*>(psc + cc);
                        f1[j] = *reinterpret_cast<const float4*>(psh + cc);
                    }
                } else if (act.ln_gamma) {
#pragma unroll
                    for (int j = 0; j < SEG; ++j) {
                        const int cc = min(c0 + j * 4 * QL, K - 4);
                        f0[j] = *reinterpret_cast<const float4*>(act.ln_gamma + cc);
                        f1[j] = *reinterpret_cast<const float4*>(act.ln_beta + cc);
                    }
                }
#ifdef DGQ_DIAG
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                asm volatile("" : "+v"(v[0][0]), "+v"(v[1][0]), "+v"(v[2][0]), "+v"(v[3][0]));
#endif
                DGQ_STAMP_ACC(12, dg_q0);                                  // (diagnostic) the round's loads
                DGQ_STAMP_NOW(dg_q1);
#pragma unroll
                for (int j = 0; j < SEG; ++j) {
                    const int c = c0 + j * 4 * QL;                     // (past K: the clamped load's values, computed and discarded)
                    // ... unless the whole wave is past the end (K = 320: the second round holds one segment, not four): wave-uniform
                    if (c - sl * 4 >= kend) break;
                    if (psc) {
                        v[j][0] = v[j][0] * f0[j].x + f1[j].x; v[j][1] = v[j][1] * f0[j].y + f1[j].y;
                        v[j][2] = v[j][2] * f0[j].z + f1[j].z; v[j][3] = v[j][3] * f0[j].w + f1[j].w;
                    } else if (act.ln_gamma) {
                        v[j][0] = (v[j][0] - mu) * rstd * f0[j].x + f1[j].x; v[j][1] = (v[j][1] - mu) * rstd * f0[j].y + f1[j].y;
                        v[j][2] = (v[j][2] - mu) * rstd * f0[j].z + f1[j].z; v[j][3] = (v[j][3] - mu) * rstd * f0[j].w + f1[j].w;
                    }
                    if (act.pre_act == 1) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[j][e] = dgq_silu(v[j][e]);
                    }
                    if constexpr (PER_M) {
                        {
                            const float d4[4] = {rmd, rmd, rmd, rmd}, i4[4] = {rinv, rinv, rinv, rinv}, z4[4] = {rmz, rmz, rmz, rmz};
                            float qv[4], biased[4], fsum = 0.0f;
                            dgq_affine_code4_fast(v[j], d4, i4, z4, qmax, qv);
#pragma unroll
                            for (int e = 0; e < 4; ++e) biased[e] = (c < K) ? qv[e] + bias : 128.0f;
                            const uint32_t w = dgq_pack4(biased, fsum);
                            if (rv && c < kend) *reinterpret_cast<uint32_t*>(smem + panel_addr(row, c)) = w;
                            partial += (c < kend) ? fsum - 512.0f : 0.0f;
                        }
                    } else {
                        {
                            const uint32_t dst[4] = {(uint32_t)kd[j].x, (uint32_t)kd[j].y, (uint32_t)kd[j].z, (uint32_t)kd[j].w};
                            float d4[4], i4[4], z4[4], qv[4];
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const float4 t4 = tq[dst[e] >> 20];
                                d4[e] = t4.x; z4[e] = t4.y; i4[e] = t4.z;
                            }
                            dgq_affine_code4_fast(v[j], d4, i4, z4, qmax, qv);
                            const bool live = rv && c < K;
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const float scode = qv[e] - aoff;
                                // panel_addr(row, kp) = row·BK + (offset at row 0 ^ the row's 16-byte swizzle)
                                if (live) smem[row_base + ((dst[e] & 0xFFFFFu) ^ row_swz)] = (uint8_t)(int)scode;
                                partial += (c < K) ? d4[e] * scode : 0.0f;
                            }
                        }
                    }
                }
                DGQ_STAMP_ACC(7, dg_q1);                                   // (diagnostic) the round's arithmetic + panel writes
            }
#pragma unroll
            for (int o = QL / 2; o > 0; o >>= 1) partial += __shfl_xor(partial, o, 64);
            if (rv && sl == 0) {                             // the row's epilogue constants: R0 R1 R2
                float r0v = 1.0f, r1v = partial, r2v = 0.0f;
                if (PER_M) { r0v = rmd; r1v = rmd * partial; r2v = rmd * (p.offset - rmz); }
                vtab[row] = r0v; vtab[BM + row] = r1v; vtab[2 * BM + row] = r2v;
            }
        }
    }

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the panel (DMA), the first W tiles and the tables
    DGQ_STAMP(4);
    gemm_cols_commit<PER_M, BN>(cr, vcol, tid, has_col);
    if constexpr (!PER_M) gemm_flush_commit<NT>(p, fr, ctab, n_tab, tid, tab_ref);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    DGQ_STAMP(5);

    // ---- K loop (gemm_wfrag.h): the wave's K tiles, slice tile w_t0 + t from stream tile t
    const int lr = lane & 31, hh = lane >> 5;
    int a_off[NCH];
#pragma unroll
    for (int cg = 0; cg < NCH; ++cg) a_off[cg] = lr * BK + (((2 * cg + hh) ^ ((lr >> 1) & 7)) << 4);
    v16i acc[ACCS][1][1];
    v16f accf[1][1];
    constexpr int ACC0 = PER_M ? 0 : DGQ_ACC_BIAS_I;         // per-K (W4): totals carry DGQ_ACC_BIAS_I (gemm_device.h)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int a = 0; a < ACCS; ++a) acc[a][0][0][r] = ACC0;
        accf[0][0][r] = 0.0f;
    }
    float pend = 0.0f;
    const float* tclr = ctab + nk * NCH;
    for (int tb = 0; tb < w_nk; tb += WF_NS) {
#pragma unroll
        for (int sl = 0; sl < WF_NS; ++sl) {
            const int t = tb + sl;
            if (t < w_nk) {                                   // wave-uniform
                wfrag_acquire(wsrc, t, w_nk, wr, sl);
                const int ts = w_t0 + t;
                wfrag_tile<PER_M>(smem + ts * (BM * BK), a_off, ctab + ts * NCH, tclr + ts, wr[sl][0], wr[sl][1], acc, accf, pend);
            }
        }
    }
    if constexpr (!PER_M) gemm_flush<true>(accf, acc[1], pend);
    DGQ_STAMP(6);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // this wave's panel reads are complete ...
    __builtin_amdgcn_s_barrier();                            // ... everyone's: region 0 becomes scratch

    // ---- the K waves' partial tiles meet in LDS (behind the epilogue's own scratch): wave (0, nq) adds those of (1, nq), (2, nq) ...
    // in that order — int32 for per-M (exact), fp32 for per-K — and stores the tile alone
    if constexpr (KW > 1) {
        uint8_t* red = smem + Cfg::EP_BYTES;
        if (kq > 0) {
            uint8_t* dst = red + ((kq - 1) * NW + nq) * (BM * 32 * 4) + lane * 16;
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                uint8_t* q = dst + r4 * 1024;
                if constexpr (PER_M) *reinterpret_cast<v4i*>(q) = (v4i){acc[0][0][0][4 * r4], acc[0][0][0][4 * r4 + 1], acc[0][0][0][4 * r4 + 2], acc[0][0][0][4 * r4 + 3]};
                else *reinterpret_cast<v4f*>(q) = (v4f){accf[0][0][4 * r4], accf[0][0][4 * r4 + 1], accf[0][0][4 * r4 + 2], accf[0][0][4 * r4 + 3]};
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (kq > 0) {
            DGQ_STAMP(9); DGQ_STAMP(10); DGQ_STAMP_REAL(11);
            DGQ_DIAG_FLUSH(panel, NWT, wid, lane);
            return;
        }
#pragma unroll
        for (int k = 1; k < KW; ++k) {
            const uint8_t* src = red + ((k - 1) * NW + nq) * (BM * 32 * 4) + lane * 16;
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                const uint8_t* q = src + r4 * 1024;
                if constexpr (PER_M) {
                    const v4i u = *reinterpret_cast<const v4i*>(q);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[0][0][0][4 * r4 + e] += u[e];
                } else {
                    const v4f u = *reinterpret_cast<const v4f*>(q);
#pragma unroll
                    for (int e = 0; e < 4; ++e) accf[0][0][4 * r4 + e] += u[e];
                }
            }
        }
    }

    gemm_store_tile<PER_M, TIO, BM, BN, 1, NW, 1, Cfg::EP_BYTES, 1, 1>(p, zsplit, smem, vtab, vcol, nq, lane, 0, nq, 0, m0, n0, acc[0],
                                                                       accf DGQ_DIAG_ARG);
    DGQ_STAMP(9);
    DGQ_DIAG_DRAIN();
    DGQ_STAMP(10); DGQ_STAMP_REAL(11);
#ifdef DGQ_DIAG
    dg.t[13] = (unsigned long long)nk | ((unsigned long long)tile_m << 16) | ((unsigned long long)tile_n << 32) | ((unsigned long long)wid << 48);
#endif
    DGQ_DIAG_FLUSH(panel, NWT, wid, lane);
}

template <bool PER_M, typename TIO, int NW, int KW>
void launch_panel(const GemmBatch& bt, hipStream_t st) {
    using Cfg = PanelCfg<NW, KW>;
    const GemmParams& p = bt.p[0];
    int maxN = 0, maxM = 0, max_tps = 0;
    size_t a_bytes = 0, w_bytes = 0;
    for (int i = 0; i < bt.n; ++i) {
        maxN = bt.p[i].N > maxN ? bt.p[i].N : maxN;
        maxM = bt.p[i].M > maxM ? bt.p[i].M : maxM;
        max_tps = bt.p[i].tiles_per_split > max_tps ? bt.p[i].tiles_per_split : max_tps;
        a_bytes += (size_t)bt.p[i].M * bt.p[i].Kp;
        w_bytes += (size_t)bt.p[i].N * bt.p[i].Kp / 2;
    }
    const int lds = panel_lds<NW, KW>(PER_M, max_tps);
    static std::atomic<bool> attr_set[64];
    dgq_allow_dynamic_lds(attr_set, {{&gemm_panel_kernel<PER_M, TIO, NW, KW>, 160 * 1024}});
    dim3 grid((maxN + Cfg::BN - 1) / Cfg::BN, (maxM + Cfg::BM - 1) / Cfg::BM, bt.n > 1 ? bt.n : p.splits), block(Cfg::NT);
    hipLaunchKernelGGL((gemm_panel_kernel<PER_M, TIO, NW, KW>), grid, block, lds, st, bt, w_bytes > a_bytes ? 1 : 0);
}

// configurations (NW, KW): key = NW·10 + KW.  (Round 5 also carried ten configurations that took a materialised code matrix — measured
// slower inside the step than the tile family, profiles/r05_panel_plan_in_step_ab.txt — and two 16-wave quantise-on-load ones that
// compiled with scratch beside the hand-counted W-stream waits: removed in round 6; the Makefile's `check-scratch` fails the build if
// any kernel of this file needs scratch.)
#define DGQ_PANEL_CONFIGS(X) X(10, 1) X(5, 1) X(5, 2) X(4, 2)

template <bool PER_M, typename TIO>
int launch_panel_cfg(const GemmBatch& bt, int nw, int kw, hipStream_t st) {
    switch (nw * 10 + kw) {
#define X(NW_, KW_) case (NW_) * 10 + (KW_): launch_panel<PER_M, TIO, NW_, KW_>(bt, st); break;
        DGQ_PANEL_CONFIGS(X)
#undef X
        default: dgq_set_error("dgq_gemm_wxa8: no panel configuration TM=1 NW=%d KW=%d", nw, kw); return DGQ_EINVAL;
    }
    return DGQ_OK;
}

}  // namespace

// does the configuration exist, and how much LDS does a launch with K slices of `tiles` K tiles need (0: no such configuration)
size_t dgq_gemm_panel_lds_bytes(int nw, int kw, bool per_m, int tiles) {
    switch (nw * 10 + kw) {
#define X(NW_, KW_) case (NW_) * 10 + (KW_): return (size_t)panel_lds<NW_, KW_>(per_m, tiles);
        DGQ_PANEL_CONFIGS(X)
#undef X
        default: return 0;
    }
}

int dgq_launch_gemm_panel(const GemmBatch& bt, bool per_m, int y_dtype, int nw, int kw, hipStream_t st) {
    switch (y_dtype) {
        case DGQ_F32: return per_m ? launch_panel_cfg<true, float>(bt, nw, kw, st) : launch_panel_cfg<false, float>(bt, nw, kw, st);
        case DGQ_F16: return per_m ? launch_panel_cfg<true, __half>(bt, nw, kw, st) : launch_panel_cfg<false, __half>(bt, nw, kw, st);
        case DGQ_BF16: return per_m ? launch_panel_cfg<true, __hip_bfloat16>(bt, nw, kw, st) : launch_panel_cfg<false, __hip_bfloat16>(bt, nw, kw, st);
        default: dgq_set_error("dgq_gemm_wxa8: unknown y dtype %d", y_dtype); return DGQ_EINVAL;
    }
}
