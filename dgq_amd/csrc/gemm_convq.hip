// gemm_convq.hip — a 3x3 convolution layer of the quantized UNet as ONE launch: the activation quantiser of the unfolded operand
// INSIDE the contraction (round 6; BASELINE.json north_star: "activations group-quantized on the fly").
//
// Reference: QuantLayer.forward for a Conv2d under group quantisation (quant/quant_layer.py:626-661): F.unfold (:630-638) ->
// aqtizer on the [B, C·kh·kw, L] operand (:640-641, one (δ, z) per (channel, tap) or per output position) -> weight @ unfolded
// (input_unfolded_pseudo_conv2d, :526-574).  The two-launch form of this library materialises that operand as an int8 code matrix
// [M][Kp] in HBM (quant_act_conv_kernel: 25 MB written and read back for a 64 x 64 x 320 layer, more than its fp32 input) — the largest
// class of a step's traffic that the algorithm does not need ("what's missing" 1).  Here a workgroup owns a 4 x 8 tile of
// output positions (= the 32 rows of one MFMA tile) and ALL N <= 320 output channels (NW column waves):
//   1. the tile's (4 + kh − 1) x (8 + kw − 1) x C input patch goes to LDS once, as fp32, with the folded GroupNorm scale / shift and
//      SiLU applied (zeros outside the image: F.unfold pads before the quantiser sees the operand) — quant_act_conv_kernel's staging;
//   2. K is walked in slabs of `slab` K tiles (the A image of 32 rows x the whole Kp does not fit beside the patch): the waves gather
//      and quantise the slab's codes from the patch through the kpat table straight into the slab's LDS image — the same lane
//      mapping and arithmetic as quant_act_conv_kernel (dgq_affine_code4_fast, quant_common.h), so codes AND row sums are the
//      two-launch form's bit for bit — and
//   3. run the slab's K tiles of the quantise-on-load K loop (gemm_wfrag.h): A fragments from LDS, int4 weights streamed fragment-major into registers
//      (hand-counted waits; the stream runs on across the slab switches), per-K group flushes by summation by parts;
//   4. the dequantising store epilogue of the family (gemm_tile.h, TILED row mapping: residual / temb rows / GroupNorm partials).
// No code matrix, no row-sum vector, one launch instead of two.  LDS (C = 320, Kp = 3072): patch 75 KB + tables 8 KB + slab 40 KB +
// epilogue vectors 6 KB.  Layers it takes (dgq_gemm_conv_act_fuses): 3x3, stride 1, pad 1, W4, N % 32 == 0 and N <= 320, H % 4 == 0,
// W % 8 == 0, patch + tables + a 10-tile slab within 160 KB (C <= 340) — the C = 320 convolutions of the 64 x 64 level of SD.  Layers with
// more input channels (the concatenated up-path inputs, the 32 x 32 level) keep the two-launch form: their patch alone exceeds the LDS.
#include "gemm_wfrag.h"
#include "quant_common.h"

DGQ_DIAG_BUFFER(convq)

namespace {

constexpr int CQ_TH = 4, CQ_TW = 8;                      // output positions per workgroup: one 32-row MFMA tile
__host__ __device__ constexpr int cq_align16(int v) { return (v + 15) & ~15; }

struct ConvqLds {                                        // byte offsets of the LDS regions
    int patch, tab, tdl, rowt, slab, vtab, total;
};
__host__ __device__ inline ConvqLds convq_lds(int C, int kh, int kw, int stride, int Kp, int nw, int slab_tiles, bool per_m) {
    const int PH = (CQ_TH - 1) * stride + kh, PW = (CQ_TW - 1) * stride + kw;
    const int ep = nw * 32 * (32 + 4) * 4;               // gemm_store_tile's transposition scratch: over the (then idle) patch
    const int patch = PH * PW * C * 4;
    ConvqLds l;
    l.patch = 0;
    l.tab = cq_align16(patch > ep ? patch : ep);
    l.tdl = l.tab + cq_align16(Kp * 2);
    l.rowt = l.tdl + cq_align16(dgq_conv_rec_bytes(Kp));   // the per-chunk records (quant_common.h)
    l.slab = l.rowt + 3 * 32 * 4;
    l.vtab = l.slab + slab_tiles * 32 * BK;
    l.total = l.vtab + (3 * 32 + 4 * 32 * nw) * 4 + (per_m ? 0 : cq_align16((NCH + 1) * (Kp / BK) * 4));
    return l;
}

template <bool PER_M, typename TIO, int NW>
__global__ __launch_bounds__(64 * NW) void gemm_convq_kernel(GemmBatch bt, int slab_tiles) {
    constexpr int BM = 32, BN = 32 * NW, NT = 64 * NW;
    constexpr int ACCS = PER_M ? 1 : 2;
    const GemmParams& p = bt.p[0];
    gemm_prefetch_params(p);
    DGQ_DIAG_DECL
    DGQ_STAMP(0); DGQ_STAMP_REAL(1); DGQ_STAMP_WHERE(2);
    const dgq_gemm_act_t& act = p.act;
    const int C = act.K, H = act.H, W = act.W, kh = act.kh, kw = act.kw, stride = act.stride, pad = act.pad;
    const int Ho = (H + 2 * pad - kh) / stride + 1, Wo = (W + 2 * pad - kw) / stride + 1;
    const int tiles_w = Wo / CQ_TW, tiles_h = Ho / CQ_TH;
    // XCD-aware tile order: XCD k owns a contiguous range of tiles (neighbours share their halo rows in one L2)
    const int tile = dgq_xcd_logical(blockIdx.x, gridDim.x);
    const int b = tile / (tiles_h * tiles_w);
    const int trem = tile - b * tiles_h * tiles_w;
    const int th = trem / tiles_w, tw = trem - th * tiles_w;
    const int ho0 = th * CQ_TH, wo0 = tw * CQ_TW;
    const int m0 = (b * Ho + ho0) * Wo + wo0;              // the tile's first output position (row r = m0 + (r >> 3)·Wo + (r & 7))
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nk = p.Kp / BK;
    const ConvqLds L = convq_lds(C, kh, kw, stride, p.Kp, NW, slab_tiles, PER_M);

    // ---- W stream (gemm_wfrag.h): this wave's 32 columns, fragment-major
    const int ntile32 = (p.N + 31) >> 5;
    const int jt = min(wid, ntile32 - 1);                  // a wave past N recomputes the last column tile and stores nothing
    const uint4* wsrc = reinterpret_cast<const uint4*>(p.wfrag) + ((int64_t)jt * (nk * 2)) * 64 + lane;
    v4i wr[WF_NS][2];
    wfrag_start(wsrc, nk, wr);

    // ---- epilogue vectors and flush coefficients (table: linear over the chunks; two sequences, one K range)
    float* vtab = reinterpret_cast<float*>(smem + L.vtab);   // [3][32]: R0 R1 R2 | [4][BN]: alpha zw gamma vn
    float* vcol = vtab + 3 * BM;
    float* ctab = vcol + 4 * BN;                              // per-K: [nk·4] flush coefficients | [nk] clear flags
    const int n_coef = PER_M ? 0 : nk * NCH, n_tab = PER_M ? 0 : n_coef + nk;
    const FlushGeom fg = {ACCS, 0, nk, nk, 0};
    auto tab_ref = [&](int e) { return flush_ref(fg, e < n_coef, e < n_coef ? e : 0, e - n_coef); };
    const bool has_col = tid < BN;
    GemmColRegs cr = gemm_cols_issue<PER_M>(p, min(tid, p.N - 1));
    GemmFlushRegs fr = {};
    if constexpr (!PER_M) fr = gemm_flush_issue(p, n_tab, tid, tab_ref);

    // ---- 1. the input patch (quant_act_conv_kernel's staging: wave w takes pixels w, w + NW, ...)
    // (every load below is an ordinary one: the asm loads above are all OLDER, so hipcc's counted waits for these stay correct)
    float* patch = reinterpret_cast<float*>(smem + L.patch);
    const int PH = (CQ_TH - 1) * stride + kh, PW = (CQ_TW - 1) * stride + kw;
    const int hi0 = ho0 * stride - pad, wi0 = wo0 * stride - pad;
    {
        const TIO* img = reinterpret_cast<const TIO*>(act.x) + (int64_t)b * H * W * act.ldx;
        const float* pre_sc = act.pre_scale ? act.pre_scale + (int64_t)b * C : nullptr;
        const float* pre_sh = act.pre_scale ? act.pre_shift + (int64_t)b * C : nullptr;
        // a wave's pixels in batches of PB: every 16-byte load of a batch is issued before the first is used (one memory latency per
        // batch — pixel by pixel, each load → SiLU → LDS store chain paid its own)
        constexpr int PB = 6;
        const int npx = PH * PW;
        for (int p0 = wid; p0 < npx; p0 += NW * PB) {
            float v[PB][2][4];
            bool inb[PB];
#pragma unroll
            for (int i = 0; i < PB; ++i) {
                const int pp = min(p0 + NW * i, npx - 1);
                const int ph = pp / PW, pw_ = pp - ph * PW;
                const int hi = hi0 + ph, wi = wi0 + pw_;
                inb[i] = hi >= 0 && hi < H && wi >= 0 && wi < W;                 // wave-uniform
                const TIO* src = img + ((int64_t)min(max(hi, 0), H - 1) * W + min(max(wi, 0), W - 1)) * act.ldx;   // (clamped: loaded, then zeroed)
#pragma unroll
                for (int h = 0; h < 2; ++h) load4<TIO>(src + min(lane * 4 + 256 * h, C - 4), v[i][h]);
            }
#pragma unroll
            for (int i = 0; i < PB; ++i) {
                const int pp = p0 + NW * i;
                if (pp >= npx) break;                                            // wave-uniform
                float* dst = patch + pp * C;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int c = lane * 4 + 256 * h;
                    if (c >= C) continue;
                    float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (inb[i]) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) o[j] = v[i][h][j];
                        if (pre_sc) {
                            const float4 sc = *reinterpret_cast<const float4*>(pre_sc + c);
                            const float4 sh = *reinterpret_cast<const float4*>(pre_sh + c);
                            o[0] = o[0] * sc.x + sh.x; o[1] = o[1] * sc.y + sh.y; o[2] = o[2] * sc.z + sh.z; o[3] = o[3] * sc.w + sh.w;
                        }
                        if (act.pre_act == 1) {
#pragma unroll
                            for (int j = 0; j < 4; ++j) o[j] = dgq_silu(o[j]);
                        }
                    }
                    *reinterpret_cast<float4*>(dst + c) = make_float4(o[0], o[1], o[2], o[3]);
                }
            }
        }
    }
    DGQ_STAMP(3);                                          // (diagnostic) patch staged
    // the gather table and the chunks' records, resolved once per workgroup (quant_common.h), and the rows' (δ, z, 1/δ) into LDS
    uint16_t* tab = reinterpret_cast<uint16_t*>(smem + L.tab);
    DgqChunkRec* rec = reinterpret_cast<DgqChunkRec*>(smem + L.tdl);
    float* rowt = reinterpret_cast<float*>(smem + L.rowt);     // per-M: [3][32] δ, z, 1/δ of the tile's rows
    dgq_conv_tables_resolve<PER_M>(act.kpat, p.cdelta, act.czp, p.Kp, tab, rec, tid, NT);
    if constexpr (PER_M) {
        if (tid < 32) {
            const int li = (m0 + (tid >> 3) * Wo + (tid & 7)) % p.L;
            const float md = p.mdelta[li];
            rowt[tid] = md; rowt[32 + tid] = p.mzp[li]; rowt[64 + tid] = dgq_rcp(md);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the first W tiles and the tables
    gemm_cols_commit<PER_M, BN>(cr, vcol, tid, has_col);
    if constexpr (!PER_M) {
        gemm_flush_commit<NT>(p, fr, ctab, n_tab, tid, tab_ref);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // (long K only: ordinary loads of the loop above)
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    DGQ_STAMP(4);                                          // (diagnostic) tables staged, everyone's patch rows visible

    // ---- 2 + 3. slabs of the K range: quantise into the slab image, then its K tiles
    uint8_t* slab = smem + L.slab;
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
    // the rows this wave quantises: wid, wid + NW, ... < 32; their running row sums live across the slabs
    constexpr int RQ = (32 + NW - 1) / NW;
    float partial[RQ];
#pragma unroll
    for (int q = 0; q < RQ; ++q) partial[q] = 0.0f;
    const float qmax = (float)((1 << act.bits) - 1);
    const uint32_t bias4 = (uint32_t)(int)(128.0f - p.offset) * 0x01010101u;
    const uint32_t sh4 = 4u * (lane & 7);
    auto quantise_slab = [&](int k0, int k1) {
#pragma unroll
        for (int q = 0; q < RQ; ++q) {
            const int r = wid + NW * q;
            if (r >= 32) continue;                           // wave-uniform
            const int i = r >> 3, j = r & 7;
            const float* pr = patch + ((i * stride) * PW + j * stride) * C;
            float md = 1.0f, mz = 0.0f, minv = 1.0f;
            if (PER_M) { md = rowt[r]; mz = rowt[32 + r]; minv = rowt[64 + r]; }
            const uint32_t row_base = (uint32_t)(r * BK), row_swz = (uint32_t)(((r >> 1) & 7) << 4);
            auto store = [&](int kp0, uint32_t w) {
                const int ks = kp0 - k0;                     // position inside the slab image
                *reinterpret_cast<uint32_t*>(slab + (ks >> 7) * (BM * BK) + row_base + ((((uint32_t)ks & 127u) & ~15u) ^ row_swz) + (ks & 15)) = w;
            };
            float part = partial[q];
            // QU = 5 steps of 256 codes per round: a 10-tile slab (1280 codes) is ONE round — every table read and every gather of the row's
            // slab in flight together.  (The lane -> code mapping and each lane's ascending order are quant_act_conv_kernel's, whose rounds
            // are 4 steps: the row sums add up in the same order.)  Whole rounds test no position; the last round of the last slab is
            // the guarded form (wave-uniform skips, and the upper half-wave of a last half step when Kp is an odd multiple of 128).
            constexpr int QU = 5;
            int kbu = k0;                                    // wave-uniform round base
            for (; kbu + 256 * QU <= k1; kbu += 256 * QU)
                part = dgq_conv_quant_round<PER_M, QU, true>(pr, tab, rec, kbu, k1, lane, sh4, md, mz, minv, qmax, bias4, part, store);
            if (kbu < k1)
                part = dgq_conv_quant_round<PER_M, QU, false>(pr, tab, rec, kbu, k1, lane, sh4, md, mz, minv, qmax, bias4, part, store);
            partial[q] = part;
        }
    };
    for (int tb = 0; tb < nk; tb += WF_NS) {
        if (tb % slab_tiles == 0) {                          // (slab_tiles is a multiple of WF_NS: a slab starts at sl == 0 only)
            DGQ_STAMP_NOW(dg_s0);
            if (tb > 0) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's reads of the previous slab are complete ...
                __builtin_amdgcn_s_barrier();                        // ... everyone's
            }
            DGQ_STAMP_ACC(12, dg_s0);                                // (diagnostic) waiting for the slab image to be free
            DGQ_STAMP_NOW(dg_s1);
            quantise_slab(tb * BK, min(nk, tb + slab_tiles) * BK);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            DGQ_STAMP_ACC(7, dg_s1);                                 // (diagnostic) this wave's rows of the slab
            DGQ_STAMP_NOW(dg_s2);
            __builtin_amdgcn_s_barrier();
            DGQ_STAMP_ACC(13, dg_s2);                                // (diagnostic) waiting for the other waves' rows
        }
        const int ts0 = tb % slab_tiles;
#pragma unroll
        for (int sl = 0; sl < WF_NS; ++sl) {
            const int t = tb + sl;                            // K tile t: tile ts0 + sl of the slab image
            if (t < nk) {                                     // wave-uniform
                wfrag_acquire(wsrc, t, nk, wr, sl);
                wfrag_tile<PER_M>(slab + (ts0 + sl) * (BM * BK), a_off, ctab + t * NCH, tclr + t, wr[sl][0], wr[sl][1], acc, accf, pend);
            }
        }
    }
    if constexpr (!PER_M) gemm_flush<true>(accf, acc[1], pend);
    DGQ_STAMP(6);
    // the rows' epilogue constants R0 R1 R2 (row sums complete: every slab has been quantised)
#pragma unroll
    for (int q = 0; q < RQ; ++q) {
        const int r = wid + NW * q;
        float part = partial[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) part += __shfl_down(part, o, 64);
        if (r < 32 && lane == 0) {
            float r0v = 1.0f, r1v = part, r2v = 0.0f;
            if (PER_M) { const float md = rowt[r]; r0v = md; r1v = md * part; r2v = md * (p.offset - rowt[32 + r]); }
            vtab[r] = r0v; vtab[BM + r] = r1v; vtab[2 * BM + r] = r2v;
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // this wave's slab reads are complete, its vtab rows written ...
    __builtin_amdgcn_s_barrier();                            // ... everyone's: the patch region becomes the epilogue's scratch
    gemm_store_tile<PER_M, TIO, BM, BN, 1, NW, 1, NW * 32 * (32 + 4) * 4, 1, 1, true>(p, 0, smem + L.patch, vtab, vcol, wid, lane, 0, wid, 0, m0, 0,
                                                                                      acc[0], accf DGQ_DIAG_ARG, Wo, tile * 2);
    DGQ_STAMP(9);
    DGQ_DIAG_DRAIN();
    DGQ_STAMP(10); DGQ_STAMP_REAL(11);
    DGQ_DIAG_FLUSH(convq, NW, wid, lane);
}

template <bool PER_M, typename TIO, int NW>
int launch_convq(const GemmBatch& bt, int slab_tiles, int lds, hipStream_t st) {
    const dgq_gemm_act_t& a = bt.p[0].act;
    const int Ho = (a.H + 2 * a.pad - a.kh) / a.stride + 1, Wo = (a.W + 2 * a.pad - a.kw) / a.stride + 1;
    static std::atomic<bool> attr_set[64];
    dgq_allow_dynamic_lds(attr_set, {{&gemm_convq_kernel<PER_M, TIO, NW>, 160 * 1024}});
    const dim3 grid(a.B * (Ho / CQ_TH) * (Wo / CQ_TW)), block(64 * NW);
    hipLaunchKernelGGL((gemm_convq_kernel<PER_M, TIO, NW>), grid, block, lds, st, bt, slab_tiles);
    return DGQ_OK;
}

}  // namespace

// The slab length (K tiles, a multiple of 5 = the weight ring's slots) and LDS bytes of a convolution in this form, or 0 where it does
// not take the layer.  Shapes only; the caller checks pointers and dtypes.
int dgq_gemm_convq_plan(int B, int H, int W, int C, int kh, int kw, int stride, int pad, int N, int Kp, int w_bits, bool per_m, int* lds_bytes) {
    if (kh != 3 || kw != 3 || stride != 1 || pad != 1 || w_bits != 4 || B < 1 || C < 4 || C % 4 != 0 || C > 512 || H % CQ_TH != 0 || W % CQ_TW != 0 ||
        (N != 160 && N != 320) || Kp % BK != 0 || Kp < C * kh * kw)
        return 0;
    const int nk = Kp / BK, nw = N / 32;
    if ((CQ_TH + kh - 1) * (CQ_TW + kw - 1) * C >= 0xFFFF) return 0;      // 16-bit patch indices
    // a slab is a multiple of 5 K tiles (the weight ring's slots: a slab starts at slot 0) and — unless it is the only one — of 2 (its first
    // code a multiple of 256: every lane keeps the code positions quant_act_conv_kernel gives it, so the row sums add up in that order)
    const int one = (nk + 4) / 5 * 5;
    const int cand[3] = {one <= 20 ? one : 20, 20, 10};
    for (int i = 0; i < 3; ++i) {
        const int s = cand[i] < one ? cand[i] : one;
        const ConvqLds l = convq_lds(C, kh, kw, stride, Kp, nw, s, per_m);
        if (l.total <= 160 * 1024 - 64) {
            if (lds_bytes) *lds_bytes = l.total;
            return s;
        }
    }
    return 0;
}

int dgq_launch_gemm_convq(const GemmBatch& bt, bool per_m, int y_dtype, int slab_tiles, int lds, hipStream_t st) {
    const int nw = bt.p[0].N / 32;
#define CQ_NW(PM, T) (nw == 10 ? launch_convq<PM, T, 10>(bt, slab_tiles, lds, st) : launch_convq<PM, T, 5>(bt, slab_tiles, lds, st))
#define CQ_PM(T) (per_m ? CQ_NW(true, T) : CQ_NW(false, T))
    switch (y_dtype) {
        case DGQ_F32: return CQ_PM(float);
        case DGQ_F16: return CQ_PM(__half);
        case DGQ_BF16: return CQ_PM(__hip_bfloat16);
        default: dgq_set_error("dgq_gemm_wxa8: unknown y dtype %d", y_dtype); return DGQ_EINVAL;
    }
#undef CQ_PM
#undef CQ_NW
}
