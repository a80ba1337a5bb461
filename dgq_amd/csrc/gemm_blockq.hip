// gemm_blockq.hip — the W4A8 / W8A8 layer under the real-time BLOCK activation quantiser (quant_block.hip): one (δ, β) per row and
// 32-chunk of K, so the per-M kernels (one scale per row) and the per-K kernels (one scale per chunk, shared by all rows) cannot
// express it.  The K loop here keeps NO running total: every 32-chunk is one mfma_i32_32x32x32_i8 into a ZEROED accumulator, then
//   accf[r] = fma(β[m_r, c], Vc[n, c], fma(δ[m_r, c], float(P[r]), accf[r]))           r = 0..15, chunks in ascending order
// with m_r the row of accumulator register r (gemm_tile.h: (r & 3) + 8·(r >> 2) + 4·(lane >> 5)) and n the lane's column; the rest
// is the family's dequantising store epilogue gemm_store_tile<false, ...> with gamma = bias and rowsum R[m] = Σ_c δ·rs:
// dgq_dequant<false> gives ga + al·(accf − zw·R).  Residual, res_div bias rows, GEGLU pairs, GroupNorm partials, y2 / ldy redirects and
// 16-bit outputs are that epilogue's, not rewritten here.
//
// Operands: A = the quantiser's int8 codes [pixels][C] (MFMA rows), B = the natural-order weight image (W4: dgq_pack_w4 layout 1,
// widened as gemm_wxa8.hip does; W8: int8).  A convolution gathers: chunk c = tap·(C/32) + cb of output row m is the 32 contiguous
// code bytes, and the table entry cb, of pixel (ho·stride − pad + dh, wo·stride − pad + dw) (>> ups); outside the image codes, δ and β
// are 0, so the tap contributes exactly 0.  A Linear layer is the 1x1 case with pixel = row.
//
// One tile shape: 64 x 64 per workgroup, 8 waves (2 x 2 x 2: the two K waves of a 32x32 MFMA tile take the even / the odd chunks of
// every K tile and meet in the epilogue's LDS transposition, k = 0 first — a fixed order; the K loop is a chain of dependent
// latencies, and a second wave per SIMD overlaps them: −10 % of the SD step against one K wave), K in tiles of 256 = 8 chunks, one staged
// chunk per wave (against 4-chunk tiles: the same times — the loop is bound by the per-chunk body, not by the staging round trips;
// profiles/r12_realtime_block.txt).  Plain global -> register -> LDS staging, the loads of tile t + 1 in flight behind the MFMAs of
// tile t; thread (row = tid & 63, chunk = tid >> 6) stages the 32 code bytes, the {δ, β} pair, the weight piece and the Vc entry of its
// (row, chunk) — the chunk, hence the tap, is wave-uniform.  No K split over workgroups, no atomics, nothing exchanged between
// workgroups.  The per-chunk body — the MFMA, then cvt + 2 fma per accumulator register (48 VALU per MFMA) behind 8 broadcast LDS
// reads of {δ, β} — is what a faster loop has to attack: several MFMA tiles per wave, the β·Vc term as an fp32 MFMA pass.
#include "gemm_tile.h"

DGQ_DIAG_BUFFER(blockq)

namespace {

struct BlockqGeom {
    const float2* table; int ldt;
    const float* vc; int nchp;            // Vc row pitch = Kp / 32
    int B, H, W, Hs, Ws, C, cpb, kh, kw, stride, pad, ups, Ho, Wo;
    int nch;                              // real chunks: kh·kw·C/32
    int plain;                            // 1x1, stride 1, pad 0, no ups: pixel = row
};

constexpr int BQ_BM = 64, BQ_BN = 64, BQ_NT = 512, BQ_NW = 8;
constexpr int BQ_CH = 8;                                 // chunks per K tile = one staged chunk per wave
constexpr int BQ_A = BQ_CH * BQ_BM * 32;                   // [chunk][row][32 B]
constexpr int BQ_DB = BQ_CH * BQ_BM * 8, BQ_VC = BQ_CH * BQ_BN * 4;
constexpr int bq_w_bytes(int wbits) { return BQ_CH * BQ_BN * (wbits == 4 ? 16 : 32); }
constexpr int BQ_EP = BQ_NW * 32 * (32 + 4) * 4;             // gemm_store_tile's transposition scratch (over the idle operand images)
constexpr int bq_ring(int wbits) { return BQ_A + bq_w_bytes(wbits) + BQ_DB + BQ_VC > BQ_EP ? BQ_A + bq_w_bytes(wbits) + BQ_DB + BQ_VC : BQ_EP; }

template <int WBITS, typename TOut>
__global__ __launch_bounds__(BQ_NT) void gemm_blockq_kernel(GemmParams p, BlockqGeom q) {
    static_assert(BQ_CH == BQ_NW, "one staged chunk per wave");
    constexpr int RING = bq_ring(WBITS);
    __shared__ __attribute__((aligned(16))) uint8_t smem[RING + (3 * BQ_BM + 4 * BQ_BN) * 4];
    DGQ_DIAG_DECL
    DGQ_STAMP(0); DGQ_STAMP_REAL(1); DGQ_STAMP_WHERE(2);
    uint8_t* a_lds = smem;
    uint8_t* w_lds = smem + BQ_A;
    float2* db_lds = reinterpret_cast<float2*>(smem + BQ_A + bq_w_bytes(WBITS));
    float* vc_lds = reinterpret_cast<float*>(smem + BQ_A + bq_w_bytes(WBITS) + BQ_DB);
    float* vtab = reinterpret_cast<float*>(smem + RING);   // [3][BM]: R0 R1 R2 | [4][BN]: alpha zw gamma vn
    float* vcol = vtab + 3 * BQ_BM;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_k = wid >> 2, wave_m = (wid >> 1) & 1, wave_n = wid & 1;
    const int sch = wid;                                    // the chunk of a K tile this wave stages
    const int m0 = blockIdx.y * BQ_BM, n0 = blockIdx.x * BQ_BN;
    const int lr = lane & 31, hh = lane >> 5;

    // ---- the staged (row, chunk) of this thread: output position of the row, weight row of the column
    const int srow = lane;                                  // = tid & 63
    const int m = min(m0 + srow, p.M - 1);
    int64_t pix0;                                           // first pixel of the row's image (plain: the row's own pixel)
    int hbase = 0, wbase = 0;
    if (q.plain) {
        pix0 = m;
    } else {
        const int L = q.Ho * q.Wo;
        const int b = m / L, l = m - b * L;
        const int ho = l / q.Wo, wo = l - ho * q.Wo;
        hbase = ho * q.stride - q.pad; wbase = wo * q.stride - q.pad;
        pix0 = (int64_t)b * q.Hs * q.Ws;
    }
    const int n = min(n0 + srow, p.N - 1);
    const uint8_t* wrow = p.wpacked + (int64_t)n * (WBITS == 4 ? p.Kp / 2 : p.Kp);
    const float* vcrow = q.vc + (int64_t)n * q.nchp;

    // ---- epilogue vectors: R[m] (the in-image taps' rho in tap order), the column constants
    if (tid < BQ_BM) {
        float R = 0.0f;
        if (q.plain) {
            R = p.rowsum[pix0];
        } else {
            for (int dh = 0; dh < q.kh; ++dh)
                for (int dw = 0; dw < q.kw; ++dw) {
                    const int hi = hbase + dh, wi = wbase + dw;
                    if ((unsigned)hi < (unsigned)q.H && (unsigned)wi < (unsigned)q.W) R += p.rowsum[pix0 + (int64_t)(hi >> q.ups) * q.Ws + (wi >> q.ups)];
                }
        }
        vtab[tid] = 1.0f; vtab[BQ_BM + tid] = R; vtab[2 * BQ_BM + tid] = 0.0f;
        vcol[tid] = p.alpha[n]; vcol[BQ_BN + tid] = p.zw[n]; vcol[2 * BQ_BN + tid] = p.gamma[n]; vcol[3 * BQ_BN + tid] = 0.0f;
    }

    // ---- staging registers of one K tile
    uint4 ra0, ra1, rw0, rw1;
    float2 rdb;
    float rvc;
    auto load_tile = [&](int kt) {
        const int cc = kt * BQ_CH + sch;                    // wave-uniform chunk
        ra0 = ra1 = rw0 = rw1 = make_uint4(0u, 0u, 0u, 0u);
        rdb = make_float2(0.0f, 0.0f);
        rvc = 0.0f;
        bool in = cc < q.nch;
        int64_t pix = pix0;
        int cb = cc;
        if (!q.plain) {
            const int tap = cc / q.cpb;
            cb = cc - tap * q.cpb;
            const int dh = tap / q.kw, dw = tap - dh * q.kw;
            const int hi = hbase + dh, wi = wbase + dw;
            in = in && (unsigned)hi < (unsigned)q.H && (unsigned)wi < (unsigned)q.W;
            pix = pix0 + (int64_t)(hi >> q.ups) * q.Ws + (wi >> q.ups);
        }
        if (in) {
            const uint4* src = reinterpret_cast<const uint4*>(p.codes + pix * q.C + cb * 32);
            ra0 = src[0]; ra1 = src[1];
            rdb = q.table[pix * q.ldt + cb];
        }
        if (cc < q.nchp) {                                  // the weight image and Vc end at Kp (a multiple of 4 chunks, not of 8)
            if (WBITS == 4) {
                rw0 = *reinterpret_cast<const uint4*>(wrow + cc * 16);
            } else {
                rw0 = *reinterpret_cast<const uint4*>(wrow + cc * 32);
                rw1 = *reinterpret_cast<const uint4*>(wrow + cc * 32 + 16);
            }
            rvc = vcrow[cc];
        }
    };
    auto store_tile = [&]() {
        uint4* da = reinterpret_cast<uint4*>(a_lds + (sch * BQ_BM + srow) * 32);
        da[0] = ra0; da[1] = ra1;
        if (WBITS == 4) {
            *reinterpret_cast<uint4*>(w_lds + (sch * BQ_BN + srow) * 16) = rw0;
        } else {
            uint4* dw = reinterpret_cast<uint4*>(w_lds + (sch * BQ_BN + srow) * 32);
            dw[0] = rw0; dw[1] = rw1;
        }
        db_lds[sch * BQ_BM + srow] = rdb;
        vc_lds[sch * BQ_BN + srow] = rvc;
    };

    v16f accf[1][1];
#pragma unroll
    for (int r = 0; r < 16; ++r) accf[0][0][r] = 0.0f;
    const int arow = wave_m * 32 + lr, wcol = wave_n * 32 + lr;
    const int nkt = (q.nch + BQ_CH - 1) / BQ_CH;
    load_tile(0);
    for (int kt = 0; kt < nkt; ++kt) {
        store_tile();
        __syncthreads();
        if (kt + 1 < nkt) load_tile(kt + 1);
#pragma unroll
        for (int ii = 0; ii < BQ_CH / 2; ++ii) {
            const int ci = 2 * ii + wave_k;                 // this K wave's chunks of the tile
            if (kt * BQ_CH + ci >= q.nch) break;            // (wave-uniform: the chunks of the K padding)
            const v4i af = *reinterpret_cast<const v4i*>(a_lds + (ci * BQ_BM + arow) * 32 + hh * 16);
            v4i bf;
            if constexpr (WBITS == 4) {
                // layout 1: rows with bit 4 set keep the two 8-byte halves of a chunk exchanged (n0 is a multiple of 64)
                const uint2 v = *reinterpret_cast<const uint2*>(w_lds + (ci * BQ_BN + wcol) * 16 + ((hh ^ ((wcol >> 4) & 1)) << 3));
                bf = (v4i){(int)(v.x & 0x0F0F0F0Fu), (int)((v.x >> 4) & 0x0F0F0F0Fu), (int)(v.y & 0x0F0F0F0Fu), (int)((v.y >> 4) & 0x0F0F0F0Fu)};
            } else {
                bf = *reinterpret_cast<const v4i*>(w_lds + (ci * BQ_BN + wcol) * 32 + hh * 16);
            }
            v16i pz;
#pragma unroll
            for (int r = 0; r < 16; ++r) pz[r] = 0;
            const v16i P = __builtin_amdgcn_mfma_i32_32x32x32_i8(af, bf, pz, 0, 0, 0);
            const float vcv = vc_lds[ci * BQ_BN + wcol];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                // rows 8g + 4hh .. + 3 of the wave tile: registers 4g .. 4g + 3
                const float4* t = reinterpret_cast<const float4*>(db_lds + ci * BQ_BM + wave_m * 32 + 8 * g + 4 * hh);
                const float4 t0 = t[0], t1 = t[1];
                const float dl[4] = {t0.x, t0.z, t1.x, t1.z}, be[4] = {t0.y, t0.w, t1.y, t1.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int r = 4 * g + j;
                    accf[0][0][r] = __builtin_fmaf(be[j], vcv, __builtin_fmaf(dl[j], (float)P[r], accf[0][0][r]));
                }
            }
        }
        __syncthreads();
    }
    DGQ_STAMP(6);
    // (the barrier that ends the loop — or, with no K tile at all, none is needed: nothing was staged — has retired every read of the
    // operand images; vtab / vcol were written before the loop's first barrier)
    if (nkt == 0) __syncthreads();
    v16i acc0[1][1];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[0][0][r] = 0;
    gemm_store_tile<false, TOut, BQ_BM, BQ_BN, 2, 2, 2, RING, 1, 1>(p, 0, smem, vtab, vcol, wid, lane, wave_m, wave_n, wave_k, m0, n0, acc0, accf DGQ_DIAG_ARG);
    DGQ_STAMP(9);
    DGQ_DIAG_DRAIN();
    DGQ_STAMP(10); DGQ_STAMP_REAL(11);
    DGQ_DIAG_FLUSH(blockq, BQ_NW, wid, lane);
}

template <int WBITS>
int launch_blockq(const GemmParams& p, const BlockqGeom& q, int y_dtype, hipStream_t st) {
    const dim3 grid((p.N + BQ_BN - 1) / BQ_BN, (p.M + BQ_BM - 1) / BQ_BM), block(BQ_NT);
    switch (y_dtype) {
        case DGQ_F32: hipLaunchKernelGGL((gemm_blockq_kernel<WBITS, float>), grid, block, 0, st, p, q); break;
        case DGQ_F16: hipLaunchKernelGGL((gemm_blockq_kernel<WBITS, __half>), grid, block, 0, st, p, q); break;
        case DGQ_BF16: hipLaunchKernelGGL((gemm_blockq_kernel<WBITS, __hip_bfloat16>), grid, block, 0, st, p, q); break;
        default: dgq_set_error("dgq_gemm_blockq: unknown y dtype %d", y_dtype); return DGQ_EINVAL;
    }
    return dgq_launch_status("dgq_gemm_blockq");
}

}  // namespace

extern "C" int dgq_gemm_blockq(const dgq_gemm_args_t* g, const dgq_gemm_block_t* blk, void* stream) {
    DGQ_CHECK_ARG(g && blk, "dgq_gemm_blockq: null pointer");
    const dgq_gemm_args_t& a = *g;
    const dgq_gemm_block_t& k = *blk;
    DGQ_CHECK_ARG(a.codes && a.rowsum && a.wpacked && a.alpha && a.zw && a.gamma && a.y && k.table && k.vc, "dgq_gemm_blockq: null pointer");
    DGQ_CHECK_ARG(a.M > 0 && a.N > 0 && a.Kp > 0 && a.Kp % DGQ_KTILE == 0, "dgq_gemm_blockq: bad shape M=%d N=%d Kp=%d", a.M, a.N, a.Kp);
    DGQ_CHECK_ARG(a.w_bits == 4 || a.w_bits == 8, "dgq_gemm_blockq: w_bits=%d unsupported", a.w_bits);
    DGQ_CHECK_ARG(a.rowsum_parts == 1, "dgq_gemm_blockq: rowsum is the quantiser's rho, one part");
    DGQ_CHECK_ARG(k.B > 0 && k.H > 0 && k.W > 0 && k.C > 0 && k.C % DGQ_KCHUNK == 0 && k.kh > 0 && k.kw > 0 && k.stride > 0 && k.pad >= 0,
                  "dgq_gemm_blockq: bad geometry (C %% 32 == 0)");
    const int ups = k.ups ? 1 : 0;
    DGQ_CHECK_ARG(!ups || (k.H % 2 == 0 && k.W % 2 == 0), "dgq_gemm_blockq: ups needs even H, W");
    const int Ho = (k.H + 2 * k.pad - k.kh) / k.stride + 1, Wo = (k.W + 2 * k.pad - k.kw) / k.stride + 1;
    DGQ_CHECK_ARG(Ho > 0 && Wo > 0 && (int64_t)k.B * Ho * Wo == a.M, "dgq_gemm_blockq: M=%d is not B*Ho*Wo", a.M);
    const int64_t K = (int64_t)k.kh * k.kw * k.C;
    DGQ_CHECK_ARG(K <= a.Kp, "dgq_gemm_blockq: Kp=%d < kh*kw*C=%lld", a.Kp, (long long)K);
    DGQ_CHECK_ARG(k.ldt >= k.C / DGQ_KCHUNK, "dgq_gemm_blockq: table pitch %d < %d blocks", k.ldt, k.C / DGQ_KCHUNK);
    DGQ_CHECK_ARG((int64_t)k.B * k.H * k.W * k.C < (1LL << 40), "dgq_gemm_blockq: input too large");
    DGQ_CHECK_ARG((reinterpret_cast<uintptr_t>(a.codes) & 15) == 0 && (reinterpret_cast<uintptr_t>(a.wpacked) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(k.table) & 7) == 0, "dgq_gemm_blockq: codes / wpacked must be 16-byte aligned, the table 8-byte aligned");
    const int out_cols = a.extra && a.extra->geglu ? a.N / 2 : a.N;
    DGQ_CHECK_ARG(a.ldy >= out_cols, "dgq_gemm_blockq: ldy < output columns");
    GemmParams p = {};
    p.codes = a.codes; p.rowsum = a.rowsum; p.rowsum_parts = 1; p.M = a.M; p.Kp = a.Kp; p.N = a.N;
    p.wpacked = reinterpret_cast<const uint8_t*>(a.wpacked);
    p.L = 1; p.offset = a.offset; p.alpha = a.alpha; p.zw = a.zw; p.gamma = a.gamma; p.y = a.y; p.ldy = a.ldy;
    p.splits = 1; p.tiles_per_split = a.Kp / BK;
    p.ex.res_div = 1; p.ex.fq_T = 1; p.ex.fq_D = 1; p.ex.fq_qmax = 255.0f;
    if (a.extra) {
        const dgq_gemm_extra_t& e = *a.extra;
        DGQ_CHECK_ARG(!e.conv && !e.act, "dgq_gemm_blockq: no implicit-conv / quantise-on-load descriptor (the gather is this entry's own)");
        DGQ_CHECK_ARG(e.fq_mode >= 0 && e.fq_mode <= 3, "dgq_gemm_blockq: bad fq_mode");
        DGQ_CHECK_ARG(e.fq_mode == 0 || (e.fq_delta && e.fq_zp && e.fq_T > 0 && e.fq_D > 0), "dgq_gemm_blockq: fused quantizer needs tables");
        DGQ_CHECK_ARG(!e.residual || (e.ldr >= a.N && e.res_div >= 1 && e.res_dtype >= DGQ_F32 && e.res_dtype <= DGQ_BF16),
                      "dgq_gemm_blockq: bad residual descriptor (ldr < N, res_div < 1 or unknown dtype)");
        DGQ_CHECK_ARG(!e.geglu || (a.N % 4 == 0 && !e.residual && e.fq_mode == 0), "dgq_gemm_blockq: the GEGLU epilogue needs N %% 4 == 0 and no other extra");
        DGQ_CHECK_ARG(!e.y2 || (e.ldy2 >= a.N && !e.geglu), "dgq_gemm_blockq: y2 needs ldy2 >= N and no GEGLU epilogue");
        DGQ_CHECK_ARG(!e.gn_partial || (a.M % 16 == 0 && a.N % 4 == 0 && !e.geglu && e.fq_mode == 0 && (reinterpret_cast<uintptr_t>(e.gn_partial) & 15) == 0),
                      "dgq_gemm_blockq: GroupNorm partials need M %% 16 == 0, N %% 4 == 0, a 16-byte aligned buffer and no GEGLU / fused quantizer");
        p.ex = e;
        p.ex.conv = nullptr; p.ex.flush_coef = nullptr; p.ex.wfrag = nullptr; p.ex.act = nullptr;
        if (!e.residual) p.ex.res_div = 1;
    }
    BlockqGeom q;
    q.table = reinterpret_cast<const float2*>(k.table); q.ldt = k.ldt; q.vc = k.vc; q.nchp = a.Kp / DGQ_KCHUNK;
    q.B = k.B; q.H = k.H; q.W = k.W; q.Hs = k.H >> ups; q.Ws = k.W >> ups; q.C = k.C; q.cpb = k.C / DGQ_KCHUNK;
    q.kh = k.kh; q.kw = k.kw; q.stride = k.stride; q.pad = k.pad; q.ups = ups; q.Ho = Ho; q.Wo = Wo;
    q.nch = (int)(K / DGQ_KCHUNK);
    q.plain = (k.kh == 1 && k.kw == 1 && k.stride == 1 && k.pad == 0 && !ups) ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    return a.w_bits == 4 ? launch_blockq<4>(p, q, a.y_dtype, st) : launch_blockq<8>(p, q, a.y_dtype, st);
}
