// gemm_mx6.hip — the W4 layer under the real-time MXFP6 activation quantiser (quant_mx6.hip) on the block-scaled matrix cores: every K
// step is v_mfma_scale_f32_32x32x64_f8f6f4 with both operands FP6 E2M3.  The instruction takes one E8M0 scale per lane = per (row,
// 32-element K block), which is exactly the quantiser's block: ONE fp32 accumulator for the whole K, no per-chunk VALU, no table reads
// (against gemm_blockq.hip: cvt + 2 fma per accumulator register and chunk behind 8 LDS reads of {δ, β}).
//   y[m,n] = gamma[n] + alpha[n]·Σ_c 2^(E[m,c]+1)·Σ_{k∈c} a[m,k]·w6[n,k]
// A = the activation codes [pixels][C/32][24 B], scale_a = the lane's own (row, block) byte; B = the weight image of dgq_pack_w_mx6:
// the E2M3 codes of (q − z)/2 — exact for integer z and |q − z| <= 15 — with the constant block scale 2^1 (byte 128).  No zero-point
// terms: the epilogue is the family's gemm_store_tile<false, ...> with R = 0, zw = 0, gamma = bias, alpha = δw (residual, res_div, GEGLU
// pairs, GroupNorm partials, y2 / ldy redirects and 16-bit outputs are that epilogue's).
//
// Operand maps (pinned by the one-hot tests of tests/test_gpu_realtime_mxfp6.py): lane l holds row / column l & 31 and the K block
// l >> 5 of the 64-deep step — 32 consecutive k as the 192-bit little-endian string of their 6-bit codes in the first six registers
// (element j at bits 6j .. 6j + 5), and its scale in byte 0 of the scale register.
//
// The gather, tile and wave layout are gemm_blockq.hip's: 64 x 64 per workgroup, 8 waves (2 x 2 x 2, the two K waves meet in the
// epilogue's LDS transposition, k = 0 first), K tiles of 8 chunks, thread (row = tid & 63, chunk = tid >> 6) stages the 24 code bytes, the
// scale byte and the weight piece of its (row, chunk); one MFMA covers the chunk pair (2i, 2i + 1), one chunk per lane half.  Chunk c =
// tap·(C/32) + cb of output row m reads pixel (ho·stride − pad + dh, wo·stride − pad + dw) (>> ups); a tap outside the image (and the K
// padding) stages zero codes under the scale 2^0 and contributes exactly 0.  The LDS images keep 32 bytes per (row, chunk) — a lane
// reads 16 + 8 of them, as gemm_blockq.hip's fragment reads are spaced; the HBM images stay at 24.  No K split, no atomics.
#include "gemm_tile.h"

DGQ_DIAG_BUFFER(mx6)

typedef int v8i __attribute__((ext_vector_type(8)));

namespace {

struct Mx6Geom {
    const uint8_t* scale; int lds;
    int B, H, W, Hs, Ws, C, cpb, kh, kw, stride, pad, ups, Ho, Wo;
    int nch;                              // real chunks: kh·kw·C/32
    int nchp;                             // chunks of the weight image: Kp / 32
    int plain;                            // 1x1, stride 1, pad 0, no ups: pixel = row
};

constexpr int MX_BM = 64, MX_BN = 64, MX_NT = 512, MX_NW = 8;
constexpr int MX_CH = 8;                                 // chunks per K tile = one staged chunk per wave
constexpr int MX_A = MX_CH * MX_BM * 32, MX_W = MX_CH * MX_BN * 32;      // [chunk][row][32 B], 24 used
constexpr int MX_SC = MX_CH * MX_BM;                                     // [chunk][row] scale bytes
constexpr int MX_EP = MX_NW * 32 * (32 + 4) * 4;             // gemm_store_tile's transposition scratch (over the idle operand images)
constexpr int MX_RING = MX_A + MX_W + MX_SC > MX_EP ? MX_A + MX_W + MX_SC : MX_EP;

template <typename TOut>
__global__ __launch_bounds__(MX_NT) void gemm_mx6_kernel(GemmParams p, Mx6Geom q) {
    static_assert(MX_CH == MX_NW, "one staged chunk per wave");
    __shared__ __attribute__((aligned(16))) uint8_t smem[MX_RING + (3 * MX_BM + 4 * MX_BN) * 4];
    DGQ_DIAG_DECL
    DGQ_STAMP(0); DGQ_STAMP_REAL(1); DGQ_STAMP_WHERE(2);
    uint8_t* a_lds = smem;
    uint8_t* w_lds = smem + MX_A;
    uint8_t* sc_lds = smem + MX_A + MX_W;
    float* vtab = reinterpret_cast<float*>(smem + MX_RING);   // [3][BM]: R0 R1 R2 | [4][BN]: alpha zw gamma vn
    float* vcol = vtab + 3 * MX_BM;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_k = wid >> 2, wave_m = (wid >> 1) & 1, wave_n = wid & 1;
    const int sch = wid;                                    // the chunk of a K tile this wave stages
    const int m0 = blockIdx.y * MX_BM, n0 = blockIdx.x * MX_BN;
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
    const uint8_t* wrow = p.wpacked + (int64_t)n * q.nchp * 24;
    const int64_t apitch = (int64_t)q.cpb * 24;             // code bytes per pixel

    // ---- epilogue vectors: no row terms (R = 0), the column constants with zw = 0
    if (tid < MX_BM) {
        vtab[tid] = 1.0f; vtab[MX_BM + tid] = 0.0f; vtab[2 * MX_BM + tid] = 0.0f;
        vcol[tid] = p.alpha[n]; vcol[MX_BN + tid] = 0.0f; vcol[2 * MX_BN + tid] = p.gamma[n]; vcol[3 * MX_BN + tid] = 0.0f;
    }

    // ---- staging registers of one K tile
    uint2 ra0, ra1, ra2, rw0, rw1, rw2;
    uint32_t rsc;
    auto load_tile = [&](int kt) {
        const int cc = kt * MX_CH + sch;                    // wave-uniform chunk
        ra0 = ra1 = ra2 = rw0 = rw1 = rw2 = make_uint2(0u, 0u);
        rsc = 127u;                                         // zero codes under 2^0: exactly 0
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
            const uint2* src = reinterpret_cast<const uint2*>(reinterpret_cast<const uint8_t*>(p.codes) + pix * apitch + cb * 24);
            ra0 = src[0]; ra1 = src[1]; ra2 = src[2];
            rsc = q.scale[pix * q.lds + cb];
        }
        if (cc < q.nchp) {                                  // the weight image ends at Kp (a multiple of 4 chunks, not of 8)
            const uint2* src = reinterpret_cast<const uint2*>(wrow + cc * 24);
            rw0 = src[0]; rw1 = src[1]; rw2 = src[2];
        }
    };
    auto store_tile = [&]() {
        uint2* da = reinterpret_cast<uint2*>(a_lds + (sch * MX_BM + srow) * 32);
        da[0] = ra0; da[1] = ra1; da[2] = ra2;
        uint2* dw = reinterpret_cast<uint2*>(w_lds + (sch * MX_BN + srow) * 32);
        dw[0] = rw0; dw[1] = rw1; dw[2] = rw2;
        sc_lds[sch * MX_BM + srow] = (uint8_t)rsc;
    };

    v16f accf[1][1];
#pragma unroll
    for (int r = 0; r < 16; ++r) accf[0][0][r] = 0.0f;
    const int arow = wave_m * 32 + lr, wcol = wave_n * 32 + lr;
    const int nkt = (q.nch + MX_CH - 1) / MX_CH;
    load_tile(0);
    for (int kt = 0; kt < nkt; ++kt) {
        store_tile();
        __syncthreads();
        if (kt + 1 < nkt) load_tile(kt + 1);
#pragma unroll
        for (int ii = 0; ii < MX_CH / 4; ++ii) {
            const int pr = 2 * ii + wave_k;                 // this K wave's chunk pairs of the tile
            if (kt * MX_CH + 2 * pr >= q.nch) break;        // (wave-uniform: both chunks of the pair are K padding)
            const int ci = 2 * pr + hh;                     // the lane half's chunk = its K block of the 64-deep step
            const uint8_t* ap = a_lds + (ci * MX_BM + arow) * 32;
            const uint8_t* bp = w_lds + (ci * MX_BN + wcol) * 32;
            const uint4 a4 = *reinterpret_cast<const uint4*>(ap);
            const uint2 a2 = *reinterpret_cast<const uint2*>(ap + 16);
            const uint4 b4 = *reinterpret_cast<const uint4*>(bp);
            const uint2 b2 = *reinterpret_cast<const uint2*>(bp + 16);
            const int sa = sc_lds[ci * MX_BM + arow];
            const v8i af = {(int)a4.x, (int)a4.y, (int)a4.z, (int)a4.w, (int)a2.x, (int)a2.y, 0, 0};
            const v8i bf = {(int)b4.x, (int)b4.y, (int)b4.z, (int)b4.w, (int)b2.x, (int)b2.y, 0, 0};
            accf[0][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af, bf, accf[0][0], 2, 2, 0, sa, 0, 128);
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
    gemm_store_tile<false, TOut, MX_BM, MX_BN, 2, 2, 2, MX_RING, 1, 1>(p, 0, smem, vtab, vcol, wid, lane, wave_m, wave_n, wave_k, m0, n0, acc0, accf DGQ_DIAG_ARG);
    DGQ_STAMP(9);
    DGQ_DIAG_DRAIN();
    DGQ_STAMP(10); DGQ_STAMP_REAL(11);
    DGQ_DIAG_FLUSH(mx6, MX_NW, wid, lane);
}

// E2M3 code of h = (q − z)/2 for an integer d = q − z, |d| <= 15: every such h is a grid value (0.5 is the subnormal 4/8; 1 .. 7.5 in
// steps of 0.5 have at most 3 mantissa bits), so the code is read off the float's exponent and top mantissa bits, no rounding
__device__ __forceinline__ uint32_t mx6_weight_code(int d) {
    const uint32_t a = (uint32_t)(d < 0 ? -d : d);
    if (a == 0) return 0u;
    const float h = (float)a * 0.5f;
    const uint32_t hb = __float_as_uint(h);
    const uint32_t mag = h < 1.0f ? (uint32_t)(h * 8.0f) : ((((hb >> 23) - 126u) << 3) | ((hb >> 20) & 7u));
    return mag | (d < 0 ? 0x20u : 0u);
}

// one thread per (n, 32-block of the natural K order): 24 bytes
__global__ void pack_w_mx6_kernel(const uint8_t* __restrict__ codes, const float* __restrict__ zw, int N, int C, int taps, int Kp,
                                  uint32_t* __restrict__ packed) {
    const int nb = Kp / 32;
    const int K = C * taps;
    const int64_t total = (int64_t)N * nb;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int n = (int)(i / nb), blk = (int)(i - (int64_t)n * nb);
        const int z = (int)zw[n];
        uint32_t w[6] = {0u, 0u, 0u, 0u, 0u, 0u};
        for (int j = 0; j < 32; ++j) {
            const int kp = blk * 32 + j;
            uint32_t c6 = 0u;
            if (kp < K) {
                const int tap = kp / C, c = kp - tap * C;
                c6 = mx6_weight_code((int)codes[(int64_t)n * K + (int64_t)c * taps + tap] - z);
            }
            const int bit = 6 * j;
            w[bit >> 5] |= c6 << (bit & 31);
            if ((bit & 31) > 26) w[(bit >> 5) + 1] |= c6 >> (32 - (bit & 31));
        }
        for (int k = 0; k < 6; ++k) packed[i * 6 + k] = w[k];
    }
}

template <typename TOut>
void launch_mx6_t(const GemmParams& p, const Mx6Geom& q, hipStream_t st) {
    const dim3 grid((p.N + MX_BN - 1) / MX_BN, (p.M + MX_BM - 1) / MX_BM), block(MX_NT);
    hipLaunchKernelGGL((gemm_mx6_kernel<TOut>), grid, block, 0, st, p, q);
}

}  // namespace

extern "C" int dgq_pack_w_mx6(const uint8_t* codes, const float* zw, int N, int C, int taps, int Kp, uint8_t* packed, void* stream) {
    DGQ_CHECK_ARG(codes && zw && packed, "dgq_pack_w_mx6: null pointer");
    DGQ_CHECK_ARG(N > 0 && C > 0 && taps > 0 && Kp > 0 && Kp % DGQ_KTILE == 0 && (int64_t)C * taps <= Kp,
                  "dgq_pack_w_mx6: Kp=%d must be a multiple of %d and >= C*taps", Kp, DGQ_KTILE);
    DGQ_CHECK_ARG((reinterpret_cast<uintptr_t>(packed) & 3) == 0, "dgq_pack_w_mx6: packed must be 4-byte aligned");
    int64_t g = ((int64_t)N * (Kp / 32) + 255) / 256;
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL(pack_w_mx6_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, codes, zw, N, C, taps, Kp,
                       reinterpret_cast<uint32_t*>(packed));
    return dgq_launch_status("dgq_pack_w_mx6");
}

extern "C" int dgq_gemm_mx6(const dgq_gemm_args_t* g, const dgq_gemm_mx6_t* mx, void* stream) {
    DGQ_CHECK_ARG(g && mx, "dgq_gemm_mx6: null pointer");
    const dgq_gemm_args_t& a = *g;
    const dgq_gemm_mx6_t& k = *mx;
    DGQ_CHECK_ARG(a.codes && a.wpacked && a.alpha && a.gamma && a.y && k.scale, "dgq_gemm_mx6: null pointer");
    DGQ_CHECK_ARG(a.M > 0 && a.N > 0 && a.Kp > 0 && a.Kp % DGQ_KTILE == 0, "dgq_gemm_mx6: bad shape M=%d N=%d Kp=%d", a.M, a.N, a.Kp);
    DGQ_CHECK_ARG(k.B > 0 && k.H > 0 && k.W > 0 && k.C > 0 && k.C % DGQ_KCHUNK == 0 && k.kh > 0 && k.kw > 0 && k.stride > 0 && k.pad >= 0,
                  "dgq_gemm_mx6: bad geometry (C %% 32 == 0)");
    const int ups = k.ups ? 1 : 0;
    DGQ_CHECK_ARG(!ups || (k.H % 2 == 0 && k.W % 2 == 0), "dgq_gemm_mx6: ups needs even H, W");
    const int Ho = (k.H + 2 * k.pad - k.kh) / k.stride + 1, Wo = (k.W + 2 * k.pad - k.kw) / k.stride + 1;
    DGQ_CHECK_ARG(Ho > 0 && Wo > 0 && (int64_t)k.B * Ho * Wo == a.M, "dgq_gemm_mx6: M=%d is not B*Ho*Wo", a.M);
    const int64_t K = (int64_t)k.kh * k.kw * k.C;
    DGQ_CHECK_ARG(K <= a.Kp, "dgq_gemm_mx6: Kp=%d < kh*kw*C=%lld", a.Kp, (long long)K);
    DGQ_CHECK_ARG(k.lds >= k.C / DGQ_KCHUNK, "dgq_gemm_mx6: scale pitch %d < %d blocks", k.lds, k.C / DGQ_KCHUNK);
    DGQ_CHECK_ARG((int64_t)k.B * k.H * k.W * k.C < (1LL << 40), "dgq_gemm_mx6: input too large");
    DGQ_CHECK_ARG((reinterpret_cast<uintptr_t>(a.codes) & 15) == 0 && (reinterpret_cast<uintptr_t>(a.wpacked) & 15) == 0,
                  "dgq_gemm_mx6: codes / wpacked must be 16-byte aligned");
    const int out_cols = a.extra && a.extra->geglu ? a.N / 2 : a.N;
    DGQ_CHECK_ARG(a.ldy >= out_cols, "dgq_gemm_mx6: ldy < output columns");
    GemmParams p = {};
    p.codes = a.codes; p.rowsum = nullptr; p.rowsum_parts = 1; p.M = a.M; p.Kp = a.Kp; p.N = a.N;
    p.wpacked = reinterpret_cast<const uint8_t*>(a.wpacked);
    p.L = 1; p.offset = 0.0f; p.alpha = a.alpha; p.zw = nullptr; p.gamma = a.gamma; p.y = a.y; p.ldy = a.ldy;
    p.splits = 1; p.tiles_per_split = a.Kp / BK;
    p.ex.res_div = 1; p.ex.fq_T = 1; p.ex.fq_D = 1; p.ex.fq_qmax = 255.0f;
    if (a.extra) {
        const dgq_gemm_extra_t& e = *a.extra;
        DGQ_CHECK_ARG(!e.conv && !e.act, "dgq_gemm_mx6: no implicit-conv / quantise-on-load descriptor (the gather is this entry's own)");
        DGQ_CHECK_ARG(e.fq_mode >= 0 && e.fq_mode <= 3, "dgq_gemm_mx6: bad fq_mode");
        DGQ_CHECK_ARG(e.fq_mode == 0 || (e.fq_delta && e.fq_zp && e.fq_T > 0 && e.fq_D > 0), "dgq_gemm_mx6: fused quantizer needs tables");
        DGQ_CHECK_ARG(!e.residual || (e.ldr >= a.N && e.res_div >= 1 && e.res_dtype >= DGQ_F32 && e.res_dtype <= DGQ_BF16),
                      "dgq_gemm_mx6: bad residual descriptor (ldr < N, res_div < 1 or unknown dtype)");
        DGQ_CHECK_ARG(!e.geglu || (a.N % 4 == 0 && !e.residual && e.fq_mode == 0), "dgq_gemm_mx6: the GEGLU epilogue needs N %% 4 == 0 and no other extra");
        DGQ_CHECK_ARG(!e.y2 || (e.ldy2 >= a.N && !e.geglu), "dgq_gemm_mx6: y2 needs ldy2 >= N and no GEGLU epilogue");
        DGQ_CHECK_ARG(!e.gn_partial || (a.M % 16 == 0 && a.N % 4 == 0 && !e.geglu && e.fq_mode == 0 && (reinterpret_cast<uintptr_t>(e.gn_partial) & 15) == 0),
                      "dgq_gemm_mx6: GroupNorm partials need M %% 16 == 0, N %% 4 == 0, a 16-byte aligned buffer and no GEGLU / fused quantizer");
        p.ex = e;
        p.ex.conv = nullptr; p.ex.flush_coef = nullptr; p.ex.wfrag = nullptr; p.ex.act = nullptr;
        if (!e.residual) p.ex.res_div = 1;
    }
    Mx6Geom q;
    q.scale = k.scale; q.lds = k.lds; q.nchp = a.Kp / DGQ_KCHUNK;
    q.B = k.B; q.H = k.H; q.W = k.W; q.Hs = k.H >> ups; q.Ws = k.W >> ups; q.C = k.C; q.cpb = k.C / DGQ_KCHUNK;
    q.kh = k.kh; q.kw = k.kw; q.stride = k.stride; q.pad = k.pad; q.ups = ups; q.Ho = Ho; q.Wo = Wo;
    q.nch = (int)(K / DGQ_KCHUNK);
    q.plain = (k.kh == 1 && k.kw == 1 && k.stride == 1 && k.pad == 0 && !ups) ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    switch (a.y_dtype) {
        case DGQ_F32: launch_mx6_t<float>(p, q, st); break;
        case DGQ_F16: launch_mx6_t<__half>(p, q, st); break;
        case DGQ_BF16: launch_mx6_t<__hip_bfloat16>(p, q, st); break;
        default: dgq_set_error("dgq_gemm_mx6: unknown y dtype %d", a.y_dtype); return DGQ_EINVAL;
    }
    return dgq_launch_status("dgq_gemm_mx6");
}
