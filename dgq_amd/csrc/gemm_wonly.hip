// Weight-only state from the packed codes (use_wq = True, use_aq = False: BASELINE config 1): y = x · ŵᵀ + b with unquantised
// activations, where ŵ = δ_n·(q − z_n) is formed from the W4 / W8 codes of the natural-order image (PackedWeight.natural()) while a
// K tile is staged into LDS — no fp32 copy of the weight exists.  The numbers are those of dgq_conv2d_f32w on the dequantised weight,
// bit for bit: fp32-input MFMA is a k-ordered fmaf chain, so the only freedom is the M x N tiling and the MFMA shape; the chain runs
// from +0.0f over k = 0 .. K−1 in (tap, c) order without a K split, continues with +0 products to the next multiple of 16 (where that
// kernel's last 16-deep tile ends), and `+ bias` (0.0f without one) and one rounding to y's dtype follow.  Past that, padding rows and
// columns carry −0 · +0 products: the identity of the fp32 add, so a longer tile changes no bit.
//
// Two forms, 256 threads (2 x 2 waves), 32-deep K tiles through a double-buffered LDS with the global loads of tile t+2 in flight
// while tile t is multiplied:
//   WQ_T64: 64 x 64 workgroup tile, a 32 x 32 wave tile on V_MFMA_F32_32X32X2_F32 (64-cycle issue = latency: throughput form);
//   WQ_T32: 32 x 32 workgroup tile, a 16 x 16 wave tile on V_MFMA_F32_16X16X4_F32 (40-cycle dependent latency per 4 k against 64 per
//           2 k: the chain of a long-K, small-M layer is 3.2x shorter).
// wq_pick chooses between them from the number of waves each launches and the length of its chain.
#include "quant_common.h"

typedef float v16f __attribute__((ext_vector_type(16)));

struct WqParams {
    const void* x;           // [B][Hs][Ws][C] channels-last (Hs = H, or H/2 under ups), x_dtype
    const uint8_t* w;        // natural-order image: W4 [N][Kp/2] (dgq_pack_w4 layout 1) or W8 [N][Kp] int8 (code − 128)
    const float* delta;      // [N]
    const float* zp;         // [N]
    const float* bias;       // [N] or nullptr
    void* y;                 // [M][ldy], y_dtype
    int x_dtype, y_dtype, w_bits, ups, geglu;
    int B, H, W, C, kh, kw, stride, pad, Hs, Ws, Ho, Wo, N, K, K16, Kp, M, ldy;
};

__device__ __forceinline__ void wq_store(void* p, int dtype, int64_t i, float v) {
    if (dtype == DGQ_F16) reinterpret_cast<__half*>(p)[i] = __float2half(v);
    else if (dtype == DGQ_BF16) reinterpret_cast<__hip_bfloat16*>(p)[i] = __float2bfloat16(v);
    else reinterpret_cast<float*>(p)[i] = v;
}
__device__ __forceinline__ float wq_load1(const void* p, int dtype, int64_t i) {
    if (dtype == DGQ_F16) return __half2float(reinterpret_cast<const __half*>(p)[i]);
    if (dtype == DGQ_BF16) return __bfloat162float(reinterpret_cast<const __hip_bfloat16*>(p)[i]);
    return reinterpret_cast<const float*>(p)[i];
}

#define WQ_BK 32
#define WQ_RS (WQ_BK + 4)        // LDS row pitch in floats: 16-byte aligned rows for the vector writes

template <int MF, int BM, int BN>
struct WqCfg {
    static constexpr int KG = 64 / MF;                 // lane groups along k of one MFMA (2: 32x32x2, 4: 16x16x4)
    static constexpr int UA = BM * (WQ_BK / 4) / 256;  // activation units (row, 4 consecutive k) per thread
    static constexpr int BU = BN * (WQ_BK / 8);        // weight units (row, 8 consecutive k) per tile: thread tid < BU owns one
    static_assert(BM == 2 * MF && BN == 2 * MF, "2 x 2 waves, one MFMA tile each");
    static_assert(UA >= 1 && BU <= 256, "staging roles");
};

// the staged operands of one K tile, in registers between their global loads and their LDS writes
template <int UA>
struct WqRegs {
    float a[UA][4];
    uint32_t b0, b1;          // W4: b0 = the word of 8 codes; W8: b0, b1 = 8 int8 codes
};

template <int MF, int BM, int BN>
__global__ __launch_bounds__(256) void wq_gemm_kernel(WqParams p) {
    using Cfg = WqCfg<MF, BM, BN>;
    constexpr int UA = Cfg::UA, KG = Cfg::KG;
    __shared__ __attribute__((aligned(16))) float As[2][BM][WQ_RS];
    __shared__ __attribute__((aligned(16))) float Bs[2][BN][WQ_RS];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;

    // ---- activation staging role: rows (tid >> 3) + 32·i of the tile, k = 4·(tid & 7) .. +3 of every K tile
    const int ja = tid & 7;
    int ab[UA], ahb[UA], awb[UA];
    bool am_ok[UA];
#pragma unroll
    for (int i = 0; i < UA; ++i) {
        const int m = m0 + (tid >> 3) + 32 * i;
        am_ok[i] = m < p.M;
        const int mm = am_ok[i] ? m : 0;
        const int L = p.Ho * p.Wo;
        const int b = mm / L, l = mm - b * L;
        const int ho = l / p.Wo, wo = l - ho * p.Wo;
        ab[i] = b;
        ahb[i] = ho * p.stride - p.pad;
        awb[i] = wo * p.stride - p.pad;
    }
    // four consecutive k in one tap, read as one vector: C % 4 == 0 and x aligned to the vector (kernel-uniform)
    const int xsz = p.x_dtype == DGQ_F32 ? 4 : 2;
    const bool avec = (p.C & 3) == 0 && (reinterpret_cast<uintptr_t>(p.x) & (4 * xsz - 1)) == 0;
    // (tap, c) of this thread's first k in the next tile to load, advanced by WQ_BK per tile (no division per element)
    int tc = 4 * ja, tdh = 0, tdw = 0;
    while (tc >= p.C) {
        tc -= p.C;
        if (++tdw == p.kw) { tdw = 0; ++tdh; }
    }

    // ---- weight staging role: row tid >> 2 of the tile, k = 8·(tid & 3) .. +7
    const bool bown = tid < Cfg::BU;
    const int bn = n0 + (tid >> 2), jb = tid & 3;
    const bool bn_ok = bown && bn < p.N;
    const float bd = bn_ok ? p.delta[bn] : 0.0f, bz = bn_ok ? p.zp[bn] : 0.0f;
    const int64_t brow = (int64_t)(bn_ok ? bn : 0) * (p.w_bits == 4 ? p.Kp / 2 : p.Kp);
    const int bswap = (p.w_bits == 4 && (bn & 16)) ? 2 : 0;          // layout 1: rows with n & 16 keep word w at w ^ 2

    const int T = (p.K16 + WQ_BK - 1) / WQ_BK;

    auto load_tile = [&](int t, WqRegs<UA>& r) {
        const int kb = t * WQ_BK + 4 * ja;
        // padding past K: +0 up to the old chain's end (K16), −0 beyond it
        const float padv = kb < p.K16 ? 0.0f : -0.0f;
#pragma unroll
        for (int i = 0; i < UA; ++i) {
            if (avec) {
                const int hi = ahb[i] + tdh, wi = awb[i] + tdw;
                const bool ok = am_ok[i] && kb < p.K && hi >= 0 && hi < p.H && wi >= 0 && wi < p.W;
                float v[4] = {kb < p.K ? 0.0f : padv, kb < p.K ? 0.0f : padv, kb < p.K ? 0.0f : padv, kb < p.K ? 0.0f : padv};
                if (ok) {
                    const int64_t pix = p.ups ? ((int64_t)ab[i] * p.Hs + (hi >> 1)) * p.Ws + (wi >> 1)
                                              : ((int64_t)ab[i] * p.H + hi) * p.W + wi;
                    const int64_t xi = pix * p.C + tc;
                    if (p.x_dtype == DGQ_F32) load4<float>(reinterpret_cast<const float*>(p.x) + xi, v);
                    else if (p.x_dtype == DGQ_BF16) load4<__hip_bfloat16>(reinterpret_cast<const __hip_bfloat16*>(p.x) + xi, v);
                    else load4<__half>(reinterpret_cast<const __half*>(p.x) + xi, v);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) r.a[i][e] = v[e];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = kb + e;
                    float v = k < p.K16 ? 0.0f : -0.0f;
                    if (k < p.K && am_ok[i]) {
                        const int tap = k / p.C, c = k - tap * p.C;
                        const int dh = tap / p.kw, dw = tap - dh * p.kw;
                        const int hi = ahb[i] + dh, wi = awb[i] + dw;
                        if (hi >= 0 && hi < p.H && wi >= 0 && wi < p.W) {
                            const int64_t pix = p.ups ? ((int64_t)ab[i] * p.Hs + (hi >> 1)) * p.Ws + (wi >> 1)
                                                      : ((int64_t)ab[i] * p.H + hi) * p.W + wi;
                            v = wq_load1(p.x, p.x_dtype, pix * p.C + c);
                        }
                    }
                    r.a[i][e] = v;
                }
            }
        }
        tc += WQ_BK;
        while (tc >= p.C) {
            tc -= p.C;
            if (++tdw == p.kw) { tdw = 0; ++tdh; }
        }
        // weights: k < round_up(K16, 32) <= Kp, so the load stays inside row bn
        r.b0 = r.b1 = 0u;
        if (bn_ok) {
            const int k = t * WQ_BK + 8 * jb;
            if (p.w_bits == 4) {
                r.b0 = *reinterpret_cast<const uint32_t*>(p.w + brow + 4 * ((k >> 3) ^ bswap));
            } else {
                const uint2 q = *reinterpret_cast<const uint2*>(p.w + brow + k);
                r.b0 = q.x; r.b1 = q.y;
            }
        }
    };

    auto store_tile = [&](int t, int buf, const WqRegs<UA>& r) {
#pragma unroll
        for (int i = 0; i < UA; ++i)
            *reinterpret_cast<float4*>(&As[buf][(tid >> 3) + 32 * i][4 * ja]) = make_float4(r.a[i][0], r.a[i][1], r.a[i][2], r.a[i][3]);
        if (bown) {
            const int k = t * WQ_BK + 8 * jb;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float q;
                if (p.w_bits == 4) q = (float)((r.b0 >> (8 * (e & 3) + 4 * (e >> 2))) & 15u);      // dgq_pack_w4: code j at bits 8(j&3) + 4(j>>2)
                else q = (float)((int)(int8_t)(((e < 4 ? r.b0 : r.b1) >> (8 * (e & 3))) & 0xFFu) + 128);
                // ŵ = δ·(q − z): one subtract, one multiply (dequantized_weight's two tensor ops; -ffp-contract=off)
                const float wv = bd * (q - bz);
                v[e] = (bn_ok && k + e < p.K) ? wv : 0.0f;
            }
            *reinterpret_cast<float4*>(&Bs[buf][tid >> 2][8 * jb]) = make_float4(v[0], v[1], v[2], v[3]);
            *reinterpret_cast<float4*>(&Bs[buf][tid >> 2][8 * jb + 4]) = make_float4(v[4], v[5], v[6], v[7]);
        }
    };

    // ---- this wave's MFMA tile
    const int wm = (wid >> 1) * MF, wn = (wid & 1) * MF;
    const int lr = lane % MF, lk = lane / MF;
    typedef float vacc __attribute__((ext_vector_type(MF == 32 ? 16 : 4)));
    vacc acc;
#pragma unroll
    for (int r = 0; r < (MF == 32 ? 16 : 4); ++r) acc[r] = 0.0f;

    auto compute = [&](int buf) {
#pragma unroll
        for (int kk = 0; kk < WQ_BK; kk += KG) {
            const float av = As[buf][wm + lr][kk + lk];
            const float bv = Bs[buf][wn + lr][kk + lk];
            if constexpr (MF == 32) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
            else acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
        }
    };

    // ---- main loop: two register sets, loads of tile t+2 issued before tile t is multiplied
    WqRegs<UA> r0, r1;
    load_tile(0, r0);
    if (T > 1) load_tile(1, r1);
    store_tile(0, 0, r0);
    __syncthreads();
    for (int t = 0; t < T; t += 2) {
        if (t + 2 < T) load_tile(t + 2, r0);
        compute(0);
        if (t + 1 < T) store_tile(t + 1, 1, r1);
        __syncthreads();
        if (t + 1 >= T) break;
        if (t + 3 < T) load_tile(t + 3, r1);
        compute(1);
        if (t + 2 < T) store_tile(t + 2, 0, r0);
        __syncthreads();
    }

    // ---- epilogue: + bias, one rounding; geglu: packed row 2i -> column i, 2i + 1 -> column i + N/2
    const int n = n0 + wn + lr;
    if (n >= p.N) return;
    const float bias = p.bias ? p.bias[n] : 0.0f;
    const int col = p.geglu ? ((n >> 1) + (n & 1) * (p.N >> 1)) : n;
    if constexpr (MF == 32) {
        // C/D layout: column = lane & 31, row = (r & 3) + 8·(r >> 2) + 4·(lane >> 5)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * lk;
            if (m < p.M) wq_store(p.y, p.y_dtype, (int64_t)m * p.ldy + col, acc[r] + bias);
        }
    } else {
        // C/D layout: column = lane & 15, row = 4·(lane >> 4) + r
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + wm + 4 * lk + r;
            if (m < p.M) wq_store(p.y, p.y_dtype, (int64_t)m * p.ldy + col, acc[r] + bias);
        }
    }
}

// Tile choice from SIMD cycles (MI355X: 1024 SIMDs; one resident wave per SIMD and round assumed): a T64 wave issues K/2
// 32x32x2 MFMAs at 64 cycles; a T32 wave K/4 16x16x4 MFMAs at 32 cycles of issue (x 1.25 for its larger share of LDS traffic per
// MFMA) but never faster than its 40-cycle dependent chain.
static int wq_pick(int M, int N, int K) {
    const double w64 = (double)((M + 63) / 64) * ((N + 63) / 64) * 4, w32 = (double)((M + 31) / 32) * ((N + 31) / 32) * 4;
    const double r64 = (double)(int64_t)((w64 + 1023) / 1024), r32 = (double)(int64_t)((w32 + 1023) / 1024);
    const double t64 = r64 * (K / 2.0) * 64.0;
    double t32 = r32 * (K / 4.0) * 32.0 * 1.25;
    if (t32 < (K / 4.0) * 40.0) t32 = (K / 4.0) * 40.0;
    return t32 < t64 ? 32 : 64;
}

extern "C" int dgq_conv2d_wq(const void* x, int x_dtype, int B, int H, int W, int C, int kh, int kw, int stride, int pad, int upsample,
                             const uint8_t* w_packed, int w_bits, int Kp, const float* delta, const float* zp, const float* bias, int N,
                             int geglu_rows, void* y, int y_dtype, int ldy, void* stream) {
    DGQ_CHECK_ARG(x && w_packed && delta && zp && y, "dgq_conv2d_wq: null pointer");
    DGQ_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && kh > 0 && kw > 0 && stride > 0 && pad >= 0, "dgq_conv2d_wq: bad geometry");
    DGQ_CHECK_ARG((x_dtype == DGQ_F32 || x_dtype == DGQ_F16 || x_dtype == DGQ_BF16) && (y_dtype == DGQ_F32 || y_dtype == DGQ_F16 || y_dtype == DGQ_BF16),
                  "dgq_conv2d_wq: unknown dtype");
    DGQ_CHECK_ARG(w_bits == 4 || w_bits == 8, "dgq_conv2d_wq: w_bits=%d (4 or 8)", w_bits);
    DGQ_CHECK_ARG(N > 8, "dgq_conv2d_wq: N=%d (N <= 8 layers stay on dgq_conv2d_f32w)", N);
    DGQ_CHECK_ARG(ldy >= N, "dgq_conv2d_wq: ldy=%d < N=%d", ldy, N);
    DGQ_CHECK_ARG(!geglu_rows || N % 2 == 0, "dgq_conv2d_wq: geglu_rows needs an even N");
    DGQ_CHECK_ARG(!upsample || (H % 2 == 0 && W % 2 == 0), "dgq_conv2d_wq: upsample needs an even H, W");
    const int64_t K = (int64_t)kh * kw * C;
    DGQ_CHECK_ARG(Kp > 0 && Kp % DGQ_KTILE == 0 && Kp >= K, "dgq_conv2d_wq: Kp=%d must be a multiple of %d and >= kh·kw·C = %lld",
                  Kp, DGQ_KTILE, (long long)K);
    WqParams p;
    p.x = x; p.w = w_packed; p.delta = delta; p.zp = zp; p.bias = bias; p.y = y;
    p.x_dtype = x_dtype; p.y_dtype = y_dtype; p.w_bits = w_bits; p.ups = upsample ? 1 : 0; p.geglu = geglu_rows ? 1 : 0;
    p.B = B; p.H = H; p.W = W; p.C = C; p.kh = kh; p.kw = kw; p.stride = stride; p.pad = pad;
    p.Hs = upsample ? H / 2 : H; p.Ws = upsample ? W / 2 : W;
    p.Ho = (H + 2 * pad - kh) / stride + 1; p.Wo = (W + 2 * pad - kw) / stride + 1;
    DGQ_CHECK_ARG(p.Ho > 0 && p.Wo > 0, "dgq_conv2d_wq: empty output");
    const int64_t M = (int64_t)B * p.Ho * p.Wo;
    DGQ_CHECK_ARG(M < (1LL << 31) - 64, "dgq_conv2d_wq: M too large");
    p.N = N; p.K = (int)K; p.K16 = (int)((K + 15) / 16 * 16); p.Kp = Kp; p.M = (int)M; p.ldy = ldy;
    if (wq_pick(p.M, N, p.K) == 32) {
        dim3 grid((p.M + 31) / 32, (N + 31) / 32);
        DGQ_CHECK_ARG(grid.y <= 65535, "dgq_conv2d_wq: N too large");
        hipLaunchKernelGGL((wq_gemm_kernel<16, 32, 32>), grid, dim3(256), 0, (hipStream_t)stream, p);
    } else {
        dim3 grid((p.M + 63) / 64, (N + 63) / 64);
        DGQ_CHECK_ARG(grid.y <= 65535, "dgq_conv2d_wq: N too large");
        hipLaunchKernelGGL((wq_gemm_kernel<32, 64, 64>), grid, dim3(256), 0, (hipStream_t)stream, p);
    }
    return dgq_launch_status("dgq_conv2d_wq");
}
