// Weight-only state on the 16-bit matrix cores (opt-in: QuantLayer.weight_only_mfma16):
//     y[m,n] = round_to_y( b[n] + δ[n] · Σ_k x̃[m,k] · (q[n,k] − z[n]) ),   k in (tap, c) order.
// q − z is an integer in [−15, 15] (W4) or [−255, 255] (W8): exact in bf16 (8 significant bits) and in f16 (11), and its product with
// a bf16 / f16 activation is exact in fp32.  So with 16-bit x the only rounding before the epilogue is that of the fp32 accumulation;
// against dgq_conv2d_wq (gemm_wonly.hip: the k-ordered fmaf chain of the exact-fp32 MFMA on ŵ = δ·(q − z)) the order of summation
// differs and δ moves to the epilogue, so the result is NOT bit-identical to that route.  The operands are read exactly as that kernel
// reads them: channels-last x, implicit im2col with zero padding, (h >> 1, w >> 1) under upsample, the natural-order W4 / W8 image.
//   bf16 x: V_MFMA_F32_32X32X16_BF16 / 16X16X32_BF16, x̃ = x;      f16 x: the _F16 forms, x̃ = x;
//   fp32 x: two bf16 terms, hi = bf16_rn(x), lo = bf16_rn(x − hi): two MFMAs per K step into the same accumulator, first lo, then hi;
//           x̃ = hi + lo, |x − x̃| <= 2^-16·|x| (the attention kernels' split, attn_bf16x3_dev.h, with two terms).
// One K loop per workgroup: no K split, no atomics, nothing exchanged between workgroups; the order is fixed by the shape.
//
// 256 threads (2 x 2 waves, one MFMA tile each); K tiles of BK through a double-buffered LDS held in the operand type (rows of
// BK + 8 elements: the 16-byte fragment reads of 16 consecutive rows fall on distinct banks), global loads of tile t+2 in flight
// while tile t is multiplied.  q − z is converted once, while the weight tile is staged: 8 codes -> one 16-byte LDS write.
//   T64: 64 x 64, BK 64, a 32x32x16 tile per wave;
//   T32: 32 x 32, BK 128, a 16x16x32 tile per wave — the layers with few rows launch too few workgroups to hide the memory latency
//        behind one another: what a workgroup has in flight is what counts, so its K tile is the deepest the LDS takes.
// wq16_pick chooses from the number of workgroups the 64 x 64 form launches (profiles/r13_weight_only_mfma16.txt).
#include <stdlib.h>
#include <type_traits>
#include "quant_common.h"
#include "quant_prologue.h"

typedef float v16f __attribute__((ext_vector_type(16)));
typedef __bf16 wq16_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 wq16_f16x8 __attribute__((ext_vector_type(8)));

struct Wq16Params {
    const void* x;           // [B][Hs][Ws][C] channels-last (Hs = H, or H/2 under ups), x_dtype
    const uint8_t* w;        // natural-order image: W4 [N][Kp/2] (dgq_pack_w4 layout 1) or W8 [N][Kp] int8 (code − 128)
    const float* delta;      // [N]
    const float* zp;         // [N]
    const float* bias;       // [N] or nullptr
    void* y;                 // [M][ldy], y_dtype
    int y_dtype, w_bits, ups, geglu;
    int B, H, W, C, kh, kw, stride, pad, Hs, Ws, Ho, Wo, N, K, Kp, M, ldy;
};

// The fused form (dgq_conv2d_wq_mfma16_fused): the element-wise neighbours of the layer folded into its load and its epilogue.
//     x′ = act(norm(x)) in fp32, in the order and rounding of dgq_prologue4 (quant_prologue.h); 0 EXACTLY for a tap outside the image,
//          for k >= K and for rows m >= M — padding comes after the norm and the activation, never act(shift);
//     x̃  = x′ rounded once to the operand type (bf16 / f16 x), or its two-term bf16 split (fp32 x);
//     t  = δ[n]·acc + bias[n] [+ bias_rows[b(m)][n]];   y = round_y(t [+ residual[m][n]])   or   round_y(dgq_geglu(t[2i], t[2i + 1])).
// FUSE is a template parameter: 0 is the kernel as it was (same parameter block, same registers), 1 adds the epilogue terms, 2 the
// prologue as well.  The tables of a unit's 8 channels (scale / shift of the row's image, or γ / β) are loaded in load_tile beside the
// unit's x and ride in the register set with it, so store_tile waits for nothing new; a row's image and its (mean, rstd) are the
// same for every K tile and are taken once.
struct Wq16Fuse {
    const float* pre_scale; const float* pre_shift;     // [B][C] fp32 (GroupNorm folded), or nullptr
    const float* ln_stats;                              // [M][2] (mean, rstd) (LayerNorm folded), or nullptr
    const float* ln_gamma; const float* ln_beta;        // [C]
    const void* residual; const void* bias_rows;        // [M][ldr], [B][N]: y's dtype, or nullptr
    int pre_act, ldr, geglu_out;
};
struct Wq16FusedParams : Wq16Params { Wq16Fuse f; };

__device__ __forceinline__ float wq16_load(const void* p, int dtype, int64_t i) {
    if (dtype == DGQ_F16) return __half2float(reinterpret_cast<const __half*>(p)[i]);
    if (dtype == DGQ_BF16) return __bfloat162float(reinterpret_cast<const __hip_bfloat16*>(p)[i]);
    return reinterpret_cast<const float*>(p)[i];
}
__device__ __forceinline__ void wq16_store(void* p, int dtype, int64_t i, float v) {
    if (dtype == DGQ_F16) reinterpret_cast<__half*>(p)[i] = __float2half(v);
    else if (dtype == DGQ_BF16) reinterpret_cast<__hip_bfloat16*>(p)[i] = __float2bfloat16(v);
    else reinterpret_cast<float*>(p)[i] = v;
}
__device__ __forceinline__ uint32_t wq16_bf16(float v) { return __builtin_bit_cast(unsigned short, __float2bfloat16(v)); }
__device__ __forceinline__ uint32_t wq16_f16(float v) { return __half_as_ushort(__float2half(v)); }

// F16: the operand type is f16 (x is f16), bf16 otherwise; SPLIT: x is fp32, staged as two bf16 images
template <int MF, int BK, bool F16, bool SPLIT>
struct Wq16Cfg {
    static_assert(MF == 32 || MF == 16, "32x32x16 or 16x16x32");
    static_assert(!(F16 && SPLIT), "the split is a bf16 split");
    static constexpr int BM = 2 * MF;               // workgroup tile (square): 2 x 2 waves, one MFMA tile each
    static constexpr int KM = 512 / MF;             // k of one MFMA
    static constexpr int KG = 64 / MF;              // lane groups along k: lane holds k = 8·(lane / MF) .. +7
    static constexpr int CPR = BK / 8;              // staging units (8 consecutive k: 16 bytes of LDS) per tile row
    static constexpr int RPP = 256 / CPR;           // rows one pass of the 256 threads stages
    static constexpr int U = BM / RPP;              // units per thread, of each operand
    static constexpr int PITCH = (BK + 8) * 2;      // LDS row pitch in bytes
    static constexpr int NA = SPLIT ? 2 : 1;        // activation images: [0] = x or hi, [1] = lo
    static constexpr int NACC = MF == 32 ? 16 : 4;
    static_assert(BK % KM == 0 && U >= 1 && BM % RPP == 0, "staging roles");
    static_assert((2 * NA + 2) * BM * PITCH <= 65536, "static LDS");
};

// the staged operands of one K tile, in registers between their global loads and their LDS writes
template <int U, int NA>
struct Wq16Regs {
    uint4 a[U][NA];           // 8 x 16-bit, or (SPLIT) 8 x fp32 in two vectors
    uint32_t b0[U], b1[U];    // W4: b0 = the word of 8 codes; W8: b0, b1 = 8 int8 codes
};
// ... with the prologue (FUSE 2): the norm's two tables for the unit's 8 elements and which of the 8 lie inside the image and below K
template <int U, int NA>
struct Wq16ProRegs : Wq16Regs<U, NA> {
    float ta[U][8], tb[U][8];
    uint32_t ok[U];
};

template <int MF, int BK, bool F16, bool SPLIT, int FUSE>
__device__ __forceinline__ void wq16_gemm_body(const std::conditional_t<FUSE != 0, Wq16FusedParams, Wq16Params>& p) {
    using Cfg = Wq16Cfg<MF, BK, F16, SPLIT>;
    constexpr int BM = Cfg::BM, U = Cfg::U, NA = Cfg::NA, CPR = Cfg::CPR, RPP = Cfg::RPP, PITCH = Cfg::PITCH, NACC = Cfg::NACC;
    constexpr bool PRO = FUSE == 2;
    typedef float vacc __attribute__((ext_vector_type(NACC)));
    typedef std::conditional_t<PRO, Wq16ProRegs<U, NA>, Wq16Regs<U, NA>> Regs;
    __shared__ __attribute__((aligned(16))) uint8_t As[2][NA][BM][PITCH];
    __shared__ __attribute__((aligned(16))) uint8_t Bs[2][BM][PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BM;

    // ---- staging role, the same for both operands: rows (tid / CPR) + RPP·i of the tile, k = 8·(tid % CPR) .. +7 of every K tile
    const int ju = tid % CPR, ru = tid / CPR;
    int ab[U], ahb[U], awb[U];
    bool am_ok[U];
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const int m = m0 + ru + RPP * i;
        am_ok[i] = m < p.M;
        const int mm = am_ok[i] ? m : 0;
        const int L = p.Ho * p.Wo;
        const int b = mm / L, l = mm - b * L;
        const int ho = l / p.Wo, wo = l - ho * p.Wo;
        ab[i] = b;
        ahb[i] = ho * p.stride - p.pad;
        awb[i] = wo * p.stride - p.pad;
    }
    // prologue: the norm (kernel-uniform: 0 none, 1 GroupNorm, 2 LayerNorm), the rows of its two tables and the row's statistics
    int nmode = 0;
    const float* pta[U];
    const float* ptb[U];
    float lmu[U], lrs[U];
    if constexpr (PRO) {
        nmode = p.f.pre_scale ? 1 : (p.f.ln_stats ? 2 : 0);
#pragma unroll
        for (int i = 0; i < U; ++i) {
            pta[i] = nmode == 1 ? p.f.pre_scale + (int64_t)ab[i] * p.C : p.f.ln_gamma;
            ptb[i] = nmode == 1 ? p.f.pre_shift + (int64_t)ab[i] * p.C : p.f.ln_beta;
            lmu[i] = 0.0f; lrs[i] = 1.0f;
            if (nmode == 2 && am_ok[i]) {
                const float2 st = *reinterpret_cast<const float2*>(p.f.ln_stats + 2 * (int64_t)(m0 + ru + RPP * i));
                lmu[i] = st.x; lrs[i] = st.y;
            }
        }
    }
    // eight consecutive k in one tap, read as one (fp32: two) 16-byte vector: C % 8 == 0 and x aligned to 16 bytes (kernel-uniform)
    constexpr int XSZ = SPLIT ? 4 : 2;
    const bool avec = (p.C & 7) == 0 && (reinterpret_cast<uintptr_t>(p.x) & 15) == 0;
    // (tap, c) of this thread's first k in the next tile to load, advanced by BK per tile (no division per element)
    int tc = 8 * ju, tdh = 0, tdw = 0;
    while (tc >= p.C) {
        tc -= p.C;
        if (++tdw == p.kw) { tdw = 0; ++tdh; }
    }

    bool bn_ok[U];
    float bz[U];
    int64_t brow[U];
    int bswap[U];
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const int n = n0 + ru + RPP * i;
        bn_ok[i] = n < p.N;
        bz[i] = bn_ok[i] ? p.zp[n] : 0.0f;
        brow[i] = (int64_t)(bn_ok[i] ? n : 0) * (p.w_bits == 4 ? p.Kp / 2 : p.Kp);
        bswap[i] = (p.w_bits == 4 && (n & 16)) ? 2 : 0;              // layout 1: rows with n & 16 keep word w at w ^ 2
    }

    const int T = (p.K + BK - 1) / BK;
    const uint8_t* xb = reinterpret_cast<const uint8_t*>(p.x);

    auto pixel = [&](int i, int hi, int wi) -> int64_t {
        return p.ups ? ((int64_t)ab[i] * p.Hs + (hi >> 1)) * p.Ws + (wi >> 1) : ((int64_t)ab[i] * p.H + hi) * p.W + wi;
    };

    auto load_tile = [&](int t, Regs& r) {
        const int kb = t * BK + 8 * ju;
#pragma unroll
        for (int i = 0; i < U; ++i) {
#pragma unroll
            for (int s = 0; s < NA; ++s) r.a[i][s] = make_uint4(0u, 0u, 0u, 0u);
            if (avec) {
                // kb % 8 == 0 and K % 8 == 0: kb < K covers the whole unit
                const int hi = ahb[i] + tdh, wi = awb[i] + tdw;
                const bool in = am_ok[i] && kb < p.K && hi >= 0 && hi < p.H && wi >= 0 && wi < p.W;
                if (in) {
                    const uint4* src = reinterpret_cast<const uint4*>(xb + (pixel(i, hi, wi) * p.C + tc) * XSZ);
#pragma unroll
                    for (int s = 0; s < NA; ++s) r.a[i][s] = src[s];
                }
                if constexpr (PRO) {
                    r.ok[i] = in ? 0xFFu : 0u;
                    if (nmode) {                                  // tc < C whatever kb is, and the tables are 16-byte aligned (host)
                        const float4 a0 = *reinterpret_cast<const float4*>(pta[i] + tc), a1 = *reinterpret_cast<const float4*>(pta[i] + tc + 4);
                        const float4 b0 = *reinterpret_cast<const float4*>(ptb[i] + tc), b1 = *reinterpret_cast<const float4*>(ptb[i] + tc + 4);
                        r.ta[i][0] = a0.x; r.ta[i][1] = a0.y; r.ta[i][2] = a0.z; r.ta[i][3] = a0.w;
                        r.ta[i][4] = a1.x; r.ta[i][5] = a1.y; r.ta[i][6] = a1.z; r.ta[i][7] = a1.w;
                        r.tb[i][0] = b0.x; r.tb[i][1] = b0.y; r.tb[i][2] = b0.z; r.tb[i][3] = b0.w;
                        r.tb[i][4] = b1.x; r.tb[i][5] = b1.y; r.tb[i][6] = b1.z; r.tb[i][7] = b1.w;
                    }
                }
            } else {
                uint32_t e32[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int k = kb + e;
                    e32[e] = 0u;
                    if constexpr (PRO) {
                        if (e == 0) r.ok[i] = 0u;
                        r.ta[i][e] = 1.0f; r.tb[i][e] = 0.0f;
                    }
                    if (k < p.K && am_ok[i]) {
                        const int tap = k / p.C, c = k - tap * p.C;
                        const int dh = tap / p.kw, dw = tap - dh * p.kw;
                        const int hi = ahb[i] + dh, wi = awb[i] + dw;
                        if (hi >= 0 && hi < p.H && wi >= 0 && wi < p.W) {
                            const int64_t xi = pixel(i, hi, wi) * p.C + c;
                            if (SPLIT) e32[e] = reinterpret_cast<const uint32_t*>(p.x)[xi];
                            else e32[e] = reinterpret_cast<const uint16_t*>(p.x)[xi];
                            if constexpr (PRO) r.ok[i] |= 1u << e;
                        }
                        if constexpr (PRO) {
                            if (nmode) { r.ta[i][e] = pta[i][c]; r.tb[i][e] = ptb[i][c]; }
                        }
                    }
                }
                if (SPLIT) {
                    r.a[i][0] = make_uint4(e32[0], e32[1], e32[2], e32[3]);
                    r.a[i][NA - 1] = make_uint4(e32[4], e32[5], e32[6], e32[7]);
                } else {
                    r.a[i][0] = make_uint4(e32[0] | (e32[1] << 16), e32[2] | (e32[3] << 16), e32[4] | (e32[5] << 16), e32[6] | (e32[7] << 16));
                }
            }
            // weights: k < round_up(K, BK) <= Kp (Kp is a multiple of DGQ_KTILE, BK divides it), so the load stays inside row n
            r.b0[i] = r.b1[i] = 0u;
            if (bn_ok[i] && kb < p.Kp) {
                if (p.w_bits == 4) {
                    r.b0[i] = *reinterpret_cast<const uint32_t*>(p.w + brow[i] + 4 * ((kb >> 3) ^ bswap[i]));
                } else {
                    const uint2 q = *reinterpret_cast<const uint2*>(p.w + brow[i] + kb);
                    r.b0[i] = q.x; r.b1[i] = q.y;
                }
            }
        }
        tc += BK;
        while (tc >= p.C) {
            tc -= p.C;
            if (++tdw == p.kw) { tdw = 0; ++tdh; }
        }
    };

    auto store_tile = [&](int t, int buf, const Regs& r) {
        const int kb = t * BK + 8 * ju;
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const int row = ru + RPP * i;
            float xp[8];                                          // x′ of the unit (FUSE 2)
            if constexpr (PRO) {
                if (SPLIT) {
                    const uint32_t f[8] = {r.a[i][0].x, r.a[i][0].y, r.a[i][0].z, r.a[i][0].w,
                                           r.a[i][NA - 1].x, r.a[i][NA - 1].y, r.a[i][NA - 1].z, r.a[i][NA - 1].w};
#pragma unroll
                    for (int e = 0; e < 8; ++e) xp[e] = __uint_as_float(f[e]);
                } else {
                    const uint32_t f[4] = {r.a[i][0].x, r.a[i][0].y, r.a[i][0].z, r.a[i][0].w};
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const uint32_t h16 = (f[e >> 1] >> (16 * (e & 1))) & 0xFFFFu;
                        xp[e] = F16 ? __half2float(__ushort_as_half((unsigned short)h16)) : __uint_as_float(h16 << 16);
                    }
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float v = xp[e];
                    if (nmode == 1) v = v * r.ta[i][e] + r.tb[i][e];
                    else if (nmode == 2) v = (v - lmu[i]) * lrs[i] * r.ta[i][e] + r.tb[i][e];
                    if (p.f.pre_act == 1) v = dgq_silu(v);
                    xp[e] = ((r.ok[i] >> e) & 1u) ? v : 0.0f;
                }
            }
            if constexpr (PRO && !SPLIT) {
                uint32_t v16[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) v16[e] = F16 ? wq16_f16(xp[e]) : wq16_bf16(xp[e]);
                *reinterpret_cast<uint4*>(&As[buf][0][row][16 * ju]) =
                    make_uint4(v16[0] | (v16[1] << 16), v16[2] | (v16[3] << 16), v16[4] | (v16[5] << 16), v16[6] | (v16[7] << 16));
            } else if (SPLIT) {
                const uint32_t f[8] = {r.a[i][0].x, r.a[i][0].y, r.a[i][0].z, r.a[i][0].w,
                                       r.a[i][NA - 1].x, r.a[i][NA - 1].y, r.a[i][NA - 1].z, r.a[i][NA - 1].w};
                uint32_t h[8], l[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float xv = PRO ? xp[e] : __uint_as_float(f[e]);
                    h[e] = wq16_bf16(xv);
                    l[e] = wq16_bf16(xv - __uint_as_float(h[e] << 16));
                }
                *reinterpret_cast<uint4*>(&As[buf][0][row][16 * ju]) =
                    make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
                *reinterpret_cast<uint4*>(&As[buf][NA - 1][row][16 * ju]) =
                    make_uint4(l[0] | (l[1] << 16), l[2] | (l[3] << 16), l[4] | (l[5] << 16), l[6] | (l[7] << 16));
            } else {
                *reinterpret_cast<uint4*>(&As[buf][0][row][16 * ju]) = r.a[i][0];
            }
            uint32_t v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float q;
                if (p.w_bits == 4) q = (float)((r.b0[i] >> (8 * (e & 3) + 4 * (e >> 2))) & 15u);      // dgq_pack_w4: code j at bits 8(j&3) + 4(j>>2)
                else q = (float)((int)(int8_t)(((e < 4 ? r.b0[i] : r.b1[i]) >> (8 * (e & 3))) & 0xFFu) + 128);
                const float wv = (bn_ok[i] && kb + e < p.K) ? q - bz[i] : 0.0f;                       // the integer q − z: exact in the operand type
                v[e] = F16 ? wq16_f16(wv) : wq16_bf16(wv);
            }
            *reinterpret_cast<uint4*>(&Bs[buf][row][16 * ju]) =
                make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
        }
    };

    // ---- this wave's MFMA tile.  A/B lane maps: lane l holds row (l % MF), k = 8·(l / MF) + j in element j of its fragment
    const int wm = (wid >> 1) * MF, wn = (wid & 1) * MF;
    const int lr = lane % MF, lk = lane / MF;
    vacc acc;
#pragma unroll
    for (int e = 0; e < NACC; ++e) acc[e] = 0.0f;

    auto mfma = [&](const uint4& a, const uint4& b, vacc c) -> vacc {
        if constexpr (F16) {
            const wq16_f16x8 av = __builtin_bit_cast(wq16_f16x8, a), bv = __builtin_bit_cast(wq16_f16x8, b);
            if constexpr (MF == 32) return __builtin_amdgcn_mfma_f32_32x32x16_f16(av, bv, c, 0, 0, 0);
            else return __builtin_amdgcn_mfma_f32_16x16x32_f16(av, bv, c, 0, 0, 0);
        } else {
            const wq16_bf16x8 av = __builtin_bit_cast(wq16_bf16x8, a), bv = __builtin_bit_cast(wq16_bf16x8, b);
            if constexpr (MF == 32) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, c, 0, 0, 0);
            else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, c, 0, 0, 0);
        }
    };

    auto compute = [&](int buf) {
#pragma unroll
        for (int kk = 0; kk < BK; kk += Cfg::KM) {
            const int ko = 2 * (kk + 8 * lk);
            uint4 a[NA];
#pragma unroll
            for (int s = 0; s < NA; ++s) a[s] = *reinterpret_cast<const uint4*>(&As[buf][s][wm + lr][ko]);
            const uint4 b = *reinterpret_cast<const uint4*>(&Bs[buf][wn + lr][ko]);
            if (SPLIT) acc = mfma(a[NA - 1], b, acc);          // first lo, then hi
            acc = mfma(a[0], b, acc);
        }
    };

    // ---- main loop: two register sets, loads of tile t+2 issued before tile t is multiplied
    Regs r0, r1;
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

    if constexpr (FUSE != 0) {
        // ---- fused epilogue: every lane stays to the end (the GEGLU exchange reads its neighbour); packed rows 2i (value) and 2i + 1
        // (gate) are adjacent columns, so adjacent lanes of the C/D layout with the same rows: one exchange, the even lane stores.
        // bias_rows and residual are the CALLER's tensors, in the output's (reference) column order: both are read at `col`, the
        // column packed row n stands for, never at the packed index (under geglu_out too: value column i, gate column i + N/2)
        const int n = n0 + wn + lr;
        const bool n_ok = n < p.N;
        const int nn = n_ok ? n : 0;
        const float dn = p.delta[nn], bias = p.bias ? p.bias[nn] : 0.0f;
        const int col = p.geglu ? ((nn >> 1) + (nn & 1) * (p.N >> 1)) : nn;
        const int L = p.Ho * p.Wo;
#pragma unroll
        for (int e = 0; e < NACC; ++e) {
            const int m = m0 + wm + (MF == 32 ? (e & 3) + 8 * (e >> 2) + 4 * lk : 4 * lk + e);
            const bool ok = n_ok && m < p.M;
            float t = dn * acc[e] + bias;
            if (p.f.bias_rows && ok) t += wq16_load(p.f.bias_rows, p.y_dtype, (int64_t)(m / L) * p.N + col);
            if (p.f.geglu_out) {
                const float g = __shfl_xor(t, 1, 64);
                if (ok && !(nn & 1)) wq16_store(p.y, p.y_dtype, (int64_t)m * p.ldy + (nn >> 1), dgq_geglu(t, g));
            } else if (ok) {
                if (p.f.residual) t += wq16_load(p.f.residual, p.y_dtype, (int64_t)m * p.f.ldr + col);
                wq16_store(p.y, p.y_dtype, (int64_t)m * p.ldy + col, t);
            }
        }
        return;
    }
    // ---- epilogue: · δ, + bias, one rounding; geglu: packed row 2i -> column i, 2i + 1 -> column i + N/2
    const int n = n0 + wn + lr;
    if (n >= p.N) return;
    const float dn = p.delta[n], bias = p.bias ? p.bias[n] : 0.0f;
    const int col = p.geglu ? ((n >> 1) + (n & 1) * (p.N >> 1)) : n;
#pragma unroll
    for (int e = 0; e < NACC; ++e) {
        // C/D layout: 32x32: column = lane & 31, row = (e & 3) + 8·(e >> 2) + 4·(lane >> 5); 16x16: column = lane & 15, row = 4·(lane >> 4) + e
        const int m = m0 + wm + (MF == 32 ? (e & 3) + 8 * (e >> 2) + 4 * lk : 4 * lk + e);
        if (m < p.M) wq16_store(p.y, p.y_dtype, (int64_t)m * p.ldy + col, dn * acc[e] + bias);
    }
}

template <int MF, int BK, bool F16, bool SPLIT>
__global__ __launch_bounds__(256) void wq16_gemm_kernel(Wq16Params p) { wq16_gemm_body<MF, BK, F16, SPLIT, 0>(p); }
template <int MF, int BK, bool F16, bool SPLIT, int FUSE>
__global__ __launch_bounds__(256) void wq16_gemm_fused_kernel(Wq16FusedParams p) { wq16_gemm_body<MF, BK, F16, SPLIT, FUSE>(p); }

// Tile choice (MI355X: 256 CUs), measured with each form forced on the 49 layer shapes of the SD UNet: the 64 x 64 form is the faster
// one where it launches at least one workgroup per CU (it stages half the bytes per output element), the 32 x 32 form everywhere
// else (four times the workgroups).  DGQ_WQ16_TILE = 32 / 64 forces a form (tools/bench_weight_only_mfma16.py measures them against
// each other; no product path sets it).
static int wq16_pick(int M, int N) {
    static const int forced = [] { const char* e = getenv("DGQ_WQ16_TILE"); return e ? atoi(e) : 0; }();
    if (forced == 32 || forced == 64) return forced;
    return (int64_t)((M + 63) / 64) * ((N + 63) / 64) >= 256 ? 64 : 32;
}

template <int MF, int BK>
static void wq16_launch(const Wq16Params& p, int x_dtype, hipStream_t stream) {
    constexpr int BM = 2 * MF;
    const dim3 grid((p.M + BM - 1) / BM, (p.N + BM - 1) / BM);
    if (x_dtype == DGQ_F32) hipLaunchKernelGGL((wq16_gemm_kernel<MF, BK, false, true>), grid, dim3(256), 0, stream, p);
    else if (x_dtype == DGQ_F16) hipLaunchKernelGGL((wq16_gemm_kernel<MF, BK, true, false>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((wq16_gemm_kernel<MF, BK, false, false>), grid, dim3(256), 0, stream, p);
}

template <int MF, int BK, int FUSE>
static void wq16_launch_fused(const Wq16FusedParams& p, int x_dtype, hipStream_t stream) {
    constexpr int BM = 2 * MF;
    const dim3 grid((p.M + BM - 1) / BM, (p.N + BM - 1) / BM);
    if (x_dtype == DGQ_F32) hipLaunchKernelGGL((wq16_gemm_fused_kernel<MF, BK, false, true, FUSE>), grid, dim3(256), 0, stream, p);
    else if (x_dtype == DGQ_F16) hipLaunchKernelGGL((wq16_gemm_fused_kernel<MF, BK, true, false, FUSE>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((wq16_gemm_fused_kernel<MF, BK, false, false, FUSE>), grid, dim3(256), 0, stream, p);
}

// The arguments the two entries share: their one check (`who` names the entry in the message), the kernel's parameter block and the tile.
// `ncols`: the columns a row of y holds (N, or N/2 where the fused epilogue forms the GEGLU).
static int wq16_setup(const char* who, const void* x, int x_dtype, int B, int H, int W, int C, int kh, int kw, int stride, int pad, int upsample,
                      const uint8_t* w_packed, int w_bits, int Kp, const float* delta, const float* zp, const float* bias, int N, int geglu_rows,
                      void* y, int y_dtype, int ldy, int ncols, Wq16Params& p, int& tile) {
    DGQ_CHECK_ARG(x && w_packed && delta && zp && y, "%s: null pointer", who);
    DGQ_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && kh > 0 && kw > 0 && stride > 0 && pad >= 0, "%s: bad geometry", who);
    DGQ_CHECK_ARG((x_dtype == DGQ_F32 || x_dtype == DGQ_F16 || x_dtype == DGQ_BF16) && (y_dtype == DGQ_F32 || y_dtype == DGQ_F16 || y_dtype == DGQ_BF16),
                  "%s: unknown dtype", who);
    DGQ_CHECK_ARG(w_bits == 4 || w_bits == 8, "%s: w_bits=%d (4 or 8)", who, w_bits);
    DGQ_CHECK_ARG(N > 8, "%s: N=%d (N <= 8 layers stay on dgq_conv2d_f32w)", who, N);
    DGQ_CHECK_ARG(ldy >= ncols, "%s: ldy=%d < N=%d", who, ldy, ncols);
    DGQ_CHECK_ARG(!geglu_rows || N % 2 == 0, "%s: geglu_rows needs an even N", who);
    DGQ_CHECK_ARG(!upsample || (H % 2 == 0 && W % 2 == 0), "%s: upsample needs an even H, W", who);
    const int64_t K = (int64_t)kh * kw * C;
    DGQ_CHECK_ARG(Kp > 0 && Kp % DGQ_KTILE == 0 && Kp >= K, "%s: Kp=%d must be a multiple of %d and >= kh·kw·C = %lld", who,
                  Kp, DGQ_KTILE, (long long)K);
    p.x = x; p.w = w_packed; p.delta = delta; p.zp = zp; p.bias = bias; p.y = y;
    p.y_dtype = y_dtype; p.w_bits = w_bits; p.ups = upsample ? 1 : 0; p.geglu = geglu_rows ? 1 : 0;
    p.B = B; p.H = H; p.W = W; p.C = C; p.kh = kh; p.kw = kw; p.stride = stride; p.pad = pad;
    p.Hs = upsample ? H / 2 : H; p.Ws = upsample ? W / 2 : W;
    p.Ho = (H + 2 * pad - kh) / stride + 1; p.Wo = (W + 2 * pad - kw) / stride + 1;
    DGQ_CHECK_ARG(p.Ho > 0 && p.Wo > 0, "%s: empty output", who);
    const int64_t M = (int64_t)B * p.Ho * p.Wo;
    DGQ_CHECK_ARG(M < (1LL << 31) - 64, "%s: M too large", who);
    p.N = N; p.K = (int)K; p.Kp = Kp; p.M = (int)M; p.ldy = ldy;
    tile = wq16_pick(p.M, N);
    DGQ_CHECK_ARG((N + tile - 1) / tile <= 65535, "%s: N too large", who);
    return DGQ_OK;
}

extern "C" int dgq_conv2d_wq_mfma16(const void* x, int x_dtype, int B, int H, int W, int C, int kh, int kw, int stride, int pad, int upsample,
                                    const uint8_t* w_packed, int w_bits, int Kp, const float* delta, const float* zp, const float* bias,
                                    int N, int geglu_rows, void* y, int y_dtype, int ldy, void* stream) {
    Wq16Params p;
    int tile = 0;
    if (int rc = wq16_setup("dgq_conv2d_wq_mfma16", x, x_dtype, B, H, W, C, kh, kw, stride, pad, upsample, w_packed, w_bits, Kp, delta, zp, bias,
                            N, geglu_rows, y, y_dtype, ldy, N, p, tile)) return rc;
    if (tile == 64) wq16_launch<32, 64>(p, x_dtype, (hipStream_t)stream);
    else wq16_launch<16, 128>(p, x_dtype, (hipStream_t)stream);
    return dgq_launch_status("dgq_conv2d_wq_mfma16");
}

extern "C" int dgq_conv2d_wq_mfma16_fused(const void* x, int x_dtype, int B, int H, int W, int C, int kh, int kw, int stride, int pad, int upsample,
                                          const uint8_t* w_packed, int w_bits, int Kp, const float* delta, const float* zp, const float* bias,
                                          int N, int geglu_rows, void* y, int y_dtype, int ldy, const dgq_wq16_fuse_t* f, void* stream) {
    static const char* who = "dgq_conv2d_wq_mfma16_fused";
    static const dgq_wq16_fuse_t none = {};
    const dgq_wq16_fuse_t& u = f ? *f : none;
    DGQ_CHECK_ARG((u.pre_scale == nullptr) == (u.pre_shift == nullptr), "%s: GroupNorm prologue needs pre_scale and pre_shift", who);
    DGQ_CHECK_ARG(!(u.pre_scale && (u.ln_stats || u.ln_gamma || u.ln_beta)), "%s: GroupNorm and LayerNorm prologue both set", who);
    DGQ_CHECK_ARG(!(u.ln_stats || u.ln_gamma || u.ln_beta) || (u.ln_stats && u.ln_gamma && u.ln_beta),
                  "%s: LayerNorm prologue needs ln_stats, gamma and beta", who);
    DGQ_CHECK_ARG(!u.ln_stats || (kh == 1 && kw == 1 && stride == 1 && pad == 0 && !upsample),
                  "%s: LayerNorm prologue is for Linear inputs (kh = kw = 1, stride 1, no padding)", who);
    DGQ_CHECK_ARG(u.pre_act == 0 || u.pre_act == 1, "%s: pre_act=%d (0 none, 1 SiLU)", who, u.pre_act);
    DGQ_CHECK_ARG(!(u.geglu_out && u.residual), "%s: geglu_out takes no residual", who);
    DGQ_CHECK_ARG(!u.geglu_out || (geglu_rows && N % 2 == 0), "%s: geglu_out needs geglu_rows and an even N", who);
    DGQ_CHECK_ARG(!u.residual || u.ldr >= N, "%s: ldr=%d < N=%d", who, u.ldr, N);
    for (const float* t : {u.pre_scale, u.pre_shift, u.ln_gamma, u.ln_beta})
        DGQ_CHECK_ARG(((uintptr_t)t & 15) == 0, "%s: the prologue's tables must be 16-byte aligned", who);
    DGQ_CHECK_ARG(((uintptr_t)u.ln_stats & 7) == 0, "%s: ln_stats must be 8-byte aligned", who);
    Wq16FusedParams p;
    int tile = 0;
    if (int rc = wq16_setup(who, x, x_dtype, B, H, W, C, kh, kw, stride, pad, upsample, w_packed, w_bits, Kp, delta, zp, bias, N, geglu_rows,
                            y, y_dtype, ldy, u.geglu_out ? N / 2 : N, p, tile)) return rc;
    p.f.pre_scale = u.pre_scale; p.f.pre_shift = u.pre_shift; p.f.ln_stats = u.ln_stats; p.f.ln_gamma = u.ln_gamma; p.f.ln_beta = u.ln_beta;
    p.f.residual = u.residual; p.f.bias_rows = u.bias_rows; p.f.pre_act = u.pre_act; p.f.ldr = u.ldr; p.f.geglu_out = u.geglu_out ? 1 : 0;
    const bool pro = u.pre_scale || u.ln_stats || u.pre_act, epi = u.residual || u.bias_rows || u.geglu_out;
    hipStream_t s = (hipStream_t)stream;
    if (pro) {
        if (tile == 64) wq16_launch_fused<32, 64, 2>(p, x_dtype, s);
        else wq16_launch_fused<16, 128, 2>(p, x_dtype, s);
    } else if (epi) {
        if (tile == 64) wq16_launch_fused<32, 64, 1>(p, x_dtype, s);
        else wq16_launch_fused<16, 128, 1>(p, x_dtype, s);
    } else {                                              // nothing to fold: the kernel of dgq_conv2d_wq_mfma16 itself
        if (tile == 64) wq16_launch<32, 64>(p, x_dtype, s);
        else wq16_launch<16, 128>(p, x_dtype, s);
    }
    return dgq_launch_status(who);
}

// (mean, rstd) of every row of x [rows][C] for the LayerNorm prologue above, one wave per row; one launch serves every consumer of the
// normalised tensor.  The row is read once into registers in the pattern of row_layernorm_stats (quant_prologue.h: lane l holds
// columns 4l + 256i), mean first, then Σ(x − mean)² about the fp32 mean that is written out — but both sums, the division by C, + eps,
// the square root and the reciprocal are carried in fp64 and each result is rounded to fp32 ONCE: mean and rstd are the float64
// statistics to within 2^-24 relative.  row_layernorm_stats itself is fp32 throughout: q/C, + eps, sqrtf and 1/x allow 2.5·2^-24 on rstd
// by themselves and the fp32 sum of up to 2048 squares (32 sequential additions per lane, then a tree) the rest, so it cannot promise
// the 4·2^-24 this entry is held to (tests/test_gpu_weight_only_fused.py); the quantisers' kernels keep it, so these statistics are NOT
// theirs bit for bit.  32 fp64 additions per lane: nothing beside the row's read.
template <typename TIn>
__global__ __launch_bounds__(256) void wq16_ln_row_stats_kernel(const TIn* x, int rows, int C, float eps, float* out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;                              // (wave-uniform)
    const TIn* xr = x + (int64_t)row * C;
    float v[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = lane * 4 + 256 * i;
        if (c < C) load4<TIn>(xr + c, v[i]);
        else v[i][0] = v[i][1] = v[i][2] = v[i][3] = 0.0f;
    }
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += ((double)v[i][0] + (double)v[i][1]) + ((double)v[i][2] + (double)v[i][3]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float mu = (float)(s / (double)C);
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (lane * 4 + 256 * i < C) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double d = (double)v[i][j] - (double)mu;
                q += d * d;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
    const float rstd = (float)(1.0 / sqrt(q / (double)C + (double)eps));
    if (lane == 0) *reinterpret_cast<float2*>(out + 2 * (int64_t)row) = make_float2(mu, rstd);
}

extern "C" int dgq_layernorm_row_stats(const void* x, int x_dtype, int rows, int C, float eps, float* out, void* stream) {
    static const char* who = "dgq_layernorm_row_stats";
    DGQ_CHECK_ARG(x && out, "%s: null pointer", who);
    DGQ_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 7) == 0, "%s: x must be 16-byte and out 8-byte aligned", who);
    DGQ_CHECK_ARG(rows > 0 && rows < (1 << 30), "%s: rows=%d", who, rows);
    DGQ_CHECK_ARG(C > 0 && C % 4 == 0 && C <= DGQ_LN_MAX_C, "%s: C=%d (C %% 4 == 0, C <= %d)", who, C, DGQ_LN_MAX_C);
    DGQ_CHECK_ARG(eps > 0.0f, "%s: eps must be positive", who);
    DGQ_QUANT_DTYPE_SWITCH(x_dtype, who, hipLaunchKernelGGL(wq16_ln_row_stats_kernel<TIn>, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream,
                                                            reinterpret_cast<const TIn*>(x), rows, C, eps, out));
    return dgq_launch_status(who);
}
