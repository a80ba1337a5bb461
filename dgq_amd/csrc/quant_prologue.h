// The folded prologues of the quantise-on-load pass (LayerNorm row statistics; GroupNorm scale / shift, LayerNorm, SiLU, GEGLU applied to
// an element vector) shared by quant_act.hip and act_rowparams.hip: the real-time row parameters must be taken from the very x′ the
// quantiser sees, bit for bit.
#pragma once
#include "dgq_common.h"
#include "quant_common.h"

// LayerNorm statistics of one row of C <= 2048 elements (C % 4 == 0), computed by the wave that quantises the row: the
// row is read ONCE into registers (8 float4 per lane), mean first, then Σ(x − mean)² from the registers; biased
// variance, rstd = 1/sqrt(var + eps) as nn.LayerNorm.
#define DGQ_LN_MAX_C 2048
template <typename TIn>
__device__ __forceinline__ void row_layernorm_stats(const TIn* xr, int C, float eps, int lane, float& mu, float& rstd) {
    float v[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = lane * 4 + 256 * i;
        if (c < C) load4<TIn>(xr + c, v[i]);
        else v[i][0] = v[i][1] = v[i][2] = v[i][3] = 0.0f;
    }
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    mu = s / (float)C;
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = lane * 4 + 256 * i;
        if (c < C) {
#pragma unroll
            for (int j = 0; j < 4; ++j) q += (v[i][j] - mu) * (v[i][j] - mu);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
    rstd = 1.0f / sqrtf(q / (float)C + eps);
}

// The folded prologues of the quantise-on-load kernels for four consecutive channels c .. c + 3 of one element vector, in their
// order and rounding (x·scale + shift of a folded GroupNorm; (x − μ)·rstd·γ + β of a folded LayerNorm; SiLU; GEGLU x·gelu(g) with g the
// four gate values): what a kernel that must see the quantiser's own x′ (act_rowparams.hip) evaluates.  pre_sc / pre_sh: this
// image's [C] rows or NULL.
__device__ __forceinline__ void dgq_prologue4(float (&v)[4], int c, const float* pre_sc, const float* pre_sh,
                                              const float* ln_gamma, const float* ln_beta, float ln_mu, float ln_rstd,
                                              int pre_act, const float (&g)[4]) {
    if (pre_sc) {
        const float4 sc = *reinterpret_cast<const float4*>(pre_sc + c);
        const float4 sh = *reinterpret_cast<const float4*>(pre_sh + c);
        v[0] = v[0] * sc.x + sh.x; v[1] = v[1] * sc.y + sh.y; v[2] = v[2] * sc.z + sh.z; v[3] = v[3] * sc.w + sh.w;
    }
    if (ln_gamma) {
        const float4 ga = *reinterpret_cast<const float4*>(ln_gamma + c);
        const float4 be = *reinterpret_cast<const float4*>(ln_beta + c);
        v[0] = (v[0] - ln_mu) * ln_rstd * ga.x + be.x; v[1] = (v[1] - ln_mu) * ln_rstd * ga.y + be.y;
        v[2] = (v[2] - ln_mu) * ln_rstd * ga.z + be.z; v[3] = (v[3] - ln_mu) * ln_rstd * ga.w + be.w;
    }
    if (pre_act == 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = dgq_silu(v[j]);
    } else if (pre_act == 2) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = v[j] * (0.5f * g[j] * (1.0f + erff(g[j] * 0.70710678118654752f)));
    }
}

// MINMAX of one row from its extrema (0 already included): dgq_amd/quant/quant_layer.py row_minmax.  fp64 for the range and its division, one
// rounding to fp32; IEEE fp32 division for z (no reciprocal).
__device__ __forceinline__ void minmax_params(float lo, float hi, float levels, float& delta, float& zp) {
    float d = (float)(((double)hi - (double)lo) / (double)levels);
    if (d < 1e-8f) d = 1e-8f;
    delta = d;
    zp = rintf(__fdiv_rn(-lo, d));
}
