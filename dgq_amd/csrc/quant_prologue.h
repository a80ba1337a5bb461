// What the activation quantisers share: the input description of a dgq_quant_act_args_t and its ONE host-side check (the three entries
// dgq_quant_act_batch, dgq_act_row_params_batch, dgq_quant_act_block), the dtype switch of their launchers, a wave's row of a [rows][ldc]
// input (the row source of act_rowparams.hip and quant_block.hip), the LayerNorm row statistics and the folded prologue (GroupNorm
// scale / shift, LayerNorm, SiLU, GEGLU) of four channels: the real-time row and block parameters must be taken from the very x′ the
// quantiser sees, bit for bit.  The kernels of quant_act.hip take row_layernorm_stats from here and spell the prologue inline: with the
// prologue, row set-up and code step shared the step measured slower (profiles/r13_quant_shared_resources.txt).
// gemm_panel.hip and gemm_convq.hip spell it between their hand-issued loads and counted waits.
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

// The folded prologues for four consecutive channels c .. c + 3 of one element vector, in their order and rounding (x·scale + shift of
// a folded GroupNorm; (x − μ)·rstd·γ + β of a folded LayerNorm; SiLU; GEGLU x·gelu(g) with g the four gate values — the caller loads
// them when pre_act == 2 and passes zeros otherwise): what a kernel that must see the quantiser's own x′ evaluates.  pre_sc / pre_sh: this
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
        for (int j = 0; j < 4; ++j) v[j] = dgq_geglu(v[j], g[j]);
    }
}
// The input of the real-time kernels (act_rowparams.hip, quant_block.hip): [rows][ldc] channels-last rows — a Linear row, or one
// source pixel of a convolution's input — with the folded prologue to apply.  Filled by dgq_check_quant_input.
struct QuantRowInput {
    const void* x;
    int rows;                 // B·Hs·Ws source pixels (Linear: M)
    int rows_per_image;       // Hs·Ws (pre_scale / pre_shift are [B][C])
    int C, ldc;               // ldc: elements per row (C, or 2C for GEGLU)
    const float* pre_scale; const float* pre_shift; int pre_act;
    const float* ln_gamma; const float* ln_beta; float ln_eps;
    float levels;             // 2^b − 1
};
// What the wave that owns `row` needs of it: the row, this image's GroupNorm rows (or NULL) and the row's LayerNorm statistics
template <typename TIn>
struct QuantRowSource { const TIn* xr; const float* pre_sc; const float* pre_sh; float ln_mu, ln_rstd; };
template <typename TIn>
__device__ __forceinline__ QuantRowSource<TIn> quant_row_source(const QuantRowInput& in, int row, int lane) {
    QuantRowSource<TIn> s;
    s.xr = reinterpret_cast<const TIn*>(in.x) + (int64_t)row * in.ldc;
    const int b = row / in.rows_per_image;
    s.pre_sc = in.pre_scale ? in.pre_scale + (int64_t)b * in.C : nullptr;
    s.pre_sh = in.pre_shift ? in.pre_shift + (int64_t)b * in.C : nullptr;
    s.ln_mu = 0.0f; s.ln_rstd = 1.0f;
    if (in.ln_gamma) row_layernorm_stats<TIn>(s.xr, in.C, in.ln_eps, lane, s.ln_mu, s.ln_rstd);
    return s;
}

// The one host-side check of the input description of a dgq_quant_act_args_t (x, geometry, bits, folded prologue, ups) for the three
// entries that take one; `who` names the entry in the message.  Where the entries genuinely differ the rule is a parameter:
//   c_multiple  C must be a multiple of it (1: dgq_quant_act, whose natural order asks for 4 itself; 4: row parameters; 32: blocks)
//   window      the kh x kw / stride / pad window is read (quantiser, row parameters): it is checked, the output must not be empty and
//               ups needs a convolution.  The block quantiser works per input pixel and reads kh, kw only to tell a Linear input.
//   row_source  x is read through quant_row_source (16-byte aligned, < 2^30 rows); otherwise through the ksrc tables, whose entries
//               hold the channel in 16 bits.
// Fills `in` (rows = the source pixels) and the output size Ho x Wo (window only).
struct QuantInputRules { int c_multiple; bool window, row_source; };
static inline int dgq_check_quant_input(const dgq_quant_act_args_t& a, const char* who, const QuantInputRules& r, QuantRowInput& in,
                                        int& Ho, int& Wo) {
    DGQ_CHECK_ARG(a.x, "%s: null pointer", who);
    DGQ_CHECK_ARG(!r.row_source || ((uintptr_t)a.x & 15) == 0, "%s: x must be 16-byte aligned", who);
    DGQ_CHECK_ARG(a.B > 0 && a.H > 0 && a.W > 0 && a.C > 0, "%s: bad geometry", who);
    DGQ_CHECK_ARG(!r.window || (a.kh > 0 && a.kw > 0 && a.stride > 0 && a.pad >= 0), "%s: bad geometry", who);
    DGQ_CHECK_ARG(!r.window || (a.kh <= 0x7F && a.kw <= 0xFF), "%s: kernel size out of range", who);
    DGQ_CHECK_ARG(r.row_source || a.C <= 0xFFFF, "%s: channel count out of range", who);
    DGQ_CHECK_ARG(a.C % r.c_multiple == 0, "%s: C=%d must be a multiple of %d", who, a.C, r.c_multiple);
    DGQ_CHECK_ARG(a.bits >= 2 && a.bits <= 8, "%s: bits=%d", who, a.bits);
    DGQ_CHECK_ARG((a.pre_scale == nullptr) == (a.pre_shift == nullptr) && a.pre_act >= 0 && a.pre_act <= 2, "%s: bad prologue", who);
    const bool one = a.kh == 1 && a.kw == 1;
    DGQ_CHECK_ARG(a.pre_act != 2 || (one && !a.pre_scale), "%s: GEGLU prologue is for Linear inputs", who);
    DGQ_CHECK_ARG((a.ln_gamma == nullptr) == (a.ln_beta == nullptr), "%s: LayerNorm prologue needs gamma and beta", who);
    DGQ_CHECK_ARG(!a.ln_gamma || (one && !a.pre_scale && a.pre_act == 0 && a.C % 4 == 0 && a.C <= DGQ_LN_MAX_C && a.ln_eps > 0.0f),
                  "%s: LayerNorm prologue is for Linear inputs (1x1, C %% 4 == 0, C <= %d, no other prologue)", who, DGQ_LN_MAX_C);
    const int ups = a.ups ? 1 : 0;
    DGQ_CHECK_ARG(!ups || (a.H % 2 == 0 && a.W % 2 == 0 && (!r.window || a.kh * a.kw > 1)), "%s: ups needs even H, W%s", who,
                  r.window ? " and a convolution" : "");
    Ho = Wo = 0;
    if (r.window) {
        Ho = (a.H + 2 * a.pad - a.kh) / a.stride + 1;
        Wo = (a.W + 2 * a.pad - a.kw) / a.stride + 1;
        DGQ_CHECK_ARG(Ho > 0 && Wo > 0, "%s: empty output", who);
    }
    const int Hs = a.H >> ups, Ws = a.W >> ups;
    const int64_t rows = (int64_t)a.B * Hs * Ws;
    DGQ_CHECK_ARG(!r.row_source || rows < (1LL << 30), "%s: too many rows", who);
    in.x = a.x; in.rows = (int)rows; in.rows_per_image = Hs * Ws; in.C = a.C; in.ldc = a.pre_act == 2 ? 2 * a.C : a.C;
    in.pre_scale = a.pre_scale; in.pre_shift = a.pre_shift; in.pre_act = a.pre_act;
    in.ln_gamma = a.ln_gamma; in.ln_beta = a.ln_beta; in.ln_eps = a.ln_eps;
    in.levels = (float)((1 << a.bits) - 1);
    return DGQ_OK;
}

// The three input dtypes of this family: `...` (a launch) runs with TIn bound to the element type; an unknown code is DGQ_EINVAL.
#define DGQ_QUANT_DTYPE_SWITCH(dtype, who, ...)                                           \
    switch (dtype) {                                                                      \
        case DGQ_F32: { using TIn = float; __VA_ARGS__; } break;                          \
        case DGQ_F16: { using TIn = __half; __VA_ARGS__; } break;                         \
        case DGQ_BF16: { using TIn = __hip_bfloat16; __VA_ARGS__; } break;                \
        default: dgq_set_error("%s: unknown dtype %d", who, dtype); return DGQ_EINVAL;    \
    }

// ---- the real-time BLOCK quantisers (quant_block.hip, quant_mx6.hip): one wave per input row, four rows per 256-thread block; a lane
// holds 4 consecutive channels, 8 lanes one 32-channel block.
// The row walk: wave-uniform steps of 256 channels = 8 blocks; C % 32 == 0, so the 8 lanes of a block are all inside the row or all
// past it (a block past the end computes on a clamped address and must store nothing).  Per step body(v, c, inside, base) gets the
// lane's four x′ behind the folded prologue, their first channel c (clamped), whether the lane's block is inside, and the step's base.
template <typename TIn, typename Body>
__device__ __forceinline__ void quant_block_walk(const QuantRowInput& in, const QuantRowSource<TIn>& s, int lane, Body&& body) {
    for (int base = 0; base < in.C; base += 256) {
        const int c0 = base + lane * 4;
        const bool inside = c0 < in.C;
        const int c = min(c0, in.C - 4);
        float v[4], g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        load4<TIn>(s.xr + c, v);
        if (in.pre_act == 2) load4<TIn>(s.xr + in.C + c, g);
        dgq_prologue4(v, c, s.pre_sc, s.pre_sh, in.ln_gamma, in.ln_beta, s.ln_mu, s.ln_rstd, in.pre_act, g);
        body(v, c, inside, base);
    }
}
// host side of the two entries: the input check, the pitch of the per-block output (>= C/32 entries per row) and the grid
static inline int dgq_check_block_quant(const dgq_quant_act_args_t& a, const char* who, int pitch, QuantRowInput& in, dim3& grid) {
    int Ho, Wo;
    const int rc = dgq_check_quant_input(a, who, {DGQ_KCHUNK, false, true}, in, Ho, Wo);
    if (rc != DGQ_OK) return rc;
    DGQ_CHECK_ARG(pitch >= a.C / DGQ_KCHUNK, "%s: block pitch %d < %d blocks", who, pitch, a.C / DGQ_KCHUNK);
    DGQ_CHECK_ARG((int64_t)in.rows * a.C < (1LL << 40), "%s: too many rows", who);
    grid = dim3((in.rows + 3) / 4);
    return DGQ_OK;
}
// ... and of the two dequant entries (four codes per thread): the shape check and the grid
static inline int dgq_check_block_dequant(const char* who, int64_t rows, int C, int pitch, dim3& grid) {
    DGQ_CHECK_ARG(rows > 0 && C > 0 && C % DGQ_KCHUNK == 0 && pitch >= C / DGQ_KCHUNK && rows * C < (1LL << 40),
                  "%s: bad shape rows=%lld C=%d pitch=%d", who, (long long)rows, C, pitch);
    grid = dim3((unsigned)((rows * C / 4 + 255) / 256));
    return DGQ_OK;
}

// MINMAX of one row from its extrema (0 already included): dgq_amd/quant/quant_layer.py row_minmax.  fp64 for the range and its division, one
// rounding to fp32; IEEE fp32 division for z (no reciprocal).
__device__ __forceinline__ void minmax_params(float lo, float hi, float levels, float& delta, float& zp) {
    float d = (float)(((double)hi - (double)lo) / (double)levels);
    if (d < 1e-8f) d = 1e-8f;
    delta = d;
    zp = rintf(__fdiv_rn(-lo, d));
}
