// Real-time per-row activation quantiser parameters: one (δ, z) per row the activation quantiser sees, from Scaler.MINMAX applied
// to that row at run time (dgq_amd/quant/quant_layer.py minmax): lo = min(row min, 0), hi = max(row max, 0),
// δ = fp32((double(hi) − double(lo)) / (2^b − 1)) (fp32(1e-8) when smaller), z = rne(fp32(−lo) / δ) with an IEEE division.
// The tables it writes are the mdelta / mzp [L = M] of the per-M routes (dgq_quant_act, dgq_gemm_wxa8 with or without
// quantise-on-load), which read them as mdelta[m % L].  A mode of this library — the reference has no such layer quantiser.
//
// Two kernels, at most two launches per call, no atomics, nothing exchanged between workgroups of a launch:
//   rows   one wave per row of the [rows][ldc] channels-last input (a Linear row, or one PIXEL of a convolution's input): the folded
//          prologue (GroupNorm scale / shift, LayerNorm, SiLU, GEGLU) evaluated by the device functions of the quantise kernels
//          (quant_prologue.h: the quantiser later sees the same x′ bit for bit), min / max over the C channels by an in-wave
//          butterfly.  A Linear layer without a fold is finished here; otherwise the extrema go to the caller's workspace.
//   finish one thread per table entry: the kh x kw window of pixel extrema of an output position (taps outside the image add the 0
//          that MINMAX includes anyway; a folded 2x upsample reads pixel (h/2, w/2)), or — fold_T — the extrema of all rows r with
//          the same r % fold_T (the (1, T, 1) layout of the attention-side quantisers), then δ and z.
// HBM-bound: the input is read once (a convolution's input once per pixel, not once per tap).
#include <algorithm>
#include <cstdint>
#include "dgq_common.h"
#include "quant_prologue.h"

#define DGQ_RP_BATCH 4

struct RowParamsProblem {
    QuantRowInput in;         // the rows of the rows kernel
    float* ext;               // [rows][2] (min(row min, 0), max(row max, 0)), or NULL: the rows kernel writes δ / z itself
    float* delta; float* zp;
    int entries;              // table entries the finish kernel writes: M, or fold_T
    int fold_T;               // > 0: entry t folds the rows t, t + T, ... of `rows`
    int B, Hs, Ws, H, W, kh, kw, stride, pad, Ho, Wo, ups;
};
struct RowParamsBatch {
    RowParamsProblem p[DGQ_RP_BATCH];
};

template <typename TIn>
__global__ __launch_bounds__(256) void rowparams_rows_kernel(RowParamsBatch bt) {
    const RowParamsProblem& p = bt.p[blockIdx.y];
    const QuantRowInput& in = p.in;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= in.rows) return;                             // whole wave leaves; no barriers below
    const QuantRowSource<TIn> s = quant_row_source<TIn>(in, row, lane);
    float mn = 0.0f, mx = 0.0f;                             // MINMAX includes 0 in the range
    // four 16-byte loads per lane in flight; every load goes out unconditionally at a clamped address (C % 4 == 0, C >= 4) and a
    // vector past the end is computed and discarded
    for (int c0 = lane * 4; c0 < in.C; c0 += 1024) {
        float v[4][4], g[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = min(c0 + 256 * u, in.C - 4);
            load4<TIn>(s.xr + c, v[u]);
            if (in.pre_act == 2) load4<TIn>(s.xr + in.C + c, g[u]);
            else g[u][0] = g[u][1] = g[u][2] = g[u][3] = 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = min(c0 + 256 * u, in.C - 4);
            dgq_prologue4(v[u], c, s.pre_sc, s.pre_sh, in.ln_gamma, in.ln_beta, s.ln_mu, s.ln_rstd, in.pre_act, g[u]);
            if (c0 + 256 * u < in.C) {
                mn = fminf(mn, fminf(fminf(v[u][0], v[u][1]), fminf(v[u][2], v[u][3])));
                mx = fmaxf(mx, fmaxf(fmaxf(v[u][0], v[u][1]), fmaxf(v[u][2], v[u][3])));
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    if (lane == 0) {
        if (p.ext) {
            *reinterpret_cast<float2*>(p.ext + 2 * (int64_t)row) = make_float2(mn, mx);
        } else {
            float d, z;
            minmax_params(mn, mx, p.in.levels, d, z);
            p.delta[row] = d;
            p.zp[row] = z;
        }
    }
}

__global__ __launch_bounds__(256) void rowparams_finish_kernel(RowParamsBatch bt) {
    const RowParamsProblem& p = bt.p[blockIdx.y];
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= p.entries) return;
    const float2* ext = reinterpret_cast<const float2*>(p.ext);
    float mn = 0.0f, mx = 0.0f;
    if (p.fold_T > 0) {
        for (int r = m; r < p.in.rows; r += p.fold_T) {
            const float2 e = ext[r];
            mn = fminf(mn, e.x);
            mx = fmaxf(mx, e.y);
        }
    } else {
        const int L = p.Ho * p.Wo;
        const int b = m / L, l = m - b * L;
        const int ho = l / p.Wo, wo = l - ho * p.Wo;
        const int hbase = ho * p.stride - p.pad, wbase = wo * p.stride - p.pad;
        const float2* img = ext + (int64_t)b * p.Hs * p.Ws;
        for (int dh = 0; dh < p.kh; ++dh) {
            const int hi = hbase + dh;
            if (hi < 0 || hi >= p.H) continue;
            for (int dw = 0; dw < p.kw; ++dw) {
                const int wi = wbase + dw;
                if (wi < 0 || wi >= p.W) continue;
                const float2 e = img[(hi >> p.ups) * p.Ws + (wi >> p.ups)];
                mn = fminf(mn, e.x);
                mx = fmaxf(mx, e.y);
            }
        }
    }
    float d, z;
    minmax_params(mn, mx, p.in.levels, d, z);
    p.delta[m] = d;
    p.zp[m] = z;
}

static int fill_row_params(const dgq_quant_act_args_t& a, const dgq_act_rowparams_out_t& o, RowParamsProblem& p) {
    DGQ_CHECK_ARG(o.delta && o.zp, "dgq_act_row_params: null pointer");
    int Ho, Wo;
    const int rc = dgq_check_quant_input(a, "dgq_act_row_params", {4, true, true}, p.in, Ho, Wo);
    if (rc != DGQ_OK) return rc;
    const int ups = a.ups ? 1 : 0, Hs = a.H >> ups, Ws = a.W >> ups;
    const int64_t rows = p.in.rows, M = (int64_t)a.B * Ho * Wo;
    DGQ_CHECK_ARG(M < (1LL << 30), "dgq_act_row_params: too many rows");
    const bool plain = a.kh == 1 && a.kw == 1 && a.stride == 1 && a.pad == 0;       // a row of the table is a row of the input
    DGQ_CHECK_ARG(o.fold_T >= 0 && (o.fold_T == 0 || (plain && M % o.fold_T == 0)), "dgq_act_row_params: fold_T=%d needs a Linear input "
                  "whose row count (%lld) it divides", o.fold_T, (long long)M);
    const bool two = !plain || o.fold_T > 0;
    DGQ_CHECK_ARG(!two || (o.ws && ((uintptr_t)o.ws & 7) == 0 && o.ws_floats >= (size_t)(2 * rows)),
                  "dgq_act_row_params: workspace of %lld floats (8-byte aligned) needed, %zu given", (long long)(2 * rows), o.ws_floats);
    p.ext = two ? o.ws : nullptr;
    p.delta = o.delta; p.zp = o.zp;
    p.entries = o.fold_T > 0 ? o.fold_T : (int)M;
    p.fold_T = o.fold_T;
    p.B = a.B; p.Hs = Hs; p.Ws = Ws; p.H = a.H; p.W = a.W; p.kh = a.kh; p.kw = a.kw; p.stride = a.stride; p.pad = a.pad;
    p.Ho = Ho; p.Wo = Wo; p.ups = ups;
    return DGQ_OK;
}

extern "C" int dgq_act_row_params_batch(int n, const dgq_quant_act_args_t* in, const dgq_act_rowparams_out_t* out, void* stream) {
    DGQ_CHECK_ARG(in && out && n >= 1 && n <= DGQ_RP_BATCH, "dgq_act_row_params_batch: n=%d (1..%d)", n, DGQ_RP_BATCH);
    RowParamsBatch bt;
    int rows = 0, entries = 0;
    bool any_two = false, all_two = true;
    for (int i = 0; i < n; ++i) {
        const int rc = fill_row_params(in[i], out[i], bt.p[i]);
        if (rc != DGQ_OK) return rc;
        DGQ_CHECK_ARG(in[i].x_dtype == in[0].x_dtype, "dgq_act_row_params_batch: problem %d differs from problem 0 in dtype", i);
        rows = std::max(rows, bt.p[i].in.rows);
        const bool two = bt.p[i].ext != nullptr;
        any_two = any_two || two;
        all_two = all_two && two;
        if (two) entries = std::max(entries, bt.p[i].entries);
    }
    DGQ_CHECK_ARG(any_two == all_two, "dgq_act_row_params_batch: the problems of one call are all folded / convolutions, or none is");
    for (int i = n; i < DGQ_RP_BATCH; ++i) bt.p[i] = bt.p[0];
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((rows + 3) / 4, n), block(256);
    DGQ_QUANT_DTYPE_SWITCH(in[0].x_dtype, "dgq_act_row_params", hipLaunchKernelGGL((rowparams_rows_kernel<TIn>), grid, block, 0, st, bt))
    if (any_two) hipLaunchKernelGGL(rowparams_finish_kernel, dim3((entries + 255) / 256, n), dim3(256), 0, st, bt);
    return dgq_launch_status("dgq_act_row_params");
}

extern "C" int dgq_act_row_params(const dgq_quant_act_args_t* in, int fold_T, float* ws, size_t ws_floats, float* delta_out, float* zp_out,
                                  void* stream) {
    DGQ_CHECK_ARG(in, "dgq_act_row_params: null pointer");
    dgq_act_rowparams_out_t o;
    o.fold_T = fold_T; o.ws = ws; o.ws_floats = ws_floats; o.delta = delta_out; o.zp = zp_out;
    return dgq_act_row_params_batch(1, in, &o, stream);
}
