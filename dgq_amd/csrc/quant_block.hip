// Real-time activation quantiser per row and 32-channel block (a mode of this library; the reference has no such layer quantiser): every
// block of DGQ_KCHUNK = 32 consecutive channels of every input row gets its own Scaler.MINMAX pair at run time — the statement is
// dgq_amd/quant/quant_layer.py block_minmax (= row_minmax of the block's extrema) — so an outlier sets the step of its own 32 channels
// only.  In the natural (tap, c) K order a 32-chunk of a convolution's unfolded row is 32 channels of ONE input pixel: the input is
// quantised once per pixel and the unfolded operand never exists (dgq_gemm_blockq gathers the taps).
//
// One launch, one wave per input row (a Linear row or one pixel; rowparams_rows_kernel's mapping), nothing exchanged between waves:
//   - the folded prologue (GroupNorm scale / shift, LayerNorm, SiLU, GEGLU) by the device functions of quant_prologue.h — the same x′
//     bit for bit as the row mode and the calibrated quantisers see;
//   - a lane holds 4 consecutive channels (one 16-byte load of fp32, clamped at the row end), 8 lanes one block: a 3-step in-wave
//     min / max (0 included), then minmax_params;
//   - codes by the exact-division arithmetic of quant_common.h: == clamp(rne(x/δ) + z, 0, 2^b − 1) under a true fp32 division;
//   - written: centred int8 codes s = q − 2^(b−1) [rows][C] in natural order; {δ, β = δ·(2^(b−1) − z)} per block, [rows][ldt] float2
//     (entries C/32 .. ldt − 1, the chunks of a Linear layer's K padding, are written {0, 0}); ρ[row] = Σ_c δ_c·rs_c with
//     rs_c = Σ_{k∈c} s (an exact integer), added in ASCENDING block order c = 0, 1, ... by every lane alike (one fp32 addition per
//     block, starting from 0): deterministic, and the order the CPU statement of the tests uses.
// dgq_dequant_act_block: x̂ = δ·(q − z) from the codes and the table (the stand-alone fake-quant form of the quantizer).
#include <cstdint>
#include "dgq_common.h"
#include "quant_prologue.h"

struct BlockQuantProblem {
    QuantRowInput in;
    float qmax, offset;
    int8_t* codes; float2* table; int ldt; float* rho;
};

template <typename TIn>
__global__ __launch_bounds__(256) void quant_block_kernel(BlockQuantProblem p) {
    const QuantRowInput& in = p.in;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= in.rows) return;                             // whole wave leaves; no barriers below
    const QuantRowSource<TIn> s = quant_row_source<TIn>(in, row, lane);
    int8_t* crow = p.codes + (int64_t)row * in.C;
    float2* trow = p.table + (int64_t)row * p.ldt;
    float rho = 0.0f;
    quant_block_walk<TIn>(in, s, lane, [&](const float (&v)[4], int c, bool inside, int base) {
        float mn = fminf(0.0f, fminf(fminf(v[0], v[1]), fminf(v[2], v[3])));       // MINMAX includes 0 in the range
        float mx = fmaxf(0.0f, fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) {
            mn = fminf(mn, __shfl_xor(mn, o, 64));
            mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        }
        float d, z;
        minmax_params(mn, mx, in.levels, d, z);
        float q[4];
        dgq_affine_code4_fast(v, d, dgq_rcp(d), z, p.qmax, q);
        const float biased[4] = {q[0] - p.offset + 128.0f, q[1] - p.offset + 128.0f, q[2] - p.offset + 128.0f, q[3] - p.offset + 128.0f};
        float fs = 0.0f;
        const uint32_t w = dgq_pack4(biased, fs);
        float rs = fs - 512.0f;                              // Σ s of the lane's four codes, then of the block (exact integers)
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) rs += __shfl_xor(rs, o, 64);
        if (inside) {
            *reinterpret_cast<uint32_t*>(crow + c) = w;
            if ((lane & 7) == 0) trow[c >> 5] = make_float2(d, d * (p.offset - z));
        }
        const float term = d * rs;
#pragma unroll
        for (int j = 0; j < 8; ++j) {                        // ascending block order, the same chain in every lane
            const float t = __shfl(term, 8 * j, 64);
            if (base + 32 * j < in.C) rho += t;
        }
    });
    for (int cb = (in.C >> 5) + lane; cb < p.ldt; cb += 64) trow[cb] = make_float2(0.0f, 0.0f);
    if (lane == 0) p.rho[row] = rho;
}

extern "C" int dgq_quant_act_block(const dgq_quant_act_args_t* in, const dgq_act_block_out_t* out, void* stream) {
    DGQ_CHECK_ARG(in && out, "dgq_quant_act_block: null pointer");
    const dgq_quant_act_args_t& a = *in;
    const dgq_act_block_out_t& o = *out;
    DGQ_CHECK_ARG(o.codes && o.table && o.rho, "dgq_quant_act_block: null pointer");
    DGQ_CHECK_ARG(((uintptr_t)o.codes & 15) == 0 && ((uintptr_t)o.table & 7) == 0,
                  "dgq_quant_act_block: codes must be 16-byte aligned, the table 8-byte aligned");
    BlockQuantProblem p;
    dim3 grid, block(256);
    const int rc = dgq_check_block_quant(a, "dgq_quant_act_block", o.ldt, p.in, grid);
    if (rc != DGQ_OK) return rc;
    p.qmax = p.in.levels; p.offset = (float)(1 << (a.bits - 1));
    p.codes = o.codes; p.table = reinterpret_cast<float2*>(o.table); p.ldt = o.ldt; p.rho = o.rho;
    hipStream_t st = (hipStream_t)stream;
    DGQ_QUANT_DTYPE_SWITCH(a.x_dtype, "dgq_quant_act_block", hipLaunchKernelGGL((quant_block_kernel<TIn>), grid, block, 0, st, p))
    return dgq_launch_status("dgq_quant_act_block");
}

// x̂ = δ·(q − z) of four codes per thread.  The table holds β = fl(δ·(o − z)) with o − z an integer of magnitude <= 2^b: rint(β / δ)
// returns it exactly, and δ·(s + (o − z)) = δ·(q − z) is the reference's one rounding (quant_layer.py:299).
template <typename TOut>
__global__ __launch_bounds__(256) void dequant_block_kernel(const int8_t* codes, const float2* table, int ldt, int64_t rows, int C, TOut* y) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= rows * C) return;
    const int64_t row = i / C;
    const int c = (int)(i - row * C);
    const float2 t = table[row * ldt + (c >> 5)];
    const float oz = rintf(__fdiv_rn(t.y, t.x));
    const uint32_t w = *reinterpret_cast<const uint32_t*>(codes + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) y[i + j] = dgq_from_float<TOut>(t.x * ((float)(int8_t)(w >> (8 * j)) + oz));
}

extern "C" int dgq_dequant_act_block(const int8_t* codes, const float* table, int ldt, int64_t rows, int C, void* y, int y_dtype, void* stream) {
    DGQ_CHECK_ARG(codes && table && y, "dgq_dequant_act_block: null pointer");
    dim3 grid, block(256);
    const int rc = dgq_check_block_dequant("dgq_dequant_act_block", rows, C, ldt, grid);
    if (rc != DGQ_OK) return rc;
    DGQ_CHECK_ARG(((uintptr_t)codes & 3) == 0 && ((uintptr_t)table & 7) == 0, "dgq_dequant_act_block: codes 4-byte, table 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const float2* tb = reinterpret_cast<const float2*>(table);
    DGQ_QUANT_DTYPE_SWITCH(y_dtype, "dgq_dequant_act_block",
                           hipLaunchKernelGGL((dequant_block_kernel<TIn>), grid, block, 0, st, codes, tb, ldt, rows, C, reinterpret_cast<TIn*>(y)))
    return dgq_launch_status("dgq_dequant_act_block");
}
