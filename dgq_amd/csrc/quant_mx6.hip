// Real-time MXFP6 activation quantiser (a mode of this library; the reference has no such layer quantiser): every block of DGQ_KCHUNK = 32
// consecutive channels of every input row gets ONE power-of-two scale 2^E (an E8M0 byte) and 32 FP6 E2M3 codes — the statement is
// dgq_amd/quant/quant_layer.py mx6_block: E = floor(log2 amax) − 2 read off the exponent field of amax = max |x′| and clamped to
// [−127, 127] (E = −127 for amax = 0), code = rne(x′·2^−E) on the E2M3 grid, saturating at ±7.5; a zero magnitude is the code +0.  The
// block is the operand of one K block of v_mfma_scale_f32_32x32x64_f8f6f4 (dgq_gemm_mx6); the input is quantised once per row / pixel.
//
// One launch, one wave per input row and the row source / folded prologue of quant_block.hip (quant_prologue.h): the same x′ bit for bit
// as every other mode sees.  A lane holds 4 consecutive channels, 8 lanes one block: a 3-step in-wave max of |x′|, then the codes by exact
// fp32 arithmetic — x′·2^−E is an exponent shift (2^−E is a normal float for every E the rule can give: amax finite means E <= 125), and
// rint(v / step)·step with step a power of two is the round-to-nearest-even of the grid; the hardware conversion is not used, so its
// rounding and saturation are not this statement's concern.  A lane's four codes are 24 bits; three of every four lanes combine theirs
// with the next lane's into one 4-byte store, so a block is the 192-bit little-endian string (element j at bits 6j .. 6j + 5).
//   codes [rows][C/32][24 bytes]; scale [rows][lds] E8M0 bytes, entries C/32 .. lds − 1 written 127 (2^0: the K padding of a Linear layer).
// dgq_dequant_act_mx6: x̂ = code·2^E from such codes and scales (the stand-alone fake-quant form of the quantizer).
#include <cstdint>
#include "dgq_common.h"
#include "quant_prologue.h"

struct Mx6QuantProblem {
    QuantRowInput in;
    uint8_t* codes; uint8_t* scale; int lds;
};

// 2^e for e in [−127, 127] (−127: the subnormal 2^−127)
__device__ __forceinline__ float mx6_pow2(int e) {
    return e >= -126 ? __uint_as_float((uint32_t)(e + 127) << 23) : __uint_as_float(0x00400000u);
}

// E2M3 code of v (|v| < 8, finite): sign | magnitude, round to nearest even on the grid, saturating at 7.5; magnitude 0 -> +0
__device__ __forceinline__ uint32_t mx6_code(float v) {
    const float a = fabsf(v);
    const float inv_step = a < 2.0f ? 8.0f : (a < 4.0f ? 4.0f : 2.0f);
    const float step = a < 2.0f ? 0.125f : (a < 4.0f ? 0.25f : 0.5f);
    const float q = fminf(rintf(a * inv_step) * step, 7.5f);                     // on the grid (a step boundary rounds onto the next range's first value)
    const uint32_t qb = __float_as_uint(q);
    const uint32_t mag = q < 1.0f ? (uint32_t)(q * 8.0f) : ((((qb >> 23) - 126u) << 3) | ((qb >> 20) & 7u));
    return mag ? (mag | ((__float_as_uint(v) >> 26) & 0x20u)) : 0u;
}

template <typename TIn>
__global__ __launch_bounds__(256) void quant_mx6_kernel(Mx6QuantProblem p) {
    const QuantRowInput& in = p.in;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= in.rows) return;                             // whole wave leaves; no barriers below
    const QuantRowSource<TIn> s = quant_row_source<TIn>(in, row, lane);
    uint8_t* crow = p.codes + (int64_t)row * (in.C / 4 * 3);
    uint8_t* srow = p.scale + (int64_t)row * p.lds;
    quant_block_walk<TIn>(in, s, lane, [&](const float (&v)[4], int c, bool inside, int) {
        // max |x′| as an integer (the bits of a non-negative finite float order like the value)
        uint32_t am = max(max(__float_as_uint(v[0]) & 0x7FFFFFFFu, __float_as_uint(v[1]) & 0x7FFFFFFFu),
                          max(__float_as_uint(v[2]) & 0x7FFFFFFFu, __float_as_uint(v[3]) & 0x7FFFFFFFu));
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) am = max(am, (uint32_t)__shfl_xor((int)am, o, 64));
        const int E = max((int)(am >> 23) - 129, -127);    // floor(log2 amax) − 2; subnormal or zero amax: −127
        const float inv = mx6_pow2(-E);
        const uint32_t piece = mx6_code(v[0] * inv) | (mx6_code(v[1] * inv) << 6) | (mx6_code(v[2] * inv) << 12) | (mx6_code(v[3] * inv) << 18);
        const uint32_t next = (uint32_t)__shfl_down((int)piece, 1, 64);
        const int t = lane & 3;                            // lanes 4g .. 4g + 3 hold 96 bits = 3 words; lane t < 3 writes word t
        if (inside) {
            if (t < 3) *reinterpret_cast<uint32_t*>(crow + (c >> 2) * 3 + t) = (piece >> (8 * t)) | (next << (24 - 8 * t));
            if ((lane & 7) == 0) srow[c >> 5] = (uint8_t)(E + 127);
        }
    });
    for (int cb = (in.C >> 5) + lane; cb < p.lds; cb += 64) srow[cb] = 127;
}

extern "C" int dgq_quant_act_mx6(const dgq_quant_act_args_t* in, const dgq_act_mx6_out_t* out, void* stream) {
    DGQ_CHECK_ARG(in && out, "dgq_quant_act_mx6: null pointer");
    const dgq_quant_act_args_t& a = *in;
    const dgq_act_mx6_out_t& o = *out;
    DGQ_CHECK_ARG(o.codes && o.scale, "dgq_quant_act_mx6: null pointer");
    DGQ_CHECK_ARG(((uintptr_t)o.codes & 15) == 0, "dgq_quant_act_mx6: codes must be 16-byte aligned");
    Mx6QuantProblem p;
    dim3 grid, block(256);
    const int rc = dgq_check_block_quant(a, "dgq_quant_act_mx6", o.lds, p.in, grid);
    if (rc != DGQ_OK) return rc;
    p.codes = o.codes; p.scale = o.scale; p.lds = o.lds;
    hipStream_t st = (hipStream_t)stream;
    DGQ_QUANT_DTYPE_SWITCH(a.x_dtype, "dgq_quant_act_mx6", hipLaunchKernelGGL((quant_mx6_kernel<TIn>), grid, block, 0, st, p))
    return dgq_launch_status("dgq_quant_act_mx6");
}

// x̂ of four codes per thread: three bytes hold them; magnitude (1 + m/8)·2^(e−1), or m/8 for e = 0, times 2^E — exact in fp32
// (E >= −127: the smallest product 2^−130 is a subnormal), one rounding into a 16-bit y
template <typename TOut>
__global__ __launch_bounds__(256) void dequant_mx6_kernel(const uint8_t* codes, const uint8_t* scale, int lds, int64_t rows, int C, TOut* y) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= rows * C) return;
    const int64_t row = i / C;
    const int c = (int)(i - row * C);
    const float sc = mx6_pow2((int)scale[row * lds + (c >> 5)] - 127);
    const uint8_t* b = codes + i / 4 * 3;
    const uint32_t w = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t code = (w >> (6 * j)) & 63u;
        const uint32_t e = (code >> 3) & 3u, m = code & 7u;
        const float mag = e ? (float)(8u + m) * 0.125f * (float)(1u << (e - 1u)) : (float)m * 0.125f;
        y[i + j] = dgq_from_float<TOut>((code & 32u ? -mag : mag) * sc);
    }
}

extern "C" int dgq_dequant_act_mx6(const uint8_t* codes, const uint8_t* scale, int lds, int64_t rows, int C, void* y, int y_dtype, void* stream) {
    DGQ_CHECK_ARG(codes && scale && y, "dgq_dequant_act_mx6: null pointer");
    dim3 grid, block(256);
    const int rc = dgq_check_block_dequant("dgq_dequant_act_mx6", rows, C, lds, grid);
    if (rc != DGQ_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    DGQ_QUANT_DTYPE_SWITCH(y_dtype, "dgq_dequant_act_mx6",
                           hipLaunchKernelGGL((dequant_mx6_kernel<TIn>), grid, block, 0, st, codes, scale, lds, rows, C, reinterpret_cast<TIn*>(y)))
    return dgq_launch_status("dgq_dequant_act_mx6");
}
