// Real-time MXFP4 activation quantiser (a mode of this library; the reference has no such layer quantiser): every block of DGQ_KCHUNK = 32
// consecutive channels of every input row gets ONE power-of-two scale 2^E (an E8M0 byte) and 32 FP4 E2M1 codes — the statement is
// dgq_amd/quant/quant_layer.py mx4_block: E = floor(log2 amax) − 2 read off the exponent field of amax = max |x′| and clamped to
// [−127, 127] (E = −127 for a zero or subnormal amax), code = rne(x′·2^−E) on the E2M1 grid {0, 0.5, 1, 1.5, 2, 3, 4, 6}, ties to the
// even code, saturating at ±6; a zero magnitude is the code +0.  The block is the A operand of one K block of
// v_mfma_scale_f32_32x32x64_f8f6f4 (dgq_gemm_mx4); the input is quantised once per row / pixel.
//
// One launch, one wave per input row and the row source / folded prologue of quant_block.hip (quant_prologue.h): the same x′ bit for bit
// as every other mode sees.  A lane holds 4 consecutive channels, 8 lanes one block: a 3-step in-wave max of |x′|, then the codes by exact
// fp32 arithmetic — x′·2^−E is an exponent shift, and rint(v / step)·step with step a power of two (0.5 below 2, 1 below 4, 2 above) is
// the round-to-nearest-even of the grid: in every range the even multiples of the step are the even codes.  The packed conversion
// instruction of gfx950 is not used, so its rounding and saturation are not this statement's concern.  A lane's four codes are 16 bits;
// the block's eight lanes meet in its first lane by four in-wave shifts, and a block leaves as ONE 16-byte store: the 128-bit
// little-endian string (element j at bits 4j .. 4j + 3) the FP4 operand reads from a lane's first four registers.
//   codes [rows][C/32][16 bytes]; scale [rows][lds] E8M0 bytes, entries C/32 .. lds − 1 written 127 (2^0: the K padding of a Linear layer).
// dgq_dequant_act_mx4: x̂ = code·2^E from such codes and scales (the stand-alone fake-quant form of the quantizer).
#include <cstdint>
#include "dgq_common.h"
#include "quant_prologue.h"

struct Mx4QuantProblem {
    QuantRowInput in;
    uint8_t* codes; uint8_t* scale; int lds;
};

// (mx4_pow2, mx4_code and the block statement mx4_block_codes: quant_common.h — shared with linear_smallm_mx.hip)

template <typename TIn>
__global__ __launch_bounds__(256) void quant_mx4_kernel(Mx4QuantProblem p) {
    const QuantRowInput& in = p.in;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= in.rows) return;                             // whole wave leaves; no barriers below
    const QuantRowSource<TIn> s = quant_row_source<TIn>(in, row, lane);
    uint8_t* crow = p.codes + (int64_t)row * (in.C / 2);
    uint8_t* srow = p.scale + (int64_t)row * p.lds;
    quant_block_walk<TIn>(in, s, lane, [&](const float (&v)[4], int c, bool inside, int) {
        int E;
        const uint4 blk = mx4_block_codes(v, E);           // the block's 128 bits in its first lane
        if (inside && (lane & 7) == 0) {
            *reinterpret_cast<uint4*>(crow + (c >> 5) * 16) = blk;
            srow[c >> 5] = (uint8_t)(E + 127);
        }
    });
    for (int cb = (in.C >> 5) + lane; cb < p.lds; cb += 64) srow[cb] = 127;
}

extern "C" int dgq_quant_act_mx4(const dgq_quant_act_args_t* in, const dgq_act_mx4_out_t* out, void* stream) {
    DGQ_CHECK_ARG(in && out, "dgq_quant_act_mx4: null pointer");
    const dgq_quant_act_args_t& a = *in;
    const dgq_act_mx4_out_t& o = *out;
    DGQ_CHECK_ARG(o.codes && o.scale, "dgq_quant_act_mx4: null pointer");
    DGQ_CHECK_ARG(((uintptr_t)o.codes & 15) == 0, "dgq_quant_act_mx4: codes must be 16-byte aligned");
    Mx4QuantProblem p;
    dim3 grid, block(256);
    const int rc = dgq_check_block_quant(a, "dgq_quant_act_mx4", o.lds, p.in, grid);
    if (rc != DGQ_OK) return rc;
    p.codes = o.codes; p.scale = o.scale; p.lds = o.lds;
    hipStream_t st = (hipStream_t)stream;
    DGQ_QUANT_DTYPE_SWITCH(a.x_dtype, "dgq_quant_act_mx4", hipLaunchKernelGGL((quant_mx4_kernel<TIn>), grid, block, 0, st, p))
    return dgq_launch_status("dgq_quant_act_mx4");
}

// x̂ of four codes per thread: two bytes hold them; magnitude (1 + m/2)·2^(e−1), or m/2 for e = 0, times 2^E — exact in fp32
// (E >= −127: the smallest product 2^−128 is a subnormal), one rounding into a 16-bit y
template <typename TOut>
__global__ __launch_bounds__(256) void dequant_mx4_kernel(const uint8_t* codes, const uint8_t* scale, int lds, int64_t rows, int C, TOut* y) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= rows * C) return;
    const int64_t row = i / C;
    const int c = (int)(i - row * C);
    const float sc = mx4_pow2((int)scale[row * lds + (c >> 5)] - 127);
    const uint32_t w = *reinterpret_cast<const uint16_t*>(codes + i / 2);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t code = (w >> (4 * j)) & 15u;
        const uint32_t e = (code >> 1) & 3u, m = code & 1u;
        const float mag = e ? (float)(2u + m) * 0.5f * (float)(1u << (e - 1u)) : (float)m * 0.5f;
        y[i + j] = dgq_from_float<TOut>((code & 8u ? -mag : mag) * sc);
    }
}

extern "C" int dgq_dequant_act_mx4(const uint8_t* codes, const uint8_t* scale, int lds, int64_t rows, int C, void* y, int y_dtype, void* stream) {
    DGQ_CHECK_ARG(codes && scale && y, "dgq_dequant_act_mx4: null pointer");
    DGQ_CHECK_ARG(((uintptr_t)codes & 1) == 0, "dgq_dequant_act_mx4: codes must be 2-byte aligned");
    dim3 grid, block(256);
    const int rc = dgq_check_block_dequant("dgq_dequant_act_mx4", rows, C, lds, grid);
    if (rc != DGQ_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    DGQ_QUANT_DTYPE_SWITCH(y_dtype, "dgq_dequant_act_mx4",
                           hipLaunchKernelGGL((dequant_mx4_kernel<TIn>), grid, block, 0, st, codes, scale, lds, rows, C, reinterpret_cast<TIn*>(y)))
    return dgq_launch_status("dgq_dequant_act_mx4");
}
