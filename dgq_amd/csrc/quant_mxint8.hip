// Real-time MXINT8 activation quantiser (a mode of this library; the reference has no such layer quantiser): every block of DGQ_KCHUNK = 32
// consecutive channels of every input row gets ONE power-of-two scale 2^E (an E8M0 byte) and 32 two's-complement codes s of value
// s·2^(E−6) — the OCP MXINT8 block.  The statement is dgq_amd/quant/quant_layer.py mxint8_block: E = floor(log2 amax), read off the
// exponent field of amax = max |x′| and clamped to [−120, 127] (−120 for a zero or subnormal amax), s = clamp(rne(x′·2^(6−E)), −127, 127).
//
// gfx950 has no MXINT8 operand type, but a code splits exactly into two FP6 E2M3 terms: s = 16·h + l with h = s >> 4 in [−8, 7] and
// l = s & 15 in [0, 15], and both h/2 and l/2 are E2M3 grid values.  The split and the 6-bit packing are done HERE, once per element
// (in the GEMM every column block would repeat them): a block is 48 bytes — the hi plane's 192-bit little-endian string (element j at
// bits 6j .. 6j + 5; sign-magnitude h/2, h = 0 stored +0), then the lo plane's (l/2) — two FP6 operand images of
// v_mfma_scale_f32_32x32x64_f8f6f4 (dgq_gemm_mxint8), 16-byte aligned: three 16-byte loads.
//
// One launch, one wave per input row and the row source / folded prologue of quant_block.hip (quant_prologue.h): the same x′ bit for bit
// as every other mode sees.  A lane holds 4 consecutive channels, 8 lanes one block: a 3-step in-wave max of the |x′| bits, then
// x′·2^(6−E) — an exact exponent shift: both 2^(6−E) and 2^(E−6) are normal floats for every E in the clamp — and rintf.  A lane's four
// codes are 24 bits per plane; three of every four lanes combine theirs with the next lane's into one 4-byte store per plane.
//   codes [rows][C/32][48 bytes]; scale [rows][lds] E8M0 bytes, entries C/32 .. lds − 1 written 127 (2^0: the K padding of a Linear layer).
// dgq_dequant_act_mxint8: x̂ = (16h + l)·2^(E−6) from such codes and scales (the stand-alone fake-quant form of the quantizer).
#include <cstdint>
#include "dgq_common.h"
#include "quant_prologue.h"

struct MxInt8QuantProblem {
    QuantRowInput in;
    uint8_t* codes; uint8_t* scale; int lds;
};

// (mxint8_pow2, mxint8_split and the block statement mxint8_block_codes: quant_common.h — shared with linear_smallm_mx.hip)

template <typename TIn>
__global__ __launch_bounds__(256) void quant_mxint8_kernel(MxInt8QuantProblem p) {
    const QuantRowInput& in = p.in;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= in.rows) return;                             // whole wave leaves; no barriers below
    const QuantRowSource<TIn> s = quant_row_source<TIn>(in, row, lane);
    uint8_t* crow = p.codes + (int64_t)row * (in.C / 32 * 48);
    uint8_t* srow = p.scale + (int64_t)row * p.lds;
    quant_block_walk<TIn>(in, s, lane, [&](const float (&v)[4], int c, bool inside, int) {
        int E;
        uint32_t hi, lo;
        mxint8_block_codes(v, E, hi, lo);
        const uint32_t hi_next = (uint32_t)__shfl_down((int)hi, 1, 64);
        const uint32_t lo_next = (uint32_t)__shfl_down((int)lo, 1, 64);
        const int t = lane & 3;                            // lanes 4g .. 4g + 3 hold 96 bits = 3 words per plane; lane t < 3 writes word t
        if (inside) {
            if (t < 3) {
                uint8_t* blk = crow + (c >> 5) * 48 + ((c >> 2) & 7) * 3 + t;      // (12·(lane group of the block) + 4t: 4-byte aligned)
                *reinterpret_cast<uint32_t*>(blk) = mx6_lane_word(hi, hi_next, t);
                *reinterpret_cast<uint32_t*>(blk + 24) = mx6_lane_word(lo, lo_next, t);
            }
            if ((lane & 7) == 0) srow[c >> 5] = (uint8_t)(E + 127);
        }
    });
    for (int cb = (in.C >> 5) + lane; cb < p.lds; cb += 64) srow[cb] = 127;
}

extern "C" int dgq_quant_act_mxint8(const dgq_quant_act_args_t* in, const dgq_act_mxint8_out_t* out, void* stream) {
    DGQ_CHECK_ARG(in && out, "dgq_quant_act_mxint8: null pointer");
    const dgq_quant_act_args_t& a = *in;
    const dgq_act_mxint8_out_t& o = *out;
    DGQ_CHECK_ARG(o.codes && o.scale, "dgq_quant_act_mxint8: null pointer");
    DGQ_CHECK_ARG(((uintptr_t)o.codes & 15) == 0, "dgq_quant_act_mxint8: codes must be 16-byte aligned");
    MxInt8QuantProblem p;
    dim3 grid, block(256);
    const int rc = dgq_check_block_quant(a, "dgq_quant_act_mxint8", o.lds, p.in, grid);
    if (rc != DGQ_OK) return rc;
    p.codes = o.codes; p.scale = o.scale; p.lds = o.lds;
    hipStream_t st = (hipStream_t)stream;
    DGQ_QUANT_DTYPE_SWITCH(a.x_dtype, "dgq_quant_act_mxint8", hipLaunchKernelGGL((quant_mxint8_kernel<TIn>), grid, block, 0, st, p))
    return dgq_launch_status("dgq_quant_act_mxint8");
}

// twice the magnitude of an E2M3 code that holds a multiple of one half: an integer in [0, 15]
__device__ __forceinline__ int mxint8_twice(uint32_t code) {
    const uint32_t e = (code >> 3) & 3u, m = code & 7u;
    return (int)(e ? ((8u + m) << (e - 1u)) >> 2 : m >> 2);
}

// x̂ of four codes per thread: three bytes of each plane hold them; s = 16h + l, x̂ = s·2^(E−6) — exact in fp32 (|s| <= 127 and E − 6 >=
// −126: a normal product), one rounding into a 16-bit y
template <typename TOut>
__global__ __launch_bounds__(256) void dequant_mxint8_kernel(const uint8_t* codes, const uint8_t* scale, int lds, int64_t rows, int C, TOut* y) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= rows * C) return;
    const int64_t row = i / C;
    const int c = (int)(i - row * C);
    const int E = max((int)scale[row * lds + (c >> 5)] - 127, -120);
    const float sc = mxint8_pow2(E - 6);
    const uint8_t* b = codes + (row * (C >> 5) + (c >> 5)) * 48 + ((c >> 2) & 7) * 3;
    const uint32_t wh = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16);
    const uint32_t wl = (uint32_t)b[24] | ((uint32_t)b[25] << 8) | ((uint32_t)b[26] << 16);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t ch = (wh >> (6 * j)) & 63u, cl = (wl >> (6 * j)) & 63u;
        const int h = mxint8_twice(ch);
        const int sj = 16 * (ch & 32u ? -h : h) + mxint8_twice(cl);
        y[i + j] = dgq_from_float<TOut>((float)sj * sc);
    }
}

extern "C" int dgq_dequant_act_mxint8(const uint8_t* codes, const uint8_t* scale, int lds, int64_t rows, int C, void* y, int y_dtype, void* stream) {
    DGQ_CHECK_ARG(codes && scale && y, "dgq_dequant_act_mxint8: null pointer");
    dim3 grid, block(256);
    const int rc = dgq_check_block_dequant("dgq_dequant_act_mxint8", rows, C, lds, grid);
    if (rc != DGQ_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    DGQ_QUANT_DTYPE_SWITCH(y_dtype, "dgq_dequant_act_mxint8",
                           hipLaunchKernelGGL((dequant_mxint8_kernel<TIn>), grid, block, 0, st, codes, scale, lds, rows, C, reinterpret_cast<TIn*>(y)))
    return dgq_launch_status("dgq_dequant_act_mxint8");
}
