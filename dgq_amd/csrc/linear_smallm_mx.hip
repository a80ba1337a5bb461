// linear_smallm_mx.hip — the batch-row Linear layers under the real-time MX activation modes in ONE launch: y_l = b_l + δw_l·Σ x̂·(q − z)_l
// for up to 24 W4 layers that share one input x [M <= 16][K] — the time_emb_proj(SiLU(temb)) projections of a UNet forward, which the
// general MX route runs as one quantiser launch over two rows + one GEMM launch whose 32-row MFMA tile holds 30 dead rows, per layer.
// The work is weight streaming; this kernel is built around that:
//
//  * One workgroup (256 threads, 4 waves) owns a slab of 64 output columns of ONE problem; the grid is the concatenation of all
//    problems' slabs (block0 per problem, as linear_smallm.hip).
//  * At entry the workgroup quantises x into LDS, once, with the block statements of the stand-alone quantisers (quant_common.h:
//    mx6_block_codes / mxint8_block_codes / mx4_block_codes behind the same fp32 SiLU) — a lane holds 4 channels, 8 lanes a block,
//    a wave a row at a time.  The image is [K block][16 rows][AB bytes] (AB = 24 MXFP6, 48 MXINT8 = hi plane | lo plane, 16 MXFP4)
//    and one E8M0 byte per (block, row): at most 49 KiB.  Rows M .. 15 and the blocks K/32 .. Kp/32 − 1 are zero codes under the
//    byte 127 and contribute exactly 0.
//  * The K step is v_mfma_scale_f32_16x16x128_f8f6f4: 16 activation rows against 16 weight columns, four 32-blocks per issue.  Lane
//    l holds row / column l & 15 and the K block l >> 4 of the step — 32 consecutive k as the little-endian string of their codes in
//    the first six (FP6) or four (FP4) registers — and the activation scale of its own (row, block) in byte 0 of the scale register;
//    the accumulator register i of lane l is y[4·(l >> 4) + i][l & 15].  The weight side is the constant byte of the MX GEMMs (128;
//    MXINT8: lo plane under 123, then hi plane under 127, into the one accumulator; MXFP4: cbsz = 4 against blgp = 2).
//  * A wave owns 16 columns and walks the WHOLE K in ascending order.  Its weight fragments go global -> registers directly from the
//    layer's existing image [N][Kp/32][24] (dgq_pack_w_mx6): a lane's 24 bytes ARE its B operand, no LDS, every weight byte read
//    once device-wide, a ring of 4 steps in flight (the load of step s + 4 is issued before the MFMA of step s).  The A fragments
//    come from LDS.  No K split, no cross-wave reduction: the fp32 summation order is fixed by (K, format) alone.
//  * Epilogue: the MX GEMMs' plain store (dgq_dequant<false> with R = 0, zw = 0: fma(alpha, acc, gamma)), one rounding into y's
//    dtype, rows < M and columns < N only.  A ragged last slab clamps its loads to column N − 1; a wave wholly past N leaves.
#include <cstdint>
#include "dgq_common.h"
#include "gemm_device.h"
#include "quant_common.h"

// the limits of linear_smallm.hip
constexpr int SMX_MAX_PROBLEMS = 24, SMX_MAX_M = 16, SMX_MAX_K = 2048;

typedef int v8i __attribute__((ext_vector_type(8)));

namespace {

struct SmallMMxProblem {
    const uint8_t* w;          // [N][Kp/32][24] E2M3 codes of (q − z)/2
    const float* alpha;        // δw [N]
    const float* gamma;        // bias [N]
    void* y;                   // [M][ldy]
    int ldy, N, Kp, block0;
};

struct SmallMMxBatch {
    SmallMMxProblem p[SMX_MAX_PROBLEMS];
    int n;
    const void* x;             // [M][ldx] shared input
    int M, K, Kq, ldx, pre_act;  // Kq: the largest Kp of the batch = the K extent of the LDS image
};

constexpr int smx_code_bytes(int fmt) { return fmt == 8 ? 48 : (fmt == 6 ? 24 : 16); }

template <typename T, int FMT>
__global__ __launch_bounds__(256) void linear_smallm_mx_kernel(SmallMMxBatch b) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr int AB = smx_code_bytes(FMT);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nbq = b.Kq >> 5;
    uint8_t* a_lds = smem;                                  // [block][16][AB]
    uint8_t* sc_lds = smem + nbq * 16 * AB;                 // [block][16]

    // ---- x -> codes and scale bytes, the stand-alone quantisers' statement: wave = one row at a time, lane = 4 channels of a step of 256
    const T* x = reinterpret_cast<const T*>(b.x);
    for (int row = wid; row < 16; row += 4) {
        for (int base = 0; base < b.Kq; base += 256) {
            const int c = base + lane * 4;
            const bool live = row < b.M && c < b.K;         // K % 32 == 0: the 8 lanes of a block agree
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (live) {
                load4<T>(x + (int64_t)row * b.ldx + c, v);
                if (b.pre_act == 1) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = dgq_silu(v[j]);
                }
            }
            const bool in = c < b.Kq;
            uint8_t* blk = a_lds + ((c >> 5) * 16 + row) * AB;
            int E;
            if constexpr (FMT == 6) {
                const int t = lane & 3;
                const uint32_t piece = mx6_block_codes(v, E);
                const uint32_t word = mx6_lane_word(piece, (uint32_t)__shfl_down((int)piece, 1, 64), t);
                if (in && t < 3) *reinterpret_cast<uint32_t*>(blk + ((c >> 2) & 7) * 3 + t) = word;
            } else if constexpr (FMT == 8) {
                uint32_t hi, lo;
                mxint8_block_codes(v, E, hi, lo);
                const int t = lane & 3;
                const uint32_t hi_word = mx6_lane_word(hi, (uint32_t)__shfl_down((int)hi, 1, 64), t);
                const uint32_t lo_word = mx6_lane_word(lo, (uint32_t)__shfl_down((int)lo, 1, 64), t);
                if (in && t < 3) {
                    *reinterpret_cast<uint32_t*>(blk + ((c >> 2) & 7) * 3 + t) = hi_word;
                    *reinterpret_cast<uint32_t*>(blk + 24 + ((c >> 2) & 7) * 3 + t) = lo_word;
                }
            } else {
                const uint4 q = mx4_block_codes(v, E);
                if (in && (lane & 7) == 0) *reinterpret_cast<uint4*>(blk) = q;
            }
            if (in && (lane & 7) == 0) sc_lds[(c >> 5) * 16 + row] = live ? (uint8_t)(E + 127) : (uint8_t)127;
        }
    }
    __syncthreads();

    // ---- this wave's 16 columns of its problem's slab
    int pi = 0;
    while (pi + 1 < b.n && (int)blockIdx.x >= b.p[pi + 1].block0) ++pi;
    const SmallMMxProblem& P = b.p[pi];
    const int nw = ((int)blockIdx.x - P.block0) * 64 + wid * 16;
    if (nw >= P.N) return;                                  // whole wave past the ragged end; no barriers below
    const int lr = lane & 15, kq = lane >> 4;               // operand row / column and K block of the 128-deep step
    const int n = nw + lr, nc = min(n, P.N - 1);
    const int nsteps = P.Kp >> 7;
    const uint8_t* wp = P.w + ((int64_t)nc * (P.Kp >> 5) + kq) * 24;

    uint2 wb[4][3];                                         // the ring: weight fragments of four steps
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        wb[u][0] = wb[u][1] = wb[u][2] = make_uint2(0u, 0u);
        if (u < nsteps) {
            const uint2* src = reinterpret_cast<const uint2*>(wp + u * 96);
            wb[u][0] = src[0]; wb[u][1] = src[1]; wb[u][2] = src[2];
        }
    }
    v4f acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int s0 = 0; s0 < nsteps; s0 += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int s = s0 + u;
            if (s >= nsteps) break;                         // wave-uniform
            const v8i bf = {(int)wb[u][0].x, (int)wb[u][0].y, (int)wb[u][1].x, (int)wb[u][1].y, (int)wb[u][2].x, (int)wb[u][2].y, 0, 0};
            if (s + 4 < nsteps) {
                const uint2* src = reinterpret_cast<const uint2*>(wp + (s + 4) * 96);
                wb[u][0] = src[0]; wb[u][1] = src[1]; wb[u][2] = src[2];
            }
            const int kb = 4 * s + kq;
            const uint8_t* ap = a_lds + (kb * 16 + lr) * AB;
            const int sa = sc_lds[kb * 16 + lr];
            if constexpr (FMT == 6) {
                const uint2 a0 = *reinterpret_cast<const uint2*>(ap), a1 = *reinterpret_cast<const uint2*>(ap + 8),
                            a2 = *reinterpret_cast<const uint2*>(ap + 16);
                const v8i af = {(int)a0.x, (int)a0.y, (int)a1.x, (int)a1.y, (int)a2.x, (int)a2.y, 0, 0};
                acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af, bf, acc, 2, 2, 0, sa, 0, 128);
            } else if constexpr (FMT == 8) {
                const uint4 h4 = *reinterpret_cast<const uint4*>(ap);
                const uint4 m4 = *reinterpret_cast<const uint4*>(ap + 16);     // hi[16..23] | lo[0..7]
                const uint4 l4 = *reinterpret_cast<const uint4*>(ap + 32);     // lo[8..23]
                const v8i hf = {(int)h4.x, (int)h4.y, (int)h4.z, (int)h4.w, (int)m4.x, (int)m4.y, 0, 0};
                const v8i lf = {(int)m4.z, (int)m4.w, (int)l4.x, (int)l4.y, (int)l4.z, (int)l4.w, 0, 0};
                acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(lf, bf, acc, 2, 2, 0, sa, 0, 123);
                acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(hf, bf, acc, 2, 2, 0, sa, 0, 127);
            } else {
                const uint4 a4 = *reinterpret_cast<const uint4*>(ap);
                const v8i af = {(int)a4.x, (int)a4.y, (int)a4.z, (int)a4.w, 0, 0, 0, 0};
                acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af, bf, acc, 4, 2, 0, sa, 0, 128);
            }
        }
    }

    // ---- the MX GEMMs' plain store: register i of the lane is row 4·kq + i of column n
    if (n < P.N) {
        const float al = P.alpha[n], ga = P.gamma[n];
        T* y = reinterpret_cast<T*>(P.y);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = 4 * kq + i;
            if (m < b.M) y[(int64_t)m * P.ldy + n] = dgq_from_float<T>(dgq_dequant<false>(acc[i], 1.0f, 0.0f, 0.0f, al, 0.0f, ga, 0.0f));
        }
    }
}

template <typename T>
void smx_launch(int a_format, dim3 grid, size_t lds, hipStream_t st, const SmallMMxBatch& b) {
    if (a_format == 6) hipLaunchKernelGGL((linear_smallm_mx_kernel<T, 6>), grid, dim3(256), lds, st, b);
    else if (a_format == 8) hipLaunchKernelGGL((linear_smallm_mx_kernel<T, 8>), grid, dim3(256), lds, st, b);
    else hipLaunchKernelGGL((linear_smallm_mx_kernel<T, 4>), grid, dim3(256), lds, st, b);
}

}  // namespace

extern "C" int dgq_linear_smallm_mx_batch(const void* x, int x_dtype, int M, int K, int64_t ldx, int pre_act, int a_format, int n_problems,
                                          const dgq_smallm_mx_problem_t* probs, int y_dtype, void* stream) {
    const char* who = "dgq_linear_smallm_mx_batch";
    DGQ_CHECK_ARG(x && probs, "%s: null pointer", who);
    DGQ_CHECK_ARG(M >= 1 && M <= SMX_MAX_M, "%s: M=%d (1 .. %d)", who, M, SMX_MAX_M);
    DGQ_CHECK_ARG(K >= DGQ_KCHUNK && K % DGQ_KCHUNK == 0 && K <= SMX_MAX_K, "%s: K=%d must be a multiple of %d, <= %d", who, K, DGQ_KCHUNK, SMX_MAX_K);
    DGQ_CHECK_ARG(ldx >= K && ldx % 4 == 0 && ldx < (1LL << 30) && (reinterpret_cast<uintptr_t>(x) & 15) == 0,
                  "%s: x must be 16-byte aligned with a row stride %lld >= K, a multiple of 4", who, (long long)ldx);
    DGQ_CHECK_ARG(pre_act == 0 || pre_act == 1, "%s: pre_act=%d (0 or 1)", who, pre_act);
    DGQ_CHECK_ARG(a_format == 6 || a_format == 8 || a_format == 4, "%s: a_format=%d (6 mxfp6, 8 mxint8, 4 mxfp4)", who, a_format);
    DGQ_CHECK_ARG(n_problems >= 1 && n_problems <= SMX_MAX_PROBLEMS, "%s: %d problems (max %d)", who, n_problems, SMX_MAX_PROBLEMS);
    DGQ_CHECK_ARG(x_dtype == y_dtype && (x_dtype == DGQ_F32 || x_dtype == DGQ_F16 || x_dtype == DGQ_BF16), "%s: x/y dtypes %d/%d", who, x_dtype, y_dtype);
    SmallMMxBatch b;
    b.n = n_problems; b.x = x; b.M = M; b.K = K; b.Kq = 0; b.ldx = (int)ldx; b.pre_act = pre_act;
    int blocks = 0;
    for (int i = 0; i < n_problems; ++i) {
        const dgq_smallm_mx_problem_t& q = probs[i];
        DGQ_CHECK_ARG(q.wpacked && q.alpha && q.gamma && q.y, "%s: null pointer in problem %d", who, i);
        DGQ_CHECK_ARG(q.N > 0 && q.ldy >= q.N && q.Kp >= K && q.Kp % DGQ_KTILE == 0 && q.Kp <= SMX_MAX_K, "%s: bad problem %d (N=%d ldy=%d Kp=%d)", who, i,
                      q.N, q.ldy, q.Kp);
        DGQ_CHECK_ARG((reinterpret_cast<uintptr_t>(q.wpacked) & 15) == 0, "%s: wpacked of problem %d must be 16-byte aligned", who, i);
        SmallMMxProblem& P = b.p[i];
        P.w = reinterpret_cast<const uint8_t*>(q.wpacked); P.alpha = q.alpha; P.gamma = q.gamma; P.y = q.y;
        P.ldy = q.ldy; P.N = q.N; P.Kp = q.Kp; P.block0 = blocks;
        blocks += (q.N + 63) / 64;
        if (q.Kp > b.Kq) b.Kq = q.Kp;
    }
    const size_t lds = (size_t)(b.Kq / 32) * 16 * (smx_code_bytes(a_format) + 1);     // <= 49 KiB: within the default dynamic LDS
    hipStream_t st = (hipStream_t)stream;
    if (x_dtype == DGQ_F32) smx_launch<float>(a_format, dim3(blocks), lds, st, b);
    else if (x_dtype == DGQ_F16) smx_launch<__half>(a_format, dim3(blocks), lds, st, b);
    else smx_launch<__hip_bfloat16>(a_format, dim3(blocks), lds, st, b);
    return dgq_launch_status(who);
}
