// The W4 register stream and the K tile of the two quantise-on-load kernels (gemm_panel.hip, gemm_convq.hip): one wave, one 32 x 32
// output tile, A fragments from an LDS image, int4 weights from HBM straight into registers.
//
// W never touches LDS.  dgq_pack_w4 layout 2 stores the weights FRAGMENT-MAJOR: for every 32-column tile and every pair of 32-wide K
// chunks one 1-KiB block in which lane l finds, at l·16, the 8 bytes of its column (l & 31) and K half (l >> 5) of both chunks — 2 x 16
// bytes per lane per K tile, prefetched WF_DT K tiles ahead.  The loads are asm statements with hand-counted waits: inside a loop whose
// steps are guarded (t < n), hipcc's own bookkeeping merges the paths conservatively and drains the ring (s_waitcnt vmcnt(0)) at every
// step.  WF_NS = WF_DT + 1 register slots: the loads of tile t + WF_DT go to the slot tile t − 1 has just left, so WF_DT tiles stay in
// flight while tile t computes.  A kernel with these waits must not spill (the Makefile's check-scratch).
#pragma once
#include "gemm_tile.h"

constexpr int WF_DT = 4, WF_NS = WF_DT + 1;                 // prefetch depth in K tiles / register slots

// the two 16-byte loads of stream tile t (wsrc: the lane's address in the stream's first tile)
__device__ __forceinline__ void wfrag_load(const uint4* wsrc, int t, v4i (&dst)[2]) {
    const uint4* q = wsrc + (t * 2) * 64;
    asm volatile("global_load_dwordx4 %0, %2, off\n\tglobal_load_dwordx4 %1, %2, off offset:1024"
                 : "=&v"(dst[0]), "=&v"(dst[1]) : "v"(q) : "memory");
}
// the first WF_DT tiles of a stream of n
__device__ __forceinline__ void wfrag_start(const uint4* wsrc, int n, v4i (&wr)[WF_NS][2]) {
#pragma unroll
    for (int d = 0; d < WF_DT; ++d)
        if (d < n) wfrag_load(wsrc, d, wr[d]);
#pragma unroll
    for (int j = 0; j < 2; ++j) wr[WF_DT][j] = (v4i){0, 0, 0, 0};
}
template <int N>
__device__ __forceinline__ void wfrag_wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// Stream tile t (< n, wave-uniform) in slot sl (a constant of the caller's unrolled slot loop): tile t + WF_DT goes out, then tile t's
// two loads — the oldest in flight — are waited for; 2·min(WF_DT, n − 1 − t) younger ones may stay.
__device__ __forceinline__ void wfrag_acquire(const uint4* wsrc, int t, int n, v4i (&wr)[WF_NS][2], int sl) {
    static_assert(WF_DT == 4, "the wait ladder is written for WF_DT = 4");
    if (t + WF_DT < n) wfrag_load(wsrc, t + WF_DT, wr[(sl + WF_DT) % WF_NS]);
    const int young = min(WF_DT, n - 1 - t);
    if (young >= 4) wfrag_wait_vmcnt<8>();
    else if (young == 3) wfrag_wait_vmcnt<6>();
    else if (young == 2) wfrag_wait_vmcnt<4>();
    else if (young == 1) wfrag_wait_vmcnt<2>();
    else wfrag_wait_vmcnt<0>();
    asm volatile("" : "+v"(wr[sl][0]), "+v"(wr[sl][1]));               // the slot's registers are defined HERE for the compiler
    __builtin_amdgcn_sched_barrier(0);
}
// chunk ci of a K tile as the MFMA's B operand: the register pairs w0 (chunks 0, 1) and w1 (chunks 2, 3), int4 -> int8
__device__ __forceinline__ v4i wfrag_widen(const v4i& w0, const v4i& w1, int ci) {
    const v4i& w = ci < 2 ? w0 : w1;
    const uint32_t x = (uint32_t)((ci & 1) ? w[2] : w[0]), y = (uint32_t)((ci & 1) ? w[3] : w[1]);
    return (v4i){(int)(x & 0x0F0F0F0Fu), (int)((x >> 4) & 0x0F0F0F0Fu), (int)(y & 0x0F0F0F0Fu), (int)((y >> 4) & 0x0F0F0F0Fu)};
}

// One K tile: per chunk one ds_read_b128 (A fragment at sa + a_off[ci]), one widening, one MFMA and (per-K) the flush that is due.
// Per-K runs two accumulator sets: consecutive chunks alternate, and a chunk's flush is issued behind the NEXT chunk's MFMA (`pend`:
// the coefficient of the chunk whose flush is pending; the caller flushes acc[1] with it behind the last tile).  coef4: the tile's
// four coefficients, flag: its clear flag (both in the kernel's LDS table; not read for per-M).
template <bool PER_M, int ACCS>
__device__ __forceinline__ void wfrag_tile(const uint8_t* sa, const int (&a_off)[NCH], const float* coef4, const float* flag, const v4i& w0,
                                           const v4i& w1, v16i (&acc)[ACCS][1][1], v16f (&accf)[1][1], float& pend) {
    static_assert(ACCS == (PER_M ? 1 : 2), "per-K: two accumulator sets");
    constexpr bool BIASED = !PER_M;                         // per-K (W4): totals carry DGQ_ACC_BIAS_I (gemm_device.h)
    typedef float cvec_t __attribute__((ext_vector_type(NCH)));
    cvec_t cq;
    float tc = 0.0f;
    if (!PER_M) {
        cq = *reinterpret_cast<const cvec_t*>(coef4);
        tc = *flag;
    }
#pragma unroll
    for (int ci = 0; ci < NCH; ++ci) {
        const v4i af = *reinterpret_cast<const v4i*>(sa + a_off[ci]);
        const v4i bf = wfrag_widen(w0, w1, ci);
        if constexpr (PER_M) {
            acc[0][0][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af, bf, acc[0][0][0], 0, 0, 0);
        } else {
            if (ci & 1) {
                acc[1][0][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af, bf, acc[1][0][0], 0, 0, 0);
                gemm_flush<BIASED>(accf, acc[0], pend);
            } else {
                acc[0][0][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af, bf, acc[0][0][0], 0, 0, 0);
                gemm_flush<BIASED>(accf, acc[1], pend);
            }
            pend = cq[ci];
        }
    }
    if constexpr (!PER_M) {
        if (__builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, tc)) != 0) {     // rare: a segment of running totals ends
            gemm_flush<BIASED>(accf, acc[1], pend);
            pend = 0.0f;
            gemm_clear_totals<DGQ_ACC_BIAS_I>(acc);
        }
    }
}
