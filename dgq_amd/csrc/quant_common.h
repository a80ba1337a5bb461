// Element loads and code packing shared by the quantise-on-load kernels (quant_act.hip) and the GEMM that quantises its own operand
// panel (gemm_panel.hip, FUSE) — one implementation, so that both produce the same codes.
#pragma once
#include "dgq_common.h"

template <typename TIn>
__device__ __forceinline__ void load4(const TIn* p, float (&v)[4]);
template <>
__device__ __forceinline__ void load4<float>(const float* p, float (&v)[4]) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
template <>
__device__ __forceinline__ void load4<__half>(const __half* p, float (&v)[4]) {
    const uint2 t = *reinterpret_cast<const uint2*>(p);
    const __half* h = reinterpret_cast<const __half*>(&t);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = __half2float(h[j]);
}
template <>
__device__ __forceinline__ void load4<__hip_bfloat16>(const __hip_bfloat16* p, float (&v)[4]) {
    const uint2 t = *reinterpret_cast<const uint2*>(p);
    const uint16_t* h = reinterpret_cast<const uint16_t*>(&t);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = __uint_as_float(((uint32_t)h[j]) << 16);
}

// Four codes q_j ∈ [0, 2^b−1] (floats) -> one dword of centred int8 codes s_j = q_j − off, 0 for padding:
// v_cvt_pk_u8_f32 inserts u8(q − off + 128) per byte, and u8(x + 128) ^ 0x80 is the two's-complement byte of x.
// `biased[j]` = valid ? q_j − off + 128 : 128 ; returns the dword, adds Σ biased to `fsum` (exact small integers).
__device__ __forceinline__ uint32_t dgq_pack4(const float (&biased)[4], float& fsum) {
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) w = __builtin_amdgcn_cvt_pk_u8_f32(biased[j], j, w);
    fsum += (float)__builtin_amdgcn_sad_u8(w, 0u, 0u);       // Σ of the four bytes (the values are integers in [0, 255]: the bytes ARE the values)
    return w ^ 0x80808080u;
}


// dgq_affine_code_fast (dgq_common.h) for four elements, each with its own (δ, 1/δ, z): the same codes bit for bit, but the IEEE-division
// fallback of the tie band is ONE wave-uniform, rarely taken branch (any lane, any of the four: ~2.5 % of the calls) instead of a
// divergent branch per element — in a loop that quantises dozens of elements per lane the per-element form compiles to two or three
// taken branches per element (~100 cycles each, profiles/r05_small_launch_timeline.txt).
__device__ __forceinline__ void dgq_affine_code4_fast(const float (&x)[4], const float (&d)[4], const float (&inv)[4], const float (&z)[4],
                                                      float qmax, float (&q)[4]) {
    float r[4];
    bool nearj[4];
    bool near = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        // the tie band of dgq_affine_code_fast, |t − r| >= 0.5 − |t|·4e-7, as one fma + one compare (|t| >= 1.25e6, infinities and NaN
        // fall inside it by themselves)
        const float t = x[j] * inv[j];
        r[j] = rintf(t);
        // (written as the VOP3 instruction itself: both |.| are source modifiers.  From the C expression the compiler forms packed
        // v_pk_fma_f32 pairs, which take no modifiers, and pays a v_and_b32 per absolute value)
        float s;
        asm("v_fma_f32 %0, |%1|, %2, |%3|" : "=v"(s) : "v"(t), "v"(4.0e-7f), "v"(t - r[j]));
        nearj[j] = !(s < 0.5f);
        near = near || nearj[j];
    }
    if (__builtin_amdgcn_ballot_w64(near) != 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float rr = rintf(__fdiv_rn(x[j], d[j]));
            r[j] = nearj[j] ? rr : r[j];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = __builtin_amdgcn_fmed3f(r[j] + z[j], 0.0f, qmax);
}

// ... four elements under ONE (δ, 1/δ, z)
__device__ __forceinline__ void dgq_affine_code4_fast(const float (&x)[4], float d, float inv, float z, float qmax, float (&q)[4]) {
    const float d4[4] = {d, d, d, d}, i4[4] = {inv, inv, inv, inv}, z4[4] = {z, z, z, z};
    dgq_affine_code4_fast(x, d4, i4, z4, qmax, q);
}


// ---- Block-staged convolution quantisers (quant_act_conv_kernel, gemm_convq_kernel): a workgroup stages the input patch of its tile of
// output positions in LDS and every row of the tile gathers its codes from it through the kpat table.  What the gather needs of the
// tables depends on the column kp alone, so it is resolved ONCE per workgroup, where the tables are staged, and not per code:
//   tab[Kp]    16-bit patch index; a padding entry (kpat < 0) holds index 0 — in bounds, so the gather address needs no test, and the
//              value read is never used: the byte of a padding position is replaced after the pack (vm below);
//   rec[Kp/32] per 32-chunk {δ, z, 1/δ (dgq_rcp: the bits the per-dword evaluation gave), vm}; vm bit i = position 32·c + i is valid.
//              Per-M / scalar layers use vm alone (their δ, z, 1/δ belong to the row).
struct DgqChunkRec { float d, z, inv; uint32_t vm; };
static_assert(sizeof(DgqChunkRec) == 16, "one ds_read_b128 per record");
__host__ __device__ constexpr int dgq_conv_rec_bytes(int Kp) { return (Kp >> 5) * (int)sizeof(DgqChunkRec); }

// All `nthreads` (a multiple of 8) threads of the workgroup; Kp % 32 == 0, so the 8 consecutive lanes of a chunk run together.
template <bool PER_M>
__device__ __forceinline__ void dgq_conv_tables_resolve(const int32_t* kpat, const float* delta, const float* zp, int Kp, uint16_t* tab,
                                                        DgqChunkRec* rec, int tid, int nthreads) {
    for (int k = tid * 4; k < Kp; k += 4 * nthreads) {
        const int4 e = *reinterpret_cast<const int4*>(kpat + k);
        const uint32_t i0 = e.x < 0 ? 0u : (uint32_t)e.x, i1 = e.y < 0 ? 0u : (uint32_t)e.y, i2 = e.z < 0 ? 0u : (uint32_t)e.z,
                       i3 = e.w < 0 ? 0u : (uint32_t)e.w;
        *reinterpret_cast<uint2*>(tab + k) = make_uint2(i0 | (i1 << 16), i2 | (i3 << 16));
        uint32_t vm = ((e.x >= 0 ? 1u : 0u) | (e.y >= 0 ? 2u : 0u) | (e.z >= 0 ? 4u : 0u) | (e.w >= 0 ? 8u : 0u)) << (4 * (tid & 7));
        vm |= __shfl_xor(vm, 1, 64);
        vm |= __shfl_xor(vm, 2, 64);
        vm |= __shfl_xor(vm, 4, 64);
        if ((tid & 7) == 0) {
            DgqChunkRec rc = {1.0f, 0.0f, 1.0f, vm};
            if (!PER_M) { rc.d = delta[k >> 5]; rc.z = zp[k >> 5]; rc.inv = dgq_rcp(rc.d); }
            rec[k >> 5] = rc;
        }
    }
}

// Element idx of the row's patch window, idx = the low (HI = 0) or the high (HI = 1) 16 bits of `pair`: the LDS byte address is ONE
// v_mad_u32_u16 (op_sel picks the half; base + 4·idx) — from the C expression the compiler unpacks the half and then shifts and adds.
// `base`: the window's LDS byte address (wave-uniform).
typedef const __attribute__((address_space(3))) float dgq_lds_cfloat;
template <int HI>
__device__ __forceinline__ float dgq_lds_gather16(uint32_t base, uint32_t pair) {
    uint32_t a;
    if (HI) asm("v_mad_u32_u16 %0, %1, 4, %2 op_sel:[1,0,0,0]" : "=v"(a) : "v"(pair), "s"(base));
    else asm("v_mad_u32_u16 %0, %1, 4, %2" : "=v"(a) : "v"(pair), "s"(base));
    return *reinterpret_cast<dgq_lds_cfloat*>(a);
}

// One round of a row: QU steps of 256 codes from the wave-uniform position kbu; lane = 4 consecutive kp (one packed dword) per step.
// Every table read and every gather of the round is issued before the first code is formed.  `k1` (a multiple of 128) ends the range:
// FULL = the caller knows kbu + 256·QU <= k1 and no position is tested; otherwise a step at or past k1 is skipped (wave-uniform) and the
// upper half-wave of a last half step computes on a clamped position, stores nothing and adds 0.  store(kp0, dword) takes the codes.
// Returns `part` plus the round's terms of the row sum, one addition per step in ascending order (per-K: δ_c·Σs, per-M: Σs).
// `pr`: the row's window of the patch; `sh4` = 4·(lane & 7), the lane's nibble of vm; `bias4` = (128 − offset) in each byte.
template <bool PER_M, int QU, bool FULL, typename Store>
__device__ __forceinline__ float dgq_conv_quant_round(const float* pr, const uint16_t* tab, const DgqChunkRec* rec, int kbu, int k1, int lane,
                                                      uint32_t sh4, float md, float mz, float minv, float qmax, uint32_t bias4, float part,
                                                      Store&& store) {
    uint2 tt[QU];
    int kpc[QU];
#pragma unroll
    for (int u = 0; u < QU; ++u) {
        kpc[u] = kbu + 256 * u + lane * 4;
        if (!FULL) kpc[u] = min(kpc[u], k1 - 4);
        tt[u] = *reinterpret_cast<const uint2*>(tab + kpc[u]);
    }
    const uint32_t prb = (uint32_t)reinterpret_cast<uintptr_t>((dgq_lds_cfloat*)pr);
    float v[QU][4];
#pragma unroll
    for (int u = 0; u < QU; ++u) {
        v[u][0] = dgq_lds_gather16<0>(prb, tt[u].x); v[u][1] = dgq_lds_gather16<1>(prb, tt[u].x);
        v[u][2] = dgq_lds_gather16<0>(prb, tt[u].y); v[u][3] = dgq_lds_gather16<1>(prb, tt[u].y);
    }
    // the lane's records of a whole round: 8 lanes per chunk, 8 chunks per step — constant offsets from one address
    const DgqChunkRec* rl = rec + (lane >> 3) + (kbu >> 5);
    // (constants of the selector below, held in registers: as literals they keep v_and_or_b32, a VOP3, from being formed)
    uint32_t sel_bit = 0x04040404u, sel_id = 0x03020100u;
    asm("" : "+s"(sel_bit));
    asm("" : "+v"(sel_id));
#pragma unroll
    for (int u = 0; u < QU; ++u) {
        if (!FULL && kbu + 256 * u >= k1) break;             // wave-uniform
        const DgqChunkRec rc = FULL ? rl[8 * u] : rec[kpc[u] >> 5];
        float qv[4];
        dgq_affine_code4_fast(v[u], PER_M ? md : rc.d, PER_M ? minv : rc.inv, PER_M ? mz : rc.z, qmax, qv);
        uint32_t w = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) w = __builtin_amdgcn_cvt_pk_u8_f32(qv[j], j, w);
        w += bias4;                                          // q <= 2^b − 1 and offset = 2^(b−1): q − offset + 128 <= 255, no byte carries
        // padding bytes -> 128 (code 0): the lane's four valid bits, one per byte at bit 2, make the selector of ONE v_perm_b32 —
        // byte j of w where valid (4 + j), a byte of the constant where not (j)
        const uint32_t nib = __builtin_amdgcn_ubfe(rc.vm, sh4, 4u);
        const uint32_t sel = (__umul24(nib, 0x810204u) & sel_bit) | sel_id;
        w = __builtin_amdgcn_perm(w, 0x80808080u, sel);
        // Σ (s_j + 128) − 512 = Σ s_j, formed in the sad's accumulator (integers: the float of it is the value the fp32 subtraction gave)
        const float fsum = (float)(int)__builtin_amdgcn_sad_u8(w, 0u, (uint32_t)-512);
        const float term = PER_M ? fsum : rc.d * fsum;
        if (FULL) {
            store(kpc[u], w ^ 0x80808080u);
            part += term;
        } else {
            const bool in = kbu + 256 * u + lane * 4 < k1;
            if (in) store(kpc[u], w ^ 0x80808080u);
            part += in ? term : 0.0f;
        }
    }
    return part;
}
