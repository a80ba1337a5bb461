// Un-quantised attention on the 16-bit matrix cores, one launch, no workspace (opt-in: the attention modules' attention_mfma16 flag for
// fp16 / bf16 tensors, attention_mfma16_fp32 for the fp32 state):
//     o[b,t,h,:] = Σ_j p̂_j·v[b,j,h,:] / l,   s_j = fp32(Σ_d q_d·k_{j,d})·scale,   p_j = exp(s_j − m),   l = Σ_j p_j
// on tensors in the projection layout (q [B][T][H·D], k / v [B][S][H·D], o [B][T][H·D]).  Both products accumulate in fp32.  Online
// softmax over stages of 64 keys (two 32-key score tiles) or 32: running maximum m in log2 units, rescale of l and of the accumulator
// when m moves (skipped for a stage in which no query of the wave moved its maximum: the factor is exactly 1 then).  l sums the
// UNROUNDED fp32 p_j, so the normaliser adds no rounding of its own.  The exponential runs in base 2 (v_exp_f32 on s·scale·log2 e).
// No quantiser, so no global δ: no statistics pass, no workspace, no merge — nothing is exchanged between workgroups.
//
// Orientation as in attn_bf16x3.hip: the score tile is transposed (Sᵀ = K·Qᵀ: key on the register, query on the lane), so a query's
// statistics live in the lane pair (l, l ^ 32) and the tile's accumulator registers, converted pairwise to 16 bits, are directly the
// B operand of Oᵀ = Vᵀ·P̂ᵀ in the permuted k order key_of(r, h) (attn_bf16x3_dev.h).  V is therefore staged TRANSPOSED with the keys
// of a 32-key tile in that order: key 16s + 8a + 4h + b sits in slot 16s + 8h + 4a + b of its Vᵀ row.
//
// 256 threads = four waves x 32 query rows share the K / Vᵀ tiles of one (batch, head) through LDS: the global loads of stage t+1 are
// issued before stage t is multiplied and written behind its products — to the other buffer, one barrier per stage, or (one-buffer
// form) to the same one behind a second barrier.
// Ragged edges by construction: every global load is clamped in bounds (key min(j, S−1), query min(t, T−1)); keys j >= S get score
// −inf, so p = 0 exactly (every stage the loop visits holds at least one real key, so m is finite from the first stage on and no
// (−inf) − (−inf) is formed); query rows t >= T are computed on the clamped row and not stored.  The head dim is zero padded to the
// MFMA's K granularity (8 -> 16, 40 -> 48) by LDS columns / Vᵀ rows that are cleared once and never written.
//
// ONE kernel body serves both element types; an operand policy (Op16<F16>, OpSplit below) holds the four places where they differ:
//   1. operand element.  16-bit tensors enter the matrix cores as they are (their products are exact in fp32); p̂_j is p_j rounded to
//      the tensors' dtype (round to nearest even) for the P·V product ONLY.  Every fp32 operand enters as the two-term bf16 split
//      hi = bf16_rn(x), lo = bf16_rn(x − hi)  (x − hi is exact in fp32): Q is split once into registers, K and V ONCE per workgroup
//      while the tile is staged (fp32 global load -> registers -> two bf16 LDS planes), p when it is formed.  A stage is
//      [K planes][Vᵀ planes] with the same pitches for both.
//   2. products per K step.  One V_MFMA_F32_32X32X16_BF16 / _F16 for 16-bit operands; three _BF16 into ONE accumulator for the split,
//      the small terms first: lo·hi, hi·lo, hi·hi (lo·lo, 2^-18 relative, is dropped) — am16_term().
//      16-bit operands go into the MFMA as they are read from LDS, tile by tile; the split loads the fragments of all tiles of a
//      K step first and issues term by term over them — group().
//   3. epilogue.  16 bits: acc·(1/l) rounded to the dtype, one 8-byte store.  fp32: acc / l as an IEEE division ((S·c) / S == c
//      exactly), one 16-byte store — quot4(), which RETURNS the four elements: the kernel stores them.
//   4. LDS.  16-bit tensors: a static array with two buffers (<= 50 176 bytes).  Two planes double the image (up to 100 352 bytes
//      at D = 80), so the LDS of the fp32 entry is dynamic, with ONE buffer or two.  The form per head dim is chosen at the two
//      launchers below.
// The places marked (schedule) are written as they are because the other spelling moved the compiler's schedule away from the
// two kernels this one replaces (profiles/r19_attention_mfma16_shared_ab.txt).  profiles/r19_attention_mfma16_shared_resources.txt
// lists which instruction streams equal theirs: after a change to such a place, compare `hipcc -S` listings again, kernel by kernel
// (tools/kernel_resources_diff.py --rename, or a diff of the streams), before anything is timed.
#include <stdlib.h>
#include <type_traits>
#include "attn_bf16x3_dev.h"

typedef _Float16 am16_f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 am16_bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 am16_f16x2 __attribute__((ext_vector_type(2)));

template <typename E> struct Am16Params {
    const E* q;
    const E* k;
    const E* v;
    E* o;
    int B, H, T, S;
    float scale2;            // scale · log2 e
};

template <int D, int NKT, int NBUF, int NP> struct Am16Geo {
    static constexpr int KTW = KT * NKT;              // keys per stage: NKT score tiles of 32 keys
    static constexpr int DP = (D + 15) / 16 * 16;     // depth of the score product
    static constexpr int NKK = DP / 16;
    static constexpr int NDT = (D + 31) / 32;         // 32-row d tiles of Oᵀ
    static constexpr int DV = NDT * 32;
    static constexpr int KLD = DP + 8;                // elements per K row (16-byte aligned rows, de-conflicted)
    static constexpr int VLD = KTW + 8;               // elements per Vᵀ row
    static constexpr int CK = D / 8;                  // 8-element chunks of one key's head slice
    static constexpr int K_TASKS = KTW * CK;          // staging: (key row, chunk) -> one 16-byte LDS write per plane
    static constexpr int V_TASKS = (KTW / 2) * CK;    // staging: (key pair, chunk) -> eight 4-byte LDS writes of Vᵀ per plane
    static constexpr int KU = (K_TASKS + 255) / 256;
    static constexpr int VU = (V_TASKS + 255) / 256;
    static constexpr int K_ELEMS = KTW * KLD;         // one plane; K plane q at q·K_ELEMS, V plane q at q·V_ELEMS behind all K planes
    static constexpr int V_ELEMS = DV * VLD;
    static constexpr int STAGE_ELEMS = NP * (K_ELEMS + V_ELEMS);
    static constexpr int LDS_BYTES = NBUF * STAGE_ELEMS * 2;
    static_assert(LDS_BYTES <= 160 * 1024 && LDS_BYTES % 16 == 0, "LDS");
};

// Product i of one K step as (ab = 0: plane of the A operand K / Vᵀ, ab = 1: plane of the B operand Q / P̂), plane 0 = hi, 1 = lo.
// One plane: the single product (0, 0); two planes: three, small terms first.
__device__ constexpr int am16_term(int np, int i, int ab) {
    constexpr int t[3][2] = {{0, 1}, {1, 0}, {0, 0}};
    return np == 1 ? 0 : t[i][ab];
}

__device__ __forceinline__ uint32_t am16_pack_bf16(float a, float b) {
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f2{a, b}, am16_bf16x2));
}

// 16-bit tensors: the operands as they are
template <bool F16> struct Op16 {
    using E = uint16_t;
    static constexpr int NP = 1;
    static constexpr bool STATIC_LDS = true;          // two buffers of one plane fit a static array (<= 50 176 bytes): constant addresses
    // tiles whose fragments are loaded before their products are issued, of n: one — every MFMA takes its A operand as it is read
    static constexpr int group(int n) { return 1; }
    struct Raw {                                      // eight elements as loaded
        v4i x;
        static __device__ __forceinline__ Raw load8(const E* p) { return Raw{*reinterpret_cast<const v4i*>(p)}; }
    };
    static __device__ __forceinline__ void planes(const Raw& r, v4i (&f)[1]) { f[0] = r.x; }
    static __device__ __forceinline__ void pair(const Raw& a, const Raw& b, int e, uint32_t (&w)[1]) {
        const uint32_t x = (uint32_t)a.x[e >> 1], y = (uint32_t)b.x[e >> 1];
        w[0] = (e & 1) ? (x >> 16) | (y & 0xFFFF0000u) : (x & 0xFFFFu) | (y << 16);
    }
    static __device__ __forceinline__ void round2(float p0, float p1, uint32_t (&w)[1]) {
        if constexpr (F16) w[0] = __builtin_bit_cast(uint32_t, __builtin_convertvector(f2{p0, p1}, am16_f16x2));
        else w[0] = am16_pack_bf16(p0, p1);
    }
    static __device__ __forceinline__ v16f mfma(const v4i& a, const v4i& b, v16f c) {
        if constexpr (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(am16_f16x8, a), __builtin_bit_cast(am16_f16x8, b), c, 0, 0, 0);
        else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
    using Out4 = uint2;                               // four output elements as stored
    static __device__ __forceinline__ Out4 quot4(float a0, float a1, float a2, float a3, float l) {
        const float inv = 1.0f / l;
        uint32_t w[2][1];
        round2(a0 * inv, a1 * inv, w[0]);
        round2(a2 * inv, a3 * inv, w[1]);
        return make_uint2(w[0][0], w[1][0]);
    }
};

// fp32 tensors: two bf16 planes (hi, lo) of every operand
struct OpSplit {
    using E = float;
    static constexpr int NP = 2;
    static constexpr bool STATIC_LDS = false;         // up to 100 352 bytes: dynamic
    static constexpr int group(int n) { return n; }   // all n tiles: the term loop runs over them, small terms first
    struct Raw {                                      // the fp32 values: they are split when they are written to LDS, behind the stage's products
        v4f x[2];
        static __device__ __forceinline__ Raw load8(const E* p) { return Raw{{*reinterpret_cast<const v4f*>(p), *reinterpret_cast<const v4f*>(p + 4)}}; }
    };
    // two values -> the packed hi pair and the packed lo pair (a in the low half)
    static __device__ __forceinline__ void round2(float a, float b, uint32_t (&w)[2]) {
        w[0] = am16_pack_bf16(a, b);
        w[1] = am16_pack_bf16(a - __uint_as_float(w[0] << 16), b - __uint_as_float(w[0] & 0xFFFF0000u));
    }
    static __device__ __forceinline__ void planes(const Raw& r, v4i (&f)[2]) {
        uint32_t w[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i) round2(r.x[i >> 1][2 * (i & 1)], r.x[i >> 1][2 * (i & 1) + 1], w[i]);
#pragma unroll
        for (int q = 0; q < 2; ++q) f[q] = v4i{(int)w[0][q], (int)w[1][q], (int)w[2][q], (int)w[3][q]};
    }
    static __device__ __forceinline__ void pair(const Raw& a, const Raw& b, int e, uint32_t (&w)[2]) { round2(a.x[e >> 2][e & 3], b.x[e >> 2][e & 3], w); }
    static __device__ __forceinline__ v16f mfma(const v4i& a, const v4i& b, v16f c) { return Op16<false>::mfma(a, b, c); }
    using Out4 = v4f;
    static __device__ __forceinline__ Out4 quot4(float a0, float a1, float a2, float a3, float l) {
        return v4f{__fdiv_rn(a0, l), __fdiv_rn(a1, l), __fdiv_rn(a2, l), __fdiv_rn(a3, l)};
    }
};

extern __shared__ __attribute__((aligned(16))) uint16_t am16_lds[];

template <int D, int NKT, int NBUF, typename Op>
__global__ __launch_bounds__(256) void am16_kernel(Am16Params<typename Op::E> p) {
    using E = typename Op::E;
    using Raw = typename Op::Raw;
    constexpr int NP = Op::NP, NTERM = NP == 1 ? 1 : 3;
    using G = Am16Geo<D, NKT, NBUF, NP>;
    uint16_t* lds;
    if constexpr (Op::STATIC_LDS) {
        __shared__ __attribute__((aligned(16))) uint16_t img[G::LDS_BYTES / 2];
        lds = img;
    } else {
        lds = am16_lds;
    }
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, h32 = lane >> 5, l31 = lane & 31;
    int bx, bh;
    attn_block_coords(1, bx, bh);
    const int b = bh / p.H, hd = bh - b * p.H;
    const int64_t HD = (int64_t)p.H * D;
    const E* kbase = p.k + (int64_t)b * p.S * HD + hd * D;
    const E* vbase = p.v + (int64_t)b * p.S * HD + hd * D;

    // ---- clear every stage once: the padding columns of K and the rows d >= D of Vᵀ are never written again
    for (int i = tid; i < G::LDS_BYTES / 16; i += 256) reinterpret_cast<v4i*>(lds)[i] = v4i{0, 0, 0, 0};

    // ---- this lane's query as B-operand fragments per plane: element j of qf[kk][q] = q[t][16kk + 8h + j]
    const int t = bx * 128 + wid * 32 + l31;
    const E* qrow = p.q + ((int64_t)b * p.T + min(t, p.T - 1)) * HD + hd * D;
    v4i qf0[G::NKK] = {}, qf1[G::NKK] = {};          // (schedule: an array per plane; qf1 is unused, and gone, for one plane)
#pragma unroll
    for (int kk = 0; kk < G::NKK; ++kk) {
        const int d0 = 16 * kk + 8 * h32;              // D % 8 == 0: the eight elements are all inside D or all padding
        if (d0 < D) {
            v4i f[NP];
            Op::planes(Raw::load8(qrow + d0), f);
            qf0[kk] = f[0];
            qf1[kk] = f[NP - 1];
        }
    }

    // ---- staging roles.  K: task i = (key row i / CK, chunk i % CK).  V: task i = (chunk, key pair), pairs fastest: keys 2·pair and
    // 2·pair + 1 are neighbours in the permuted slot order too, so one 4-byte write per head-dim element and plane places both
    Raw kr[G::KU], va[G::VU], vb[G::VU];            // (native vectors inside: an array of HIP's uint4 struct stayed in scratch)
    auto load_tile = [&](int s0) {
#pragma unroll
        for (int u = 0; u < G::KU; ++u) {
            const int i = min(tid + 256 * u, G::K_TASKS - 1);
            const int r = i / G::CK, c = i - r * G::CK;
            kr[u] = Raw::load8(kbase + (int64_t)min(s0 + r, p.S - 1) * HD + 8 * c);
        }
#pragma unroll
        for (int u = 0; u < G::VU; ++u) {
            const int i = min(tid + 256 * u, G::V_TASKS - 1);
            const int c = i / (G::KTW / 2), key = s0 + 2 * (i - c * (G::KTW / 2));
            const E* sa = vbase + (int64_t)min(key, p.S - 1) * HD + 8 * c;      // (schedule: both addresses before the loads)
            const E* sb = vbase + (int64_t)min(key + 1, p.S - 1) * HD + 8 * c;
            va[u] = Raw::load8(sa);
            vb[u] = Raw::load8(sb);
        }
    };
    auto store_tile = [&](int buf) {
        uint16_t* ks = lds + buf * G::STAGE_ELEMS;
        uint16_t* vs = ks + NP * G::K_ELEMS;
#pragma unroll
        for (int u = 0; u < G::KU; ++u) {
            const int i = tid + 256 * u;
            if (i < G::K_TASKS) {
                const int r = i / G::CK, c = i - r * G::CK;
                v4i f[NP];
                Op::planes(kr[u], f);
                *reinterpret_cast<v4i*>(ks + r * G::KLD + 8 * c) = f[0];
                if constexpr (NP == 2) *reinterpret_cast<v4i*>(ks + G::K_ELEMS + r * G::KLD + 8 * c) = f[1];      // (schedule: not a loop)
            }
        }
#pragma unroll
        for (int u = 0; u < G::VU; ++u) {
            const int i = tid + 256 * u;
            if (i < G::V_TASKS) {
                const int c = i / (G::KTW / 2), key = 2 * (i - c * (G::KTW / 2));
                const int slot = (key & ~15) + 8 * ((key >> 2) & 1) + 4 * ((key >> 3) & 1) + (key & 3);     // key 16s+8a+4h+b -> 16s+8h+4a+b
                uint16_t* dst = vs + (8 * c) * G::VLD + slot;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    uint32_t w[NP];                        // (this key | the next key << 16) of head-dim element 8c + e
                    Op::pair(va[u], vb[u], e, w);
#pragma unroll
                    for (int q = 0; q < NP; ++q) *reinterpret_cast<uint32_t*>(dst + q * G::V_ELEMS + e * G::VLD) = w[q];
                }
            }
        }
    };

    v16f acc[G::NDT] = {};
    float m = -INFINITY, l = 0.0f;         // m in log2 units, shared by the lane pair; l: this lane's half of the row sum

    const int NT = (p.S + G::KTW - 1) / G::KTW;
    load_tile(0);
    __syncthreads();                        // (the clear is complete)
    store_tile(0);
    __syncthreads();
    for (int it = 0; it < NT; ++it) {
        const int s0 = it * G::KTW;
        if (it + 1 < NT) load_tile(s0 + G::KTW);
        const uint16_t* ks = lds + (NBUF == 2 ? (it & 1) : 0) * G::STAGE_ELEMS;
        const uint16_t* vs = ks + NP * G::K_ELEMS;

        // ---- Sᵀ tiles: sc[j][r] = Σ_d k[s0 + 32j + key_of(r, h)][d]·q[t][d], per K step the terms of am16_term (NKT independent chains)
        v16f sc[NKT] = {};
        const uint16_t* kp = ks + l31 * G::KLD + 8 * h32;
        constexpr int JB = Op::group(NKT);      // score tiles whose fragments are loaded before their products are issued
#pragma unroll
        for (int kk = 0; kk < G::NKK; ++kk)
#pragma unroll
            for (int j0 = 0; j0 < NKT; j0 += JB) {
                v4i kf[JB][NP];
#pragma unroll
                for (int j = 0; j < JB; ++j) {            // (schedule: the planes written out, not a loop)
                    kf[j][0] = *reinterpret_cast<const v4i*>(kp + (32 * (j0 + j)) * G::KLD + 16 * kk);
                    if constexpr (NP == 2) kf[j][1] = *reinterpret_cast<const v4i*>(kp + G::K_ELEMS + (32 * (j0 + j)) * G::KLD + 16 * kk);
                }
                if constexpr (NP == 1) {
#pragma unroll
                    for (int i = 0; i < NTERM; ++i)
#pragma unroll
                        for (int j = 0; j < JB; ++j) sc[j0 + j] = Op::mfma(kf[j][am16_term(NP, i, 0)], am16_term(NP, i, 1) ? qf1[kk] : qf0[kk], sc[j0 + j]);
                } else {                    // (schedule: the rows of am16_term written out; as the loop above, the fp32 D = 80 loops moved)
#pragma unroll
                    for (int j = 0; j < JB; ++j) sc[j0 + j] = Op::mfma(kf[j][0], qf1[kk], sc[j0 + j]);
#pragma unroll
                    for (int j = 0; j < JB; ++j) sc[j0 + j] = Op::mfma(kf[j][1], qf0[kk], sc[j0 + j]);
#pragma unroll
                    for (int j = 0; j < JB; ++j) sc[j0 + j] = Op::mfma(kf[j][0], qf0[kk], sc[j0 + j]);
                }
            }

        // ---- online softmax in log2 units, one maximum and one rescale per stage
        float x[NKT][16];
#pragma unroll
        for (int j = 0; j < NKT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) x[j][r] = sc[j][r] * p.scale2;
        if (s0 + G::KTW > p.S) {            // the last, partial stage (wave-uniform)
#pragma unroll
            for (int j = 0; j < NKT; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (s0 + 32 * j + key_of(r, h32) >= p.S) x[j][r] = -INFINITY;
        }
        float mx = x[0][0];
#pragma unroll
        for (int j = 0; j < NKT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, x[j][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mn = fmaxf(m, mx);      // finite: the stage holds at least one real key
        if (__any(mn != m)) {
            const float alpha = __builtin_amdgcn_exp2f(m - mn);       // exp2(−inf) = 0 on the first stage; 1 for a lane that did not move
            l *= alpha;
#pragma unroll
            for (int dt = 0; dt < G::NDT; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[dt][r] *= alpha;
            m = mn;
        }
        uint32_t pw[NKT][8][NP];
#pragma unroll
        for (int j = 0; j < NKT; ++j)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const float p0 = __builtin_amdgcn_exp2f(x[j][r] - m), p1 = __builtin_amdgcn_exp2f(x[j][r + 1] - m);
                l += p0;
                l += p1;
                Op::round2(p0, p1, pw[j][r >> 1]);
            }

        // ---- Oᵀ += Vᵀ·P̂ᵀ: registers 8s .. 8s+7 of score tile j are the B fragment of k-step 2j + s; per k-step the terms of am16_term
        const uint16_t* vp = vs + l31 * G::VLD + 8 * h32;
        // (DTB d tiles per k-step, as JB above: one plane takes a d tile's two k-steps back to back)
        constexpr int DTB = Op::group(G::NDT);
#pragma unroll
        for (int j = 0; j < NKT; ++j)
#pragma unroll
            for (int d0 = 0; d0 < G::NDT; d0 += DTB)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    v4i pb[NP], vf[DTB][NP];
#pragma unroll
                    for (int q = 0; q < NP; ++q)
                        pb[q] = v4i{(int)pw[j][4 * s][q], (int)pw[j][4 * s + 1][q], (int)pw[j][4 * s + 2][q], (int)pw[j][4 * s + 3][q]};
#pragma unroll
                    for (int dt = 0; dt < DTB; ++dt)
#pragma unroll
                        for (int q = 0; q < NP; ++q)
                            vf[dt][q] = *reinterpret_cast<const v4i*>(vp + q * G::V_ELEMS + (32 * (d0 + dt)) * G::VLD + 32 * j + 16 * s);
#pragma unroll
                    for (int i = 0; i < NTERM; ++i)
#pragma unroll
                        for (int dt = 0; dt < DTB; ++dt) acc[d0 + dt] = Op::mfma(vf[dt][am16_term(NP, i, 0)], pb[am16_term(NP, i, 1)], acc[d0 + dt]);
                }

        if constexpr (NBUF == 2) {
            if (it + 1 < NT) store_tile((it + 1) & 1);
            __syncthreads();
        } else {                            // one buffer: every wave has read the stage before it is overwritten
            __syncthreads();
            if (it + 1 < NT) store_tile(0);
            __syncthreads();
        }
    }

    // ---- epilogue: o[t][32dt + 8g + 4h + 0..3] = acc[dt][4g + 0..3] / l, one store
    l += __shfl_xor(l, 32, 64);
    if (t >= p.T) return;
    E* orow = p.o + ((int64_t)b * p.T + t) * HD + hd * D;
#pragma unroll
    for (int dt = 0; dt < G::NDT; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int d = 32 * dt + 8 * g + 4 * h32;
            if (d < D)                       // (schedule: a policy function that stored through a pointer argument moved the fp32 epilogue)
                *reinterpret_cast<typename Op::Out4*>(orow + d) = Op::quot4(acc[dt][4 * g], acc[dt][4 * g + 1], acc[dt][4 * g + 2], acc[dt][4 * g + 3], l);
        }
}

template <int D, int NKT, int NBUF, typename Op>
static void am16_launch_form(const Am16Params<typename Op::E>& p, hipStream_t st) {
    using G = Am16Geo<D, NKT, NBUF, Op::NP>;
    constexpr int DYN = Op::STATIC_LDS ? 0 : G::LDS_BYTES;
    if constexpr (DYN > 0) {
        static std::atomic<bool> attr_set[64];
        dgq_allow_dynamic_lds(attr_set, {{&am16_kernel<D, NKT, NBUF, Op>, DYN}});
    }
    const dim3 grid((p.T + 127) / 128, p.B * p.H);
    hipLaunchKernelGGL((am16_kernel<D, NKT, NBUF, Op>), grid, dim3(256), DYN, st, p);
}

// 16-bit tensors, keys per stage: 64 (two score tiles per barrier, two independent MFMA chains, one maximum and one rescale for both)
// below D = 160, 32 at D = 160 (two 64-key stages do not fit the static LDS), always two buffers.  DGQ_ATTN16_KT = 32 in the environment
// (read per call) forces the 32-key form: tools/bench_attention_mfma16.py measures the two against each other; no product path sets it.
template <int D>
static void am16_launch(const Am16Params<uint16_t>& p, int dtype, hipStream_t st) {
    if constexpr (D <= 80) {
        const char* e = getenv("DGQ_ATTN16_KT");
        if (!(e && atoi(e) == 32)) return dtype == DGQ_F16 ? am16_launch_form<D, 2, 2, Op16<true>>(p, st) : am16_launch_form<D, 2, 2, Op16<false>>(p, st);
    }
    return dtype == DGQ_F16 ? am16_launch_form<D, 1, 2, Op16<true>>(p, st) : am16_launch_form<D, 1, 2, Op16<false>>(p, st);
}

// fp32 tensors, the form per head dim: 0 = 64-key stages, two buffers (65 536 … 100 352 bytes); 1 = 32-key stages, two buffers; 2 = the
// widest stage with ONE buffer and a second barrier per stage.  D = 160 has no 64-key form (two planes of one such stage are 89 088
// bytes): a request for form 0 gets form 1 there.  Measured (profiles/r15_attention_mfma16_fp32.txt): below D = 160 form 0 — form 1
// is 10–25 % slower on the 1024- and 4096-key calls and 0.4–1.7 us faster on the 77-key ones, form 2 within ±5 % of form 0 with no
// side ahead on every shape of a head dim; at D = 160 (key ranges of 64–256 in the models served, i.e. 2–8 stages) form 2: 0.4–0.5 us
// faster than form 1 on each of its four shapes — half the LDS to clear, and no second stage in flight to pay for it.
// DGQ_ATTN16F_FORM = 0 / 1 / 2 in the environment (read per call) forces a form: tools/bench_attention_mfma16.py measures them against
// each other; no product path sets it.
template <int D>
static void am16f_launch(const Am16Params<float>& p, hipStream_t st) {
    int form = D == 160 ? 2 : 0;
    if (const char* e = getenv("DGQ_ATTN16F_FORM")) {
        const int f = atoi(e);
        if (f >= 0 && f <= 2) form = f;
    }
    if constexpr (D <= 80) {
        if (form == 0) return am16_launch_form<D, 2, 2, OpSplit>(p, st);
        if (form == 2) return am16_launch_form<D, 2, 1, OpSplit>(p, st);
        return am16_launch_form<D, 1, 2, OpSplit>(p, st);
    } else {
        if (form == 2) return am16_launch_form<D, 1, 1, OpSplit>(p, st);
        return am16_launch_form<D, 1, 2, OpSplit>(p, st);
    }
}

// the checks both entries share, under the entry's own name; dtype: the 16-bit entry's tensor type (nullptr: fp32 by signature)
static int am16_check_args(const char* name, const void* q, const void* k, const void* v, const void* o, const int* dtype, int B, int H, int T,
                           int S, int D) {
    DGQ_CHECK_ARG(q && k && v && o, "%s: null pointer", name);
    DGQ_CHECK_ARG(B > 0 && H > 0 && T > 0 && S > 0, "%s: bad geometry (B=%d H=%d T=%d S=%d)", name, B, H, T, S);
    DGQ_CHECK_ARG(D == 8 || D == 16 || D == 40 || D == 64 || D == 80 || D == 160, "%s: head_dim D=%d (8, 16, 40, 64, 80, 160)", name, D);
    if (dtype && *dtype == DGQ_F32) {
        dgq_set_error("%s: fp32 tensors stay on dgq_attention (mode 0: the exact fp32 MFMA)", name);
        return DGQ_EUNSUPPORTED;
    }
    DGQ_CHECK_ARG(!dtype || *dtype == DGQ_F16 || *dtype == DGQ_BF16, "%s: unknown dtype %d", name, dtype ? *dtype : 0);
    DGQ_CHECK_ARG((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) & 15) == 0, "%s: q, k, v, o must be 16-byte aligned", name);
    DGQ_CHECK_ARG((int64_t)B * H <= 65535, "%s: B·H=%lld exceeds the grid", name, (long long)B * H);
    return DGQ_OK;
}

// the head-dim switch of both entries: f(std::integral_constant<int, Ds>) for the one Ds that equals D (am16_check_args admitted it)
template <int... Ds, typename F> static void am16_head_dim(int D, F&& f) { ((D == Ds ? f(std::integral_constant<int, Ds>()) : void()), ...); }

extern "C" int dgq_attention_mfma16(const void* q, const void* k, const void* v, void* o, int dtype, int B, int H, int T, int S, int D,
                                    float scale, void* stream) {
    if (const int rc = am16_check_args("dgq_attention_mfma16", q, k, v, o, &dtype, B, H, T, S, D)) return rc;
    using E = const uint16_t*;
    const Am16Params<uint16_t> p = {E(q), E(k), E(v), reinterpret_cast<uint16_t*>(o), B, H, T, S, scale * LOG2E};
    am16_head_dim<8, 16, 40, 64, 80, 160>(D, [&](auto d) { am16_launch<decltype(d)::value>(p, dtype, (hipStream_t)stream); });
    return dgq_launch_status("dgq_attention_mfma16");
}

extern "C" int dgq_attention_mfma16_f32(const float* q, const float* k, const float* v, float* o, int B, int H, int T, int S, int D, float scale,
                                        void* stream) {
    if (const int rc = am16_check_args("dgq_attention_mfma16_f32", q, k, v, o, nullptr, B, H, T, S, D)) return rc;
    const Am16Params<float> p = {q, k, v, o, B, H, T, S, scale * LOG2E};
    am16_head_dim<8, 16, 40, 64, 80, 160>(D, [&](auto d) { am16f_launch<decltype(d)::value>(p, (hipStream_t)stream); });
    return dgq_launch_status("dgq_attention_mfma16_f32");
}
