// Un-quantised attention of the fp32 state on the bf16 matrix cores (opt-in: the attention modules' attention_mfma16_fp32 flag), one
// launch, no workspace.  fp32 q [B][T][H·D], k / v [B][S][H·D], fp32 o.  Every fp32 operand enters the matrix cores as the two-term
// bf16 split  hi = bf16_rn(x), lo = bf16_rn(x − hi)  (x − hi is exact in fp32):
//     s_j = scale · fp32( Σ_d q_lo·k_hi + q_hi·k_lo + q_hi·k_hi )          three V_MFMA_F32_32X32X16_BF16 per K step into ONE accumulator,
//     acc += p_lo·v_hi + p_hi·v_lo + p_hi·v_hi,  (p_hi, p_lo) = split(p)    the small terms first; lo·lo (2^-18 relative) is dropped,
//     o = acc / l                                                           an IEEE division: (S·c) / S == c exactly.
// Online softmax in fp32 exactly as am16_kernel (attn_mfma16.hip) runs it: running maximum m in log2 units, p_j = exp2(x_j − m), l sums
// the UNROUNDED p_j, l and the accumulator are rescaled when m moves (skipped for a stage in which no query of the wave moved).
//
// Taken over from attn_mfma16.hip (copied, not shared: that file's kernel stays as it is): the orientation Sᵀ = K·Qᵀ (key on the
// register, query on the lane), the key_of order, Vᵀ staging (key 16s + 8a + 4h + b in slot 16s + 8h + 4a + b of its Vᵀ row), four
// waves x 32 queries per workgroup, one barrier per stage, every global load clamped in bounds, keys >= S at score −inf, rows >= T
// not stored, the head dim zero padded to the MFMA's K granularity by LDS that is cleared once and never written.
//
// K and V are split ONCE per workgroup while the tile is staged: fp32 global load -> registers -> two bf16 LDS planes (hi, lo), so a
// stage is [K hi][K lo][Vᵀ hi][Vᵀ lo] with the pitches of the 16-bit kernel.  Q is split once into registers.  Two planes double the
// LDS image, so the LDS is dynamic (up to 100 352 bytes at D = 80); the form per head dim — keys per stage, one or two buffers — is
// as3_form() below, chosen by measurement.
#include <stdlib.h>
#include "attn_bf16x3_dev.h"

typedef __bf16 as3_bf16x2 __attribute__((ext_vector_type(2)));

struct As3Params {
    const float* q;
    const float* k;
    const float* v;
    float* o;
    int B, H, T, S;
    float scale2;            // scale · log2 e
};

template <int D, int NKT, int NBUF> struct As3Geo {
    static constexpr int KTW = KT * NKT;              // keys per stage: NKT score tiles of 32 keys
    static constexpr int DP = (D + 15) / 16 * 16;     // depth of the score product
    static constexpr int NKK = DP / 16;
    static constexpr int NDT = (D + 31) / 32;         // 32-row d tiles of Oᵀ
    static constexpr int DV = NDT * 32;
    static constexpr int KLD = DP + 8;                // elements per K row (16-byte aligned rows, de-conflicted)
    static constexpr int VLD = KTW + 8;               // elements per Vᵀ row
    static constexpr int CK = D / 8;                  // 8-element (32-byte fp32) chunks of one key's head slice
    static constexpr int K_TASKS = KTW * CK;          // staging: (key row, chunk) -> one 16-byte LDS write per plane
    static constexpr int V_TASKS = (KTW / 2) * CK;    // staging: (key pair, chunk) -> eight 4-byte LDS writes of Vᵀ per plane
    static constexpr int KU = (K_TASKS + 255) / 256;
    static constexpr int VU = (V_TASKS + 255) / 256;
    static constexpr int K_ELEMS = KTW * KLD;         // one plane
    static constexpr int V_ELEMS = DV * VLD;
    static constexpr int STAGE_ELEMS = 2 * (K_ELEMS + V_ELEMS);
    static constexpr int LDS_BYTES = NBUF * STAGE_ELEMS * 2;
    static_assert(LDS_BYTES <= 160 * 1024 && LDS_BYTES % 16 == 0, "LDS");
};

__device__ __forceinline__ uint32_t as3_pack(float a, float b) {
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f2{a, b}, as3_bf16x2));
}

// two values -> the packed hi pair and the packed lo pair (a in the low half)
__device__ __forceinline__ void as3_split2(float a, float b, uint32_t& hi, uint32_t& lo) {
    hi = as3_pack(a, b);
    lo = as3_pack(a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xFFFF0000u));
}

__device__ __forceinline__ void as3_split8(const v4f& a, const v4f& b, v4i& hi, v4i& lo) {
    uint32_t h[4], l[4];
    as3_split2(a.x, a.y, h[0], l[0]);
    as3_split2(a.z, a.w, h[1], l[1]);
    as3_split2(b.x, b.y, h[2], l[2]);
    as3_split2(b.z, b.w, h[3], l[3]);
    hi = v4i{(int)h[0], (int)h[1], (int)h[2], (int)h[3]};
    lo = v4i{(int)l[0], (int)l[1], (int)l[2], (int)l[3]};
}

__device__ __forceinline__ v16f as3_mfma(const v4i& a, const v4i& b, v16f c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

extern __shared__ __attribute__((aligned(16))) uint16_t as3_lds[];

template <int D, int NKT, int NBUF>
__global__ __launch_bounds__(256) void as3_kernel(As3Params p) {
    using G = As3Geo<D, NKT, NBUF>;
    uint16_t* lds = as3_lds;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, h32 = lane >> 5, l31 = lane & 31;
    int bx, bh;
    attn_block_coords(1, bx, bh);
    const int b = bh / p.H, hd = bh - b * p.H;
    const int64_t HD = (int64_t)p.H * D;
    const float* kbase = p.k + (int64_t)b * p.S * HD + hd * D;
    const float* vbase = p.v + (int64_t)b * p.S * HD + hd * D;

    // ---- clear every stage once: the padding columns of K and the rows d >= D of Vᵀ are never written again
    for (int i = tid; i < G::LDS_BYTES / 16; i += 256) reinterpret_cast<v4i*>(lds)[i] = v4i{0, 0, 0, 0};

    // ---- this lane's query as B-operand fragments, split once: element j of qh / ql[kk] = hi / lo of q[t][16kk + 8h + j]
    const int t = bx * 128 + wid * 32 + l31;
    const float* qrow = p.q + ((int64_t)b * p.T + min(t, p.T - 1)) * HD + hd * D;
    v4i qh[G::NKK], ql[G::NKK];
#pragma unroll
    for (int kk = 0; kk < G::NKK; ++kk) {
        const int d0 = 16 * kk + 8 * h32;              // D % 8 == 0: the eight elements are all inside D or all padding
        qh[kk] = ql[kk] = v4i{0, 0, 0, 0};
        if (d0 < D) as3_split8(*reinterpret_cast<const v4f*>(qrow + d0), *reinterpret_cast<const v4f*>(qrow + d0 + 4), qh[kk], ql[kk]);
    }

    // ---- staging roles as in am16_kernel.  K: task i = (key row i / CK, chunk i % CK).  V: task i = (chunk, key pair), pairs fastest:
    // keys 2·pair and 2·pair + 1 are neighbours in the permuted slot order too, so one 4-byte write per head-dim element and plane
    // places both.  The registers hold the fp32 values; they are split when they are written to LDS, behind the stage's products.
    v4f kr[G::KU][2], va[G::VU][2], vb[G::VU][2];
    auto load_tile = [&](int s0) {
#pragma unroll
        for (int u = 0; u < G::KU; ++u) {
            const int i = min(tid + 256 * u, G::K_TASKS - 1);
            const int r = i / G::CK, c = i - r * G::CK;
            const float* src = kbase + (int64_t)min(s0 + r, p.S - 1) * HD + 8 * c;
            kr[u][0] = *reinterpret_cast<const v4f*>(src);
            kr[u][1] = *reinterpret_cast<const v4f*>(src + 4);
        }
#pragma unroll
        for (int u = 0; u < G::VU; ++u) {
            const int i = min(tid + 256 * u, G::V_TASKS - 1);
            const int c = i / (G::KTW / 2), key = s0 + 2 * (i - c * (G::KTW / 2));
            const float* sa = vbase + (int64_t)min(key, p.S - 1) * HD + 8 * c;
            const float* sb = vbase + (int64_t)min(key + 1, p.S - 1) * HD + 8 * c;
            va[u][0] = *reinterpret_cast<const v4f*>(sa);
            va[u][1] = *reinterpret_cast<const v4f*>(sa + 4);
            vb[u][0] = *reinterpret_cast<const v4f*>(sb);
            vb[u][1] = *reinterpret_cast<const v4f*>(sb + 4);
        }
    };
    auto store_tile = [&](int buf) {
        uint16_t* ks = lds + buf * G::STAGE_ELEMS;
        uint16_t* vs = ks + 2 * G::K_ELEMS;
#pragma unroll
        for (int u = 0; u < G::KU; ++u) {
            const int i = tid + 256 * u;
            if (i < G::K_TASKS) {
                const int r = i / G::CK, c = i - r * G::CK;
                v4i hi, lo;
                as3_split8(kr[u][0], kr[u][1], hi, lo);
                *reinterpret_cast<v4i*>(ks + r * G::KLD + 8 * c) = hi;
                *reinterpret_cast<v4i*>(ks + G::K_ELEMS + r * G::KLD + 8 * c) = lo;
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
                    uint32_t hi, lo;                       // (this key | the next key << 16) of head-dim element 8c + e
                    as3_split2(va[u][e >> 2][e & 3], vb[u][e >> 2][e & 3], hi, lo);
                    *reinterpret_cast<uint32_t*>(dst + e * G::VLD) = hi;
                    *reinterpret_cast<uint32_t*>(dst + G::V_ELEMS + e * G::VLD) = lo;
                }
            }
        }
    };

    v16f acc[G::NDT];
#pragma unroll
    for (int dt = 0; dt < G::NDT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[dt][r] = 0.0f;
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
        const uint16_t* vs = ks + 2 * G::K_ELEMS;

        // ---- Sᵀ tiles: sc[j][r] = Σ_d k[s0 + 32j + key_of(r, h)][d]·q[t][d], per K step lo·hi, hi·lo, hi·hi (NKT independent chains)
        v16f sc[NKT];
#pragma unroll
        for (int j = 0; j < NKT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) sc[j][r] = 0.0f;
        const uint16_t* kp = ks + l31 * G::KLD + 8 * h32;
#pragma unroll
        for (int kk = 0; kk < G::NKK; ++kk) {
            v4i kh[NKT], kl[NKT];
#pragma unroll
            for (int j = 0; j < NKT; ++j) {
                kh[j] = *reinterpret_cast<const v4i*>(kp + (32 * j) * G::KLD + 16 * kk);
                kl[j] = *reinterpret_cast<const v4i*>(kp + G::K_ELEMS + (32 * j) * G::KLD + 16 * kk);
            }
#pragma unroll
            for (int j = 0; j < NKT; ++j) sc[j] = as3_mfma(kh[j], ql[kk], sc[j]);
#pragma unroll
            for (int j = 0; j < NKT; ++j) sc[j] = as3_mfma(kl[j], qh[kk], sc[j]);
#pragma unroll
            for (int j = 0; j < NKT; ++j) sc[j] = as3_mfma(kh[j], qh[kk], sc[j]);
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
        uint32_t ph[NKT][8], pl[NKT][8];
#pragma unroll
        for (int j = 0; j < NKT; ++j)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const float p0 = __builtin_amdgcn_exp2f(x[j][r] - m), p1 = __builtin_amdgcn_exp2f(x[j][r + 1] - m);
                l += p0;
                l += p1;
                as3_split2(p0, p1, ph[j][r >> 1], pl[j][r >> 1]);
            }

        // ---- Oᵀ += Vᵀ·Pᵀ: registers 8s .. 8s+7 of score tile j are the B fragment of k-step 2j + s; per k-step lo·hi, hi·lo, hi·hi
        const uint16_t* vp = vs + l31 * G::VLD + 8 * h32;
#pragma unroll
        for (int j = 0; j < NKT; ++j)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const v4i pbh = v4i{(int)ph[j][4 * s], (int)ph[j][4 * s + 1], (int)ph[j][4 * s + 2], (int)ph[j][4 * s + 3]};
                const v4i pbl = v4i{(int)pl[j][4 * s], (int)pl[j][4 * s + 1], (int)pl[j][4 * s + 2], (int)pl[j][4 * s + 3]};
                v4i vh[G::NDT], vl[G::NDT];
#pragma unroll
                for (int dt = 0; dt < G::NDT; ++dt) {
                    vh[dt] = *reinterpret_cast<const v4i*>(vp + (32 * dt) * G::VLD + 32 * j + 16 * s);
                    vl[dt] = *reinterpret_cast<const v4i*>(vp + G::V_ELEMS + (32 * dt) * G::VLD + 32 * j + 16 * s);
                }
#pragma unroll
                for (int dt = 0; dt < G::NDT; ++dt) acc[dt] = as3_mfma(vh[dt], pbl, acc[dt]);
#pragma unroll
                for (int dt = 0; dt < G::NDT; ++dt) acc[dt] = as3_mfma(vl[dt], pbh, acc[dt]);
#pragma unroll
                for (int dt = 0; dt < G::NDT; ++dt) acc[dt] = as3_mfma(vh[dt], pbh, acc[dt]);
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

    // ---- epilogue: o[t][32dt + 8g + 4h + 0..3] = acc[dt][4g + 0..3] / l (IEEE division), one 16-byte store
    l += __shfl_xor(l, 32, 64);
    if (t >= p.T) return;
    float* orow = p.o + ((int64_t)b * p.T + t) * HD + hd * D;
#pragma unroll
    for (int dt = 0; dt < G::NDT; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int d = 32 * dt + 8 * g + 4 * h32;
            if (d < D)
                *reinterpret_cast<v4f*>(orow + d) = v4f{__fdiv_rn(acc[dt][4 * g], l), __fdiv_rn(acc[dt][4 * g + 1], l),
                                                        __fdiv_rn(acc[dt][4 * g + 2], l), __fdiv_rn(acc[dt][4 * g + 3], l)};
        }
}

template <int D, int NKT, int NBUF>
static void as3_launch_form(const As3Params& p, hipStream_t st) {
    using G = As3Geo<D, NKT, NBUF>;
    static std::atomic<bool> attr_set[64];
    dgq_allow_dynamic_lds(attr_set, {{&as3_kernel<D, NKT, NBUF>, G::LDS_BYTES}});
    const dim3 grid((p.T + 127) / 128, p.B * p.H);
    hipLaunchKernelGGL((as3_kernel<D, NKT, NBUF>), grid, dim3(256), G::LDS_BYTES, st, p);
}

// The form per head dim: 0 = 64-key stages, two buffers in dynamic LDS (65 536 … 100 352 bytes); 1 = 32-key stages, two buffers; 2 = the
// widest stage with ONE buffer and a second barrier per stage.  D = 160 has no 64-key form (two planes of one such stage are 89 088
// bytes): a request for form 0 gets form 1 there.  Measured (profiles/r15_attention_mfma16_fp32.txt): below D = 160 form 0 — form 1
// is 10–25 % slower on the 1024- and 4096-key calls and 0.4–1.7 us faster on the 77-key ones, form 2 within ±5 % of form 0 with no
// side ahead on every shape of a head dim; at D = 160 (key ranges of 64–256 in the models served, i.e. 2–8 stages) form 2: 0.4–0.5 us
// faster than form 1 on each of its four shapes — half the LDS to clear, and no second stage in flight to pay for it.
// DGQ_ATTN16F_FORM = 0 / 1 / 2 in the environment (read per call) forces a form: tools/bench_attention_mfma16.py measures them against
// each other; no product path sets it.
template <int D> static constexpr int as3_form() { return D == 160 ? 2 : 0; }

template <int D>
static void as3_launch(const As3Params& p, hipStream_t st) {
    int form = as3_form<D>();
    if (const char* e = getenv("DGQ_ATTN16F_FORM")) {
        const int f = atoi(e);
        if (f >= 0 && f <= 2) form = f;
    }
    if constexpr (D <= 80) {
        if (form == 0) return as3_launch_form<D, 2, 2>(p, st);
        if (form == 2) return as3_launch_form<D, 2, 1>(p, st);
        return as3_launch_form<D, 1, 2>(p, st);
    } else {
        if (form == 2) return as3_launch_form<D, 1, 1>(p, st);
        return as3_launch_form<D, 1, 2>(p, st);
    }
}

extern "C" int dgq_attention_mfma16_f32(const float* q, const float* k, const float* v, float* o, int B, int H, int T, int S, int D, float scale,
                                        void* stream) {
    DGQ_CHECK_ARG(q && k && v && o, "dgq_attention_mfma16_f32: null pointer");
    DGQ_CHECK_ARG(B > 0 && H > 0 && T > 0 && S > 0, "dgq_attention_mfma16_f32: bad geometry (B=%d H=%d T=%d S=%d)", B, H, T, S);
    DGQ_CHECK_ARG(D == 8 || D == 16 || D == 40 || D == 64 || D == 80 || D == 160, "dgq_attention_mfma16_f32: head_dim D=%d (8, 16, 40, 64, 80, 160)", D);
    DGQ_CHECK_ARG((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) & 15) == 0, "dgq_attention_mfma16_f32: q, k, v, o must be 16-byte aligned");
    DGQ_CHECK_ARG((int64_t)B * H <= 65535, "dgq_attention_mfma16_f32: B·H=%lld exceeds the grid", (long long)B * H);
    As3Params p;
    p.q = q; p.k = k; p.v = v; p.o = o;
    p.B = B; p.H = H; p.T = T; p.S = S;
    p.scale2 = scale * LOG2E;
    hipStream_t st = (hipStream_t)stream;
    switch (D) {
        case 8: as3_launch<8>(p, st); break;
        case 16: as3_launch<16>(p, st); break;
        case 40: as3_launch<40>(p, st); break;
        case 64: as3_launch<64>(p, st); break;
        case 80: as3_launch<80>(p, st); break;
        default: as3_launch<160>(p, st); break;
    }
    return dgq_launch_status("dgq_attention_mfma16_f32");
}
