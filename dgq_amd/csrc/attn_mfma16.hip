// Un-quantised attention on the 16-bit matrix cores (opt-in: the attention modules' attention_mfma16 flag), one launch:
//     o[b,t,h,:] = round_dtype( Σ_j p̂_j·v[b,j,h,:] / l ),   s_j = fp32(Σ_d q_d·k_{j,d})·scale,   p_j = exp(s_j − m),   l = Σ_j p_j
// on fp16 / bf16 tensors in the projection layout (q [B][T][H·D], k / v [B][S][H·D], o [B][T][H·D]).  The 16-bit products are exact in
// fp32 and both products accumulate in fp32 (V_MFMA_F32_32X32X16_BF16 / _F16).  Online softmax over stages of 64 keys (two 32-key score
// tiles; 32 keys at D = 160, where two 64-key stages do not fit the static LDS): running maximum m, rescale of l and of the accumulator
// when m moves (skipped for a stage in which no query of the wave moved its maximum: the factor is exactly 1 then).  p_j is rounded to the tensors' dtype (round to nearest even) for the P·V product ONLY: l sums the UNROUNDED
// fp32 p_j, so the normaliser adds no rounding of its own.  The exponential runs in base 2 (v_exp_f32 on s·scale·log2 e).
// No quantiser, so no global δ: no statistics pass, no workspace, no merge — nothing is exchanged between workgroups.
//
// Orientation as in attn_bf16x3.hip: the score tile is transposed (Sᵀ = K·Qᵀ: key on the register, query on the lane), so a query's
// statistics live in the lane pair (l, l ^ 32) and the tile's accumulator registers, converted pairwise to 16 bits, are directly the
// B operand of Oᵀ = Vᵀ·P̂ᵀ in the permuted k order key_of(r, h) (attn_bf16x3_dev.h).  V is therefore staged TRANSPOSED with the keys
// of a 32-key tile in that order: key 16s + 8a + 4h + b sits in slot 16s + 8h + 4a + b of its Vᵀ row.
//
// 256 threads = four waves x 32 query rows share the K / Vᵀ tiles of one (batch, head) through a double-buffered LDS: the global
// loads of stage t+1 are issued before stage t is multiplied and written to the other buffer after it, one barrier per stage.
// Ragged edges by construction: every global load is clamped in bounds (key min(j, S−1), query min(t, T−1)); keys j >= S get score
// −inf, so p = 0 exactly (every stage the loop visits holds at least one real key, so m is finite from the first stage on and no
// (−inf) − (−inf) is formed); query rows t >= T are computed on the clamped row and not stored.  The head dim is zero padded to the
// MFMA's K granularity (8 -> 16, 40 -> 48) by LDS columns / Vᵀ rows that are cleared once and never written.
#include <stdlib.h>
#include "attn_bf16x3_dev.h"

typedef _Float16 am16_f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 am16_bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 am16_f16x2 __attribute__((ext_vector_type(2)));

struct Am16Params {
    const uint16_t* q;
    const uint16_t* k;
    const uint16_t* v;
    uint16_t* o;
    int B, H, T, S;
    float scale2;            // scale · log2 e
};

template <int D, int NKT> struct Am16Geo {
    static constexpr int KTW = KT * NKT;              // keys per stage: NKT score tiles of 32 keys
    static constexpr int DP = (D + 15) / 16 * 16;     // depth of the score product
    static constexpr int NKK = DP / 16;
    static constexpr int NDT = (D + 31) / 32;         // 32-row d tiles of Oᵀ
    static constexpr int DV = NDT * 32;
    static constexpr int KLD = DP + 8;                // elements per K row (16-byte aligned rows, de-conflicted)
    static constexpr int VLD = KTW + 8;               // elements per Vᵀ row
    static constexpr int CK = D / 8;                  // 16-byte chunks of one key's head slice
    static constexpr int K_TASKS = KTW * CK;          // staging: (key row, chunk) -> one 16-byte LDS write
    static constexpr int V_TASKS = (KTW / 2) * CK;    // staging: (key pair, chunk) -> eight 4-byte LDS writes of Vᵀ
    static constexpr int KU = (K_TASKS + 255) / 256;
    static constexpr int VU = (V_TASKS + 255) / 256;
    static constexpr int K_ELEMS = KTW * KLD;
    static constexpr int V_ELEMS = DV * VLD;
    static_assert(2 * 2 * (K_ELEMS + V_ELEMS) <= 65536, "static LDS");
};

template <bool F16> __device__ __forceinline__ uint32_t am16_pack(float a, float b) {
    if constexpr (F16) return __builtin_bit_cast(uint32_t, __builtin_convertvector(f2{a, b}, am16_f16x2));
    else return __builtin_bit_cast(uint32_t, __builtin_convertvector(f2{a, b}, am16_bf16x2));
}

template <bool F16> __device__ __forceinline__ v16f am16_mfma(const uint4& a, const uint4& b, v16f c) {
    if constexpr (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(am16_f16x8, a), __builtin_bit_cast(am16_f16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

template <int D, int NKT, bool F16>
__global__ __launch_bounds__(256) void am16_kernel(Am16Params p) {
    using G = Am16Geo<D, NKT>;
    __shared__ __attribute__((aligned(16))) uint16_t lds[2 * (G::K_ELEMS + G::V_ELEMS)];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, h32 = lane >> 5, l31 = lane & 31;
    int bx, bh;
    attn_block_coords(1, bx, bh);
    const int b = bh / p.H, hd = bh - b * p.H;
    const int64_t HD = (int64_t)p.H * D;
    const uint16_t* kbase = p.k + (int64_t)b * p.S * HD + hd * D;
    const uint16_t* vbase = p.v + (int64_t)b * p.S * HD + hd * D;

    // ---- clear both stages once: the padding columns of K and the rows d >= D of Vᵀ are never written again
    for (int i = tid; i < (int)(sizeof(lds) / 16); i += 256) reinterpret_cast<uint4*>(lds)[i] = make_uint4(0u, 0u, 0u, 0u);

    // ---- this lane's query as B-operand fragments: element j of qf[kk] = q[t][16kk + 8h + j]
    const int t = bx * 128 + wid * 32 + l31;
    const uint16_t* qrow = p.q + ((int64_t)b * p.T + min(t, p.T - 1)) * HD + hd * D;
    uint4 qf[G::NKK];
#pragma unroll
    for (int kk = 0; kk < G::NKK; ++kk) {
        const int d0 = 16 * kk + 8 * h32;              // D % 8 == 0: the eight elements are all inside D or all padding
        qf[kk] = make_uint4(0u, 0u, 0u, 0u);
        if (d0 < D) qf[kk] = *reinterpret_cast<const uint4*>(qrow + d0);
    }

    // ---- staging roles.  K: task i = (key row i / CK, chunk i % CK).  V: task i = (chunk, key pair), pairs fastest: keys 2·pair and
    // 2·pair + 1 are neighbours in the permuted slot order too, so one 4-byte write per head-dim element places both
    v4i kr[G::KU], va[G::VU], vb[G::VU];            // (native vectors: an array of HIP's uint4 struct stayed in scratch)
    auto load_tile = [&](int s0) {
#pragma unroll
        for (int u = 0; u < G::KU; ++u) {
            const int i = min(tid + 256 * u, G::K_TASKS - 1);
            const int r = i / G::CK, c = i - r * G::CK;
            kr[u] = *reinterpret_cast<const v4i*>(kbase + (int64_t)min(s0 + r, p.S - 1) * HD + 8 * c);
        }
#pragma unroll
        for (int u = 0; u < G::VU; ++u) {
            const int i = min(tid + 256 * u, G::V_TASKS - 1);
            const int c = i / (G::KTW / 2), key = s0 + 2 * (i - c * (G::KTW / 2));
            va[u] = *reinterpret_cast<const v4i*>(vbase + (int64_t)min(key, p.S - 1) * HD + 8 * c);
            vb[u] = *reinterpret_cast<const v4i*>(vbase + (int64_t)min(key + 1, p.S - 1) * HD + 8 * c);
        }
    };
    auto store_tile = [&](int buf) {
        uint16_t* ks = lds + buf * (G::K_ELEMS + G::V_ELEMS);
        uint16_t* vs = ks + G::K_ELEMS;
#pragma unroll
        for (int u = 0; u < G::KU; ++u) {
            const int i = tid + 256 * u;
            if (i < G::K_TASKS) {
                const int r = i / G::CK, c = i - r * G::CK;
                *reinterpret_cast<v4i*>(ks + r * G::KLD + 8 * c) = kr[u];
            }
        }
#pragma unroll
        for (int u = 0; u < G::VU; ++u) {
            const int i = tid + 256 * u;
            if (i < G::V_TASKS) {
                const int c = i / (G::KTW / 2), key = 2 * (i - c * (G::KTW / 2));
                const int slot = (key & ~15) + 8 * ((key >> 2) & 1) + 4 * ((key >> 3) & 1) + (key & 3);     // key 16s+8a+4h+b -> 16s+8h+4a+b
                const uint32_t a4[4] = {(uint32_t)va[u].x, (uint32_t)va[u].y, (uint32_t)va[u].z, (uint32_t)va[u].w};
                const uint32_t b4[4] = {(uint32_t)vb[u].x, (uint32_t)vb[u].y, (uint32_t)vb[u].z, (uint32_t)vb[u].w};
                uint16_t* dst = vs + (8 * c) * G::VLD + slot;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    *reinterpret_cast<uint32_t*>(dst + (2 * e) * G::VLD) = (a4[e] & 0xFFFFu) | (b4[e] << 16);
                    *reinterpret_cast<uint32_t*>(dst + (2 * e + 1) * G::VLD) = (a4[e] >> 16) | (b4[e] & 0xFFFF0000u);
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
        const uint16_t* ks = lds + (it & 1) * (G::K_ELEMS + G::V_ELEMS);
        const uint16_t* vs = ks + G::K_ELEMS;

        // ---- Sᵀ tiles: sc[j][r] = Σ_d k[s0 + 32j + key_of(r, h)][d]·q[t][d]  (NKT independent accumulator chains)
        v16f sc[NKT];
#pragma unroll
        for (int j = 0; j < NKT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) sc[j][r] = 0.0f;
        const uint16_t* kp = ks + l31 * G::KLD + 8 * h32;
#pragma unroll
        for (int kk = 0; kk < G::NKK; ++kk)
#pragma unroll
            for (int j = 0; j < NKT; ++j)
                sc[j] = am16_mfma<F16>(*reinterpret_cast<const uint4*>(kp + (32 * j) * G::KLD + 16 * kk), qf[kk], sc[j]);

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
        uint32_t pw[NKT][8];
#pragma unroll
        for (int j = 0; j < NKT; ++j)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const float p0 = __builtin_amdgcn_exp2f(x[j][r] - m), p1 = __builtin_amdgcn_exp2f(x[j][r + 1] - m);
                l += p0;
                l += p1;
                pw[j][r >> 1] = am16_pack<F16>(p0, p1);
            }

        // ---- Oᵀ += Vᵀ·P̂ᵀ: registers 8s .. 8s+7 of score tile j are the B fragment of k-step 2j + s
        const uint16_t* vp = vs + l31 * G::VLD + 8 * h32;
#pragma unroll
        for (int j = 0; j < NKT; ++j) {
            const uint4 pb0 = make_uint4(pw[j][0], pw[j][1], pw[j][2], pw[j][3]), pb1 = make_uint4(pw[j][4], pw[j][5], pw[j][6], pw[j][7]);
#pragma unroll
            for (int dt = 0; dt < G::NDT; ++dt) {
                acc[dt] = am16_mfma<F16>(*reinterpret_cast<const uint4*>(vp + (32 * dt) * G::VLD + 32 * j), pb0, acc[dt]);
                acc[dt] = am16_mfma<F16>(*reinterpret_cast<const uint4*>(vp + (32 * dt) * G::VLD + 32 * j + 16), pb1, acc[dt]);
            }
        }

        if (it + 1 < NT) store_tile((it + 1) & 1);
        __syncthreads();
    }

    // ---- epilogue: o[t][32dt + 8g + 4h + 0..3] = acc[dt][4g + 0..3] / l, one 8-byte store
    l += __shfl_xor(l, 32, 64);
    if (t >= p.T) return;
    const float inv = 1.0f / l;
    uint16_t* orow = p.o + ((int64_t)b * p.T + t) * HD + hd * D;
#pragma unroll
    for (int dt = 0; dt < G::NDT; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int d = 32 * dt + 8 * g + 4 * h32;
            if (d < D)
                *reinterpret_cast<uint2*>(orow + d) = make_uint2(am16_pack<F16>(acc[dt][4 * g] * inv, acc[dt][4 * g + 1] * inv),
                                                                 am16_pack<F16>(acc[dt][4 * g + 2] * inv, acc[dt][4 * g + 3] * inv));
        }
}

template <int D, int NKT>
static void am16_launch_form(const Am16Params& p, int dtype, hipStream_t st) {
    const dim3 grid((p.T + 127) / 128, p.B * p.H);
    if (dtype == DGQ_F16) hipLaunchKernelGGL((am16_kernel<D, NKT, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((am16_kernel<D, NKT, false>), grid, dim3(256), 0, st, p);
}

// Keys per stage: 64 (two score tiles per barrier, two independent MFMA chains, one maximum and one rescale for both) wherever two
// stages of it fit the static LDS, 32 at D = 160.  DGQ_ATTN16_KT = 32 in the environment (read per call) forces the 32-key form:
// tools/bench_attention_mfma16.py measures the two against each other; no product path sets it.
template <int D>
static void am16_launch(const Am16Params& p, int dtype, hipStream_t st) {
    if constexpr (D <= 80) {
        const char* e = getenv("DGQ_ATTN16_KT");
        if (!(e && atoi(e) == 32)) return am16_launch_form<D, 2>(p, dtype, st);
    }
    am16_launch_form<D, 1>(p, dtype, st);
}

extern "C" int dgq_attention_mfma16(const void* q, const void* k, const void* v, void* o, int dtype, int B, int H, int T, int S, int D,
                                    float scale, void* stream) {
    DGQ_CHECK_ARG(q && k && v && o, "dgq_attention_mfma16: null pointer");
    DGQ_CHECK_ARG(B > 0 && H > 0 && T > 0 && S > 0, "dgq_attention_mfma16: bad geometry (B=%d H=%d T=%d S=%d)", B, H, T, S);
    DGQ_CHECK_ARG(D == 8 || D == 16 || D == 40 || D == 64 || D == 80 || D == 160, "dgq_attention_mfma16: head_dim D=%d (8, 16, 40, 64, 80, 160)", D);
    if (dtype == DGQ_F32) {
        dgq_set_error("dgq_attention_mfma16: fp32 tensors stay on dgq_attention (mode 0: the exact fp32 MFMA)");
        return DGQ_EUNSUPPORTED;
    }
    DGQ_CHECK_ARG(dtype == DGQ_F16 || dtype == DGQ_BF16, "dgq_attention_mfma16: unknown dtype %d", dtype);
    DGQ_CHECK_ARG((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) & 15) == 0, "dgq_attention_mfma16: q, k, v, o must be 16-byte aligned");
    DGQ_CHECK_ARG((int64_t)B * H <= 65535, "dgq_attention_mfma16: B·H=%lld exceeds the grid", (long long)B * H);
    Am16Params p;
    p.q = reinterpret_cast<const uint16_t*>(q); p.k = reinterpret_cast<const uint16_t*>(k); p.v = reinterpret_cast<const uint16_t*>(v);
    p.o = reinterpret_cast<uint16_t*>(o);
    p.B = B; p.H = H; p.T = T; p.S = S;
    p.scale2 = scale * LOG2E;
    hipStream_t st = (hipStream_t)stream;
    switch (D) {
        case 8: am16_launch<8>(p, dtype, st); break;
        case 16: am16_launch<16>(p, dtype, st); break;
        case 40: am16_launch<40>(p, dtype, st); break;
        case 64: am16_launch<64>(p, dtype, st); break;
        case 80: am16_launch<80>(p, dtype, st); break;
        default: am16_launch<160>(p, dtype, st); break;
    }
    return dgq_launch_status("dgq_attention_mfma16");
}
