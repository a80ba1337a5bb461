// gemm_mxw8.hip — the W8 layer under the real-time MX activation quantisers (quant_mx6.hip, quant_mxint8.hip; both unchanged) on the
// block-scaled matrix cores.  For an integer zero point d = q − z lies in [−255, 255]; with H = |d| >> 4 and L = |d| & 15,
//   d = sign(d)·(16·H + L) = 32·(±H/2) + 2·(±L/2),
// and ±H/2, ±L/2 are FP6 E2M3 grid values (0 .. 7.5 in steps of 0.5): a W8 weight is TWO FP6 planes (the sign-magnitude split; the
// two's-complement one of the MXINT8 activation codes would need h = −16, h/2 = −8, which E2M3 does not hold).  dgq_pack_w_mx6x2 writes
// them once per layer as [N][Kp/32][48 B]: per 32-block the H plane's 24 bytes, then the L plane's (the statement: quant_layer.py
// mxw8_split + mx6_pack).
//
// One kernel body, templated on the activation planes NA.  NA = 1: MXFP6 codes a (24 B per block), x̂ = a·2^E.  NA = 2: MXINT8 codes
// s = 32·(hi/2) + 2·(lo/2) (48 B per block: hi plane, lo plane), x̂ = s·2^(E−6).  Per chunk pair a lane reads its activation fragment(s)
// and both weight fragments ONCE and issues 2·NA v_mfma_scale_f32_32x32x64_f8f6f4 into the ONE fp32 accumulator of the whole K — no
// zero-point terms, no Vc, no row sums, no per-chunk VALU.  scale_a is the block's own byte E + 127; a product of codes a·w enters as
// a·w·2^E·2^(scale_b − 127), so the weight-side byte carries the constant of its term.  The order inside a chunk pair is fixed,
// smallest scale first:
//   NA = 1   y = Σ 2^E·a·d:        a·(L/2)·2^E·2^1                     L: 128,    then a·(H/2)·2^E·2^5                      H: 132
//   NA = 2   y = Σ 2^(E−6)·s·d:    (lo/2)(L/2)·2^E·2^(1+1−6)        lo·L: 123,    then (hi/2)(L/2)·2^E·2^(5+1−6)        hi·L: 127,
//                                  (lo/2)(H/2)·2^E·2^(1+5−6)        lo·H: 127,    then (hi/2)(H/2)·2^E·2^(5+5−6)        hi·H: 131
// (pinned, with the plane order and the operand maps — gemm_mx6.hip's, per plane — by the one-hot tests of
// tests/test_gpu_realtime_mx_w8.py).  Every product is exact; only the fp32 accumulation rounds.
//
// The gather, tile, roles, set-up, launch, store epilogue and split partials are the block family's (gemm_gather.h, gemm_block.h): 64 x
// 64 per workgroup, 8 waves (2 x 2 x 2), K tiles of 8 chunks, thread (row = tid & 63, chunk = tid >> 6) stages the code bytes, the
// scale byte and the 48 weight bytes of its (row, chunk) with 16-byte loads.
//
// LDS.  At the family's 32 bytes per (row, chunk, plane) NA = 2 would need 32 + 32 + 0.5 KiB and the epilogue vectors: over the static
// 64 KiB.  Chosen: 24-byte plane slots, laid PAIRWISE — the two planes of a (row, chunk) share one 48-byte slot, H | L exactly as in
// HBM.  48 is a multiple of 16, so a lane's two fragments are three aligned 16-byte reads ([H0..15] [H16..23 L0..7] [L8..23]) where two
// 32-byte slots take four (16 + 8 twice), and the stager's three 16-byte loads go to LDS as they came.  Lanes are 12 dwords apart: the
// 16-byte reads of 8 (16) consecutive lanes fall on distinct quads of 32 (64) banks.  The weight image is 24 KiB; the MXINT8 activation
// image is laid the same way (24 KiB, ring 48.5 KiB), the MXFP6 one keeps gemm_mx6.hip's 32-byte slots (16 KiB, ring 40.5 KiB).  The
// 8-chunk tile stays, so the K-tile count, the split partials, the combine kernel and the plan (gemm_mx_split.hip) serve this file
// unchanged, and nothing is launched with dynamic LDS.  Dynamic LDS with 32-byte slots and a 4-chunk tile were not built: the choice
// between the three is unmeasured.  A tap outside the image (and the K padding) stages zero codes under the scale 2^0 and contributes
// exactly 0.  No atomics.  dgq_gemm_mxw8 walks the whole K in one workgroup per tile; dgq_gemm_mxw8_splitk is the family's K split.
#include "gemm_block.h"

DGQ_DIAG_BUFFER(mxw8)

typedef int v8i __attribute__((ext_vector_type(8)));

namespace {

struct MxW8Operand { const uint8_t* scale; int lds; };        // E8M0 byte per (pixel, block)

constexpr int MW8_W = BLK_CH * BLK_BN * 48;                    // [chunk][column][H 24 B | L 24 B]
constexpr int MW8_SC = BLK_CH * BLK_BM;                        // [chunk][row] scale bytes
constexpr int mw8_a_slot(int NA) { return NA == 2 ? 48 : 32; } // [chunk][row][hi 24 B | lo 24 B]  /  [chunk][row][32 B], 24 used
constexpr int mw8_ring(int NA) { return block_ring(BLK_CH * BLK_BM * mw8_a_slot(NA) + MW8_W + MW8_SC); }
static_assert(mw8_ring(2) + BLK_VEC <= 64 * 1024 && mw8_ring(1) + BLK_VEC <= 64 * 1024, "the 8-chunk tile within the static LDS");
// scale_b of (activation plane, weight plane); see above
constexpr int MW8_A6_L = 128, MW8_A6_H = 132;
constexpr int MW8_A8_LO_L = 123, MW8_A8_HI_L = 127, MW8_A8_LO_H = 127, MW8_A8_HI_H = 131;

// the two 24-byte planes of one 48-byte slot as MFMA fragments (first, second)
__device__ __forceinline__ void mw8_planes(const uint8_t* slot, v8i& first, v8i& second) {
    const uint4 x = *reinterpret_cast<const uint4*>(slot);
    const uint4 y = *reinterpret_cast<const uint4*>(slot + 16);
    const uint4 z = *reinterpret_cast<const uint4*>(slot + 32);
    first = v8i{(int)x.x, (int)x.y, (int)x.z, (int)x.w, (int)y.x, (int)y.y, 0, 0};
    second = v8i{(int)y.z, (int)y.w, (int)z.x, (int)z.y, (int)z.z, (int)z.w, 0, 0};
}

// One workgroup's walk: un-split (SPLIT false) the whole K and the store epilogue; split, K tiles [blockIdx.z·z.tps, + z.tps) and the raw
// accumulators into z.slab (gemm_block.h) — the gather, the staging, the LDS images and the MFMA steps are the same text.
template <typename TOut, int NA, bool SPLIT>
__device__ __forceinline__ void gemm_mxw8_tile(const GemmParams& p, const BlockGather& q, const MxW8Operand& o, const BlockSplit& z) {
    constexpr int ASLOT = mw8_a_slot(NA), MW8_A = BLK_CH * BLK_BM * ASLOT, RING = mw8_ring(NA);
    __shared__ __attribute__((aligned(16))) uint8_t smem[RING + BLK_VEC];
    DGQ_DIAG_DECL
    DGQ_STAMP(0); DGQ_STAMP_REAL(1); DGQ_STAMP_WHERE(2);
    uint8_t* a_lds = smem;
    uint8_t* w_lds = smem + MW8_A;
    uint8_t* sc_lds = smem + MW8_A + MW8_W;
    float* vtab = reinterpret_cast<float*>(smem + RING);
    const BlockRoles r = block_roles();

    // ---- the staged (row, chunk) of this thread: output position of the row, weight row of the column
    const BlockRow row = block_row(q, min(r.m0 + r.srow, p.M - 1));
    const int n = min(r.n0 + r.srow, p.N - 1);
    const uint8_t* wrow = p.wpacked + (int64_t)n * q.nchp * 48;
    const int64_t apitch = (int64_t)q.cpb * (24 * NA);      // code bytes per pixel

    // ---- epilogue vectors: no row terms (R = 0), the column constants with zw = 0
    if (!SPLIT && r.tid < BLK_BM) block_vectors(vtab, vtab + 3 * BLK_BM, r.tid, p, n, 0.0f, 0.0f);

    // ---- staging registers of one K tile: 24·NA activation bytes (NA = 1: ra0 and half of ra1), 48 weight bytes, the scale byte
    uint4 ra0, ra1, ra2, rw0, rw1, rw2;
    uint32_t rsc;
    auto load_tile = [&](int kt) {
        const int cc = kt * BLK_CH + r.sch;                 // wave-uniform chunk
        ra0 = ra1 = ra2 = rw0 = rw1 = rw2 = make_uint4(0u, 0u, 0u, 0u);
        rsc = 127u;                                         // zero codes under 2^0: exactly 0
        const BlockChunk x = block_chunk(q, row, cc);
        if (x.in) {
            const uint8_t* src = reinterpret_cast<const uint8_t*>(p.codes) + x.pix * apitch + x.cb * (24 * NA);
            if constexpr (NA == 2) {
                const uint4* s4 = reinterpret_cast<const uint4*>(src);
                ra0 = s4[0]; ra1 = s4[1]; ra2 = s4[2];
            } else {                                        // (24-byte blocks: 8-byte aligned)
                const uint2* s2 = reinterpret_cast<const uint2*>(src);
                const uint2 u0 = s2[0], u1 = s2[1], u2 = s2[2];
                ra0 = make_uint4(u0.x, u0.y, u1.x, u1.y); ra1 = make_uint4(u2.x, u2.y, 0u, 0u);
            }
            rsc = o.scale[x.pix * o.lds + x.cb];
        }
        if (cc < q.nchp) {                                  // the weight image ends at Kp (a multiple of 4 chunks, not of 8)
            const uint4* src = reinterpret_cast<const uint4*>(wrow + cc * 48);
            rw0 = src[0]; rw1 = src[1]; rw2 = src[2];
        }
    };
    auto store_tile = [&]() {
        uint4* da = reinterpret_cast<uint4*>(a_lds + (r.sch * BLK_BM + r.srow) * ASLOT);
        da[0] = ra0; da[1] = ra1;
        if constexpr (NA == 2) da[2] = ra2;
        uint4* dw = reinterpret_cast<uint4*>(w_lds + (r.sch * BLK_BN + r.srow) * 48);
        dw[0] = rw0; dw[1] = rw1; dw[2] = rw2;
        sc_lds[r.sch * BLK_BM + r.srow] = (uint8_t)rsc;
    };

    v16f accf[1][1];
#pragma unroll
    for (int i = 0; i < 16; ++i) accf[0][0][i] = 0.0f;
    const int nkt = (q.nch + BLK_CH - 1) / BLK_CH;
    const int kt0 = SPLIT ? (int)blockIdx.z * z.tps : 0, kt1 = SPLIT ? min(kt0 + z.tps, nkt) : nkt;
    load_tile(kt0);
    for (int kt = kt0; kt < kt1; ++kt) {
        store_tile();
        __syncthreads();
        if (kt + 1 < kt1) load_tile(kt + 1);
#pragma unroll
        for (int ii = 0; ii < BLK_CH / 4; ++ii) {
            const int pr = 2 * ii + r.wave_k;               // this K wave's chunk pairs of the tile
            if (kt * BLK_CH + 2 * pr >= q.nch) break;       // (wave-uniform: both chunks of the pair are K padding)
            const int ci = 2 * pr + r.hh;                   // the lane half's chunk = its K block of the 64-deep step
            const uint8_t* ap = a_lds + (ci * BLK_BM + r.arow) * ASLOT;
            const int sa = sc_lds[ci * BLK_BM + r.arow];
            v8i wh, wl;
            mw8_planes(w_lds + (ci * BLK_BN + r.wcol) * 48, wh, wl);
            if constexpr (NA == 2) {
                v8i ah, al;
                mw8_planes(ap, ah, al);
                accf[0][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(al, wl, accf[0][0], 2, 2, 0, sa, 0, MW8_A8_LO_L);
                accf[0][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(ah, wl, accf[0][0], 2, 2, 0, sa, 0, MW8_A8_HI_L);
                accf[0][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(al, wh, accf[0][0], 2, 2, 0, sa, 0, MW8_A8_LO_H);
                accf[0][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(ah, wh, accf[0][0], 2, 2, 0, sa, 0, MW8_A8_HI_H);
            } else {
                const uint4 a4 = *reinterpret_cast<const uint4*>(ap);
                const uint2 a2 = *reinterpret_cast<const uint2*>(ap + 16);
                const v8i af = {(int)a4.x, (int)a4.y, (int)a4.z, (int)a4.w, (int)a2.x, (int)a2.y, 0, 0};
                accf[0][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af, wl, accf[0][0], 2, 2, 0, sa, 0, MW8_A6_L);
                accf[0][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af, wh, accf[0][0], 2, 2, 0, sa, 0, MW8_A6_H);
            }
        }
        __syncthreads();
    }
    if constexpr (SPLIT) block_store_partial(z, r, accf[0][0]);
    else block_store<TOut, RING>(p, smem, r, nkt, accf DGQ_DIAG_ARG);
    DGQ_DIAG_FLUSH(mxw8, BLK_NW, r.wid, r.lane);
}

template <typename TOut, int NA>
__global__ __launch_bounds__(BLK_NT) void gemm_mxw8_kernel(GemmParams p, BlockGather q, MxW8Operand o) {
    gemm_mxw8_tile<TOut, NA, false>(p, q, o, BlockSplit{});
}
template <int NA>
__global__ __launch_bounds__(BLK_NT) void gemm_mxw8_split_kernel(GemmParams p, BlockGather q, MxW8Operand o, BlockSplit z) {
    gemm_mxw8_tile<float, NA, true>(p, q, o, z);
}

template <int NA>
struct MxW8Kernel {
    template <typename TOut> static constexpr auto fn = gemm_mxw8_kernel<TOut, NA>;
    static constexpr auto split = gemm_mxw8_split_kernel<NA>;
};

// E2M3 magnitude code of a/2 for a = 0 .. 15, each a grid value: 0.5 is the subnormal 4/8; from 1 on, exponent field 1 + floor(log2(a/2))
// and the three bits under a's leading one
__device__ __forceinline__ uint32_t mw8_half_code(uint32_t a) {
    if (a < 2u) return a * 4u;
    const uint32_t e = 31u - (uint32_t)__clz((int)a);       // 1 .. 3
    return (e << 3) | ((a << (3u - e)) & 7u);
}

// one thread per (n, 32-block of the natural K order): 48 bytes = H plane | L plane
__global__ void pack_w_mx6x2_kernel(const uint8_t* __restrict__ codes, const float* __restrict__ zw, int N, int C, int taps, int Kp,
                                    uint32_t* __restrict__ packed) {
    const int nb = Kp / 32;
    const int K = C * taps;
    const int64_t total = (int64_t)N * nb;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int n = (int)(i / nb), blk = (int)(i - (int64_t)n * nb);
        const int z = (int)zw[n];
        uint32_t w[12] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        for (int j = 0; j < 32; ++j) {
            const int kp = blk * 32 + j;
            uint32_t h6 = 0u, l6 = 0u;
            if (kp < K) {
                const int tap = kp / C, c = kp - tap * C;
                const int d = (int)codes[(int64_t)n * K + (int64_t)c * taps + tap] - z;
                const uint32_t a = (uint32_t)(d < 0 ? -d : d), H = a >> 4, L = a & 15u, sign = d < 0 ? 0x20u : 0u;
                h6 = mw8_half_code(H) | (H ? sign : 0u);    // a zero magnitude is stored +0
                l6 = mw8_half_code(L) | (L ? sign : 0u);
            }
            const int bit = 6 * j, at = bit >> 5, sh = bit & 31;
            w[at] |= h6 << sh;
            w[6 + at] |= l6 << sh;
            if (sh > 26) {
                w[at + 1] |= h6 >> (32 - sh);
                w[6 + at + 1] |= l6 >> (32 - sh);
            }
        }
        for (int k = 0; k < 12; ++k) packed[i * 12 + k] = w[k];
    }
}

}  // namespace

extern "C" int dgq_pack_w_mx6x2(const uint8_t* codes, const float* zw, int N, int C, int taps, int Kp, uint8_t* packed, void* stream) {
    DGQ_CHECK_ARG(codes && zw && packed, "dgq_pack_w_mx6x2: null pointer");
    DGQ_CHECK_ARG(N > 0 && C > 0 && taps > 0 && Kp > 0 && Kp % DGQ_KTILE == 0 && (int64_t)C * taps <= Kp,
                  "dgq_pack_w_mx6x2: Kp=%d must be a multiple of %d and >= C*taps", Kp, DGQ_KTILE);
    DGQ_CHECK_ARG((reinterpret_cast<uintptr_t>(packed) & 3) == 0, "dgq_pack_w_mx6x2: packed must be 4-byte aligned");
    int64_t g = ((int64_t)N * (Kp / 32) + 255) / 256;
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL(pack_w_mx6x2_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, codes, zw, N, C, taps, Kp,
                       reinterpret_cast<uint32_t*>(packed));
    return dgq_launch_status("dgq_pack_w_mx6x2");
}

// what both entries do in front of their launch: the family's set-up and this format's operand
static int gemm_mxw8_setup(const char* who, const dgq_gemm_args_t* g, const dgq_gemm_mxw8_t* mx, GemmParams& p, BlockGather& q, MxW8Operand& o) {
    DGQ_CHECK_ARG(g && mx && mx->scale, "%s: null pointer", who);
    const dgq_gemm_mxw8_t& k = *mx;
    DGQ_CHECK_ARG(k.a_format == 6 || k.a_format == 8, "%s: a_format=%d is 6 (MXFP6 codes) or 8 (MXINT8 codes)", who, k.a_format);
    const int rc = block_gemm_setup(who, *g, k.B, k.H, k.W, k.C, k.kh, k.kw, k.stride, k.pad, k.ups, false, p, q);
    if (rc != DGQ_OK) return rc;
    DGQ_CHECK_ARG(k.lds >= q.cpb, "%s: scale pitch %d < %d blocks", who, k.lds, q.cpb);
    o = {k.scale, k.lds};
    return DGQ_OK;
}

extern "C" int dgq_gemm_mxw8(const dgq_gemm_args_t* g, const dgq_gemm_mxw8_t* mx, void* stream) {
    const char* who = "dgq_gemm_mxw8";
    GemmParams p;
    BlockGather q;
    MxW8Operand o;
    const int rc = gemm_mxw8_setup(who, g, mx, p, q, o);
    if (rc != DGQ_OK) return rc;
    return mx->a_format == 8 ? block_gemm_launch<MxW8Kernel<2>>(who, p, q, o, g->y_dtype, (hipStream_t)stream)
                             : block_gemm_launch<MxW8Kernel<1>>(who, p, q, o, g->y_dtype, (hipStream_t)stream);
}

extern "C" int dgq_gemm_mxw8_splitk(const dgq_gemm_args_t* g, const dgq_gemm_mxw8_t* mx, int splits, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "dgq_gemm_mxw8_splitk";
    GemmParams p;
    BlockGather q;
    MxW8Operand o;
    const int rc = gemm_mxw8_setup(who, g, mx, p, q, o);
    if (rc != DGQ_OK) return rc;
    return mx->a_format == 8
               ? block_gemm_launch_split<MxW8Kernel<2>>(who, p, q, o, g->y_dtype, splits, workspace, workspace_bytes, (hipStream_t)stream)
               : block_gemm_launch_split<MxW8Kernel<1>>(who, p, q, o, g->y_dtype, splits, workspace, workspace_bytes, (hipStream_t)stream);
}
