// gemm_mxint8.hip — the W4 layer under the real-time MXINT8 activation quantiser (quant_mxint8.hip) on the block-scaled matrix cores.
// gfx950 has no MXINT8 operand type; an int8 code splits exactly into two FP6 E2M3 terms, s = 16·h + l = 32·(h/2) + 2·(l/2) (h = s >> 4,
// l = s & 15), which the quantiser has already written as two 6-bit planes.  Per chunk pair TWO v_mfma_scale_f32_32x32x64_f8f6f4 against
// the SAME weight fragment and the SAME activation scale byte, lo plane first, into ONE fp32 accumulator for the whole K — the FP8 rate,
// no per-chunk VALU, no table reads, no zero-point terms (against gemm_blockq.hip: cvt + 2 fma per accumulator register and chunk behind
// 8 LDS reads of {δ, β}).
//   y[m,n] = gamma[n] + alpha[n]·Σ_c 2^(E[m,c]−6)·Σ_{k∈c} s[m,k]·(q−z)[n,k]
// B = the weight image of dgq_pack_w_mx6, the E2M3 codes of w6 = (q − z)/2.  With scale_a = the block's byte E + 127 a product of codes
// a·w6 enters as a·w6·2^E·2^(scale_b − 127); the lo term is 2^(E−6)·2·(l/2)·2·w6 = (l/2)·w6·2^(E−4): scale_b = 123; the hi term is
// 2^(E−6)·32·(h/2)·2·w6 = (h/2)·w6·2^E: scale_b = 127.  The factor 16 between the planes is the difference 4 of the two constants (pinned by
// the one-hot tests of tests/test_gpu_realtime_mxint8.py, which also pin the operand maps: gemm_mx6.hip's, per plane).
//
// The gather, tile, roles, set-up, launch and store are the block family's (gemm_gather.h, gemm_block.h): 64 x 64 per workgroup, 8
// waves (2 x 2 x 2), K tiles of 8 chunks — the ring is 48.5 KiB + the epilogue vectors, within the static LDS, so the 8-chunk tile
// stays.  Thread (row = tid & 63, chunk = tid >> 6) stages the 48 code bytes (three 16-byte loads), the scale byte and the 24 weight
// bytes of its (row, chunk).  The LDS image is 64 bytes per activation (row, chunk), each plane on its own 32 bytes (24 used) in a
// plane-major array, so a lane's 16 + 8 byte fragment reads are spaced as gemm_mx6.hip's, and 32 bytes per weight (row, chunk).  A tap
// outside the image (and the K padding) stages zero codes under the scale 2^0 and contributes exactly 0.  No atomics.  dgq_gemm_mxint8
// walks the whole K in one workgroup per tile; dgq_gemm_mxint8_splitk is gemm_mx6.hip's K split on this format's walk (same partial layout,
// same combine kernel and plan: gemm_block.h, gemm_mx_split.hip) for the long-K low-M shapes.
#include "gemm_block.h"

DGQ_DIAG_BUFFER(mxint8)

typedef int v8i __attribute__((ext_vector_type(8)));

namespace {

struct MxInt8Operand { const uint8_t* scale; int lds; };      // E8M0 byte per (pixel, block)

constexpr int MXI_PLANE = BLK_CH * BLK_BM * 32;                // [chunk][row][32 B], 24 used
constexpr int MXI_A = 2 * MXI_PLANE, MXI_W = BLK_CH * BLK_BN * 32;
constexpr int MXI_SC = BLK_CH * BLK_BM;                        // [chunk][row] scale bytes
constexpr int MXI_RING = block_ring(MXI_A + MXI_W + MXI_SC);
static_assert(MXI_RING + BLK_VEC <= 64 * 1024, "the 8-chunk tile within the static LDS");
constexpr int MXI_SB_LO = 123, MXI_SB_HI = 127;                // scale_b of the lo / hi plane (see above)

// One workgroup's walk: un-split (SPLIT false) the whole K and the store epilogue; split, K tiles [blockIdx.z·z.tps, + z.tps) and the raw
// accumulators into z.slab (gemm_block.h) — the gather, the staging, the LDS images and the MFMA steps are the same text.
template <typename TOut, bool SPLIT>
__device__ __forceinline__ void gemm_mxint8_tile(const GemmParams& p, const BlockGather& q, const MxInt8Operand& o, const BlockSplit& z) {
    __shared__ __attribute__((aligned(16))) uint8_t smem[MXI_RING + BLK_VEC];
    DGQ_DIAG_DECL
    DGQ_STAMP(0); DGQ_STAMP_REAL(1); DGQ_STAMP_WHERE(2);
    uint8_t* hi_lds = smem;
    uint8_t* lo_lds = smem + MXI_PLANE;
    uint8_t* w_lds = smem + MXI_A;
    uint8_t* sc_lds = smem + MXI_A + MXI_W;
    float* vtab = reinterpret_cast<float*>(smem + MXI_RING);
    const BlockRoles r = block_roles();

    // ---- the staged (row, chunk) of this thread: output position of the row, weight row of the column
    const BlockRow row = block_row(q, min(r.m0 + r.srow, p.M - 1));
    const int n = min(r.n0 + r.srow, p.N - 1);
    const uint8_t* wrow = p.wpacked + (int64_t)n * q.nchp * 24;
    const int64_t apitch = (int64_t)q.cpb * 48;             // code bytes per pixel

    // ---- epilogue vectors: no row terms (R = 0), the column constants with zw = 0
    if (!SPLIT && r.tid < BLK_BM) block_vectors(vtab, vtab + 3 * BLK_BM, r.tid, p, n, 0.0f, 0.0f);

    // ---- staging registers of one K tile: a block's 48 bytes are hi[0..15] | hi[16..23] lo[0..7] | lo[8..23]
    uint4 ra0, ra1, ra2;
    uint2 rw0, rw1, rw2;
    uint32_t rsc;
    auto load_tile = [&](int kt) {
        const int cc = kt * BLK_CH + r.sch;                 // wave-uniform chunk
        ra0 = ra1 = ra2 = make_uint4(0u, 0u, 0u, 0u);
        rw0 = rw1 = rw2 = make_uint2(0u, 0u);
        rsc = 127u;                                         // zero codes under 2^0: exactly 0
        const BlockChunk x = block_chunk(q, row, cc);
        if (x.in) {
            const uint4* src = reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(p.codes) + x.pix * apitch + x.cb * 48);
            ra0 = src[0]; ra1 = src[1]; ra2 = src[2];
            rsc = o.scale[x.pix * o.lds + x.cb];
        }
        if (cc < q.nchp) {                                  // the weight image ends at Kp (a multiple of 4 chunks, not of 8)
            const uint2* src = reinterpret_cast<const uint2*>(wrow + cc * 24);
            rw0 = src[0]; rw1 = src[1]; rw2 = src[2];
        }
    };
    auto store_tile = [&]() {
        const int at = (r.sch * BLK_BM + r.srow) * 32;
        *reinterpret_cast<uint4*>(hi_lds + at) = ra0;
        *reinterpret_cast<uint2*>(hi_lds + at + 16) = make_uint2(ra1.x, ra1.y);
        *reinterpret_cast<uint4*>(lo_lds + at) = make_uint4(ra1.z, ra1.w, ra2.x, ra2.y);
        *reinterpret_cast<uint2*>(lo_lds + at + 16) = make_uint2(ra2.z, ra2.w);
        uint2* dw = reinterpret_cast<uint2*>(w_lds + (r.sch * BLK_BN + r.srow) * 32);
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
            const int at = (ci * BLK_BM + r.arow) * 32;
            const uint8_t* bp = w_lds + (ci * BLK_BN + r.wcol) * 32;
            const uint4 l4 = *reinterpret_cast<const uint4*>(lo_lds + at);
            const uint2 l2 = *reinterpret_cast<const uint2*>(lo_lds + at + 16);
            const uint4 h4 = *reinterpret_cast<const uint4*>(hi_lds + at);
            const uint2 h2 = *reinterpret_cast<const uint2*>(hi_lds + at + 16);
            const uint4 b4 = *reinterpret_cast<const uint4*>(bp);
            const uint2 b2 = *reinterpret_cast<const uint2*>(bp + 16);
            const int sa = sc_lds[ci * BLK_BM + r.arow];
            const v8i lf = {(int)l4.x, (int)l4.y, (int)l4.z, (int)l4.w, (int)l2.x, (int)l2.y, 0, 0};
            const v8i hf = {(int)h4.x, (int)h4.y, (int)h4.z, (int)h4.w, (int)h2.x, (int)h2.y, 0, 0};
            const v8i bf = {(int)b4.x, (int)b4.y, (int)b4.z, (int)b4.w, (int)b2.x, (int)b2.y, 0, 0};
            accf[0][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(lf, bf, accf[0][0], 2, 2, 0, sa, 0, MXI_SB_LO);
            accf[0][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(hf, bf, accf[0][0], 2, 2, 0, sa, 0, MXI_SB_HI);
        }
        __syncthreads();
    }
    if constexpr (SPLIT) block_store_partial(z, r, accf[0][0]);
    else block_store<TOut, MXI_RING>(p, smem, r, nkt, accf DGQ_DIAG_ARG);
    DGQ_DIAG_FLUSH(mxint8, BLK_NW, r.wid, r.lane);
}

template <typename TOut>
__global__ __launch_bounds__(BLK_NT) void gemm_mxint8_kernel(GemmParams p, BlockGather q, MxInt8Operand o) {
    gemm_mxint8_tile<TOut, false>(p, q, o, BlockSplit{});
}
__global__ __launch_bounds__(BLK_NT) void gemm_mxint8_split_kernel(GemmParams p, BlockGather q, MxInt8Operand o, BlockSplit z) {
    gemm_mxint8_tile<float, true>(p, q, o, z);
}

struct MxInt8Kernel {
    template <typename TOut> static constexpr auto fn = gemm_mxint8_kernel<TOut>;
    static constexpr auto split = gemm_mxint8_split_kernel;
};

}  // namespace

// what both entries do in front of their launch: the family's set-up and this format's operand
static int gemm_mxint8_setup(const char* who, const dgq_gemm_args_t* g, const dgq_gemm_mxint8_t* mx, GemmParams& p, BlockGather& q, MxInt8Operand& o) {
    DGQ_CHECK_ARG(g && mx && mx->scale, "%s: null pointer", who);
    const dgq_gemm_mxint8_t& k = *mx;
    const int rc = block_gemm_setup(who, *g, k.B, k.H, k.W, k.C, k.kh, k.kw, k.stride, k.pad, k.ups, false, p, q);
    if (rc != DGQ_OK) return rc;
    DGQ_CHECK_ARG(k.lds >= q.cpb, "%s: scale pitch %d < %d blocks", who, k.lds, q.cpb);
    o = {k.scale, k.lds};
    return DGQ_OK;
}

extern "C" int dgq_gemm_mxint8(const dgq_gemm_args_t* g, const dgq_gemm_mxint8_t* mx, void* stream) {
    const char* who = "dgq_gemm_mxint8";
    GemmParams p;
    BlockGather q;
    MxInt8Operand o;
    const int rc = gemm_mxint8_setup(who, g, mx, p, q, o);
    if (rc != DGQ_OK) return rc;
    return block_gemm_launch<MxInt8Kernel>(who, p, q, o, g->y_dtype, (hipStream_t)stream);
}

extern "C" int dgq_gemm_mxint8_splitk(const dgq_gemm_args_t* g, const dgq_gemm_mxint8_t* mx, int splits, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "dgq_gemm_mxint8_splitk";
    GemmParams p;
    BlockGather q;
    MxInt8Operand o;
    const int rc = gemm_mxint8_setup(who, g, mx, p, q, o);
    if (rc != DGQ_OK) return rc;
    return block_gemm_launch_split<MxInt8Kernel>(who, p, q, o, g->y_dtype, splits, workspace, workspace_bytes, (hipStream_t)stream);
}
