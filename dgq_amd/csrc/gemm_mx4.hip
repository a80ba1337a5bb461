// gemm_mx4.hip — the W4 layer under the real-time MXFP4 activation quantiser (quant_mx4.hip) on the block-scaled matrix cores: every K
// step is v_mfma_scale_f32_32x32x64_f8f6f4 with the A operand FP4 E2M1 (cbsz = 4) and the B operand FP6 E2M3 (blgp = 2) — the
// instruction takes a format per operand.  W4A4 with the block scale inside the instruction: ONE fp32 accumulator for the whole K, no
// per-chunk VALU, no table reads.
//   y[m,n] = gamma[n] + alpha[n]·Σ_c 2^(E[m,c]+1)·Σ_{k∈c} a4[m,k]·w6[n,k]
// A = the activation codes [pixels][C/32][16 B], scale_a = the lane's own (row, block) byte; B = the weight image of dgq_pack_w_mx6,
// unchanged: the E2M3 codes of (q − z)/2 under the constant block scale 2^1 (byte 128).  Every product a4·w6 is a multiple of 1/4 of at
// most 6·7.5 and exact in fp32; only the accumulation rounds.  No zero-point terms: the epilogue is the family's
// gemm_store_tile<false, ...> with R = 0, zw = 0, gamma = bias, alpha = δw (residual, res_div, GEGLU pairs, GroupNorm partials, y2 / ldy
// redirects and 16-bit outputs are that epilogue's).
//
// Operand maps (pinned by the one-hot tests of tests/test_gpu_realtime_mxfp4.py): lane l holds row / column l & 31 and the K block
// l >> 5 of the 64-deep step.  A: 32 consecutive k as the 128-bit little-endian string of their 4-bit codes in the lane's FIRST FOUR
// registers (element j at bits 4j .. 4j + 3), registers 4 .. 7 zero; B: the 192-bit string of 6-bit codes in the first six, as in
// gemm_mx6.hip; each side's scale in byte 0 of its scale register.
//
// The gather, tile and wave layout are the block family's (gemm_gather.h, gemm_block.h): 64 x 64 per workgroup, 8 waves (2 x 2 x 2),
// K tiles of 8 chunks, thread (row = tid & 63, chunk = tid >> 6) stages its (row, chunk); one MFMA covers the chunk pair (2i, 2i + 1),
// one chunk per lane half.  A tap outside the image (and the K padding) stages zero codes under the scale 2^0 and contributes exactly 0.
//
// Data movement of the A side is this kernel's own.  An FP4 block is 16 bytes: a thread stages ONE uint4 (one 128-bit HBM load, one
// 128-bit LDS write) and a lane's operand is ONE aligned 128-bit LDS read (gemm_mx6: three 8-byte loads, and 16 + 8 bytes read out of a
// 32-byte slot).  The A image is [chunk][row][16 B], 1 KiB per chunk, no padding: lanes 0 .. 31 of a read are 32 consecutive rows of one
// chunk = 512 contiguous bytes, every bank the same number of times in any pass the hardware forms out of consecutive lanes — the
// minimum a 128-bit read can have (gemm_mx6's 32-byte slots put consecutive lanes 32 bytes apart, two lanes per bank in an 8-lane
// pass).  Lanes 32 .. 63 read the next chunk, 1 KiB further: the same banks as lanes 0 .. 31, which costs only if one pass mixes the
// two lane halves; how the hardware forms the passes of a 128-bit read is unmeasured here, and so is a staggered odd chunk.  The
// staging write is the same 512-byte run per half wave.  The weight image keeps the family's 32-byte slots (24 used).
// What the smaller A image frees — 8 KiB of LDS and four staging registers — is left free: the workgroup's LDS is set by the
// epilogue's transposition scratch (BLK_EP, 36 KiB), which the operand images (8 + 16 KiB) sit under either way, and the tile stays
// the family's 8 chunks (one staged chunk per wave).  A 16-chunk tile and a second workgroup per CU are unmeasured.
// dgq_gemm_mx4 walks the whole K in one workgroup per tile; dgq_gemm_mx4_splitk runs the same walk over 1/S of the K tiles per
// workgroup (blockIdx.z = split) and leaves raw accumulators for the family's combine launch (gemm_block.h, gemm_mx_split.hip).
#include "gemm_block.h"

DGQ_DIAG_BUFFER(mx4)

typedef int v8i __attribute__((ext_vector_type(8)));

namespace {

struct Mx4Operand { const uint8_t* scale; int lds; };         // E8M0 byte per (pixel, block)

constexpr int MX4_A = BLK_CH * BLK_BM * 16;                   // [chunk][row][16 B]
constexpr int MX4_W = BLK_CH * BLK_BN * 32;                   // [chunk][column][32 B], 24 used
constexpr int MX4_SC = BLK_CH * BLK_BM;                       // [chunk][row] scale bytes
constexpr int MX4_RING = block_ring(MX4_A + MX4_W + MX4_SC);

// One workgroup's walk: un-split (SPLIT false) the whole K and the store epilogue; split, K tiles [blockIdx.z·z.tps, + z.tps) and the raw
// accumulators into z.slab (gemm_block.h) — the gather, the staging, the LDS images and the MFMA steps are the same text.
template <typename TOut, bool SPLIT>
__device__ __forceinline__ void gemm_mx4_tile(const GemmParams& p, const BlockGather& q, const Mx4Operand& o, const BlockSplit& z) {
    __shared__ __attribute__((aligned(16))) uint8_t smem[MX4_RING + BLK_VEC];
    DGQ_DIAG_DECL
    DGQ_STAMP(0); DGQ_STAMP_REAL(1); DGQ_STAMP_WHERE(2);
    uint8_t* a_lds = smem;
    uint8_t* w_lds = smem + MX4_A;
    uint8_t* sc_lds = smem + MX4_A + MX4_W;
    float* vtab = reinterpret_cast<float*>(smem + MX4_RING);
    const BlockRoles r = block_roles();

    // ---- the staged (row, chunk) of this thread: output position of the row, weight row of the column
    const BlockRow row = block_row(q, min(r.m0 + r.srow, p.M - 1));
    const int n = min(r.n0 + r.srow, p.N - 1);
    const uint8_t* wrow = p.wpacked + (int64_t)n * q.nchp * 24;
    const int64_t apitch = (int64_t)q.cpb * 16;             // code bytes per pixel

    // ---- epilogue vectors: no row terms (R = 0), the column constants with zw = 0
    if (!SPLIT && r.tid < BLK_BM) block_vectors(vtab, vtab + 3 * BLK_BM, r.tid, p, n, 0.0f, 0.0f);

    // ---- staging registers of one K tile: the whole FP4 block in one
    uint4 ra;
    uint2 rw0, rw1, rw2;
    uint32_t rsc;
    auto load_tile = [&](int kt) {
        const int cc = kt * BLK_CH + r.sch;                 // wave-uniform chunk
        ra = make_uint4(0u, 0u, 0u, 0u);
        rw0 = rw1 = rw2 = make_uint2(0u, 0u);
        rsc = 127u;                                         // zero codes under 2^0: exactly 0
        const BlockChunk x = block_chunk(q, row, cc);
        if (x.in) {
            ra = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(p.codes) + x.pix * apitch + x.cb * 16);
            rsc = o.scale[x.pix * o.lds + x.cb];
        }
        if (cc < q.nchp) {                                  // the weight image ends at Kp (a multiple of 4 chunks, not of 8)
            const uint2* src = reinterpret_cast<const uint2*>(wrow + cc * 24);
            rw0 = src[0]; rw1 = src[1]; rw2 = src[2];
        }
    };
    auto store_tile = [&]() {
        *reinterpret_cast<uint4*>(a_lds + (r.sch * BLK_BM + r.srow) * 16) = ra;
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
            const uint4 a4 = *reinterpret_cast<const uint4*>(a_lds + (ci * BLK_BM + r.arow) * 16);
            const uint8_t* bp = w_lds + (ci * BLK_BN + r.wcol) * 32;
            const uint4 b4 = *reinterpret_cast<const uint4*>(bp);
            const uint2 b2 = *reinterpret_cast<const uint2*>(bp + 16);
            const int sa = sc_lds[ci * BLK_BM + r.arow];
            const v8i af = {(int)a4.x, (int)a4.y, (int)a4.z, (int)a4.w, 0, 0, 0, 0};
            const v8i bf = {(int)b4.x, (int)b4.y, (int)b4.z, (int)b4.w, (int)b2.x, (int)b2.y, 0, 0};
            accf[0][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af, bf, accf[0][0], 4, 2, 0, sa, 0, 128);
        }
        __syncthreads();
    }
    if constexpr (SPLIT) block_store_partial(z, r, accf[0][0]);
    else block_store<TOut, MX4_RING>(p, smem, r, nkt, accf DGQ_DIAG_ARG);
    DGQ_DIAG_FLUSH(mx4, BLK_NW, r.wid, r.lane);
}

template <typename TOut>
__global__ __launch_bounds__(BLK_NT) void gemm_mx4_kernel(GemmParams p, BlockGather q, Mx4Operand o) {
    gemm_mx4_tile<TOut, false>(p, q, o, BlockSplit{});
}
__global__ __launch_bounds__(BLK_NT) void gemm_mx4_split_kernel(GemmParams p, BlockGather q, Mx4Operand o, BlockSplit z) {
    gemm_mx4_tile<float, true>(p, q, o, z);
}

struct Mx4Kernel {
    template <typename TOut> static constexpr auto fn = gemm_mx4_kernel<TOut>;
    static constexpr auto split = gemm_mx4_split_kernel;
};

}  // namespace

// what both entries do in front of their launch: the family's set-up and this format's operand
static int gemm_mx4_setup(const char* who, const dgq_gemm_args_t* g, const dgq_gemm_mx4_t* mx, GemmParams& p, BlockGather& q, Mx4Operand& o) {
    DGQ_CHECK_ARG(g && mx && mx->scale, "%s: null pointer", who);
    const dgq_gemm_mx4_t& k = *mx;
    const int rc = block_gemm_setup(who, *g, k.B, k.H, k.W, k.C, k.kh, k.kw, k.stride, k.pad, k.ups, false, p, q);
    if (rc != DGQ_OK) return rc;
    DGQ_CHECK_ARG(k.lds >= q.cpb, "%s: scale pitch %d < %d blocks", who, k.lds, q.cpb);
    o = {k.scale, k.lds};
    return DGQ_OK;
}

extern "C" int dgq_gemm_mx4(const dgq_gemm_args_t* g, const dgq_gemm_mx4_t* mx, void* stream) {
    const char* who = "dgq_gemm_mx4";
    GemmParams p;
    BlockGather q;
    Mx4Operand o;
    const int rc = gemm_mx4_setup(who, g, mx, p, q, o);
    if (rc != DGQ_OK) return rc;
    return block_gemm_launch<Mx4Kernel>(who, p, q, o, g->y_dtype, (hipStream_t)stream);
}

extern "C" int dgq_gemm_mx4_splitk(const dgq_gemm_args_t* g, const dgq_gemm_mx4_t* mx, int splits, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "dgq_gemm_mx4_splitk";
    GemmParams p;
    BlockGather q;
    Mx4Operand o;
    const int rc = gemm_mx4_setup(who, g, mx, p, q, o);
    if (rc != DGQ_OK) return rc;
    return block_gemm_launch_split<Mx4Kernel>(who, p, q, o, g->y_dtype, splits, workspace, workspace_bytes, (hipStream_t)stream);
}
