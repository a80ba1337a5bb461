// gemm_mx_split.hip — the second launch of a K-split GEMM of the real-time block family (dgq_gemm_mx6_splitk, dgq_gemm_mxint8_splitk, ...;
// dgq_gemm_blockq_splitk with the int format's zero-point term) and the plans that decide when to split.  The long-K low-M convolutions of the 8x8 / 16x16 UNet levels (M = 128 .. 512, K = 11 520 .. 23 040) are
// 40 .. 160 tiles on 256 CUs, each a serial walk of 45 .. 90 K tiles; split S ways they are S times the workgroups, each with 1/S of
// the walk, and leave 2S partial accumulators per output tile in the caller's workspace (gemm_block.h: the layout and the split
// kernels' store).
//
// The combine is ONE kernel for both formats — a partial is an fp32 MFMA accumulator whatever fed it.  Grid = the tile grid, 512
// threads in the family's roles: wave w of a tile reads ITS OWN partials, [s][tile][w][reg / 4][lane] as float4 — per register quad
// one coalesced 1 KiB row per split, the S loads of a quad batched before the adds (splitk_sum, gemm_tile.h) — and adds them in split
// order into the very registers the un-split kernel would hold behind its K loop.  Then the un-split tail runs unchanged: the epilogue
// vectors and block_store (the K waves meet in the LDS transposition, k = 0 first).  So every epilogue form — residual / res_div, fused
// quantiser, GEGLU pairs, GroupNorm partials, y2 / ldy2, 16-bit outputs — serves split launches with no code of its own, and the sum has
// ONE order (s ascending inside a K wave, then K wave 0 + K wave 1): deterministic, independent of scheduling, and equal to the un-split
// result wherever fp32 addition is exact.  The kernel boundary is the only exchange: no counter, no spin, no atomics.
#include "gemm_block.h"

DGQ_DIAG_BUFFER(mx_split)

namespace {

// ZeroPoint (gemm_blockq.hip: the epilogue is ga + al·(accf − zw[n]·R[m])): thread tid < 64 forms R of row m0 + tid over the in-image taps
// of the gather and reads zw of column n0 + tid, exactly as the un-split kernel does in front of its K loop; the term is applied once, in
// the epilogue, to the summed accumulator.  Without (the MX formats) q is not read: R = 0, zw = 0.
template <typename TOut, bool ZeroPoint>
__device__ __forceinline__ void block_combine_tile(const GemmParams& p, const BlockSplit& z, int splits, const BlockGather& q) {
    __shared__ __attribute__((aligned(16))) uint8_t smem[BLK_EP + BLK_VEC];
    DGQ_DIAG_DECL
    DGQ_STAMP(0); DGQ_STAMP_REAL(1); DGQ_STAMP_WHERE(2);
    float* vtab = reinterpret_cast<float*>(smem + BLK_EP);
    const BlockRoles r = block_roles();
    if (r.tid < BLK_BM) {
        const int n = min(r.n0 + r.tid, p.N - 1);
        if constexpr (ZeroPoint) {
            const BlockRow row = block_row(q, min(r.m0 + r.tid, p.M - 1));
            block_vectors(vtab, vtab + 3 * BLK_BM, r.tid, p, n, block_rowsum_taps(q, row, p.rowsum), p.zw[n]);
        } else {
            block_vectors(vtab, vtab + 3 * BLK_BM, r.tid, p, n, 0.0f, 0.0f);
        }
    }
    const float* part = reinterpret_cast<const float*>(z.slab + block_partial_at(r, 0));
    const int64_t stride = (int64_t)gridDim.x * gridDim.y * BLK_PART4 * 4;      // floats between the splits of one tile
    v16f accf[1][1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        splitk_sum(part + 64 * 4 * j, stride, splits, a);
#pragma unroll
        for (int k = 0; k < 4; ++k) accf[0][0][4 * j + k] = a[k];
    }
    block_store<TOut, BLK_EP>(p, smem, r, 0, accf DGQ_DIAG_ARG);                 // (nkt = 0: its barrier publishes vtab / vcol)
    DGQ_DIAG_FLUSH(mx_split, BLK_NW, r.wid, r.lane);
}

template <typename TOut>
__global__ __launch_bounds__(BLK_NT) void block_combine_kernel(GemmParams p, BlockSplit z, int splits) {
    block_combine_tile<TOut, false>(p, z, splits, BlockGather{});
}
template <typename TOut>
__global__ __launch_bounds__(BLK_NT) void block_combine_zp_kernel(GemmParams p, BlockSplit z, int splits, BlockGather q) {
    block_combine_tile<TOut, true>(p, z, splits, q);
}

// ---- the plan, from the forced-S sweep of profiles/r23_mx_ksplit.txt (both formats agree):
//  * the pair of launches beats the un-split one once a split keeps about a dozen K tiles: S = nkt / 11 took the best or second-best column
//    of every row with nkt >= 23 (23 -> 2, 45 -> 4, 68 -> 6, 90 -> 8; 13 % .. 70 % off), while nkt <= 12 lost at every S on 160 .. 640 tiles;
//  * grids of up to 1280 workgroups were measured to gain (320 tiles x 4, 160 x 8) and nothing beyond: tiles·S <= 1280, which also bounds
//    the workspace at 40 MiB;
//  * a problem of ONE tile leaves 255 CUs idle and gained from 2 K tiles per split at nkt = 9 (19 % / 35 % off).  Four tiles gained alike,
//    but stay un-split: the layers of the miniature UNet are pinned to one launch, and no SD / SDXL layer has so few tiles.
constexpr int MXS_MAX = 16;              // cap
constexpr int MXS_TARGET = 1280;         // workgroups the split may fill (tiles·S <= target)
constexpr int MXS_MIN_TPS = 11;          // fewest K tiles a split is worth a second launch for
constexpr int MXS_ONE_TILE_TPS = 2, MXS_ONE_TILE_NKT = 8;    // ... of a one-tile problem with at least that many K tiles

// ---- the int block format's own plan (gemm_blockq.hip), the same shape with constants read off the forced-S sweep of its own kernel
// (profiles/r27_block_ksplit.txt; its K tile carries 48 VALU per MFMA behind 8 LDS table reads and costs several MX tiles; W4 and W8 agree):
//  * every shape with nkt <= 12 lost or was level at every S (160 and 640 tiles at nkt = 12: 7 % .. 34 % slower), nkt = 23 gained from S = 2
//    on: at least 8 K tiles per split keeps every nkt < 16 on one launch and gave 23 -> 2 (3 % off), 45 -> 4 / 5 (25 % .. 30 %), 90 -> 10 (74 %);
//  * the grids that gained most are 1280 workgroups (320 tiles x 4, 160 x 8) and 640 (40 x 16): the MX target and cap carry over;
//  * no one-tile rule: every problem of few tiles and fewer than 16 K tiles stays one launch (the miniature UNet, the shapes of the tests).
constexpr int BQS_MAX = 16;
constexpr int BQS_TARGET = 1280;
constexpr int BQS_MIN_TPS = 8;

// the plan's shape: S <= cap, tiles·S <= target, at least min_tps K tiles per split, what the workspace holds, no empty split
int split_plan(int M, int N, int nkt, size_t workspace_bytes, int cap, int target, int min_tps) {
    const int64_t tiles = (int64_t)((M + BLK_BM - 1) / BLK_BM) * ((N + BLK_BN - 1) / BLK_BN);
    int64_t s = target / tiles;
    if (s > nkt / min_tps) s = nkt / min_tps;
    if (s > cap) s = cap;
    const int64_t fit = (int64_t)(workspace_bytes / ((size_t)tiles * BLK_PART_BYTES));
    if (s > fit) s = fit;
    if (s <= 1) return 1;
    const int tps = (nkt + (int)s - 1) / (int)s;
    return (nkt + tps - 1) / tps;                       // no empty split
}

}  // namespace

int block_split_plan(int M, int N, int nkt, size_t workspace_bytes) {
    const bool one_tile = M <= BLK_BM && N <= BLK_BN && nkt >= MXS_ONE_TILE_NKT;
    return split_plan(M, N, nkt, workspace_bytes, MXS_MAX, MXS_TARGET, one_tile ? MXS_ONE_TILE_TPS : MXS_MIN_TPS);
}

int blockq_split_plan(int M, int N, int nkt, int w_bits, size_t workspace_bytes) {
    (void)w_bits;                                       // W4 and W8 agree in the sweep (profiles/r27_block_ksplit.txt)
    return split_plan(M, N, nkt, workspace_bytes, BQS_MAX, BQS_TARGET, BQS_MIN_TPS);
}

int block_combine_launch(const char* who, const GemmParams& p, const BlockSplit& z, int splits, int y_dtype, hipStream_t st, const BlockGather* zp) {
    const dim3 grid((p.N + BLK_BN - 1) / BLK_BN, (p.M + BLK_BM - 1) / BLK_BM), block(BLK_NT);
    if (zp) {
        switch (y_dtype) {
            case DGQ_F32: hipLaunchKernelGGL(block_combine_zp_kernel<float>, grid, block, 0, st, p, z, splits, *zp); break;
            case DGQ_F16: hipLaunchKernelGGL(block_combine_zp_kernel<__half>, grid, block, 0, st, p, z, splits, *zp); break;
            case DGQ_BF16: hipLaunchKernelGGL(block_combine_zp_kernel<__hip_bfloat16>, grid, block, 0, st, p, z, splits, *zp); break;
            default: dgq_set_error("%s: unknown y dtype %d", who, y_dtype); return DGQ_EINVAL;
        }
        return dgq_launch_status(who);
    }
    switch (y_dtype) {
        case DGQ_F32: hipLaunchKernelGGL(block_combine_kernel<float>, grid, block, 0, st, p, z, splits); break;
        case DGQ_F16: hipLaunchKernelGGL(block_combine_kernel<__half>, grid, block, 0, st, p, z, splits); break;
        case DGQ_BF16: hipLaunchKernelGGL(block_combine_kernel<__hip_bfloat16>, grid, block, 0, st, p, z, splits); break;
        default: dgq_set_error("%s: unknown y dtype %d", who, y_dtype); return DGQ_EINVAL;
    }
    return dgq_launch_status(who);
}

static int mx_ktiles(int Kp) { return (Kp / DGQ_KCHUNK + BLK_CH - 1) / BLK_CH; }

extern "C" int dgq_gemm_mx_plan_splits(int M, int N, int Kp, size_t workspace_bytes) {
    if (M <= 0 || N <= 0 || Kp <= 0) return 1;
    return block_split_plan(M, N, mx_ktiles(Kp), workspace_bytes);
}

extern "C" size_t dgq_gemm_mx_workspace_bytes(int M, int N, int Kp) {
    if (M <= 0 || N <= 0 || Kp <= 0) return 0;
    const int s = block_split_plan(M, N, mx_ktiles(Kp), (size_t)-1);
    return s > 1 ? (size_t)s * ((M + BLK_BM - 1) / BLK_BM) * ((N + BLK_BN - 1) / BLK_BN) * BLK_PART_BYTES : 0;
}

extern "C" int dgq_gemm_blockq_plan_splits(int M, int N, int Kp, int w_bits, size_t workspace_bytes) {
    if (M <= 0 || N <= 0 || Kp <= 0) return 1;
    return blockq_split_plan(M, N, mx_ktiles(Kp), w_bits, workspace_bytes);
}

extern "C" size_t dgq_gemm_blockq_workspace_bytes(int M, int N, int Kp, int w_bits) {
    if (M <= 0 || N <= 0 || Kp <= 0) return 0;
    const int s = blockq_split_plan(M, N, mx_ktiles(Kp), w_bits, (size_t)-1);
    return s > 1 ? (size_t)s * ((M + BLK_BM - 1) / BLK_BM) * ((N + BLK_BN - 1) / BLK_BN) * BLK_PART_BYTES : 0;
}
