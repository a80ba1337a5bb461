// What the real-time block GEMMs (gemm_blockq.hip: int8 codes under {δ, β} per block; gemm_mx6.hip: FP6 codes under an E8M0 scale per
// block) share: the tile and its thread / wave roles, the epilogue vectors and the tail around the family's store epilogue, and on the
// host the ONE set-up of a launch (checks, GemmParams, the gather of gemm_gather.h) and the launch by output dtype.  A format supplies
// its staged registers with their load and store, one MFMA step, its LDS image sizes and the checks on its own arguments; its K loop —
// load, store, barrier, next load, steps, barrier — stays written out in its file.
//
// One tile shape: 64 x 64 per workgroup, 8 waves (2 x 2 x 2: the two K waves of a 32x32 MFMA tile meet in the epilogue's LDS
// transposition, k = 0 first — a fixed order), K in tiles of 256 = 8 chunks, one staged chunk per wave: thread (row = tid & 63, chunk =
// tid >> 6) stages the operand pieces of its (row, chunk) — the chunk, hence the tap, is wave-uniform.
#pragma once
#include "gemm_tile.h"
#include "gemm_gather.h"

static_assert(DGQ_KCHUNK == 32, "gemm_gather.h spells the chunk width");
constexpr int BLK_BM = 64, BLK_BN = 64, BLK_NT = 512, BLK_NW = 8;
constexpr int BLK_CH = 8;                                    // chunks per K tile = one staged chunk per wave
static_assert(BLK_CH == BLK_NW, "one staged chunk per wave");
constexpr int BLK_EP = BLK_NW * 32 * (32 + 4) * 4;           // gemm_store_tile's transposition scratch (over the idle operand images)
constexpr int BLK_VEC = (3 * BLK_BM + 4 * BLK_BN) * 4;       // behind the ring: vtab [3][BM] R0 R1 R2 | vcol [4][BN] alpha zw gamma vn
constexpr int block_ring(int images) { return images > BLK_EP ? images : BLK_EP; }

struct BlockRoles {
    int tid, lane, wid;
    int wave_k, wave_m, wave_n;
    int sch, srow;                        // the (chunk of a K tile, row / column of the tile) this thread stages
    int lr, hh;                           // MFMA operand row / column and K half of the lane
    int arow, wcol;                       // ... in the workgroup's tile
    int m0, n0;
};
__device__ __forceinline__ BlockRoles block_roles() {
    BlockRoles r;
    r.tid = threadIdx.x; r.lane = r.tid & 63;
    r.wid = __builtin_amdgcn_readfirstlane(r.tid >> 6);
    r.wave_k = r.wid >> 2; r.wave_m = (r.wid >> 1) & 1; r.wave_n = r.wid & 1;
    r.sch = r.wid; r.srow = r.lane;
    r.lr = r.lane & 31; r.hh = r.lane >> 5;
    r.arow = r.wave_m * 32 + r.lr; r.wcol = r.wave_n * 32 + r.lr;
    r.m0 = blockIdx.y * BLK_BM; r.n0 = blockIdx.x * BLK_BN;
    return r;
}

// epilogue vectors of thread tid < BLK_BM: its row's R (0 without zero-point terms) and its column n's constants
__device__ __forceinline__ void block_vectors(float* vtab, float* vcol, int tid, const GemmParams& p, int n, float R, float zw) {
    vtab[tid] = 1.0f; vtab[BLK_BM + tid] = R; vtab[2 * BLK_BM + tid] = 0.0f;
    vcol[tid] = p.alpha[n]; vcol[BLK_BN + tid] = zw; vcol[2 * BLK_BN + tid] = p.gamma[n]; vcol[3 * BLK_BN + tid] = 0.0f;
}

// Behind the K loop: the barrier that ends the loop has retired every read of the operand images (with no K tile at all nothing was
// staged, and the barrier here publishes vtab / vcol, otherwise written before the loop's first barrier).
template <typename TOut, int RING>
__device__ __forceinline__ void block_store(const GemmParams& p, uint8_t* smem, const BlockRoles& r, int nkt,
                                            const v16f (&accf)[1][1] DGQ_DIAG_PARAM) {
    DGQ_STAMP(6);
    if (nkt == 0) __syncthreads();
    const float* vtab = reinterpret_cast<const float*>(smem + RING);
    v16i acc0[1][1];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc0[0][0][i] = 0;
    gemm_store_tile<false, TOut, BLK_BM, BLK_BN, 2, 2, 2, RING, 1, 1>(p, 0, smem, vtab, vtab + 3 * BLK_BM, r.wid, r.lane, r.wave_m, r.wave_n, r.wave_k,
                                                                      r.m0, r.n0, acc0, accf DGQ_DIAG_ARG);
    DGQ_STAMP(9);
    DGQ_DIAG_DRAIN();
    DGQ_STAMP(10); DGQ_STAMP_REAL(11);
}

// The shared part of a block entry: checks of the problem, the geometry and the extras; GemmParams and the gather.  zero_point: the
// format has zero-point terms (row sums, zw, offset); without, the epilogue runs with R = 0 and zw = 0 and the three are not read.
static inline int block_gemm_setup(const char* who, const dgq_gemm_args_t& a, int B, int H, int W, int C, int kh, int kw, int stride, int pad, int ups,
                                   bool zero_point, GemmParams& p, BlockGather& q) {
    DGQ_CHECK_ARG(a.codes && a.wpacked && a.alpha && a.gamma && a.y && (!zero_point || (a.rowsum && a.zw)), "%s: null pointer", who);
    DGQ_CHECK_ARG(a.M > 0 && a.N > 0 && a.Kp > 0 && a.Kp % DGQ_KTILE == 0, "%s: bad shape M=%d N=%d Kp=%d", who, a.M, a.N, a.Kp);
    DGQ_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && C % DGQ_KCHUNK == 0 && kh > 0 && kw > 0 && stride > 0 && pad >= 0,
                  "%s: bad geometry (C %% 32 == 0)", who);
    DGQ_CHECK_ARG(!ups || (H % 2 == 0 && W % 2 == 0), "%s: ups needs even H, W", who);
    q = block_gather(B, H, W, C, kh, kw, stride, pad, ups ? 1 : 0, a.Kp);
    DGQ_CHECK_ARG(q.Ho > 0 && q.Wo > 0 && (int64_t)B * q.Ho * q.Wo == a.M, "%s: M=%d is not B*Ho*Wo", who, a.M);
    const int64_t K = (int64_t)kh * kw * C;
    DGQ_CHECK_ARG(K <= a.Kp, "%s: Kp=%d < kh*kw*C=%lld", who, a.Kp, (long long)K);
    DGQ_CHECK_ARG((int64_t)B * H * W * C < (1LL << 40), "%s: input too large", who);
    DGQ_CHECK_ARG((reinterpret_cast<uintptr_t>(a.codes) & 15) == 0 && (reinterpret_cast<uintptr_t>(a.wpacked) & 15) == 0,
                  "%s: codes / wpacked must be 16-byte aligned", who);
    DGQ_CHECK_ARG(a.ldy >= (a.extra && a.extra->geglu ? a.N / 2 : a.N), "%s: ldy < output columns", who);
    p = {};
    p.codes = a.codes; p.rowsum = zero_point ? a.rowsum : nullptr; p.rowsum_parts = 1; p.M = a.M; p.Kp = a.Kp; p.N = a.N;
    p.wpacked = reinterpret_cast<const uint8_t*>(a.wpacked);
    p.L = 1; p.offset = zero_point ? a.offset : 0.0f; p.alpha = a.alpha; p.zw = zero_point ? a.zw : nullptr; p.gamma = a.gamma; p.y = a.y; p.ldy = a.ldy;
    p.splits = 1; p.tiles_per_split = a.Kp / BK;
    p.ex.res_div = 1; p.ex.fq_T = 1; p.ex.fq_D = 1; p.ex.fq_qmax = 255.0f;
    if (a.extra) {
        const dgq_gemm_extra_t& e = *a.extra;
        DGQ_CHECK_ARG(!e.conv && !e.act, "%s: no implicit-conv / quantise-on-load descriptor (the gather is this entry's own)", who);
        const int rc = gemm_check_extra(who, a.M, a.N, e);
        if (rc != DGQ_OK) return rc;
        p.ex = e;
        p.ex.conv = nullptr; p.ex.flush_coef = nullptr; p.ex.wfrag = nullptr; p.ex.act = nullptr;
        if (!e.residual) p.ex.res_div = 1;
    }
    return DGQ_OK;
}

// The launch by output dtype.  Kernel: a struct with `template <typename TOut> static constexpr auto fn` = the kernel instance taking
// (GemmParams, BlockGather, Operand).
template <typename Kernel, typename Operand>
static int block_gemm_launch(const char* who, const GemmParams& p, const BlockGather& q, const Operand& o, int y_dtype, hipStream_t st) {
    const dim3 grid((p.N + BLK_BN - 1) / BLK_BN, (p.M + BLK_BM - 1) / BLK_BM), block(BLK_NT);
    switch (y_dtype) {
        case DGQ_F32: hipLaunchKernelGGL((Kernel::template fn<float>), grid, block, 0, st, p, q, o); break;
        case DGQ_F16: hipLaunchKernelGGL((Kernel::template fn<__half>), grid, block, 0, st, p, q, o); break;
        case DGQ_BF16: hipLaunchKernelGGL((Kernel::template fn<__hip_bfloat16>), grid, block, 0, st, p, q, o); break;
        default: dgq_set_error("%s: unknown y dtype %d", who, y_dtype); return DGQ_EINVAL;
    }
    return dgq_launch_status(who);
}
