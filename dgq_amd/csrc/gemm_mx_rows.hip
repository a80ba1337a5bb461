// gemm_mx_rows.hip — the W4 Linear layer under a real-time MX activation format (MXFP6, MXINT8, MXFP4) in ONE launch: the workgroup
// quantises its own rows into LDS and multiplies them there, so the codes and scale bytes of dgq_quant_act_mx* never reach HBM and
// the quantiser launch in front of dgq_gemm_mx* goes away.  Up to 4 problems that share the input x (the q / k / v projections) run in
// the same launch.  linear_smallm_mx.hip does this for M <= 16 by streaming weights; this is the general-M form, a row-PANEL kernel:
//
//  * A workgroup (512 threads, 8 waves) owns a panel of PR input rows and a contiguous range of column tiles; grid = (column splits,
//    panels).  PR = 64 with 64-column tiles and the family's 2 x 2 x 2 wave roles (gemm_block.h), or — where 64 rows of the format do
//    not fit the LDS beside the epilogue scratch (MXINT8 beyond K = 1152) — PR = 32 with 128-column tiles and 1 x 4 x 2 roles: every
//    wave keeps a 32 x 32 MFMA tile, and the two K waves of an output element are the family's either way.
//  * Phase 1, quantise: a wave takes one row at a time through quant_row_source (LayerNorm statistics, GroupNorm rows) and
//    quant_block_walk (SiLU, GEGLU) and calls the format's block statement (quant_common.h) — the x′, codes and scale bytes of the
//    stand-alone quantisers bit for bit — and writes them into the A image [chunk][row][slot] for the whole K: slot = the HBM block
//    itself, packed (24 B MXFP6, 48 B = hi plane | lo plane MXINT8, 16 B MXFP4), and one E8M0 byte per (chunk, row) behind it.  Rows
//    past M and the chunks K/32 .. Kp/32 − 1 are zero codes under byte 127 and contribute exactly 0.  One __syncthreads().
//  * Phase 2, column tiles: per tile the MX GEMMs' K walk against the resident panel.  Weights are the unchanged dgq_pack_w_mx6 image,
//    staged per K tile of 8 chunks into a ring [chunk][column][32 B] (24 used) with a register prefetch that also runs ahead over the
//    epilogue into the next column tile.  K wave wave_k takes chunk pairs 2·ii + wave_k of each K tile in ascending order; the MFMA
//    steps and scale bytes are gemm_mx6.hip's / gemm_mxint8.hip's (lo under 123, then hi under 127) / gemm_mx4.hip's (cbsz 4, blgp 2).
//    The tile ends in gemm_store_tile<false, ...> with R = 0, zw = 0 and the tile's n0; its transposition scratch lies over the weight
//    ring, never over the panel.  Residual, res_div, GEGLU pairs, y2 / ldy redirects and 16-bit outputs are that function's.
//
// Every output element therefore sees the same codes, the same MFMA sequence (the K partition does not depend on the tile shape) and
// the same epilogue as dgq_quant_act_mx* + dgq_gemm_mx* un-split: the result is bit-identical to the two-launch route on any data.
// Nothing is exchanged between workgroups: no atomics, no counters, capture-safe.  No K split here: layers the MX plan splits keep the
// two-launch route.  LDS = 36 KiB (scratch over the ring) + the epilogue vectors + Kp/32 · PR · (slot + 1), dynamic, up to 160 KiB —
// one workgroup per CU at large K.  A-side reads: three 8-byte (MXFP6), three 16-byte (MXINT8), one 16-byte (MXFP4) per lane and chunk;
// consecutive lanes are consecutive rows, slot bytes apart.  The bank behaviour of the packed slots against padded 32-byte ones is
// unmeasured.
#include "gemm_block.h"
#include "quant_prologue.h"
#include <atomic>

DGQ_DIAG_BUFFER(mx_rows)

typedef int v8i __attribute__((ext_vector_type(8)));

constexpr int ROWS_MAX_PROBLEMS = 4;
constexpr int ROWS_LDS = 160 * 1024;
// the plan aims at this many workgroups (the CUs of an MI355X: at large K one workgroup is resident per CU)
constexpr int ROWS_TARGET_WGS = 256;

namespace {

constexpr int rows_slot(int fmt) { return fmt == 8 ? 48 : (fmt == 6 ? 24 : 16); }

template <int PR>
struct RowsTile {
    static_assert(PR == 64 || PR == 32, "panel rows");
    static constexpr int BM = PR, BN = PR == 64 ? 64 : 128;
    static constexpr int WVM = PR / 32, WVN = 4 / WVM;
    static constexpr int RING = block_ring(BLK_CH * BN * 32);             // weight ring [chunk][column][32 B] under the epilogue scratch
    static constexpr int VEC = (3 * BM + 4 * BN) * 4;                     // vtab [3][BM] | vcol [4][BN]
};
constexpr int rows_bn(int pr) { return pr == 64 ? 64 : 128; }
constexpr int rows_lds_bytes(int fmt, int pr, int nchp) {
    return (pr == 64 ? RowsTile<64>::RING + RowsTile<64>::VEC : RowsTile<32>::RING + RowsTile<32>::VEC) + nchp * pr * (rows_slot(fmt) + 1);
}
// the panel of a (format, padded K): 64 rows where they fit, else 32, else 0
int rows_panel(int fmt, int nchp) {
    if (rows_lds_bytes(fmt, 64, nchp) <= ROWS_LDS) return 64;
    if (rows_lds_bytes(fmt, 32, nchp) <= ROWS_LDS) return 32;
    return 0;
}

struct RowsBatch {
    GemmParams p[ROWS_MAX_PROBLEMS];
    int tile0[ROWS_MAX_PROBLEMS];         // first column tile of each problem in the launch's tile list
    int n;                                // problems
    int tiles, tps;                       // column tiles of all problems; tiles per column split (grid.x splits, none empty)
    int nch, nchp;                        // real chunks C/32, chunks of the padded K
    QuantRowInput in;
};

template <typename T, int FMT, int PR>
__global__ __launch_bounds__(BLK_NT) void gemm_mx_rows_kernel(RowsBatch b) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    using TL = RowsTile<PR>;
    constexpr int BM = TL::BM, BN = TL::BN, SB = rows_slot(FMT), NWP = BN / 64;
    DGQ_DIAG_DECL
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_k = wid >> 2, wave_m = PR == 64 ? (wid >> 1) & 1 : 0, wave_n = PR == 64 ? wid & 1 : wid & 3;
    const int lr = lane & 31, hh = lane >> 5;
    const int arow = wave_m * 32 + lr, wcol = wave_n * 32 + lr;
    uint8_t* w_lds = smem;
    float* vtab = reinterpret_cast<float*>(smem + TL::RING);
    float* vcol = vtab + 3 * BM;
    uint8_t* a_lds = smem + TL::RING + TL::VEC;            // [chunk][row][SB]
    uint8_t* sc_lds = a_lds + b.nchp * PR * SB;            // [chunk][row]
    const int m0 = blockIdx.y * PR;

    // ---- phase 1: this panel's rows -> codes and scale bytes, the stand-alone quantisers' statement; no row terms in the epilogue
    if (tid < BM) { vtab[tid] = 1.0f; vtab[BM + tid] = 0.0f; vtab[2 * BM + tid] = 0.0f; }
    for (int r = wid; r < PR; r += BLK_NW) {
        const int m = m0 + r;                               // wave-uniform
        int cb0 = 0;
        if (m < b.in.rows) {
            const QuantRowSource<T> s = quant_row_source<T>(b.in, m, lane);
            quant_block_walk<T>(b.in, s, lane, [&](const float (&v)[4], int c, bool inside, int) {
                uint8_t* blk = a_lds + ((c >> 5) * PR + r) * SB;
                const int t = lane & 3;                    // lanes 4g .. 4g + 3 hold 96 bits = 3 words per 6-bit plane; lane t < 3 writes word t
                int E;
                if constexpr (FMT == 6) {
                    const uint32_t piece = mx6_block_codes(v, E);
                    const uint32_t word = mx6_lane_word(piece, (uint32_t)__shfl_down((int)piece, 1, 64), t);
                    if (inside && t < 3) *reinterpret_cast<uint32_t*>(blk + ((c >> 2) & 7) * 3 + t) = word;
                } else if constexpr (FMT == 8) {
                    uint32_t hi, lo;
                    mxint8_block_codes(v, E, hi, lo);
                    const uint32_t hi_word = mx6_lane_word(hi, (uint32_t)__shfl_down((int)hi, 1, 64), t);
                    const uint32_t lo_word = mx6_lane_word(lo, (uint32_t)__shfl_down((int)lo, 1, 64), t);
                    if (inside && t < 3) {
                        *reinterpret_cast<uint32_t*>(blk + ((c >> 2) & 7) * 3 + t) = hi_word;
                        *reinterpret_cast<uint32_t*>(blk + 24 + ((c >> 2) & 7) * 3 + t) = lo_word;
                    }
                } else {
                    const uint4 q = mx4_block_codes(v, E);  // the block's 128 bits in its first lane
                    if (inside && (lane & 7) == 0) *reinterpret_cast<uint4*>(blk) = q;
                }
                if (inside && (lane & 7) == 0) sc_lds[(c >> 5) * PR + r] = (uint8_t)(E + 127);
            });
            cb0 = b.in.C >> 5;
        }
        for (int cb = cb0 + lane; cb < b.nchp; cb += 64) {  // a row past M, the K padding: zero codes under 2^0
            uint2* z = reinterpret_cast<uint2*>(a_lds + (cb * PR + r) * SB);
#pragma unroll
            for (int j = 0; j < SB / 8; ++j) z[j] = make_uint2(0u, 0u);
            sc_lds[cb * PR + r] = 127;
        }
    }
    __syncthreads();

    // ---- phase 2: the column tiles [ct0, ct1) of the launch's tile list against the resident panel
    const int ct0 = blockIdx.x * b.tps, ct1 = min(ct0 + b.tps, b.tiles);
    const int nkt = (b.nch + BLK_CH - 1) / BLK_CH;
    uint2 rw[NWP][3];                                       // staging registers: this thread's (column(s), chunk wid) of one K tile
    auto load_w = [&](const GemmParams& P, int n0, int kt) {
        const int cc = kt * BLK_CH + wid;                   // wave-uniform chunk
#pragma unroll
        for (int j = 0; j < NWP; ++j) {
            rw[j][0] = rw[j][1] = rw[j][2] = make_uint2(0u, 0u);
            if (cc < b.nchp) {                              // the weight image ends at Kp (a multiple of 4 chunks, not of 8)
                const int n = min(n0 + 64 * j + lane, P.N - 1);
                const uint2* src = reinterpret_cast<const uint2*>(P.wpacked + ((int64_t)n * b.nchp + cc) * 24);
                rw[j][0] = src[0]; rw[j][1] = src[1]; rw[j][2] = src[2];
            }
        }
    };
    auto store_w = [&]() {
#pragma unroll
        for (int j = 0; j < NWP; ++j) {
            uint2* dw = reinterpret_cast<uint2*>(w_lds + (wid * BN + 64 * j + lane) * 32);
            dw[0] = rw[j][0]; dw[1] = rw[j][1]; dw[2] = rw[j][2];
        }
    };
    auto problem_of = [&](int ct, int pi) {
        while (pi + 1 < b.n && ct >= b.tile0[pi + 1]) ++pi;
        return pi;
    };

    int pi = problem_of(ct0, 0);
    load_w(b.p[pi], (ct0 - b.tile0[pi]) * BN, 0);
    for (int ct = ct0; ct < ct1; ++ct) {
        const GemmParams& P = b.p[pi];
        const int n0 = (ct - b.tile0[pi]) * BN;
        if (ct > ct0) __syncthreads();                      // the last tile's epilogue has read the scratch (over the ring) and vcol
        if (tid < BN) {
            const int n = min(n0 + tid, P.N - 1);
            vcol[tid] = P.alpha[n]; vcol[BN + tid] = 0.0f; vcol[2 * BN + tid] = P.gamma[n]; vcol[3 * BN + tid] = 0.0f;
        }
        v16f accf[1][1];
#pragma unroll
        for (int i = 0; i < 16; ++i) accf[0][0][i] = 0.0f;
        for (int kt = 0; kt < nkt; ++kt) {
            store_w();
            __syncthreads();
            if (kt + 1 < nkt) load_w(P, n0, kt + 1);
#pragma unroll
            for (int ii = 0; ii < BLK_CH / 4; ++ii) {
                const int pr = 2 * ii + wave_k;             // this K wave's chunk pairs of the tile
                if (kt * BLK_CH + 2 * pr >= b.nch) break;   // (wave-uniform: both chunks of the pair are K padding)
                const int ci = 2 * pr + hh;                 // the lane half's chunk = its K block of the 64-deep step
                const int cg = kt * BLK_CH + ci;            // ... in the panel (<= nch < nchp where nch is odd)
                const uint8_t* ap = a_lds + (cg * PR + arow) * SB;
                const uint8_t* bp = w_lds + (ci * BN + wcol) * 32;
                const uint4 b4 = *reinterpret_cast<const uint4*>(bp);
                const uint2 b2 = *reinterpret_cast<const uint2*>(bp + 16);
                const int sa = sc_lds[cg * PR + arow];
                const v8i bf = {(int)b4.x, (int)b4.y, (int)b4.z, (int)b4.w, (int)b2.x, (int)b2.y, 0, 0};
                if constexpr (FMT == 6) {
                    const uint2 a0 = *reinterpret_cast<const uint2*>(ap), a1 = *reinterpret_cast<const uint2*>(ap + 8),
                                a2 = *reinterpret_cast<const uint2*>(ap + 16);
                    const v8i af = {(int)a0.x, (int)a0.y, (int)a1.x, (int)a1.y, (int)a2.x, (int)a2.y, 0, 0};
                    accf[0][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af, bf, accf[0][0], 2, 2, 0, sa, 0, 128);
                } else if constexpr (FMT == 8) {
                    const uint4 h4 = *reinterpret_cast<const uint4*>(ap);
                    const uint4 m4 = *reinterpret_cast<const uint4*>(ap + 16);     // hi[16..23] | lo[0..7]
                    const uint4 l4 = *reinterpret_cast<const uint4*>(ap + 32);     // lo[8..23]
                    const v8i hf = {(int)h4.x, (int)h4.y, (int)h4.z, (int)h4.w, (int)m4.x, (int)m4.y, 0, 0};
                    const v8i lf = {(int)m4.z, (int)m4.w, (int)l4.x, (int)l4.y, (int)l4.z, (int)l4.w, 0, 0};
                    accf[0][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(lf, bf, accf[0][0], 2, 2, 0, sa, 0, 123);
                    accf[0][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(hf, bf, accf[0][0], 2, 2, 0, sa, 0, 127);
                } else {
                    const uint4 a4 = *reinterpret_cast<const uint4*>(ap);
                    const v8i af = {(int)a4.x, (int)a4.y, (int)a4.z, (int)a4.w, 0, 0, 0, 0};
                    accf[0][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af, bf, accf[0][0], 4, 2, 0, sa, 0, 128);
                }
            }
            __syncthreads();                                // (behind the last K tile: the ring is idle, the scratch may lie over it)
        }
        const int pn = ct + 1 < ct1 ? problem_of(ct + 1, pi) : pi;
        if (ct + 1 < ct1) load_w(b.p[pn], (ct + 1 - b.tile0[pn]) * BN, 0);       // the next tile's first weights fly over the epilogue
        v16i acc0[1][1];
#pragma unroll
        for (int i = 0; i < 16; ++i) acc0[0][0][i] = 0;
        gemm_store_tile<false, T, BM, BN, TL::WVM, TL::WVN, 2, TL::RING, 1, 1>(P, 0, smem, vtab, vcol, wid, lane, wave_m, wave_n, wave_k, m0, n0,
                                                                               acc0, accf DGQ_DIAG_ARG);
        pi = pn;
    }
    DGQ_DIAG_FLUSH(mx_rows, BLK_NW, wid, lane);
}

// one instantiation: the dynamic-LDS opt-in once, then the launch
template <typename T, int FMT, int PR>
int rows_launch(const char* who, dim3 grid, size_t lds, hipStream_t st, const RowsBatch& b) {
    static std::atomic<bool> raised{false};
    const auto fn = gemm_mx_rows_kernel<T, FMT, PR>;
    if (!raised.load(std::memory_order_acquire)) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, ROWS_LDS) != hipSuccess) {
            (void)hipGetLastError();
            dgq_set_error("%s: cannot raise the dynamic LDS to %d bytes", who, ROWS_LDS);
            return DGQ_EINVAL;
        }
        raised.store(true, std::memory_order_release);
    }
    hipLaunchKernelGGL(fn, grid, dim3(BLK_NT), lds, st, b);
    return dgq_launch_status(who);
}
template <typename T>
int rows_launch_fmt(const char* who, int fmt, int pr, dim3 grid, size_t lds, hipStream_t st, const RowsBatch& b) {
    if (pr == 64) {
        if (fmt == 6) return rows_launch<T, 6, 64>(who, grid, lds, st, b);
        if (fmt == 8) return rows_launch<T, 8, 64>(who, grid, lds, st, b);
        return rows_launch<T, 4, 64>(who, grid, lds, st, b);
    }
    if (fmt == 6) return rows_launch<T, 6, 32>(who, grid, lds, st, b);
    if (fmt == 8) return rows_launch<T, 8, 32>(who, grid, lds, st, b);
    return rows_launch<T, 4, 32>(who, grid, lds, st, b);
}

// column splits for `panels` row panels over `tiles` column tiles: enough workgroups for the device, none empty
int rows_splits(int panels, int tiles) {
    int s = (ROWS_TARGET_WGS + panels - 1) / panels;
    s = s < 1 ? 1 : (s > tiles ? tiles : s);
    const int tps = (tiles + s - 1) / s;
    return (tiles + tps - 1) / tps;
}

}  // namespace

extern "C" int dgq_gemm_mx_rows_plan(int M, int Nsum, int Kp, int a_format) {
    if (M <= 0 || Nsum <= 0 || Kp <= 0 || Kp % DGQ_KTILE != 0 || !(a_format == 6 || a_format == 8 || a_format == 4)) return 0;
    const int pr = rows_panel(a_format, Kp / DGQ_KCHUNK);
    if (pr == 0) return 0;                                  // the panel does not fit the LDS
    const int tiles = (Nsum + rows_bn(pr) - 1) / rows_bn(pr);
    if (tiles < 2) return 0;                                // one column tile in all: nothing to keep resident for
    return rows_splits((M + pr - 1) / pr, tiles);
}

extern "C" int dgq_gemm_mx_rows(const dgq_quant_act_args_t* in, int a_format, int n_problems, const dgq_gemm_args_t* probs, int col_splits,
                                void* stream) {
    const char* who = "dgq_gemm_mx_rows";
    DGQ_CHECK_ARG(in && probs, "%s: null pointer", who);
    DGQ_CHECK_ARG(a_format == 6 || a_format == 8 || a_format == 4, "%s: a_format=%d (6 mxfp6, 8 mxint8, 4 mxfp4)", who, a_format);
    DGQ_CHECK_ARG(n_problems >= 1 && n_problems <= ROWS_MAX_PROBLEMS, "%s: %d problems (1 .. %d)", who, n_problems, ROWS_MAX_PROBLEMS);
    DGQ_CHECK_ARG(col_splits >= 0, "%s: col_splits=%d", who, col_splits);
    const dgq_quant_act_args_t& a = *in;
    RowsBatch b;
    int Ho, Wo;
    int rc = dgq_check_quant_input(a, who, {DGQ_KCHUNK, false, true}, b.in, Ho, Wo);
    if (rc != DGQ_OK) return rc;
    DGQ_CHECK_ARG(a.kh == 1 && a.kw == 1 && !a.ups, "%s: Linear inputs only (kh = kw = 1, no ups); a convolution's rows go through the gather", who);
    DGQ_CHECK_ARG((int64_t)b.in.rows * a.C < (1LL << 40), "%s: too many rows", who);
    const int Kp = probs[0].Kp, y_dtype = probs[0].y_dtype;
    DGQ_CHECK_ARG(y_dtype == a.x_dtype && (y_dtype == DGQ_F32 || y_dtype == DGQ_F16 || y_dtype == DGQ_BF16), "%s: x / y dtypes %d / %d must be one of the three and equal",
                  who, a.x_dtype, y_dtype);
    const int pr = Kp > 0 && Kp % DGQ_KTILE == 0 ? rows_panel(a_format, Kp / DGQ_KCHUNK) : 64;      // (a bad Kp: the set-up below refuses it)
    DGQ_CHECK_ARG(pr != 0, "%s: a 32-row panel of Kp=%d does not fit the LDS (%d bytes)", who, Kp, ROWS_LDS);
    const int bn = rows_bn(pr);
    b.n = n_problems; b.tiles = 0;
    for (int i = 0; i < n_problems; ++i) {
        dgq_gemm_args_t g = probs[i];
        DGQ_CHECK_ARG(g.Kp == Kp && g.y_dtype == y_dtype, "%s: problem %d has Kp=%d, y dtype %d; the problems must share Kp=%d and y dtype %d", who, i, g.Kp,
                      g.y_dtype, Kp, y_dtype);
        DGQ_CHECK_ARG(!g.extra || !g.extra->gn_partial, "%s: no GroupNorm partials (problem %d)", who, i);
        g.codes = reinterpret_cast<const int8_t*>(a.x);     // unused: the codes are formed in LDS (the set-up wants a 16-byte aligned pointer)
        BlockGather q;
        rc = block_gemm_setup(who, g, a.B, a.H, a.W, a.C, 1, 1, 1, 0, 0, false, b.p[i], q);
        if (rc != DGQ_OK) return rc;
        b.p[i].codes = nullptr;
        b.tile0[i] = b.tiles;
        b.tiles += (g.N + bn - 1) / bn;
        b.nch = q.nch; b.nchp = q.nchp;
    }
    for (int i = n_problems; i < ROWS_MAX_PROBLEMS; ++i) { b.p[i] = b.p[0]; b.tile0[i] = b.tiles; }
    const int panels = (b.in.rows + pr - 1) / pr;
    DGQ_CHECK_ARG(panels <= 65535, "%s: %d row panels (max 65535)", who, panels);
    int s = col_splits == 0 ? rows_splits(panels, b.tiles) : col_splits;
    s = s > b.tiles ? b.tiles : s;
    b.tps = (b.tiles + s - 1) / s;
    s = (b.tiles + b.tps - 1) / b.tps;                      // no empty split
    const dim3 grid(s, panels);
    const size_t lds = (size_t)rows_lds_bytes(a_format, pr, b.nchp);
    hipStream_t st = (hipStream_t)stream;
    DGQ_QUANT_DTYPE_SWITCH(a.x_dtype, who, return rows_launch_fmt<TIn>(who, a_format, pr, grid, lds, st, b))
    return DGQ_OK;
}
