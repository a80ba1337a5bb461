// gemm_blockq.hip — the W4A8 / W8A8 layer under the real-time BLOCK activation quantiser (quant_block.hip): one (δ, β) per row and
// 32-chunk of K, so the per-M kernels (one scale per row) and the per-K kernels (one scale per chunk, shared by all rows) cannot
// express it.  The K loop here keeps NO running total: every 32-chunk is one mfma_i32_32x32x32_i8 into a ZEROED accumulator, then
//   accf[r] = fma(β[m_r, c], Vc[n, c], fma(δ[m_r, c], float(P[r]), accf[r]))           r = 0..15, chunks in ascending order
// with m_r the row of accumulator register r (gemm_tile.h: (r & 3) + 8·(r >> 2) + 4·(lane >> 5)) and n the lane's column; the rest
// is the family's dequantising store epilogue gemm_store_tile<false, ...> with gamma = bias and rowsum R[m] = Σ_c δ·rs:
// dgq_dequant<false> gives ga + al·(accf − zw·R).  Residual, res_div bias rows, GEGLU pairs, GroupNorm partials, y2 / ldy redirects and
// 16-bit outputs are that epilogue's, not rewritten here.
//
// Operands: A = the quantiser's int8 codes [pixels][C] (MFMA rows), B = the natural-order weight image (W4: dgq_pack_w4 layout 1,
// widened as gemm_wxa8.hip does; W8: int8).  A convolution gathers: chunk c = tap·(C/32) + cb of output row m is the 32 contiguous
// code bytes, and the table entry cb, of pixel (ho·stride − pad + dh, wo·stride − pad + dw) (>> ups); outside the image codes, δ and β
// are 0, so the tap contributes exactly 0.  A Linear layer is the 1x1 case with pixel = row.
//
// One tile shape: 64 x 64 per workgroup, 8 waves (2 x 2 x 2: the two K waves of a 32x32 MFMA tile take the even / the odd chunks of
// every K tile and meet in the epilogue's LDS transposition, k = 0 first — a fixed order; the K loop is a chain of dependent
// latencies, and a second wave per SIMD overlaps them: −10 % of the SD step against one K wave), K in tiles of 256 = 8 chunks, one staged
// chunk per wave (against 4-chunk tiles: the same times — the loop is bound by the per-chunk body, not by the staging round trips;
// profiles/r12_realtime_block.txt).  Plain global -> register -> LDS staging, the loads of tile t + 1 in flight behind the MFMAs of
// tile t; thread (row = tid & 63, chunk = tid >> 6) stages the 32 code bytes, the {δ, β} pair, the weight piece and the Vc entry of its
// (row, chunk) — the chunk, hence the tap, is wave-uniform.  No K split over workgroups, no atomics, nothing exchanged between
// workgroups.  The per-chunk body — the MFMA, then cvt + 2 fma per accumulator register (48 VALU per MFMA) behind 8 broadcast LDS
// reads of {δ, β} — is what a faster loop has to attack: several MFMA tiles per wave, the β·Vc term as an fp32 MFMA pass.
#include "gemm_block.h"

DGQ_DIAG_BUFFER(blockq)

namespace {

struct BlockqOperand {
    const float2* table; int ldt;         // {δ, β} per (pixel, block)
    const float* vc;                      // Vc [N][nchp]
};

constexpr int BQ_A = BLK_CH * BLK_BM * 32;                   // [chunk][row][32 B]
constexpr int BQ_DB = BLK_CH * BLK_BM * 8, BQ_VC = BLK_CH * BLK_BN * 4;
constexpr int bq_w_bytes(int wbits) { return BLK_CH * BLK_BN * (wbits == 4 ? 16 : 32); }

template <int WBITS, typename TOut>
__global__ __launch_bounds__(BLK_NT) void gemm_blockq_kernel(GemmParams p, BlockGather q, BlockqOperand o) {
    constexpr int RING = block_ring(BQ_A + bq_w_bytes(WBITS) + BQ_DB + BQ_VC);
    __shared__ __attribute__((aligned(16))) uint8_t smem[RING + BLK_VEC];
    DGQ_DIAG_DECL
    DGQ_STAMP(0); DGQ_STAMP_REAL(1); DGQ_STAMP_WHERE(2);
    uint8_t* a_lds = smem;
    uint8_t* w_lds = smem + BQ_A;
    float2* db_lds = reinterpret_cast<float2*>(smem + BQ_A + bq_w_bytes(WBITS));
    float* vc_lds = reinterpret_cast<float*>(smem + BQ_A + bq_w_bytes(WBITS) + BQ_DB);
    float* vtab = reinterpret_cast<float*>(smem + RING);
    const BlockRoles r = block_roles();

    // ---- the staged (row, chunk) of this thread: output position of the row, weight row of the column
    const BlockRow row = block_row(q, min(r.m0 + r.srow, p.M - 1));
    const int n = min(r.n0 + r.srow, p.N - 1);
    const uint8_t* wrow = p.wpacked + (int64_t)n * (WBITS == 4 ? p.Kp / 2 : p.Kp);
    const float* vcrow = o.vc + (int64_t)n * q.nchp;

    // ---- epilogue vectors: R[m] (the in-image taps' rho in tap order), the column constants
    if (r.tid < BLK_BM) block_vectors(vtab, vtab + 3 * BLK_BM, r.tid, p, n, block_rowsum_taps(q, row, p.rowsum), p.zw[n]);

    // ---- staging registers of one K tile
    uint4 ra0, ra1, rw0, rw1;
    float2 rdb;
    float rvc;
    auto load_tile = [&](int kt) {
        const int cc = kt * BLK_CH + r.sch;                 // wave-uniform chunk
        ra0 = ra1 = rw0 = rw1 = make_uint4(0u, 0u, 0u, 0u);
        rdb = make_float2(0.0f, 0.0f);
        rvc = 0.0f;
        const BlockChunk x = block_chunk(q, row, cc);
        if (x.in) {
            const uint4* src = reinterpret_cast<const uint4*>(p.codes + x.pix * q.C + x.cb * 32);
            ra0 = src[0]; ra1 = src[1];
            rdb = o.table[x.pix * o.ldt + x.cb];
        }
        if (cc < q.nchp) {                                  // the weight image and Vc end at Kp (a multiple of 4 chunks, not of 8)
            if (WBITS == 4) {
                rw0 = *reinterpret_cast<const uint4*>(wrow + cc * 16);
            } else {
                rw0 = *reinterpret_cast<const uint4*>(wrow + cc * 32);
                rw1 = *reinterpret_cast<const uint4*>(wrow + cc * 32 + 16);
            }
            rvc = vcrow[cc];
        }
    };
    auto store_tile = [&]() {
        uint4* da = reinterpret_cast<uint4*>(a_lds + (r.sch * BLK_BM + r.srow) * 32);
        da[0] = ra0; da[1] = ra1;
        if (WBITS == 4) {
            *reinterpret_cast<uint4*>(w_lds + (r.sch * BLK_BN + r.srow) * 16) = rw0;
        } else {
            uint4* dw = reinterpret_cast<uint4*>(w_lds + (r.sch * BLK_BN + r.srow) * 32);
            dw[0] = rw0; dw[1] = rw1;
        }
        db_lds[r.sch * BLK_BM + r.srow] = rdb;
        vc_lds[r.sch * BLK_BN + r.srow] = rvc;
    };

    v16f accf[1][1];
#pragma unroll
    for (int i = 0; i < 16; ++i) accf[0][0][i] = 0.0f;
    const int nkt = (q.nch + BLK_CH - 1) / BLK_CH;
    load_tile(0);
    for (int kt = 0; kt < nkt; ++kt) {
        store_tile();
        __syncthreads();
        if (kt + 1 < nkt) load_tile(kt + 1);
#pragma unroll
        for (int ii = 0; ii < BLK_CH / 2; ++ii) {
            const int ci = 2 * ii + r.wave_k;               // this K wave's chunks of the tile
            if (kt * BLK_CH + ci >= q.nch) break;           // (wave-uniform: the chunks of the K padding)
            const v4i af = *reinterpret_cast<const v4i*>(a_lds + (ci * BLK_BM + r.arow) * 32 + r.hh * 16);
            v4i bf;
            if constexpr (WBITS == 4) {
                // layout 1: rows with bit 4 set keep the two 8-byte halves of a chunk exchanged (n0 is a multiple of 64)
                const uint2 v = *reinterpret_cast<const uint2*>(w_lds + (ci * BLK_BN + r.wcol) * 16 + ((r.hh ^ ((r.wcol >> 4) & 1)) << 3));
                bf = (v4i){(int)(v.x & 0x0F0F0F0Fu), (int)((v.x >> 4) & 0x0F0F0F0Fu), (int)(v.y & 0x0F0F0F0Fu), (int)((v.y >> 4) & 0x0F0F0F0Fu)};
            } else {
                bf = *reinterpret_cast<const v4i*>(w_lds + (ci * BLK_BN + r.wcol) * 32 + r.hh * 16);
            }
            v16i pz;
#pragma unroll
            for (int i = 0; i < 16; ++i) pz[i] = 0;
            const v16i P = __builtin_amdgcn_mfma_i32_32x32x32_i8(af, bf, pz, 0, 0, 0);
            const float vcv = vc_lds[ci * BLK_BN + r.wcol];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                // rows 8g + 4hh .. + 3 of the wave tile: registers 4g .. 4g + 3
                const float4* t = reinterpret_cast<const float4*>(db_lds + ci * BLK_BM + r.wave_m * 32 + 8 * g + 4 * r.hh);
                const float4 t0 = t[0], t1 = t[1];
                const float dl[4] = {t0.x, t0.z, t1.x, t1.z}, be[4] = {t0.y, t0.w, t1.y, t1.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int i = 4 * g + j;
                    accf[0][0][i] = __builtin_fmaf(be[j], vcv, __builtin_fmaf(dl[j], (float)P[i], accf[0][0][i]));
                }
            }
        }
        __syncthreads();
    }
    block_store<TOut, RING>(p, smem, r, nkt, accf DGQ_DIAG_ARG);
    DGQ_DIAG_FLUSH(blockq, BLK_NW, r.wid, r.lane);
}

template <int WBITS>
struct BlockqKernel { template <typename TOut> static constexpr auto fn = gemm_blockq_kernel<WBITS, TOut>; };

}  // namespace

extern "C" int dgq_gemm_blockq(const dgq_gemm_args_t* g, const dgq_gemm_block_t* blk, void* stream) {
    const char* who = "dgq_gemm_blockq";
    DGQ_CHECK_ARG(g && blk && blk->table && blk->vc, "dgq_gemm_blockq: null pointer");
    const dgq_gemm_args_t& a = *g;
    const dgq_gemm_block_t& k = *blk;
    DGQ_CHECK_ARG(a.w_bits == 4 || a.w_bits == 8, "dgq_gemm_blockq: w_bits=%d unsupported", a.w_bits);
    DGQ_CHECK_ARG(a.rowsum_parts == 1, "dgq_gemm_blockq: rowsum is the quantiser's rho, one part");
    GemmParams p;
    BlockGather q;
    const int rc = block_gemm_setup(who, a, k.B, k.H, k.W, k.C, k.kh, k.kw, k.stride, k.pad, k.ups, true, p, q);
    if (rc != DGQ_OK) return rc;
    DGQ_CHECK_ARG(k.ldt >= q.cpb, "dgq_gemm_blockq: table pitch %d < %d blocks", k.ldt, q.cpb);
    DGQ_CHECK_ARG((reinterpret_cast<uintptr_t>(k.table) & 7) == 0, "dgq_gemm_blockq: the table must be 8-byte aligned");
    const BlockqOperand o = {reinterpret_cast<const float2*>(k.table), k.ldt, k.vc};
    hipStream_t st = (hipStream_t)stream;
    return a.w_bits == 4 ? block_gemm_launch<BlockqKernel<4>>(who, p, q, o, a.y_dtype, st) : block_gemm_launch<BlockqKernel<8>>(who, p, q, o, a.y_dtype, st);
}
