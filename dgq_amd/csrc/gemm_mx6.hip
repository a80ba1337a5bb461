// gemm_mx6.hip — the W4 layer under the real-time MXFP6 activation quantiser (quant_mx6.hip) on the block-scaled matrix cores: every K
// step is v_mfma_scale_f32_32x32x64_f8f6f4 with both operands FP6 E2M3.  The instruction takes one E8M0 scale per lane = per (row,
// 32-element K block), which is exactly the quantiser's block: ONE fp32 accumulator for the whole K, no per-chunk VALU, no table reads
// (against gemm_blockq.hip: cvt + 2 fma per accumulator register and chunk behind 8 LDS reads of {δ, β}).
//   y[m,n] = gamma[n] + alpha[n]·Σ_c 2^(E[m,c]+1)·Σ_{k∈c} a[m,k]·w6[n,k]
// A = the activation codes [pixels][C/32][24 B], scale_a = the lane's own (row, block) byte; B = the weight image of dgq_pack_w_mx6:
// the E2M3 codes of (q − z)/2 — exact for integer z and |q − z| <= 15 — with the constant block scale 2^1 (byte 128).  No zero-point
// terms: the epilogue is the family's gemm_store_tile<false, ...> with R = 0, zw = 0, gamma = bias, alpha = δw (residual, res_div, GEGLU
// pairs, GroupNorm partials, y2 / ldy redirects and 16-bit outputs are that epilogue's).
//
// Operand maps (pinned by the one-hot tests of tests/test_gpu_realtime_mxfp6.py): lane l holds row / column l & 31 and the K block
// l >> 5 of the 64-deep step — 32 consecutive k as the 192-bit little-endian string of their 6-bit codes in the first six registers
// (element j at bits 6j .. 6j + 5), and its scale in byte 0 of the scale register.
//
// The gather, tile and wave layout are the block family's (gemm_gather.h, gemm_block.h; shared with gemm_blockq.hip): 64 x 64 per workgroup, 8 waves (2 x 2 x 2, the two K waves meet in the
// epilogue's LDS transposition, k = 0 first), K tiles of 8 chunks, thread (row = tid & 63, chunk = tid >> 6) stages the 24 code bytes, the
// scale byte and the weight piece of its (row, chunk); one MFMA covers the chunk pair (2i, 2i + 1), one chunk per lane half.  Chunk c =
// tap·(C/32) + cb of output row m reads pixel (ho·stride − pad + dh, wo·stride − pad + dw) (>> ups); a tap outside the image (and the K
// padding) stages zero codes under the scale 2^0 and contributes exactly 0.  The LDS images keep 32 bytes per (row, chunk) — a lane
// reads 16 + 8 of them, as gemm_blockq.hip's fragment reads are spaced; the HBM images stay at 24.  No K split, no atomics.
#include "gemm_block.h"

DGQ_DIAG_BUFFER(mx6)

typedef int v8i __attribute__((ext_vector_type(8)));

namespace {

struct Mx6Operand { const uint8_t* scale; int lds; };         // E8M0 byte per (pixel, block)

constexpr int MX_A = BLK_CH * BLK_BM * 32, MX_W = BLK_CH * BLK_BN * 32;  // [chunk][row][32 B], 24 used
constexpr int MX_SC = BLK_CH * BLK_BM;                                   // [chunk][row] scale bytes
constexpr int MX_RING = block_ring(MX_A + MX_W + MX_SC);

template <typename TOut>
__global__ __launch_bounds__(BLK_NT) void gemm_mx6_kernel(GemmParams p, BlockGather q, Mx6Operand o) {
    __shared__ __attribute__((aligned(16))) uint8_t smem[MX_RING + BLK_VEC];
    DGQ_DIAG_DECL
    DGQ_STAMP(0); DGQ_STAMP_REAL(1); DGQ_STAMP_WHERE(2);
    uint8_t* a_lds = smem;
    uint8_t* w_lds = smem + MX_A;
    uint8_t* sc_lds = smem + MX_A + MX_W;
    float* vtab = reinterpret_cast<float*>(smem + MX_RING);
    const BlockRoles r = block_roles();

    // ---- the staged (row, chunk) of this thread: output position of the row, weight row of the column
    const BlockRow row = block_row(q, min(r.m0 + r.srow, p.M - 1));
    const int n = min(r.n0 + r.srow, p.N - 1);
    const uint8_t* wrow = p.wpacked + (int64_t)n * q.nchp * 24;
    const int64_t apitch = (int64_t)q.cpb * 24;             // code bytes per pixel

    // ---- epilogue vectors: no row terms (R = 0), the column constants with zw = 0
    if (r.tid < BLK_BM) block_vectors(vtab, vtab + 3 * BLK_BM, r.tid, p, n, 0.0f, 0.0f);

    // ---- staging registers of one K tile
    uint2 ra0, ra1, ra2, rw0, rw1, rw2;
    uint32_t rsc;
    auto load_tile = [&](int kt) {
        const int cc = kt * BLK_CH + r.sch;                 // wave-uniform chunk
        ra0 = ra1 = ra2 = rw0 = rw1 = rw2 = make_uint2(0u, 0u);
        rsc = 127u;                                         // zero codes under 2^0: exactly 0
        const BlockChunk x = block_chunk(q, row, cc);
        if (x.in) {
            const uint2* src = reinterpret_cast<const uint2*>(reinterpret_cast<const uint8_t*>(p.codes) + x.pix * apitch + x.cb * 24);
            ra0 = src[0]; ra1 = src[1]; ra2 = src[2];
            rsc = o.scale[x.pix * o.lds + x.cb];
        }
        if (cc < q.nchp) {                                  // the weight image ends at Kp (a multiple of 4 chunks, not of 8)
            const uint2* src = reinterpret_cast<const uint2*>(wrow + cc * 24);
            rw0 = src[0]; rw1 = src[1]; rw2 = src[2];
        }
    };
    auto store_tile = [&]() {
        uint2* da = reinterpret_cast<uint2*>(a_lds + (r.sch * BLK_BM + r.srow) * 32);
        da[0] = ra0; da[1] = ra1; da[2] = ra2;
        uint2* dw = reinterpret_cast<uint2*>(w_lds + (r.sch * BLK_BN + r.srow) * 32);
        dw[0] = rw0; dw[1] = rw1; dw[2] = rw2;
        sc_lds[r.sch * BLK_BM + r.srow] = (uint8_t)rsc;
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
        for (int ii = 0; ii < BLK_CH / 4; ++ii) {
            const int pr = 2 * ii + r.wave_k;               // this K wave's chunk pairs of the tile
            if (kt * BLK_CH + 2 * pr >= q.nch) break;       // (wave-uniform: both chunks of the pair are K padding)
            const int ci = 2 * pr + r.hh;                   // the lane half's chunk = its K block of the 64-deep step
            const uint8_t* ap = a_lds + (ci * BLK_BM + r.arow) * 32;
            const uint8_t* bp = w_lds + (ci * BLK_BN + r.wcol) * 32;
            const uint4 a4 = *reinterpret_cast<const uint4*>(ap);
            const uint2 a2 = *reinterpret_cast<const uint2*>(ap + 16);
            const uint4 b4 = *reinterpret_cast<const uint4*>(bp);
            const uint2 b2 = *reinterpret_cast<const uint2*>(bp + 16);
            const int sa = sc_lds[ci * BLK_BM + r.arow];
            const v8i af = {(int)a4.x, (int)a4.y, (int)a4.z, (int)a4.w, (int)a2.x, (int)a2.y, 0, 0};
            const v8i bf = {(int)b4.x, (int)b4.y, (int)b4.z, (int)b4.w, (int)b2.x, (int)b2.y, 0, 0};
            accf[0][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af, bf, accf[0][0], 2, 2, 0, sa, 0, 128);
        }
        __syncthreads();
    }
    block_store<TOut, MX_RING>(p, smem, r, nkt, accf DGQ_DIAG_ARG);
    DGQ_DIAG_FLUSH(mx6, BLK_NW, r.wid, r.lane);
}

struct Mx6Kernel { template <typename TOut> static constexpr auto fn = gemm_mx6_kernel<TOut>; };

// E2M3 code of h = (q − z)/2 for an integer d = q − z, |d| <= 15: every such h is a grid value (0.5 is the subnormal 4/8; 1 .. 7.5 in
// steps of 0.5 have at most 3 mantissa bits), so the code is read off the float's exponent and top mantissa bits, no rounding
__device__ __forceinline__ uint32_t mx6_weight_code(int d) {
    const uint32_t a = (uint32_t)(d < 0 ? -d : d);
    if (a == 0) return 0u;
    const float h = (float)a * 0.5f;
    const uint32_t hb = __float_as_uint(h);
    const uint32_t mag = h < 1.0f ? (uint32_t)(h * 8.0f) : ((((hb >> 23) - 126u) << 3) | ((hb >> 20) & 7u));
    return mag | (d < 0 ? 0x20u : 0u);
}

// one thread per (n, 32-block of the natural K order): 24 bytes
__global__ void pack_w_mx6_kernel(const uint8_t* __restrict__ codes, const float* __restrict__ zw, int N, int C, int taps, int Kp,
                                  uint32_t* __restrict__ packed) {
    const int nb = Kp / 32;
    const int K = C * taps;
    const int64_t total = (int64_t)N * nb;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int n = (int)(i / nb), blk = (int)(i - (int64_t)n * nb);
        const int z = (int)zw[n];
        uint32_t w[6] = {0u, 0u, 0u, 0u, 0u, 0u};
        for (int j = 0; j < 32; ++j) {
            const int kp = blk * 32 + j;
            uint32_t c6 = 0u;
            if (kp < K) {
                const int tap = kp / C, c = kp - tap * C;
                c6 = mx6_weight_code((int)codes[(int64_t)n * K + (int64_t)c * taps + tap] - z);
            }
            const int bit = 6 * j;
            w[bit >> 5] |= c6 << (bit & 31);
            if ((bit & 31) > 26) w[(bit >> 5) + 1] |= c6 >> (32 - (bit & 31));
        }
        for (int k = 0; k < 6; ++k) packed[i * 6 + k] = w[k];
    }
}

}  // namespace

extern "C" int dgq_pack_w_mx6(const uint8_t* codes, const float* zw, int N, int C, int taps, int Kp, uint8_t* packed, void* stream) {
    DGQ_CHECK_ARG(codes && zw && packed, "dgq_pack_w_mx6: null pointer");
    DGQ_CHECK_ARG(N > 0 && C > 0 && taps > 0 && Kp > 0 && Kp % DGQ_KTILE == 0 && (int64_t)C * taps <= Kp,
                  "dgq_pack_w_mx6: Kp=%d must be a multiple of %d and >= C*taps", Kp, DGQ_KTILE);
    DGQ_CHECK_ARG((reinterpret_cast<uintptr_t>(packed) & 3) == 0, "dgq_pack_w_mx6: packed must be 4-byte aligned");
    int64_t g = ((int64_t)N * (Kp / 32) + 255) / 256;
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL(pack_w_mx6_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, codes, zw, N, C, taps, Kp,
                       reinterpret_cast<uint32_t*>(packed));
    return dgq_launch_status("dgq_pack_w_mx6");
}

extern "C" int dgq_gemm_mx6(const dgq_gemm_args_t* g, const dgq_gemm_mx6_t* mx, void* stream) {
    const char* who = "dgq_gemm_mx6";
    DGQ_CHECK_ARG(g && mx && mx->scale, "dgq_gemm_mx6: null pointer");
    const dgq_gemm_mx6_t& k = *mx;
    GemmParams p;
    BlockGather q;
    const int rc = block_gemm_setup(who, *g, k.B, k.H, k.W, k.C, k.kh, k.kw, k.stride, k.pad, k.ups, false, p, q);
    if (rc != DGQ_OK) return rc;
    DGQ_CHECK_ARG(k.lds >= q.cpb, "dgq_gemm_mx6: scale pitch %d < %d blocks", k.lds, q.cpb);
    const Mx6Operand o = {k.scale, k.lds};
    return block_gemm_launch<Mx6Kernel>(who, p, q, o, g->y_dtype, (hipStream_t)stream);
}
