// The tap gather of the real-time block GEMMs (gemm_blockq.hip, gemm_mx6.hip) — ONE statement of which input pixel chunk cc of output
// row m reads under stride, padding and a folded 2x upsample, for the device (both kernels stage through it, gemm_block.h) and for a
// plain C++ compiler (tests/host/block_gather_main.cpp checks it on a CPU against F.unfold).  This header includes nothing.
//
// K is in the natural (tap, c) order in chunks of 32 channels: chunk cc = tap·cpb + cb with tap = dh·kw + dw is channels 32·cb ..
// 32·cb + 31 of input pixel (ho·stride − pad + dh, wo·stride − pad + dw); with ups that position is taken in the 2x nearest-upsampled
// image H x W and read from the stored Hs x Ws = H/2 x W/2 one (>> ups).  A position outside H x W, and every chunk of the K padding
// (cc >= nch), reads nothing.  A Linear layer is the plain case: pixel = row, cb = cc.
#pragma once

#if defined(__HIP__)
#define DGQ_GATHER_FN __host__ __device__ inline
#else
#define DGQ_GATHER_FN inline
#endif

struct BlockGather {
    int B, H, W, Hs, Ws, C, cpb;          // H, W: behind a folded upsample; Hs, Ws: as stored; cpb = C / 32
    int kh, kw, stride, pad, ups, Ho, Wo;
    int nch;                              // real chunks: kh·kw·C/32
    int nchp;                             // chunks of the padded K: Kp / 32
    int plain;                            // 1x1, stride 1, pad 0, no ups: pixel = row
};

// The gather of a checked geometry (all positive, C % 32 == 0, even H, W under ups, Kp % 32 == 0, kh·kw·C <= Kp); ups: 0 or 1
DGQ_GATHER_FN BlockGather block_gather(int B, int H, int W, int C, int kh, int kw, int stride, int pad, int ups, int Kp) {
    BlockGather q;
    q.B = B; q.H = H; q.W = W; q.Hs = H >> ups; q.Ws = W >> ups; q.C = C; q.cpb = C / 32;
    q.kh = kh; q.kw = kw; q.stride = stride; q.pad = pad; q.ups = ups;
    q.Ho = (H + 2 * pad - kh) / stride + 1; q.Wo = (W + 2 * pad - kw) / stride + 1;
    q.nch = (int)((long long)kh * kw * q.cpb); q.nchp = Kp / 32;
    q.plain = (kh == 1 && kw == 1 && stride == 1 && pad == 0 && !ups) ? 1 : 0;
    return q;
}

struct BlockRow {
    long long pix0;                       // first pixel of the row's image (plain: the row's own pixel)
    int hbase, wbase;                     // position of tap (0, 0)
};
DGQ_GATHER_FN BlockRow block_row(const BlockGather& q, int m) {
    BlockRow r = {m, 0, 0};
    if (!q.plain) {
        const int L = q.Ho * q.Wo;
        const int b = m / L, l = m - b * L;
        const int ho = l / q.Wo, wo = l - ho * q.Wo;
        r.hbase = ho * q.stride - q.pad; r.wbase = wo * q.stride - q.pad;
        r.pix0 = (long long)b * q.Hs * q.Ws;
    }
    return r;
}

struct BlockChunk {
    long long pix;                        // the stored pixel (meaningful where in)
    int cb;                               // its 32-channel block
    bool in;                              // inside the image and below nch
};
DGQ_GATHER_FN BlockChunk block_chunk(const BlockGather& q, const BlockRow& r, int cc) {
    BlockChunk x = {r.pix0, cc, cc < q.nch};
    if (!q.plain) {
        const int tap = cc / q.cpb;
        x.cb = cc - tap * q.cpb;
        const int dh = tap / q.kw, dw = tap - dh * q.kw;
        const int hi = r.hbase + dh, wi = r.wbase + dw;
        x.in = x.in && (unsigned)hi < (unsigned)q.H && (unsigned)wi < (unsigned)q.W;
        x.pix = r.pix0 + (long long)(hi >> q.ups) * q.Ws + (wi >> q.ups);
    }
    return x;
}

// Σ rowsum[pixel] over the in-image taps of a row, in tap order (gemm_blockq.hip: R[m] of the zero-point term)
DGQ_GATHER_FN float block_rowsum_taps(const BlockGather& q, const BlockRow& r, const float* rowsum) {
    if (q.plain) return rowsum[r.pix0];
    float R = 0.0f;
    for (int dh = 0; dh < q.kh; ++dh)
        for (int dw = 0; dw < q.kw; ++dw) {
            const int hi = r.hbase + dh, wi = r.wbase + dw;
            if ((unsigned)hi < (unsigned)q.H && (unsigned)wi < (unsigned)q.W) R += rowsum[r.pix0 + (long long)(hi >> q.ups) * q.Ws + (wi >> q.ups)];
        }
    return R;
}
