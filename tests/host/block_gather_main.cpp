// Host driver of dgq_amd/csrc/gemm_gather.h for tests/test_block_gather_cpu.py: the tap gather of the real-time block GEMMs, computed by
// the very functions the kernels stage their operands through, on a CPU.
// stdin : B H W C kh kw stride pad ups Kp   (H, W: behind a folded upsample, as the GEMM entries take them)
// stdout: one line "M nch nchp", then for every output row m and chunk cc in [0, nchp) one line "pix cb in"
#include <cstdio>
#include "gemm_gather.h"

int main() {
    int B, H, W, C, kh, kw, stride, pad, ups, Kp;
    if (scanf("%d %d %d %d %d %d %d %d %d %d", &B, &H, &W, &C, &kh, &kw, &stride, &pad, &ups, &Kp) != 10 || B < 1 || H < 1 || W < 1 || C < 32 ||
        C % 32 || kh < 1 || kw < 1 || stride < 1 || pad < 0 || (ups != 0 && ups != 1) || (ups && (H % 2 || W % 2)) || Kp % 32 || kh * kw * C > Kp) {
        fprintf(stderr, "block_gather: bad geometry\n");
        return 2;
    }
    const BlockGather q = block_gather(B, H, W, C, kh, kw, stride, pad, ups, Kp);       // as block_gemm_setup (gemm_block.h) makes it
    if (q.Ho < 1 || q.Wo < 1) {
        fprintf(stderr, "block_gather: empty output\n");
        return 2;
    }
    const int M = B * q.Ho * q.Wo;
    printf("%d %d %d\n", M, q.nch, q.nchp);
    for (int m = 0; m < M; ++m) {
        const BlockRow r = block_row(q, m);
        for (int cc = 0; cc < q.nchp; ++cc) {
            const BlockChunk x = block_chunk(q, r, cc);
            printf("%lld %d %d\n", x.pix, x.cb, x.in ? 1 : 0);
        }
    }
    return 0;
}
