// Host driver of dgq_amd/csrc/gemm_flush.h for tests/test_flush_coef_cpu.py: the flush-coefficient table of one K slice, computed by
// the very functions the GEMM kernels stage their LDS tables with, on a CPU.
// stdin : S kt_begin nk nk_total KW, then nk_total·NCH cdelta values as fp32 bit patterns (hex), then nk_total·NCH cflush bytes (decimal)
// stdout: nk·NCH coefficients (linear over the slice's chunks), then nk clear flags, one fp32 bit pattern (hex) per line
#include <cstdio>
#include <cstring>
#include <vector>
#include "gemm_flush.h"

int main() {
    int S, kt_begin, nk, nk_total, KW;
    if (scanf("%d %d %d %d %d", &S, &kt_begin, &nk, &nk_total, &KW) != 5 || S < 1 || KW < 1 || nk < 1 || kt_begin < 0 || kt_begin + nk > nk_total) {
        fprintf(stderr, "flush_coef: bad header\n");
        return 2;
    }
    const int nch = nk_total * NCH;
    std::vector<float> cdelta(nch);
    std::vector<unsigned char> cflush(nch);
    for (int i = 0; i < nch; ++i) {
        unsigned bits;
        if (scanf("%x", &bits) != 1) return 2;
        memcpy(&cdelta[i], &bits, 4);
    }
    for (int i = 0; i < nch; ++i) {
        unsigned v;
        if (scanf("%u", &v) != 1) return 2;
        cflush[i] = (unsigned char)v;
    }
    const FlushGeom fg = {S, kt_begin, nk, nk_total, KW > 1 ? (nk + KW - 1) / KW : 0};
    for (int e = 0; e < nk * NCH + nk; ++e) {
        const FlushRef x = e < nk * NCH ? flush_ref_coef(fg, kt_begin * NCH + e) : flush_ref_flag(fg, e - nk * NCH);
        const float v = flush_entry(x, cdelta.data(), cflush.data());
        unsigned bits;
        memcpy(&bits, &v, 4);
        printf("%08x\n", bits);
    }
    return 0;
}
