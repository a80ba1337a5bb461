"""The GroupNorm statistics launches alone, us per call by hipGraph replay: ops.groupnorm_scale_shift (gn_partial_kernel, + gn_finalize_kernel
where the tensor is sliced) and ops.groupnorm_from_partials at the SD 64x64x320 level with B = 2, and the single-launch form at 8x8x1280.
Seven windows of 20 calls each: median and range.  A/B of two library builds: tools/ab_libs.sh "python tools/bench_groupnorm_stats.py"
parent.so - parent.so - ...   usage: bench_groupnorm_stats.py"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dgq_amd import ops
dev = torch.device("cuda:0")
R, WINDOWS = 20, 7


def replay_us(f):
    for _ in range(3): f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(R): f()
    g.replay(); torch.cuda.synchronize()
    ts = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / R)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


for (B, H, C, G) in ((2, 64, 320, 32), (2, 32, 640, 32), (2, 8, 1280, 32)):
    gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.1
    for dtype in (torch.float32, torch.bfloat16):
        x = (torch.randn(B, H * H, C, device=dev) * 1.3 + 0.2).to(dtype)
        med, lo, hi = replay_us(lambda: ops.groupnorm_scale_shift(x, B, H * H, C, G, 1e-5, gamma, beta))
        print("scale_shift   B=%d %dx%d C=%d %-8s %6.2f us  (%.2f .. %.2f)" % (B, H, H, C, str(dtype)[6:], med, lo, hi), flush=True)
    part = torch.randn(B * H * H // 16, C, 2, device=dev).abs()
    gn = dict(parts=[(part, C)], B=B, HW=H * H, C=C)
    med, lo, hi = replay_us(lambda: ops.groupnorm_from_partials(gn, G, 1e-5, gamma, beta))
    print("from_partials B=%d %dx%d C=%d %-8s %6.2f us  (%.2f .. %.2f)" % (B, H, H, C, "", med, lo, hi), flush=True)
