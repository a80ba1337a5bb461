"""Weight-only state (use_wq = True, use_aq = False) on its two routes: dgq_conv2d_wq from the packed W4 / W8 codes against
dgq_conv2d_f32w on the dequantised fp32 weight (QuantLayer.WEIGHT_ONLY_PACKED = False).  SD1.4 built in memory from the synthetic
state dict (no checkpoint written), weights self-initialised by their quantizers, 512x512 (64x64 latents), CFG pair.

Per distinct layer shape of one UNet call: both kernels timed by hipGraph replay (ITERS launches per replay, the two graphs replayed
alternately), outputs compared with torch.equal; the upsample shapes time the old kernel on the materialised interpolate (the old
route's interpolate itself is not in its figure).  Whole call: one UNet call per route, graph-captured, alternating windows timed
with device events; memory_allocated after the first forward of each route on a model holding only that route's weight copy.
GPU box only:  python tools/bench_weight_only.py [--bits 4 8] [--arch sd] [--res 64] [--batch 2] [--out FILE]
(--out: the report is also written to FILE, e.g. profiles/r07_weight_only_shapes.txt)"""
import argparse
import collections
import gc
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from dgq_amd import ops, synth
from dgq_amd.diffusers_rewrite import UNet2DConditionModel
from dgq_amd.quant import QuantModel, QuantLayer, Scaler, QMODE
from dgq_amd.quant import quant_layer as ql

PEAK_TF = 157.3            # fp32 matrix peak of the MI355X (AMD specification)
ITERS = 10
ROUNDS = 7


def build(arch, bits):
    unet = UNet2DConditionModel(arch)
    unet.load_state_dict(synth.synth_state_dict(arch, 0))
    qnn = QuantModel(model=unet, wq_params={"bits": bits, "channel_wise": True, "scaler": Scaler.MINMAX},
                     aq_params={"bits": 8, "channel_wise": False, "scaler": Scaler.MINMAX, "leaf_param": False},
                     softmax_aq_params={"softmax_a_bit": 8, "t2i_log_quant": False, "t2i_real_time": False, "t2i_start_peak": False,
                                        "log_max_1": False},
                     aq_mode=[QMODE.NORMAL.value, QMODE.QDIFF.value], tib_recon=False).cuda().eval()
    qnn.set_quant_state(True, False)
    qnn.disable_out_quantization()
    return qnn


def graph_of(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(ITERS):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def alternate_us(graphs, per_replay):
    """median µs per call of each graph, replayed alternately ROUNDS times"""
    ts = [[] for _ in graphs]
    for _ in range(ROUNDS):
        for i, g in enumerate(graphs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); g.replay(); e1.record()
            torch.cuda.synchronize()
            ts[i].append(e0.elapsed_time(e1) * 1e3 / per_replay)
    return [statistics.median(t) for t in ts]


def natural_fp32(pw, kh, kw):
    wq = pw.alpha[:, None] * (pw.codes.float() - pw.zp_true[:, None])
    return wq.view(pw.N, pw.C, kh, kw).permute(0, 2, 3, 1).reshape(pw.N, -1).contiguous()


def run(arch, bits, res, batch, out):
    p = lambda *a: (print(*a, flush=True), out.write(" ".join(str(s) for s in a) + "\n"))
    qnn = build(arch, bits)
    a = synth.ARCH[arch]
    x = synth.named_randn("latent", (batch, 4, res, res), 1).cuda()
    ctx = synth.named_randn("ctx", (batch, 77, a["ctx_dim"]), 100).cuda()
    t = torch.full((1,), 999, dtype=torch.int64, device="cuda")       # (on the device: the whole call is graph-captured)
    layers = [m for m in qnn.modules() if isinstance(m, QuantLayer) and m.use_wq]

    # record every dgq_conv2d_wq call of one forward
    calls = collections.OrderedDict()
    orig = ops.conv2d_wq

    def rec(xx, pw, kh, kw, stride, pad, upsample=False, geglu_rows=False):
        y = orig(xx, pw, kh, kw, stride, pad, upsample=upsample, geglu_rows=geglu_rows)
        M = y.numel() // pw.N
        key = (M, pw.N, pw.K, kh * kw, stride, bool(upsample), str(xx.dtype).replace("torch.", ""))
        if key not in calls:                     # (the geometry only: no activation is kept alive past the forward)
            calls[key] = dict(n=0, shape=tuple(xx.shape), dtype=xx.dtype, pw=pw, g=(kh, kw, stride, pad, upsample))
        calls[key]["n"] += 1
        return y
    ops.conv2d_wq = rec
    try:
        with torch.no_grad():
            torch.cuda.synchronize()
            y_new = qnn(x, t, ctx)[0].clone()
            torch.cuda.synchronize()
    finally:
        ops.conv2d_wq = orig
    mem_new = torch.cuda.memory_allocated()
    p("%s W%d, %dx%d latents, batch %d (CFG pair), fp32 activations: %d weight-only layer calls, %d distinct shapes"
      % (arch, bits, res, res, batch, sum(c["n"] for c in calls.values()), len(calls)))

    p("%7s %5s %6s %4s %3s %3s %5s | %9s %9s %6s | %7s %6s | %s" % ("M", "N", "K", "taps", "st", "up", "calls", "old us", "new us", "new/old",
                                                                      "TF/s", "%peak", "equal"))
    tot_old = tot_new = 0.0
    worst = (0.0, None)
    for key, c in calls.items():
        M, N, K, taps, stride, ups, _ = key
        kh, kw, st, pd, up = c["g"]
        pw = c["pw"]
        xx = torch.randn(c["shape"], device="cuda").to(c["dtype"])
        wn = natural_fp32(pw, kh, kw)
        xo = F.interpolate(xx, scale_factor=2.0, mode="nearest") if up else xx
        with torch.no_grad():
            y1 = ops.conv2d_wq(xx, pw, kh, kw, st, pd, upsample=up)
            y0 = ops.conv2d_f32w(xo, wn, pw.bias, kh, kw, st, pd)
            eq = torch.equal(y1, y0)
            g_old = graph_of(lambda: ops.conv2d_f32w(xo, wn, pw.bias, kh, kw, st, pd))
            g_new = graph_of(lambda: ops.conv2d_wq(xx, pw, kh, kw, st, pd, upsample=up))
        us_old, us_new = alternate_us([g_old, g_new], ITERS)
        tf = 2.0 * M * N * K / (us_new * 1e-6) / 1e12
        tot_old += us_old * c["n"]
        tot_new += us_new * c["n"]
        if us_new / us_old > worst[0]:
            worst = (us_new / us_old, key)
        p("%7d %5d %6d %4d %3d %3s %5d | %9.1f %9.1f %6.2f | %7.1f %5.1f%% | %s" % (M, N, K, taps, stride, "x" if ups else "", c["n"],
                                                                               us_old, us_new, us_new / us_old, tf, 100 * tf / PEAK_TF, eq))
        del g_old, g_new, wn, xo
    p("sum over the call (shape time x calls): old %.1f us, new %.1f us (%.2fx); slowest ratio new/old %.3f at %s"
      % (tot_old, tot_new, tot_old / tot_new, worst[0], worst[1]))
    calls.clear()
    gc.collect()
    torch.cuda.empty_cache()

    # memory: first forward of each route on a model holding only that route's weight copy
    mem_new_only = mem_new
    for m in layers:
        if m._pw is not None:
            m._pw._natural = None
    gc.collect(); torch.cuda.empty_cache()
    ql.WEIGHT_ONLY_PACKED = False
    with torch.no_grad():
        y_old = qnn(x, t, ctx)[0].clone()
        torch.cuda.synchronize()
    mem_old = torch.cuda.memory_allocated()
    ql.WEIGHT_ONLY_PACKED = True
    p("whole call: outputs torch.equal across the routes: %s" % torch.equal(y_new, y_old))
    p("memory_allocated after the first forward: old route %.3f GB, new route %.3f GB: new is %.3f GB lower"
      % (mem_old / 1e9, mem_new_only / 1e9, (mem_old - mem_new_only) / 1e9))

    # whole call timing: one graph per route, alternating windows
    graphs = []
    for packed in (False, True):
        ql.WEIGHT_ONLY_PACKED = packed
        with torch.no_grad():
            graphs.append(graph_of(lambda: qnn(x, t, ctx)))
    ql.WEIGHT_ONLY_PACKED = True
    us_old, us_new = alternate_us(graphs, ITERS)
    p("whole UNet call (graph replay, median of %d alternating windows of %d calls): old %.3f ms, new %.3f ms (%.2fx)"
      % (ROUNDS, ITERS, us_old / 1e3, us_new / 1e3, us_old / us_new))
    del graphs, qnn, layers
    gc.collect()
    torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="sd")
    ap.add_argument("--bits", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out or os.devnull, "w") as fh:
        dev = "device: %s" % torch.cuda.get_device_name(0)
        print(dev, flush=True)
        print(dev, file=fh)
        for b in args.bits:
            run(args.arch, b, args.res, args.batch, fh)
