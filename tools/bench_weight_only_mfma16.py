"""Weight-only state on its two packed-code routes: dgq_conv2d_wq (exact-fp32 MFMA, the default) against dgq_conv2d_wq_mfma16 (the
bf16 / f16 matrix cores, QuantLayer.weight_only_mfma16), by the method of tools/bench_weight_only.py: SD1.4 built in memory from the
synthetic state dict, weights self-initialised by their quantizers, 512x512 (64x64 latents), CFG pair.

Per distinct layer shape of one UNet call and per activation dtype (fp32, bf16, f16): both kernels timed by hipGraph replay (ITERS
launches per replay, the two graphs replayed alternately), and the rel-L2 between their outputs.  Whole call: one UNet call per route
and state, graph-captured, alternating windows timed with device events.
GPU box only:  python tools/bench_weight_only_mfma16.py [--bits 4 8] [--dtypes float32 bfloat16 float16] [--no-whole] [--commit ID]
                                                         [--out FILE]      (e.g. profiles/r13_weight_only_mfma16.txt)
DGQ_WQ16_TILE=32|64|128 in the environment forces one tile form of the new kernel for every shape (how wq16_pick was chosen)."""
import argparse
import collections
import gc
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from dgq_amd import ops, synth
from dgq_amd.quant import QuantLayer
from bench_weight_only import build, graph_of, alternate_us, ITERS, ROUNDS

DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}


def run(arch, bits, res, batch, dtypes, whole, out):
    p = lambda *a: (print(*a, flush=True), out.write(" ".join(str(s) for s in a) + "\n"))
    qnn = build(arch, bits)
    a = synth.ARCH[arch]
    x = synth.named_randn("latent", (batch, 4, res, res), 1).cuda()
    ctx = synth.named_randn("ctx", (batch, 77, a["ctx_dim"]), 100).cuda()
    t = torch.full((1,), 999, dtype=torch.int64, device="cuda")
    layers = [m for m in qnn.modules() if isinstance(m, QuantLayer) and m.use_wq]

    # record every dgq_conv2d_wq call of one forward (the shapes are those of every state)
    calls = collections.OrderedDict()
    orig = ops.conv2d_wq

    def rec(xx, pw, kh, kw, stride, pad, upsample=False, geglu_rows=False):
        y = orig(xx, pw, kh, kw, stride, pad, upsample=upsample, geglu_rows=geglu_rows)
        key = (y.numel() // pw.N, pw.N, pw.K, kh * kw, stride, bool(upsample))
        if key not in calls:
            calls[key] = dict(n=0, shape=tuple(xx.shape), pw=pw, g=(kh, kw, stride, pad, upsample))
        calls[key]["n"] += 1
        return y
    ops.conv2d_wq = rec
    try:
        with torch.no_grad():
            qnn(x, t, ctx)
            torch.cuda.synchronize()
    finally:
        ops.conv2d_wq = orig
    p("%s W%d, %dx%d latents, batch %d (CFG pair): %d weight-only layer calls, %d distinct shapes, all eligible: %s; tile forced: %s"
      % (arch, bits, res, res, batch, sum(c["n"] for c in calls.values()), len(calls),
         all(m.packed_weight().mfma16_eligible() for m in layers), os.environ.get("DGQ_WQ16_TILE", "no")))
    names = [str(d).replace("torch.", "") for d in dtypes]
    p("%7s %5s %6s %4s %3s %3s %5s |" % ("M", "N", "K", "taps", "st", "up", "calls")
      + "|".join(" %9s %9s %5s %8s " % (n[:5] + " wq", "mfma16", "ratio", "rel-L2") for n in names))
    tot = {n: [0.0, 0.0] for n in names}
    worst = {n: (0.0, None) for n in names}
    for key, c in calls.items():
        M, N, K, taps, stride, ups = key
        kh, kw, st, pd, up = c["g"]
        pw = c["pw"]
        line = "%7d %5d %6d %4d %3d %3s %5d |" % (M, N, K, taps, stride, "x" if ups else "", c["n"])
        cells = []
        for n, dt in zip(names, dtypes):
            xx = torch.randn(c["shape"], device="cuda").to(dt)
            with torch.no_grad():
                y0 = ops.conv2d_wq(xx, pw, kh, kw, st, pd, upsample=up).double()
                y1 = ops.conv2d_wq_mfma16(xx, pw, kh, kw, st, pd, upsample=up).double()
                rel = float((y1 - y0).norm() / y0.norm())
                g_old = graph_of(lambda: ops.conv2d_wq(xx, pw, kh, kw, st, pd, upsample=up))
                g_new = graph_of(lambda: ops.conv2d_wq_mfma16(xx, pw, kh, kw, st, pd, upsample=up))
            us_old, us_new = alternate_us([g_old, g_new], ITERS)
            tot[n][0] += us_old * c["n"]
            tot[n][1] += us_new * c["n"]
            if us_new / us_old > worst[n][0]:
                worst[n] = (us_new / us_old, key)
            cells.append(" %9.1f %9.1f %5.2f %8.1e " % (us_old, us_new, us_new / us_old, rel))
            del g_old, g_new
        p(line + "|".join(cells))
    for n in names:
        p("%s: sum over the call (shape time x calls): wq %.1f us, mfma16 %.1f us (%.2fx); slowest ratio mfma16/wq %.3f at %s"
          % (n, tot[n][0], tot[n][1], tot[n][0] / tot[n][1], worst[n][0], worst[n][1]))
    calls.clear()
    gc.collect()
    torch.cuda.empty_cache()

    if whole:
        for n, dt in zip(names, dtypes):
            qnn = qnn.to(dt)
            xd, cd = x.to(dt), ctx.to(dt)
            graphs, ys = [], []
            for flag in (False, True):
                qnn.set_weight_only_mfma16(flag)
                with torch.no_grad():
                    ys.append(qnn(xd, t, cd)[0].double())
                    graphs.append(graph_of(lambda: qnn(xd, t, cd)))
            qnn.set_weight_only_mfma16(False)
            us_old, us_new = alternate_us(graphs, ITERS)
            p("%s state, whole UNet call (graph replay, median of %d alternating windows of %d calls): wq %.3f ms, mfma16 %.3f ms (%.2fx); "
              "rel-L2 between the outputs %.2e" % (n, ROUNDS, ITERS, us_old / 1e3, us_new / 1e3, us_old / us_new,
                                                   float((ys[1] - ys[0]).norm() / ys[0].norm())))
            del graphs
            gc.collect()
            torch.cuda.empty_cache()
    del qnn, layers
    gc.collect()
    torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="sd")
    ap.add_argument("--bits", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--dtypes", nargs="+", default=list(DTYPES), choices=list(DTYPES))
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--no-whole", action="store_true", help="the shape table only")
    ap.add_argument("--commit", default="unknown", help="stamped into the report")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out or os.devnull, "w") as fh:
        head = "device: %s\ncommit: %s" % (torch.cuda.get_device_name(0), args.commit)
        print(head, flush=True)
        print(head, file=fh)
        for b in args.bits:
            run(args.arch, b, args.res, args.batch, [DTYPES[d] for d in args.dtypes], not args.no_whole, fh)
