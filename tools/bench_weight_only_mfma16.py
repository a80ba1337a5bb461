"""Weight-only state on its two packed-code routes: dgq_conv2d_wq (exact-fp32 MFMA, the default) against dgq_conv2d_wq_mfma16 (the
bf16 / f16 matrix cores, QuantLayer.weight_only_mfma16), by the method of tools/bench_weight_only.py: SD1.4 built in memory from the
synthetic state dict, weights self-initialised by their quantizers, 512x512 (64x64 latents), CFG pair.

Per distinct layer shape of one UNet call and per activation dtype (fp32, bf16, f16): both kernels timed by hipGraph replay (ITERS
launches per replay, the two graphs replayed alternately), and the rel-L2 between their outputs.  Whole call: one UNet call per route
and state, graph-captured, alternating windows timed with device events.
GPU box only:  python tools/bench_weight_only_mfma16.py [--bits 4 8] [--dtypes float32 bfloat16 float16] [--no-whole] [--commit ID]
                                                         [--out FILE]      (e.g. profiles/r13_weight_only_mfma16.txt)
DGQ_WQ16_TILE=32|64|128 in the environment forces one tile form of the new kernel for every shape (how wq16_pick was chosen).
--fused measures QuantModel.set_weight_only_fused instead (run_fused below): python tools/bench_weight_only_mfma16.py --fused --bits 4
--dtypes bfloat16 float32 --out FILE      (profiles/r20_weight_only_fused.txt)"""
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


def _unfused(x, pw, kh, kw, st, pd, upsample=False, geglu_rows=False, norm=None, ln=None, pre_act=0, residual=None, bias_rows=None, geglu=False):
    """what the model runs with the fused flag off for the same arguments: the torch operators around ops.conv2d_wq_mfma16"""
    import torch.nn.functional as F
    h = x
    if norm is not None:
        h = F.group_norm(h, norm[0], norm[2], norm[3], norm[1])
        pre_act = norm[4]
    if ln is not None:
        h = F.layer_norm(h, (h.shape[-1],), ln[1], ln[2], 1e-5)
    if pre_act:
        h = F.silu(h)
    y = ops.conv2d_wq_mfma16(h, pw, kh, kw, st, pd, upsample=upsample, geglu_rows=geglu_rows)
    if geglu:
        a, g = y.chunk(2, dim=-1)
        y = a * F.gelu(g)
    if bias_rows is not None:
        y = y + bias_rows[:, :, None, None]
    return y if residual is None else y + residual


def _rounds_ms(graphs, per_replay, rounds):
    """ms per call of each graph in each of `rounds` alternating rounds"""
    ts = [[] for _ in graphs]
    for _ in range(rounds):
        for i, g in enumerate(graphs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); g.replay(); e1.record()
            torch.cuda.synchronize()
            ts[i].append(e0.elapsed_time(e1) / per_replay)
    return ts


def _dispatches(fn):
    """device kernels of one eager call, counted by the torch profiler; None where the profiler gives no device events"""
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
        return n or None
    except Exception as e:                      # (a measurement that cannot be taken is reported as such, never guessed)
        print("dispatch count not measured: %r" % (e,))
        return None


def run_fused(arch, bits, res, batch, dtypes, whole, out):
    """QuantModel.set_weight_only_fused off against on, beside set_weight_only_mfma16 and the state's matrix-core attention switch:
    per distinct fused call of one UNet call the fused launch (with its dgq_layernorm_row_stats launch where it folds a LayerNorm:
    counted in full for every consumer, though the three projections of a self-attention share one) against the un-fused launch plus
    the torch operators it replaces; then the whole call in alternating rounds, the dispatch counts and the drift of the output."""
    import statistics
    p = lambda *a: (print(*a, flush=True), out.write(" ".join(str(s) for s in a) + "\n"))
    qnn = build(arch, bits)
    a = synth.ARCH[arch]
    x = synth.named_randn("latent", (batch, 4, res, res), 1).cuda()
    ctx = synth.named_randn("ctx", (batch, 77, a["ctx_dim"]), 100).cuda()
    t = torch.full((1,), 999, dtype=torch.int64, device="cuda")
    qnn.set_weight_only_mfma16(True)
    for dt in dtypes:
        name = str(dt).replace("torch.", "")
        qnn = qnn.to(dt)
        xd, cd = x.to(dt), ctx.to(dt)
        qnn.set_attention_mfma16(dt != torch.float32)
        qnn.set_attention_mfma16_fp32(dt == torch.float32)
        qnn.set_weight_only_fused(True)
        calls = collections.OrderedDict()
        orig = ops.conv2d_wq_mfma16_fused

        def rec(xx, pw, kh, kw, stride, pad, **kw_):
            y = orig(xx, pw, kh, kw, stride, pad, **kw_)
            on = lambda v: torch.is_tensor(v) or isinstance(v, tuple) or bool(v)
            what = "+".join(k for k in ("norm", "ln", "pre_act", "residual", "bias_rows", "geglu") if on(kw_.get(k)))
            if kw_.get("norm") is not None and kw_["norm"][4]:
                what = what.replace("norm", "norm+silu")
            key = (y.numel() // (pw.N // 2 if kw_.get("geglu") else pw.N), pw.N, pw.K, kh * kw, stride, what)
            if key not in calls:
                calls[key] = dict(n=0, shape=tuple(xx.shape), pw=pw, g=(kh, kw, stride, pad), kw={k: (v if not torch.is_tensor(v) else tuple(v.shape))
                                                                                              for k, v in kw_.items()})
            calls[key]["n"] += 1
            return y
        plain = collections.Counter()              # the layer calls that fold nothing: the un-fused entry, the same with the flag off or on
        orig_plain = ops.conv2d_wq_mfma16

        def rec_plain(xx, pw, kh, kw, stride, pad, **kw_):
            y = orig_plain(xx, pw, kh, kw, stride, pad, **kw_)
            plain[(y.numel() // pw.N, pw.N, pw.K, kh * kw, stride, bool(kw_.get("upsample")))] += 1
            return y
        ops.conv2d_wq_mfma16_fused, ops.conv2d_wq_mfma16 = rec, rec_plain
        try:
            with torch.no_grad():
                qnn(xd, t, cd)
                torch.cuda.synchronize()
        finally:
            ops.conv2d_wq_mfma16_fused, ops.conv2d_wq_mfma16 = orig, orig_plain
        p("%s W%d %s state, %dx%d latents, batch %d: %d fused calls per UNet call, %d distinct" % (arch, bits, name, res, res, batch,
                                                                                               sum(c["n"] for c in calls.values()), len(calls)))
        p("(the table lists the distinct FUSED calls, keyed by shape and by what is folded, not the 49 layer shapes of "
          "profiles/r13_weight_only_mfma16.txt: %d further layer calls of %d distinct shapes — layers with no neighbour to fold, such as the "
          "down / up sampling convolutions, shortcuts and the cross-attention k / v projections — fold nothing and run dgq_conv2d_wq_mfma16 itself, the same kernel "
          "with the flag off or on, so they have no row here)" % (sum(plain.values()), len(plain)))
        p("%7s %5s %6s %4s %3s %5s %-28s | %11s %9s %6s" % ("M", "N", "K", "taps", "st", "calls", "folded", "un-fused us", "fused us", "ratio"))
        tot = [0.0, 0.0]
        slower = 0
        for key, c in calls.items():
            M, N, K, taps, stride, what = key
            kh, kw, st, pd = c["g"]
            pw = c["pw"]
            xx = torch.randn(c["shape"], device="cuda").to(dt)
            kw_ = {}
            for k, v in c["kw"].items():
                if k == "norm" and v is not None:
                    kw_[k] = (v[0], v[1], v[2], v[3], v[4])
                elif k == "ln" and v is not None:
                    kw_[k] = v
                elif k in ("residual", "bias_rows") and v is not None:
                    kw_[k] = torch.randn(v, device="cuda").to(dt)
                    if k == "residual" and len(v) == 4:
                        kw_[k] = kw_[k].contiguous(memory_format=torch.channels_last)
                else:
                    kw_[k] = v
            ln = kw_.get("ln")

            def fused(xx=xx, pw=pw, kw_=kw_, ln=ln):
                if ln is not None:
                    kw2 = dict(kw_, ln=(ops.layernorm_row_stats(xx.reshape(-1, xx.shape[-1]), 1e-5), ln[1], ln[2]))
                    return ops.conv2d_wq_mfma16_fused(xx, pw, kh, kw, st, pd, **kw2)
                return ops.conv2d_wq_mfma16_fused(xx, pw, kh, kw, st, pd, **kw_)
            with torch.no_grad():
                g_old = graph_of(lambda: _unfused(xx, pw, kh, kw, st, pd, **kw_))
                g_new = graph_of(fused)
            us_old, us_new = alternate_us([g_old, g_new], ITERS)
            tot[0] += us_old * c["n"]
            tot[1] += us_new * c["n"]
            slower += us_new > us_old
            p("%7d %5d %6d %4d %3d %5d %-28s | %11.1f %9.1f %6.2f" % (M, N, K, taps, stride, c["n"], what, us_old, us_new, us_new / us_old))
            del g_old, g_new
        p("%s: sum over the call (shape time x calls): un-fused launch + torch operators %.1f us, fused %.1f us (%.2fx); the fused "
          "sum is slower in %d of the %d rows (ratio column)" % (name, tot[0], tot[1], tot[0] / max(tot[1], 1e-9), slower, len(calls)))
        calls.clear()
        gc.collect()
        torch.cuda.empty_cache()
        if whole:
            graphs, ys, nd = [], [], []
            for flag in (False, True):
                qnn.set_weight_only_fused(flag)
                with torch.no_grad():
                    ys.append(qnn(xd, t, cd)[0].double())
                    nd.append(_dispatches(lambda: qnn(xd, t, cd)))
                    graphs.append(graph_of(lambda: qnn(xd, t, cd)))
            rounds = 9
            ts = _rounds_ms(graphs, ITERS, rounds)
            med = [statistics.median(v) for v in ts]
            p("%s state, whole UNet call (CFG pair; graph replay, %d alternating rounds of %d calls), ms per call:" % (name, rounds, ITERS))
            p("    fused off: %s" % " ".join("%.3f" % v for v in ts[0]))
            p("    fused on:  %s" % " ".join("%.3f" % v for v in ts[1]))
            p("    medians %.3f -> %.3f ms (%.2fx, %.3f ms less); spread of the off route (max - min) %.3f ms; on faster than off in %d of %d "
              "rounds, by more than that spread in %d" % (med[0], med[1], med[0] / med[1], med[0] - med[1], max(ts[0]) - min(ts[0]),
                                                          sum(b < a_ for a_, b in zip(*ts)), rounds,
                                                          sum(a_ - b > max(ts[0]) - min(ts[0]) for a_, b in zip(*ts))))
            p("    device kernels per call: fused off %s, on %s;  rel-L2 drift of the output, on against off: %.2e"
              % (nd[0] if nd[0] else "not measured", nd[1] if nd[1] else "not measured", float((ys[1] - ys[0]).norm() / ys[0].norm())))
            del graphs
            gc.collect()
            torch.cuda.empty_cache()
    del qnn
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
    ap.add_argument("--fused", action="store_true",
                    help="measure QuantModel.set_weight_only_fused off against on instead (e.g. --bits 4 --dtypes bfloat16 float32 "
                         "--out profiles/r20_weight_only_fused.txt)")
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
            (run_fused if args.fused else run)(args.arch, b, args.res, args.batch, [DTYPES[d] for d in args.dtypes], not args.no_whole, fh)
