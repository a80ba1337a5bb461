"""Un-quantised attention of the 16-bit states on its two routes: the materialised torch formulation at the bottom of
quant_block.quant_attention_forward (matmul -> softmax -> matmul: the route without the switch) against dgq_attention_mfma16
(ops.attention_mfma16, one launch on the bf16 / f16 matrix cores), by the method of tools/bench_weight_only_mfma16.py.

Per distinct attention shape of an SD1.4 UNet call (CFG pair, 64x64 latents: 8 heads, head dim 40 / 80 / 160 / 160) and of an SDXL call
(128x128 latents, batch 1: head dim 64) and per dtype (bf16, f16): both routes timed by hipGraph replay (ITERS calls per replay, the two
graphs replayed alternately), and the rel-L2 of each against float64 softmax attention on the same 16-bit values; a third graph holds
the entry's 32-key-stage form (DGQ_ATTN16_KT=32 while it is captured; the default is 64 keys per stage below D = 160).  Then the tiny
UNet's accuracy figures of tests/test_gpu_attention_mfma16.py, and the whole weight-only SD UNet call per 16-bit state in three
configurations (set_weight_only_mfma16 alone, both switches, neither), graph-captured, alternating windows timed with device events.
GPU box only:  python tools/bench_attention_mfma16.py [--dtypes bfloat16 float16] [--no-whole] [--commit ID] [--out FILE]
                                                      (e.g. profiles/r14_attention_mfma16.txt)

--fp32 runs the fp32 state INSTEAD (profiles/r15_attention_mfma16_fp32.txt): per shape dgq_attention mode 0 (the exact fp32 MFMA kernel,
the route without the switch) against dgq_attention_mfma16_f32 (ops.attention_mfma16_f32: two-term bf16 splits on the bf16 matrix
cores) — every window of both, so that a row's difference can be held against the spread of the exact kernel's own windows —, the entry's
other LDS forms (DGQ_ATTN16F_FORM while they are captured), rel-L2 of both routes against float64; the tiny UNet's figures of
tests/test_gpu_attention_mfma16_fp32.py; the whole fp32-state weight-only SD call with set_weight_only_mfma16 on and the new switch off / on,
round by round."""
import argparse
import gc
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from dgq_amd import ops, synth
from bench_weight_only import build, graph_of, alternate_us, ITERS, ROUNDS

DTYPES = {"bfloat16": torch.bfloat16, "float16": torch.float16}
#: (arch, B, H, D, T, S, calls per UNet call): SD1.4 has 5 / 5 / 5 / 1 transformer blocks at 64² / 32² / 16² / 8², each one self- and one
#: cross-attention over the 77 text tokens; SDXL 10 transformer layers at 64² and 60 at 32²
SHAPES = [("sd", 2, 8, 40, 4096, 4096, 5), ("sd", 2, 8, 80, 1024, 1024, 5), ("sd", 2, 8, 160, 256, 256, 5), ("sd", 2, 8, 160, 64, 64, 1),
          ("sd", 2, 8, 40, 4096, 77, 5), ("sd", 2, 8, 80, 1024, 77, 5), ("sd", 2, 8, 160, 256, 77, 5), ("sd", 2, 8, 160, 64, 77, 1),
          ("sdxl", 1, 10, 64, 4096, 4096, 10), ("sdxl", 1, 20, 64, 1024, 1024, 60),
          ("sdxl", 1, 10, 64, 4096, 77, 10), ("sdxl", 1, 20, 64, 1024, 77, 60)]


def torch_route(q, k, v, H, D, scale):
    """the formulation quant_attention_forward runs for these tensors without the switch"""
    b, t, c = q.shape
    s = k.shape[1]
    qh, kh, vh = q.view(b, t, H, D).transpose(1, 2), k.view(b, s, H, D).transpose(1, 2), v.view(b, s, H, D).transpose(1, 2)
    p = torch.softmax(torch.matmul(qh, kh.transpose(-2, -1)) * scale, dim=-1)
    return torch.matmul(p, vh).transpose(1, 2).reshape(b, t, c)


def ref64(q, k, v, H, D, scale):
    """float64 softmax attention, one head at a time (4096² scores of 16 heads in float64 are 2 GiB)"""
    b, t, c = q.shape
    o = torch.empty(b, t, H, D, dtype=torch.float64, device=q.device)
    for h in range(H):
        sl = slice(h * D, (h + 1) * D)
        qd, kd, vd = q[..., sl].double(), k[..., sl].double(), v[..., sl].double()
        o[:, :, h] = torch.matmul(torch.softmax(torch.matmul(qd, kd.transpose(-2, -1)) * scale, dim=-1), vd)
    return o.view(b, t, c)


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def shapes_table(dtypes, p):
    names = [str(d).replace("torch.", "") for d in dtypes]
    p("attention shapes, q / k ~ N(0, 1), v ~ 1.3·N(0, 1) + 0.2, scale D^-0.5; times in us per call (median of %d alternating windows of "
      "%d calls, graph replay); rel-L2 against float64 on the same 16-bit values" % (ROUNDS, ITERS))
    p("%5s %2s %3s %4s %5s %5s %5s |" % ("arch", "B", "H", "D", "T", "S", "calls")
      + "|".join(" %9s %9s %5s %7s %9s %9s " % (n[:5] + " torch", "mfma16", "ratio", "(kt32)", "L2 torch", "L2 mfma16") for n in names))
    tot = {(n, a): [0.0, 0.0] for n in names for a in ("sd", "sdxl")}
    worst = {n: (0.0, None) for n in names}
    for arch, B, H, D, T, S, calls in SHAPES:
        cells = []
        for n, dt in zip(names, dtypes):
            g = torch.Generator(device="cuda").manual_seed(T + S + D)
            q = torch.randn(B, T, H * D, device="cuda", generator=g).to(dt)
            k = torch.randn(B, S, H * D, device="cuda", generator=g).to(dt)
            v = (1.3 * torch.randn(B, S, H * D, device="cuda", generator=g) + 0.2).to(dt)
            scale = D ** -0.5
            with torch.no_grad():
                o64 = ref64(q, k, v, H, D, scale)
                r_old, r_new = rel(torch_route(q, k, v, H, D, scale), o64), rel(ops.attention_mfma16(q, k, v, H, D, scale), o64)
                del o64
                g_old = graph_of(lambda: torch_route(q, k, v, H, D, scale))
                g_new = graph_of(lambda: ops.attention_mfma16(q, k, v, H, D, scale))
                os.environ["DGQ_ATTN16_KT"] = "32"
                try:
                    g_32 = graph_of(lambda: ops.attention_mfma16(q, k, v, H, D, scale))
                finally:
                    del os.environ["DGQ_ATTN16_KT"]
            us_old, us_new, us_32 = alternate_us([g_old, g_new, g_32], ITERS)
            tot[n, arch][0] += us_old * calls
            tot[n, arch][1] += us_new * calls
            if us_new / us_old > worst[n][0]:
                worst[n] = (us_new / us_old, (arch, D, T, S))
            cells.append(" %9.1f %9.1f %5.2f %7.1f %9.2e %9.2e " % (us_old, us_new, us_new / us_old, us_32, r_old, r_new))
            del g_old, g_new, g_32, q, k, v
            torch.cuda.empty_cache()
        p("%5s %2d %3d %4d %5d %5d %5d |" % (arch, B, H, D, T, S, calls) + "|".join(cells))
    for n in names:
        for a in ("sd", "sdxl"):
            p("%s, %s: sum over one UNet call (shape time x calls): torch %.1f us, mfma16 %.1f us (%.2fx)"
              % (n, a, tot[n, a][0], tot[n, a][1], tot[n, a][0] / tot[n, a][1]))
        p("%s: slowest ratio mfma16/torch %.3f at (arch, D, T, S) = %s" % (n, worst[n][0], worst[n][1]))
    return {n: tot[n, "sd"] for n in names}


def tiny_accuracy(dtypes, p):
    """the figures tests/test_gpu_attention_mfma16.py asserts on: arch tiny, weight-only W4, rel-L2 of each route's 16-bit-state output
    against the fp32-state output"""
    inp = synth.synth_inputs("tiny", 2, 1, 16)
    x, ctx, t = inp["sample"].cuda(), inp["encoder_hidden_states"].cuda(), torch.tensor(999)
    with torch.no_grad():
        for dt in dtypes:
            qnn = build("tiny", 4)                      # (per dtype: a second cast would round the first one's values again)
            y32 = qnn(x, t, ctx)[0].clone()
            qnn = qnn.to(dt)
            ys = []
            for flag in (False, True):
                qnn.set_attention_mfma16(flag)
                ys.append(qnn(x.to(dt), t, ctx.to(dt))[0].float())
            qnn.set_attention_mfma16(False)
            p("tiny UNet, weight-only W4, %s state: rel-L2 to the fp32-state output: torch formulation %.4e, dgq_attention_mfma16 %.4e"
              % (str(dt).replace("torch.", ""), rel(ys[0], y32), rel(ys[1], y32)))


def whole_call(dtypes, attn_us, p):
    a = synth.ARCH["sd"]
    x = synth.named_randn("latent", (2, 4, 64, 64), 1).cuda()
    ctx = synth.named_randn("ctx", (2, 77, a["ctx_dim"]), 100).cuda()
    t = torch.full((1,), 999, dtype=torch.int64, device="cuda")
    configs = [("wq_mfma16 alone", True, False), ("both switches", True, True), ("neither", False, False)]
    for dt in dtypes:
        n = str(dt).replace("torch.", "")
        qnn = build("sd", 4).to(dt)
        xd, cd = x.to(dt), ctx.to(dt)
        graphs, ys = [], []
        for _, wq16, at16 in configs:
            qnn.set_weight_only_mfma16(wq16)
            qnn.set_attention_mfma16(at16)
            with torch.no_grad():
                ys.append(qnn(xd, t, cd)[0].double())
                graphs.append(graph_of(lambda: qnn(xd, t, cd)))
        qnn.set_weight_only_mfma16(False)
        qnn.set_attention_mfma16(False)
        us = alternate_us(graphs, ITERS)
        p("%s state, sd W4 weight-only, whole UNet call (CFG pair, 64x64 latents; graph replay, median of %d alternating windows of %d calls): "
          % (n, ROUNDS, ITERS) + ", ".join("%s %.3f ms" % (c[0], u / 1e3) for c, u in zip(configs, us)))
        p("    both switches against wq_mfma16 alone: %.2fx (%.3f ms less); rel-L2 between their outputs %.2e; attention on the torch "
          "route by the table above: %.3f ms = %.0f %% of the wq_mfma16-alone call"
          % (us[0] / us[1], (us[0] - us[1]) / 1e3, rel(ys[1], ys[0]), attn_us[n][0] / 1e3, 100.0 * attn_us[n][0] / us[0]))
        del graphs, ys, qnn
        gc.collect()
        torch.cuda.empty_cache()


def alternate_rounds_us(graphs, per_replay):
    """µs per call of each graph in each of ROUNDS alternating windows"""
    ts = [[] for _ in graphs]
    for _ in range(ROUNDS):
        for i, g in enumerate(graphs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); g.replay(); e1.record()
            torch.cuda.synchronize()
            ts[i].append(e0.elapsed_time(e1) * 1e3 / per_replay)
    return ts


FORMS = {0: "64-key stages, two buffers", 1: "32-key stages, two buffers", 2: "widest stage, one buffer + second barrier"}


def fp32_shapes_table(p):
    """fp32 tensors: dgq_attention mode 0 against dgq_attention_mfma16_f32 (its default form per head dim, then forms 0 / 1 / 2 forced;
    D = 160 has no form 0: the request falls to form 1)"""
    import statistics
    med = statistics.median
    p("fp32 attention shapes, q / k ~ N(0, 1), v ~ 1.3·N(0, 1) + 0.2, scale D^-0.5; times in us per call (%d alternating windows of %d calls, "
      "graph replay): median [min .. max]; 'spread' = max − min of the exact kernel's own windows; 'over' = split median − exact median; "
      "rel-L2 against float64 on the same fp32 values; forms of the split entry: %s" % (ROUNDS, ITERS, FORMS))
    p("%5s %2s %3s %4s %5s %5s %5s | %28s | %28s | %5s %7s %7s | %8s %8s %8s | %9s %9s" % (
        "arch", "B", "H", "D", "T", "S", "calls", "exact (dgq_attention mode 0)", "split (default form)", "ratio", "spread", "over",
        "form 0", "form 1", "form 2", "L2 exact", "L2 split"))
    tot = {a: [0.0, 0.0] for a in ("sd", "sdxl")}
    slower = []
    for arch, B, H, D, T, S, calls in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(T + S + D)
        q = torch.randn(B, T, H * D, device="cuda", generator=g)
        k = torch.randn(B, S, H * D, device="cuda", generator=g)
        v = 1.3 * torch.randn(B, S, H * D, device="cuda", generator=g) + 0.2
        scale = D ** -0.5
        exact = lambda: ops.attention(q, k, v, H, D, scale, 0, 0, None, 8)
        split = lambda: ops.attention_mfma16_f32(q, k, v, H, D, scale)
        with torch.no_grad():
            o64 = ref64(q, k, v, H, D, scale)
            r_old, r_new = rel(exact(), o64), rel(split(), o64)
            del o64
            graphs = [graph_of(exact), graph_of(split)]
            for form in FORMS:
                os.environ["DGQ_ATTN16F_FORM"] = str(form)
                try:
                    graphs.append(graph_of(split))
                finally:
                    del os.environ["DGQ_ATTN16F_FORM"]
        ts = alternate_rounds_us(graphs, ITERS)
        us_old, us_new = med(ts[0]), med(ts[1])
        spread, over = max(ts[0]) - min(ts[0]), us_new - us_old
        tot[arch][0] += us_old * calls
        tot[arch][1] += us_new * calls
        if over > spread:
            slower.append((arch, D, T, S, over, spread))
        p("%5s %2d %3d %4d %5d %5d %5d | %8.1f [%7.1f .. %7.1f] | %8.1f [%7.1f .. %7.1f] | %5.2f %7.1f %+7.1f | %8.1f %8.1f %8.1f | %9.2e %9.2e"
          % (arch, B, H, D, T, S, calls, us_old, min(ts[0]), max(ts[0]), us_new, min(ts[1]), max(ts[1]), us_new / us_old, spread, over,
             med(ts[2]), med(ts[3]), med(ts[4]), r_old, r_new))
        del graphs, q, k, v
        torch.cuda.empty_cache()
    for a in ("sd", "sdxl"):
        p("fp32, %s: sum over one UNet call (shape time x calls): exact %.1f us, split %.1f us (%.2fx)" % (a, tot[a][0], tot[a][1], tot[a][0] / tot[a][1]))
    p("rows where the split entry is slower than the exact kernel by more than that kernel's own spread: %s" % (slower or "none"))
    return tot["sd"]


def fp32_tiny_accuracy(p):
    """the figures tests/test_gpu_attention_mfma16_fp32.py asserts on: arch tiny, weight-only W4, rel-L2 to the exact fp32 route of the
    fp32 state with the switch and of the f16 state on the torch formulation"""
    inp = synth.synth_inputs("tiny", 2, 1, 16)
    x, ctx, t = inp["sample"].cuda(), inp["encoder_hidden_states"].cuda(), torch.tensor(999)
    with torch.no_grad():
        qnn = build("tiny", 4)
        y_exact = qnn(x, t, ctx)[0].clone()
        qnn.set_attention_mfma16_fp32(True)
        y_split = qnn(x, t, ctx)[0].clone()
        qnn.set_attention_mfma16_fp32(False)
        y_f16 = qnn.half()(x.half(), t, ctx.half())[0].float()
    p("tiny UNet, weight-only W4: rel-L2 to the exact fp32 route: e_split (dgq_attention_mfma16_f32) %.4e, e_f16 (f16 state on the torch "
      "formulation) %.4e, e_split / e_f16 = %.2e" % (rel(y_split, y_exact), rel(y_f16, y_exact), rel(y_split, y_exact) / rel(y_f16, y_exact)))


def fp32_whole_call(attn_us, p):
    a = synth.ARCH["sd"]
    x = synth.named_randn("latent", (2, 4, 64, 64), 1).cuda()
    ctx = synth.named_randn("ctx", (2, 77, a["ctx_dim"]), 100).cuda()
    t = torch.full((1,), 999, dtype=torch.int64, device="cuda")
    qnn = build("sd", 4)
    qnn.set_weight_only_mfma16(True)
    graphs, ys = [], []
    for flag in (False, True):
        qnn.set_attention_mfma16_fp32(flag)
        with torch.no_grad():
            ys.append(qnn(x, t, ctx)[0].double())
            graphs.append(graph_of(lambda: qnn(x, t, ctx)))
    qnn.set_attention_mfma16_fp32(False)
    ts = alternate_rounds_us(graphs, ITERS)
    import statistics
    off, on = statistics.median(ts[0]), statistics.median(ts[1])
    p("fp32 state, sd W4 weight-only with wq_mfma16, whole UNet call (CFG pair, 64x64 latents; graph replay, %d alternating windows of %d calls):"
      % (ROUNDS, ITERS))
    p("    switch off, ms per round: " + " ".join("%.3f" % (u / 1e3) for u in ts[0]))
    p("    switch on,  ms per round: " + " ".join("%.3f" % (u / 1e3) for u in ts[1]))
    p("    medians: off %.3f ms, on %.3f ms: %.2fx (%.3f ms less); on below off in %d of %d rounds; rel-L2 between their outputs %.2e"
      % (off / 1e3, on / 1e3, off / on, (off - on) / 1e3, sum(b < a_ for a_, b in zip(*ts)), ROUNDS, rel(ys[1], ys[0])))
    p("    attention on the exact route by the table above: %.3f ms = %.0f %% of the switch-off call; on the split entry %.3f ms"
      % (attn_us[0] / 1e3, 100.0 * attn_us[0] / off, attn_us[1] / 1e3))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", nargs="+", default=list(DTYPES), choices=list(DTYPES))
    ap.add_argument("--no-whole", action="store_true", help="the shape table and the tiny UNet's accuracy only")
    ap.add_argument("--fp32", action="store_true", help="the fp32 state instead: dgq_attention mode 0 against dgq_attention_mfma16_f32")
    ap.add_argument("--commit", default="unknown", help="stamped into the report")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out or os.devnull, "w") as fh:
        p = lambda *a: (print(*a, flush=True), fh.write(" ".join(str(s) for s in a) + "\n"), fh.flush())
        p("device: %s\ncommit: %s" % (torch.cuda.get_device_name(0), args.commit))
        if args.fp32:
            attn_us = fp32_shapes_table(p)
            fp32_tiny_accuracy(p)
            if not args.no_whole:
                fp32_whole_call(attn_us, p)
        else:
            dts = [DTYPES[d] for d in args.dtypes]
            attn_us = shapes_table(dts, p)
            tiny_accuracy(dts, p)
            if not args.no_whole:
                whole_call(dts, attn_us, p)
