#!/usr/bin/env python3
"""Measures the real-time per-row activation mode (UniformAffineQuantizer(real_time=True), dgq_act_row_params) against the calibrated
c2 tables, same box, same process — profiles/r08_realtime_act.txt:

  * the SD-size synthetic model, CFG pair, fp32: ms per step (hipGraph replay, median of the windows), library launches per step
    (entry calls of one eager step), model_ready seconds, device memory after load — calibrated c2 (time-aware g16 tables) and
    real-time (weight-only checkpoint);
  * the row-parameter kernels alone, replayed from a hipGraph: µs and input bytes / time at four SD shapes.

    python tools/profile_realtime_act.py --out profiles/r08_realtime_act.txt --stamp "$(git rev-parse --short HEAD)"

--block measures the real-time BLOCK mode (real_time_block=32: dgq_quant_act_block + dgq_gemm_blockq) instead — profiles/r12_realtime_block.txt:
the two new kernels alone at SD layer shapes (beside the same layer in the row mode), and the step time of the three modes
(calibrated c2, real-time rows, real-time blocks) in ALTERNATING rounds of one process on one box.

    python tools/profile_realtime_act.py --block --out profiles/r12_realtime_block.txt

--mx measures the real-time MXFP6 mode (real_time_format="mxfp6": dgq_quant_act_mx6 + dgq_gemm_mx6, W4A6) — profiles/r17_realtime_mxfp6.txt:
per SD layer shape the new pair of launches against the block mode's pair and the row mode's layer call at A6, the SD step in the three
real-time modes, all in ALTERNATING rounds of hipGraph replays in one process on one box, and the rel-L2 of the tiny UNet's output in
each mode against the same model with un-quantised activations.

    python tools/profile_realtime_act.py --mx --out profiles/r17_realtime_mxfp6.txt

--mxint8 measures the real-time MXINT8 mode (real_time_format="mxint8": dgq_quant_act_mxint8 + dgq_gemm_mxint8, W4A8) the same way, against
the int8 block and row modes — profiles/r22_realtime_mxint8.txt:
    python tools/profile_realtime_act.py --mxint8 --out profiles/r22_realtime_mxint8.txt

--mx-w8 measures W8 layers under both MX formats (real_time_mx_w8=True: dgq_gemm_mxw8 on the two-plane weight image, W8A6 / W8A8) against
the route they take with the flag off (dgq_gemm_blockq at W8), which is captured twice: its own spread is the yardstick of "level" —
profiles/r24_realtime_mx_w8.txt:
    python tools/profile_realtime_act.py --mx-w8 --out profiles/r24_realtime_mx_w8.txt
"""
import argparse
import gc
import os
import statistics
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stamp_default():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return "unknown"


def replayed_us(torch, issue, rep=20, rounds=5):
    """median µs of one ``issue()`` out of ``rep`` back-to-back calls replayed from a hipGraph (launch gaps of eager calls excluded)"""
    issue()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(rep):
            issue()
    g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / rep)
    return statistics.median(out)


def kernel_table(torch, ops, dev, lines):
    lines.append("row-parameter kernels alone (fp32 input, A8; %d calls per hipGraph replay, median of 5 replays)" % 20)
    lines.append("%-28s %8s %10s %12s %9s" % ("shape", "launches", "us / call", "input MB", "GB/s"))
    g = torch.Generator().manual_seed(0)
    shapes = [("linear 8192 x 320", (8192, 1, 1, 320, 1, 1, 1, 0)), ("linear 8192 x 1280", (8192, 1, 1, 1280, 1, 1, 1, 0)),
              ("conv 2x320x64x64 k3", (2, 64, 64, 320, 3, 3, 1, 1)), ("conv 2x1280x16x16 k3", (2, 16, 16, 1280, 3, 3, 1, 1))]
    for name, geom in shapes:
        B, H, W, C = geom[:4]
        x = torch.randn(B, H, W, C, generator=g).to(dev)
        us = replayed_us(torch, lambda: ops.act_row_params(x, geom, 8))
        nbytes = x.numel() * 4
        lines.append("%-28s %8d %10.2f %12.2f %9.0f" % (name, 1 if geom[4:] == (1, 1, 1, 0) else 2, us, nbytes / 1e6, nbytes / us / 1e3))


def block_kernel_table(torch, ops, dev, lines):
    """dgq_quant_act_block and dgq_gemm_blockq alone at SD 64 x 64 / 32 x 32 layer shapes, beside the whole layer in the row mode"""
    lines.append("block-mode kernels alone (fp32, W4A8; %d calls per hipGraph replay, median of 5 replays); row mode: the whole layer call" % 20)
    lines.append("%-34s %12s %12s %12s %14s" % ("layer", "quantiser us", "GEMM us", "block us", "row-mode us"))
    g = torch.Generator().manual_seed(0)
    from dgq_amd import synth
    shapes = [("linear 8192x320 -> 320", (8192, 1, 1, 320, 1, 1, 1, 0), 320), ("linear 8192x320 -> 2560", (8192, 1, 1, 320, 1, 1, 1, 0), 2560),
              ("linear 8192x1280 -> 320", (8192, 1, 1, 1280, 1, 1, 1, 0), 320), ("linear 2048x640 -> 640", (2048, 1, 1, 640, 1, 1, 1, 0), 640),
              ("linear 2048x2560 -> 640", (2048, 1, 1, 2560, 1, 1, 1, 0), 640),
              ("conv3x3 2x320x64x64 -> 320", (2, 64, 64, 320, 3, 3, 1, 1), 320), ("conv3x3 s2 2x320x64x64 -> 320", (2, 64, 64, 320, 3, 3, 2, 1), 320),
              ("conv3x3 2x640x32x32 -> 640", (2, 32, 32, 640, 3, 3, 1, 1), 640), ("conv3x3 2x1280x32x32 -> 640", (2, 32, 32, 1280, 3, 3, 1, 1), 640)]
    for name, geom, N in shapes:
        B, H, W, C, kh, kw, stride, pad = geom
        taps = kh * kw
        w = torch.randn(N, C * taps, generator=g) * (C * taps) ** -0.5
        wd, wz = synth.channel_minmax(w, 4)
        pw = ops.PackedWeight(w.to(dev), wd.to(dev), wz.to(dev), None, torch.zeros(N).to(dev), 4, C, taps)
        blk, row = ops.BlockActBinding(pw, 8), ops.DynamicActBinding(pw, 8)
        x = (torch.randn(B, H, W, C, generator=g) * 1.3 + 0.2).to(dev)
        ldt = blk.Kp // 32 if taps == 1 else C // 32
        q = ops.quant_act_block(x, geom, 8, ldt=ldt)
        us_q = replayed_us(torch, lambda: ops.quant_act_block(x, geom, 8, ldt=ldt))
        us_g = replayed_us(torch, lambda: ops.gemm_blockq(q, geom, blk, torch.float32))
        if taps == 1:
            x2 = x.view(B, C)
            us_r = replayed_us(torch, lambda: ops.quant_linear(x2, row))
        else:
            xn = x.permute(0, 3, 1, 2)
            us_r = replayed_us(torch, lambda: ops.quant_conv2d(xn, row, kh, kw, stride, pad, gn_out=False))
        lines.append("%-34s %12.2f %12.2f %12.2f %14.2f" % (name, us_q, us_g, us_q + us_g, us_r))


def captured(torch, issue, rep=20):
    """a hipGraph of ``rep`` back-to-back ``issue()`` calls, warmed"""
    issue()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(rep):
            issue()
    g.replay()
    torch.cuda.synchronize()
    return g


def alternating_us(torch, graphs, rep=20, rounds=7):
    """median µs per call of each graph of ``graphs`` (name -> hipGraph of ``rep`` calls), replayed in alternating rounds"""
    out = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) * 1e3 / rep)
    return {k: statistics.median(v) for k, v in out.items()}


def mx_kernel_table(torch, ops, dev, lines, fmt="mxfp6"):
    """the MX quantiser + GEMM of ``fmt`` (mxfp6 at A6, mxint8 at A8) against dgq_quant_act_block + dgq_gemm_blockq and the row mode's layer
    call at the same bit width, per SD layer shape"""
    from dgq_amd import synth
    ab = 8 if fmt == "mxint8" else 6
    quant_mx, gemm_mx = (ops.quant_act_mxint8, ops.gemm_mxint8) if fmt == "mxint8" else (ops.quant_act_mx6, ops.gemm_mx6)
    lines.append("layer shapes of an SD1.4 step (fp32, W4A%d; 20 calls" % ab + " per hipGraph replay, median of 7 ALTERNATING rounds: mx quantiser, mx GEMM,")
    lines.append("block quantiser, block GEMM, row-mode layer, mx quantiser, ...); mx / block = the two launches of the mode added")
    lines.append("%-34s %9s %9s %9s %9s %9s %9s %9s %9s" % ("layer", "mx q us", "mx g us", "mx us", "blk q us", "blk g us", "block us", "row us", "mx/block"))
    g = torch.Generator().manual_seed(0)
    shapes = [("linear 8192x320 -> 320", (8192, 1, 1, 320, 1, 1, 1, 0), 320), ("linear 8192x320 -> 2560", (8192, 1, 1, 320, 1, 1, 1, 0), 2560),
              ("linear 8192x1280 -> 320", (8192, 1, 1, 1280, 1, 1, 1, 0), 320), ("linear 2048x640 -> 640", (2048, 1, 1, 640, 1, 1, 1, 0), 640),
              ("linear 2048x2560 -> 640", (2048, 1, 1, 2560, 1, 1, 1, 0), 640), ("linear 512x1280 -> 1280", (512, 1, 1, 1280, 1, 1, 1, 0), 1280),
              ("linear 154x768 -> 320", (154, 1, 1, 768, 1, 1, 1, 0), 320),
              ("conv3x3 2x320x64x64 -> 320", (2, 64, 64, 320, 3, 3, 1, 1), 320), ("conv3x3 s2 2x320x64x64 -> 320", (2, 64, 64, 320, 3, 3, 2, 1), 320),
              ("conv3x3 2x640x32x32 -> 640", (2, 32, 32, 640, 3, 3, 1, 1), 640), ("conv3x3 2x1280x32x32 -> 640", (2, 32, 32, 1280, 3, 3, 1, 1), 640),
              ("conv3x3 2x1280x16x16 -> 1280", (2, 16, 16, 1280, 3, 3, 1, 1), 1280), ("conv3x3 2x2560x8x8 -> 1280", (2, 8, 8, 2560, 3, 3, 1, 1), 1280)]
    slower = []
    for name, geom, N in shapes:
        B, H, W, C, kh, kw, stride, pad = geom
        taps = kh * kw
        w = torch.randn(N, C * taps, generator=g) * (C * taps) ** -0.5
        wd, wz = synth.channel_minmax(w, 4)
        pw = ops.PackedWeight(w.to(dev), wd.to(dev), wz.to(dev), None, torch.zeros(N).to(dev), 4, C, taps)
        mxb, blk, row = ops.MxActBinding(pw, fmt), ops.BlockActBinding(pw, ab), ops.DynamicActBinding(pw, ab)
        x = (torch.randn(B, H, W, C, generator=g) * 1.3 + 0.2).to(dev)
        pad_k = blk.Kp // 32 if taps == 1 else C // 32
        qm, qb = quant_mx(x, geom, lds=pad_k), ops.quant_act_block(x, geom, ab, ldt=pad_k)
        x2, xn = x.view(B * H * W, C), x.permute(0, 3, 1, 2)
        row_call = (lambda: ops.quant_linear(x2, row)) if taps == 1 else (lambda: ops.quant_conv2d(xn, row, kh, kw, stride, pad, gn_out=False))
        graphs = dict(mq=captured(torch, lambda: quant_mx(x, geom, lds=pad_k)), mg=captured(torch, lambda: gemm_mx(qm, geom, mxb, torch.float32)),
                      bq=captured(torch, lambda: ops.quant_act_block(x, geom, ab, ldt=pad_k)), bg=captured(torch, lambda: ops.gemm_blockq(qb, geom, blk, torch.float32)),
                      row=captured(torch, row_call))
        us = alternating_us(torch, graphs)
        m, b = us["mq"] + us["mg"], us["bq"] + us["bg"]
        lines.append("%-34s %9.2f %9.2f %9.2f %9.2f %9.2f %9.2f %9.2f %9.2f" % (name, us["mq"], us["mg"], m, us["bq"], us["bg"], b, us["row"], m / b))
        if m > b:
            slower.append(name)
        del graphs
    lines.append("shapes where the MX pair is slower than the block pair: %s" % (", ".join(slower) if slower else "none"))


#: the rows of mx_kernel_table, the SD 8x8 / 16x16 convolutions not among them, and the two 9-K-tile shapes of the tests (tiny UNet, route test)
KSPLIT_SHAPES = [("linear 8192x320 -> 320", (8192, 1, 1, 320, 1, 1, 1, 0), 320, False), ("linear 8192x320 -> 2560", (8192, 1, 1, 320, 1, 1, 1, 0), 2560, False),
                 ("linear 8192x1280 -> 320", (8192, 1, 1, 1280, 1, 1, 1, 0), 320, False), ("linear 2048x640 -> 640", (2048, 1, 1, 640, 1, 1, 1, 0), 640, False),
                 ("linear 2048x2560 -> 640", (2048, 1, 1, 2560, 1, 1, 1, 0), 640, False), ("linear 512x1280 -> 1280", (512, 1, 1, 1280, 1, 1, 1, 0), 1280, False),
                 ("linear 154x768 -> 320", (154, 1, 1, 768, 1, 1, 1, 0), 320, False),
                 ("conv3x3 2x320x64x64 -> 320", (2, 64, 64, 320, 3, 3, 1, 1), 320, False), ("conv3x3 s2 2x320x64x64 -> 320", (2, 64, 64, 320, 3, 3, 2, 1), 320, False),
                 ("conv3x3 2x640x32x32 -> 640", (2, 32, 32, 640, 3, 3, 1, 1), 640, False), ("conv3x3 2x1280x32x32 -> 640", (2, 32, 32, 1280, 3, 3, 1, 1), 640, False),
                 ("conv3x3 2x1280x16x16 -> 1280", (2, 16, 16, 1280, 3, 3, 1, 1), 1280, False), ("conv3x3 2x2560x8x8 -> 1280", (2, 8, 8, 2560, 3, 3, 1, 1), 1280, False),
                 ("conv3x3 2x1280x8x8 -> 1280", (2, 8, 8, 1280, 3, 3, 1, 1), 1280, False), ("conv3x3 2x2560x16x16 -> 1280", (2, 16, 16, 2560, 3, 3, 1, 1), 1280, False),
                 ("conv3x3 2x1920x16x16 -> 1280", (2, 16, 16, 1920, 3, 3, 1, 1), 1280, False), ("conv3x3 ups 2x1280x8x8 -> 1280", (2, 16, 16, 1280, 3, 3, 1, 1), 1280, True),
                 ("conv3x3 s2 2x640x32x32 -> 640", (2, 32, 32, 640, 3, 3, 2, 1), 640, False), ("conv3x3 s2 2x1280x16x16 -> 1280", (2, 16, 16, 1280, 3, 3, 2, 1), 1280, False),
                 ("conv3x3 2x256x8x8 -> 128 (tiny)", (2, 8, 8, 256, 3, 3, 1, 1), 128, False), ("conv3x3 2x256x4x4 -> 64 (test)", (2, 4, 4, 256, 3, 3, 1, 1), 64, False)]


def mx_ksplit_table(torch, ops, dev, lines, fmt, sweep=(2, 4, 8, 16)):
    """the MX GEMM of ``fmt`` per shape: un-split (captured twice: the spread of its own medians), forced K splits, and the plan's route —
    the split figures are the PAIR of launches (GEMM + combine); alternating rounds of hipGraph replays"""
    from dgq_amd import _lib, synth
    quant_mx, gemm_mx = (ops.quant_act_mxint8, ops.gemm_mxint8) if fmt == "mxint8" else (ops.quant_act_mx6, ops.gemm_mx6)
    lines += ["", "%s GEMM alone per shape (fp32 out; 20 calls per hipGraph replay, median of 7 ALTERNATING rounds): un-split twice (S=1, S=1'),"
              % fmt.upper(), "forced splits (GEMM + combine), the plan's route; tiles = 64x64 output tiles, nkt = K tiles of 256; MB = the plan's workspace",
              "%-34s %6s %4s %8s %8s %s %5s %8s %7s" % ("layer", "tiles", "nkt", "S=1 us", "S=1' us", " ".join("%8s" % ("S=%d us" % s) for s in sweep), "plan", "plan us", "MB")]
    g = torch.Generator().manual_seed(0)
    lib, worst_ws = _lib.load(), 0
    for name, geom, N, ups in KSPLIT_SHAPES:
        B, H, W, C, kh, kw, stride, pad = geom
        taps = kh * kw
        w = torch.randn(N, C * taps, generator=g) * (C * taps) ** -0.5
        wd, wz = synth.channel_minmax(w, 4)
        mxb = ops.MxActBinding(ops.PackedWeight(w.to(dev), wd.to(dev), wz.to(dev), None, torch.zeros(N).to(dev), 4, C, taps), fmt)
        sh = 1 if ups else 0
        x = (torch.randn(B, H >> sh, W >> sh, C, generator=g) * 1.3 + 0.2).to(dev)
        qm = quant_mx(x, geom, ups=ups, lds=mxb.Kp // 32 if taps == 1 else C // 32)
        M = B * ((H + 2 * pad - kh) // stride + 1) * ((W + 2 * pad - kw) // stride + 1)
        tiles, nkt = ((M + 63) // 64) * ((N + 63) // 64), (C * taps // 32 + 7) // 8
        call = lambda s: captured(torch, lambda: gemm_mx(qm, geom, mxb, torch.float32, ups=ups, ksplit=s))
        plan = lib.dgq_gemm_mx_plan_splits(M, N, mxb.Kp, ops.WORKSPACE_BYTES)
        graphs = {"a": call(1), "b": call(1)}
        graphs.update({s: call(s) for s in sweep if s <= nkt})
        graphs["plan"] = call(1 if plan == 1 else None)
        us = alternating_us(torch, graphs)
        ws = lib.dgq_gemm_mx_workspace_bytes(M, N, mxb.Kp)
        worst_ws = max(worst_ws, ws)
        lines.append("%-34s %6d %4d %8.2f %8.2f %s %5d %8.2f %7.1f" % (name, tiles, nkt, us["a"], us["b"], " ".join("%8.2f" % us[s] if s in us else "%8s" % "-" for s in sweep),
                                                                  plan, us["plan"], ws / 2 ** 20))
        del graphs
    lines.append("largest plan workspace over these shapes: %.1f MB of ops.WORKSPACE_BYTES = %d MB" % (worst_ws / 2 ** 20, ops.WORKSPACE_BYTES >> 20))


def mx_rows_table(torch, ops, dev, lines, fmt, sweep=(1, 2, 4, 8, 16)):
    """the Linear layer of ``fmt`` in one launch (ops.gemm_mx_rows) against its quantiser + GEMM pair per SD Linear shape: the pair captured
    twice (the spread of its own medians), forced column splits, the plan's choice; alternating rounds of hipGraph replays"""
    from dgq_amd import _lib, synth
    s_ = {"mxfp6": "mx6", "mxint8": "mxint8", "mxfp4": "mx4"}[fmt]
    quant_mx, gemm_mx = getattr(ops, "quant_act_" + s_), getattr(ops, "gemm_" + s_)
    lines += ["", "%s Linear layers, one launch (dgq_gemm_mx_rows) against quantiser + GEMM (fp32; 20 calls per hipGraph replay, median of 7 ALTERNATING"
              % fmt.upper(), "rounds): the pair twice (pair, pair'), forced column splits, the plan's choice (0: shape not taken, then = pair)",
              "%-28s %8s %8s %s %5s %8s %9s" % ("layer", "pair us", "pair' us", " ".join("%8s" % ("S=%d us" % s) for s in sweep), "plan", "plan us", "plan/pair")]
    g = torch.Generator().manual_seed(0)
    lib = _lib.load()
    for name, geom, N, _ups in [r for r in KSPLIT_SHAPES if r[0].startswith("linear")]:
        M, C = geom[0], geom[3]
        w = torch.randn(N, C, generator=g) * C ** -0.5
        wd, wz = synth.channel_minmax(w, 4)
        mxb = ops.MxActBinding(ops.PackedWeight(w.to(dev), wd.to(dev), wz.to(dev), None, torch.zeros(N).to(dev), 4, C, 1), fmt)
        x = (torch.randn(M, C, generator=g) * 1.3 + 0.2).to(dev)
        plan = lib.dgq_gemm_mx_rows_plan(M, N, mxb.Kp, mxb.abits)
        if lib.dgq_gemm_mx_rows_plan(M, 1 << 20, mxb.Kp, mxb.abits) == 0:       # the panel does not fit: nothing to time
            lines.append("%-28s not taken (LDS)" % name)
            continue
        pair = lambda: captured(torch, lambda: gemm_mx(quant_mx(x, geom, lds=mxb.Kp // 32), geom, mxb, torch.float32))
        graphs = {"a": pair(), "b": pair()}
        graphs.update({s: captured(torch, lambda s=s: ops.gemm_mx_rows(x, [mxb], col_splits=s)) for s in sweep})
        if plan:
            graphs["plan"] = captured(torch, lambda: ops.gemm_mx_rows(x, [mxb]))
        us = alternating_us(torch, graphs)
        pl = us.get("plan", us["a"])
        lines.append("%-28s %8.2f %8.2f %s %5d %8.2f %9.3f" % (name, us["a"], us["b"], " ".join("%8.2f" % us[s] for s in sweep), plan, pl, pl / us["a"]))
        del graphs


def mxw8_kernel_table(torch, ops, dev, lines, fmt):
    """dgq_gemm_mxw8 under ``fmt`` activations, by the plan's K split as the layers run it, against dgq_gemm_blockq at W8 and the same bit
    width (captured twice), with both quantisers, per SD layer shape of mx_kernel_table"""
    from dgq_amd import synth
    ab = 8 if fmt == "mxint8" else 6
    quant_mx = ops.quant_act_mxint8 if fmt == "mxint8" else ops.quant_act_mx6
    lines += ["", "layer shapes of an SD1.4 step (fp32, W8A%d, %s activations; 20 calls per hipGraph replay, median of 7 ALTERNATING rounds); on = dgq_gemm_mxw8"
              % (ab, fmt.upper()), "(the plan's K split), off = dgq_gemm_blockq twice (off, off'); level: on within [min, max] of the two off medians",
              "%-34s %8s %8s %8s %8s %8s %8s %8s  %s" % ("layer", "on q us", "on g us", "off q us", "off g us", "off' g us", "g on/off", "pair", "GEMM")]
    g = torch.Generator().manual_seed(0)
    verdicts = {}
    for name, geom, N, _ups in KSPLIT_SHAPES[:13]:
        B, H, W, C, kh, kw, stride, pad = geom
        taps = kh * kw
        w = torch.randn(N, C * taps, generator=g) * (C * taps) ** -0.5
        wd, wz = synth.channel_minmax(w, 8)
        pw = ops.PackedWeight(w.to(dev), wd.to(dev), wz.to(dev), None, torch.zeros(N).to(dev), 8, C, taps)
        mxb, blk = ops.MxActBinding(pw, fmt, w_bits=8), ops.BlockActBinding(pw, ab)
        x = (torch.randn(B, H, W, C, generator=g) * 1.3 + 0.2).to(dev)
        pad_k = blk.Kp // 32 if taps == 1 else C // 32
        qm, qb = quant_mx(x, geom, lds=pad_k), ops.quant_act_block(x, geom, ab, ldt=pad_k)
        off = lambda: captured(torch, lambda: ops.gemm_blockq(qb, geom, blk, torch.float32))
        graphs = dict(mq=captured(torch, lambda: quant_mx(x, geom, lds=pad_k)), mg=captured(torch, lambda: ops._block_gemm(mxb, qm, geom, torch.float32)),
                      bq=captured(torch, lambda: ops.quant_act_block(x, geom, ab, ldt=pad_k)), bg=off(), bg2=off())
        us = alternating_us(torch, graphs)
        lo, hi = sorted((us["bg"], us["bg2"]))
        verdict = "faster" if us["mg"] < lo else "level" if us["mg"] <= hi else "SLOWER"
        verdicts.setdefault(verdict, []).append(name)
        lines.append("%-34s %8.2f %8.2f %8.2f %8.2f %8.2f %8.2f %8.2f  %s" % (name, us["mq"], us["mg"], us["bq"], us["bg"], us["bg2"], us["mg"] / ((lo + hi) / 2),
                                                                         (us["mq"] + us["mg"]) / (us["bq"] + (lo + hi) / 2), verdict))
        del graphs
    lines.append("; ".join("%s: %s" % (k, ", ".join(v)) for k, v in verdicts.items()))


def build_rt_model(torch, arch, fmt, abits, steps_cfg, batch, res, dev, use_aq=True, wbits=4, mx_w8=False):
    """a real-time model of ``arch`` from a weight-only checkpoint at W``wbits`` / ``abits``: fmt "row", "block", "mxfp6" or "mxint8"
    (mx_w8: with real_time_mx_w8=True); use_aq False: the weight-only state (un-quantised activations)"""
    import bench
    from dgq_amd import synth
    from dgq_amd.diffusers_rewrite import UNet2DConditionModel
    from dgq_amd.quant import get_qmodel, Scaler
    from dgq_amd.runtime import quant_params
    cfg = dict(bench.CONFIGS["c2"]["cfg"])
    path = "/tmp/dgq_synth_%s_w%da%d_weight_only.pth" % (arch, wbits, abits)
    if not os.path.exists(path):
        synth.write_cali_ckpt(path, arch, wbits, abits, 1, num_slots=1, seed=0, batch=batch, res=res, with_act=False)
    unet = UNet2DConditionModel(arch)
    unet.load_state_dict(synth.state_dict_from_ckpt(path))
    wq, aq, sm = quant_params(Scaler, wbits, abits, True, cfg["log"], cfg["rt"], cfg["sp"])
    aq["real_time"] = True
    if mx_w8:
        aq["real_time_mx_w8"] = True
    if fmt != "row":
        aq["real_time_block"] = 32
    if fmt in ("mxfp6", "mxint8", "mxfp4"):
        aq["real_time_format"] = fmt
    qnn = get_qmodel(arch, types.SimpleNamespace(unet=unet), path, wq, use_aq, aq, sm, False, steps_cfg, False, device=dev)
    qnn = qnn.float().to(dev)
    if use_aq:
        qnn.disable_out_quantization()
    torch.cuda.synchronize()
    return qnn


MX_MODES = (("row", "real-time rows, A6"), ("block", "real-time blocks of 32, A6 (int)"), ("mxfp6", "real-time MXFP6 blocks, A6"))
MXINT8_MODES = (("row", "real-time rows, A8"), ("block", "real-time blocks of 32, A8 (int)"), ("mxint8", "real-time MXINT8 blocks, A8"))


def mx_step_table(torch, ops, args, dev, lines, modes=MX_MODES, ab=6, build=None, wbits=4):
    """the SD step in the three real-time modes at W4A6 (MXINT8_MODES: W4A8), alternating rounds of one process.  build(mode) -> model
    replaces the W4 models; a mode "<m>#2" is the model and graphs of mode "<m>" timed in a second slot of every round"""
    from dgq_amd import synth
    from dgq_amd.runtime import DDIMScheduler
    sched = DDIMScheduler(50).timesteps
    n = args.steps + args.warmup
    timesteps = [int(sched[i % min(n, len(sched))]) for i in range(n)]
    sch = DDIMScheduler(50)
    lat = synth.named_randn("latent", (1, 4, 64, 64), 1).to(dev)
    ctx = synth.named_randn("ctx", (2, 77, 768), 100).to(dev)
    models, info = {}, {}
    for mode, _label in modes:
        if mode.endswith("#2"):
            models[mode], info[mode] = models[mode[:-2]], info[mode[:-2]][:2] + ([],)
            continue
        ops.MX_KSPLIT = 1 if mode.endswith("@1") else None     # "<fmt>@1": the MX mode captured with its K split off (the plan is read at capture)
        qnn = build(mode) if build else build_rt_model(torch, "sd", mode.split("@")[0], ab, 50, 2, 64, dev)

        def one_step(x, t, qnn=qnn):
            eps = qnn(torch.cat([x, x], dim=0), t, ctx)[0]
            return sch.step_guided(eps, t, x, 7.5) if hasattr(sch, "step_guided") else sch.step(eps.chunk(2)[0] + 7.5 * (eps.chunk(2)[1] - eps.chunk(2)[0]), t, x)
        calls, orig = [], ops._lib_call
        with torch.no_grad():
            one_step(lat, timesteps[0])
            ops._lib_call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
            try:
                one_step(lat, timesteps[0])
            finally:
                ops._lib_call = orig
            qnn.enable_graphs(True)
            for t in sorted(set(timesteps), reverse=True):
                one_step(lat, t)
        by = {}
        for c in calls:
            by[c] = by.get(c, 0) + 1
        models[mode], info[mode] = one_step, (len(calls), by, [])
    ops.MX_KSPLIT = None
    with torch.no_grad():
        for _ in range(args.windows):
            for mode, _label in modes:
                x = lat
                for t in timesteps[:args.warmup]:
                    x = models[mode](x, t)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for t in timesteps[args.warmup:]:
                    x = models[mode](x, t)
                torch.cuda.synchronize()
                info[mode][2].append((time.perf_counter() - t0) / args.steps * 1e3)
                assert torch.isfinite(x).all()
    lines += ["", "SD1.4-size synthetic model, 512^2 (64x64 latents), CFG pair, fp32, W%dA%d, weight-only checkpoint; hipGraph replay, %d timed steps behind"
              % (wbits, ab, args.steps), "%d warm-up steps per window, %d ALTERNATING rounds (%s, %s, ...) in one process on one box"
              % (args.warmup, args.windows, ", ".join(m for m, _ in modes) if build else "rows, blocks, MX blocks", modes[0][0] if build else "rows"),
              "%-44s %10s %10s %10s %12s" % ("mode", "median ms", "min ms", "max ms", "entry calls")]
    args.rounds_log = [info[mode][2] for mode, _ in modes]     # per mode, the rounds in order
    for mode, label in modes:
        ncalls, by, ms = info[mode]
        lines.append("%-44s %10.3f %10.3f %10.3f %12d" % (label, statistics.median(ms), min(ms), max(ms), ncalls))
    lines += ["", "entry calls = calls of libdgq_hip.so entries in one eager step, by entry:"]
    lines += ["%s: %s" % (mode, ", ".join("%s %d" % kv for kv in sorted(info[mode][1].items(), key=lambda kv: -kv[1]))) for mode, _ in modes]


def mx_tiny_error(torch, dev, lines, modes=MX_MODES, ab=6):
    """rel-L2 of the tiny UNet's output in each real-time mode at W4A6 (MXINT8_MODES: W4A8) against the same weights with UN-QUANTISED activations"""
    from dgq_amd import synth
    inp = synth.synth_inputs("tiny", 2, 1, 16)
    x, ctx = inp["sample"].to(dev), inp["encoder_hidden_states"].to(dev)
    with torch.no_grad():
        ref = build_rt_model(torch, "tiny", "row", ab, 25, 2, 16, dev, use_aq=False)(x, torch.tensor(999), ctx)[0].double()
        lines += ["", "tiny UNet (weight-only checkpoint, W4A%d, t = 999)" % ab + ": rel-L2 of the output against the same weights with un-quantised activations"]
        for mode, label in modes:
            y = build_rt_model(torch, "tiny", mode, ab, 25, 2, 16, dev)(x, torch.tensor(999), ctx)[0].double()
            lines.append("%-44s %10.4g" % (label, float((y - ref).norm() / ref.norm())))


def build_model(torch, mode, steps_cfg, slots, batch, dev):
    """(qnn, seconds until ready, GB allocated on the device once ready)"""
    import bench
    from dgq_amd import synth
    from dgq_amd.runtime import build_synthetic_qnn, quant_params
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    cfg = dict(bench.CONFIGS["c2"]["cfg"])
    if mode == "calibrated":
        bench.write_synthetic_ckpt("sd", cfg, 64, batch, max(slots) + 1)
        qnn, _ = build_synthetic_qnn("sd", cfg, 64, batch, max(slots) + 1, device=dev)
        qnn.prepare_slots(slots)
    else:
        from dgq_amd.diffusers_rewrite import UNet2DConditionModel
        from dgq_amd.quant import get_qmodel, Scaler
        path = "/tmp/dgq_synth_sd_w4_weight_only.pth"
        if not os.path.exists(path):
            synth.write_cali_ckpt(path, "sd", 4, 8, 1, num_slots=1, seed=0, batch=batch, res=64, with_act=False)
        unet = UNet2DConditionModel("sd")
        unet.load_state_dict(synth.state_dict_from_ckpt(path))
        wq, aq, sm = quant_params(Scaler, 4, 8, True, cfg["log"], cfg["rt"], cfg["sp"])
        aq["real_time"] = True
        if mode == "real_time_block":
            aq["real_time_block"] = 32
        qnn = get_qmodel("sd", types.SimpleNamespace(unet=unet), path, wq, True, aq, sm, False, steps_cfg, False, device=dev)
        qnn = qnn.float().to(dev)
        qnn.disable_out_quantization()
    torch.cuda.synchronize()
    ready = time.perf_counter() - t0
    return qnn, ready, (torch.cuda.memory_allocated() - base) / 1e9


def time_model(torch, ops, qnn, timesteps, warmup, windows, dev):
    from dgq_amd import synth
    from dgq_amd.runtime import DDIMScheduler
    sch = DDIMScheduler(50)
    lat = synth.named_randn("latent", (1, 4, 64, 64), 1).to(dev)
    ctx = synth.named_randn("ctx", (2, 77, 768), 100).to(dev)

    def one_step(x, t):
        eps = qnn(torch.cat([x, x], dim=0), t, ctx)[0]
        return sch.step_guided(eps, t, x, 7.5) if hasattr(sch, "step_guided") else sch.step(eps.chunk(2)[0] + 7.5 * (eps.chunk(2)[1] - eps.chunk(2)[0]), t, x)

    calls = []
    orig = ops._lib_call
    with torch.no_grad():
        one_step(lat, timesteps[0])                          # lazy initialisations, eager
        ops._lib_call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
        try:
            one_step(lat, timesteps[0])
        finally:
            ops._lib_call = orig
        torch.cuda.synchronize()
        after_step = torch.cuda.memory_allocated() / 1e9
        qnn.enable_graphs(True)
        for t in sorted(set(timesteps), reverse=True):
            one_step(lat, t)
        x = lat
        for t in timesteps[:warmup]:
            x = one_step(x, t)
        xw, secs = x, []
        for _ in range(windows):
            x = xw
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in timesteps[warmup:]:
                x = one_step(x, t)
            torch.cuda.synchronize()
            secs.append((time.perf_counter() - t0) / len(timesteps[warmup:]))
        assert torch.isfinite(x).all()
        qnn.enable_graphs(False)
    by = {}
    for n in calls:
        by[n] = by.get(n, 0) + 1
    return statistics.median(secs) * 1e3, len(calls), by, after_step


def block_step_table(torch, ops, args, dev, lines):
    """the three modes' step times in alternating rounds of one process: every model is built and captured first, then each round
    times calibrated, rows, blocks in turn"""
    from dgq_amd import synth
    from dgq_amd.runtime import DDIMScheduler
    sched = DDIMScheduler(50).timesteps
    n = args.steps + args.warmup
    timesteps = [int(sched[i % min(n, len(sched))]) for i in range(n)]
    slots = sorted({(1000 - t) // 20 for t in timesteps})
    sch = DDIMScheduler(50)
    lat = synth.named_randn("latent", (1, 4, 64, 64), 1).to(dev)
    ctx = synth.named_randn("ctx", (2, 77, 768), 100).to(dev)
    modes = (("calibrated", "calibrated c2 (g16, %d time-aware slots)" % len(slots)), ("real_time", "real-time rows (weight-only ckpt)"),
             ("real_time_block", "real-time blocks of 32 (weight-only ckpt)"))
    models, info = {}, {}
    for mode, _label in modes:
        qnn, ready, gb = build_model(torch, mode, 50, slots, 2, dev)

        def one_step(x, t, qnn=qnn):
            eps = qnn(torch.cat([x, x], dim=0), t, ctx)[0]
            return sch.step_guided(eps, t, x, 7.5) if hasattr(sch, "step_guided") else sch.step(eps.chunk(2)[0] + 7.5 * (eps.chunk(2)[1] - eps.chunk(2)[0]), t, x)
        calls, orig = [], ops._lib_call
        with torch.no_grad():
            one_step(lat, timesteps[0])
            ops._lib_call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
            try:
                one_step(lat, timesteps[0])
            finally:
                ops._lib_call = orig
            qnn.enable_graphs(True)
            for t in sorted(set(timesteps), reverse=True):
                one_step(lat, t)
        by = {}
        for c in calls:
            by[c] = by.get(c, 0) + 1
        models[mode], info[mode] = one_step, (len(calls), by, ready, gb, [])
    with torch.no_grad():
        for _ in range(args.windows):
            for mode, _label in modes:
                x = lat
                for t in timesteps[:args.warmup]:
                    x = models[mode](x, t)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for t in timesteps[args.warmup:]:
                    x = models[mode](x, t)
                torch.cuda.synchronize()
                info[mode][4].append((time.perf_counter() - t0) / args.steps * 1e3)
                assert torch.isfinite(x).all()
    lines += ["", "SD1.4-size synthetic model, 512^2 (64x64 latents), CFG pair, fp32, W4A8; hipGraph replay, %d timed steps behind %d warm-up steps per window,"
              % (args.steps, args.warmup), "%d ALTERNATING rounds (calibrated, rows, blocks, calibrated, ...) in one process on one box" % args.windows,
              "%-44s %10s %10s %10s %12s %14s" % ("mode", "median ms", "min ms", "max ms", "entry calls", "GB after load")]
    for mode, label in modes:
        ncalls, by, ready, gb, ms = info[mode]
        lines.append("%-44s %10.3f %10.3f %10.3f %12d %14.2f" % (label, statistics.median(ms), min(ms), max(ms), ncalls, gb))
    lines += ["", "entry calls = calls of libdgq_hip.so entries in one eager step (a call is one to three kernel launches), by entry:"]
    lines += ["%s: %s" % (mode, ", ".join("%s %d" % kv for kv in sorted(info[mode][1].items(), key=lambda kv: -kv[1]))) for mode, _ in modes]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/r08_realtime_act.txt")
    ap.add_argument("--stamp", default=None, help="commit the tree was built from (default: git rev-parse)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--block", action="store_true", help="measure the real-time block mode (see the head of this file)")
    ap.add_argument("--mx", action="store_true", help="measure the real-time MXFP6 mode (see the head of this file)")
    ap.add_argument("--mxint8", action="store_true", help="measure the real-time MXINT8 mode (see the head of this file)")
    ap.add_argument("--mx-ksplit", action="store_true", help="measure the K split of the two MX GEMMs: per shape, and (without --kernels-only) per step")
    ap.add_argument("--mx-w8", action="store_true", help="measure W8 layers under both MX formats, flag on against flag off (see the head of this file)")
    ap.add_argument("--mx-rows", action="store_true", help="measure the one-launch Linear layers of the MX modes (ops.MX_ROWS_FUSED): per shape, and (without --kernels-only) per step")
    ap.add_argument("--append", default=None, help="--mx / --mxint8: a text file whose lines are appended to the report (the tests' measured constants)")
    args = ap.parse_args(argv)
    import torch
    from dgq_amd import _lib, ops
    from dgq_amd.runtime import DDIMScheduler
    _lib.require_gpu()
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    dev = torch.device("cuda", 0)
    if args.mx_w8:
        lines = ["W8 layers under the real-time MX formats (real_time_mx_w8=True: dgq_gemm_mxw8, W8A6 / W8A8) — tools/profile_realtime_act.py --mx-w8",
                 "commit %s; %s; torch %s; ABI %d" % (args.stamp or stamp_default(), torch.cuda.get_device_name(0), torch.__version__, _lib.ABI_VERSION)]
        for fmt, ab in (("mxfp6", 6), ("mxint8", 8)):
            mxw8_kernel_table(torch, ops, dev, lines, fmt)
        for fmt, ab in (() if args.kernels_only else (("mxfp6", 6), ("mxint8", 8))):
            modes = (("off", "%s asked, flag off (int blocks, A%d)" % (fmt.upper(), ab)), ("on", "%s, real_time_mx_w8=True" % fmt.upper()), ("off#2", "flag off, second slot"))
            mx_step_table(torch, ops, args, dev, lines, modes, ab, build=lambda m: build_rt_model(torch, "sd", fmt, ab, 50, 2, 64, dev, wbits=8, mx_w8=m == "on"), wbits=8)
            lines.append("per round (ms), off | on | off#2: " + "; ".join("%.3f | %.3f | %.3f" % p for p in zip(*args.rounds_log)))
            ops._WORKSPACE.clear()
            gc.collect()
            torch.cuda.empty_cache()
        if args.append:
            lines += [""] + open(args.append).read().splitlines()
        text = "\n".join(lines) + "\n"
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
        print(text)
        return 0
    if args.mx_rows:
        lines = ["One-launch Linear layers of the real-time MX modes (dgq_gemm_mx_rows, ops.MX_ROWS_FUSED) — tools/profile_realtime_act.py --mx-rows",
                 "commit %s; %s; torch %s; ABI %d" % (args.stamp or stamp_default(), torch.cuda.get_device_name(0), torch.__version__, _lib.ABI_VERSION)]
        for fmt in ("mxfp6", "mxint8", "mxfp4"):
            mx_rows_table(torch, ops, dev, lines, fmt)
        for fmt, ab in (() if args.kernels_only else (("mxfp4", 4), ("mxfp6", 6))):
            def build(m, fmt=fmt, ab=ab):
                ops.MX_ROWS_FUSED = m == "on"               # read at capture, right behind the build
                return build_rt_model(torch, "sd", fmt, ab, 50, 2, 64, dev)
            modes = (("off", "%s, MX_ROWS_FUSED off" % fmt.upper()), ("on", "%s, MX_ROWS_FUSED on" % fmt.upper()), ("off#2", "off, second slot"))
            mx_step_table(torch, ops, args, dev, lines, modes, ab, build=build)
            ops.MX_ROWS_FUSED = False
            lines.append("per round (ms), off | on | off#2: " + "; ".join("%.3f | %.3f | %.3f" % p for p in zip(*args.rounds_log)))
            ops._WORKSPACE.clear()
            gc.collect()
            torch.cuda.empty_cache()
        if args.append:
            lines += [""] + open(args.append).read().splitlines()
        text = "\n".join(lines) + "\n"
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
        print(text)
        return 0
    if args.mx_ksplit:
        lines = ["K split of the block-scaled MX GEMMs (dgq_gemm_mx6_splitk / dgq_gemm_mxint8_splitk) — tools/profile_realtime_act.py --mx-ksplit",
                 "commit %s; %s; torch %s; ABI %d" % (args.stamp or stamp_default(), torch.cuda.get_device_name(0), torch.__version__, _lib.ABI_VERSION)]
        for fmt in ("mxfp6", "mxint8"):
            mx_ksplit_table(torch, ops, dev, lines, fmt)
        if not args.kernels_only:
            for fmt, ab in (("mxfp6", 6), ("mxint8", 8)):
                mx_step_table(torch, ops, args, dev, lines, (("row", "real-time rows, A%d" % ab), (fmt + "@1", "real-time %s blocks, un-split" % fmt.upper()),
                                                             (fmt, "real-time %s blocks, the plan's K split" % fmt.upper())), ab)
                lines.append("per round (ms), un-split | split: " + "; ".join("%.3f | %.3f" % p for p in zip(args.rounds_log[-2], args.rounds_log[-1])))
                ops._WORKSPACE.clear()
                gc.collect()
                torch.cuda.empty_cache()
        if args.append:
            lines += [""] + open(args.append).read().splitlines()
        text = "\n".join(lines) + "\n"
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
        print(text)
        return 0
    if args.mx or args.mxint8:
        fmt, modes, ab = ("mxint8", MXINT8_MODES, 8) if args.mxint8 else ("mxfp6", MX_MODES, 6)
        lines = ["real-time %s activation mode (real_time_format=\"%s\", W4A%d) — tools/profile_realtime_act.py --%s"
                 % (fmt.upper(), fmt, ab, "mxint8" if args.mxint8 else "mx"),
                 "commit %s; %s; torch %s; ABI %d" % (args.stamp or stamp_default(), torch.cuda.get_device_name(0), torch.__version__, _lib.ABI_VERSION), ""]
        mx_kernel_table(torch, ops, dev, lines, fmt)
        mx_tiny_error(torch, dev, lines, modes, ab)
        if not args.kernels_only:
            mx_step_table(torch, ops, args, dev, lines, modes, ab)
        if args.append:
            lines += [""] + open(args.append).read().splitlines()
        text = "\n".join(lines) + "\n"
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
        print(text)
        return 0
    if args.block:
        lines = ["real-time block activation mode (real_time_block=32) — tools/profile_realtime_act.py --block",
                 "commit %s; %s; torch %s; ABI %d" % (args.stamp or stamp_default(), torch.cuda.get_device_name(0), torch.__version__, _lib.ABI_VERSION), ""]
        block_kernel_table(torch, ops, dev, lines)
        if not args.kernels_only:
            block_step_table(torch, ops, args, dev, lines)
        text = "\n".join(lines) + "\n"
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
        print(text)
        return 0
    lines = ["real-time per-row activation mode vs calibrated c2 tables — tools/profile_realtime_act.py",
             "commit %s; %s; torch %s; ABI %d" % (args.stamp or stamp_default(), torch.cuda.get_device_name(0), torch.__version__, _lib.ABI_VERSION), ""]
    kernel_table(torch, ops, dev, lines)
    if not args.kernels_only:
        sched = DDIMScheduler(50).timesteps
        n = args.steps + args.warmup
        timesteps = [int(sched[i % min(n, len(sched))]) for i in range(n)]
        slots = sorted({(1000 - t) // 20 for t in timesteps})
        lines += ["", "SD1.4-size synthetic model, 512^2 (64x64 latents), CFG pair, fp32, W4A8; %d timed steps x %d windows behind %d warm-up steps, hipGraph replay"
                  % (args.steps, args.windows, args.warmup),
                  "%-38s %10s %12s %14s %14s %14s" % ("mode", "ms / step", "launches", "model_ready s", "GB after load", "GB after step")]
        detail = []
        for mode, label in (("calibrated", "calibrated c2 (g16, %d time-aware slots)" % len(slots)), ("real_time", "real-time rows (weight-only ckpt)")):
            qnn, ready, gb = build_model(torch, mode, 50, slots, 2, dev)
            ms, ncalls, by, gb_step = time_model(torch, ops, qnn, timesteps, args.warmup, args.windows, dev)
            lines.append("%-38s %10.3f %12d %14.1f %14.2f %14.2f" % (label, ms, ncalls, ready, gb, gb_step))
            detail.append("%s: %s" % (mode, ", ".join("%s %d" % kv for kv in sorted(by.items(), key=lambda kv: -kv[1]))))
            del qnn
            ops._WORKSPACE.clear()
            gc.collect()
            torch.cuda.empty_cache()
        lines += ["", "launches = entry calls of libdgq_hip.so in one eager step (a call is one to three kernel launches), by entry:"] + detail
        lines += ["", "GB = torch.cuda.memory_allocated() growth over the build (weights, packed images, tables; the calibrated figure counts the",
                  "slots this run visits, not all 25 / 50 of a full schedule); model_ready includes writing the synthetic checkpoint when /tmp has none."]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
