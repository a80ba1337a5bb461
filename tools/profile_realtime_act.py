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


def mx_kernel_table(torch, ops, dev, lines):
    """dgq_quant_act_mx6 + dgq_gemm_mx6 against dgq_quant_act_block + dgq_gemm_blockq and the row mode's layer call, A6, per SD layer shape"""
    from dgq_amd import synth
    lines.append("layer shapes of an SD1.4 step (fp32, W4A6; 20 calls per hipGraph replay, median of 7 ALTERNATING rounds: mx quantiser, mx GEMM,")
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
        mxb, blk, row = ops.MxActBinding(pw), ops.BlockActBinding(pw, 6), ops.DynamicActBinding(pw, 6)
        x = (torch.randn(B, H, W, C, generator=g) * 1.3 + 0.2).to(dev)
        pad_k = blk.Kp // 32 if taps == 1 else C // 32
        qm, qb = ops.quant_act_mx6(x, geom, lds=pad_k), ops.quant_act_block(x, geom, 6, ldt=pad_k)
        x2, xn = x.view(B * H * W, C), x.permute(0, 3, 1, 2)
        row_call = (lambda: ops.quant_linear(x2, row)) if taps == 1 else (lambda: ops.quant_conv2d(xn, row, kh, kw, stride, pad, gn_out=False))
        graphs = dict(mq=captured(torch, lambda: ops.quant_act_mx6(x, geom, lds=pad_k)), mg=captured(torch, lambda: ops.gemm_mx6(qm, geom, mxb, torch.float32)),
                      bq=captured(torch, lambda: ops.quant_act_block(x, geom, 6, ldt=pad_k)), bg=captured(torch, lambda: ops.gemm_blockq(qb, geom, blk, torch.float32)),
                      row=captured(torch, row_call))
        us = alternating_us(torch, graphs)
        m, b = us["mq"] + us["mg"], us["bq"] + us["bg"]
        lines.append("%-34s %9.2f %9.2f %9.2f %9.2f %9.2f %9.2f %9.2f %9.2f" % (name, us["mq"], us["mg"], m, us["bq"], us["bg"], b, us["row"], m / b))
        if m > b:
            slower.append(name)
        del graphs
    lines.append("shapes where the MXFP6 pair is slower than the block pair: %s" % (", ".join(slower) if slower else "none"))


def build_rt_model(torch, arch, fmt, abits, steps_cfg, batch, res, dev, use_aq=True):
    """a real-time model of ``arch`` from a weight-only checkpoint at W4 / ``abits``: fmt "row", "block" or "mxfp6"; use_aq False: the
    weight-only state (un-quantised activations)"""
    import bench
    from dgq_amd import synth
    from dgq_amd.diffusers_rewrite import UNet2DConditionModel
    from dgq_amd.quant import get_qmodel, Scaler
    from dgq_amd.runtime import quant_params
    cfg = dict(bench.CONFIGS["c2"]["cfg"])
    path = "/tmp/dgq_synth_%s_w4a%d_weight_only.pth" % (arch, abits)
    if not os.path.exists(path):
        synth.write_cali_ckpt(path, arch, 4, abits, 1, num_slots=1, seed=0, batch=batch, res=res, with_act=False)
    unet = UNet2DConditionModel(arch)
    unet.load_state_dict(synth.state_dict_from_ckpt(path))
    wq, aq, sm = quant_params(Scaler, 4, abits, True, cfg["log"], cfg["rt"], cfg["sp"])
    aq["real_time"] = True
    if fmt != "row":
        aq["real_time_block"] = 32
    if fmt == "mxfp6":
        aq["real_time_format"] = "mxfp6"
    qnn = get_qmodel(arch, types.SimpleNamespace(unet=unet), path, wq, use_aq, aq, sm, False, steps_cfg, False, device=dev)
    qnn = qnn.float().to(dev)
    if use_aq:
        qnn.disable_out_quantization()
    torch.cuda.synchronize()
    return qnn


MX_MODES = (("row", "real-time rows, A6"), ("block", "real-time blocks of 32, A6 (int)"), ("mxfp6", "real-time MXFP6 blocks, A6"))


def mx_step_table(torch, ops, args, dev, lines):
    """the SD step in the three real-time modes at W4A6, alternating rounds of one process"""
    from dgq_amd import synth
    from dgq_amd.runtime import DDIMScheduler
    sched = DDIMScheduler(50).timesteps
    n = args.steps + args.warmup
    timesteps = [int(sched[i % min(n, len(sched))]) for i in range(n)]
    sch = DDIMScheduler(50)
    lat = synth.named_randn("latent", (1, 4, 64, 64), 1).to(dev)
    ctx = synth.named_randn("ctx", (2, 77, 768), 100).to(dev)
    models, info = {}, {}
    for mode, _label in MX_MODES:
        qnn = build_rt_model(torch, "sd", mode, 6, 50, 2, 64, dev)

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
    with torch.no_grad():
        for _ in range(args.windows):
            for mode, _label in MX_MODES:
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
    lines += ["", "SD1.4-size synthetic model, 512^2 (64x64 latents), CFG pair, fp32, W4A6, weight-only checkpoint; hipGraph replay, %d timed steps behind"
              % args.steps, "%d warm-up steps per window, %d ALTERNATING rounds (rows, blocks, mxfp6, rows, ...) in one process on one box" % (args.warmup, args.windows),
              "%-44s %10s %10s %10s %12s" % ("mode", "median ms", "min ms", "max ms", "entry calls")]
    for mode, label in MX_MODES:
        ncalls, by, ms = info[mode]
        lines.append("%-44s %10.3f %10.3f %10.3f %12d" % (label, statistics.median(ms), min(ms), max(ms), ncalls))
    lines += ["", "entry calls = calls of libdgq_hip.so entries in one eager step, by entry:"]
    lines += ["%s: %s" % (mode, ", ".join("%s %d" % kv for kv in sorted(info[mode][1].items(), key=lambda kv: -kv[1]))) for mode, _ in MX_MODES]


def mx_tiny_error(torch, dev, lines):
    """rel-L2 of the tiny UNet's output in each real-time mode at W4A6 against the same weights with UN-QUANTISED activations"""
    from dgq_amd import synth
    inp = synth.synth_inputs("tiny", 2, 1, 16)
    x, ctx = inp["sample"].to(dev), inp["encoder_hidden_states"].to(dev)
    with torch.no_grad():
        ref = build_rt_model(torch, "tiny", "row", 6, 25, 2, 16, dev, use_aq=False)(x, torch.tensor(999), ctx)[0].double()
        lines += ["", "tiny UNet (weight-only checkpoint, W4A6, t = 999): rel-L2 of the output against the same weights with un-quantised activations"]
        for mode, label in MX_MODES:
            y = build_rt_model(torch, "tiny", mode, 6, 25, 2, 16, dev)(x, torch.tensor(999), ctx)[0].double()
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
    ap.add_argument("--append", default=None, help="--mx: a text file whose lines are appended to the report (the tests' measured constants)")
    args = ap.parse_args(argv)
    import torch
    from dgq_amd import _lib, ops
    from dgq_amd.runtime import DDIMScheduler
    _lib.require_gpu()
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    dev = torch.device("cuda", 0)
    if args.mx:
        lines = ["real-time MXFP6 activation mode (real_time_format=\"mxfp6\", W4A6) — tools/profile_realtime_act.py --mx",
                 "commit %s; %s; torch %s; ABI %d" % (args.stamp or stamp_default(), torch.cuda.get_device_name(0), torch.__version__, _lib.ABI_VERSION), ""]
        mx_kernel_table(torch, ops, dev, lines)
        mx_tiny_error(torch, dev, lines)
        if not args.kernels_only:
            mx_step_table(torch, ops, args, dev, lines)
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
