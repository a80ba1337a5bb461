"""Measures the real-time MXFP4 mode (real_time_format="mxfp4": dgq_quant_act_mx4 + dgq_gemm_mx4, W4A4) with the helpers of
tools/profile_realtime_act.py — profiles/r26_realtime_mxfp4.txt:
    python tools/profile_realtime_mxfp4.py --out profiles/r26_realtime_mxfp4.txt
  * per SD layer shape: the MXFP4 quantiser and GEMM against the MXFP6 pair (the mixed FP4 x FP6 instruction against FP6 x FP6; both
    un-split and by the K-split plan) — 20 calls per hipGraph replay, median of 7 alternating rounds;
  * the SD step at W4A4 in the int4 row mode, the int4 block mode and MXFP4, and MXFP6 at W4A6, in alternating rounds of one process.
Every mode runs from this tree's library on one box."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

STEP_MODES = (("row", "real-time rows, A4"), ("block", "real-time blocks of 32, A4 (int)"), ("mxfp4", "real-time MXFP4 blocks, A4"),
              ("mxfp6", "real-time MXFP6 blocks, A6"))


def gemm_table(torch, ops, pra, dev, lines):
    from dgq_amd import synth
    lines += ["layer shapes of an SD1.4 step (fp32, W4; 20 calls per hipGraph replay, median of 7 ALTERNATING rounds); q = quantiser, g = GEMM",
              "un-split, gp = GEMM by the K-split plan (ksplit=None); 4/6 = (mx4 q + mx4 gp) / (mx6 q + mx6 gp)",
              "%-34s %8s %8s %8s %8s %8s %8s %7s %7s" % ("layer", "mx4 q", "mx4 g", "mx4 gp", "mx6 q", "mx6 g", "mx6 gp", "g4/g6", "4/6")]
    g = torch.Generator().manual_seed(0)
    slower = []
    for name, geom, N, _ups in pra.KSPLIT_SHAPES[:13]:
        B, H, W, C, kh, kw, stride, pad = geom
        taps = kh * kw
        w = torch.randn(N, C * taps, generator=g) * (C * taps) ** -0.5
        wd, wz = synth.channel_minmax(w, 4)
        pw = ops.PackedWeight(w.to(dev), wd.to(dev), wz.to(dev), None, torch.zeros(N).to(dev), 4, C, taps)
        b4, b6 = ops.MxActBinding(pw, "mxfp4"), ops.MxActBinding(pw, "mxfp6")
        x = (torch.randn(B, H, W, C, generator=g) * 1.3 + 0.2).to(dev)
        lds = b4.Kp // 32 if taps == 1 else C // 32
        q4, q6 = ops.quant_act_mx4(x, geom, lds=lds), ops.quant_act_mx6(x, geom, lds=lds)
        cap = lambda f: pra.captured(torch, f)
        graphs = dict(q4=cap(lambda: ops.quant_act_mx4(x, geom, lds=lds)), g4=cap(lambda: ops.gemm_mx4(q4, geom, b4, torch.float32)),
                      p4=cap(lambda: ops.gemm_mx4(q4, geom, b4, torch.float32, ksplit=None)),
                      q6=cap(lambda: ops.quant_act_mx6(x, geom, lds=lds)), g6=cap(lambda: ops.gemm_mx6(q6, geom, b6, torch.float32)),
                      p6=cap(lambda: ops.gemm_mx6(q6, geom, b6, torch.float32, ksplit=None)))
        us = pra.alternating_us(torch, graphs)
        lines.append("%-34s %8.2f %8.2f %8.2f %8.2f %8.2f %8.2f %7.3f %7.3f" % (name, us["q4"], us["g4"], us["p4"], us["q6"], us["g6"], us["p6"],
                                                                             us["g4"] / us["g6"], (us["q4"] + us["p4"]) / (us["q6"] + us["p6"])))
        if us["g4"] > us["g6"]:
            slower.append(name)
        del graphs
    lines.append("shapes where dgq_gemm_mx4 is slower than dgq_gemm_mx6 (un-split): %s" % (", ".join(slower) if slower else "none"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r26_realtime_mxfp4.txt")
    ap.add_argument("--stamp", default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args(argv)
    import torch
    import profile_realtime_act as pra
    from dgq_amd import _lib, ops
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    lines = ["real-time MXFP4 activation mode (real_time_format=\"mxfp4\", W4A4) — tools/profile_realtime_mxfp4.py",
             "commit %s; %s; torch %s; ABI %d" % (args.stamp or pra.stamp_default(), torch.cuda.get_device_name(0), torch.__version__, _lib.ABI_VERSION), ""]
    gemm_table(torch, ops, pra, dev, lines)
    if not args.kernels_only:
        build = lambda mode: pra.build_rt_model(torch, "sd", mode, 6 if mode == "mxfp6" else 4, 50, 2, 64, dev)
        pra.mx_step_table(torch, ops, args, dev, lines, STEP_MODES, 4, build=build)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
