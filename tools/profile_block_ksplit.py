#!/usr/bin/env python3
"""Measures the K split of the real-time int block GEMM (dgq_gemm_blockq_splitk) — profiles/r27_block_ksplit.txt:

  * per SD layer shape (the 13 of tools/profile_realtime_act.py), W4 and W8 at A8: dgq_gemm_blockq un-split (captured twice: the spread
    of its own medians is the yardstick), forced S = 2 / 4 / 8 / 16 (the PAIR of launches, GEMM + combine) and the plan's route,
    alternating rounds of hipGraph replays in one process;
  * the SD step in the int block mode (real_time_block=32, W4A8) with ops.BLOCKQ_KSPLIT = 1 and = None (the plan), and the un-split model
    again in a second slot of every round, alternating rounds of hipGraph replays in one process.

    python tools/profile_block_ksplit.py --out profiles/r27_block_ksplit.txt

--unsplit-step-only times the un-split step alone; it runs from a checkout of the parent commit too (the reference "against the parent",
a process of its own).  --append FILE adds the lines of FILE (the tests' printed figures) to the report."""
import argparse
import gc
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import profile_realtime_act as pra                       # noqa: E402  (also puts the repository root on sys.path)


def sweep_table(torch, ops, dev, lines, wbits, sweep=(2, 4, 8, 16)):
    from dgq_amd import _lib, synth
    lines += ["", "dgq_gemm_blockq alone per shape (W%dA8, fp32 out; 20 calls per hipGraph replay, median of 7 ALTERNATING rounds): un-split twice (S=1, S=1')," % wbits,
              "forced splits (GEMM + combine), the plan's route; tiles = 64x64 output tiles, nkt = K tiles of 256; verdict of the plan's route against [min, max] of S=1, S=1'",
              "%-34s %6s %4s %8s %8s %s %5s %8s  %s" % ("layer", "tiles", "nkt", "S=1 us", "S=1' us", " ".join("%8s" % ("S=%d us" % s) for s in sweep), "plan", "plan us", "plan")]
    g = torch.Generator().manual_seed(0)
    lib = _lib.load()
    for name, geom, N, ups in pra.KSPLIT_SHAPES[:13]:
        B, H, W, C, kh, kw, stride, pad = geom
        taps = kh * kw
        w = torch.randn(N, C * taps, generator=g) * (C * taps) ** -0.5
        wd, wz = synth.channel_minmax(w, wbits)
        ab = ops.BlockActBinding(ops.PackedWeight(w.to(dev), wd.to(dev), wz.to(dev), None, torch.zeros(N).to(dev), wbits, C, taps), 8)
        x = (torch.randn(B, H, W, C, generator=g) * 1.3 + 0.2).to(dev)
        q = ops.quant_act_block(x, geom, 8, ldt=ab.Kp // 32 if taps == 1 else C // 32)
        M = B * ((H + 2 * pad - kh) // stride + 1) * ((W + 2 * pad - kw) // stride + 1)
        tiles, nkt = ((M + 63) // 64) * ((N + 63) // 64), (C * taps // 32 + 7) // 8
        call = lambda s: pra.captured(torch, lambda: ops.gemm_blockq(q, geom, ab, torch.float32, ksplit=s))
        plan = lib.dgq_gemm_blockq_plan_splits(M, N, ab.Kp, wbits, ops.WORKSPACE_BYTES)
        graphs = {"a": call(1), "b": call(1)}
        graphs.update({s: call(s) for s in sweep if s <= nkt})
        graphs["plan"] = call(1 if plan == 1 else None)
        us = pra.alternating_us(torch, graphs)
        lo, hi = sorted((us["a"], us["b"]))
        verdict = "un-split" if plan == 1 else "faster" if us["plan"] < lo else "level" if us["plan"] <= hi else "SLOWER"
        lines.append("%-34s %6d %4d %8.2f %8.2f %s %5d %8.2f  %s" % (name, tiles, nkt, us["a"], us["b"], " ".join("%8.2f" % us[s] if s in us else "%8s" % "-" for s in sweep),
                                                                plan, us["plan"], verdict))
        del graphs


def step_table(torch, ops, args, dev, lines, unsplit_only):
    modes = (("off", "int blocks of 32, A8, un-split (BLOCKQ_KSPLIT = 1)"),)
    if not unsplit_only:
        modes += (("on", "int blocks of 32, A8, the plan's K split"), ("off#2", "un-split, second slot of the round"))

    def build(mode):
        ops.BLOCKQ_KSPLIT = 1 if mode == "off" else None   # read at capture; an attribute without effect on a tree without the split
        return pra.build_rt_model(torch, "sd", "block", 8, 50, 2, 64, dev)
    pra.mx_step_table(torch, ops, args, dev, lines, modes, 8, build=build)
    ops.BLOCKQ_KSPLIT = None
    lines.append("per round (ms), %s: " % " | ".join(m for m, _ in modes) + "; ".join(" | ".join("%.3f" % v for v in p) for p in zip(*args.rounds_log)))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/r27_block_ksplit.txt")
    ap.add_argument("--stamp", default=None, help="commit the tree was built from (default: git rev-parse)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--unsplit-step-only", action="store_true")
    ap.add_argument("--append", default=None)
    args = ap.parse_args(argv)
    import torch
    from dgq_amd import _lib, ops
    _lib.require_gpu()
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    dev = torch.device("cuda", 0)
    lines = ["K split of the real-time int block GEMM (dgq_gemm_blockq_splitk) — tools/profile_block_ksplit.py",
             "commit %s; %s; torch %s; ABI %d" % (args.stamp or pra.stamp_default(), torch.cuda.get_device_name(0), torch.__version__, _lib.ABI_VERSION)]
    if not args.unsplit_step_only:
        for wbits in (4, 8):
            sweep_table(torch, ops, dev, lines, wbits)
            gc.collect()
            torch.cuda.empty_cache()
    if not args.kernels_only:
        step_table(torch, ops, args, dev, lines, args.unsplit_step_only)
    if args.append:
        lines += [""] + open(args.append).read().splitlines()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
