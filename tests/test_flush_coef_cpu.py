"""The flush-coefficient formula of the per-K GEMM family (dgq_amd/csrc/gemm_flush.h), checked on a CPU: the header every kernel
stages its LDS table with is compiled into a stand-alone host program (tests/host/flush_coef_main.cpp, address + UB sanitizers where
they link) and run as a child process."""
import os
import shutil
import struct
import subprocess

import pytest
import torch

from dgq_amd import plan, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCH = plan.KTILE // plan.KCHUNK


@pytest.fixture(scope="module")
def flush_prog(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    assert hipcc, "hipcc not found"
    out = str(tmp_path_factory.mktemp("flush_coef") / "flush_coef")
    # the host compiler as the Makefile's abi.o rule uses it
    base = [hipcc, "-O2", "-std=c++17", "-x", "c++", "-I", os.path.join(ROOT, "dgq_amd", "csrc"),
            os.path.join(ROOT, "tests", "host", "flush_coef_main.cpp"), "-o", out]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if san.returncode != 0:
        print("sanitizers do not link here, building without:\n" + san.stderr[-2000:])
        subprocess.run(base, check=True, capture_output=True, text=True)
    return out


def _table(prog, S, kt_begin, nk, nk_total, KW, cdelta, cflush):
    """[nk·NCH] coefficients (linear over the slice's chunks) + [nk] clear flags, as the host program prints them"""
    cd = cdelta.detach().float().contiguous()
    assert cd.numel() == nk_total * NCH and cflush.numel() == nk_total * NCH
    text = "%d %d %d %d %d\n" % (S, kt_begin, nk, nk_total, KW)
    text += " ".join("%08x" % b for b in struct.unpack("<%dI" % cd.numel(), cd.numpy().tobytes())) + "\n"
    text += " ".join(str(int(v)) for v in cflush.tolist()) + "\n"
    r = subprocess.run([prog], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    bits = [int(l, 16) for l in r.stdout.split()]
    assert len(bits) == nk * NCH + nk
    return torch.tensor(struct.unpack("<%df" % len(bits), struct.pack("<%dI" % len(bits), *bits)), dtype=torch.float32)


@pytest.mark.parametrize("K", [320, 2304, 9216])
def test_whole_k_single_sequence_equals_plan_flush_coefficients(flush_prog, K):
    """S = 1 over the whole K (the 256-row kernel's table): bit for bit plan.flush_coefficients, on plan_act tables"""
    delta, zp = synth._group_params(K, 16, 8, "flush_coef|K%d" % K, 7)
    lay = plan.plan_act(delta.view(1, 1, K), zp.view(1, 1, K), "linear", K, 1, 8)
    fl = plan.mark_clears(lay.cflush, 8, 4)
    if K > 320:
        assert int((fl == 2).sum()) >= 1
    nk = lay.Kp // plan.KTILE
    for last_marked in (False, True):                        # a mark on the very last chunk: full δ, but nothing to clear behind it
        if last_marked:
            fl = fl.clone()
            fl[-1] = 2
        got = _table(flush_prog, 1, 0, nk, nk, 1, lay.cdelta, fl)
        want = plan.flush_coefficients(lay.cdelta, fl)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), last_marked


def _exact_tables(nk_total):
    """The table pattern of test_gpu_kernels._gemm_exact_case: power-of-two δ, group ends off the tile ends, clear marks inside groups
    (3::12), on chunks where they are ignored (6::16) and — 7::24, chunks that end a group and a K tile — at group ends."""
    nch = nk_total * NCH
    cd = torch.tensor([2.0 ** ((i % 5) - 2) for i in range(nch)])
    gend = torch.tensor([(i % 3 == 1 or i == nch - 1) for i in range(nch)])
    fl = gend.to(torch.uint8)
    fl[3::12] = 2
    fl[6::16] = 2
    fl[7::24] = 2
    gscale = cd.clone()
    for i in range(nch - 2, -1, -1):
        if not gend[i]:
            gscale[i] = gscale[i + 1]
    at_end = [i for i in range(nch - 1) if fl[i] == 2 and i % NCH == NCH - 1 and gend[i]]
    inside = [i for i in range(nch - 1) if fl[i] == 2 and i % NCH == NCH - 1 and not gend[i]]
    assert at_end and inside
    return gscale, fl


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("S,KW", [(1, 1), (2, 1), (2, 2), (4, 1)])
def test_summation_by_parts_identity(flush_prog, S, KW, splits):
    """The kernels' K loop in float64 — S interleaved running totals per K range, accf += coef·T per chunk, totals cleared behind a
    flagged tile, the KW ranges and the K splits summed — must EQUAL Σ_c δ_group(c)·P_c for integer chunk products P and
    power-of-two δ (every step exact)."""
    nk_total = 21                                            # (KW = 2: the range boundaries — behind tile 10; tiles 3 / 10 / 17 of the 3 splits — sit on and off clear marks)
    gscale, fl = _exact_tables(nk_total)
    g = torch.Generator().manual_seed(100 * S + 10 * KW + splits)
    P = torch.randint(-4000, 4000, (nk_total * NCH, 6), generator=g).double()
    want = (gscale.double()[:, None] * P).sum(0)
    tps = (nk_total + splits - 1) // splits
    got = torch.zeros(6, dtype=torch.float64)
    for kt_begin in range(0, nk_total, tps):
        nk = min(nk_total, kt_begin + tps) - kt_begin
        tab = _table(flush_prog, S, kt_begin, nk, nk_total, KW, gscale, fl).double()
        coef, flag = tab[:nk * NCH], tab[nk * NCH:]
        per_kw = (nk + KW - 1) // KW
        for t0 in range(0, nk, per_kw):                     # one K range: its own running totals
            T = torch.zeros(S, 6, dtype=torch.float64)
            for t in range(t0, min(nk, t0 + per_kw)):
                for c in range(NCH):
                    T[c % S] += P[(kt_begin + t) * NCH + c]
                    got += coef[t * NCH + c] * T[c % S]
                if flag[t] != 0:
                    T.zero_()
    assert torch.equal(got, want), (S, KW, splits, got - want)
