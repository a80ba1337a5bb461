"""The K split of the weight-only matrix-core layer (dgq_conv2d_wq_mfma16_splitk with its plan and workspace entries,
ops.conv2d_wq_mfma16(ksplit=), ops.WQ16_KSPLIT behind QuantLayer.weight_only_mfma16).

A split launch differs from the un-split one in the order of the fp32 summation only, so the route's two contracts carry over
(tests/test_gpu_weight_only_mfma16.py, whose cases, packing and float64 reference are used here):
  * exact data (small-integer x, power-of-two δ): split == un-split == the float64 formula, bit for bit;
  * random data: every element within K·2^-24·S_abs + u_x·S_abs + u_out·|y64|, an order-independent bound; two runs bit-equal.
The first two tests need no GPU."""
import pytest
import torch
import torch.nn as nn

from dgq_amd import ops, _lib
from tests import test_gpu_weight_only_mfma16 as base

gpu = pytest.mark.gpu
ENTRY = "dgq_conv2d_wq_mfma16_splitk"
CASES = dict(base.CASES, **base.LONG)
CASES.update({
    "conv3_1x96x6x6_40": base._conv(1, 96, 6, 6, 40, 3, 1, 1),          # K = 864, T = 7: splits begin mid-tap, at a channel offset
    "geglu_33x256_128": dict(base._lin(33, 256, 128), geglu=True),
    "t64_1000x200_1030": base._lin(1000, 200, 1030),                     # the 64 x 64 form: 272 tiles, T = 4 of 64, ragged both ways
})


def test_splitk_export_and_workspace_refusal():
    lib = _lib.load()
    assert lib.dgq_version() == 123
    p = 1 << 20                          # never dereferenced: refused before a launch.  One 32 x 32 tile, K = 512: T = 4, 2 x 4 KiB

    def call(ws, nbytes):
        return lib.dgq_conv2d_wq_mfma16_splitk(p, 0, 1, 1, 1, 512, 1, 1, 1, 0, 0, p, 4, 512, p, p, None, 32, 0, p, 0, 32, 2, ws, nbytes, None)
    for ws, nbytes in [(None, 1 << 20), (p, 8191), (p, 0)]:
        assert call(ws, nbytes) == -1
        assert ENTRY in _lib.last_error() and "8192" in _lib.last_error(), _lib.last_error()
    assert lib.dgq_conv2d_wq_mfma16_splitk(p, 0, 1, 1, 1, 512, 1, 1, 1, 0, 0, p, 2, 512, p, p, None, 32, 0, p, 0, 32, 2, p, 8192, None) == -1
    assert ENTRY in _lib.last_error() and "w_bits" in _lib.last_error()          # the argument check of the un-split entry


@pytest.mark.parametrize("x_dtype", [0, 2])
def test_plan_properties(x_dtype):
    lib = _lib.load()
    plan, need = lib.dgq_conv2d_wq_mfma16_plan_splits, lib.dgq_conv2d_wq_mfma16_workspace_bytes
    for M, N in [(2, 1280), (128, 1280), (512, 1280), (2048, 640), (8192, 320), (37, 24)]:
        tile = 64 if ((M + 63) // 64) * ((N + 63) // 64) >= 256 else 32
        bk, part = (64, 16384) if tile == 64 else (128, 4096)                    # K tile; bytes of one partial
        tiles = -(-M // tile) * -(-N // tile)
        for K in [1, bk, 2 * bk, 320, 2880, 5760, 11520, 23040]:
            T = -(-K // bk)
            full = plan(M, N, K, x_dtype, 1 << 40)
            assert plan(M, N, K, x_dtype, 0) == 1
            assert T > 2 or full == 1
            for ws in (1 << 16, 1 << 22, 128 << 20, 1 << 40):
                s = plan(M, N, K, x_dtype, ws)
                assert 1 <= s <= T and (s == 1 or s * tiles * part <= ws)
                assert s == 1 or (s - 1) * -(-T // s) < T                        # no empty split
            assert need(M, N, K, x_dtype) == (full * tiles * part if full > 1 else 0)
            assert plan(M, N, K, x_dtype, max(need(M, N, K, x_dtype), 1)) == full


def _exact_layer(c, bits, seed):
    """(x fp32, PackedWeight, w, b) of base.test_exact_integer_twin: x in {-3..3}, δ_n in {1/2, 1/4, 1/8}, integer z, bias in quarters"""
    N, C, k, qmax = c["N"], c["C"], c["k"], 2 ** bits - 1
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, qmax + 1, (N, C, k, k), generator=g)
    zp = torch.randint(0, qmax + 1, (N,), generator=g).float()
    delta = 2.0 ** -(1.0 + (torch.arange(N) % 3).float())
    w = delta[:, None, None, None] * (codes.float() - zp[:, None, None, None])
    b = torch.randint(-8, 9, (N,), generator=g).float() / 4
    return torch.randint(-3, 4, c["x"], generator=g).float(), base._pack(c, w, delta, zp, b, bits), w, b


def _split_and_unsplit(c, x, pw, S, spy):
    """(un-split, split S ways) through ops.conv2d_wq_mfma16; the forced split must have taken the split entry"""
    run = lambda ks: ops.conv2d_wq_mfma16(x, pw, c["k"], c["k"], c["s"], c["p"], upsample=c["ups"], geglu_rows=c["geglu"], ksplit=ks)
    y1 = run(1)
    assert ENTRY not in spy.names
    yS = run(S)
    assert spy.names.count(ENTRY) == 1
    spy.names.clear()
    return y1, yS


EXACT = [("linear_37x320_24", 4, 2), ("linear_37x320_24", 4, 3), ("linear_70x360_72", 4, 2), ("linear_70x360_72", 8, 2),
         ("conv3_s1", 4, 2), ("conv3_s1", 4, 5), ("conv3_s1", 4, 16), ("conv3_s2", 4, 2), ("conv3_s2", 4, 5), ("conv3_s2", 4, 16),
         ("conv3_1x96x6x6_40", 4, 2), ("conv3_1x96x6x6_40", 4, 7), ("conv3_c20", 4, 2), ("conv3_upsample_4x4", 4, 3),
         ("geglu_33x256_128", 4, 2), ("t64_1000x200_1030", 4, 2), ("t64_1000x200_1030", 4, 4)]


@gpu
@pytest.mark.parametrize("dtype", base.DTYPES, ids=["fp32", "bf16", "f16"])
@pytest.mark.parametrize("case,bits,S", EXACT, ids=["%s-W%d-S%d" % e for e in EXACT])
def test_exact_split_equals_unsplit_and_float64(case, bits, S, dtype, monkeypatch):
    """|Σ| <= 864·3·255 < 2^24: every partial sum of every split, their sum, δ·Σ and + b are exact in fp32"""
    c = CASES[case]
    spy = base._Spy(monkeypatch)
    with torch.no_grad():
        x, pw, w, b = _exact_layer(c, bits, sum(map(ord, case)) + bits)
        x = x.to(dtype).cuda()
        y64, _ = base._ref64(c, x, w.double().cuda(), b.double().cuda())
        y1, yS = _split_and_unsplit(c, x, pw, S, spy)
    assert yS.dtype == dtype and yS.shape == y64.shape
    assert torch.equal(yS, y1), "differs from the un-split launch in %d of %d elements" % (int((yS != y1).sum()), yS.numel())
    assert torch.equal(yS, y64.to(dtype))


RANDOM = [("linear_37x320_24", 3), ("conv3_s1", 5), ("conv3_128rows_k2880_40", 4)]


@gpu
@pytest.mark.parametrize("dtype", base.DTYPES, ids=["fp32", "bf16", "f16"])
@pytest.mark.parametrize("case,S", RANDOM, ids=["%s-S%d" % e for e in RANDOM])
def test_random_split_within_the_bound_and_repeatable(case, S, dtype, monkeypatch):
    c = CASES[case]
    spy = base._Spy(monkeypatch)
    w, delta, zp, b = base._random_layer(c, 4, 100 + len(case))
    x = torch.randn(c["x"], generator=torch.Generator().manual_seed(7 + len(case))).to(dtype).cuda()
    with torch.no_grad():
        pw = base._pack(c, w, delta, zp, b, 4)
        wq = (pw.alpha.double()[:, None] * (pw.codes.double() - pw.zp_true.double()[:, None])).view(w.shape)   # δ·(q − z) in float64
        y64, S_abs = base._ref64(c, x, wq, b.double().cuda())
        _, y = _split_and_unsplit(c, x, pw, S, spy)
        _, y_again = _split_and_unsplit(c, x, pw, S, spy)
    base._assert_bound(y, y64, S_abs, c["C"] * c["k"] ** 2, dtype, "%s S=%d" % (case, S))
    assert torch.equal(y, y_again)


@gpu
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_layer_knob_forced_against_never(dtype, exact, monkeypatch):
    """ops.WQ16_KSPLIT = 3 against 1 through a 3x3 QuantLayer with the switch on.  exact: weights in eighths on [-1, 7/8] with both ends
    in every row (MINMAX gives δ = 1/8, z = 8), x in {-3..3}, bias in quarters — equal bit for bit; random: both within the bound."""
    spy = base._Spy(monkeypatch)
    g = torch.Generator().manual_seed(11)
    mod = nn.Conv2d(64, 96, 3, padding=1)
    x = torch.randn((1, 64, 8, 8), generator=g)
    if exact:
        with torch.no_grad():
            mod.weight.copy_(torch.randint(-8, 8, mod.weight.shape, generator=g).float() / 8)
            mod.weight[:, 0, 0, 0], mod.weight[:, 1, 0, 0] = -1.0, 0.875
            mod.bias.copy_(torch.randint(-8, 9, (96,), generator=g).float() / 4)
        x = torch.randint(-3, 4, x.shape, generator=g).float()
    layer = base._qlayer(mod, 4).to(dtype)
    layer.weight_only_mfma16 = True
    x = x.to(dtype).cuda()
    ys = {}
    with torch.no_grad():
        for ks in (1, 3):
            monkeypatch.setattr(ops, "WQ16_KSPLIT", ks)
            ys[ks] = layer(x)
            assert spy.names.count(ENTRY) == (ks == 3) and spy.names.count("dgq_conv2d_wq_mfma16") == (ks == 1)
            spy.names.clear()
        y64, S_abs = base._ref64(dict(ups=False, s=1, p=1), x, layer.dequantized_weight(torch.float32).double(), layer.b.double())
    if exact:
        assert torch.equal(ys[3], ys[1]) and torch.equal(ys[3], y64.to(dtype))
    for ks in (1, 3):
        base._assert_bound(ys[ks], y64, S_abs, 576, dtype, "layer WQ16_KSPLIT=%d" % ks)
