"""The float64 layer reference of tests/layer_reference.py, pinned without a GPU: it reproduces the reference's own golden layer
outputs (tests/golden/f3_layers.pt), and every exact-integer case of the GPU matrix satisfies its precondition."""
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import dgq_oracle as orc
from tests import layer_reference as lr
from tests.golden import recipes

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F3 = [c for c in recipes.f3_cases() if c["state"] == "wa" and c["wbits"] == 4 and c["abits"] == 8 and c["G"] in (1, 16) and not c.get("two_d")]


@pytest.mark.parametrize("case", F3, ids=lambda c: c["name"])
def test_reference_layer_reproduces_the_f3_goldens(case):
    """one Linear and the three conv geometries (3x3 stride 1 / 2, 1x1) in the per-K, per-M and scalar layouts: y within the 2e-5 of
    test_f3_layers_vs_reference, codes equal to orc.uaq_codes as that test forms them"""
    g = torch.load(os.path.join(GOLD, "f3_layers.pt"), map_location="cpu")[case["name"]]
    inp = recipes.f3_inputs(case)
    w_deq = orc.uaq(inp["w"], g["wdelta"], g["wzp"], case["wbits"])
    k, s, p = case.get("k", 1), case.get("stride", 1), case.get("padding", 0)
    y, q = lr.reference_layer(inp["x"], w_deq, inp["b"], inp["adelta"], inp["azp"], case["abits"], case["kind"], k, s, p)
    assert y.dtype == torch.float64 and y.shape == g["y"].shape
    err = ((y - g["y"].double()).norm() / g["y"].double().norm()).item()
    assert err < 2e-5, err
    if case["kind"] == "linear":
        want = orc.uaq_codes(inp["x"], inp["adelta"], inp["azp"], case["abits"])
        rows = want.reshape(-1, want.shape[-1])
    else:
        cols = F.unfold(inp["x"], kernel_size=k, padding=p, stride=s)
        want = orc.uaq_codes(cols, inp["adelta"], inp["azp"], case["abits"])
        rows = want.permute(0, 2, 1).reshape(-1, cols.shape[1])
    assert torch.equal(q, want)
    assert torch.equal(lr.codes_rows(q, dict(kind=case["kind"])), rows)


def test_reference_layer_upsample_and_residual():
    x = torch.randn(1, 8, 5, 6)
    w = torch.randn(4, 8, 3, 3)
    res = torch.randn(1, 4, 10, 12)
    y, q = lr.reference_layer(x, w, None, torch.tensor(0.05), torch.tensor(120.0), 8, "conv", 3, 1, 1, residual=res, upsample=True)
    xq = orc.uaq(F.interpolate(x, scale_factor=2.0, mode="nearest"), torch.tensor(0.05), torch.tensor(120.0), 8)
    want = F.conv2d(xq.double(), w.double(), None, padding=1) + res.double()       # 0 <= z <= 255: the native form pads with the code z
    assert q.shape == (1, 72, 120) and torch.allclose(y, want, rtol=0, atol=1e-9)


@pytest.mark.parametrize("name,layout,abits,wbits", lr.exact_params(), ids=lambda v: str(v))
def test_exact_case_precondition(name, layout, abits, wbits):
    """every cell of the exact GPU matrix: the term magnitudes stay below 2^24 units (layer_reference.exact_margin, asserted by the
    recipe), the clamps and the out-of-range zero points are really exercised, and the formula evaluates identically in fp32 — in the
    natural and in a random K order — and in float64"""
    case = lr.CASES_BY_NAME[name]
    d = lr.exact_case(name, layout, abits, wbits)
    assert d["margin"] < 1.0 and lr.exact_margin(d, case) == d["margin"]
    y64, q = lr.reference_of(d, case)
    qmax = 2 ** abits - 1
    clamped = float(((q == 0) | (q == qmax)).float().mean())
    assert clamped > 0.01, clamped
    if layout != "scalar":
        z = d["azp"].reshape(-1)
        assert bool((z < 0).any()) and bool((z > qmax).any())
    deq = (d["adelta"] * (q - d["azp"]))
    rows = lr.codes_rows(deq, case)                                               # [M][K] fp32
    w2 = d["w"].reshape(case["N"], -1)
    perm = torch.randperm(w2.shape[1], generator=torch.Generator().manual_seed(1))
    M = rows.shape[0]
    if case["kind"] == "linear":
        fixed = d["bias"][None, :] + d["residual"].reshape(M, -1)
        want = y64.reshape(M, -1)
    else:
        fixed = d["bias"][None, :] + d["residual"].permute(0, 2, 3, 1).reshape(M, -1)
        want = y64.permute(0, 2, 3, 1).reshape(M, -1)
    for cols in (slice(None), perm):
        y32 = rows[:, cols] @ w2[:, cols].t() + fixed
        assert y32.dtype == torch.float32 and torch.equal(y32.double(), want)
