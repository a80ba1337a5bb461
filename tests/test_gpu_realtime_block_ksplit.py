"""The K split of the real-time int block GEMM (dgq_gemm_blockq_splitk: S workgroups per tile leave raw fp32 accumulators in the
workspace, the family's combine adds them in a fixed order and runs the un-split epilogue with the zero-point term zw[n]·R[m]).  On
planted exact data a split layer EQUALS the un-split one and the float64 formula for every S, weight width, output type and epilogue
form; on random data it stays inside the un-split kernel's bound; the clamps, the plan and the route through QuantLayer are pinned."""
import pytest
import torch

from tests import layer_reference as lr
from tests import realtime_block_ref as rb
from tests import test_gpu_layer_routes as routes
from tests import test_gpu_realtime_block as tb
from tests.test_gpu_realtime_block import dev, rel_l2          # noqa: F401  (module-scoped fixture of the block mode)

pytestmark = pytest.mark.gpu
LIN = lr.linear_case(70, 768, 72)          # 3 K tiles: a ragged last split at S = 2, one tile each at S = 3; ragged row and column tiles
HALF = lr.linear_case(64, 384, 64)         # Kp = 384 = 12 chunks: the last split is half a K tile
CONV = lambda stride=1, **kw: lr.conv_case(2, 32, 5, 5, stride, 24, **kw)      # 9 chunks: split 1 starts at tap 8, behind it the K padding
UPS = lr.conv_case(2, 32, 4, 4, 1, 24, upsample=True)
CASES = [(LIN, 2), (LIN, 3), (HALF, 2), (CONV(), 2), (CONV(2), 2), (UPS, 2)]
ids = lambda v: v["name"] if isinstance(v, dict) else str(v).replace("torch.", "")


def launch(ops, case, ab, x, dev, ksplit, dtype=torch.float32, **kw):
    """quantiser + ops.gemm_blockq as quant_linear / quant_conv2d issue them, with the split forced -> y [M][N]"""
    B, H, W, Ho, Wo, M, K, taps = lr.geometry(case)
    if case["kind"] == "linear":
        geom, ups = (M, 1, 1, K, 1, 1, 1, 0), False
        q = ops.quant_act_block(x.to(dev).view(M, K), geom, ab.abits, ldt=ab.Kp // 32)
    else:
        geom, ups = (B, H, W, case["C"], 3, 3, case["stride"], 1), case["upsample"]
        q = ops.quant_act_block(x.to(dev).contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1), geom, ab.abits, ups=ups)
    return ops.gemm_blockq(q, geom, ab, dtype, ups=ups, ksplit=ksplit, **kw)


def rows(t, case):
    return t.reshape(-1, t.shape[-1]) if case["kind"] == "linear" else t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=ids)
@pytest.mark.parametrize("wbits", [4, 8])
@pytest.mark.parametrize("case,S", CASES, ids=ids)
def test_exact_layers_equal_unsplit_and_formula(case, S, wbits, dtype, dev):
    """every fp32 sum of the planted data is exact (tb._exact_layer asserts the margin), so any split order gives the float64 formula's
    value: fp32 with the residual in the combine's epilogue, bf16 without, rounded once; the GEGLU epilogue bit for bit as un-split"""
    from dgq_amd import ops
    d, y_ref, ab = tb._exact_layer(ops, case, 8, wbits, dev)
    res = rows(d["residual"], case).contiguous()
    kw = dict(extra=ops.make_extra(residual=res.to(dev))) if dtype == torch.float32 else {}
    y1, ys = (launch(ops, case, ab, d["x"], dev, s, dtype, **kw).cpu() for s in (1, S))
    want = rows(y_ref, case) - (0 if kw else res.double())
    assert torch.equal(ys, y1) and torch.equal(ys.double(), want.float().to(dtype).double()), (ys != y1).nonzero()[:4].tolist()
    g1, gs = (launch(ops, case, ab, d["x"], dev, s, dtype, extra=ops.make_extra(geglu=True)) for s in (1, S))
    assert tuple(gs.shape) == (y1.shape[0], case["N"] // 2) and torch.equal(gs, g1)


@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("case", [LIN, CONV()], ids=ids)
def test_random_layers_inside_the_unsplit_bound(case, S, dev, capsys):
    """randn data against the float64 formula over the CPU statement's codes: rel-L2 <= 2e-5, the bound test_real_layers_vs_reference
    asserts for the un-split kernel, unchanged — it bounds fp32 accumulation of these terms in any order (S = 3 of the 2-tile conv clamps)"""
    from dgq_amd import ops
    d = lr.real_case(case, "perM")
    y_ref = rb.block_reference(case, d)[0]
    y = launch(ops, case, tb._real_layer(ops, case, d, dev), d["x"], dev, S, extra=ops.make_extra(residual=rows(d["residual"], case).contiguous().to(dev)))
    err = rel_l2(y.cpu(), rows(y_ref, case))
    with capsys.disabled():
        print("\nBLOCK K-SPLIT %s S=%d: rel-L2 vs float64 %.3g = %.3g of the bound" % (case["name"], S, err, err / 2e-5))
    assert err <= 2e-5, err


def test_clamps_workspace_and_plan(dev, monkeypatch):
    """S beyond the 3 K tiles is S = 3; a workspace that holds 2 of 3 forced splits of the 4-tile layer gives the bits of S = 2, none at
    all the un-split bits (the family's launch clamps, as for the MX entries); one 8 bytes off a 16-byte boundary is DGQ_EINVAL"""
    from dgq_amd import _lib, ops
    d = lr.real_case(LIN, "perM")
    ab = tb._real_layer(ops, LIN, d, dev)
    # block scales spread over 2^±10: the fp32 sums round, so each summation order has its own bits
    x = d["x"].view(70, 24, 32) * 2.0 ** torch.randint(-10, 11, (70, 24, 1), generator=torch.Generator().manual_seed(5)).float()
    y1, y2, y3 = (launch(ops, LIN, ab, x, dev, s) for s in (1, 2, 3))
    assert not torch.equal(y2, y1) and not torch.equal(y3, y2)
    assert torch.equal(launch(ops, LIN, ab, x, dev, 16), y3)
    full = ops.workspace(dev)
    monkeypatch.setattr(ops, "workspace", lambda device: full[:2 * 4 * 32768 + 32000])
    assert torch.equal(launch(ops, LIN, ab, x, dev, 3), y2)
    monkeypatch.setattr(ops, "workspace", lambda device: full[:32000])
    assert torch.equal(launch(ops, LIN, ab, x, dev, 3), y1)
    monkeypatch.setattr(ops, "workspace", lambda device: full[8:])
    with pytest.raises(RuntimeError, match=r"_splitk failed \(-1\)"):
        launch(ops, LIN, ab, x, dev, 2)
    lib, ws = _lib.load(), ops.WORKSPACE_BYTES
    for wbits in (4, 8):
        assert all(lib.dgq_gemm_blockq_plan_splits(M, N, Kp, wbits, ws) == 1 for M, N, Kp in [(70, 72, 768), (64, 64, 384), (50, 24, 384), (128, 128, 1792)])
        S = lib.dgq_gemm_blockq_plan_splits(128, 1280, 23040, wbits, ws)
        assert S > 1 and lib.dgq_gemm_blockq_plan_splits(128, 1280, 23040, wbits, 0) == 1
        assert lib.dgq_gemm_blockq_workspace_bytes(128, 1280, 23040, wbits) == S * 2 * 20 * 32768 <= ws


def test_quant_layer_takes_the_knob(dev, monkeypatch):
    """a block-mode QuantLayer on the conv shape under ops.BLOCKQ_KSPLIT = 2: one dgq_gemm_blockq_splitk call, the bits of ops.gemm_blockq(..., ksplit=2)"""
    from dgq_amd import _lib, ops
    from dgq_amd.quant import QuantLayer, Scaler
    case = CONV()
    d = lr.real_case(case, "perM")
    conv = torch.nn.Conv2d(32, 24, 3, padding=1)
    conv.weight.data.copy_(d["w_raw"])
    conv.bias.data.copy_(d["bias"])
    aq = {"bits": 8, "channel_wise": False, "scaler": Scaler.MINMAX, "leaf_param": True, "real_time": True, "real_time_block": 32}
    layer = QuantLayer(conv, {"bits": 4, "channel_wise": True, "scaler": Scaler.MINMAX}, aq).to(dev)
    layer.set_quant_state(True, True)
    spy = routes.Spy(ops, _lib)
    monkeypatch.setattr(ops, "_lib_call", spy)
    monkeypatch.setattr(ops, "BLOCKQ_KSPLIT", 2)
    with torch.no_grad():
        y = layer(d["x"].to(dev))
    names = [c["name"] for c in spy.take()]
    assert names.count("dgq_gemm_blockq_splitk") == 1 and "dgq_gemm_blockq" not in names, names
    assert torch.equal(rows(y, case), launch(ops, case, layer._bindings["real_time"], d["x"], dev, 2))
