"""The K split of the two block-scaled GEMMs (dgq_gemm_mx6_splitk / dgq_gemm_mxint8_splitk: S workgroups per tile leave raw fp32
accumulators in the workspace, one combine kernel adds them in a fixed order and runs the family's store epilogue).  On planted exact
data a split layer EQUALS the float64 layer — hence the un-split one — for every S, epilogue form and output type; on real data it stays
inside the formats' bound widened by the 2S − 1 additions of partials; the plan, the route and the argument checks are pinned."""
import pytest
import torch

from tests import layer_reference as lr
from tests import mxfp6_ref as mx
from tests import test_gpu_groupnorm_stats as gs
from tests import test_gpu_layer_routes as routes
from tests import test_gpu_realtime_mxfp6 as t6
from tests import test_gpu_realtime_mxint8 as t8
from tests.test_gpu_realtime_act import dev          # noqa: F401  (module-scoped fixture of the row mode)

pytestmark = pytest.mark.gpu
FMTS = ["mxfp6", "mxint8"]
LIN = lr.linear_case(70, 928, 72)          # ragged row and column tiles; 29 chunks = 4 K tiles, the last with 5: an odd pair and a padding chunk
CONV = lambda stride=1, **kw: lr.conv_case(2, 64, 9, 9, stride, 24, **kw)      # 18 chunks = 3 K tiles: split boundaries inside taps
ROUTE = lr.conv_case(2, 256, 4, 4, 1, 64)  # M = 32, K = 2304: one tile, 9 K tiles
#: the sum term of each format's own real-data bound, in units of 2^-24·T (tests/test_gpu_realtime_mxfp6.py, ..._mxint8.py)
C_FMT = dict(mxfp6=lambda K: t6.C_SUM * K, mxint8=lambda K: t8.C_SUM * 2 * K)


def planted(ops, fmt, case, dev):
    """(binding, x, residual, y64 without residual) of the format's exact recipe at this case.  The budget at K = 928: MXFP6 terms are
    multiples of u = min(2^-6·δw, 1) with |x̂| <= 7.5, |q − z| <= 15 — magnitudes sum to at most 928·7.5·15·2^6·u + bias + residual
    < 2^23·u (asserted: mx6_exact_margin < 1); MXINT8 terms multiples of u = min(2^-9·δw, 1) with |s| <= 64 — (15·928 + 16)·2^9·u
    < 2^23·u.  Below 2^24·u every fp32 sum of such terms is exact in any order, so every partial and every combine step is."""
    if fmt == "mxfp6":
        d, _, ab = t6._exact_layer(ops, case, dev)
        x = d["x"]
    else:
        d = lr._build_exact(case, "perM", 8, 4, lr.PROFILES[0])
        g = torch.Generator().manual_seed(lr._seed("planted-mxint8", case["name"]))
        R, C = mx.input_rows(case, d["x"]).shape
        s, E = torch.randint(-64, 65, (R, C // 32, 32), generator=g), torch.randint(-3, 1, (R, C // 32, 1), generator=g)
        s[:, :, 0] = 64
        x = mx.rows_to_input(case, (s.double() * 2.0 ** (E.double() - 6.0)).float().reshape(R, C), d["x"]).contiguous()
        ab = t8._binding(ops, case, d, dev)
    return ab, x, d["residual"], mx.layer_float64(case, x.double(), d["qw"], d["wzp"], d["wdelta"], d["bias"])


def split_calls(spy, fmt):
    names = [c["name"] for c in spy.take()]
    stem = "dgq_gemm_mx6" if fmt == "mxfp6" else "dgq_gemm_mxint8"
    assert sum(n.startswith("dgq_quant_act_mx") for n in names) == 1 and stem not in names, names
    return names.count(stem + "_splitk")


# ----------------------------------------------------------------------------------------------- 1. exact layers, forced splits
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=gs.ids_dtype)
@pytest.mark.parametrize("case,S", [(LIN, 2), (LIN, 4), (LIN, 16), (CONV(), 3), (CONV(2), 3), (CONV(upsample=True), 3)], ids=lambda v: v["name"] if isinstance(v, dict) else "S%d" % v)
@pytest.mark.parametrize("fmt", FMTS)
def test_exact_layers_forced_splits(fmt, case, S, dtype, dev, monkeypatch):
    """y EQUALS the float64 layer (fp32: with the fp32 residual; bf16: without, rounded once) for every forced S (16 is clamped to the 4 K
    tiles); the convolutions' taps outside the image fall into every split"""
    from dgq_amd import ops
    ab, x, res, y64 = planted(ops, fmt, case, dev)
    res = res if dtype == torch.float32 else None
    spy = gs.spied(ops, monkeypatch)
    monkeypatch.setattr(ops, "MX_KSPLIT", S)
    y = routes.run_layer(ops, case, ab, x.to(dev, dtype), res.to(dev) if res is not None else None)
    assert split_calls(spy, fmt) == 1
    want = (y64 if res is None else y64 + res.double()).float().to(dtype)
    assert y.dtype == dtype and torch.equal(y.cpu(), want), (y.cpu() != want).nonzero()[:4].tolist()


# ----------------------------------------------------------------------------------------------- 2. epilogue forms through the combine
@pytest.mark.parametrize("form", ["res_div", "geglu", "y2_ldy", "f16"])
@pytest.mark.parametrize("fmt", FMTS)
def test_epilogue_forms_equal_unsplit(fmt, form, dev):
    """S = 2 against ksplit = 1 on the exact Linear data, bit for bit, and the bytes around a redirected output untouched"""
    from dgq_amd import ops
    ab, x, _, _ = planted(ops, fmt, LIN, dev)
    M, K, N = LIN["M"], LIN["K"], LIN["N"]
    geom = (M, 1, 1, K, 1, 1, 1, 0)
    quant, gemm = (ops.quant_act_mx6, ops.gemm_mx6) if fmt == "mxfp6" else (ops.quant_act_mxint8, ops.gemm_mxint8)
    q = quant(x.to(dev).view(M, K), geom, lds=ab.Kp // 32)
    r2 = torch.randint(-8, 9, (M // 2, N), generator=torch.Generator().manual_seed(3)).float().to(dev)
    got = []
    for ks in (1, 2):
        buf, wide = torch.zeros(M, N + 72, device=dev), torch.zeros(M, N + 40, device=dev)
        kw = dict(res_div=dict(extra=ops.make_extra(residual=r2, res_div=2)), geglu=dict(extra=ops.make_extra(geglu=True)),
                  y2_ldy=dict(out=wide[:, 8:8 + N], extra=ops.make_extra(y2=buf[:, 40:40 + N])), f16={})[form]
        y = gemm(q, geom, ab, torch.float16 if form == "f16" else torch.float32, ksplit=ks, **kw)
        got.append((y.clone(), buf, wide))
    for a, b in zip(*got):
        assert torch.equal(a, b)
    y, buf, wide = got[1]
    assert tuple(y.shape) == (M, N // 2 if form == "geglu" else N) and float(y.float().abs().max()) > 0
    if form == "y2_ldy":
        assert torch.equal(buf[:, 40:40 + N], y) and float(buf[:, :40].abs().max()) == 0.0 == float(buf[:, 40 + N:].abs().max())
        assert float(wide[:, :8].abs().max()) == 0.0 == float(wide[:, 8 + N:].abs().max())


@pytest.mark.parametrize("fmt", FMTS)
def test_groupnorm_partials_through_the_combine(fmt, dev, monkeypatch):
    """the partials the combine's epilogue leaves, by the metric and tolerance of tests/test_gpu_groupnorm_stats.py (K = 576: S = 2)"""
    from dgq_amd import ops, synth
    B, C, H, N, G = 2, 64, 8, 64, 8
    w = torch.randn(N, C, 3, 3, generator=torch.Generator().manual_seed(11)) * 0.05
    wd, wz = synth.channel_minmax(w, 4)
    ab = ops.MxActBinding(ops.PackedWeight(w.to(dev), wd.to(dev), wz.to(dev), None, gs.chan_bias(N, G, 11).to(dev), 4, C, 9), fmt)
    spy = gs.spied(ops, monkeypatch)
    monkeypatch.setattr(ops, "MX_KSPLIT", 2)
    for kind in gs.RES_KINDS:
        y = ops.quant_conv2d(gs.image(B, C, H, H, torch.float32, dev, 12), ab, 3, 3, 1, 1, residual=gs.residual(kind, B, H, H, N, G, torch.float32, dev), gn_out=True)
        assert split_calls(spy, fmt) == 1
        gs.check_partials(ops, dev, kind, "%s split 3x3 %s" % (fmt, kind), y, G)


# ----------------------------------------------------------------------------------------------- 3. real data inside a derived bound
def real_layer(ops, fmt, case, data, dev):
    """(y, y64, T): the layer on real data, the float64 sum over the KERNEL's own codes and the term magnitudes, as each format's
    test_real_layers_inside_the_bound computes them (MXINT8: the magnitudes of both planes' terms)"""
    d = lr.real_case(case, "perM", 6 if fmt == "mxfp6" else 8, 4)
    x = d["x"]
    if data == "outlier":
        x = mx.rows_to_input(case, mx.outlier_rows(mx.input_rows(case, x)), x).contiguous()
    if fmt == "mxfp6":
        _, y, y64, T, _ = t6.real_layer_ratio(ops, case, d, x, dev)
        return y, y64, T
    ab = t8._binding(ops, case, d, dev, "w_raw")
    B, H, W, Ho, Wo, M, K, taps = lr.geometry(case)
    y = routes.run_layer(ops, case, ab, x.to(dev), None).cpu().double()
    lin = case["kind"] == "linear"
    xs = x.to(dev).reshape(M, K) if lin else x.to(dev).contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
    got = ops.quant_act_mxint8(xs, (M, 1, 1, K, 1, 1, 1, 0) if lin else (B, H, W, K // taps, 3, 3, 1, 1))
    s, unit, _ = t8.check_quantiser(got, mx.input_rows(case, x), K // taps // 32)
    qw, zw, wd = ab.pw.codes.cpu().long(), ab.pw.zp_true.cpu(), ab.pw.alpha.cpu()
    y64 = mx.layer_float64(case, mx.rows_to_input(case, s.double() * unit, x), qw, zw, wd, d["bias"])
    T = mx.term_magnitudes(case, mx.rows_to_input(case, (16.0 * (s >> 4).abs() + (s & 15)).double() * unit, x), qw, zw, wd, d["bias"])
    return y, y64, T


def check_bound(fmt, case, S, what, y, y64, T, capsys):
    """|y − y64| <= 2^-24·|y64| + (c_fmt + 2S)·2^-24·T per element: the format's own sum term, and 2S − 1 fp32 additions of partials,
    each rounding at most 2^-24 of a partial magnitude <= T.  Prints the worst |y − y64| / that bound."""
    K = lr.geometry(case)[6]
    bound = 2.0 ** -24 * y64.abs() + (C_FMT[fmt](K) + 2 * S) * 2.0 ** -24 * T
    with capsys.disabled():
        print("\nMX K-SPLIT %s %s %s S=%d: worst |y - y64| / bound = %.4g" % (fmt, case["name"], what, S, float(((y - y64).abs() / bound).max())))
    assert bool(((y - y64).abs() <= bound).all())


@pytest.mark.parametrize("data", ["randn", "outlier"])
@pytest.mark.parametrize("case,S", [(LIN, 4), (CONV(), 3)], ids=lambda v: v["name"] if isinstance(v, dict) else "S%d" % v)
@pytest.mark.parametrize("fmt", FMTS)
def test_real_layers_inside_the_bound(fmt, case, S, data, dev, capsys, monkeypatch):
    from dgq_amd import ops
    spy = gs.spied(ops, monkeypatch)
    monkeypatch.setattr(ops, "MX_KSPLIT", S)
    y, y64, T = real_layer(ops, fmt, case, data, dev)
    assert [c["name"] for c in spy.take()].count("dgq_gemm_mx6_splitk" if fmt == "mxfp6" else "dgq_gemm_mxint8_splitk") == 1
    check_bound(fmt, case, S, data, y, y64, T, capsys)


# ----------------------------------------------------------------------------------------------- 4. the plan and the route
@pytest.mark.parametrize("fmt", FMTS)
def test_plan_route_and_graph_replay(fmt, dev, capsys, monkeypatch):
    """the default MX_KSPLIT on a one-tile, 9-K-tile convolution: the plan splits it, the layer is one quantiser call and one *_splitk
    call, inside the bound, and two eager runs and the replays of a captured one agree bit for bit"""
    from dgq_amd import _lib, ops
    assert ops.MX_KSPLIT is None
    S = _lib.load().dgq_gemm_mx_plan_splits(32, 64, 2304, ops.WORKSPACE_BYTES)
    assert S > 1
    spy = gs.spied(ops, monkeypatch)
    y, y64, T = real_layer(ops, fmt, ROUTE, "randn", dev)
    assert [c["name"] for c in spy.take()].count("dgq_gemm_mx6_splitk" if fmt == "mxfp6" else "dgq_gemm_mxint8_splitk") == 1
    check_bound(fmt, ROUTE, S, "plan", y, y64, T, capsys)
    d = lr.real_case(ROUTE, "perM", 6 if fmt == "mxfp6" else 8, 4)
    ab, x = t8._binding(ops, ROUTE, d, dev, "w_raw") if fmt == "mxint8" else None, d["x"].to(dev)
    if ab is None:
        ab = ops.MxActBinding(ops.PackedWeight(d["w_raw"].to(dev), d["wdelta"].to(dev), d["wzp"].to(dev), None, d["bias"].to(dev), 4, 256, 9))
    run = lambda: routes.run_layer(ops, ROUTE, ab, x, None)
    e1 = run().clone()
    assert split_calls(spy, fmt) == 1
    e2 = run().clone()
    assert torch.equal(e1.cpu().double(), y) and torch.equal(e1, e2)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        yg = run()
    for _ in range(3):
        yg.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(yg, e1)


def test_plan_function(dev):
    from dgq_amd import _lib, ops
    lib, ws = _lib.load(), ops.WORKSPACE_BYTES
    assert lib.dgq_gemm_mx_plan_splits(128, 1280, 23040, ws) > 1
    assert lib.dgq_gemm_mx_plan_splits(8192, 320, 320, ws) == 1
    assert lib.dgq_gemm_mx_plan_splits(32, 64, 256, ws) == 1 and lib.dgq_gemm_mx_plan_splits(32, 64, 512, ws) == 1     # too few K tiles to split
    assert lib.dgq_gemm_mx_plan_splits(128, 1280, 23040, 0) == 1
    need = lib.dgq_gemm_mx_workspace_bytes(128, 1280, 23040)
    assert need == lib.dgq_gemm_mx_plan_splits(128, 1280, 23040, ws) * 2 * 20 * 32768 <= ws and lib.dgq_gemm_mx_workspace_bytes(8192, 320, 320) == 0


# ----------------------------------------------------------------------------------------------- 5. arguments
@pytest.mark.parametrize("fmt", FMTS)
def test_workspace_and_extras(fmt, dev, monkeypatch):
    """a workspace that holds 3 of the 4 forced splits of the 4-tile Linear layer gives the bits of S = 3 forced (two K tiles per split);
    a workspace 8 bytes off a 16-byte boundary, and extra.conv / extra.act, are DGQ_EINVAL"""
    from dgq_amd import ops
    d = lr.real_case(LIN, "perM", 6 if fmt == "mxfp6" else 8, 4)
    ab = ops.MxActBinding(ops.PackedWeight(d["w_raw"].to(dev), d["wdelta"].to(dev), d["wzp"].to(dev), None, d["bias"].to(dev), 4, LIN["K"], 1), fmt)
    M, K = LIN["M"], LIN["K"]
    geom = (M, 1, 1, K, 1, 1, 1, 0)
    quant, gemm = (ops.quant_act_mx6, ops.gemm_mx6) if fmt == "mxfp6" else (ops.quant_act_mxint8, ops.gemm_mxint8)
    # block scales spread over 2^±10: the fp32 sums round (plain randn sums are exact at this K), so each summation order has its own bits
    spread = 2.0 ** torch.randint(-10, 11, (M, K // 32, 1), generator=torch.Generator().manual_seed(5)).float()
    q = quant((d["x"].view(M, K // 32, 32) * spread).to(dev).view(M, K), geom, lds=ab.Kp // 32)
    y1, y3, y4 = (gemm(q, geom, ab, torch.float32, ksplit=s) for s in (1, 3, 4))
    assert not torch.equal(y3, y1) and not torch.equal(y4, y3)
    full = ops.workspace(dev)
    monkeypatch.setattr(ops, "workspace", lambda device: full[:3 * 4 * 32768 + 32000])
    assert torch.equal(gemm(q, geom, ab, torch.float32, ksplit=4), y3)
    monkeypatch.setattr(ops, "workspace", lambda device: full[:32000])      # not one split's partials: un-split
    assert torch.equal(gemm(q, geom, ab, torch.float32, ksplit=4), y1)
    monkeypatch.setattr(ops, "workspace", lambda device: full[8:])
    with pytest.raises(RuntimeError, match=r"_splitk failed \(-1\)"):
        gemm(q, geom, ab, torch.float32, ksplit=2)
    monkeypatch.setattr(ops, "workspace", lambda device: full)
    act, conv = ops._lib.GemmExtra(), ops._lib.GemmExtra()
    act.res_div, act.act, conv.res_div, conv.conv = 1, 256, 1, 256         # (non-null pointer values: refused before anything reads them)
    for ex in (act, conv):
        with pytest.raises(RuntimeError, match=r"_splitk failed \(-1\)"):
            gemm(q, geom, ab, torch.float32, extra=ex, ksplit=2)
