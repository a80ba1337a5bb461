"""Real-time per-row activation quantisation (UniformAffineQuantizer(real_time=True), dgq_act_row_params): every row the layer's
quantiser sees gets its own (δ, z) from Scaler.MINMAX applied to that row at run time — a mode of this library.

The statement the kernel must reproduce BIT FOR BIT is ``quant_layer.row_minmax`` (== the scalar ``quant_layer.minmax`` per row,
tests/test_realtime_act_cpu.py).  Everything downstream is checked against tests/layer_reference.py under the CPU-made tables: the
codes equal ``orc.uaq_codes``, exact-integer layers EQUAL the float64 formula on every route a dynamic binding can take, real-valued
layers stay within the project's bounds (2e-5 without a prologue, the bounds of test_real_layer_folded_prologue with one).
"""
import types

import pytest
import torch
import torch.nn.functional as F

from tests import layer_reference as lr
from tests import test_gpu_layer_routes as routes

pytestmark = pytest.mark.gpu


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


@pytest.fixture(scope="module")
def dev():
    from dgq_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


# ----------------------------------------------------------------------------------------------- the CPU statement
def cpu_tables_linear(x2d, bits, fold_T=0):
    """(δ, z) [M] of the rows of x2d [M][K] (fp32 values), or [fold_T] over the rows with equal r % fold_T"""
    from dgq_amd.quant.quant_layer import row_minmax
    mn, mx = x2d.float().min(dim=1)[0], x2d.float().max(dim=1)[0]
    if fold_T:
        mn, mx = mn.view(-1, fold_T).min(dim=0)[0], mx.view(-1, fold_T).max(dim=0)[0]
    return row_minmax(mn, mx, 2 ** bits)


def cpu_tables_conv(x, bits, k, stride, pad, upsample=False):
    """(δ, z) [B][L] of the rows of the unfolded operand of x [B, C, H, W] (zeros outside the image, behind a 2x upsample)"""
    from dgq_amd.quant.quant_layer import row_minmax
    if upsample:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    cols = F.unfold(x.float(), kernel_size=k, dilation=1, padding=pad, stride=stride)          # [B, C·k·k, L]
    d, z = row_minmax(cols.min(dim=1)[0].reshape(-1), cols.max(dim=1)[0].reshape(-1), 2 ** bits)
    return d.view(x.shape[0], -1), z.view(x.shape[0], -1)


def gpu_tables_conv(ops, x, bits, k, stride, pad, upsample=False, pre=None):
    """dgq_act_row_params on the channels-last storage of x [B, C, H, W] as quant_conv2d hands it over -> (δ, z) [B·L]"""
    B, C, H, W = x.shape
    up = 2 if upsample else 1
    xs = x.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
    return ops.act_row_params(xs, (B, H * up, W * up, C, k, k, stride, pad), bits, pre, ups=upsample)


def special_rows(x2d):
    """rows 0 .. 3 of a [M][K] tensor made all-positive, all-negative, all-zero (the 1e-8 clamp) and carrying a 1e4 outlier"""
    x2d[0] = x2d[0].abs() + 0.1
    x2d[1] = -x2d[1].abs() - 0.1
    x2d[2] = 0.0
    x2d[3, 5] = 1e4
    return x2d


def special_image(x):
    """image 0 all-positive with a 1e4 outlier; image 1: upper rows all-negative, the rows from H/2 on all-zero (k x k windows that
    lie inside either region see only that sign — or only zeros: the 1e-8 clamp)"""
    H = x.shape[2]
    x[0] = x[0].abs() + 0.1
    x[0, 3, 2, 1] = 1e4
    x[1, :, :H // 2] = -x[1, :, :H // 2].abs() - 0.1
    x[1, :, H // 2:] = 0.0
    return x


CONV_TABLE_CASES = [dict(B=2, C=32, H=9, W=9, k=3, stride=1, ups=False), dict(B=2, C=64, H=11, W=13, k=3, stride=2, ups=False),
                    dict(B=2, C=64, H=8, W=8, k=3, stride=1, ups=True), dict(B=2, C=64, H=7, W=9, k=1, stride=1, ups=False)]


# ----------------------------------------------------------------------------------------------- 1. row tables, bit exact
@pytest.mark.parametrize("bits", [8, 6])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=lambda d: str(d).replace("torch.", ""))
@pytest.mark.parametrize("M,K", [(154, 768), (37, 320)])
def test_row_tables_linear_bit_exact(M, K, dtype, bits, dev):
    from dgq_amd import ops
    g = torch.Generator().manual_seed(M * 1000 + K + bits)
    x = special_rows(torch.randn(M, K, generator=g) * 1.3 + 0.2).to(dtype)
    d, z = ops.act_row_params(x.to(dev), (M, 1, 1, K, 1, 1, 1, 0), bits)
    dr, zr = cpu_tables_linear(x.float(), bits)
    assert float(dr[2]) == float(torch.tensor(1e-8)) and float(zr[2]) == 0.0                  # the all-zero row takes the clamp
    assert float(zr.min()) >= 0 and float(zr.max()) <= 2 ** bits - 1
    assert torch.equal(d.cpu(), dr), "δ differs on rows %s" % (d.cpu() != dr).nonzero().flatten().tolist()[:8]
    assert torch.equal(z.cpu(), zr), "z differs on rows %s" % (z.cpu() != zr).nonzero().flatten().tolist()[:8]


@pytest.mark.parametrize("bits", [8, 6])
@pytest.mark.parametrize("c", CONV_TABLE_CASES, ids=lambda c: "c%d_%dx%d_k%d_s%d%s" % (c["C"], c["H"], c["W"], c["k"], c["stride"], "_ups" if c["ups"] else ""))
def test_row_tables_conv_bit_exact(c, bits, dev):
    from dgq_amd import ops
    g = torch.Generator().manual_seed(c["C"] + c["H"] + bits)
    x = special_image(torch.randn(c["B"], c["C"], c["H"], c["W"], generator=g) * 1.3 + 0.2)
    k, s, p = c["k"], c["stride"], c["k"] // 2
    d, z = gpu_tables_conv(ops, x.to(dev), bits, k, s, p, c["ups"])
    dr, zr = cpu_tables_conv(x, bits, k, s, p, c["ups"])
    assert int((dr == float(torch.tensor(1e-8))).sum()) > 0, "no all-zero window in the case"
    assert torch.equal(d.cpu(), dr.reshape(-1)), "δ differs at %s" % (d.cpu() != dr.reshape(-1)).nonzero().flatten().tolist()[:8]
    assert torch.equal(z.cpu(), zr.reshape(-1)), "z differs at %s" % (z.cpu() != zr.reshape(-1)).nonzero().flatten().tolist()[:8]


@pytest.mark.parametrize("bits", [8, 6])
@pytest.mark.parametrize("B,T,C", [(2, 77, 320), (2, 64, 64)])
def test_row_tables_fold_bit_exact(B, T, C, bits, dev):
    """the attention-side layout: one pair per token t over the rows b·T + t — q, k and v of one attention in ONE call"""
    from dgq_amd import ops
    g = torch.Generator().manual_seed(T + C + bits)
    xs = [special_rows(torch.randn(B * T, C, generator=g) * (0.5 + i) + 0.1 * i) for i in range(3)]
    xs[1][T + 2] = 0.0                                             # token 2: all-zero in BOTH batch entries
    got = ops.act_row_params_multi([(x.to(dev), (B * T, 1, 1, C, 1, 1, 1, 0), bits, None, None, False, T) for x in xs])
    for i, (x, (d, z)) in enumerate(zip(xs, got)):
        dr, zr = cpu_tables_linear(x, bits, fold_T=T)
        assert d.shape == (T,)
        assert torch.equal(d.cpu(), dr) and torch.equal(z.cpu(), zr), "problem %d of the batch" % i
    assert float(got[1][0][2]) == float(torch.tensor(1e-8))


# ----------------------------------------------------------------------------------------------- 2. codes, bit exact
def _packed(ops, dev, N, C, taps, seed, wbits=4):
    from dgq_amd import synth
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, C * taps, generator=g) * (C * taps) ** -0.5
    wd, wz = synth.channel_minmax(w, wbits)
    return ops.PackedWeight(w.to(dev), wd.to(dev), wz.to(dev), None, torch.zeros(N).to(dev), wbits, C, taps)


def _perm_lay():
    return types.SimpleNamespace(mode="perM", kperm=None)


@pytest.mark.parametrize("bits", [8, 6])
@pytest.mark.parametrize("M,K", [(154, 768), (37, 320)])
def test_codes_linear_bit_exact(M, K, bits, dev):
    """dgq_quant_act under the GPU-made tables == orc.uaq_codes under the CPU-made ones"""
    from dgq_amd import ops
    g = torch.Generator().manual_seed(M + K + bits)
    x = special_rows(torch.randn(M, K, generator=g) * 1.3 + 0.2)
    case = lr.linear_case(M, K, 32)
    ab = ops.DynamicActBinding(_packed(ops, dev, 32, K, 1, 3), bits)
    bound = ab.bound(*ops.act_row_params(x.to(dev), (M, 1, 1, K, 1, 1, 1, 0), bits))
    assert bound.L == M and not bound.dynamic and ab.dynamic
    codes, rowsum, _ = ops.quant_act(x.to(dev), M, 1, 1, K, 1, 1, 1, 0, bound)
    dr, zr = cpu_tables_linear(x, bits)
    q, _ = lr.reference_codes(x.view(1, M, K), dr.view(1, M, 1), zr.view(1, M, 1), bits, "linear")
    routes.check_codes(case, _perm_lay(), codes, rowsum, lr.codes_rows(q, case), dict(abits=bits), 0, "linear %dx%d a%d" % (M, K, bits))


@pytest.mark.parametrize("bits", [8, 6])
@pytest.mark.parametrize("c", CONV_TABLE_CASES, ids=lambda c: "c%d_%dx%d_k%d_s%d%s" % (c["C"], c["H"], c["W"], c["k"], c["stride"], "_ups" if c["ups"] else ""))
def test_codes_conv_bit_exact(c, bits, dev):
    from dgq_amd import ops
    g = torch.Generator().manual_seed(c["C"] + c["W"] + bits)
    x = special_image(torch.randn(c["B"], c["C"], c["H"], c["W"], generator=g) * 1.3 + 0.2)
    k, s, p = c["k"], c["stride"], c["k"] // 2
    case = lr.conv_case(c["B"], c["C"], c["H"], c["W"], s, 32, k=k, upsample=c["ups"])
    ab = ops.DynamicActBinding(_packed(ops, dev, 32, c["C"], k * k, 5), bits)
    bound = ab.bound(*gpu_tables_conv(ops, x.to(dev), bits, k, s, p, c["ups"]))
    codes, rowsum, _ = routes.run_quantiser(ops, case, bound, x.to(dev))
    dr, zr = cpu_tables_conv(x, bits, k, s, p, c["ups"])
    qs = [lr.reference_codes(x[b:b + 1], dr[b].view(1, 1, -1), zr[b].view(1, 1, -1), bits, "conv", k, s, p, c["ups"])[0] for b in range(c["B"])]
    routes.check_codes(case, _perm_lay(), codes, rowsum, lr.codes_rows(torch.cat(qs), case), dict(abits=bits), 0, case["name"])


# ----------------------------------------------------------------------------------------------- 3. exact-integer layers
def _planted_exact(case, abits, wbits):
    """``layer_reference._build_exact`` with the inputs kept INSIDE the planted extremes −z·2^e and (2^b − 1 − z)·2^e of every row
    (linear: per row; conv: one (e, z) per image, the pair planted in every pixel, so every window holds it): per-row MINMAX then
    returns δ = 2^e and z exactly, and every fp32 step of every route is exact.  No clamping lattice (it would move the extremes).
    Returns the recipe dict with x replaced and the per-row tables the CPU statement gives ((1, M, 1) / [B][L])."""
    prof = lr.PROFILES[lr.profile_for(case, "perM", abits, wbits)]
    d = lr._build_exact(case, "perM", abits, wbits, prof)
    g = torch.Generator().manual_seed(lr._seed("planted", case["name"], abits, wbits))
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g)
    B, H, W, Ho, Wo, M, K, taps = lr.geometry(case)
    lin = case["kind"] == "linear"
    n = M if lin else B
    e = torch.tensor(prof["dexp"])[ri(0, len(prof["dexp"]) - 1, (n,))].double()
    z = (2 ** (abits - 1) + prof["zstep"] * ri(-4, 4, (n,))).double()
    lo, hi = (-z * 2.0 ** e).float(), ((2 ** abits - 1 - z) * 2.0 ** e).float()
    x = (2 * ri(-prof["xr"], prof["xr"], tuple(d["x"].shape))).float()
    if lin:
        x = torch.maximum(torch.minimum(x, hi.view(1, M, 1)), lo.view(1, M, 1))
        c0, c1 = ri(0, K // 2 - 1, (M,)), ri(K // 2, K - 1, (M,))
        x[0, torch.arange(M), c0], x[0, torch.arange(M), c1] = lo, hi
        dr, zr = cpu_tables_linear(x.view(M, K), abits)
        d["adelta"], d["azp"] = dr.view(1, M, 1), zr.view(1, M, 1)
    else:
        C = case["C"]
        x = torch.maximum(torch.minimum(x, hi.view(B, 1, 1, 1)), lo.view(B, 1, 1, 1))
        x[:, 0], x[:, C - 1] = lo.view(B, 1, 1).expand(B, case["H"], case["W"]), hi.view(B, 1, 1).expand(B, case["H"], case["W"])
        dr, zr = cpu_tables_conv(x, abits, case["k"], case["stride"], case["pad"], case["upsample"])
        d["adelta"], d["azp"] = dr, zr
    assert torch.equal(dr.reshape(n, -1), (2.0 ** e).float().view(n, 1).expand(n, dr.numel() // n)), "planted rows: δ is not 2^e"
    assert torch.equal(zr.reshape(n, -1), z.float().view(n, 1).expand(n, zr.numel() // n)), "planted rows: z is not the planted one"
    d["x"] = x
    return d


def _reference(case, d):
    """y (float64), per image for a convolution (its (1, 1, L) table cannot vary over the batch), and the margin of the data"""
    if case["kind"] == "linear":
        return lr.reference_of(d, case)[0], lr.exact_margin(d, case) if "qw" in d else None
    ys, margin = [], 0.0
    for b in range(case["B"]):
        db = dict(d, x=d["x"][b:b + 1], residual=d["residual"][b:b + 1], adelta=d["adelta"][b].view(1, 1, -1), azp=d["azp"][b].view(1, 1, -1))
        ys.append(lr.reference_of(db, case)[0])
        if "qw" in d:
            margin = max(margin, lr.exact_margin(db, case))
    return torch.cat(ys), margin if "qw" in d else None


#: (case, abits, wbits, what the spy must see): the smallest shape that takes each route a dynamic binding can take
EXACT_ROUTES = [
    (lr.linear_case(154, 768, 320), 8, 4, dict(route="plain tile", fused=False, splits=1)),
    (lr.linear_case(154, 768, 320), 6, 4, dict(route="plain tile, A6", fused=False, splits=1)),
    (lr.linear_case(154, 768, 320), 8, 8, dict(route="plain tile, W8", fused=False, splits=1)),
    (lr.linear_case(32, 8192, 64), 8, 4, dict(route="split-K + combine", fused=False, splits=8)),
    (lr.linear_case(2048, 320, 320), 8, 4, dict(route="panel (quantiser inside)", fused=True, splits=1)),
    (lr.conv_case(2, 320, 8, 8, 1, 320), 8, 4, dict(route="conv inside the GEMM", fused=True, splits=1)),
    (lr.conv_case(2, 32, 9, 9, 1, 24), 8, 4, dict(route="two-launch conv", fused=False, splits=1)),
    (lr.conv_case(2, 64, 11, 13, 2, 64), 8, 4, dict(route="stride-2 conv", fused=False, splits=1)),
    (lr.conv_case(2, 320, 16, 16, 1, 64, upsample=True), 8, 4, dict(route="upsample fold", fused=False, splits=1, variant=5)),
]


@pytest.mark.parametrize("case,abits,wbits,want", EXACT_ROUTES, ids=lambda v: v["route"].replace(" ", "_") if isinstance(v, dict) and "route" in v else None)
def test_exact_layers_equal_the_formula(case, abits, wbits, want, dev, monkeypatch):
    from dgq_amd import _lib, ops
    monkeypatch.delenv("DGQ_GEMM_FORCE", raising=False)
    monkeypatch.delenv("DGQ_GEMM_FUSE_ALL", raising=False)
    d = _planted_exact(case, abits, wbits)
    y_ref, margin = _reference(case, d)
    assert margin < 1.0, "%s: the term magnitudes reach %.3f x 2^24 units — narrow the ranges" % (case["name"], margin)
    B, H, W, Ho, Wo, M, K, taps = lr.geometry(case)
    C = K // taps
    pw = ops.PackedWeight(d["w"].to(dev), d["wdelta"].to(dev), d["wzp"].to(dev), None, d["bias"].to(dev), wbits, C, taps)
    assert torch.equal(pw.codes.cpu().long(), d["qw"])
    ab = ops.DynamicActBinding(pw, abits)
    assert lib_splits(_lib, ops, M, case["N"], ab.Kp, wbits) == want["splits"], "the planner's K split for %s moved" % want["route"]
    spy = routes.Spy(ops, _lib)
    monkeypatch.setattr(ops, "_lib_call", spy)
    y = routes.run_layer(ops, case, ab, d["x"].to(dev), d["residual"].to(dev))
    torch.cuda.synchronize()
    calls = spy.take()
    gemm = [c for c in calls if c["name"] == "dgq_gemm_wxa8"]
    quant = [c for c in calls if c["name"] == "dgq_quant_act_batch"]
    assert [c["name"] for c in calls].count("dgq_act_row_params_batch") == 1, calls
    assert len(gemm) == 1 and gemm[0]["fused"] == want["fused"] and len(quant) == (0 if want["fused"] else 1), (want, calls)
    if "variant" in want:
        assert quant[0]["variant"] == want["variant"], (want, quant)
    got = y.cpu().double()
    if not torch.equal(got, y_ref):
        bad = got != y_ref
        idx = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s [%s]: y differs from the formula on %d of %d elements, first at %s: got %r, want %r"
                             % (case["name"], want["route"], int(bad.sum()), bad.numel(), idx, float(got[idx]), float(y_ref[idx])))


def lib_splits(_lib, ops, M, N, Kp, wbits):
    return _lib.load().dgq_gemm_plan_splits(M, N, Kp, wbits, 1, ops.WORKSPACE_BYTES)


# ----------------------------------------------------------------------------------------------- 4. real-valued layers
def _dynamic_layer(ops, case, d, dev):
    B, H, W, Ho, Wo, M, K, taps = lr.geometry(case)
    pw = ops.PackedWeight(d["w_raw"].to(dev), d["wdelta"].to(dev), d["wzp"].to(dev), None, d["bias"].to(dev), d["wbits"], K // taps, taps)
    return ops.DynamicActBinding(pw, d["abits"])


def _with_cpu_tables(case, d, x_in=None):
    """d under the CPU statement's per-row tables of x_in (default: the recipe's own input)"""
    x = d["x"] if x_in is None else x_in
    if case["kind"] == "linear":
        M, K = x.shape[-2], x.shape[-1]
        dr, zr = cpu_tables_linear(x.reshape(M, K), d["abits"])
        return dict(d, adelta=dr.view(1, M, 1), azp=zr.view(1, M, 1))
    dr, zr = cpu_tables_conv(x, d["abits"], case["k"], case["stride"], case["pad"], case["upsample"])
    return dict(d, adelta=dr, azp=zr)


def _reference_real(case, d, x_in=None):
    if case["kind"] == "linear":
        return lr.reference_of(d, case, x=x_in)[0]
    x = d["x"] if x_in is None else x_in
    return torch.cat([lr.reference_of(dict(d, residual=d["residual"][b:b + 1], adelta=d["adelta"][b].view(1, 1, -1), azp=d["azp"][b].view(1, 1, -1)),
                                      case, x=x[b:b + 1])[0] for b in range(x.shape[0])])


@pytest.mark.parametrize("name", ["conv3x3_b2_c32_9x9_s1_n24", "linear_m154_k768_n320", "linear_m2048_k640_n640"])
def test_real_layers_vs_reference(name, dev, monkeypatch, capsys):
    """no prologue: the codes are identical to the reference's under the same tables, only the GEMM's fp32 order remains — 2e-5 (F3)"""
    from dgq_amd import ops
    monkeypatch.delenv("DGQ_GEMM_FORCE", raising=False)
    monkeypatch.delenv("DGQ_GEMM_FUSE_ALL", raising=False)
    case = lr.CASES_BY_NAME[name]
    d = _with_cpu_tables(case, lr.real_case(case, "perM"))
    y_ref = _reference_real(case, d)
    ab = _dynamic_layer(ops, case, d, dev)
    errs = []
    for fuse in (True, False):
        monkeypatch.setattr(ops, "GEMM_FUSE", fuse)
        monkeypatch.setattr(ops, "CONV_FUSE", fuse)
        y = routes.run_layer(ops, case, ab, d["x"].to(dev), d["residual"].to(dev))
        torch.cuda.synchronize()
        errs.append(rel_l2(y.cpu(), y_ref))
    with capsys.disabled():
        print("\nREAL-TIME %s: rel-L2 vs float64 planner %.3g two-launch %.3g" % (name, errs[0], errs[1]))
    assert max(errs) <= 2e-5, errs


# ----------------------------------------------------------------------------------------------- 5. folded prologues
@pytest.mark.parametrize("fold,name", [("geglu", "linear_m2048_k1280_n320"), ("gn_silu", "conv3x3_b2_c64_64x64_s1_n64"), ("ln", "linear_m2048_k640_n640")])
def test_real_layers_folded_prologue(fold, name, dev, monkeypatch, capsys):
    """GroupNorm + SiLU, LayerNorm and GEGLU folded into the load, against the fp32 CPU prologue followed by the float64 formula under the
    CPU statement's tables of that prologue'd input: y within 2e-3, the bound of tests/test_gpu_layer_routes.py::
    test_real_layer_folded_prologue for these shapes (the folded norm rounds differently from the materialised one)."""
    from dgq_amd import ops
    monkeypatch.delenv("DGQ_GEMM_FORCE", raising=False)
    monkeypatch.delenv("DGQ_GEMM_FUSE_ALL", raising=False)
    case = lr.CASES_BY_NAME[name]
    d = lr.real_case(case, "perM")
    g = torch.Generator().manual_seed(17)
    B, H, W, Ho, Wo, M, K, taps = lr.geometry(case)
    x = d["x"]
    if fold == "gn_silu":
        C = case["C"]
        gam, bet = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
        x_in = F.silu(F.group_norm(x, 32, gam, bet, 1e-5))
        kw = dict(norm=(32, 1e-5, gam.to(dev), bet.to(dev), 1))
    elif fold == "ln":
        gam, bet = 1 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
        x_in = F.layer_norm(x, (K,), gam, bet, 1e-5)
        kw = dict(ln=(gam.to(dev), bet.to(dev), 1e-5))
    else:
        x = torch.cat([x, torch.randn(x.shape, generator=g)], dim=-1)                 # [1, M, 2K]: value ‖ gate
        x_in = x[..., :K] * F.gelu(x[..., K:])
        kw = dict(pre_act=2)
    d = _with_cpu_tables(case, d, x_in)
    y_ref = _reference_real(case, d, x_in)
    ab = _dynamic_layer(ops, case, d, dev)
    errs = []
    for fuse in (True, False):
        monkeypatch.setattr(ops, "GEMM_FUSE", fuse)
        monkeypatch.setattr(ops, "CONV_FUSE", fuse)
        y = routes.run_layer(ops, case, ab, x.to(dev), d["residual"].to(dev), **kw)
        torch.cuda.synchronize()
        errs.append(rel_l2(y.cpu(), y_ref))
    with capsys.disabled():
        print("\nREAL-TIME PROLOGUE %s %s: rel-L2 planner %.3g two-launch %.3g" % (fold, name, errs[0], errs[1]))
    assert max(errs) < 2e-3, errs


# ----------------------------------------------------------------------------------------------- 6. row independence
@pytest.mark.parametrize("M,K,N", [(154, 768, 320), (2048, 320, 320)])
def test_rows_are_independent(M, K, N, dev):
    """permuting the rows of a Linear input (same M, same plan) permutes the output rows bit for bit"""
    from dgq_amd import ops
    g = torch.Generator().manual_seed(M + N)
    x = (torch.randn(M, K, generator=g) * 1.3 + 0.2).to(dev)
    ab = ops.DynamicActBinding(_packed(ops, dev, N, K, 1, 9), 8)
    perm = torch.randperm(M, generator=g).to(dev)
    y = ops.quant_linear(x, ab)
    yp = ops.quant_linear(x[perm].contiguous(), ab)
    assert torch.equal(yp, y[perm])


def test_standalone_quantizer_forward(dev):
    """UniformAffineQuantizer(real_time=True).forward — the fake-quant path: dgq_act_row_params + dgq_fakequant_rows == the oracle's
    quantise-dequantise under the CPU statement's per-row tables"""
    from oracle import dgq_oracle as orc
    from dgq_amd.quant.quant_layer import UniformAffineQuantizer
    g = torch.Generator().manual_seed(4)
    x = special_rows(torch.randn(2 * 37, 320, generator=g) * 1.3 + 0.2).view(2, 37, 320)
    q = UniformAffineQuantizer(bits=6, real_time=True)
    y = q(x.to(dev))
    dr, zr = cpu_tables_linear(x.view(-1, 320), 6)
    want = orc.uaq(x.view(-1, 320), dr.view(-1, 1), zr.view(-1, 1), 6).view(x.shape)
    assert torch.equal(y.cpu(), want)
    with pytest.raises(NotImplementedError):
        q(torch.zeros(1, 4, 8, 8, device=dev))


# ----------------------------------------------------------------------------------------------- 7. model level
def _build_qnn(path, dev, steps=25, time_aware=False, real_time=True):
    from dgq_amd import synth
    from dgq_amd.diffusers_rewrite import UNet2DConditionModel
    from dgq_amd.quant import get_qmodel, Scaler
    from dgq_amd.runtime import quant_params
    unet = UNet2DConditionModel("tiny")
    unet.load_state_dict(synth.state_dict_from_ckpt(path))
    wq, aq, sm = quant_params(Scaler, 4, 8, True, True, True, True)
    if real_time:
        aq["real_time"] = True
    qnn = get_qmodel("tiny", types.SimpleNamespace(unet=unet), path, wq, True, aq, sm, False, steps, time_aware, device=dev)
    qnn = qnn.float().to(dev)
    qnn.disable_out_quantization()
    return qnn


@pytest.fixture(scope="module")
def rt_ckpts(tmp_path_factory):
    """a weight-only synthetic checkpoint, and the same weights with act_* blocks (which the real-time mode ignores)"""
    from dgq_amd import synth
    d = tmp_path_factory.mktemp("rt_ck")
    wonly, full = str(d / "wonly.pth"), str(d / "full.pth")
    synth.write_cali_ckpt(wonly, "tiny", 4, 8, 1, num_slots=1, seed=0, batch=2, res=16, start_peak=True, with_act=False)
    synth.write_cali_ckpt(full, "tiny", 4, 8, 4, num_slots=2, seed=0, batch=2, res=16, start_peak=True, with_act=True)
    return wonly, full


@pytest.fixture(scope="module")
def rt_inputs(dev):
    from dgq_amd import synth
    inp = synth.synth_inputs("tiny", 2, 1, 16)
    return inp["sample"].to(dev), inp["encoder_hidden_states"].to(dev)


@pytest.fixture(scope="module")
def rt_qnn(rt_ckpts, dev):
    return _build_qnn(rt_ckpts[0], dev)


def _inner_layers(qnn):
    from dgq_amd.quant import QuantLayer
    return {n: m for n, m in qnn.model.named_modules() if isinstance(m, QuantLayer) and m.use_wq and m.use_aq and not m.disable_aq}


def _layer_reference(layer, x_in):
    """float64 output of one QuantLayer on the (prologue'd, CPU fp32) input x_in under the CPU statement's per-row tables"""
    w = layer.dequantized_weight(torch.float32).float().cpu().contiguous()
    b = layer.b.detach().float().cpu() if layer.b is not None else None
    bits = layer.aqtizer.bits
    if layer.is_conv:
        kh, kw, st, pd = layer._conv_geom()
        dr, zr = cpu_tables_conv(x_in, bits, kh, st, pd)
        return torch.cat([lr.reference_layer(x_in[i:i + 1], w, b, dr[i].view(1, 1, -1), zr[i].view(1, 1, -1), bits, "conv", kh, st, pd)[0]
                          for i in range(x_in.shape[0])])
    K = x_in.shape[-1]
    x2 = x_in.reshape(1, -1, K)
    dr, zr = cpu_tables_linear(x2[0], bits)
    return lr.reference_layer(x2, w, b, dr.view(1, -1, 1), zr.view(1, -1, 1), bits, "linear")[0].reshape(*x_in.shape[:-1], -1)


def _prologue_input(mods, name, x):
    """the tensor the quantiser of layer ``name`` sees when its call folded a prologue: the norm / activation in front of it, in fp32
    on the CPU (the module graph of diffusers_rewrite/unet.py and quant_block.py)"""
    cpu = lambda p: p.detach().float().cpu()
    parent, leaf = name.rsplit(".", 1)
    if leaf in ("time_emb_proj", "linear_2"):
        return F.silu(x)
    if leaf in ("conv1", "conv2", "proj_in"):
        norm = mods[parent + (".norm" if leaf == "proj_in" else ".norm" + leaf[-1])]
        y = F.group_norm(x, norm.num_groups, cpu(norm.weight), cpu(norm.bias), norm.eps)
        return y if leaf == "proj_in" else F.silu(y)
    if leaf in ("to_q", "to_k", "to_v"):
        block, attn = parent.rsplit(".", 1)
        norm = mods[block + (".norm1" if attn == "attn1" else ".norm2")]
    elif name.endswith(".ff.net.0.proj"):
        norm = mods[name[:-len(".ff.net.0.proj")] + ".norm3"]
    else:
        raise AssertionError("layer %s reported a folded prologue this test does not know" % name)
    return F.layer_norm(x, norm.normalized_shape, cpu(norm.weight), cpu(norm.bias), norm.eps)


def test_model_teacher_forced_vs_reference(rt_qnn, rt_inputs, capsys):
    """arch ``tiny`` from a WEIGHT-ONLY checkpoint, get_qmodel(use_aq=True) with real-time aq_params, the fused graph: every quantised
    layer reports once through LAYER_TAP and is within 2e-5 (no prologue) / 2e-3 (folded GroupNorm / LayerNorm / SiLU: the bound of
    the layer-level prologue test) of the float64 formula on its OWN tapped input under the CPU statement's tables; the layer's output is
    replaced by that reference (teacher-forced)."""
    from dgq_amd.quant import quant_layer
    qnn = rt_qnn
    inner = _inner_layers(qnn)
    names = {id(m): n for n, m in inner.items()}
    mods = dict(qnn.model.named_modules())
    seen, errs = [], {False: [], True: []}

    def tap(layer, y, x=None, prologue=False, residual=None, bias_rows=None, fq=None, geglu=False):
        name = names[id(layer)]
        seen.append(name)
        assert fq is None
        x_in = x.detach().float().cpu()
        if prologue:
            x_in = _prologue_input(mods, name, x_in)
        ref = _layer_reference(layer, x_in)
        if geglu:
            a, gte = ref.chunk(2, dim=-1)
            ref = a * F.gelu(gte)
        ref = ref.reshape(y.shape)
        if residual is not None:
            ref = ref + residual.detach().double().cpu().reshape(y.shape)
        if bias_rows is not None:
            ref = ref + bias_rows.detach().double().cpu()[:, :, None, None]
        errs[bool(prologue)].append((rel_l2(y.detach().cpu(), ref), name))
        return ref.to(y.device, y.dtype)

    quant_layer.LAYER_TAP = tap
    try:
        with torch.no_grad():
            out = qnn(rt_inputs[0], torch.tensor(999), rt_inputs[1])[0]
    finally:
        quant_layer.LAYER_TAP = None
    assert torch.isfinite(out).all()
    assert sorted(seen) == sorted(inner), "layers not seen exactly once: %s" % (set(inner) ^ set(seen) or [n for n in seen if seen.count(n) > 1])
    assert len(inner) == 119
    worst = {k: max(v) for k, v in errs.items() if v}
    with capsys.disabled():
        print("\nREAL-TIME MODEL tiny: %d layers without a prologue, worst %.3g (%s); %d with one, worst %.3g (%s)"
              % (len(errs[False]), *worst[False], len(errs[True]), *worst[True]))
    assert worst[False][0] <= 2e-5, worst[False]
    assert worst[True][0] < 2e-3, worst[True]


def _packed_images(qnn):
    """{data_ptr: bytes} of every packed weight image the model's layers hold (bindings and PackedWeight caches)"""
    imgs = {}
    for layer in _inner_layers(qnn).values():
        for ab in layer._bindings.values():
            for t in (ab.wpacked, getattr(ab, "wfrag", None)):
                if t is not None:
                    imgs[t.data_ptr()] = t.numel() * t.element_size()
    return imgs


def test_model_graph_replay_images_and_loader(rt_qnn, rt_ckpts, rt_inputs, dev):
    from dgq_amd import ops
    from dgq_amd.quant import get_qmodel
    qnn = rt_qnn
    x, ctx = rt_inputs
    with torch.no_grad():
        y_e = qnn(x, torch.tensor(999), ctx)[0].clone()
        y_e2 = qnn(x, torch.tensor(499), ctx)[0].clone()
        qnn.enable_graphs(True)
        y_g = qnn(x, torch.tensor(999), ctx)[0].clone()
        y_g_again = qnn(x, torch.tensor(999), ctx)[0].clone()
        qnn.enable_graphs(False)
    assert torch.isfinite(y_e).all() and not torch.equal(y_e, y_e2)
    assert torch.equal(y_g, y_e) and torch.equal(y_g_again, y_e), "graph replay differs from the eager run"
    # exactly one natural-order image (and its fragment-major twin) per layer, after forwards at two timesteps
    inner = _inner_layers(qnn)
    for name, layer in inner.items():
        assert list(layer._bindings) == ["real_time"] and isinstance(layer._bindings["real_time"], ops.DynamicActBinding), name
        ab, pw = layer._bindings["real_time"], layer._pw
        assert ab.wpacked is pw._natural[0] and ab.wfrag is pw._natural_frag and ab.wfrag is not None, name
        assert not layer._act_tables
    imgs = _packed_images(qnn)
    assert len(imgs) == 2 * len(inner)
    # ... whatever num_inference_steps: a 50-step model from the checkpoint WITH act_* blocks holds the same images and computes the same
    qnn50 = _build_qnn(rt_ckpts[1], dev, steps=50)
    with torch.no_grad():
        y50 = qnn50(x, torch.tensor(999), ctx)[0]
        qnn50(x, torch.tensor(21), ctx)
    imgs50 = _packed_images(qnn50)
    assert sorted(imgs50.values()) == sorted(imgs.values())
    assert torch.equal(y50, y_e), "the act_* blocks of the checkpoint changed the result"
    with pytest.raises(ValueError):
        _build_qnn(rt_ckpts[0], dev, time_aware=True)


# ----------------------------------------------------------------------------------------------- 8. CLI
def test_cli_aq_real_time(tmp_path):
    from dgq_amd import inference_qmodel as cli
    out = str(tmp_path / "lat_{rank}.pt")
    cli.main(["--model_type", "tiny", "--use_aq", "--aq_real_time", "--t2i_log_quant", "--t2i_real_time", "--num_inference_steps", "2",
              "--out", out])
    d = torch.load(out.format(rank=0))
    assert sorted(d) == [0, 1] and all(torch.isfinite(v).all() for v in d.values())
