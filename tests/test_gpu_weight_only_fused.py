"""Weight-only matrix-core layers with their element-wise neighbours folded in (dgq_conv2d_wq_mfma16_fused, dgq_layernorm_row_stats,
ops.conv2d_wq_mfma16_fused, QuantLayer.weight_only_fused, QuantModel.set_weight_only_fused).

The contract, as for the un-fused entry (tests/test_gpu_weight_only_mfma16.py), has two halves:
  * where every operation is exact in fp32 (planted small-integer data and tables, power-of-two δ) the result is the float64 value of
    the statement rounded once, bit for bit: a border tap that picks up the shift, the neighbouring image's tables, a wrong lane pair
    of the GEGLU epilogue show as wrong numbers;
  * on random data every element is under the a-priori bound of tests/weight_only_fused_ref.py (derived there; its CPU self-check shows
    that the bound notices each of those mistakes), with the SAME fp32 tables on both sides: real dgq_groupnorm_scale_shift output
    and real dgq_layernorm_row_stats output.
With nothing to fold the entry is dgq_conv2d_wq_mfma16 itself.  The first test needs no GPU."""
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from dgq_amd import ops, _lib
from tests import weight_only_fused_ref as fr

gpu = pytest.mark.gpu
DT_IDS = ["fp32", "bf16", "f16"]


# ------------------------------------------------------------------------------------------------------------- exports and refusals
def test_exports_and_refusals():
    lib = _lib.load()
    assert lib.dgq_version() == 123
    assert len(_lib.SIGNATURES["dgq_conv2d_wq_mfma16_fused"]) == len(_lib.SIGNATURES["dgq_conv2d_wq_mfma16"]) + 1 == 24
    assert len(_lib.SIGNATURES["dgq_layernorm_row_stats"]) == 7
    f, g = lib.dgq_conv2d_wq_mfma16_fused, lib.dgq_layernorm_row_stats
    p = 1 << 20                             # never dereferenced: every call below is refused before a launch

    def call(fuse, kh=1, N=32, geglu_rows=0, ldy=32):
        fz = _lib.Wq16Fuse()
        for k, v in fuse.items():
            setattr(fz, k, v)
        return f(p, 0, 1, 4, 4, 64, kh, kh, 1, kh // 2, 0, p, 4, 640 if kh == 3 else 128, p, p, None, N, geglu_rows, p, 0, ldy, ctypes.byref(fz), None)
    for fuse, kw, what in [(dict(pre_scale=p, pre_shift=p, ln_stats=p, ln_gamma=p, ln_beta=p), {}, "both"),
                           (dict(ln_stats=p, ln_gamma=p, ln_beta=p), dict(kh=3), "Linear"),
                           (dict(geglu_out=1, residual=p, ldr=32), dict(geglu_rows=1), "residual"),
                           (dict(residual=p, ldr=16), {}, "ldr"),
                           (dict(ln_stats=p), {}, "gamma and beta"),
                           (dict(pre_scale=p), {}, "pre_shift"),
                           (dict(geglu_out=1), {}, "geglu_rows"),
                           (dict(pre_act=2), {}, "pre_act"),
                           ({}, dict(N=8, ldy=8), "N=8")]:
        assert call(fuse, **kw) == -1, (fuse, kw)
        assert "dgq_conv2d_wq_mfma16_fused" in _lib.last_error() and what in _lib.last_error(), (fuse, _lib.last_error())
    for C in (6, 4096):
        assert g(p, 0, 4, C, ctypes.c_float(1e-5), p, None) == -1
        assert "dgq_layernorm_row_stats" in _lib.last_error() and "C=%d" % C in _lib.last_error()
    assert not ops.layernorm_row_stats_ok(6) and not ops.layernorm_row_stats_ok(4096) and ops.layernorm_row_stats_ok(320)


def test_switch_and_cli_refusal():
    from dgq_amd import inference_qmodel
    from dgq_amd.quant import QuantLayer
    assert QuantLayer.weight_only_fused is False
    for argv, word in [(["--wq_fused", "--model_type", "tiny"], "--wq_mfma16"), (["--wq_fused", "--wq_mfma16", "--use_aq", "--model_type", "tiny"], "--use_aq")]:
        with pytest.raises(SystemExit) as e:
            inference_qmodel.main(argv)
        assert word in str(e.value)
    assert inference_qmodel.parse_args([]).wq_fused is False and inference_qmodel.parse_args(["--wq_fused"]).wq_fused is True


# ------------------------------------------------------------------------------------------------------------- helpers
def _row_perm(N):
    return torch.stack([torch.arange(N // 2), torch.arange(N // 2) + N // 2], 1).flatten()


def _pack(name, w, delta, zp, b, bits, geglu):
    c = fr.GEOM[name]
    w, delta, zp, b = w.cuda(), delta.cuda(), zp.cuda(), b.cuda()
    if geglu:
        rp = _row_perm(c["N"]).cuda()
        w, delta, zp, b = w[rp], delta[rp], zp[rp], b[rp]
    return ops.PackedWeight(w, delta, zp, None, b, bits, c["C"], c["k"] * c["k"])


def _fused(name, x, pw, fz, geglu_rows):
    """ops.conv2d_wq_mfma16_fused on the case with the fused inputs fz (CPU tensors), as [M][cols] rows on the CPU"""
    c = fr.GEOM[name]
    kw = {}
    if "scale" in fz:
        kw["norm"] = (fz["scale"].cuda(), fz["shift"].cuda())
    if "ln_stats" in fz:
        kw["ln"] = (fz["ln_stats"].cuda(), fz["gamma"].cuda(), fz["beta"].cuda())
    if "residual" in fz:
        kw["residual"] = fr.nchw_of(name, fz["residual"].cuda())
    if "bias_rows" in fz:
        kw["bias_rows"] = fz["bias_rows"].cuda()
    y = ops.conv2d_wq_mfma16_fused(x.cuda(), pw, c["k"], c["k"], c["s"], c["p"], upsample=c["ups"], geglu_rows=geglu_rows,
                                   pre_act=fz.get("act", 0), geglu=bool(fz.get("geglu")), **kw)
    return fr.rows_of(name, y).cpu()


def _w_int(codes, zp):
    return fr.weight_rows(codes.float() - zp.view(-1, *([1] * (codes.dim() - 1))))


# ------------------------------------------------------------------------------------------------------------- empty fuse
@gpu
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dtype", fr.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", ["linear_70x360_72", "conv3_s2", "conv3_upsample_4x4", "conv3_c7_s2", "t64_1000x72_1030"])
def test_empty_fuse_is_the_unfused_entry(name, dtype, bits):
    c = fr.GEOM[name]
    x, w, _codes, delta, zp, bias, _fz = fr.random_case(name, "res", dtype, bits)
    with torch.no_grad():
        pw = _pack(name, w, delta, zp, bias, bits, False)
        y0 = ops.conv2d_wq_mfma16(x.cuda(), pw, c["k"], c["k"], c["s"], c["p"], upsample=c["ups"])
        y1 = ops.conv2d_wq_mfma16_fused(x.cuda(), pw, c["k"], c["k"], c["s"], c["p"], upsample=c["ups"])
    assert y1.dtype == dtype and torch.equal(y0, y1)


# ------------------------------------------------------------------------------------------------------------- exact planted data
@gpu
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dtype", fr.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name,kind", fr.PLANTED, ids=["%s-%s" % nk for nk in fr.PLANTED])
def test_planted_data_equals_the_float64_formula(name, kind, dtype, bits):
    x, w, codes, delta, zp, bias, fz, y64 = fr.planted_case(name, kind, dtype, bits)
    geglu = bool(fz.get("geglu") or fz.get("perm"))              # (rows packed interleaved; "perm": without the GEGLU epilogue)
    with torch.no_grad():
        pw = _pack(name, w, delta, zp, bias, bits, geglu)
        rp = _row_perm(codes.shape[0]) if geglu else torch.arange(codes.shape[0])
        assert torch.equal(pw.codes.cpu(), codes.flatten(1)[rp].to(torch.uint8)) and pw.mfma16_eligible()     # (the test's own construction)
        y = _fused(name, x, pw, fz, geglu)
    want = y64.to(dtype)
    assert y.dtype == dtype and y.shape == want.shape
    if not torch.equal(y, want):
        d = (y.double() - y64).abs()
        raise AssertionError("differs from the float64 formula in %d of %d elements, max |diff| %.3g" % (int((y != want).sum()), d.numel(), float(d.max())))


# ------------------------------------------------------------------------------------------------------------- random data
@gpu
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dtype", fr.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name,kind", fr.RANDOM, ids=["%s-%s" % nk for nk in fr.RANDOM])
def test_random_data_under_the_bound(name, kind, dtype, bits):
    c, g = fr.GEOM[name], fr.geometry(name)
    x, w, codes, delta, zp, bias, fz = fr.random_case(name, kind, dtype, bits)
    fz = dict(fz)
    geglu = bool(fz.get("geglu") or fz.get("perm"))
    with torch.no_grad():
        xd = x.cuda()
        if "gn" in fz:                         # the library's own tables, of data with |mean| >> std in one group
            groups, eps, gamma, beta = fz["gn"]
            B, C, H, W = x.shape
            xs = xd.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
            sc, sh = ops.groupnorm_scale_shift(xs, B, H * W, C, groups, eps, gamma.cuda(), beta.cuda())
            fz["scale"], fz["shift"] = sc.cpu(), sh.cpu()
        if "ln_stats" in fz:                   # the library's own statistics
            fz["ln_stats"] = ops.layernorm_row_stats(xd, fz["eps"]).cpu()
        fz = fr.kernel_inputs(fz)
        pw = _pack(name, w, delta, zp, bias, bits, geglu)
        assert pw.mfma16_eligible()
        y = _fused(name, x, pw, fz, geglu)
    y64, bound = fr.ref64(name, x, _w_int(codes, zp), delta, bias, fz, dtype)
    worst = fr.worst_ratio(y, y64, bound)
    print("%s %s W%d %s: max |err| / bound = %.3f" % (name, kind, bits, dtype, worst))
    assert y.dtype == dtype and y.shape == y64.shape and worst <= 1.0, worst


# ------------------------------------------------------------------------------------------------------------- row statistics
@gpu
@pytest.mark.parametrize("dtype", fr.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("rows", [1, 37])
@pytest.mark.parametrize("C", [4, 320, 1280, 2048])
def test_layernorm_row_stats_against_float64(C, rows, dtype):
    """rows with |mean| = 100·std: a one-pass variance would lose everything; mean within 4·2^-24·max|x| absolute, rstd within 4·2^-24
    relative of the float64 statistics of the same (rounded) data.  (row_layernorm_stats — fp32 throughout, four roundings
    behind an fp32 sum of 2048 squares — cannot promise this tolerance at C = 2048; the entry therefore carries its sums and the final
    arithmetic in fp64.)"""
    g = torch.Generator().manual_seed(C + rows)
    x = (torch.randn(rows, C, generator=g) + 100.0 * (2 * torch.randint(0, 2, (rows, 1), generator=g) - 1)).to(dtype)
    st = ops.layernorm_row_stats(x.cuda(), 1e-5).cpu().double()
    x64 = x.double()
    mu, rstd = x64.mean(-1), 1.0 / torch.sqrt(x64.var(-1, unbiased=False) + 1e-5)
    e_mu = float(((st[:, 0] - mu).abs() / (4 * fr.U * x64.abs().amax(-1))).max())
    e_rs = float(((st[:, 1] - rstd).abs() / (4 * fr.U * rstd)).max())
    print("C %d rows %d %s: mean error / tolerance %.3f, rstd error / tolerance %.3f" % (C, rows, dtype, e_mu, e_rs))
    assert st.shape == (rows, 2) and e_mu <= 1.0 and e_rs <= 1.0


# ------------------------------------------------------------------------------------------------------------- one QuantLayer
ENTRIES = ("dgq_conv2d_wq", "dgq_conv2d_wq_mfma16", "dgq_conv2d_wq_mfma16_fused", "dgq_layernorm_row_stats")


class _Spy:
    """counts the library entries that ops calls"""

    def __init__(self, monkeypatch):
        self.names = []
        orig = ops._lib_call

        def call(name, *a):
            self.names.append(name)
            return orig(name, *a)
        monkeypatch.setattr(ops, "_lib_call", call)

    def take(self):
        n = tuple(self.names.count(k) for k in ENTRIES)
        self.names.clear()
        return n


def _qlayer(mod, bits, dtype, geglu=False):
    from dgq_amd.quant import QuantLayer, Scaler
    q = QuantLayer(mod, wq_params={"bits": bits, "channel_wise": True, "scaler": Scaler.MINMAX},
                   aq_params={"bits": 8, "channel_wise": False, "scaler": Scaler.MINMAX, "leaf_param": False})
    q.set_quant_state(True, False)
    q.geglu_rows = geglu
    q = q.cuda().to(dtype)
    q.weight_only_mfma16 = True
    return q


def _layer_ref(name, layer, x, fz, dtype):
    """(y64, bound) rows of the layer's statement on x with the fused inputs fz (CPU tensors)"""
    pw = layer.packed_weight()
    N = pw.N
    w_int = (pw.codes.double() - pw.zp_true.double()[:, None]).cpu()
    delta, bias = pw.alpha.cpu(), pw.bias.cpu()
    if layer.geglu_rows:
        inv = torch.argsort(_row_perm(N))
        w_int, delta, bias = w_int[inv], delta[inv], bias[inv]
    w_int = fr.weight_rows(w_int.view(N, *layer.w.shape[1:]))
    return fr.ref64(name, x.cpu(), w_int, delta, bias, fz, dtype)


def _check(what, y_rows, ref, dtype):
    y64, bound = ref
    worst = fr.worst_ratio(y_rows.cpu(), y64, bound)
    print("%s %s: max |err| / bound = %.3f" % (what, dtype, worst))
    assert y_rows.dtype == dtype and y_rows.shape == y64.shape and worst <= 1.0, (what, worst)


def _gn_tables(x, norm):
    B, C, H, W = x.shape
    xs = x.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
    sc, sh = ops.groupnorm_scale_shift(xs, B, H * W, C, norm.num_groups, norm.eps, norm.weight, norm.bias)
    return sc.cpu(), sh.cpu()


def _norm(mod, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        mod.weight.copy_(1.0 + 0.2 * torch.randn(mod.weight.shape, generator=g))
        mod.bias.copy_(0.3 * torch.randn(mod.bias.shape, generator=g))
    return mod.cuda().to(dtype)


@gpu
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dtype", fr.DTYPES, ids=DT_IDS)
def test_layer_methods_flag_off_then_on(bits, dtype, monkeypatch):
    """every folding method: with the flag off the old sequence runs (one un-fused entry call, today's bits); with it on exactly one
    fused call, no un-fused one, and the result is under the bound"""
    from dgq_amd.quant import quant_layer
    from dgq_amd.quant.quant_block import QuantResnetBlock2D, PreLN, _apply
    torch.manual_seed(0)
    spy = _Spy(monkeypatch)
    g = torch.Generator().manual_seed(11)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dtype).cuda()
    nac = lambda norm, conv, x, **kw: QuantResnetBlock2D._norm_act_conv(None, norm, conv, x, **kw)
    with torch.no_grad():
        # -- forward_prenorm(norm, silu=True, bias_rows=…) and (..., residual=…), through the resnet block's own call
        name = "layer_conv3_2x64x8x8_96"
        conv = _qlayer(nn.Conv2d(64, 96, 3, padding=1), bits, dtype)
        gn = _norm(nn.GroupNorm(32, 64), dtype, 1)
        x, te, res = rnd(2, 64, 8, 8), rnd(2, 96), rnd(2, 96, 8, 8).contiguous(memory_format=torch.channels_last)
        for kw, fzk in [(dict(bias_rows=te), dict(bias_rows=te.cpu())), (dict(residual=res), dict(residual=fr.rows_of(name, res).cpu()))]:
            conv.weight_only_fused = False
            assert not conv.can_fuse_prenorm(x)
            y_off = nac(gn, conv, x, **kw)
            assert spy.take() == (0, 1, 0, 0)
            h = conv(F.silu(gn(x)))
            today = h + te[:, :, None, None] if "bias_rows" in kw else conv(F.silu(gn(x))) + res
            assert torch.equal(y_off, today)
            spy.take()
            conv.weight_only_fused = True
            assert conv.can_fuse_prenorm(x)
            y_on = nac(gn, conv, x, **kw)
            assert [n for n in spy.names if n in ENTRIES] == ["dgq_conv2d_wq_mfma16_fused"] and spy.take() == (0, 0, 1, 0)
            sc, sh = _gn_tables(x, gn)
            _check("forward_prenorm %s W%d" % (list(kw)[0], bits), fr.rows_of(name, y_on),
                   _layer_ref(name, conv, x, dict(fzk, scale=sc, shift=sh, act=1), dtype), dtype)
        # -- forward_residual
        conv.weight_only_fused = False
        y_off = conv.forward_residual(x, res)
        assert spy.take() == (0, 1, 0, 0) and torch.equal(y_off, conv(x) + res)
        spy.take()
        conv.weight_only_fused = True
        y_on = conv.forward_residual(x, res)
        assert spy.take() == (0, 0, 1, 0)
        _check("forward_residual W%d" % bits, fr.rows_of(name, y_on), _layer_ref(name, conv, x, dict(residual=fr.rows_of(name, res).cpu()), dtype), dtype)

        # -- forward_fused(ln=…, residual=…)
        name = "layer_linear_38x320_72"
        lin = _qlayer(nn.Linear(320, 72), bits, dtype)
        ln = _norm(nn.LayerNorm(320), dtype, 2)
        x, res = rnd(2, 19, 320) + 2.0, rnd(2, 19, 72)
        lin.weight_only_fused = False
        y_off = lin.forward_fused(x, ln=ln, residual=res)
        assert spy.take() == (0, 1, 0, 0) and torch.equal(y_off, lin(ln(x)) + res)
        spy.take()
        lin.weight_only_fused = True
        y_on = lin.forward_fused(x, ln=ln, residual=res)
        assert spy.take() == (0, 0, 1, 1)
        st = ops.layernorm_row_stats(x.reshape(-1, 320), ln.eps)
        fz = dict(ln_stats=st.cpu(), gamma=ln.weight.float().cpu(), beta=ln.bias.float().cpu(), residual=res.reshape(-1, 72).cpu())
        _check("forward_fused ln residual W%d" % bits, y_on.reshape(-1, 72), _layer_ref(name, lin, x.reshape(-1, 320), fz, dtype), dtype)
        # ... γ / β that are views at an odd offset of a larger buffer (not 16-byte aligned in fp32): the op hands the kernel an aligned
        # copy, the layer stays on the fused route and the bits are the same
        buf = torch.zeros(642, device="cuda", dtype=dtype)
        buf[1:321].copy_(ln.weight)
        buf[321:641].copy_(ln.bias)
        ln_odd = nn.LayerNorm(320).cuda().to(dtype)
        ln_odd.weight, ln_odd.bias = nn.Parameter(buf[1:321]), nn.Parameter(buf[321:641])
        assert dtype != torch.float32 or ln_odd.weight.data_ptr() % 16 != 0
        spy.take()
        y_odd = lin.forward_fused(x, ln=ln_odd, residual=res)
        assert spy.take() == (0, 0, 1, 1) and torch.equal(y_odd, y_on)
        # ... three consumers of one PreLN share one statistics launch
        spy.take()
        pre = PreLN(x, ln)
        ys = [_apply(lin, pre) for _ in range(3)]
        assert spy.take() == (0, 0, 3, 1) and torch.equal(ys[0], ys[2])
        lin.weight_only_fused = False
        pre = PreLN(x, ln)
        ys_off = [_apply(lin, pre) for _ in range(3)]
        assert spy.take() == (0, 3, 0, 0) and torch.equal(ys_off[0], lin(ln(x)))
        spy.take()

        # -- forward_fused(geglu=True) with geglu_rows
        name = "linear_33x64_128"
        ff = _qlayer(nn.Linear(64, 128), bits, dtype, geglu=True)
        x = rnd(33, 64)
        ff.weight_only_fused = False
        y_off = ff.forward_fused(x, geglu=True)
        a, gt = ff(x).chunk(2, dim=-1)
        assert spy.take() == (0, 2, 0, 0) and torch.equal(y_off, a * F.gelu(gt))
        ff.weight_only_fused = True
        y_on = ff.forward_fused(x, geglu=True)
        assert spy.take() == (0, 0, 1, 0) and y_on.shape == (33, 64)
        _check("forward_fused geglu W%d" % bits, y_on, _layer_ref(name, ff, x, dict(geglu=True), dtype), dtype)
        # ... and a residual on the same interleaved layer without the GEGLU: it is added at the output's columns, not the packed ones
        res = rnd(33, 128)
        y_on = ff.forward_fused(x, residual=res)
        assert spy.take() == (0, 0, 1, 0) and y_on.shape == (33, 128)
        _check("forward_fused geglu_rows residual W%d" % bits, y_on, _layer_ref(name, ff, x, dict(residual=res.cpu()), dtype), dtype)

        # -- forward_fused(pre_act=1) at M = 2 (time_emb_proj)
        name = "layer_linear_2x1280_320"
        tp = _qlayer(nn.Linear(1280, 320), bits, dtype)
        x = rnd(2, 1280)
        tp.weight_only_fused = False
        y_off = tp.forward_fused(x, pre_act=1)
        assert spy.take() == (0, 1, 0, 0) and torch.equal(y_off, tp(F.silu(x)))
        spy.take()
        tp.weight_only_fused = True
        y_on = tp.forward_fused(x, pre_act=1)
        assert spy.take() == (0, 0, 1, 0)
        _check("forward_fused silu M=2 W%d" % bits, y_on, _layer_ref(name, tp, x, dict(act=1), dtype), dtype)

        # -- forward_prenorm_tokens / forward_residual_tokens (SDXL's Linear proj_in / proj_out)
        name = "layer_conv1_2x64x6x6_64"
        pj = _qlayer(nn.Linear(64, 64), bits, dtype)
        gn = _norm(nn.GroupNorm(32, 64, eps=1e-6), dtype, 3)
        x = rnd(2, 64, 6, 6)
        tok = lambda t: t.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1).reshape(2, 36, -1)
        pj.weight_only_fused = False
        assert not pj.can_fuse_tokens(x)
        y_off = pj(tok(gn(x)))                                   # (Transformer2DModel's own sequence with the flag off)
        assert spy.take() == (0, 1, 0, 0)
        pj.weight_only_fused = True
        assert pj.can_fuse_tokens(x)
        y_on = pj.forward_prenorm_tokens(x, gn)
        assert spy.take() == (0, 0, 1, 0) and y_on.shape == y_off.shape
        sc, sh = _gn_tables(x, gn)
        _check("forward_prenorm_tokens W%d" % bits, y_on.reshape(-1, 64), _layer_ref(name, pj, x, dict(scale=sc, shift=sh), dtype), dtype)
        hh, res = rnd(2, 36, 64), rnd(2, 64, 6, 6)
        y_on = pj.forward_residual_tokens(hh, res)
        assert spy.take() == (0, 0, 1, 0) and y_on.shape == res.shape
        xin = hh.reshape(2, 6, 6, 64).permute(0, 3, 1, 2)
        _check("forward_residual_tokens W%d" % bits, fr.rows_of(name, y_on), _layer_ref(name, pj, xin, dict(residual=fr.rows_of(name, res).cpu()), dtype), dtype)
        pj.weight_only_fused = False
        y_off = pj(hh).reshape(2, 6, 6, 64).permute(0, 3, 1, 2) + res
        assert spy.take() == (0, 1, 0, 0)
        print("tokens: rel-L2 fused against un-fused %.3e" % float((y_on.double() - y_off.double()).norm() / y_off.double().norm()))

        # -- an ineligible weight (fractional zero point) and an installed layer tap stay on today's path with the flag on
        lin.weight_only_fused = True
        x, res = rnd(2, 19, 320), rnd(2, 19, 72)
        monkeypatch.setattr(quant_layer, "LAYER_TAP", lambda layer, y, **info: y)
        assert not lin.takes_fused(x)
        y_tap = lin.forward_fused(x, ln=ln, residual=res)
        assert spy.take() == (0, 1, 0, 0) and torch.equal(y_tap, lin(ln(x)) + res)
        monkeypatch.setattr(quant_layer, "LAYER_TAP", None)
        spy.take()
        assert lin.takes_fused(x)
        lin.wqtizer.zero_point.add_(0.5)
        assert not lin.takes_fused(x)
        y = lin.forward_fused(x, ln=ln, residual=res)
        assert spy.take() == (1, 0, 0, 0) and torch.isfinite(y.float()).all()


# ------------------------------------------------------------------------------------------------------------- tiny UNet
def _tiny_qnn(bits):
    from dgq_amd import synth
    from dgq_amd.diffusers_rewrite import UNet2DConditionModel
    from dgq_amd.quant import QuantModel, Scaler, QMODE
    unet = UNet2DConditionModel("tiny")
    unet.load_state_dict(synth.synth_state_dict("tiny", 0))
    qnn = QuantModel(model=unet, wq_params={"bits": bits, "channel_wise": True, "scaler": Scaler.MINMAX},
                     aq_params={"bits": 8, "channel_wise": False, "scaler": Scaler.MINMAX, "leaf_param": False},
                     softmax_aq_params={"softmax_a_bit": 8, "t2i_log_quant": False, "t2i_real_time": False, "t2i_start_peak": False,
                                        "log_max_1": False},
                     aq_mode=[QMODE.NORMAL.value, QMODE.QDIFF.value], tib_recon=False).cuda().eval()
    qnn.set_quant_state(True, False)
    qnn.disable_out_quantization()
    return qnn


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


class _Counters:
    """calls of nn.GroupNorm.forward, nn.LayerNorm.forward, F.gelu and F.silu; SiLU calls made while the timestep-embedding MLP runs
    are counted apart: that module's SiLU is not a neighbour of a resnet or transformer layer (DESIGN.md §8 lists it as not built; where
    the module hands it to linear_2.forward_fused it folds like time_emb_proj's, and the count is 0)"""

    def __init__(self, monkeypatch, qnn):
        self.n = dict(gn=0, ln=0, gelu=0, silu=0, silu_time_mlp=0)
        self.in_mlp = False

        def counted(key, fn):
            def call(*a, **k):
                self.n["silu_time_mlp" if key == "silu" and self.in_mlp else key] += 1
                return fn(*a, **k)
            return call
        gn_fwd, ln_fwd = nn.GroupNorm.forward, nn.LayerNorm.forward
        monkeypatch.setattr(nn.GroupNorm, "forward", counted("gn", gn_fwd))
        monkeypatch.setattr(nn.LayerNorm, "forward", counted("ln", ln_fwd))
        monkeypatch.setattr(F, "gelu", counted("gelu", F.gelu))
        monkeypatch.setattr(F, "silu", counted("silu", F.silu))
        mlp = qnn.model.time_embedding
        mlp_fwd = mlp.forward

        def mlp_call(*a, **k):
            self.in_mlp = True
            try:
                return mlp_fwd(*a, **k)
            finally:
                self.in_mlp = False
        monkeypatch.setattr(mlp, "forward", mlp_call)

    def take(self):
        n = dict(self.n)
        for k in self.n:
            self.n[k] = 0
        return n


@gpu
def test_tiny_unet_routing_graphs_and_accuracy(monkeypatch):
    """W4, fp32 and bf16 states, the matrix-core switch on throughout; the fused flag off, then on."""
    from dgq_amd import synth
    from dgq_amd.quant.quant_block import QuantBasicTransformerBlock
    spy = _Spy(monkeypatch)
    qnn = _tiny_qnn(4)
    cnt = _Counters(monkeypatch, qnn)
    inp = synth.synth_inputs("tiny", 2, 1, 16)
    x, ctx, t = inp["sample"].cuda(), inp["encoder_hidden_states"].cuda(), torch.tensor(999)
    n_blocks = sum(isinstance(m, QuantBasicTransformerBlock) for m in qnn.modules())
    out = {}
    with torch.no_grad():
        for dtype in (torch.float32, torch.bfloat16):
            if dtype == torch.bfloat16:
                qnn = qnn.to(torch.bfloat16)
            xd, cd = x.to(dtype), ctx.to(dtype)
            # the yardstick, on existing code only: the exact route in this state
            qnn.set_weight_only_mfma16(False)
            qnn.set_weight_only_fused(False)
            out["exact", dtype] = qnn(xd, t, cd)[0].clone()
            n_exact = spy.take()
            assert n_exact[0] > 0 and n_exact[1:] == (0, 0, 0)
            qnn.set_weight_only_mfma16(True)
            cnt.take()
            out["off", dtype] = qnn(xd, t, cd)[0].clone()
            n_off, c_off = spy.take(), cnt.take()
            assert n_off == (0, n_exact[0], 0, 0)                        # today's counts: every call on the un-fused entry
            assert c_off["gn"] > 0 and c_off["ln"] > 0 and c_off["silu"] > 0
            qnn.set_weight_only_fused(True)
            out["on", dtype] = qnn(xd, t, cd)[0].clone()
            n_on, c_on = spy.take(), cnt.take()
            print("%s state: entry calls (exact, mfma16, fused, row stats) off %s on %s; torch operators off %s on %s" % (dtype, n_off, n_on, c_off, c_on))
            assert n_on[0] == 0 and n_on[2] > 0 and n_on[1] + n_on[2] == n_off[1]
            assert c_on["gn"] == 0 and c_on["ln"] == 0 and c_on["gelu"] == 0 and c_on["silu"] == 0
            assert n_on[3] == 3 * n_blocks                               # norm1 (to_q, to_k, to_v share it), norm2, norm3 of every block
            assert out["on", dtype].dtype == dtype and torch.isfinite(out["on", dtype].float()).all()
            # graph replay == eager, bit for bit; the setter after a capture gives the other route, not a stale replay
            qnn.enable_graphs(True)
            qnn(xd, t, cd)
            y_graph = qnn(xd, t, cd)[0].clone()
            spy.take()
            qnn.set_weight_only_fused(False)
            y_flip = qnn(xd, t, cd)[0].clone()
            n_flip = spy.take()
            assert n_flip[2] == 0 and n_flip[1] == 2 * n_off[1]          # (warmed up and captured again, on the un-fused route)
            y_flip_replay = qnn(xd, t, cd)[0].clone()
            assert spy.take() == (0, 0, 0, 0)                            # (a replay: no entry is called)
            qnn.enable_graphs(False)
            assert torch.equal(y_graph, out["on", dtype])
            assert torch.equal(y_flip, out["off", dtype]) and torch.equal(y_flip_replay, out["off", dtype])
            assert not torch.equal(out["on", dtype], out["off", dtype])
    d0 = _rel(out["exact", torch.bfloat16].float(), out["exact", torch.float32])
    d_bf16 = _rel(out["on", torch.bfloat16], out["off", torch.bfloat16])
    d_fp32 = _rel(out["on", torch.float32], out["off", torch.float32])
    print("W4 tiny UNet: d0 (exact bf16 state vs exact fp32 state) %.3e; fused vs un-fused mfma16: bf16 state %.3e, fp32 state %.3e" % (d0, d_bf16, d_fp32))
    assert d_bf16 <= d0 and d_fp32 <= d0
