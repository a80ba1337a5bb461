"""Real-time MXFP4 activations on the block-scaled matrix cores (UniformAffineQuantizer(real_time=True, real_time_block=32,
real_time_format="mxfp4"): dgq_quant_act_mx4 + dgq_gemm_mx4, W4A4) — a mode of this library.

The quantiser must reproduce ``quant_layer.mx4_block`` BIT FOR BIT (== the float64 restatement of tests/mxfp4_ref.py).  The operand maps
of the mixed FP4 x FP6 V_MFMA_SCALE_F32_32X32X64_F8F6F4 (nibble order, register placement, which operand carries which format, which
scale byte goes with which K block) are pinned by one-hot operands whose output is a gather; layers on planted exact data EQUAL the
float64 layer, split or not; real-valued layers stay inside the a-priori bound of an fp32 sum (constant 1)."""
import pytest
import torch
import torch.nn.functional as F

from tests import layer_reference as lr
from tests import mxfp4_ref as mx
from tests import realtime_block_ref as rb
from tests import test_gpu_groupnorm_stats as gs
from tests import test_gpu_layer_routes as routes
from tests import test_gpu_realtime_act as rta
from tests import test_gpu_realtime_mxfp6 as t6
from tests.test_gpu_realtime_act import dev, rt_inputs, rel_l2          # noqa: F401  (module-scoped fixtures of the row mode)
from tests.test_realtime_mxfp4_cpu import MX4_OVER_ROW

pytestmark = pytest.mark.gpu
#: worst |y − y64| / (K·2^-24·T + 2^-24·|y64|) measured over test_real_layers_inside_the_bound (the bound itself keeps the constant 1)
WORST_FRACTION_MEASURED = 0.002485         # conv3x3_b2_c32_9x9_s1_n24, outlier recipe


def unpacked(got, C):
    from dgq_amd.quant.quant_layer import mx4_unpack
    codes, scale = (t.cpu() for t in got)
    assert codes.dtype == torch.uint8 and codes.shape[1:] == (C // 32, 16)
    return mx4_unpack(codes), scale


def check_quantiser(got, rows, lds, what):
    """code and scale bytes of a dgq_quant_act_mx4 launch against mx4_pack(mx4_block(rows)), torch.equal"""
    from dgq_amd.quant.quant_layer import mx4_block, mx4_pack
    R, C = rows.shape
    want_c, want_s, xhat = mx4_block(rows)
    scale = got[1].cpu()
    assert scale.shape == (R, lds) and torch.equal(scale[:, :C // 32], want_s), "%s: scale bytes differ" % what
    assert lds == C // 32 or bool((scale[:, C // 32:] == 127).all()), "%s: the padding entries must read 127" % what
    bad = got[0].cpu() != mx4_pack(want_c)
    assert not bool(bad.any()), "%s: %d code bytes differ, first at %s" % (what, int(bad.sum()), bad.nonzero()[0].tolist())
    return xhat


# ----------------------------------------------------------------------------------------------- 1. the quantiser, bit exact
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=gs.ids_dtype)
@pytest.mark.parametrize("M,K", [(154, 768), (37, 320)])
def test_quantiser_linear_bit_exact(M, K, dtype, dev):
    from dgq_amd import ops
    from dgq_amd.plan import round_up, KTILE
    x = rta.special_rows(torch.randn(M, K, generator=torch.Generator().manual_seed(M * 1000 + K)) * 1.3 + 0.2)
    x[7, 40] = 1e4
    x[6, 32:64] = 0.0
    x = x.to(dtype)
    lds = round_up(K, KTILE) // 32                            # (37, 320): Kp = 384, two padding entries
    got = ops.quant_act_mx4(x.to(dev), (M, 1, 1, K, 1, 1, 1, 0), lds=lds)
    check_quantiser(got, x.float(), lds, "linear %dx%d %s" % (M, K, dtype))


def test_quantiser_conv_input_per_pixel_bit_exact(dev):
    from dgq_amd import ops
    B, C, H, W = 2, 32, 9, 9
    x = rta.special_image(torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(C + H)) * 1.3 + 0.2)
    xs = x.to(dev).contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
    check_quantiser(ops.quant_act_mx4(xs, (B, H, W, C, 3, 3, 1, 1)), rb.pixel_rows(x), C // 32, "conv input")


def test_quantiser_edge_blocks_and_standalone_forward(dev):
    """zeros, the planted ties at three scales, saturation, −0, subnormal and largest-finite amax; dgq_dequant_act_mx4 and the
    stand-alone UniformAffineQuantizer.forward give x̂ bit for bit (16-bit outputs: x̂ rounded once)"""
    from dgq_amd import ops
    from dgq_amd.quant.quant_layer import UniformAffineQuantizer
    rows = mx.edge_blocks()
    R, C = rows.shape
    got = ops.quant_act_mx4(rows.to(dev), (R, 1, 1, C, 1, 1, 1, 0))
    xhat = check_quantiser(got, rows, C // 32, "edge blocks")
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        assert torch.equal(ops.dequant_act_mx4(got[0], got[1], torch.empty(R, C, device=dev, dtype=dt)).cpu(), xhat.to(dt))
    q = UniformAffineQuantizer(bits=4, real_time=True, real_time_block=32, real_time_format="mxfp4")
    assert torch.equal(q(rows.view(1, R, C).to(dev)).cpu(), xhat.view(1, R, C))


@pytest.mark.parametrize("fold", ["gn_silu", "ln", "geglu"])
def test_quantiser_folded_prologue(fold, dev):
    """SiLU, erf and the LayerNorm statistics are the device's own approximations, so x′ is the CPU's only to within tol: as for MXFP6
    the exact check that remains is an interval — the statement is monotone in x′ under a fixed E.  Blocks whose amax is within tol of a
    power of two may carry either E and are few; elsewhere the E is the statement's and every value lies between the statement's on
    x′ − tol and x′ + tol.  (GroupNorm without activation is exact and bit for bit: the first branch checks it on the way.)"""
    from dgq_amd import ops
    g = torch.Generator().manual_seed(31)
    M, K = 77, 320
    if fold == "gn_silu":
        B, C, H, W = 2, 64, 8, 8
        x = torch.randn(B, C, H, W, generator=g) * 1.3 + 0.2
        xs = x.to(dev).contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
        sc, sh = ops.groupnorm_scale_shift(xs, B, H * W, C, 32, 1e-5, (1 + 0.1 * torch.randn(C, generator=g)).to(dev), (0.1 * torch.randn(C, generator=g)).to(dev))
        pre = x * sc.cpu()[:, :, None, None] + sh.cpu()[:, :, None, None]          # (exact: the launch's own scale / shift)
        check_quantiser(ops.quant_act_mx4(xs, (B, H, W, C, 3, 3, 1, 1), pre=(sc, sh, 0)), rb.pixel_rows(pre), C // 32, "GroupNorm")
        got = ops.quant_act_mx4(xs, (B, H, W, C, 3, 3, 1, 1), pre=(sc, sh, 1))
        rows = rb.pixel_rows(F.silu(pre))
        tol = 4e-6 * rows.abs() + 1e-7
    elif fold == "ln":
        x = torch.randn(M, K, generator=g) * 1.3 + 0.2
        gam, bet = 1 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
        got = ops.quant_act_mx4(x.to(dev), (M, 1, 1, K, 1, 1, 1, 0), ln=(gam.to(dev), bet.to(dev), 1e-5))
        rows = F.layer_norm(x.double(), (K,), gam.double(), bet.double(), 1e-5).float()
        tol = (2.0 ** -20 * (x.abs().amax(dim=1, keepdim=True) + 1.0)).expand_as(rows).contiguous()
    else:
        x = torch.randn(M, 2 * K, generator=g) * 1.3 + 0.2
        got = ops.quant_act_mx4(x.to(dev), (M, 1, 1, K, 1, 1, 1, 0), pre=(None, None, 2))
        rows = (x[:, :K].double() * F.gelu(x[:, K:].double())).float()
        tol = 4e-6 * rows.abs() + 1e-6 * x[:, :K].abs()
    codes, scale = unpacked(got, rows.shape[1])
    x_lo, x_hi = mx.mx4_reference(rows - tol)[2], mx.mx4_reference(rows + tol)[2]
    am_lo, am_hi = mx.mx4_reference(torch.clamp(rows.abs() - tol, min=0.0))[1], mx.mx4_reference(rows.abs() + tol)[1]
    firm = am_lo == am_hi
    assert float(firm.float().mean()) > 0.98 and torch.equal(scale[firm], am_hi[firm])
    assert bool(((scale == am_lo) | (scale == am_hi)).all())
    got_x, fe = mx.decode(codes, scale), firm.repeat_interleave(32, dim=1)
    assert bool(((got_x >= torch.minimum(x_lo, x_hi)) & (got_x <= torch.maximum(x_lo, x_hi)))[fe].all()), fold
    assert float((got_x == mx.mx4_reference(rows)[2])[fe].float().mean()) > 0.995


# ----------------------------------------------------------------------------------------------- 2. operand maps
def _handmade(dev, codes, E, lds):
    """(codes, scale) on the device as dgq_quant_act_mx4 writes them, from 4-bit codes [M][K] and exponents E [M][K/32]"""
    from dgq_amd.quant.quant_layer import mx4_pack
    scale = torch.full((codes.shape[0], lds), 127, dtype=torch.uint8)
    scale[:, :E.shape[1]] = (E + 127).to(torch.uint8)
    return mx4_pack(codes.to(torch.uint8)).contiguous().to(dev), scale.to(dev)


def _distinct_E(M, nb, seed):
    E = torch.randint(-6, 7, (M, nb), generator=torch.Generator().manual_seed(seed))
    E[:, 1:] = torch.where(E[:, 1:] == E[:, :-1], E[:, 1:] + 1, E[:, 1:])     # neighbouring blocks differ: a swapped lane half fails
    return E


def _equal(y, want):
    got = y.cpu().double()
    bad = got != want
    assert not bool(bad.any()), "%d of %d elements differ, first at %s: got %r, want %r" % (
        int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist(), float(got[bad][0]), float(want[bad][0]))


@pytest.mark.parametrize("M,K,N", [(64, 64, 64), (37, 320, 24)])
def test_operand_map_one_hot_activations(M, K, N, dev):
    """row m holds the FP4 code of 1.0 at ONE k_m (distinct per row; odd and even k: both nibbles), every (row, block) its own E:
    y[m, n] = δw[n]·(q − z)[n, k_m]·2^E[m, k_m / 32] — a gather, bit for bit.  A wrong nibble or lane map reads another k or n, the formats
    swapped between the operands another value, a wrong scale byte another block's E."""
    from dgq_amd import ops
    qw, zw, wd = t6._asym_weight(N, K)
    ab = ops.MxActBinding(t6._packed_weight(ops, dev, qw, zw, wd), "mxfp4")
    km = (torch.arange(M) * 7 + 3) % K
    codes = torch.zeros(M, K, dtype=torch.int64)
    codes[torch.arange(M), km] = 2                                        # 1.0 in E2M1
    E = _distinct_E(M, K // 32, M + K)
    y = ops.gemm_mx4(_handmade(dev, codes, E, ab.Kp // 32), (M, 1, 1, K, 1, 1, 1, 0), ab, torch.float32)
    _equal(y, wd[None, :].double() * (qw.double() - zw[:, None].double())[:, km].t() * (2.0 ** E[torch.arange(M), km // 32].double())[:, None])


@pytest.mark.parametrize("M,K,N", [(64, 64, 64), (37, 320, 24)])
def test_operand_map_one_hot_weights(M, K, N, dev):
    """the transpose: column n holds q − z = 2 (the E2M3 value 1.0 under the constant scale 2^1) at ONE k_n, the activations every FP4
    code asymmetric in (m, k) with their own E per (row, block): y[m, n] = δw[n]·2·x̂[m, k_n], bit for bit"""
    from dgq_amd import ops
    kn = (torch.arange(N) * 5 + 1) % K
    zw = (1 + (5 * torch.arange(N)) % 13).float()
    qw = zw.long()[:, None].repeat(1, K)
    qw[torch.arange(N), kn] += 2
    wd = (2.0 ** ((torch.arange(N) % 3) - 1).double()).float()
    ab = ops.MxActBinding(t6._packed_weight(ops, dev, qw, zw, wd), "mxfp4")
    m, k = torch.arange(M)[:, None], torch.arange(K)[None, :]
    codes = (7 * m + 11 * k + (m * k) % 5) % 16
    E = _distinct_E(M, K // 32, N + K)
    y = ops.gemm_mx4(_handmade(dev, codes, E, ab.Kp // 32), (M, 1, 1, K, 1, 1, 1, 0), ab, torch.float32)
    _equal(y, 2.0 * wd[None, :].double() * mx.decode(codes.to(torch.uint8), (E + 127).to(torch.uint8))[:, kn])


# ----------------------------------------------------------------------------------------------- 3. exact layers, un-split and split
EXACT_CASES = [lr.linear_case(37, 320, 24), lr.conv_case(2, 32, 9, 9, 1, 24), lr.conv_case(2, 64, 11, 13, 2, 64),
               lr.conv_case(2, 64, 8, 8, 1, 64, upsample=True), lr.conv_case(2, 64, 7, 9, 1, 64, k=1)]
SPLIT_CASE = lr.conv_case(2, 64, 8, 8, 1, 64)             # 18 chunks = 3 K tiles


def _exact_layer(ops, case, dev):
    d = mx.planted_mx4(case)
    y64 = mx.layer_float64(case, d["x"].double(), d["qw"], d["wzp"], d["wdelta"], d["bias"])
    assert t6.mx.mx6_exact_margin(case, d["x"].double(), d["qw"], d["wzp"], d["wdelta"], d["bias"], d["residual"]) < 1.0
    K, taps = lr.geometry(case)[6:8]
    pw = ops.PackedWeight(d["w"].to(dev), d["wdelta"].to(dev), d["wzp"].to(dev), None, d["bias"].to(dev), 4, K // taps, taps)
    assert torch.equal(pw.codes.cpu().long(), d["qw"]) and pw.mx6_eligible
    return d, y64, ops.MxActBinding(pw, "mxfp4")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=gs.ids_dtype)
@pytest.mark.parametrize("case", EXACT_CASES, ids=lambda c: c["name"])
def test_exact_layers_equal_the_reference(case, dtype, dev, monkeypatch):
    """every product and partial sum is an fp32 number: y EQUALS the float64 layer (fp32: with the residual; bf16: rounded once)"""
    from dgq_amd import ops
    d, y64, ab = _exact_layer(ops, case, dev)
    res = d["residual"] if dtype == torch.float32 else None
    spy = gs.spied(ops, monkeypatch)
    y = routes.run_layer(ops, case, ab, d["x"].to(dev, dtype), res.to(dev) if res is not None else None)
    names = [c["name"] for c in spy.take()]
    assert names.count("dgq_quant_act_mx4") == 1 and names.count("dgq_gemm_mx4") == 1 and "dgq_gemm_blockq" not in names, names
    want = (y64 if res is None else y64 + res.double()).float().to(dtype)
    assert y.dtype == dtype and torch.equal(y.cpu(), want), (y.cpu() != want).nonzero()[:4].tolist()


def test_exact_linear_geglu_epilogue(dev):
    """packed rows (value, gate) interleaved: the projection is exact, the erf of kernel and host differ in their last bits (1e-6, as
    the family's GEGLU tests)"""
    from dgq_amd import ops
    d, y64, ab = _exact_layer(ops, EXACT_CASES[0], dev)
    y = ops.quant_linear(d["x"].to(dev), ab, geglu=True)
    assert tuple(y.shape) == (1, 37, 12) and rel_l2(y.cpu(), y64[..., 0::2] * F.gelu(y64[..., 1::2])) < 1e-6


@pytest.mark.parametrize("S", [2, 3])
def test_split_equals_unsplit(S, dev, monkeypatch):
    """forced splits of 3 K tiles (S = 2: a ragged last split) on the exact data: dgq_gemm_mx4_splitk + the family's combine give the
    un-split bits, which are the float64 layer's"""
    from dgq_amd import ops
    d, y64, ab = _exact_layer(ops, SPLIT_CASE, dev)
    y1 = routes.run_layer(ops, SPLIT_CASE, ab, d["x"].to(dev), None)
    spy = gs.spied(ops, monkeypatch)
    monkeypatch.setattr(ops, "MX_KSPLIT", S)
    yS = routes.run_layer(ops, SPLIT_CASE, ab, d["x"].to(dev), None)
    names = [c["name"] for c in spy.take()]
    assert names.count("dgq_gemm_mx4_splitk") == 1 and "dgq_gemm_mx4" not in names, names
    assert torch.equal(yS, y1) and torch.equal(y1.cpu().double(), y64)


def test_plan_splits_the_long_k_convolution():
    from dgq_amd import _lib, ops
    assert _lib.load().dgq_gemm_mx_plan_splits(2 * 8 * 8, 1280, 2560 * 9, ops.WORKSPACE_BYTES) > 1      # conv 2x2560x8x8 -> 1280


# ----------------------------------------------------------------------------------------------- 4. real-valued layers
@pytest.mark.parametrize("data", ["randn", "outlier"])
@pytest.mark.parametrize("name", ["linear_m154_k768_n320", "conv3x3_b2_c32_9x9_s1_n24"])
def test_real_layers_inside_the_bound(name, data, dev, capsys):
    """per element |y − y64| <= K·2^-24·T + 2^-24·|y64|: the a-priori ceiling of an fp32 sum of K exact terms (constant 1) plus the one
    rounding of the result; T = |bias| + δw·Σ|x̂·(q − z)|, y64 the float64 layer over the KERNEL's own codes and scales"""
    from dgq_amd import ops
    case = lr.CASES_BY_NAME[name]
    d = lr.real_case(case, "perM", 4, 4)
    x = d["x"]
    if data == "outlier":
        x = mx.rows_to_input(case, mx.outlier_rows(mx.input_rows(case, x)), x).contiguous()
    B, H, W, Ho, Wo, M, K, taps = lr.geometry(case)
    C, lin = K // taps, case["kind"] == "linear"
    pw = ops.PackedWeight(d["w_raw"].to(dev), d["wdelta"].to(dev), d["wzp"].to(dev), None, d["bias"].to(dev), 4, C, taps)
    y = routes.run_layer(ops, case, ops.MxActBinding(pw, "mxfp4"), x.to(dev), None).cpu().double()
    xs = x.to(dev).reshape(-1, C) if lin else x.to(dev).contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
    got = ops.quant_act_mx4(xs, (M, 1, 1, C, 1, 1, 1, 0) if lin else (B, H, W, C, case["k"], case["k"], case["stride"], case["pad"]))
    xhat = mx.rows_to_input(case, mx.decode(*unpacked(got, C)), x)
    qw, zw, wd = pw.codes.cpu().long(), pw.zp_true.cpu(), pw.alpha.cpu()
    y64 = mx.layer_float64(case, xhat, qw, zw, wd, d["bias"])
    bound = K * 2.0 ** -24 * mx.term_magnitudes(case, xhat, qw, zw, wd, d["bias"]) + 2.0 ** -24 * y64.abs()
    with capsys.disabled():
        print("\nREAL-TIME MXFP4 %s %s: worst |y - y64| / bound = %.4g" % (name, data, float(((y - y64).abs() / bound).max())))
    assert bool(((y - y64).abs() <= bound).all())


# ----------------------------------------------------------------------------------------------- 5. routing and the public interface
def _quant_layer(dev, lin, wbits, **aq_extra):
    from dgq_amd.quant import QuantLayer, Scaler
    aq = {"bits": 4, "channel_wise": False, "scaler": Scaler.MINMAX, "leaf_param": True, "real_time": True, **aq_extra}
    layer = QuantLayer(lin, {"bits": wbits, "channel_wise": True, "scaler": Scaler.MINMAX}, aq).to(dev)
    layer.set_quant_state(True, True)
    return layer


def test_quant_layer_routes_and_beats_the_row_mode(dev, capsys):
    """a W4 QuantLayer with the format set takes the MX binding; on the outlier data its error against the float64 product with
    unquantised activations is at most the int4 row mode's times the ratio of the CPU statements, with 1.25x for the summation order"""
    from dgq_amd import ops
    c = rb.outlier_case(64, 768, 320, 4)
    errs = {}
    for fmt, extra in (("row", {}), ("mxfp4", dict(real_time_block=32, real_time_format="mxfp4"))):
        lin = torch.nn.Linear(768, 320, bias=False)
        lin.weight.data.copy_(c["w_raw"])
        layer = _quant_layer(dev, lin, 4, **extra)
        with torch.no_grad():
            y = layer(c["x"].to(dev))
        ab = layer._bindings["real_time"]
        assert isinstance(ab, ops.MxActBinding) and ab.fmt == "mxfp4" if fmt == "mxfp4" else isinstance(ab, ops.DynamicActBinding)
        errs[fmt] = rel_l2(y.cpu(), c["x"].double() @ layer.dequantized_weight(torch.float32).double().cpu().t())
    with capsys.disabled():
        print("\nREAL-TIME MXFP4 outliers 64x768->320 A4: row %.4g mxfp4 %.4g (%.4f)" % (errs["row"], errs["mxfp4"], errs["mxfp4"] / errs["row"]))
    assert errs["mxfp4"] <= 1.25 * MX4_OVER_ROW * errs["row"], errs


@pytest.mark.parametrize("wbits,C", [(8, 64), (4, 48)], ids=["w8", "c48"])
def test_ineligible_layers_run_as_the_int_block_mode(wbits, C, dev):
    """a W8 layer (the int block GEMM at 4 activation bits) and a C = 48 layer (no whole blocks: the row form) are, bit for bit, what
    real_time_block=32 alone computes"""
    from dgq_amd import ops
    g = torch.Generator().manual_seed(C)
    w, x = torch.randn(24, C, generator=g) * C ** -0.5, (torch.randn(1, 40, C, generator=g) * 1.3 + 0.2).to(dev)
    ys = []
    for extra in (dict(real_time_block=32, real_time_format="mxfp4"), dict(real_time_block=32)):
        lin = torch.nn.Linear(C, 24, bias=False)
        lin.weight.data.copy_(w)
        layer = _quant_layer(dev, lin, wbits, **extra)
        with torch.no_grad():
            ys.append(layer(x))
        ab = layer._bindings["real_time"]
        assert isinstance(ab, ops.BlockActBinding if C % 32 == 0 else ops.DynamicActBinding) and not ab.mx and ab.abits == 4
    assert torch.isfinite(ys[0]).all() and torch.equal(ys[0], ys[1])


def test_bad_arguments_are_refused(dev, monkeypatch):
    from dgq_amd import ops
    qw, zw, wd = t6._asym_weight(24, 64)
    ab = ops.MxActBinding(t6._packed_weight(ops, dev, qw, zw, wd), "mxfp4")
    geom = (8, 1, 1, 64, 1, 1, 1, 0)
    q = ops.quant_act_mx4(torch.randn(8, 64, device=dev), geom, lds=ab.Kp // 32)
    ex = ops._lib.GemmExtra()
    ex.res_div, ex.act = 1, 256                                            # (a non-null pointer value: refused before anything reads it)
    with pytest.raises(RuntimeError, match=r"dgq_quant_act_mx4 failed \(-1\)"):       # C % 32
        ops.quant_act_mx4(torch.randn(8, 48, device=dev), (8, 1, 1, 48, 1, 1, 1, 0))
    with pytest.raises(RuntimeError, match=r"dgq_gemm_mx4 failed \(-1\)"):            # a quantise-on-load descriptor
        ops.gemm_mx4(q, geom, ab, torch.float32, extra=ex)
    full = ops.workspace(dev)
    monkeypatch.setattr(ops, "workspace", lambda device: full[8:])                    # 8 bytes off a 16-byte boundary
    with pytest.raises(RuntimeError, match=r"dgq_gemm_mx4_splitk failed \(-1\)"):
        ops.gemm_mx4(q, geom, ab, torch.float32, ksplit=2)
    with pytest.raises(AssertionError):                                               # W8 planes under FP4 activations: out of scope
        ops.MxActBinding(ab.pw, "mxfp4", w_bits=8)


def _build_qnn(path, dev):
    import types
    from dgq_amd import synth
    from dgq_amd.diffusers_rewrite import UNet2DConditionModel
    from dgq_amd.quant import get_qmodel, Scaler
    from dgq_amd.runtime import quant_params
    unet = UNet2DConditionModel("tiny")
    unet.load_state_dict(synth.state_dict_from_ckpt(path))
    wq, aq, sm = quant_params(Scaler, 4, 4, True, True, True, True)
    aq["real_time"], aq["real_time_block"], aq["real_time_format"] = True, 32, "mxfp4"
    qnn = get_qmodel("tiny", types.SimpleNamespace(unet=unet), path, wq, True, aq, sm, False, 25, False, device=dev).float().to(dev)
    qnn.disable_out_quantization()
    return qnn


def test_model_eager_and_graph_replay(tmp_path, rt_inputs, dev):
    """arch ``tiny`` from a weight-only W4A4 checkpoint: every quantised layer takes the MXFP4 binding on the shared MXFP6 weight image,
    and the replays of a captured step equal the eager one"""
    from dgq_amd import ops, synth
    path = str(tmp_path / "wonly.pth")
    synth.write_cali_ckpt(path, "tiny", 4, 4, 1, num_slots=1, seed=0, batch=2, res=16, start_peak=True, with_act=False)
    qnn = _build_qnn(path, dev)
    x, ctx = rt_inputs
    with torch.no_grad():
        y_e = qnn(x, torch.tensor(999), ctx)[0].clone()
        qnn.enable_graphs(True)
        replays = [qnn(x, torch.tensor(999), ctx)[0].clone() for _ in range(3)]
        qnn.enable_graphs(False)
    assert torch.isfinite(y_e).all() and all(torch.equal(y, y_e) for y in replays), "graph replay differs from the eager run"
    for name, layer in rta._inner_layers(qnn).items():
        ab = layer._bindings["real_time"]
        assert isinstance(ab, ops.MxActBinding) and ab.fmt == "mxfp4" and ab.wpacked is layer._pw._mx6[0], name


def test_cli_aq_real_time_format(tmp_path):
    from dgq_amd import inference_qmodel as cli
    out = str(tmp_path / "lat_{rank}.pt")
    args = ["--model_type", "tiny", "--use_aq", "--aq_real_time", "--aq_real_time_block", "32", "--aq_real_time_format", "mxfp4",
            "--t2i_log_quant", "--t2i_real_time", "--num_inference_steps", "2", "--out", out]
    cli.main(args + ["--aq", "4"])
    d = torch.load(out.format(rank=0))
    assert sorted(d) == [0, 1] and all(torch.isfinite(v).all() for v in d.values())
    with pytest.raises(SystemExit) as e:
        cli.main(args)                                                      # without --aq 4
    assert "mxfp4" in str(e.value)
