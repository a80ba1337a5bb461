"""Real-time activation quantisation per row and 32-channel block (UniformAffineQuantizer(real_time=True, real_time_block=32):
dgq_quant_act_block + dgq_gemm_blockq) — a mode of this library.

The statement the quantiser must reproduce BIT FOR BIT is ``quant_layer.block_minmax`` (== the scalar ``minmax`` of every block,
tests/test_realtime_block_cpu.py) followed by the reference's fp32 divide / round / clamp; the layer is checked against
tests/layer_reference.py under those tables expanded to one (δ, z) per element (tests/realtime_block_ref.py): exact-integer layers
EQUAL the float64 formula, real-valued layers stay within the project's bounds (2e-5 without a prologue, 2e-3 with one)."""
import pytest
import torch
import torch.nn.functional as F

from tests import layer_reference as lr
from tests import realtime_block_ref as rb
from tests import test_gpu_layer_routes as routes
from tests import test_gpu_realtime_act as rta
from tests.test_gpu_realtime_act import rt_ckpts, rt_inputs, rel_l2          # noqa: F401  (module-scoped fixtures of the row mode)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from dgq_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def special_blocks(x2d):
    """``special_rows`` (whole rows all-positive / all-negative / all-zero / with a 1e4 outlier) and the same per BLOCK: block 1 of rows
    4 .. 7 all-positive, all-negative, all-zero, carrying a 1e4 outlier"""
    x2d = rta.special_rows(x2d)
    x2d[4, 32:64] = x2d[4, 32:64].abs() + 0.1
    x2d[5, 32:64] = -x2d[5, 32:64].abs() - 0.1
    x2d[6, 32:64] = 0.0
    x2d[7, 40] = 1e4
    return x2d


def check_quantiser(got, rows, bits, ldt, what):
    """codes, {δ, β} table and ρ of a dgq_quant_act_block launch against the CPU statement on ``rows`` [R][C] (fp32 values)"""
    codes, table, rho = (t.cpu() for t in got)
    R, C = rows.shape
    nb = C // 32
    d, z = rb.block_tables(rows, bits)
    assert table.shape == (R, ldt, 2) and codes.shape == (R, C) and rho.shape == (R,)
    assert torch.equal(table[:, :nb, 0], d), "%s: δ differs at %s" % (what, (table[:, :nb, 0] != d).nonzero()[:4].tolist())
    assert torch.equal(table[:, :nb, 1], rb.beta_of(d, z, bits)), "%s: β differs at %s" % (what, (table[:, :nb, 1] != rb.beta_of(d, z, bits)).nonzero()[:4].tolist())
    assert float(table[:, nb:].abs().max()) == 0.0 if ldt > nb else True, "%s: the padding chunks must read δ = β = 0" % what
    s = rb.block_codes(rows, d, z, bits) - 2 ** (bits - 1)
    bad = codes.float() != s
    assert not bool(bad.any()), "%s: %d codes differ, first at %s" % (what, int(bad.sum()), bad.nonzero()[0].tolist())
    # ρ: the documented chain (ascending blocks, one fp32 product and one fp32 addition each) bit for bit; and within 1e-6 of the float64
    # sum — relative to the magnitude of the summed terms Σ|δ·rs|, the quantity a relative bound on a sum that may cancel refers to
    assert torch.equal(rho, rb.rho_chain(s, d)), "%s: ρ is not the ascending fp32 chain" % what
    r64, mag = rb.rho_float64(s, d)
    assert bool(((rho.double() - r64).abs() <= 1e-6 * mag).all()), "%s: ρ off by %.3g of Σ|δ·rs|" % (what, float(((rho.double() - r64).abs() / mag.clamp_min(1e-30)).max()))
    return d, z


# ----------------------------------------------------------------------------------------------- 1. tables and codes, bit exact
@pytest.mark.parametrize("bits", [8, 6])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=lambda d: str(d).replace("torch.", ""))
@pytest.mark.parametrize("M,K", [(154, 768), (37, 320)])
def test_quantiser_linear_bit_exact(M, K, dtype, bits, dev):
    from dgq_amd import ops
    from dgq_amd.plan import round_up, KTILE
    g = torch.Generator().manual_seed(M * 1000 + K + bits)
    x = special_blocks(torch.randn(M, K, generator=g) * 1.3 + 0.2).to(dtype)
    ldt = round_up(K, KTILE) // 32
    assert ldt == (24 if K == 768 else 12)                # (37, 320): Kp = 384, two padding chunks
    got = ops.quant_act_block(x.to(dev), (M, 1, 1, K, 1, 1, 1, 0), bits, ldt=ldt)
    torch.cuda.synchronize()
    d, z = check_quantiser(got, x.float(), bits, ldt, "linear %dx%d %s a%d" % (M, K, dtype, bits))
    assert float(d[2].max()) == rb.TINY and float(z[2].abs().max()) == 0.0 and float(d[6, 1]) == rb.TINY      # all-zero row / block


@pytest.mark.parametrize("bits", [8, 6])
@pytest.mark.parametrize("B,C,H,W", [(2, 32, 9, 9), (2, 64, 11, 13)])
def test_quantiser_conv_input_per_pixel_bit_exact(B, C, H, W, bits, dev):
    from dgq_amd import ops
    g = torch.Generator().manual_seed(C + H + bits)
    x = rta.special_image(torch.randn(B, C, H, W, generator=g) * 1.3 + 0.2)
    xs = x.to(dev).contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
    got = ops.quant_act_block(xs, (B, H, W, C, 3, 3, 1, 1), bits)
    torch.cuda.synchronize()
    d, _ = check_quantiser(got, rb.pixel_rows(x), bits, C // 32, "conv input %dx%dx%dx%d a%d" % (B, C, H, W, bits))
    assert int((d == rb.TINY).sum()) > 0, "no all-zero pixel block in the case"


# ----------------------------------------------------------------------------------------------- 2. exact-integer layers
EXACT_CASES = [
    (lr.linear_case(154, 768, 320), 8, 4), (lr.linear_case(154, 768, 320), 6, 4), (lr.linear_case(154, 768, 320), 8, 8),
    (lr.linear_case(2048, 320, 320), 8, 4),
    (lr.linear_case(37, 320, 24), 8, 4),                                  # ragged N, Kp = 384
    (lr.conv_case(2, 32, 9, 9, 1, 24), 8, 4),
    (lr.conv_case(2, 64, 11, 13, 2, 64), 8, 4),
    (lr.conv_case(2, 64, 8, 8, 1, 64, upsample=True), 8, 4),
    (lr.conv_case(2, 64, 7, 9, 1, 64, k=1), 8, 4),
]


def _exact_layer(ops, case, abits, wbits, dev):
    d = rb.planted_exact(case, abits, wbits)
    y_ref, q, de, ze, inside = rb.block_reference(case, d)
    margin = rb.block_exact_margin(case, d, q, de, ze, inside)
    assert margin < 1.0, "%s: the term magnitudes reach %.3f x 2^24 units — narrow the ranges" % (case["name"], margin)
    B, H, W, Ho, Wo, M, K, taps = lr.geometry(case)
    pw = ops.PackedWeight(d["w"].to(dev), d["wdelta"].to(dev), d["wzp"].to(dev), None, d["bias"].to(dev), wbits, K // taps, taps)
    assert torch.equal(pw.codes.cpu().long(), d["qw"])
    return d, y_ref, ops.BlockActBinding(pw, abits)


@pytest.mark.parametrize("case,abits,wbits", EXACT_CASES, ids=lambda v: v["name"] if isinstance(v, dict) else str(v))
def test_exact_layers_equal_the_formula(case, abits, wbits, dev, monkeypatch):
    from dgq_amd import _lib, ops
    d, y_ref, ab = _exact_layer(ops, case, abits, wbits, dev)
    spy = routes.Spy(ops, _lib)
    monkeypatch.setattr(ops, "_lib_call", spy)
    y = routes.run_layer(ops, case, ab, d["x"].to(dev), d["residual"].to(dev))
    torch.cuda.synchronize()
    names = [c["name"] for c in spy.take()]
    assert names.count("dgq_quant_act_block") == 1 and names.count("dgq_gemm_blockq") == 1, names
    assert not any(n.startswith("dgq_act_row_params") or n == "dgq_quant_act_batch" or n.startswith("dgq_gemm_wxa8") for n in names), names
    got = y.cpu().double()
    if not torch.equal(got, y_ref):
        bad = got != y_ref
        idx = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s a%dw%d: y differs from the formula on %d of %d elements, first at %s: got %r, want %r"
                             % (case["name"], abits, wbits, int(bad.sum()), bad.numel(), idx, float(got[idx]), float(y_ref[idx])))


# ----------------------------------------------------------------------------------------------- 3. real-valued layers
def _real_layer(ops, case, d, dev):
    B, H, W, Ho, Wo, M, K, taps = lr.geometry(case)
    pw = ops.PackedWeight(d["w_raw"].to(dev), d["wdelta"].to(dev), d["wzp"].to(dev), None, d["bias"].to(dev), d["wbits"], K // taps, taps)
    return ops.BlockActBinding(pw, d["abits"])


@pytest.mark.parametrize("name", ["conv3x3_b2_c32_9x9_s1_n24", "linear_m154_k768_n320", "linear_m2048_k640_n640"])
def test_real_layers_vs_reference(name, dev, capsys):
    """no prologue: the codes are the reference's under the same tables, only the fp32 order of the sums remains — 2e-5 (F3)"""
    from dgq_amd import ops
    case = lr.CASES_BY_NAME[name]
    d = lr.real_case(case, "perM")
    y_ref = rb.block_reference(case, d)[0]
    y = routes.run_layer(ops, case, _real_layer(ops, case, d, dev), d["x"].to(dev), d["residual"].to(dev))
    torch.cuda.synchronize()
    err = rel_l2(y.cpu(), y_ref)
    with capsys.disabled():
        print("\nREAL-TIME BLOCK %s: rel-L2 vs float64 %.3g" % (name, err))
    assert err <= 2e-5, err


@pytest.mark.parametrize("fold,name", [("geglu", "linear_m2048_k1280_n320"), ("gn_silu", "conv3x3_b2_c64_64x64_s1_n64"), ("ln", "linear_m2048_k640_n640")])
def test_real_layers_folded_prologue(fold, name, dev, capsys):
    """GroupNorm + SiLU, LayerNorm and GEGLU folded into the quantiser's load, against the fp32 CPU prologue followed by the float64 formula
    under the CPU statement's block tables of that prologue'd input: < 2e-3, the bound of test_real_layer_folded_prologue for these shapes"""
    from dgq_amd import ops
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
    y_ref = rb.block_reference(case, d, x=x_in)[0]
    y = routes.run_layer(ops, case, _real_layer(ops, case, d, dev), x.to(dev), d["residual"].to(dev), **kw)
    torch.cuda.synchronize()
    err = rel_l2(y.cpu(), y_ref)
    with capsys.disabled():
        print("\nREAL-TIME BLOCK PROLOGUE %s %s: rel-L2 %.3g" % (fold, name, err))
    assert err < 2e-3, err


# ----------------------------------------------------------------------------------------------- 4. epilogues
@pytest.fixture(scope="module")
def epi(dev):
    from dgq_amd import ops
    case = lr.linear_case(154, 768, 320)
    d, y_ref, ab = _exact_layer(ops, case, 8, 4, dev)
    x = d["x"].to(dev)
    return dict(case=case, d=d, ab=ab, x=x, y0=ops.quant_linear(x, ab))


def test_epilogue_residual(epi, dev):
    from dgq_amd import ops
    res = epi["d"]["residual"].to(dev)
    assert torch.equal(ops.quant_linear(epi["x"], epi["ab"], residual=res), epi["y0"] + res)


def test_epilogue_geglu(epi, dev):
    """packed rows (value, gate) interleaved: column i of the GEGLU output is y[2i]·gelu(y[2i+1]).  The projection values are the plain
    call's bit for bit; the erf of the kernel and of the host differ in their last bits: 1e-6 rel-L2, the bound of
    test_gemm_geglu_epilogue_equals_projection_then_geglu for fp32"""
    from dgq_amd import ops
    y = ops.quant_linear(epi["x"], epi["ab"], geglu=True)
    y0 = epi["y0"].double()
    a, gt = y0[..., 0::2], y0[..., 1::2]
    want = a * (0.5 * gt * (1.0 + torch.erf(gt * 0.70710678118654752)))
    assert y.shape == want.shape
    assert rel_l2(y.cpu(), want.cpu()) < 1e-6


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=lambda d: str(d).replace("torch.", ""))
def test_epilogue_16bit_output(epi, dtype, dev):
    """the planted integers are 16-bit representable: the same codes and sums, the fp32 result rounded once"""
    from dgq_amd import ops
    x16 = epi["x"].to(dtype)
    assert torch.equal(x16.float(), epi["x"])
    y = ops.quant_linear(x16, epi["ab"])
    assert y.dtype == dtype and torch.equal(y, epi["y0"].to(dtype))


def test_epilogue_second_copy(epi, dev):
    from dgq_amd import ops
    ab, x = epi["ab"], epi["x"]
    M, K, N = 154, 768, 320
    geom = (M, 1, 1, K, 1, 1, 1, 0)
    buf = torch.zeros(M, N + 72, device=dev)
    q = ops.quant_act_block(x.view(M, K), geom, 8, ldt=ab.Kp // 32)
    y = ops.gemm_blockq(q, geom, ab, torch.float32, extra=ops.make_extra(y2=buf[:, 40:40 + N]))
    assert torch.equal(y, epi["y0"].view(M, N)) and torch.equal(buf[:, 40:40 + N], y)
    assert float(buf[:, :40].abs().max()) == 0.0 and float(buf[:, 40 + N:].abs().max()) == 0.0


# ----------------------------------------------------------------------------------------------- 5. row independence
@pytest.mark.parametrize("M,K,N", [(154, 768, 320), (2048, 320, 320)])
def test_rows_are_independent(M, K, N, dev):
    from dgq_amd import ops
    g = torch.Generator().manual_seed(M + N)
    x = (torch.randn(M, K, generator=g) * 1.3 + 0.2).to(dev)
    ab = ops.BlockActBinding(rta._packed(ops, dev, N, K, 1, 9), 8)
    perm = torch.randperm(M, generator=g).to(dev)
    y = ops.quant_linear(x, ab)
    yp = ops.quant_linear(x[perm].contiguous(), ab)
    assert torch.equal(yp, y[perm])


# ----------------------------------------------------------------------------------------------- 6. public API
def test_quant_layer_block_beats_row_on_outliers(dev, capsys):
    """a QuantLayer under the block quantiser against the same layer under the row quantiser, on the outlier data of the CPU test:
    at least 2x lower error against the float64 product with unquantised activations"""
    from dgq_amd.quant import QuantLayer, Scaler
    c = rb.outlier_case(64, 768, 320, 8)
    errs = {}
    for blk in (0, 32):
        lin = torch.nn.Linear(768, 320, bias=False)
        lin.weight.data.copy_(c["w_raw"])
        aq = {"bits": 8, "channel_wise": False, "scaler": Scaler.MINMAX, "leaf_param": True, "real_time": True, "real_time_block": blk}
        layer = QuantLayer(lin, {"bits": 4, "channel_wise": True, "scaler": Scaler.MINMAX}, aq).to(dev)
        layer.set_quant_state(True, True)
        with torch.no_grad():
            y = layer(c["x"].to(dev))
        y64 = c["x"].double() @ layer.dequantized_weight(torch.float32).double().cpu().t()
        errs[blk] = rel_l2(y.cpu(), y64)
    with capsys.disabled():
        print("\nREAL-TIME BLOCK outliers 64x768->320 A8: row %.3g block %.3g (%.2fx)" % (errs[0], errs[32], errs[0] / errs[32]))
    assert errs[32] <= 0.5 * errs[0], errs


def test_standalone_quantizer_forward(dev):
    from oracle import dgq_oracle as orc
    from dgq_amd.quant.quant_layer import UniformAffineQuantizer
    g = torch.Generator().manual_seed(4)
    x = special_blocks(torch.randn(2 * 37, 320, generator=g) * 1.3 + 0.2).view(2, 37, 320)
    q = UniformAffineQuantizer(bits=6, real_time=True, real_time_block=32)
    y = q(x.to(dev))
    d, z = rb.block_tables(x.view(-1, 320), 6)
    want = orc.uaq(x.view(-1, 320), d.repeat_interleave(32, dim=1), z.repeat_interleave(32, dim=1), 6).view(x.shape)
    assert torch.equal(y.cpu(), want)
    with pytest.raises(NotImplementedError):
        q(torch.zeros(1, 4, 8, 8, device=dev))


# ----------------------------------------------------------------------------------------------- 7. model level
def _build_qnn(path, dev, steps=25, time_aware=False):
    import types
    from dgq_amd import synth
    from dgq_amd.diffusers_rewrite import UNet2DConditionModel
    from dgq_amd.quant import get_qmodel, Scaler
    from dgq_amd.runtime import quant_params
    unet = UNet2DConditionModel("tiny")
    unet.load_state_dict(synth.state_dict_from_ckpt(path))
    wq, aq, sm = quant_params(Scaler, 4, 8, True, True, True, True)
    aq["real_time"], aq["real_time_block"] = True, 32
    qnn = get_qmodel("tiny", types.SimpleNamespace(unet=unet), path, wq, True, aq, sm, False, steps, time_aware, device=dev)
    qnn = qnn.float().to(dev)
    qnn.disable_out_quantization()
    return qnn


@pytest.fixture(scope="module")
def blk_qnn(rt_ckpts, dev):
    return _build_qnn(rt_ckpts[0], dev)


def _layer_reference(layer, x_in):
    """float64 output of one QuantLayer on the (prologue'd, CPU fp32) input x_in under the CPU statement's block tables (the per-row
    statement for a layer whose input channels are no multiple of 32)"""
    if layer.in_channels % 32 != 0:
        return rta._layer_reference(layer, x_in)
    w = layer.dequantized_weight(torch.float32).float().cpu().contiguous()
    b = layer.b.detach().float().cpu() if layer.b is not None else None
    bits = layer.aqtizer.bits
    if layer.is_conv:
        kh, kw, st, pd = layer._conv_geom()
        de, ze, _ = rb.expand_conv(*rb.block_tables(rb.pixel_rows(x_in), bits), tuple(x_in.shape), kh, st, pd)
        return lr.reference_layer(x_in, w, b, de, ze, bits, "conv", kh, st, pd)[0]
    K = x_in.shape[-1]
    x2 = x_in.reshape(1, -1, K)
    de, ze = rb.expand_linear(*rb.block_tables(x2[0], bits))
    return lr.reference_layer(x2, w, b, de, ze, bits, "linear")[0].reshape(*x_in.shape[:-1], -1)


def test_model_teacher_forced_vs_reference(blk_qnn, rt_inputs, capsys):
    """arch ``tiny`` from a WEIGHT-ONLY checkpoint with real_time_block=32, the fused graph: every quantised layer reports once through
    LAYER_TAP and is within 2e-5 (no prologue) / 2e-3 (folded prologue) of the float64 formula on its OWN tapped input under the CPU
    statement's block tables; the layer's output is replaced by that reference (teacher-forced)."""
    from dgq_amd import ops
    from dgq_amd.quant import quant_layer
    qnn = blk_qnn
    inner = rta._inner_layers(qnn)
    names = {id(m): n for n, m in inner.items()}
    mods = dict(qnn.model.named_modules())
    seen, errs = [], {False: [], True: []}

    def tap(layer, y, x=None, prologue=False, residual=None, bias_rows=None, fq=None, geglu=False):
        name = names[id(layer)]
        seen.append(name)
        assert fq is None
        x_in = x.detach().float().cpu()
        if prologue:
            x_in = rta._prologue_input(mods, name, x_in)
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
    n_block = sum(isinstance(m._bindings.get("real_time"), ops.BlockActBinding) for m in inner.values())
    assert n_block == sum(m.in_channels % 32 == 0 for m in inner.values()) and n_block > 100
    worst = {k: max(v) for k, v in errs.items() if v}
    with capsys.disabled():
        print("\nREAL-TIME BLOCK MODEL tiny: %d block layers; %d calls without a prologue, worst %.3g (%s); %d with one, worst %.3g (%s)"
              % (n_block, len(errs[False]), *worst[False], len(errs[True]), *worst[True]))
    assert worst[False][0] <= 2e-5, worst[False]
    assert worst[True][0] < 2e-3, worst[True]


def test_model_graph_replay_images_and_loader(blk_qnn, rt_ckpts, rt_inputs, dev):
    from dgq_amd import ops
    qnn = blk_qnn
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
    # exactly one natural-order image per layer (no fragment-major twin, no slots), after forwards at two timesteps
    inner = rta._inner_layers(qnn)
    for name, layer in inner.items():
        assert list(layer._bindings) == ["real_time"], name
        ab, pw = layer._bindings["real_time"], layer._pw
        assert isinstance(ab, ops.BlockActBinding if layer.in_channels % 32 == 0 else ops.DynamicActBinding), name
        assert ab.wpacked is pw._natural[0] and not layer._act_tables, name
        if ab.block:
            assert ab.wfrag is None and ab.vc is pw._vc and tuple(ab.vc.shape) == (pw.N, ab.Kp // 32), name
    imgs = {l._bindings["real_time"].wpacked.data_ptr() for l in inner.values()}
    assert len(imgs) == len(inner)
    # ... whatever num_inference_steps: a 50-step model from the checkpoint WITH act_* blocks holds as many images and computes the same
    qnn50 = _build_qnn(rt_ckpts[1], dev, steps=50)
    with torch.no_grad():
        y50 = qnn50(x, torch.tensor(999), ctx)[0]
        qnn50(x, torch.tensor(21), ctx)
    inner50 = rta._inner_layers(qnn50)
    assert all(list(l._bindings) == ["real_time"] for l in inner50.values()) and len(inner50) == len(inner)
    assert torch.equal(y50, y_e), "the act_* blocks of the checkpoint changed the result"
    with pytest.raises(ValueError):
        _build_qnn(rt_ckpts[0], dev, time_aware=True)


# ----------------------------------------------------------------------------------------------- 8. CLI
def test_cli_aq_real_time_block(tmp_path):
    from dgq_amd import inference_qmodel as cli
    out = str(tmp_path / "lat_{rank}.pt")
    cli.main(["--model_type", "tiny", "--use_aq", "--aq_real_time", "--aq_real_time_block", "32", "--t2i_log_quant", "--t2i_real_time",
              "--num_inference_steps", "2", "--out", out])
    d = torch.load(out.format(rank=0))
    assert sorted(d) == [0, 1] and all(torch.isfinite(v).all() for v in d.values())
    with pytest.raises(SystemExit) as e:
        cli.main(["--model_type", "tiny", "--use_aq", "--aq_real_time_block", "32", "--num_inference_steps", "2", "--out", out])
    assert "--aq_real_time" in str(e.value)
