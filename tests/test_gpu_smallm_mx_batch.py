"""ops.linear_smallm_mx_batch (dgq_linear_smallm_mx_batch) against float64 and against the two-launch route.  Bound: the MX GEMM tests',
|y − y64| <= K·2^-24·S + u_out·|y64|, S = |bias| + δw·Σ|x̂·(q − z)|; x̂ = the format's statement (quant_layer.py) of the fp32 input, and
behind SiLU (which the CPU reproduces to a few ulp only) the stand-alone quantiser's own x̂; test 3 ties the batch kernel's codes to it."""
import types
import pytest
import torch

from tests import test_gpu_realtime_act as rta
from tests import test_gpu_realtime_mxfp6 as t6
from tests.test_gpu_realtime_act import dev, rt_inputs, rel_l2          # noqa: F401  (module-scoped fixtures of the row mode)

gpu = pytest.mark.gpu
FORMATS = ["mxfp6", "mxint8", "mxfp4"]
U_OUT = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8}     # unit roundoff: 24 and 8 significand bits


def _two_launch(ops, fmt):
    s = {"mxfp6": "mx6", "mxint8": "mxint8", "mxfp4": "mx4"}[fmt]
    return getattr(ops, "quant_act_" + s), getattr(ops, "dequant_act_" + s), getattr(ops, "gemm_" + s)


def _xhat(ops, fmt, x, pre_act):
    """x̂ [M][K] float64 of x (on the device): the statement, or behind SiLU the stand-alone quantiser's"""
    from dgq_amd.quant import quant_layer
    M, K = x.shape
    if not pre_act:
        return {"mxfp6": quant_layer.mx6_block, "mxint8": quant_layer.mxint8_block, "mxfp4": quant_layer.mx4_block}[fmt](x.float().cpu())[2].double()
    quant, dequant, _ = _two_launch(ops, fmt)
    q = quant(x, (M, 1, 1, K, 1, 1, 1, 0), (None, None, 1))
    return dequant(q[0], q[1], torch.empty((M, K), dtype=torch.float32, device=x.device)).cpu().double()


def _layers(ops, dev, fmt, K, Ns):
    out = []
    for i, N in enumerate(Ns):
        qw, zw, wd = t6._asym_weight(N, K)
        bias = torch.randn(N, generator=torch.Generator().manual_seed(N + i))
        out.append((ops.MxActBinding(t6._packed_weight(ops, dev, qw, zw, wd, bias), fmt), (qw.double() - zw.double()[:, None]), wd.double(), bias.double()))
    return out


def _ratio(y, xhat, layer, K, dtype):
    _, d, wd, bias = layer
    y64 = bias + wd * (xhat @ d.t())
    S = bias.abs() + wd * (xhat.abs() @ d.abs().t())
    return float(((y.cpu().double() - y64).abs() / (K * 2.0 ** -24 * S + U_OUT[dtype] * y64.abs())).max())


@gpu
@pytest.mark.parametrize("pre_act", [0, 1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_against_float64(fmt, dtype, pre_act, dev, capsys):
    """K = 32: one block; 320: a partly padded last step; N = 24: one wave's ragged tiles; (16, 200, 1280): a slab table, a ragged slab"""
    from dgq_amd import ops
    worst = 0.0
    for K in (32, 320, 1280):
        sets = [_layers(ops, dev, fmt, K, (24,)), _layers(ops, dev, fmt, K, (16, 200, 1280))]
        for M in (1, 2, 16):
            x = (torch.randn(M, K, generator=torch.Generator().manual_seed(M + K)) * 1.5 + 0.1).to(dev, dtype)
            xhat = _xhat(ops, fmt, x, pre_act)
            for layers in sets:
                ys = ops.linear_smallm_mx_batch(x, [l[0] for l in layers], pre_act=pre_act)
                for y, layer in zip(ys, layers):
                    assert y.dtype == dtype and tuple(y.shape) == (M, layer[1].shape[0])
                    worst = max(worst, _ratio(y, xhat, layer, K, dtype))
    with capsys.disabled():
        print("\nSMALL-M MX BATCH %s %s pre_act=%d: worst |y - y64| / bound = %.4g" % (fmt, dtype, pre_act, worst))
    assert worst <= 1.0


@gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_exact_data_equals_float64_and_the_two_launch_route(fmt, dev):
    """x in {−2 .. 2} (exact in every format), integer q − z and bias, power-of-two δw: every partial sum is an integer below 2^24"""
    from dgq_amd import ops
    M, K, N = 2, 320, 200
    qw, zw, wd = t6._asym_weight(N, K)
    bias = ((torch.arange(N) % 9) - 4).float()
    ab = ops.MxActBinding(t6._packed_weight(ops, dev, qw, zw, wd, bias), fmt)
    m, k = torch.arange(M)[:, None], torch.arange(K)[None, :]
    x = (((3 * m + 7 * k + (m * k) % 3) % 5) - 2).float().to(dev)
    y = ops.linear_smallm_mx_batch(x, [ab])[0]
    y64 = bias.double() + wd.double() * (x.cpu().double() @ (qw.double() - zw.double()[:, None]).t())
    quant, _, gemm = _two_launch(ops, fmt)
    geom = (M, 1, 1, K, 1, 1, 1, 0)
    y2 = gemm(quant(x, geom, lds=ab.Kp // 32), geom, ab, torch.float32)
    assert torch.equal(y.cpu().double(), y64) and torch.equal(y, y2)


@gpu
@pytest.mark.parametrize("K", [32, 320])
@pytest.mark.parametrize("fmt", FORMATS)
def test_outlier_rows_agree_with_the_two_launch_route(fmt, K, dev):
    """a 1e3 element behind SiLU: inside the bound; K = 32 is one block, whose 32 exact products sum exactly in fp32: bit for bit"""
    from dgq_amd import ops
    M, layer = 2, _layers(ops, dev, fmt, K, (200,))[0]
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(K))
    x[1, 5] = 1e3
    x = x.to(dev)
    y = ops.linear_smallm_mx_batch(x, [layer[0]], pre_act=1)[0]
    quant, _, gemm = _two_launch(ops, fmt)
    geom = (M, 1, 1, K, 1, 1, 1, 0)
    y2 = gemm(quant(x, geom, (None, None, 1), lds=layer[0].Kp // 32), geom, layer[0], torch.float32)
    xhat = _xhat(ops, fmt, x, 1)
    assert _ratio(y, xhat, layer, K, torch.float32) <= 1.0 and _ratio(y2, xhat, layer, K, torch.float32) <= 1.0
    if K == 32:
        assert torch.equal(y, y2)


def _build_qnn(path, dev, fmt):
    from dgq_amd import ops, synth
    from dgq_amd.diffusers_rewrite import UNet2DConditionModel
    from dgq_amd.quant import get_qmodel, Scaler
    from dgq_amd.runtime import quant_params
    unet = UNet2DConditionModel("tiny")
    unet.load_state_dict(synth.state_dict_from_ckpt(path))
    wq, aq, sm = quant_params(Scaler, 4, ops.MX_FORMAT_BITS[fmt], True, True, True, True)
    aq["real_time"], aq["real_time_block"], aq["real_time_format"] = True, 32, fmt
    qnn = get_qmodel("tiny", types.SimpleNamespace(unet=unet), path, wq, True, aq, sm, False, 25, False, device=dev).float().to(dev)
    qnn.disable_out_quantization()
    return qnn


@gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_unet_routes_the_time_embedding_group(fmt, tmp_path, rt_inputs, dev):
    """arch ``tiny``: on = ONE small-M launch, inside the MX model tests' 2e-3 rel-L2 of off; a mixed group is routed as with it off"""
    from dgq_amd import ops, synth
    path = str(tmp_path / "wonly.pth")
    synth.write_cali_ckpt(path, "tiny", 4, ops.MX_FORMAT_BITS[fmt], 1, num_slots=1, seed=0, batch=2, res=16, start_peak=True, with_act=False)
    qnn = _build_qnn(path, dev, fmt)
    x, ctx = rt_inputs
    group = [m for n, m in rta._inner_layers(qnn).items() if n.endswith("time_emb_proj")]
    seen = []

    def run(on):
        ops.MX_SMALLM_BATCH = on
        with torch.no_grad():
            return qnn(x, torch.tensor(999), ctx)[0].clone()
    try:
        y_off = run(False)
        ops.BLOCK_LAUNCH_HOOK = lambda issue, kind, info: seen.append((kind, info))
        y_on = run(True)
        ops.BLOCK_LAUNCH_HOOK = None
        small = [info for kind, info in seen if kind == "smallm"]
        assert small == [(x.shape[0], sum(l.w.shape[0] for l in group), group[0].w.shape[1])], small
        assert torch.isfinite(y_on).all() and rel_l2(y_on, y_off) < 2e-3
        group[0]._bindings.clear()
        group[0].packed_weight()._mx6_ok = False                          # as a W8 or fractional-z weight reports itself
        assert torch.equal(run(True), run(False))
    finally:
        ops.MX_SMALLM_BATCH, ops.BLOCK_LAUNCH_HOOK = False, None


def test_bad_arguments_are_refused_before_any_launch():
    from dgq_amd import ops
    b6, b4, w8 = (types.SimpleNamespace(mx=True, w_bits=w, fmt=f) for w, f in ((4, "mxfp6"), (4, "mxfp4"), (8, "mxfp6")))
    for x, binds in ((torch.zeros(2, 48), [b6]), (torch.zeros(17, 64), [b6]), (torch.zeros(2, 64), [w8]), (torch.zeros(2, 64), [b6, b4])):
        with pytest.raises(AssertionError, match="linear_smallm_mx_batch"):
            ops.linear_smallm_mx_batch(x, binds)
