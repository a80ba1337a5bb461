"""W8 weights under the real-time MX activation formats (real_time_mx_w8=True: dgq_pack_w_mx6x2 + dgq_gemm_mxw8, W8A6 / W8A8).  The
weight image must be the statement's bytes (``mxw8_split`` + ``mx6_pack``); one-hot operands pin the plane order, the six weight-side
scale bytes and the operand maps; planted exact layers EQUAL float64; real data stays inside the a-priori bound of a fp32 sum."""
import types

import pytest
import torch
import torch.nn.functional as F

from tests import layer_reference as lr
from tests import mxfp6_ref as mx
from tests import test_gpu_groupnorm_stats as gs
from tests import test_gpu_layer_routes as routes
from tests import test_gpu_realtime_act as rta
from tests.test_gpu_realtime_act import dev, rt_inputs          # noqa: F401  (module-scoped fixtures of the row mode)
from tests.test_gpu_realtime_mxfp6 import _handmade
from tests.test_gpu_realtime_mxint8 import planes

pytestmark = pytest.mark.gpu
FMTS = ["mxfp6", "mxint8"]
NA = dict(mxfp6=1, mxint8=2)
LIN, CONV = lr.linear_case(37, 320, 24), lambda stride=1: lr.conv_case(2, 64, 5, 7, stride, 24)
PLANT = torch.tensor([5, 48, 183, -200, 255, -255, 0])         # L only, H only, both, negative, the ends


def planted_weight(N, K):
    """(qw, zw, wd): every column n under z = 0, 255 or 200, its q − z drawn from PLANT asymmetrically in (n, k) (the sign flipped, else
    0, where q would leave 0 .. 255), power-of-two δw"""
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    zw = torch.tensor([0, 255, 200])[torch.arange(N) % 3]
    d = PLANT[(3 * n + 5 * k + (n * k) % 7 + k // 32) % 7]
    d = torch.where((d + zw[:, None] < 0) | (d + zw[:, None] > 255), -d, d)
    d = torch.where((d + zw[:, None] < 0) | (d + zw[:, None] > 255), 0, d)
    return d + zw[:, None], zw.float(), (2.0 ** ((torch.arange(N) % 3) - 1).double()).float()


def binding(ops, dev, fmt, qw, zw, wd, bias=None, C=None, taps=1):
    """MxActBinding on the W8 image of w = δw·(q − z), qw [N][C·taps] in the reference order; the codes must come back as planted"""
    N, C = qw.shape[0], C or qw.shape[1]
    shape = (N, C, 3, 3) if taps == 9 else (N, C)
    one = (N,) + (1,) * (len(shape) - 1)
    w = (wd[:, None] * (qw.float() - zw[:, None])).view(shape)
    pw = ops.PackedWeight(w.to(dev), wd.view(one).to(dev), zw.view(one).to(dev), None, bias.to(dev) if bias is not None else None, 8, C, taps)
    assert torch.equal(pw.codes.cpu().long(), qw) and pw.mxw8_eligible and not pw.mx6_eligible
    return ops.MxActBinding(pw, fmt, w_bits=8)


@pytest.mark.parametrize("C,taps", [(320, 1), (32, 9)], ids=["linear", "conv3x3"])
def test_weight_image_is_the_statement(C, taps, dev):
    """K = 320 and 288 under Kp = 384: the K padding, and the natural (tap, c) order of a convolution"""
    from dgq_amd import ops
    from dgq_amd.quant.quant_layer import mx6_pack, mxw8_split
    qw, zw, wd = planted_weight(24, C * taps)
    ab = binding(ops, dev, "mxfp6", qw, zw, wd, C=C, taps=taps)
    nat = F.pad((qw - zw.long()[:, None]).view(24, C, taps).permute(0, 2, 1).reshape(24, -1), (0, 384 - C * taps))
    assert ab.Kp == 384 and ab.wpacked is ab.pw.mx6x2()[0] and set(nat.unique().tolist()) >= set(PLANT.tolist())
    assert torch.equal(ab.wpacked.cpu(), torch.cat([mx6_pack(p) for p in mxw8_split(nat)], dim=2))


@pytest.mark.parametrize("hot", [5, 48, 77, "weights"], ids=["lo", "hi", "both", "weights"])
@pytest.mark.parametrize("M,K,N", [(64, 64, 64), (37, 320, 24), (64, 96, 64)])
@pytest.mark.parametrize("fmt", FMTS)
def test_operand_maps_one_hot(fmt, M, K, N, hot, dev):
    """activations: row m holds ONE code at k_m (MXINT8: lo plane only, hi plane only, both; MXFP6: the E2M3 code of that number) against
    the planted weights, every (row, block) under its own E: y[m, n] = δw[n]·(q − z)[n, k_m]·x̂[m, k_m].  weights: column n holds ONE
    q − z = ±183 (both planes) at k_n under codes asymmetric in (m, k): y[m, n] = δw[n]·(∓)183·x̂[m, k_n].  One non-zero term per element
    (MXINT8 weights: four partial products, integers below 2^24 in units of 2^(E−6)): a gather, bit for bit."""
    from dgq_amd import ops
    m, k = torch.arange(M)[:, None], torch.arange(K)[None, :]
    if hot == "weights":
        zw, wd = torch.tensor([0.0, 255.0])[torch.arange(N) % 2], (2.0 ** ((torch.arange(N) % 3) - 1).double()).float()
        qw = zw.long()[:, None].repeat(1, K)
        qw[torch.arange(N), (torch.arange(N) * 5 + 1) % K] += torch.where(zw == 0, 183, -183)
        code = (7 * m + 11 * k + (m * k) % 5) % (64 if fmt == "mxfp6" else 255) - (0 if fmt == "mxfp6" else 127)
    else:
        qw, zw, wd = planted_weight(N, K)
        code = torch.where(k == (m * 7 + 3) % K, hot % 64 if fmt == "mxfp6" else hot, 0)
    ab = binding(ops, dev, fmt, qw, zw, wd)
    E = torch.randint(-6, 7, (M, K // 32), generator=torch.Generator().manual_seed(M + K))
    if fmt == "mxfp6":
        q, xhat = _handmade(ops, dev, code, E, ab.Kp // 32), mx.decode(code.to(torch.uint8), (E + 127).to(torch.uint8))
    else:
        q, xhat = tuple(t.to(dev) for t in planes(code, E, ab.Kp // 32)), code.double() * (2.0 ** (E.double() - 6.0)).repeat_interleave(32, dim=1)
    got = ops.gemm_mxw8(q, (M, 1, 1, K, 1, 1, 1, 0), ab, torch.float32).cpu().double()
    want = xhat @ (wd[:, None].double() * (qw.double() - zw[:, None].double())).t()
    assert torch.equal(got, want), (got != want).nonzero()[:4].tolist()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=gs.ids_dtype)
@pytest.mark.parametrize("case,form", [(LIN, "plain"), (CONV(), "plain"), (CONV(2), "plain"), (CONV(), "residual"), (LIN, "geglu")],
                         ids=lambda v: v["name"] if isinstance(v, dict) else v)
@pytest.mark.parametrize("fmt", FMTS)
def test_exact_layers_equal_the_reference(fmt, case, form, dtype, dev):
    """random W8 codes and zero points (|q − z| up to 255), power-of-two δw, integer bias and residual under x′ = s·2^(E−6), s a multiple of
    8 with |s| <= 64 and one 64 per block (E in −3 .. 0): x̂ = x′ under BOTH formats (MXFP6: x′·2^(2−E) = s/16, multiples of 0.5 up to 4).
    Every term is a multiple of u = 2^-7 (x̂ of 2^-6, δw >= 1/2) and the magnitudes sum below 2^24·u = 2^17 (asserted), so every fp32
    step is exact in any order and y EQUALS the float64 layer rounded once.  geglu: the gate columns (odd n) have q = z and a bias of
    ±16, where erff saturates — the output is value·16 or 0."""
    from dgq_amd import ops
    B, H, W, Ho, Wo, M, K, taps = lr.geometry(case)
    N, lin = case["N"], case["kind"] == "linear"
    g = torch.Generator().manual_seed(lr._seed("planted-mxw8", case["name"], form))
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g)
    qw, zw, wd, bias = ri(0, 255, (N, K)), ri(0, 255, (N,)).float(), (2.0 ** ri(-1, 1, (N,)).double()).float(), ri(-8, 8, (N,)).float()
    if form == "geglu":
        qw[1::2], bias[1::2] = zw.long()[1::2, None], torch.tensor([16.0, -16.0]).repeat(N // 4)
    rows = M if lin else B * H * W
    s = 8 * ri(-8, 8, (rows, K // taps // 32, 32))
    s[:, :, 0] = 64
    like = torch.empty((1, M, K) if lin else (B, case["C"], H, W))
    x = mx.rows_to_input(case, (s.double() * 2.0 ** (ri(-3, 0, (rows, K // taps // 32, 1)).double() - 6.0)).float().reshape(rows, -1), like).contiguous()
    res = ri(-8, 8, (1, M, N) if lin else (B, N, Ho, Wo)).float() if form == "residual" else None
    y64 = mx.layer_float64(case, x.double(), qw, zw, wd, bias, res)
    assert float(mx.term_magnitudes(case, x.double(), qw, zw, wd, bias).max()) + 8 < 2.0 ** 17
    if form == "geglu":
        y64 = y64[..., 0::2] * F.gelu(y64[..., 1::2])
    ab = binding(ops, dev, fmt, qw, zw, wd, bias, C=K // taps, taps=taps)
    y = routes.run_layer(ops, case, ab, x.to(dev, dtype), res.to(dev, dtype) if res is not None else None, **(dict(geglu=True) if form == "geglu" else {}))
    assert y.dtype == dtype and torch.equal(y.cpu(), y64.float().to(dtype)), (y.cpu().double() != y64).nonzero()[:4].tolist()


@pytest.mark.parametrize("data", ["randn", "outlier"])
@pytest.mark.parametrize("case,ksplit", [(LIN, 1), (CONV(), 1), (lr.linear_case(64, 512, 64), 2)], ids=lambda v: v["name"] if isinstance(v, dict) else "S%d" % v)
@pytest.mark.parametrize("fmt", FMTS)
def test_real_layers_inside_the_bound(fmt, case, ksplit, data, dev, capsys, monkeypatch):
    """per element |y − y64| <= 2^-24·|y64| + c·(2·NA·K)·2^-24·T with c = 1, the a-priori ceiling of one rounding per accumulated exact
    product: y64 the float64 sum over the KERNEL's own codes (dequantised by the library, exact in fp32), T = |b| + δw·Σ|x̂·(q − z)|.
    Worst measured ratio: profiles/r24_realtime_mx_w8.txt.  ksplit 2 (two K tiles, one per split): the split launch and its combine
    inside the same bound; every layer runs twice to identical bits."""
    from dgq_amd import ops
    B, H, W, Ho, Wo, M, K, taps = lr.geometry(case)
    d = lr.real_case(case, "perM", 8, 8)
    x, lin = d["x"], case["kind"] == "linear"
    if data == "outlier":
        x = mx.rows_to_input(case, mx.outlier_rows(mx.input_rows(case, x)), x).contiguous()
    ab = ops.MxActBinding(ops.PackedWeight(d["w_raw"].to(dev), d["wdelta"].to(dev), d["wzp"].to(dev), None, d["bias"].to(dev), 8, K // taps, taps), fmt, w_bits=8)
    spy = gs.spied(ops, monkeypatch)
    monkeypatch.setattr(ops, "MX_KSPLIT", ksplit)
    y, y2 = (routes.run_layer(ops, case, ab, x.to(dev), None) for _ in range(2))
    names = [c["name"] for c in spy.take()]
    assert torch.equal(y, y2) and names.count("dgq_gemm_mxw8_splitk" if ksplit > 1 else "dgq_gemm_mxw8") == 2, names
    xs = x.to(dev).reshape(M, K) if lin else x.to(dev).contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
    quant, dequant = (ops.quant_act_mx6, ops.dequant_act_mx6) if fmt == "mxfp6" else (ops.quant_act_mxint8, ops.dequant_act_mxint8)
    q = quant(xs, (M, 1, 1, K, 1, 1, 1, 0) if lin else (B, H, W, K // taps, 3, 3, 1, 1))
    xhat = mx.rows_to_input(case, dequant(q[0], q[1], torch.empty(q[0].shape[0], K // taps, device=dev)).cpu().double(), x)
    qw, zw, wd = ab.pw.codes.cpu().long(), ab.pw.zp_true.cpu(), ab.pw.alpha.cpu()
    y, y64, T = y.cpu().double(), mx.layer_float64(case, xhat, qw, zw, wd, d["bias"]), mx.term_magnitudes(case, xhat, qw, zw, wd, d["bias"])
    err, unit_sum = (y - y64).abs(), 2 * NA[fmt] * K * 2.0 ** -24 * T
    with capsys.disabled():
        print("\nREAL-TIME MX W8 %s %s %s S%d: worst |y - y64| / (%dK 2^-24 T) = %.4g" % (fmt, case["name"], data, ksplit, 2 * NA[fmt], float((err / unit_sum).max())))
    assert bool((err <= 2.0 ** -24 * y64.abs() + unit_sum).all())


def _quant_layer(dev, fmt, flag, frac):
    from dgq_amd.quant import QuantLayer, Scaler
    torch.manual_seed(7)
    aq = dict(bits=6 if fmt == "mxfp6" else 8, channel_wise=False, scaler=Scaler.MINMAX, leaf_param=True, real_time=True, real_time_block=32,
              real_time_format=fmt, real_time_mx_w8=flag)
    layer = QuantLayer(torch.nn.Linear(64, 64), dict(bits=8, channel_wise=True, scaler=Scaler.MINMAX), aq).to(dev)
    layer.set_quant_state(True, True)
    layer.wqtizer.init_from(layer.w.data)
    if frac:
        layer.wqtizer.zero_point = layer.wqtizer.zero_point + 0.5
    return layer


@pytest.mark.parametrize("fmt", FMTS)
def test_quant_layer_takes_the_w8_image(fmt, dev):
    """W8 Linear 64 x 64 -> 64: with the flag the MX binding on the two-plane image, inside the bound against the float64 layer under the
    format's statement; with fractional zero points the flag changes nothing, bit for bit"""
    from dgq_amd import ops
    from dgq_amd.quant import quant_layer as ql
    x = torch.randn(64, 64, generator=torch.Generator().manual_seed(3)) * 1.3 + 0.2
    layer = _quant_layer(dev, fmt, True, False)
    with torch.no_grad():
        y = layer(x.to(dev)).cpu().double()
        frac_on, frac_off = (_quant_layer(dev, fmt, flag, True)(x.to(dev)) for flag in (True, False))
    ab = layer._bindings["real_time"]
    assert isinstance(ab, ops.MxActBinding) and ab.fmt == fmt and ab.w_bits == 8 and ab.wpacked is layer._pw._mx6x2[0]
    xhat = (ql.mx6_block if fmt == "mxfp6" else ql.mxint8_block)(x)[2].double()
    w, b = layer.dequantized_weight(torch.float32).double().cpu(), layer.b.detach().double().cpu()
    y64, T = xhat @ w.t() + b, xhat.abs() @ w.abs().t() + b.abs()
    assert bool(((y - y64).abs() <= 2.0 ** -24 * y64.abs() + 2 * NA[fmt] * 64 * 2.0 ** -24 * T).all())
    assert torch.equal(frac_on, frac_off)


@pytest.mark.parametrize("fmt", FMTS)
def test_model_from_a_w8_checkpoint_and_graph_replay(fmt, tmp_path, rt_inputs, dev):
    from dgq_amd import ops, synth
    from dgq_amd.diffusers_rewrite import UNet2DConditionModel
    from dgq_amd.quant import get_qmodel, Scaler
    from dgq_amd.runtime import quant_params
    path, abits = str(tmp_path / "wonly.pth"), 6 if fmt == "mxfp6" else 8
    synth.write_cali_ckpt(path, "tiny", 8, abits, 1, num_slots=1, seed=0, batch=2, res=16, start_peak=True, with_act=False)
    unet = UNet2DConditionModel("tiny")
    unet.load_state_dict(synth.state_dict_from_ckpt(path))
    wq, aq, sm = quant_params(Scaler, 8, abits, True, True, True, True)
    aq.update(real_time=True, real_time_block=32, real_time_format=fmt, real_time_mx_w8=True)
    qnn = get_qmodel("tiny", types.SimpleNamespace(unet=unet), path, wq, True, aq, sm, False, 25, False, device=dev).float().to(dev)
    qnn.disable_out_quantization()
    x, ctx = rt_inputs
    with torch.no_grad():
        y_e = qnn(x, torch.tensor(999), ctx)[0].clone()
        qnn.enable_graphs(True)
        y_g = [qnn(x, torch.tensor(999), ctx)[0].clone() for _ in range(3)]
        qnn.enable_graphs(False)
    assert torch.isfinite(y_e).all() and all(torch.equal(y, y_e) for y in y_g), "graph replay differs from the eager run"
    for name, layer in rta._inner_layers(qnn).items():      # every quantised layer of ``tiny`` has C % 32 == 0 and integer zero points
        ab = layer._bindings["real_time"]
        assert isinstance(ab, ops.MxActBinding) and ab.fmt == fmt and ab.w_bits == 8, name
