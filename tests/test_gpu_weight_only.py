"""Weight-only state from the packed W4 / W8 codes (dgq_conv2d_wq, ops.conv2d_wq, QuantLayer.WEIGHT_ONLY_PACKED).

The contract: every call on the new route returns, bit for bit, what dgq_conv2d_f32w returns on the dequantised fp32 weight —
kernel against kernel (twin), one QuantLayer on each route, a whole tiny UNet on each route (eager and graph-replayed).  The first
test needs no GPU: the export and the argument checks, which run before any launch."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from dgq_amd import ops, _lib

gpu = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def test_conv2d_wq_export_and_argument_checks():
    lib = _lib.load()
    assert lib.dgq_version() == 123
    f = lib.dgq_conv2d_wq
    x = y = d = z = w = 1 << 20          # never dereferenced: every call below is refused before a launch
    args = dict(x=x, x_dtype=0, B=1, H=1, W=1, C=64, kh=1, kw=1, stride=1, pad=0, upsample=0, w=w, bits=4, Kp=128, d=d, z=z, bias=None,
                N=32, geglu=0, y=y, y_dtype=0, ldy=32, stream=None)

    def call(**kw):
        a = dict(args, **kw)
        return f(a["x"], a["x_dtype"], a["B"], a["H"], a["W"], a["C"], a["kh"], a["kw"], a["stride"], a["pad"], a["upsample"],
                 a["w"], a["bits"], a["Kp"], a["d"], a["z"], a["bias"], a["N"], a["geglu"], a["y"], a["y_dtype"], a["ldy"], a["stream"])
    for bad, what in [(dict(bits=2), "w_bits"), (dict(Kp=96), "Kp"), (dict(Kp=128, C=200), "Kp"), (dict(N=8, ldy=8), "N=8"),
                      (dict(ldy=16), "ldy"), (dict(x=None), "null"), (dict(x_dtype=5), "dtype")]:
        assert call(**bad) == -1, bad
        assert "dgq_conv2d_wq" in _lib.last_error() and what in _lib.last_error(), (bad, _lib.last_error())


# ------------------------------------------------------------------------------------------------------------- helpers
def _packed(N, C, kh, kw, bits, seed, bias=True, rows=None):
    """(PackedWeight, natural fp32 weight [N][kh·kw·C] as dequantized_weight_natural builds it, bias) of a random layer; rows: a
    row permutation applied before packing (QuantLayer.geglu_rows), the natural weight and bias stay in the original order."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, C, kh, kw, generator=g) / (C * kh * kw) ** 0.5
    qmax = 2 ** bits - 1
    lo, hi = w.amin(dim=(1, 2, 3)), w.amax(dim=(1, 2, 3))
    delta = ((hi - lo) / qmax).clamp_min(1e-8)
    zp = (-lo / delta).round()
    b = torch.randn(N, generator=g) if bias else None
    w, delta, zp = w.cuda(), delta.cuda(), zp.cuda()
    b = b.cuda() if b is not None else None
    if rows is None:
        pw = ops.PackedWeight(w, delta, zp, None, b, bits, C, kh * kw)
        codes = pw.codes
    else:
        rp = rows.cuda()
        pw = ops.PackedWeight(w[rp], delta[rp], zp[rp], None, b[rp] if b is not None else None, bits, C, kh * kw)
        codes = pw.codes[torch.argsort(rp)]
    wq = delta[:, None] * (codes.float() - zp[:, None])          # δ·(q − z), as QuantLayer.dequantized_weight
    wn = wq.view(N, C, kh, kw).permute(0, 2, 3, 1).reshape(N, -1).contiguous()
    return pw, wn, (b.float().contiguous() if b is not None else None)


def _x(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype).cuda()


def _same(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if not torch.equal(a, b):
        d = (a.float() - b.float()).abs()
        raise AssertionError("not bit-identical: %d of %d elements differ, max |diff| %.3g" % (int((d != 0).sum()), d.numel(), float(d.max())))


# ------------------------------------------------------------------------------------------------------------- a. kernel twin
@gpu
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dtype", DTYPES)
def test_twin_linear_and_conv(bits, dtype):
    """Linear at M = 2 / 154 / 333 (ragged), convs 3x3 stride 1 / 2 and 1x1, ragged N (40, 330), C not a multiple of 32 (20) nor
    of 4 (7: the element-wise load, K % 16 != 0), no bias."""
    with torch.no_grad():
        for i, (M, K, N, bias) in enumerate([(2, 1280, 320, True), (154, 768, 640, True), (333, 320, 40, False), (154, 768, 330, True)]):
            pw, wn, b = _packed(N, K, 1, 1, bits, 10 + i, bias)
            x = _x((M, K) if i != 1 else (2, 77, K), dtype, 20 + i)
            _same(ops.conv2d_wq(x, pw, 1, 1, 1, 0), ops.conv2d_f32w(x, wn, b, 1, 1, 1, 0))
        for i, (B, C, H, N, k, s, p) in enumerate([(2, 64, 16, 96, 3, 1, 1), (2, 64, 16, 128, 3, 2, 1), (2, 64, 12, 128, 1, 1, 0),
                                                    (1, 20, 10, 40, 3, 1, 1), (2, 7, 9, 330, 3, 2, 1), (1, 32, 8, 24, 3, 1, 0)]):
            pw, wn, b = _packed(N, C, k, k, bits, 30 + i, bias=(i != 5))
            x = _x((B, C, H, H + 1), dtype, 40 + i)
            _same(ops.conv2d_wq(x, pw, k, k, s, p), ops.conv2d_f32w(x, wn, b, k, k, s, p))


@gpu
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_twin_upsample_and_geglu_rows(bits, dtype):
    with torch.no_grad():
        # Upsample2D: the interpolate folded into the load vs materialised
        pw, wn, b = _packed(96, 64, 3, 3, bits, 50)
        x = _x((2, 64, 8, 6), dtype, 51)
        _same(ops.conv2d_wq(x, pw, 3, 3, 1, 1, upsample=True),
              ops.conv2d_f32w(F.interpolate(x, scale_factor=2.0, mode="nearest"), wn, b, 3, 3, 1, 1))
        # ff.net.0 with interleaved rows: the output in the un-permuted order
        N = 320
        rp = torch.stack([torch.arange(N // 2), torch.arange(N // 2) + N // 2], 1).flatten()
        pw, wn, b = _packed(N, 64, 1, 1, bits, 52, rows=rp)
        x = _x((2, 40, 64), dtype, 53)
        _same(ops.conv2d_wq(x, pw, 1, 1, 1, 0, geglu_rows=True), ops.conv2d_f32w(x, wn, b, 1, 1, 1, 0))


@gpu
@pytest.mark.parametrize("bits,dtype", [(4, torch.float32), (8, torch.bfloat16)])
def test_twin_long_k_and_large_shapes(bits, dtype):
    """The latency form (M = 128 at K = 11520 / 23040: SD's 8x8 level for a CFG pair) and the throughput form (M = 8192 at
    N = 320, K = 2880; N = 2560, K = 320)."""
    with torch.no_grad():
        for i, (B, C, H, N, k) in enumerate([(2, 1280, 8, 640, 3), (2, 2560, 8, 320, 3), (2, 320, 64, 320, 3), (2, 320, 64, 2560, 1)]):
            pw, wn, b = _packed(N, C, k, k, bits, 60 + i)
            x = _x((B, C, H, H), dtype, 70 + i)
            _same(ops.conv2d_wq(x, pw, k, k, 1, k // 2), ops.conv2d_f32w(x, wn, b, k, k, 1, k // 2))


# ------------------------------------------------------------------------------------------------------------- b. layer
def _qlayer(mod, bits):
    from dgq_amd.quant import QuantLayer, Scaler
    q = QuantLayer(mod, wq_params={"bits": bits, "channel_wise": True, "scaler": Scaler.MINMAX},
                   aq_params={"bits": 8, "channel_wise": False, "scaler": Scaler.MINMAX, "leaf_param": False})
    q.set_quant_state(True, False)
    return q.cuda()


@gpu
@pytest.mark.parametrize("bits", [4, 8])
def test_layer_routes_are_bit_identical_without_fp32_weight(bits, monkeypatch):
    from dgq_amd.quant import quant_layer as ql
    torch.manual_seed(0)
    for mod, x in [(nn.Conv2d(64, 96, 3, padding=1), _x((1, 64, 8, 8), torch.float32, 80)),
                   (nn.Linear(320, 640), _x((1, 16, 320), torch.float32, 81))]:
        layer = _qlayer(mod, bits)
        N, K = layer.w.shape[0], layer.w[0].numel()
        with torch.no_grad():
            torch.cuda.synchronize()
            m0 = torch.cuda.memory_allocated()
            y_new = layer(x)
            torch.cuda.synchronize()
            grown = torch.cuda.memory_allocated() - m0
            assert layer._wdq is None and layer._wnat is None
            assert grown < N * K * 4, (grown, N * K * 4)
            monkeypatch.setattr(ql, "WEIGHT_ONLY_PACKED", False)
            y_old = layer(x)
            monkeypatch.setattr(ql, "WEIGHT_ONLY_PACKED", True)
            assert layer._wnat is not None                 # (the old route is what the comparison ran)
        _same(y_new, y_old)


# ------------------------------------------------------------------------------------------------------------- c./d. model
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


@gpu
@pytest.mark.parametrize("bits", [4, 8])
def test_tiny_unet_weight_only_routes_bit_identical(bits, monkeypatch):
    """The whole tiny UNet (resnets, cross-attention with GEGLU, downsampler, upsampler) in the weight-only state, fp32 and bf16:
    packed-code route == fp32-copy route, bit for bit; the graph replay equals the eager forward on the new route."""
    from dgq_amd import synth
    from dgq_amd.quant import quant_layer as ql
    from dgq_amd.quant import QuantLayer
    qnn = _tiny_qnn(bits)
    inp = synth.synth_inputs("tiny", 2, 1, 16)
    x, ctx, t = inp["sample"].cuda(), inp["encoder_hidden_states"].cuda(), torch.tensor(999)
    layers = [m for m in qnn.modules() if isinstance(m, QuantLayer) and m.use_wq]
    assert any(m.geglu_rows for m in layers)
    for dtype in (torch.float32, torch.bfloat16):
        if dtype == torch.bfloat16:
            qnn = qnn.to(torch.bfloat16)
        xd, cd = x.to(dtype), ctx.to(dtype)
        with torch.no_grad():
            y_new = qnn(xd, t, cd)[0].clone()
            assert all(m._wdq is None and m._wnat is None for m in layers)
            qnn.enable_graphs(True)
            qnn(xd, t, cd)
            y_graph = qnn(xd, t, cd)[0].clone()
            qnn.enable_graphs(False)
            monkeypatch.setattr(ql, "WEIGHT_ONLY_PACKED", False)
            y_old = qnn(xd, t, cd)[0].clone()
            monkeypatch.setattr(ql, "WEIGHT_ONLY_PACKED", True)
        assert y_new.dtype == dtype and torch.isfinite(y_new.float()).all()
        _same(y_new, y_old)
        _same(y_graph, y_new)
        for m in layers:                                   # (the next dtype starts from the new route again)
            m._wdq = m._wnat = None
