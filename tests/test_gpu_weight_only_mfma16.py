"""Weight-only state on the 16-bit matrix cores (dgq_conv2d_wq_mfma16, ops.conv2d_wq_mfma16, QuantLayer.weight_only_mfma16).

The route is opt-in and NOT bit-identical to the exact one (dgq_conv2d_wq), so the contract has two halves:
  * where every partial sum is exact in fp32 (small-integer x, power-of-two δ) the two routes and the float64 formula agree bit for
    bit — a wrong lane map, nibble order, word swap or geglu column shows as a wrong number, not as noise;
  * on random data every element satisfies the a-priori bound
        |y − y64| <= K·2^-24·S + u_x·S + u_out·|y64|,      S = |b| + Σ_k |x·δ(q − z)|,
    with u_x = 0 for 16-bit x and 2^-16 for fp32 x (the two-term bf16 split), u_out = 2^-24 / 2^-8 / 2^-11 for fp32 / bf16 / f16 y.
The kernel has two tile forms (wq16_pick: 64 x 64 with 64-deep K tiles where that launches >= 256 workgroups, else 32 x 32 with
128-deep K tiles); the cases name the form they take.  The first two tests need no GPU."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from dgq_amd import ops, _lib

gpu = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
U_OUT = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


# ------------------------------------------------------------------------------------------------------------- 1. / 2. no GPU
def test_conv2d_wq_mfma16_export_and_argument_checks():
    lib = _lib.load()
    assert lib.dgq_version() == 123
    f = lib.dgq_conv2d_wq_mfma16
    x = y = d = z = w = 1 << 20          # never dereferenced: every call below is refused before a launch
    args = dict(x=x, x_dtype=0, B=1, H=1, W=1, C=64, kh=1, kw=1, stride=1, pad=0, upsample=0, w=w, bits=4, Kp=128, d=d, z=z, bias=None,
                N=32, geglu=0, y=y, y_dtype=0, ldy=32, stream=None)

    def call(**kw):
        a = dict(args, **kw)
        return f(a["x"], a["x_dtype"], a["B"], a["H"], a["W"], a["C"], a["kh"], a["kw"], a["stride"], a["pad"], a["upsample"],
                 a["w"], a["bits"], a["Kp"], a["d"], a["z"], a["bias"], a["N"], a["geglu"], a["y"], a["y_dtype"], a["ldy"], a["stream"])
    for bad, what in [(dict(bits=2), "w_bits"), (dict(Kp=96), "Kp"), (dict(Kp=128, C=200), "Kp"), (dict(N=8, ldy=8), "N=8"),
                      (dict(ldy=16), "ldy"), (dict(x=None), "null"), (dict(x_dtype=5), "dtype"),
                      (dict(upsample=1), "upsample"), (dict(geglu=1, N=33, ldy=33), "geglu_rows")]:
        assert call(**bad) == -1, bad
        assert "dgq_conv2d_wq_mfma16" in _lib.last_error() and what in _lib.last_error(), (bad, _lib.last_error())


def _minmax_codes(w, bits):
    """(codes, δ, z) of a per-channel MINMAX quantiser, on the CPU"""
    qmax = 2 ** bits - 1
    flat = w.reshape(w.shape[0], -1)
    lo, hi = flat.amin(1).clamp(max=0.0), flat.amax(1).clamp(min=0.0)
    delta = ((hi - lo) / qmax).clamp_min(1e-8)
    zp = (-lo / delta).round()
    codes = (torch.round(flat / delta[:, None]) + zp[:, None]).clamp(0, qmax).to(torch.uint8)
    return codes, delta, zp


def test_eligibility_switch_and_cli_refusal():
    from dgq_amd import inference_qmodel
    from dgq_amd.diffusers_rewrite import UNet2DConditionModel
    from dgq_amd.quant import QuantModel, QuantLayer, Scaler, QMODE
    w = torch.randn(24, 40, generator=torch.Generator().manual_seed(0))
    for bits in (4, 8):
        codes, _, zp = _minmax_codes(w, bits)
        assert ops.PackedWeight.check_mfma16(codes, zp, bits)
        assert not ops.PackedWeight.check_mfma16(codes, zp + 0.25, bits)                     # a fractional zero point
        far = zp.clone()
        far[3] = -300.0                                                                      # integral, but q − z leaves the exact range
        assert not ops.PackedWeight.check_mfma16(codes, far, bits)
    # the setter reaches every layer, both ways; the attribute is off by default
    qnn = QuantModel(model=UNet2DConditionModel("tiny"), wq_params={"bits": 4, "channel_wise": True, "scaler": Scaler.MINMAX},
                     aq_params={"bits": 8, "channel_wise": False, "scaler": Scaler.MINMAX, "leaf_param": False},
                     softmax_aq_params={"softmax_a_bit": 8, "t2i_log_quant": False, "t2i_real_time": False, "t2i_start_peak": False,
                                        "log_max_1": False},
                     aq_mode=[QMODE.NORMAL.value, QMODE.QDIFF.value], tib_recon=False)
    layers = [m for m in qnn.modules() if isinstance(m, QuantLayer)]
    assert len(layers) > 10 and not any(m.weight_only_mfma16 for m in layers)
    qnn.set_weight_only_mfma16(True)
    assert all(m.weight_only_mfma16 for m in layers)
    qnn.set_weight_only_mfma16(False)
    assert not any(m.weight_only_mfma16 for m in layers)
    # the command line refuses the flag beside --use_aq before anything is built
    with pytest.raises(SystemExit) as e:
        inference_qmodel.main(["--wq_mfma16", "--use_aq", "--model_type", "tiny"])
    assert "--use_aq" in str(e.value)
    assert inference_qmodel.parse_args([]).wq_mfma16 is False and inference_qmodel.parse_args(["--wq_mfma16"]).wq_mfma16 is True


# ------------------------------------------------------------------------------------------------------------- cases and references
def _lin(M, K, N, **kw):
    return dict(x=(M, K), C=K, N=N, k=1, s=1, p=0, ups=False, geglu=False, **kw)


def _conv(B, C, H, W, N, k, s, p, ups=False):
    return dict(x=(B, C, H, W), C=C, N=N, k=k, s=s, p=p, ups=ups, geglu=False)


#: the issue's cases (all on the 32 x 32 form) ...
CASES = {
    "linear_37x320_24": _lin(37, 320, 24),                       # ragged M, N below a tile
    "linear_70x360_72": _lin(70, 360, 72),                       # K no multiple of 32 or 64, rows with n & 16 set
    "conv3_s1": _conv(2, 64, 8, 8, 64, 3, 1, 1),
    "conv3_s2": _conv(2, 64, 8, 8, 64, 3, 2, 1),
    "conv3_upsample_4x4": _conv(2, 64, 4, 4, 64, 3, 1, 1, ups=True),
    "conv1_1x96x5x7_40": _conv(1, 96, 5, 7, 40, 1, 1, 0),
    "geglu_33x64_128": dict(_lin(33, 64, 128), geglu=True),
    # ... and every other path of the kernel: C no multiple of 8 (the element-wise load; 7: K % 8 != 0 too) and the 64 x 64 form
    # (16 x 17 = 272 tiles, ragged both ways; K = 72: two K tiles, the second partial; K = 136: three)
    "conv3_c20": _conv(1, 20, 10, 11, 40, 3, 1, 1),
    "conv3_c7_s2": _conv(2, 7, 9, 10, 330, 3, 2, 1),
    "t64_1000x72_1030": _lin(1000, 72, 1030),
    "t64_1000x136_1030": _lin(1000, 136, 1030),
}
#: the long chain on the small tile, random data only (K = 1280 as a Linear layer, K = 2880 as the 3x3 conv of M = 128 rows)
LONG = {
    "linear_128x1280_40": _lin(128, 1280, 40),
    "conv3_128rows_k2880_40": _conv(2, 320, 8, 8, 40, 3, 1, 1),
}


def _row_perm(N):
    return torch.stack([torch.arange(N // 2), torch.arange(N // 2) + N // 2], 1).flatten()


def _pack(c, w, delta, zp, b, bits):
    """PackedWeight of the case (rows interleaved for geglu) from the reference-order operands"""
    w, delta, zp, b = w.cuda(), delta.cuda(), zp.cuda(), b.cuda()
    if c["geglu"]:
        rp = _row_perm(c["N"]).cuda()
        w, delta, zp, b = w[rp], delta[rp], zp[rp], b[rp]
    return ops.PackedWeight(w, delta, zp, None, b, bits, c["C"], c["k"] * c["k"])


def _ref64(c, x, w64, b64):
    """(y64, S) in the layout the ops return: the float64 value of the formula and S = |b| + Σ |x·ŵ|"""
    x64 = x.double()
    if c["ups"]:
        x64 = F.interpolate(x64, scale_factor=2.0, mode="nearest")
    if x.dim() == 4:
        return (F.conv2d(x64, w64, b64, stride=c["s"], padding=c["p"]), F.conv2d(x64.abs(), w64.abs(), b64.abs(), stride=c["s"], padding=c["p"]))
    return F.linear(x64, w64.flatten(1), b64), F.linear(x64.abs(), w64.flatten(1).abs(), b64.abs())


def _run(op, c, x, pw):
    return op(x, pw, c["k"], c["k"], c["s"], c["p"], upsample=c["ups"], geglu_rows=c["geglu"])


def _assert_bound(y, y64, S, K, x_dtype, what):
    u_x = 2.0 ** -16 if x_dtype == torch.float32 else 0.0
    bound = K * 2.0 ** -24 * S + u_x * S + U_OUT[y.dtype] * y64.abs()
    err = (y.double() - y64).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print("%s: max |err| / bound = %.3f" % (what, worst))
    assert y.shape == y64.shape and bool((err <= bound).all()), (what, worst)


# ------------------------------------------------------------------------------------------------------------- 3. exact-integer twin
@gpu
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "f16"])
@pytest.mark.parametrize("case", list(CASES))
def test_exact_integer_twin(case, dtype, bits):
    """x in {-3..3}, random codes and integer zero points (every row its own content), δ_n in {1/2, 1/4, 1/8}, bias in quarters:
    |Σ| <= 576·3·255 < 2^24, so every partial sum, δ·Σ and + b are exact in fp32 and the one rounding to y's dtype is that of the
    float64 value: torch.equal to the formula and to the exact route."""
    c = CASES[case]
    N, C, k, qmax = c["N"], c["C"], c["k"], 2 ** bits - 1
    g = torch.Generator().manual_seed(sum(map(ord, case)) + bits)
    codes = torch.randint(0, qmax + 1, (N, C, k, k), generator=g)
    zp = torch.randint(0, qmax + 1, (N,), generator=g).float()
    delta = 2.0 ** -(1.0 + (torch.arange(N) % 3).float())
    w = delta[:, None, None, None] * (codes.float() - zp[:, None, None, None])
    b = torch.randint(-8, 9, (N,), generator=g).float() / 4
    x = torch.randint(-3, 4, c["x"], generator=g).float().to(dtype).cuda()
    with torch.no_grad():
        pw = _pack(c, w, delta, zp, b, bits)
        rp = _row_perm(N) if c["geglu"] else torch.arange(N)
        assert torch.equal(pw.codes.cpu(), codes.flatten(1)[rp].to(torch.uint8)) and pw.mfma16_eligible()    # (the test's own construction)
        y64, _ = _ref64(c, x, w.double().cuda(), b.double().cuda())
        y = _run(ops.conv2d_wq_mfma16, c, x, pw)
        y_exact = _run(ops.conv2d_wq, c, x, pw)
    assert y.dtype == dtype and y.shape == y64.shape
    want = y64.to(dtype)
    if not torch.equal(y, want):
        d = (y.double() - y64).abs()
        raise AssertionError("differs from the float64 formula in %d of %d elements, max |diff| %.3g" % (int((y != want).sum()), d.numel(), float(d.max())))
    assert torch.equal(y, y_exact)


# ------------------------------------------------------------------------------------------------------------- 4. random data
def _random_layer(c, bits, seed):
    g = torch.Generator().manual_seed(seed)
    N, C, k = c["N"], c["C"], c["k"]
    w = torch.randn(N, C, k, k, generator=g) / (C * k * k) ** 0.5
    _, delta, zp = _minmax_codes(w, bits)
    b = torch.randn(N, generator=g)
    return w, delta, zp, b


@gpu
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "f16"])
@pytest.mark.parametrize("case", list(CASES) + list(LONG))
def test_random_against_float64_per_element(case, dtype, bits):
    c = dict(CASES, **LONG)[case]
    w, delta, zp, b = _random_layer(c, bits, 100 + len(case))
    x = torch.randn(c["x"], generator=torch.Generator().manual_seed(7 + len(case))).to(dtype).cuda()
    with torch.no_grad():
        pw = _pack(c, w, delta, zp, b, bits)
        assert pw.mfma16_eligible()
        rinv = torch.argsort(_row_perm(c["N"])).cuda() if c["geglu"] else torch.arange(c["N"]).cuda()
        wq = (pw.alpha.double()[:, None] * (pw.codes.double() - pw.zp_true.double()[:, None]))[rinv].view(w.shape)   # δ·(q − z) in float64
        y64, S = _ref64(c, x, wq, b.double().cuda())
        y = _run(ops.conv2d_wq_mfma16, c, x, pw)
        y_exact = _run(ops.conv2d_wq, c, x, pw)
    print("%s W%d %s: rel-L2 to ops.conv2d_wq %.3e" % (case, bits, dtype, float((y.double() - y_exact.double()).norm() / y_exact.double().norm())))
    _assert_bound(y, y64, S, c["C"] * c["k"] ** 2, dtype, case)


# ------------------------------------------------------------------------------------------------------------- 5. one QuantLayer
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
        n = {k: self.names.count(k) for k in ("dgq_conv2d_wq", "dgq_conv2d_wq_mfma16")}
        self.names.clear()
        return n["dgq_conv2d_wq"], n["dgq_conv2d_wq_mfma16"]


def _qlayer(mod, bits, geglu=False):
    from dgq_amd.quant import QuantLayer, Scaler
    q = QuantLayer(mod, wq_params={"bits": bits, "channel_wise": True, "scaler": Scaler.MINMAX},
                   aq_params={"bits": 8, "channel_wise": False, "scaler": Scaler.MINMAX, "leaf_param": False})
    q.set_quant_state(True, False)
    q.geglu_rows = geglu
    return q.cuda()


@gpu
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_layer_switch_on_against_off(bits, dtype, monkeypatch):
    torch.manual_seed(0)
    spy = _Spy(monkeypatch)
    g = torch.Generator().manual_seed(3)
    for what, mod, xs, geglu, ups in [("linear", nn.Linear(320, 72), (2, 19, 320), False, False),
                                      ("conv3", nn.Conv2d(64, 96, 3, padding=1), (1, 64, 8, 8), False, False),
                                      ("upsampled", nn.Conv2d(64, 96, 3, padding=1), (1, 64, 4, 6), False, True),
                                      ("geglu", nn.Linear(64, 128), (33, 64), True, False)]:
        layer = _qlayer(mod, bits, geglu).to(dtype)
        x = torch.randn(xs, generator=g).to(dtype).cuda()
        fwd = layer.forward_upsampled if ups else layer
        with torch.no_grad():
            y_off = fwd(x)
            assert spy.take() == (1, 0), what
            layer.weight_only_mfma16 = True
            assert layer.takes_mfma16()
            y_on = fwd(x)
            assert spy.take() == (0, 1), what
            w64 = layer.dequantized_weight(torch.float32).double()
            b64 = layer.b.double()
            c = dict(ups=ups, s=mod.stride[0] if layer.is_conv else 1, p=mod.padding[0] if layer.is_conv else 0)
            y64, S = _ref64(c, x, w64, b64)
        assert y_on.dtype == y_off.dtype == dtype
        _assert_bound(y_on, y64, S, layer.w[0].numel(), dtype, "%s W%d" % (what, bits))
        print("%s: rel-L2 switch on against off %.3e" % (what, float((y_on.double() - y_off.double()).norm() / y_off.double().norm())))
    # an ineligible weight (a fractional zero point) stays on the exact entry with the switch on; the flag is computed once per weight
    layer = _qlayer(nn.Linear(320, 72), bits).to(dtype)
    layer.weight_only_mfma16 = True
    x = torch.randn((5, 320), generator=g).to(dtype).cuda()
    with torch.no_grad():
        layer(x)
        assert spy.take() == (0, 1)
        pw = layer.packed_weight()
        assert pw._mfma16 is True and layer.packed_weight() is pw
        layer.wqtizer.zero_point.add_(0.5)                          # (in place: the weight key changes, the layer re-packs)
        y = layer(x)
        assert spy.take() == (1, 0)
        assert layer.packed_weight() is not pw and not layer.packed_weight().mfma16_eligible() and not layer.takes_mfma16()
    assert torch.isfinite(y.float()).all()


# ------------------------------------------------------------------------------------------------------------- 6. tiny UNet
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


@gpu
@pytest.mark.parametrize("bits", [4, 8])
def test_tiny_unet_routing_graphs_and_accuracy(bits, monkeypatch):
    """Routing: with the switch on every call that the exact packed route took takes the new entry (every MINMAX weight is eligible;
    no layer is kept back by a rule).  Graphs: a replay equals the eager run bit for bit, and the setter drops a captured graph.
    Accuracy, against a yardstick measured on the exact route alone: d0 = rel-L2 between its bf16-state and its fp32-state output;
    the new route stays within d0 of the exact route in either state."""
    from dgq_amd import synth
    from dgq_amd.quant import QuantLayer
    spy = _Spy(monkeypatch)
    qnn = _tiny_qnn(bits)
    inp = synth.synth_inputs("tiny", 2, 1, 16)
    x, ctx, t = inp["sample"].cuda(), inp["encoder_hidden_states"].cuda(), torch.tensor(999)
    layers = [m for m in qnn.modules() if isinstance(m, QuantLayer) and m.use_wq]
    out = {}
    with torch.no_grad():
        for dtype in (torch.float32, torch.bfloat16):
            if dtype == torch.bfloat16:
                qnn = qnn.to(torch.bfloat16)
            xd, cd = x.to(dtype), ctx.to(dtype)
            qnn.set_weight_only_mfma16(False)
            out["exact", dtype] = qnn(xd, t, cd)[0].clone()
            n_old, n_new = spy.take()
            assert n_old >= len(layers) > 0 and n_new == 0
            assert all(m.packed_weight().mfma16_eligible() for m in layers)
            qnn.set_weight_only_mfma16(True)
            out["new", dtype] = qnn(xd, t, cd)[0].clone()
            assert spy.take() == (0, n_old)
            assert out["new", dtype].dtype == dtype and torch.isfinite(out["new", dtype].float()).all()
            # graph replay == eager, bit for bit; the setter after a capture gives the other route, not a stale replay
            qnn.enable_graphs(True)
            qnn(xd, t, cd)
            y_graph = qnn(xd, t, cd)[0].clone()
            spy.take()
            qnn.set_weight_only_mfma16(False)
            y_flip = qnn(xd, t, cd)[0].clone()
            assert spy.take() == (2 * n_old, 0)                  # (warmed up and captured again, on the exact route)
            y_flip_replay = qnn(xd, t, cd)[0].clone()
            assert spy.take() == (0, 0)                          # (a replay: no entry is called)
            qnn.enable_graphs(False)
            assert torch.equal(y_graph, out["new", dtype])
            assert torch.equal(y_flip, out["exact", dtype]) and torch.equal(y_flip_replay, out["exact", dtype])
            assert not torch.equal(out["new", dtype], out["exact", dtype])
    d0 = _rel(out["exact", torch.bfloat16].float(), out["exact", torch.float32])
    d_bf16 = _rel(out["new", torch.bfloat16], out["exact", torch.bfloat16])
    d_fp32 = _rel(out["new", torch.float32], out["exact", torch.float32])
    print("W%d tiny UNet: d0 (exact bf16 state vs exact fp32 state) %.3e; new vs exact: bf16 state %.3e, fp32 state %.3e" % (bits, d0, d_bf16, d_fp32))
    assert d_bf16 <= d0 and d_fp32 <= d0
