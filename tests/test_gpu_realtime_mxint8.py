"""Real-time MXINT8 activations on the block-scaled matrix cores (real_time_format="mxint8": dgq_quant_act_mxint8 + dgq_gemm_mxint8,
W4A8).  The quantiser must reproduce ``quant_layer.mxint8_block`` bit for bit, down to the bytes of the two code planes; one-hot
operands pin the operand maps and the two weight-side scale constants; planted exact layers EQUAL float64; real data stays in a bound."""
import pytest
import torch
import torch.nn.functional as F

from tests import layer_reference as lr
from tests import mxfp6_ref as mx
from tests import mxint8_ref as mi
from tests import realtime_block_ref as rb
from tests import test_gpu_groupnorm_stats as gs
from tests import test_gpu_layer_routes as routes
from tests import test_gpu_realtime_act as rta
from tests.test_gpu_realtime_act import dev, rt_inputs, rel_l2          # noqa: F401  (module-scoped fixtures of the row mode)
from tests.test_gpu_realtime_mxfp6 import _asym_weight, _packed_weight

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
#: c of the real-data bound |y − y64| <= u_out·|y64| + c·2K·2^-24·T: 4 x the worst ratio measured over test_real_layers_inside_the_bound's
#: cases (0.0004943, conv3x3 randn; profiles/r22_realtime_mxint8.txt), rounded up to a power of two.  c = 1 is the a-priori ceiling: ANY
#: fp32 summation order of the 2K exact products satisfies it; a wrong element, plane, block or scale shows at about 2^24 / 2K.
C_SUM = 2.0 ** -8


def planes(s, E, lds):
    """(codes uint8 [M][K/32][48], scale uint8 [M][lds]) as the quantiser writes them, from codes s [M][K] and exponents E [M][K/32]"""
    from dgq_amd.quant.quant_layer import mx6_pack, mxint8_split
    scale = torch.full((s.shape[0], lds), 127, dtype=torch.uint8)
    scale[:, :E.shape[1]] = (E + 127).to(torch.uint8)
    return torch.cat([mx6_pack(p) for p in mxint8_split(s.to(torch.int8))], dim=2).contiguous(), scale


def check_quantiser(got, rows, lds):
    """the packed bytes of both planes and the scale bytes (padding entries 127) of a launch against the statement on ``rows``"""
    from dgq_amd.quant.quant_layer import mxint8_block
    s, scale, xhat = mxint8_block(rows)
    want = planes(s, scale.long() - 127, lds)
    assert torch.equal(got[1].cpu(), want[1]) and torch.equal(got[0].cpu(), want[0])
    return s.long(), torch.pow(torch.tensor(2.0, dtype=torch.float64), scale.double() - 133.0).repeat_interleave(32, dim=1), xhat


@pytest.mark.parametrize("what,dtype", [(s, d) for s in ((154, 768), (37, 320)) for d in DTYPES] + [((2, 64, 11, 13), DTYPES[0]), ("edge", DTYPES[0])], ids=str)
def test_quantiser_and_dequantiser_bit_exact(what, dtype, dev):
    from dgq_amd import ops
    g = torch.Generator().manual_seed(5)
    if what != "edge" and len(what) == 4:                 # a convolution's input, per pixel
        B, C, H, W = what
        x = rta.special_image(torch.randn(B, C, H, W, generator=g) * 1.3 + 0.2)
        xs, rows, geom, lds = x.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1), rb.pixel_rows(x), (B, H, W, C, 3, 3, 1, 1), C // 32
    else:
        rows = mi.edge_blocks() if what == "edge" else rta.special_rows(torch.randn(*what, generator=g) * 1.3 + 0.2).to(dtype)
        M, K = rows.shape
        xs, geom, lds = rows, (M, 1, 1, K, 1, 1, 1, 0), (K + 127) // 128 * 4      # (37, 320): Kp = 384, two padding entries
    got = ops.quant_act_mxint8(xs.to(dev), geom, lds=lds)
    xhat = check_quantiser(got, rows.float(), lds)[2]
    for dt in DTYPES:                                     # x̂ bit for bit; 16-bit outputs: x̂ rounded once
        assert torch.equal(ops.dequant_act_mxint8(got[0], got[1], torch.empty(xhat.shape, device=dev, dtype=dt)).cpu(), xhat.to(dt))


def test_quantiser_folded_groupnorm_silu(dev):
    """SiLU is the device's own approximation: x′ is the CPU's only to within tol.  The statement is monotone in x′ under a fixed E, so
    every block whose E is the same at |x′| ± tol carries that E and codes between the statement's at x′ ± tol."""
    from dgq_amd import ops
    B, C, H, W = 2, 64, 8, 8
    g = torch.Generator().manual_seed(31)
    x = torch.randn(B, C, H, W, generator=g) * 1.3 + 0.2
    xs = x.to(dev).contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
    sc, sh = ops.groupnorm_scale_shift(xs, B, H * W, C, 32, 1e-5, (1 + 0.1 * torch.randn(C, generator=g)).to(dev), (0.1 * torch.randn(C, generator=g)).to(dev))
    codes, scale = (t.cpu() for t in ops.quant_act_mxint8(xs, (B, H, W, C, 3, 3, 1, 1), pre=(sc, sh, 1)))
    rows = rb.pixel_rows(F.silu(x * sc.cpu()[:, :, None, None] + sh.cpu()[:, :, None, None]))
    tol = 4e-6 * rows.abs() + 1e-7
    (s_lo, _, _), (s_hi, _, _) = mi.mxint8_reference(rows - tol), mi.mxint8_reference(rows + tol)
    e_lo, e_hi = mi.mxint8_reference(torch.clamp(rows.abs() - tol, min=0.0))[1], mi.mxint8_reference(rows.abs() + tol)[1]
    firm = e_lo == e_hi
    assert float(firm.float().mean()) > 0.98 and torch.equal(scale[firm], e_hi[firm])
    from dgq_amd.quant.quant_layer import mx6_unpack
    one = torch.full(scale.shape, 127, dtype=torch.uint8)
    hi, lo = (mx.decode(mx6_unpack(codes[:, :, o:o + 24].contiguous()), one) for o in (0, 24))      # the planes' values h/2, l/2
    s = (32.0 * hi + 2.0 * lo).to(torch.int64)
    assert bool(((s >= s_lo) & (s <= s_hi))[firm.repeat_interleave(32, dim=1)].all())


@pytest.mark.parametrize("hot", [5, 48, 77, -1, "weights"], ids=["lo", "hi", "both", "borrow", "weights"])
@pytest.mark.parametrize("M,K,N", [(64, 64, 64), (37, 320, 24)])
def test_operand_maps_one_hot(M, K, N, hot, dev):
    """activations: row m holds ONE code at k_m — lo plane only, hi plane only, both, and the borrow −1 = 16·(−1) + 15 — every (row,
    block) under its own E: y[m, n] = δw[n]·(q − z)[n, k_m]·x̂[m, k_m].  weights: column n holds q − z = 2 at ONE k_n under codes asymmetric
    in (m, k): y[m, n] = δw[n]·2·x̂[m, k_n].  A gather, bit for bit: a wrong scale_b constant changes it by a power of two; a swapped plane,
    lane half or scale byte moves it."""
    from dgq_amd import ops
    m, k = torch.arange(M)[:, None], torch.arange(K)[None, :]
    if hot == "weights":
        kn = (torch.arange(N) * 5 + 1) % K
        zw, wd = (1 + (5 * torch.arange(N)) % 13).float(), (2.0 ** ((torch.arange(N) % 3) - 1).double()).float()
        qw = zw.long()[:, None].repeat(1, K)
        qw[torch.arange(N), kn] += 2
        s = (7 * m + 11 * k + (m * k) % 5) % 255 - 127
    else:
        qw, zw, wd = _asym_weight(N, K)
        s = torch.where(k == (m * 7 + 3) % K, hot, 0)
    ab = ops.MxActBinding(_packed_weight(ops, dev, qw, zw, wd), "mxint8")
    E = torch.randint(-6, 7, (M, K // 32), generator=torch.Generator().manual_seed(M + K))
    q = tuple(t.to(dev) for t in planes(s, E, ab.Kp // 32))
    got = ops.gemm_mxint8(q, (M, 1, 1, K, 1, 1, 1, 0), ab, torch.float32).cpu().double()
    xhat = s.double() * (2.0 ** (E.double() - 6.0)).repeat_interleave(32, dim=1)
    want = xhat @ (wd[:, None].double() * (qw.double() - zw[:, None].double())).t()       # one non-zero term per element: exact
    assert torch.equal(got, want), (got != want).nonzero()[:4].tolist()


def test_bad_arguments_are_refused(dev):
    from dgq_amd import ops
    ab = ops.MxActBinding(_packed_weight(ops, dev, *_asym_weight(24, 64)), "mxint8")
    geom = (8, 1, 1, 64, 1, 1, 1, 0)
    q = ops.quant_act_mxint8(torch.randn(8, 64, device=dev), geom, lds=ab.Kp // 32)
    shifted = torch.empty(q[0].numel() + 8, dtype=torch.uint8, device=dev)[8:].view(q[0].shape)
    act, conv = ops._lib.GemmExtra(), ops._lib.GemmExtra()
    act.res_div, act.act, conv.res_div, conv.conv = 1, 256, 1, 256         # (non-null pointer values: refused before anything reads them)
    for bad, kw in (((shifted, q[1]), {}), ((q[0], q[1][:, :1]), {}), (q, dict(extra=act)), (q, dict(extra=conv))):
        with pytest.raises(RuntimeError, match=r"dgq_gemm_mxint8 failed \(-1\)"):      # DGQ_EINVAL: alignment, lds < C/32, extras
            ops.gemm_mxint8(bad, geom, ab, torch.float32, **kw)
    with pytest.raises(RuntimeError, match=r"dgq_quant_act_mxint8 failed \(-1\)"):     # C % 32
        ops.quant_act_mxint8(torch.randn(8, 48, device=dev), (8, 1, 1, 48, 1, 1, 1, 0))


CONV = lambda stride=1, **kw: lr.conv_case(2, 32, 9, 9, stride, 24, **kw)       # K = 288: 9 chunks, an odd pair and a ragged tile
EXACT_CASES = [lr.linear_case(37, 320, 24), CONV(), CONV(2), CONV(upsample=True), CONV(k=1)]


def _binding(ops, case, d, dev, w="w"):
    K, taps = lr.geometry(case)[6:]
    return ops.MxActBinding(ops.PackedWeight(d[w].to(dev), d["wdelta"].to(dev), d["wzp"].to(dev), None, d["bias"].to(dev), 4, K // taps, taps), "mxint8")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=gs.ids_dtype)
@pytest.mark.parametrize("case", EXACT_CASES, ids=lambda c: c["name"])
def test_exact_layers_equal_the_reference(case, dtype, dev):
    """layer_reference's integer weights, bias and residual (power-of-two δw) under x′ = s·2^(E−6), integer |s| <= 64 with one 64 per
    block (amax = 2^E, E in −3 .. 0: x̂ = x′, bf16-representable).  Every term is a multiple of u = min(2^-9·δw, 1) and their magnitudes sum
    to at most (15·K + 16)·2^9·u < 2^22·u at K <= 320: every fp32 step is exact in any order, and y EQUALS the float64 layer (with the
    residual in fp32; a bf16 output is the result without residual rounded once)."""
    from dgq_amd import ops
    d = lr._build_exact(case, "perM", 8, 4, lr.PROFILES[0])
    g = torch.Generator().manual_seed(lr._seed("planted-mxint8", case["name"]))
    R, C = mx.input_rows(case, d["x"]).shape
    s, E = torch.randint(-64, 65, (R, C // 32, 32), generator=g), torch.randint(-3, 1, (R, C // 32, 1), generator=g)
    s[:, :, 0] = 64
    x = mx.rows_to_input(case, (s.double() * 2.0 ** (E.double() - 6.0)).float().reshape(R, C), d["x"]).contiguous()
    res = d["residual"] if dtype == torch.float32 else None
    y_ref = mx.layer_float64(case, x.double(), d["qw"], d["wzp"], d["wdelta"], d["bias"], res)
    y = routes.run_layer(ops, case, _binding(ops, case, d, dev), x.to(dev, dtype), res.to(dev) if res is not None else None)
    assert y.dtype == dtype and torch.equal(y.cpu(), y_ref.float().to(dtype)), (y.cpu().double() != y_ref).nonzero()[:4].tolist()


def test_groupnorm_partials(dev, monkeypatch):
    """the partials the epilogue (the family's gemm_store_tile) leaves, by the metric and tolerance of test_gpu_groupnorm_stats.py"""
    from dgq_amd import ops, synth
    B, C, H, N, G = 2, 64, 8, 64, 8
    w = torch.randn(N, C, 3, 3, generator=torch.Generator().manual_seed(11)) * 0.05
    wd, wz = synth.channel_minmax(w, 4)
    ab = ops.MxActBinding(ops.PackedWeight(w.to(dev), wd.to(dev), wz.to(dev), None, gs.chan_bias(N, G, 11).to(dev), 4, C, 9), "mxint8")
    spy = gs.spied(ops, monkeypatch)
    for kind in gs.RES_KINDS:
        y = ops.quant_conv2d(gs.image(B, C, H, H, torch.float32, dev, 12), ab, 3, 3, 1, 1, residual=gs.residual(kind, B, H, H, N, G, torch.float32, dev), gn_out=True)
        assert [c["name"] for c in spy.take()].count("dgq_gemm_mxint8") == 1
        gs.check_partials(ops, dev, kind, "mxint8 3x3 %s" % kind, y, G)


@pytest.mark.parametrize("data", ["randn", "outlier"])
@pytest.mark.parametrize("case", EXACT_CASES[:2], ids=lambda c: c["name"])
def test_real_layers_inside_the_bound(case, data, dev, capsys):
    """per element |y − y64| <= 2^-24·|y64| + C_SUM·2K·2^-24·T: y64 the float64 sum over the KERNEL's own codes (asserted to be the
    statement's, bit for bit), T = |bias| + δw·Σ (16|h| + l)·2^(E−6)·|q − z| the magnitudes of both planes' terms"""
    from dgq_amd import ops
    d = lr.real_case(case, "perM", 8, 4)
    x = d["x"]
    if data == "outlier":
        x = mx.rows_to_input(case, mx.outlier_rows(mx.input_rows(case, x)), x).contiguous()
    ab = _binding(ops, case, d, dev, "w_raw")
    B, H, W, Ho, Wo, M, K, taps = lr.geometry(case)
    y = routes.run_layer(ops, case, ab, x.to(dev), None).cpu().double()
    lin = case["kind"] == "linear"
    xs = x.to(dev).reshape(M, K) if lin else x.to(dev).contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
    got = ops.quant_act_mxint8(xs, (M, 1, 1, K, 1, 1, 1, 0) if lin else (B, H, W, K // taps, 3, 3, 1, 1))
    s, unit, _ = check_quantiser(got, mx.input_rows(case, x), K // taps // 32)
    qw, zw, wd = ab.pw.codes.cpu().long(), ab.pw.zp_true.cpu(), ab.pw.alpha.cpu()
    y64 = mx.layer_float64(case, mx.rows_to_input(case, s.double() * unit, x), qw, zw, wd, d["bias"])
    T = mx.term_magnitudes(case, mx.rows_to_input(case, (16.0 * (s >> 4).abs() + (s & 15)).double() * unit, x), qw, zw, wd, d["bias"])
    err, unit_sum = (y - y64).abs(), 2 * K * 2.0 ** -24 * T
    with capsys.disabled():
        print("\nREAL-TIME MXINT8 %s %s: worst |y - y64| / (2K 2^-24 T) = %.4g; rel-L2 %.3g" % (case["name"], data, float((err / unit_sum).max()), rel_l2(y, y64)))
    assert bool((err <= 2.0 ** -24 * y64.abs() + C_SUM * unit_sum).all())


def _quant_layer(dev, lin, fmt, wbits=4):
    from dgq_amd.quant import QuantLayer, Scaler
    aq = {"bits": 6 if fmt == "mxfp6" else 8, "channel_wise": False, "scaler": Scaler.MINMAX, "leaf_param": True, "real_time": True}
    if fmt != "row":
        aq.update(real_time_block=32, real_time_format=fmt)
    layer = QuantLayer(lin, {"bits": wbits, "channel_wise": True, "scaler": Scaler.MINMAX}, aq).to(dev)
    layer.set_quant_state(True, True)
    return layer


@pytest.mark.parametrize("M,K,N", [(64, 768, 320), (64, 320, 64)])
def test_quant_layer_outlier_conditions(M, K, N, dev):
    """the conditions of the CPU test through a real QuantLayer: at most 0.75 x the int8 row mode's error and half of MXFP6's"""
    from dgq_amd import ops
    c = rb.outlier_case(M, K, N, 8)
    errs = {}
    for fmt in ("row", "mxfp6", "mxint8"):
        lin = torch.nn.Linear(K, N, bias=False)
        lin.weight.data.copy_(c["w_raw"])
        layer = _quant_layer(dev, lin, fmt)
        with torch.no_grad():
            y = layer(c["x"].to(dev))
        ab = layer._bindings["real_time"]
        assert isinstance(ab, ops.MxActBinding) and ab.fmt == fmt if fmt != "row" else isinstance(ab, ops.DynamicActBinding)
        errs[fmt] = rel_l2(y.cpu(), c["x"].double() @ layer.dequantized_weight(torch.float32).double().cpu().t())
    assert errs["mxint8"] <= 0.75 * errs["row"] and errs["mxint8"] <= 0.5 * errs["mxfp6"], errs


@pytest.mark.parametrize("K,wbits", [(64, 8), (48, 4)], ids=["W8", "C48"])
def test_ineligible_layers_run_as_the_int8_block_mode(K, wbits, dev):
    g = torch.Generator().manual_seed(K)
    lin, x = torch.nn.Linear(K, 40), (torch.randn(37, K, generator=g) * 1.3 + 0.2).to(dev)
    with torch.no_grad():
        ya, yb = (_quant_layer(dev, lin, fmt, wbits)(x) for fmt in ("mxint8", "int"))
    assert torch.equal(ya, yb)


def test_model_graph_replay_bindings_and_cli(tmp_path, rt_inputs, dev):
    import types
    from dgq_amd import inference_qmodel as cli, ops, synth
    from dgq_amd.diffusers_rewrite import UNet2DConditionModel
    from dgq_amd.quant import get_qmodel, Scaler
    from dgq_amd.runtime import quant_params
    path, out = str(tmp_path / "wonly.pth"), str(tmp_path / "lat_{rank}.pt")
    synth.write_cali_ckpt(path, "tiny", 4, 8, 1, num_slots=1, seed=0, batch=2, res=16, start_peak=True, with_act=False)
    unet = UNet2DConditionModel("tiny")
    unet.load_state_dict(synth.state_dict_from_ckpt(path))
    wq, aq, sm = quant_params(Scaler, 4, 8, True, True, True, True)
    aq["real_time"], aq["real_time_block"], aq["real_time_format"] = True, 32, "mxint8"
    qnn = get_qmodel("tiny", types.SimpleNamespace(unet=unet), path, wq, True, aq, sm, False, 25, False, device=dev).float().to(dev)
    qnn.disable_out_quantization()
    x, ctx = rt_inputs
    with torch.no_grad():
        y_e = qnn(x, torch.tensor(999), ctx)[0].clone()
        qnn.enable_graphs(True)
        y_g = [qnn(x, torch.tensor(999), ctx)[0].clone() for _ in range(3)]
        qnn.enable_graphs(False)
    assert torch.isfinite(y_e).all() and all(torch.equal(y, y_e) for y in y_g), "graph replay differs from the eager run"
    for name, layer in rta._inner_layers(qnn).items():      # every quantised layer of ``tiny`` is W4 with C % 32 == 0
        ab = layer._bindings["real_time"]
        assert isinstance(ab, ops.MxActBinding) and ab.fmt == "mxint8" and ab.wpacked is layer._pw._mx6[0], name
    attn_side = [m for n, m in qnn.model.named_modules() if n.rsplit(".", 1)[-1] in ("aqtizer_q", "aqtizer_k", "aqtizer_v")]
    assert attn_side and all(m.real_time and m.real_time_format == "int" for m in attn_side)
    cli.main(["--model_type", "tiny", "--use_aq", "--aq", "8", "--aq_real_time", "--aq_real_time_block", "32", "--aq_real_time_format", "mxint8",
              "--t2i_log_quant", "--t2i_real_time", "--num_inference_steps", "2", "--out", out])
    lat = torch.load(out.format(rank=0))
    assert sorted(lat) == [0, 1] and all(torch.isfinite(v).all() for v in lat.values())
