"""Host side of the real-time MXFP6 activation mode (no GPU): the statement ``quant_layer.mx6_block`` against the independent float64
restatement of tests/mxfp6_ref.py on random data and on the edge blocks, the exactness of W4 weights in E2M3, the operand packing, the
accuracy condition that motivates the mode, the quantizer's constructor, the CLI flag and the choice of binding per layer."""
import pytest
import torch

from tests import layer_reference as lr
from tests import mxfp6_ref as mx
from tests import realtime_block_ref as rb
from dgq_amd.quant import quant_layer
from dgq_amd.quant.quant_layer import Scaler, UniformAffineQuantizer


def _same(rows):
    codes, scale, xhat = quant_layer.mx6_block(rows)
    rc, rs, rx = mx.mx6_reference(rows)
    assert codes.dtype == torch.uint8 and scale.dtype == torch.uint8 and xhat.dtype == torch.float32
    assert torch.equal(scale, rs), (scale != rs).nonzero()[:4].tolist()
    assert torch.equal(codes, rc), (codes != rc).nonzero()[:4].tolist()
    assert torch.equal(xhat.double(), rx)
    assert torch.equal(mx.decode(codes, scale), rx)
    return codes, scale, xhat


def test_statement_equals_restatement_on_randn():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(200, 96, generator=g) * torch.logspace(-4, 4, 200).view(200, 1) + 0.2
    codes, scale, xhat = _same(x)
    # the rule itself: amax lands in [4, 8)·2^E, so the error of an element is at most half the widest step, 0.25·2^E — or, saturating
    # from below 8 to 7.5, less than 0.5·2^E
    E = scale.double() - 127.0
    amax = x.view(200, 3, 32).abs().amax(dim=2).double()
    assert bool((amax >= 4.0 * 2.0 ** E).all()) and bool((amax < 8.0 * 2.0 ** E).all())
    assert bool(((x.double() - xhat.double()).abs().view(200, 3, 32) < 0.5 * (2.0 ** E)[:, :, None]).all())


def test_statement_equals_restatement_on_edge_blocks():
    rows = mx.edge_blocks()
    codes, scale, xhat = _same(rows)
    assert int(scale[0, 0]) == 0 and int(codes[0, :32].max()) == 0                  # all zeros: E = −127, every code +0
    assert int(scale[-1, 0]) == 0 and int(codes[-1, :32].max()) == 0                # all −0 likewise
    assert int(scale[1, 0]) == 127 and int(codes[1, 3]) == 24                       # amax = 4.0: E = 0, code of 4.0
    for r in (3, 4, 5, 6):                                                          # 7.6, 7.75, 7.8, 7.99 (scaled): both signs saturate at 7.5
        assert int(codes[r, 9]) == 31 and int(codes[r, 10]) == 63, r
    # ties at every step size, to the even code, both ways (the same codes at every scale)
    want = [0, 2, 8, 8, 10, 16, 16, 18, 24, 24, 26, 30, 30]
    for r in (7, 8, 9):
        assert codes[r, :13].tolist() == want and codes[r, 13:25].tolist() == [c + 32 if c else 0 for c in want[:12]], r
    assert int(scale[7, 0]) == 127 and int(scale[8, 0]) == 134 and int(scale[9, 0]) == 118
    assert codes[10, :3].tolist() == [0, 0, 0]                                      # −0, +0 and a negative value that rounds to zero: +0
    assert int(scale[11, 0]) == 0 and codes[11, 4:8].tolist() == [1, 0, 0, 0]       # amax = 2^-130: E = −127; the tie at half a step goes to 0
    assert int(scale[12, 0]) == 98 + 127 and int(codes[12, 11]) == 24
    assert int(scale[14, 0]) == 130 and int(codes[14, 13]) == 31                    # 60 = 7.5·2^3


def test_w4_weights_are_exact_in_e2m3():
    grid = set(mx.e2m3_values().tolist())
    assert len(grid) == 32 and set(quant_layer.E2M3_MAGNITUDES) == grid
    assert all(abs(d) / 2.0 in grid for d in range(-15, 16))
    assert 15.5 / 2.0 not in grid and 16 / 2.0 not in grid
    # ... and the eligibility rule is check_mfma16's
    from dgq_amd.ops import PackedWeight
    codes = torch.randint(0, 16, (6, 40))
    assert PackedWeight.check_mfma16(codes, torch.tensor([0.0, 3.0, 8.0, 15.0, 7.0, 1.0]), 4)
    assert not PackedWeight.check_mfma16(codes, torch.tensor([0.0, 3.5, 8.0, 15.0, 7.0, 1.0]), 4)
    codes[2, 5] = 15
    assert not PackedWeight.check_mfma16(codes, torch.tensor([0.0, 3.0, -1.0, 15.0, 7.0, 1.0]), 4)


def test_packing_round_trips():
    g = torch.Generator().manual_seed(3)
    codes = torch.randint(0, 64, (7, 96), generator=g).to(torch.uint8)
    packed = quant_layer.mx6_pack(codes)
    assert packed.shape == (7, 3, 24) and packed.dtype == torch.uint8
    assert torch.equal(quant_layer.mx6_unpack(packed), codes)
    # element j at bits 6j .. 6j + 5 of the block's 192-bit little-endian string
    for r, b in ((0, 0), (6, 2)):
        big = int.from_bytes(bytes(packed[r, b].tolist()), "little")
        assert [(big >> (6 * j)) & 63 for j in range(32)] == codes[r, 32 * b:32 * b + 32].tolist()


@pytest.mark.parametrize("M,K,N", [(64, 768, 320), (64, 320, 64)])
def test_accuracy_condition_on_outliers(M, K, N):
    """one 60-outlier per row of x = randn·1.3 + 0.2 at A6: the MXFP6 layer error is at most HALF the int6 row mode's (measured when the
    mode was proposed: 1/4.2 and 1/3.0) and at most 1.25x the int6 block mode's (measured 1.08x and 1.04x)"""
    c = rb.outlier_case(M, K, N, 6)
    e_row, e_blk = rb.outlier_errors(c)
    e_mx = mx.outlier_error_mx6(c)
    print("outlier %dx%d->%d A6: row %.3g block %.3g mxfp6 %.3g (row/mx %.2fx, mx/block %.2fx)" % (M, K, N, e_row, e_blk, e_mx, e_row / e_mx, e_mx / e_blk))
    assert e_mx <= 0.5 * e_row, (e_row, e_mx)
    assert e_mx <= 1.25 * e_blk, (e_blk, e_mx)


@pytest.mark.parametrize("case", [lr.linear_case(37, 320, 24), lr.conv_case(2, 64, 8, 8, 1, 64, upsample=True)], ids=lambda c: c["name"])
def test_planted_data_is_exact(case):
    """the exact GPU recipe: the quantiser reproduces the planted E and x̂ = x (asserted inside), and the margin holds"""
    d = mx.planted_mx6(case)
    y, xhat = mx.mx6_layer_reference(case, d["x"], d["qw"], d["wzp"], d["wdelta"], d["bias"], d["residual"])
    assert torch.equal(xhat, d["x"].double())
    assert mx.mx6_exact_margin(case, xhat, d["qw"], d["wzp"], d["wdelta"], d["bias"], d["residual"]) < 1.0
    assert set(d["E"].unique().tolist()) == set(mx.PLANT_E)
    assert torch.equal(y, y.float().double())              # the float64 result is an fp32 number


def test_quantizer_constructor_and_repr():
    q = UniformAffineQuantizer(bits=6, scaler=Scaler.MINMAX, leaf_param=True, real_time=True, real_time_block=32, real_time_format="mxfp6")
    assert q.real_time and q.real_time_block == 32 and q.real_time_format == "mxfp6" and q.init and q.delta is None
    assert "real_time_format=mxfp6" in q.extra_repr()
    plain = UniformAffineQuantizer(bits=6, real_time=True, real_time_block=32)
    assert plain.real_time_format == "int" and "real_time_format" not in plain.extra_repr()
    assert UniformAffineQuantizer(bits=8).real_time_format == "int"
    for bad in (dict(bits=6, real_time=True, real_time_block=32, real_time_format="mxfp8"),
                dict(bits=6, real_time=True, real_time_block=32, real_time_format="fp6"),
                dict(bits=8, real_time=True, real_time_block=32, real_time_format="mxfp6"),
                dict(bits=6, real_time=True, real_time_format="mxfp6"),
                dict(bits=6, real_time_format="mxfp6")):
        with pytest.raises(ValueError):
            UniformAffineQuantizer(**bad)


def test_cli_parser_and_flag_rules():
    from dgq_amd import inference_qmodel as cli
    base = ["--model_type", "tiny", "--use_aq", "--aq_real_time", "--aq_real_time_block", "32"]
    opt = cli.parse_args(base + ["--aq", "6", "--aq_real_time_format", "mxfp6"])
    assert opt.aq_real_time_format == "mxfp6"
    assert cli.parse_args(base).aq_real_time_format == "int"
    for bad in (base + ["--aq_real_time_format", "mxfp6"],                                                      # 8 activation bits
                ["--model_type", "tiny", "--use_aq", "--aq_real_time", "--aq", "6", "--aq_real_time_format", "mxfp6"],     # no block
                ["--model_type", "tiny", "--use_aq", "--aq", "6", "--aq_real_time_format", "mxfp6"],                        # not real-time
                ["--model_type", "tiny", "--aq", "6", "--aq_real_time_format", "mxfp6"]):
        with pytest.raises(SystemExit) as e:
            cli.main(bad)
        assert "mxfp6" in str(e.value), bad
    with pytest.raises(SystemExit):
        cli.parse_args(base + ["--aq", "6", "--aq_real_time_format", "mxfp8"])


class _StubWeight:
    def __init__(self, bits, eligible):
        self.bits, self.mx6_eligible = bits, eligible


def test_model_chooses_the_binding_per_layer(tmp_path, monkeypatch):
    """arch ``tiny`` from a weight-only checkpoint with real_time_format="mxfp6": aq_params_w and the attention-side quantizers do not
    take the format, the loader treats the mode as the row mode (act_* ignored, time_aware_aqtizer refused), and every layer picks its
    binding: MxActBinding where the weight is eligible and C % 32 == 0, the block binding for an ineligible (W8) weight, the row binding
    where C % 32 != 0.  (The bindings themselves need the GPU: stubs record the choice.)"""
    from dgq_amd import ops, synth
    from dgq_amd.diffusers_rewrite import UNet2DConditionModel
    from dgq_amd.quant import QuantLayer, QuantModel
    from dgq_amd.quant.calibration import load_cali_model

    def qnn_():
        unet = UNet2DConditionModel("tiny")
        synth.load_synth_weights(unet, "tiny", 0)
        aq = {"bits": 6, "channel_wise": False, "scaler": Scaler.MINMAX, "leaf_param": True, "real_time": True, "real_time_block": 32,
              "real_time_format": "mxfp6"}
        sm = {"softmax_a_bit": 8, "t2i_log_quant": True, "t2i_real_time": True, "t2i_start_peak": False, "log_max_1": False}
        return QuantModel(model=unet, wq_params={"bits": 4, "channel_wise": True, "scaler": Scaler.MINMAX}, aq_params=aq, softmax_aq_params=sm).eval()
    full = str(tmp_path / "full.pth")
    synth.write_cali_ckpt(full, "tiny", 4, 6, 4, num_slots=2, seed=0, batch=2, res=16, with_act=True)
    qnn = qnn_()
    load_cali_model(qnn, init_data=None, use_aq=True, path=full, use_group=True, init_forward=False)
    qnn.disable_out_quantization()
    inner = [m for m in qnn.model.modules() if isinstance(m, QuantLayer) and not m.disable_aq]
    assert inner and all(m.aqtizer.real_time and m.aqtizer.real_time_format == "mxfp6" and not m._act_tables for m in inner)
    attn_side = [m for n, m in qnn.model.named_modules() if n.rsplit(".", 1)[-1] in ("aqtizer_q", "aqtizer_k", "aqtizer_v")]
    assert attn_side and all(m.real_time and m.real_time_format == "int" for m in attn_side)
    with pytest.raises(ValueError):
        load_cali_model(qnn_(), init_data=None, use_aq=True, path=full, time_aware_aqtizer=True, num_inference_steps=2, init_forward=False)
    # the choice of binding
    made = []
    monkeypatch.setattr(ops, "MxActBinding", lambda pw: made.append("mx") or "mx")
    monkeypatch.setattr(ops, "BlockActBinding", lambda pw, bits: made.append(("block", bits)) or "block")
    monkeypatch.setattr(ops, "DynamicActBinding", lambda pw, bits: made.append(("row", bits)) or "row")
    # (every quantised layer of ``tiny`` has C % 32 == 0 and a W4 weight: a Linear layer of 48 input channels under the same parameters
    # joins them, and one layer is given a W8 weight)
    inner.append(QuantLayer(torch.nn.Linear(48, 16), dict(inner[0].wq_params), dict(inner[0].aq_params)))
    whole = [m for m in inner if m.in_channels % 32 == 0]
    ragged = [m for m in inner if m.in_channels % 32 != 0]
    assert len(whole) > 100 and len(ragged) == 1
    w8 = whole[3]
    for m in inner:
        monkeypatch.setattr(m, "packed_weight", lambda m=m: _StubWeight(8 if m is w8 else 4, m is not w8))
        m._bindings.clear()
        got = m._binding()
        want = "row" if m.in_channels % 32 != 0 else ("block" if m is w8 else "mx")
        assert got == want, (m.in_channels, got, want)
    assert made.count("mx") == len(whole) - 1 and made.count(("block", 6)) == 1 and made.count(("row", 6)) == len(ragged)
