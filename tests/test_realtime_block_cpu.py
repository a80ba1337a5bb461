"""Host side of the real-time BLOCK activation quantiser (no GPU): the block statement the kernel reproduces, the layer formula of
dgq_gemm_blockq against the float64 reference under the expanded tables, the outlier condition that motivates the mode, the quantizer's
constructor and the CLI flag."""
import pytest
import torch

from tests import layer_reference as lr
from tests import realtime_block_ref as rb
from dgq_amd.quant import quant_layer
from dgq_amd.quant.quant_layer import Scaler, UniformAffineQuantizer


def _rows(n=120, k=96, seed=5):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, k, generator=g) * torch.logspace(-3, 3, n).view(n, 1)
    x[0:10, 0:32] = x[0:10, 0:32].abs() + 1e-3            # all-positive blocks
    x[10:20, 32:64] = -x[10:20, 32:64].abs() - 1e-3       # all-negative blocks
    x[20:30, 64:96] = 0.0                                 # all-zero blocks: the 1e-8 clamp
    x[30, 40] = 1e4                                       # an outlier: its own block only
    return x


@pytest.mark.parametrize("bits", [8, 6])
def test_block_statement_equals_per_block_minmax(bits):
    """``block_minmax`` (what dgq_quant_act_block computes) == the scalar ``minmax`` of every block, δ and z, bit for bit"""
    x = _rows()
    d, z = rb.block_tables(x, bits)
    assert d.shape == (x.shape[0], 3)
    for r in range(x.shape[0]):
        for c in range(3):
            dr, zr = quant_layer.minmax(x[r, 32 * c:32 * c + 32], level=2 ** bits)
            assert torch.equal(d[r, c], dr) and torch.equal(z[r, c], zr), (r, c, float(d[r, c]), float(dr), float(z[r, c]), float(zr))
    assert float(z.min()) >= 0 and float(z.max()) <= 2 ** bits - 1
    assert torch.equal(d[20:30, 2], torch.full((10,), 1e-8)) and float(z[20:30, 2].abs().max()) == 0.0
    assert float(z[0:10, 0].max()) == 0.0 and float(z[10:20, 1].min()) == 2 ** bits - 1
    # the outlier sets the step of ITS block; the row's other blocks keep theirs
    assert float(d[30, 1]) >= 1e4 / (2 ** bits - 1) and float(d[30, 0]) < 0.1 * float(d[30, 1]) and float(d[30, 2]) < 0.1 * float(d[30, 1])
    # an all-zero block: code 0, dequantised to exactly 0
    q = rb.block_codes(x, d, z, bits)
    assert float(q[20:30, 64:96].abs().max()) == 0.0


FORMULA_CASES = [lr.linear_case(37, 320, 64), lr.conv_case(2, 32, 9, 9, 1, 24)]


@pytest.mark.parametrize("case", FORMULA_CASES, ids=lambda c: c["name"])
def test_layer_formula_equals_reference(case):
    """Σ_c (δ·P + β·Vc) − zw·R, in float64 from codes, block tables and Vc, == reference_layer under the tables expanded to one (δ, z) per
    element.  Real-valued data: the two differ by the fp32 roundings of δ·(q − z) in the reference and of β in the formula, one each
    per element (2^-24 relative) — 1e-6 rel-L2 is an order of magnitude above that and three below any indexing mistake."""
    from dgq_amd import synth
    d = lr.real_case(case, "perM")
    y_ref, q, de, ze, inside = rb.block_reference(case, dict(d, residual=None))
    assert inside is None or float(inside.min()) == 0.0   # taps outside the image exist in the conv case
    N = case["N"]
    qw = torch.clamp(torch.round(d["w_raw"].reshape(N, -1) / d["wdelta"].reshape(N, 1)) + d["wzp"].reshape(N, 1), 0, 15)
    y = rb.formula_float64(case, q, de, ze, inside, qw, d["wzp"].reshape(-1), d["wdelta"].reshape(-1), d["bias"], 8)
    y = rb.rows_to_output(y, case, y_ref)
    err = float((y - y_ref).norm() / y_ref.norm())
    assert err <= 1e-6, err


@pytest.mark.parametrize("M,K,N,abits", [(64, 768, 320, 8), (64, 768, 320, 6), (64, 320, 64, 8)])
def test_outlier_condition(M, K, N, abits):
    """one 60-outlier per row of x = randn·1.3 + 0.2: the block mode's layer error is at most HALF the row mode's (measured when the mode
    was proposed: 4.6x, 4.6x, 3.1x lower).  A condition on the arithmetic, not a measurement."""
    e_row, e_blk = rb.outlier_errors(rb.outlier_case(M, K, N, abits))
    print("outlier %dx%d->%d A%d: row %.3g block %.3g (%.2fx)" % (M, K, N, abits, e_row, e_blk, e_row / e_blk))
    assert e_blk <= 0.5 * e_row, (e_row, e_blk)


@pytest.mark.parametrize("case", [lr.linear_case(37, 320, 24), lr.conv_case(2, 64, 8, 8, 1, 64, upsample=True)], ids=lambda c: c["name"])
def test_planted_blocks_are_exact(case):
    """the exact-integer GPU recipe: block_minmax returns the planted 2^e and z (asserted inside), the margin holds, and the formula
    EQUALS the reference"""
    d = rb.planted_exact(case, 8, 4)
    y, q, de, ze, inside = rb.block_reference(case, d)
    assert rb.block_exact_margin(case, d, q, de, ze, inside) < 1.0
    yf = rb.formula_float64(case, q, de, ze, inside, d["qw"], d["wzp"].reshape(-1), d["wdelta"].reshape(-1), d["bias"], 8)
    assert torch.equal(rb.rows_to_output(yf, case, y) + d["residual"].double(), y)


def test_real_time_block_quantizer_constructs():
    q = UniformAffineQuantizer(bits=6, scaler=Scaler.MINMAX, leaf_param=True, real_time=True, real_time_block=32)
    assert q.real_time and q.real_time_block == 32 and q.init and q.delta is None
    assert "real_time_block=32" in q.extra_repr()
    assert UniformAffineQuantizer(bits=8, real_time=True).real_time_block == 0
    assert "real_time_block" not in UniformAffineQuantizer(bits=8, real_time=True).extra_repr()
    for bad in (dict(real_time=True, real_time_block=16), dict(real_time=True, real_time_block=64), dict(real_time_block=32)):
        with pytest.raises(ValueError):
            UniformAffineQuantizer(**bad)


def test_model_builds_and_loads_with_block_params(tmp_path):
    """QuantModel accepts the option (aqtizer_w does not take it), and the loader treats the mode as the row mode: weight-only ckpt,
    act_* ignored, time_aware_aqtizer refused"""
    from dgq_amd import synth
    from dgq_amd.diffusers_rewrite import UNet2DConditionModel
    from dgq_amd.quant import QuantLayer, QuantModel
    from dgq_amd.quant.calibration import load_cali_model

    def qnn_():
        unet = UNet2DConditionModel("tiny")
        synth.load_synth_weights(unet, "tiny", 0)
        aq = {"bits": 8, "channel_wise": False, "scaler": Scaler.MINMAX, "leaf_param": True, "real_time": True, "real_time_block": 32}
        sm = {"softmax_a_bit": 8, "t2i_log_quant": True, "t2i_real_time": True, "t2i_start_peak": False, "log_max_1": False}
        return QuantModel(model=unet, wq_params={"bits": 4, "channel_wise": True, "scaler": Scaler.MINMAX}, aq_params=aq, softmax_aq_params=sm).eval()
    full = str(tmp_path / "full.pth")
    synth.write_cali_ckpt(full, "tiny", 4, 8, 4, num_slots=2, seed=0, batch=2, res=16, with_act=True)
    qnn = qnn_()
    load_cali_model(qnn, init_data=None, use_aq=True, path=full, use_group=True, init_forward=False)
    qnn.disable_out_quantization()
    inner = [m for m in qnn.model.modules() if isinstance(m, QuantLayer) and not m.disable_aq]
    assert inner and all(m.aqtizer.real_time and m.aqtizer.real_time_block == 32 and not m._act_tables for m in inner)
    with pytest.raises(ValueError):
        load_cali_model(qnn_(), init_data=None, use_aq=True, path=full, time_aware_aqtizer=True, num_inference_steps=2, init_forward=False)


def test_cli_parser_and_flag_rules():
    from dgq_amd import inference_qmodel as cli
    opt = cli.parse_args(["--model_type", "tiny", "--use_aq", "--aq_real_time", "--aq_real_time_block", "32"])
    assert opt.aq_real_time and opt.aq_real_time_block == 32
    assert cli.parse_args(["--use_aq", "--aq_real_time"]).aq_real_time_block == 0
    with pytest.raises(SystemExit) as e:
        cli.main(["--model_type", "tiny", "--use_aq", "--aq_real_time_block", "32"])
    assert "--aq_real_time" in str(e.value)
