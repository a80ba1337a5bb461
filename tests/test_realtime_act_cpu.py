"""Host side of the real-time per-row activation quantiser (no GPU): the vectorised row statement the kernel reproduces, the
quantizer's constructor, the loader rules and the CLI flag."""
import pytest
import torch

from dgq_amd import synth
from dgq_amd.quant import quant_layer
from dgq_amd.quant.quant_layer import Scaler, UniformAffineQuantizer


def _rows(n=500, k=48, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, k, generator=g) * torch.logspace(-3, 3, n).view(n, 1)
    x[0:40] = x[0:40].abs() + 1e-3                 # all-positive rows
    x[40:80] = -x[40:80].abs() - 1e-3              # all-negative rows
    x[80:90] = 0.0                                 # all-zero rows: the 1e-8 clamp
    x[90, 7] = 1e4
    return x


@pytest.mark.parametrize("bits", [8, 6])
def test_row_statement_equals_per_row_minmax(bits):
    """``row_minmax`` (what dgq_act_row_params computes) == the scalar ``minmax`` of every row, δ and z, bit for bit"""
    x = _rows()
    d, z = quant_layer.row_minmax(x.min(dim=1)[0], x.max(dim=1)[0], 2 ** bits)
    for r in range(x.shape[0]):
        dr, zr = quant_layer.minmax(x[r], level=2 ** bits)
        assert torch.equal(d[r], dr) and torch.equal(z[r], zr), (r, float(d[r]), float(dr), float(z[r]), float(zr))
    assert float(z.min()) >= 0 and float(z.max()) <= 2 ** bits - 1
    assert torch.equal(d[80:90], torch.full((10,), 1e-8)) and float(z[80:90].abs().max()) == 0.0


@pytest.mark.parametrize("b", [8, 6])
def test_planted_extremes_give_power_of_two_scales(b):
    """the exact-integer GPU recipe: a row holding −z·2^e and (2^b − 1 − z)·2^e (everything else inside) has δ = 2^e and that z"""
    n = 0
    for e in (-2, -1, 0, 1):
        for z in (2 ** (b - 1) - 8, 2 ** (b - 1) - 1, 2 ** (b - 1), 2 ** (b - 1) + 3, 2 ** (b - 1) + 8, 1, 2 ** b - 2, 0, 2 ** b - 1):
            row = torch.tensor([-z * 2.0 ** e, (2 ** b - 1 - z) * 2.0 ** e, 0.0])
            d, zz = quant_layer.minmax(row, level=2 ** b)
            assert float(d) == 2.0 ** e and float(zz) == float(z), (b, e, z, float(d), float(zz))
            n += 1
    assert n == 36


def test_real_time_quantizer_constructs():
    q = UniformAffineQuantizer(bits=6, scaler=Scaler.MINMAX, leaf_param=True, real_time=True)
    assert q.real_time and q.init and q.delta is None and q.bits == 6
    assert "real_time=True" in q.extra_repr()
    q.init_from(torch.randn(4, 8))                     # a no-op: nothing to initialise
    assert q.delta is None and q.zero_point is None
    assert "real_time" not in UniformAffineQuantizer(bits=8).extra_repr()
    assert not UniformAffineQuantizer(bits=8).real_time
    for bad in (dict(channel_wise=True), dict(always_zero=True), dict(scaler=Scaler.MSE)):
        with pytest.raises(ValueError):
            UniformAffineQuantizer(real_time=True, **bad)


def _tiny_qnn(real_time=True):
    from dgq_amd.diffusers_rewrite import UNet2DConditionModel
    from dgq_amd.quant import QuantModel
    unet = UNet2DConditionModel("tiny")
    synth.load_synth_weights(unet, "tiny", 0)
    wq = {"bits": 4, "channel_wise": True, "scaler": Scaler.MINMAX}
    aq = {"bits": 8, "channel_wise": False, "scaler": Scaler.MINMAX, "leaf_param": True}
    if real_time:
        aq["real_time"] = True
    sm = {"softmax_a_bit": 8, "t2i_log_quant": True, "t2i_real_time": True, "t2i_start_peak": False, "log_max_1": False}
    return QuantModel(model=unet, wq_params=wq, aq_params=aq, softmax_aq_params=sm).eval()


def test_loader_rules(tmp_path):
    from dgq_amd.quant import QuantLayer
    from dgq_amd.quant.calibration import load_cali_model
    from dgq_amd.quant.quant_layer_text import T2ILogQuantizer
    wonly, full = str(tmp_path / "wonly.pth"), str(tmp_path / "full.pth")
    synth.write_cali_ckpt(wonly, "tiny", 4, 8, 1, num_slots=1, seed=0, batch=2, res=16, with_act=False)
    synth.write_cali_ckpt(full, "tiny", 4, 8, 4, num_slots=2, seed=0, batch=2, res=16, with_act=True)
    for path in (wonly, full):                     # a checkpoint that carries act_* blocks loads fine: they are ignored
        qnn = _tiny_qnn()
        load_cali_model(qnn, init_data=None, use_aq=True, path=path, use_group=True, init_forward=False)
        qnn.disable_out_quantization()
        layers = [m for m in qnn.model.modules() if isinstance(m, QuantLayer)]
        inner = [m for m in layers if not m.disable_aq]
        assert inner and all(m.use_wq and m.use_aq and m.aqtizer.real_time and m._has_act_table() for m in inner)
        assert all(m.aqtizer.delta is None and not m._act_tables and not m.use_group_num for m in inner)
        assert qnn.time_aware is None
        for m in qnn.model.modules():              # the attention side: q / k / v real-time as well, aqtizer_w untouched
            if hasattr(m, "aqtizer_q"):
                assert m.aqtizer_q.real_time and m.aqtizer_k.real_time and m.aqtizer_v.real_time
                assert isinstance(m.aqtizer_w, T2ILogQuantizer) and m.aqtizer_w.real_time
    with pytest.raises(ValueError):
        load_cali_model(_tiny_qnn(), init_data=None, use_aq=True, path=full, time_aware_aqtizer=True, num_inference_steps=2,
                        init_forward=False)
    qnn = _tiny_qnn()                              # use_aq=False: the weight-only state, whatever aq_params say
    load_cali_model(qnn, init_data=None, use_aq=False, path=wonly, time_aware_aqtizer=True, init_forward=False)
    assert not any(m.use_aq for m in qnn.model.modules() if isinstance(m, QuantLayer))


def test_uniform_softmax_quantizer_stays_static(tmp_path):
    """aq_params' real_time is the LAYER-side flag: without t2i_log_quant the softmax quantizer is the always_zero uniform one"""
    from dgq_amd.diffusers_rewrite import UNet2DConditionModel
    from dgq_amd.quant import QuantModel
    unet = UNet2DConditionModel("tiny")
    aq = {"bits": 8, "channel_wise": False, "scaler": Scaler.MINMAX, "leaf_param": True, "real_time": True}
    sm = {"softmax_a_bit": 8, "t2i_log_quant": False, "t2i_real_time": False, "t2i_start_peak": False, "log_max_1": False}
    qnn = QuantModel(model=unet, wq_params={"bits": 4, "channel_wise": True, "scaler": Scaler.MINMAX}, aq_params=aq, softmax_aq_params=sm)
    ws = [m.aqtizer_w for m in qnn.model.modules() if hasattr(m, "aqtizer_w")]
    assert ws and all(isinstance(w, UniformAffineQuantizer) and w.always_zero and not w.real_time for w in ws)


def test_cli_parser_accepts_the_flag():
    from dgq_amd import inference_qmodel as cli
    opt = cli.parse_args(["--model_type", "tiny", "--use_aq", "--aq_real_time", "--t2i_log_quant", "--t2i_real_time"])
    assert opt.aq_real_time and opt.use_aq
    assert not cli.parse_args(["--use_aq"]).aq_real_time
