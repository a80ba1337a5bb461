"""Host side of W8 weights under the real-time MX activation formats (real_time_mx_w8=True; no GPU): the exact split of a centred W8
weight into two E2M3 planes, the accuracy of the statement on outlier rows, constructor and CLI rules, the choice of binding."""
import pytest
import torch

from tests import mxfp6_ref as mx
from tests import realtime_block_ref as rb
from dgq_amd.quant import quant_layer
from dgq_amd.quant.quant_layer import UniformAffineQuantizer

FORMATS = [("mxfp6", 6), ("mxint8", 8)]


def test_split_is_exact_for_every_difference():
    d = torch.arange(-255, 256)
    hi, lo = quant_layer.mxw8_split(d)
    grid = mx.e2m3_values()
    for p in (hi, lo):                                     # 6-bit codes; a zero magnitude is +0
        assert p.dtype == torch.uint8 and int(p.max()) < 64 and not bool(((p & 31) == 0)[p >= 32].any())
    h2, l2 = (grid[(p & 31).long()] * torch.where(p >= 32, -1.0, 1.0) for p in (hi, lo))
    assert torch.equal(32.0 * h2 + 2.0 * l2, d.double())   # d = 32·(±H/2) + 2·(±L/2) with both on the grid


@pytest.mark.parametrize("fmt,bits", FORMATS)
def test_accuracy_on_outliers_against_w8_int_rows(fmt, bits):
    """one 60-outlier per row at 64x768 -> 320, W8: the layer error under the MX statement is at most 0.75 x the int row mode's at the
    same bits — met with room (computed: 0.0269 / 0.114 at A6, 0.0120 / 0.0285 at A8).  The int BLOCK mode, the route these layers take
    with the flag off, is the more accurate one on this data (0.0249, 0.0062): recorded, not pinned."""
    c = rb.outlier_case(64, 768, 320, bits, wbits=8)
    xhat = (quant_layer.mx6_block if fmt == "mxfp6" else quant_layer.mxint8_block)(c["x"][0])[2]
    y = xhat.double() @ c["w"].double().t()
    e_mx, (e_row, e_blk) = float((y - c["y64"]).norm() / c["y64"].norm()), rb.outlier_errors(c)
    print("outlier 64x768->320 W8A%d: int rows %.4g int blocks %.4g %s %.4g" % (bits, e_row, e_blk, fmt, e_mx))
    assert e_mx <= 0.75 * e_row, (e_row, e_mx)


def test_constructor_and_cli_rules():
    from dgq_amd import inference_qmodel as cli
    for fmt, bits in FORMATS:
        q = UniformAffineQuantizer(bits=bits, real_time=True, real_time_block=32, real_time_format=fmt, real_time_mx_w8=True)
        assert q.real_time_mx_w8 and "real_time_mx_w8=True" in q.extra_repr()
        off = UniformAffineQuantizer(bits=bits, real_time=True, real_time_block=32, real_time_format=fmt)
        assert not off.real_time_mx_w8 and "mx_w8" not in off.extra_repr()
    for bad in (dict(bits=8, real_time=True, real_time_block=32), dict(bits=8, real_time=True), dict(bits=8)):
        with pytest.raises(ValueError):
            UniformAffineQuantizer(real_time_mx_w8=True, **bad)
    base = ["--model_type", "tiny", "--use_aq", "--aq_real_time", "--aq_real_time_block", "32"]
    assert cli.parse_args(base + ["--aq_real_time_format", "mxint8", "--aq_real_time_mx_w8"]).aq_real_time_mx_w8
    assert not cli.parse_args(base).aq_real_time_mx_w8
    for bad in (base + ["--aq_real_time_mx_w8"], ["--model_type", "tiny", "--aq_real_time_mx_w8"]):      # int blocks; no quantizers
        with pytest.raises(SystemExit) as e:
            cli.main(bad)
        assert "--aq_real_time_mx_w8" in str(e.value), bad


class _StubWeight:
    """flag off: only ``bits`` and ``mx6_eligible`` exist (as in test_realtime_mxfp6_cpu.py); flag on: ``mxw8_eligible`` too"""
    def __init__(self, bits, mx6, mxw8=None):
        self.bits, self.mx6_eligible = bits, mx6
        if mxw8 is not None:
            self.mxw8_eligible = mxw8


@pytest.mark.parametrize("fmt,bits", FORMATS)
def test_binding_choice(fmt, bits, monkeypatch):
    from dgq_amd import ops
    from dgq_amd.quant import QuantLayer, Scaler
    monkeypatch.setattr(ops, "MxActBinding", lambda pw, f="mxfp6", **kw: ("mx", f, kw.get("w_bits", 4)))
    monkeypatch.setattr(ops, "BlockActBinding", lambda pw, b: ("block", b))
    monkeypatch.setattr(ops, "DynamicActBinding", lambda pw, b: ("row", b))

    def choice(K, flag, pw):
        aq = dict(bits=bits, channel_wise=False, scaler=Scaler.MINMAX, leaf_param=True, real_time=True, real_time_block=32,
                  real_time_format=fmt, real_time_mx_w8=flag)
        layer = QuantLayer(torch.nn.Linear(K, 16), dict(bits=pw.bits, channel_wise=True, scaler=Scaler.MINMAX), aq)
        monkeypatch.setattr(layer, "packed_weight", lambda: pw)
        return layer._binding()
    assert choice(64, False, _StubWeight(8, False)) == ("block", bits)                   # flag off: the parent's route, no new attribute
    assert choice(64, True, _StubWeight(8, False, True)) == ("mx", fmt, 8)
    assert choice(64, True, _StubWeight(8, False, False)) == ("block", bits)             # fractional zero points
    assert choice(48, True, _StubWeight(8, False, True)) == ("row", bits)                # C % 32 != 0
    assert choice(64, True, _StubWeight(4, True))[:2] == ("mx", fmt)                     # W4 layers keep their one-plane image
    assert choice(64, True, _StubWeight(4, True))[2] == 4
