"""Host side of the real-time MXINT8 activation mode (no GPU): ``quant_layer.mxint8_block`` against the float64 restatement of
tests/mxint8_ref.py, the exact split of a code into two E2M3 terms, the accuracy condition of the mode, constructor and CLI rules."""
import pytest
import torch

from tests import mxint8_ref as mi
from tests import mxfp6_ref as mx
from tests import realtime_block_ref as rb
from dgq_amd.quant import quant_layer
from dgq_amd.quant.quant_layer import UniformAffineQuantizer


@pytest.mark.parametrize("data", ["randn", "edge"])
def test_statement_equals_restatement(data):
    g = torch.Generator().manual_seed(11)
    rows = mi.edge_blocks() if data == "edge" else torch.randn(200, 96, generator=g) * torch.logspace(-4, 4, 200).view(200, 1) + 0.2
    codes, scale, xhat = quant_layer.mxint8_block(rows)
    rs, rscale, rx = mi.mxint8_reference(rows)
    assert codes.dtype == torch.int8 and scale.dtype == torch.uint8 and xhat.dtype == torch.float32
    assert torch.equal(scale, rscale) and torch.equal(codes.long(), rs) and torch.equal(xhat.double(), rx)
    if data == "edge":
        c = codes[:, :32].long()
        assert (scale[:, 0].long() - 127).tolist() == [-120, 2, 1, 3, 0, -120, 127]
        assert int(c[0].abs().max()) == 0 and int(c[1, 3]) == 64                        # zeros; amax = 4.0 = 64·2^(2−6)
        assert c[2, 3:5].tolist() == [127, -127] and int(c[6, 9]) == 127                  # one ulp below 2^k, FLT_MAX: 128 saturates
        assert c[3, 1:6].tolist() == [-10, -10, -8, -8, -6] and c[3, 12:15].tolist() == [0, 2, 2]      # ties of both parities: to even
        assert int(c[4, 7]) == -127 and int(c[4, 8]) == -64 and int(codes.min()) == -127   # never −128
        assert c[5, 4:7].tolist() == [0, 0, 1]                                             # 2^-4, the tie −0.5, 0.75 under E = −120


def test_split_is_exact_for_every_code():
    s = torch.arange(-127, 128).to(torch.int8)
    hi, lo = quant_layer.mxint8_split(s)
    assert int(hi.max()) < 64 and int(lo.max()) < 32 and not bool(((hi & 31) == 0)[hi >= 32].any())      # 6-bit codes; h = 0 is +0
    grid = mx.e2m3_values()
    h2, l2 = grid[(hi & 31).long()] * torch.where(hi >= 32, -1.0, 1.0), grid[lo.long()]
    assert torch.equal(32.0 * h2 + 2.0 * l2, s.double())                                  # 16·h + l == s with h/2, l/2 on the grid


@pytest.mark.parametrize("M,K,N", [(64, 768, 320), (64, 320, 64)])
def test_accuracy_condition_on_outliers(M, K, N):
    """one 60-outlier per row at A8 / W4: the layer error under the MXINT8 statement is at most 0.75 x the int8 row mode's and half of
    MXFP6's (computed when the mode was proposed: 0.42 / 0.63 and 0.44 / 0.46) — conditions on the arithmetic, not measurements"""
    c = rb.outlier_case(M, K, N, 8)
    y = quant_layer.mxint8_block(c["x"][0])[2].double() @ c["w"].double().t()
    e_i8, e_row, e_mx6 = float((y - c["y64"]).norm() / c["y64"].norm()), rb.outlier_errors(c)[0], mx.outlier_error_mx6(c)
    print("outlier %dx%d->%d W4: int8 rows %.3g MXFP6 %.3g MXINT8 %.3g" % (M, K, N, e_row, e_mx6, e_i8))
    assert e_i8 <= 0.75 * e_row and e_i8 <= 0.5 * e_mx6, (e_row, e_mx6, e_i8)


def test_constructor_and_cli_rules():
    from dgq_amd import inference_qmodel as cli
    q = UniformAffineQuantizer(bits=8, real_time=True, real_time_block=32, real_time_format="mxint8")
    assert q.real_time_format == "mxint8" and q.init and "real_time_format=mxint8" in q.extra_repr()
    for bad in (dict(bits=6, real_time=True, real_time_block=32), dict(bits=8, real_time=True), dict(bits=8)):
        with pytest.raises(ValueError):
            UniformAffineQuantizer(real_time_format="mxint8", **bad)
    base = ["--model_type", "tiny", "--use_aq", "--aq_real_time", "--aq_real_time_block", "32", "--aq_real_time_format", "mxint8"]
    assert cli.parse_args(base).aq_real_time_format == "mxint8"
    for bad in (base + ["--aq", "6"], base[:4] + base[6:], base[:3] + base[6:]):         # 6 bits; no block; not real-time
        with pytest.raises(SystemExit) as e:
            cli.main(bad)
        assert "mxint8" in str(e.value), bad
