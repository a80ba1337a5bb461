"""Host side of the real-time MXFP4 activation mode (no GPU): the statement ``quant_layer.mx4_block`` against the independent float64
restatement of tests/mxfp4_ref.py on random data and on the edge blocks, the operand packing, the exactness claim behind the mixed
FP4 x FP6 product, the accuracy on the outlier data, the quantizer's constructor and the CLI flag."""
import pytest
import torch

from tests import mxfp4_ref as mx
from tests import realtime_block_ref as rb
from dgq_amd.quant import quant_layer
from dgq_amd.quant.quant_layer import Scaler, UniformAffineQuantizer

#: layer error of MXFP4 over the int4 row mode's on the outlier data (64x768 -> 320, W4), from the statements on the CPU; the int4 block
#: mode's over MXFP4's is BLOCK_OVER_MX4
MX4_OVER_ROW = 0.4561          # row 0.4366, MXFP4 0.1991: 2.2x lower
BLOCK_OVER_MX4 = 0.4948        # block 0.09851: the int4 block mode (a fitted step and zero point per block) is 2.0x lower still


def _same(rows):
    codes, scale, xhat = quant_layer.mx4_block(rows)
    rc, rs, rx = mx.mx4_reference(rows)
    assert codes.dtype == torch.uint8 and scale.dtype == torch.uint8 and xhat.dtype == torch.float32
    assert torch.equal(scale, rs), (scale != rs).nonzero()[:4].tolist()
    assert torch.equal(codes, rc), (codes != rc).nonzero()[:4].tolist()
    assert torch.equal(xhat.double(), rx) and torch.equal(mx.decode(codes, scale), rx)
    return codes, scale, xhat


def test_statement_equals_restatement_on_randn():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(200, 96, generator=g) * torch.logspace(-4, 4, 200).view(200, 1) + 0.2
    codes, scale, xhat = _same(x)
    # the rule itself: amax lands in [4, 8)·2^E, so an element is off by at most half the widest step, 1·2^E — or, saturating from below 8, 2·2^E
    E = scale.double() - 127.0
    amax = x.view(200, 3, 32).abs().amax(dim=2).double()
    assert bool((amax >= 4.0 * 2.0 ** E).all()) and bool((amax < 8.0 * 2.0 ** E).all())
    assert bool(((x.double() - xhat.double()).abs().view(200, 3, 32) < 2.0 * (2.0 ** E)[:, :, None]).all())


def test_statement_equals_restatement_on_edge_blocks():
    rows = mx.edge_blocks()
    codes, scale, xhat = _same(rows)
    assert int(scale[0, 0]) == 0 and int(codes[0, :32].max()) == 0                  # all zeros: E = −127, every code +0
    assert int(scale[8, 0]) == 0 and int(codes[8, :32].max()) == 0                  # all −0 likewise
    want = [int((mx.GRID == v).nonzero()) for v in mx.TIES.values()]                # every planted tie, both signs, at three scales
    assert want == [0, 2, 2, 4, 4, 6, 6, 7, 7, 7]
    for r, s in ((1, 127), (2, 134), (3, 118)):
        assert int(scale[r, 0]) == s and codes[r, :10].tolist() == want and codes[r, 10:20].tolist() == [c + 8 if c else 0 for c in want], r
    assert codes[4, 9:12].tolist() == [7, 15, 7]                                    # ±7.99 and 6.01 (scaled): ±6
    assert codes[5, :3].tolist() == [0, 0, 0]                                       # −0, +0, a negative value that rounds to zero: +0
    assert int(scale[6, 0]) == 0 and codes[6, 4:7].tolist() == [0, 9, 2]            # subnormal amax 2^-127: E = −127
    assert int(scale[7, 0]) == 125 + 127 and codes[7, 11:13].tolist() == [7, 12]    # the largest finite amax saturates; −2^126 is −2·2^125


def test_packing_round_trips():
    codes = torch.randint(0, 16, (7, 96), generator=torch.Generator().manual_seed(3)).to(torch.uint8)
    packed = quant_layer.mx4_pack(codes)
    assert packed.shape == (7, 3, 16) and packed.dtype == torch.uint8
    assert torch.equal(quant_layer.mx4_unpack(packed), codes)
    for r, b in ((0, 0), (6, 2)):                                                   # element j at bits 4j .. 4j + 3 of the 128-bit string
        big = int.from_bytes(bytes(packed[r, b].tolist()), "little")
        assert [(big >> (4 * j)) & 15 for j in range(32)] == codes[r, 32 * b:32 * b + 32].tolist()


def test_products_are_exact_in_fp32():
    """the claim behind "exact": (q − z)/2 for |q − z| <= 15 times every E2M1 magnitude is an fp32 number (and the grids agree)"""
    assert list(quant_layer.E2M1_MAGNITUDES) == mx.GRID.tolist()
    h = torch.arange(-15, 16, dtype=torch.float64) / 2.0
    prod = h[:, None] * mx.GRID[None, 1:]
    assert h.numel() == 31 and torch.equal(prod.float().double(), prod)
    assert torch.equal((h.float()[:, None] * mx.GRID.float()[None, 1:]).double(), prod)


def test_accuracy_on_outliers():
    """one 60-outlier per row of x = randn·1.3 + 0.2 at A4, 64x768 -> 320: the MXFP4 layer error against the int4 row mode's and the int4
    block mode's, each from its statement.  The ratio to the row mode is pinned (the constant above, from this very computation, which
    is deterministic on the CPU); the GPU test allows 1.25x on it for the fp32 summation order."""
    c = rb.outlier_case(64, 768, 320, 4)
    e_row, e_blk = rb.outlier_errors(c)
    e_mx = mx.outlier_error_mx4(c)
    print("outlier 64x768->320 A4: row %.4g block %.4g mxfp4 %.4g (mx/row %.4f, block/mx %.4f)" % (e_row, e_blk, e_mx, e_mx / e_row, e_blk / e_mx))
    assert e_mx / e_row < 1.0
    assert e_mx / e_row == pytest.approx(MX4_OVER_ROW, rel=1e-3) and e_blk / e_mx == pytest.approx(BLOCK_OVER_MX4, rel=1e-3)


def test_quantizer_constructor_and_repr():
    q = UniformAffineQuantizer(bits=4, scaler=Scaler.MINMAX, leaf_param=True, real_time=True, real_time_block=32, real_time_format="mxfp4")
    assert q.real_time and q.real_time_block == 32 and q.real_time_format == "mxfp4" and q.init and q.delta is None
    assert "real_time_format=mxfp4" in q.extra_repr()
    for bad in (dict(bits=6, real_time=True, real_time_block=32, real_time_format="mxfp4"),
                dict(bits=4, real_time=True, real_time_format="mxfp4"),
                dict(bits=4, real_time_format="mxfp4"),
                dict(bits=4, real_time=True, real_time_block=32, real_time_format="mxfp4", real_time_mx_w8=True)):
        with pytest.raises(ValueError):
            UniformAffineQuantizer(**bad)


def test_cli_flag_rules():
    from dgq_amd import inference_qmodel as cli
    base = ["--model_type", "tiny", "--use_aq", "--aq_real_time", "--aq_real_time_block", "32"]
    assert cli.parse_args(base + ["--aq", "4", "--aq_real_time_format", "mxfp4"]).aq_real_time_format == "mxfp4"
    for bad in (base + ["--aq_real_time_format", "mxfp4"],                                                      # 8 activation bits
                base + ["--aq", "6", "--aq_real_time_format", "mxfp4"],
                ["--model_type", "tiny", "--use_aq", "--aq_real_time", "--aq", "4", "--aq_real_time_format", "mxfp4"],     # no block
                base + ["--aq", "4", "--aq_real_time_format", "mxfp4", "--aq_real_time_mx_w8"]):
        with pytest.raises(SystemExit) as e:
            cli.main(bad)
        assert "mx" in str(e.value), bad
