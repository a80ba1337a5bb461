"""TEST INFRASTRUCTURE — the CPU statements of the real-time MXFP4 activation mode (``real_time_format="mxfp4"``: dgq_quant_act_mx4 +
dgq_gemm_mx4) for tests/test_realtime_mxfp4_cpu.py and tests/test_gpu_realtime_mxfp4.py: a float64 restatement of the OCP block rule
written independently of ``quant_layer.mx4_block`` (the E2M1 grid as a table, the nearest value by explicit comparison, a tie to the
even code), the edge blocks of the issue and planted exact data.  The layer in float64 (``y64``) is tests/mxfp6_ref.py's, which takes
any dequantised input.  Nothing here touches the GPU."""
import torch

from tests import layer_reference as lr
from tests import mxfp6_ref as mx6
from tests.mxfp6_ref import input_rows, rows_to_input, layer_float64, term_magnitudes, outlier_rows      # noqa: F401  (the layer side)

BLK = 32
#: the E2M1 magnitudes by 3-bit code (exponent << 1 | mantissa)
GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)
#: the ties the issue pins, v -> the grid value it rounds to (the even code), and the saturating band
TIES = {0.25: 0.0, 0.75: 1.0, 1.25: 1.0, 1.75: 2.0, 2.5: 2.0, 3.5: 4.0, 5.0: 4.0, 6.5: 6.0, 7.0: 6.0, 7.75: 6.0}


def mx4_reference(rows):
    """(codes uint8 [R][C], scale uint8 [R][C/32], x̂ float64 [R][C]) of fp32 rows [R][C]: per 32-block E = floor(log2 amax) − 2 in
    [−127, 127] (−127 for amax = 0), v = x·2^−E in float64, the NEAREST grid magnitude (a tie takes the even code; |v| above 6 has 6 as
    its nearest), sign kept unless the magnitude is 0."""
    x = rows.detach().float().double()
    R, C = x.shape
    xb = x.view(R, C // BLK, BLK)
    amax = xb.abs().amax(dim=2)
    _, ex = torch.frexp(amax)                               # amax = m·2^ex, 0.5 <= m < 1: floor(log2 amax) = ex − 1
    E = torch.where(amax > 0, ex.to(torch.int64) - 3, torch.full_like(ex, -127, dtype=torch.int64)).clamp(-127, 127)
    two = torch.tensor(2.0, dtype=torch.float64)
    v = xb * torch.pow(two, -E.double())[:, :, None]
    assert float(v.abs().max()) < 8.0
    a = v.abs()
    lo = (torch.searchsorted(GRID, a.reshape(-1), right=True) - 1).view(a.shape)
    hi = torch.clamp(lo + 1, max=7)
    dl, dh = a - GRID[lo], GRID[hi] - a
    mag = torch.where((hi != lo) & ((dh < dl) | ((dh == dl) & (hi % 2 == 0))), hi, lo)
    neg = (v < 0) & (mag > 0)
    codes = (mag + 8 * neg.to(torch.int64)).to(torch.uint8).view(R, C)
    xhat = (torch.where(neg, -GRID[mag], GRID[mag]) * torch.pow(two, E.double())[:, :, None]).view(R, C)
    return codes, (E + 127).to(torch.uint8), xhat


def decode(codes, scale):
    """x̂ float64 [R][C] from codes uint8 [R][C] and scale bytes [R][>= C/32]"""
    R, C = codes.shape
    c = codes.to(torch.int64)
    val = GRID[c & 7] * torch.where((c & 8) != 0, -1.0, 1.0).double()
    sc = torch.pow(torch.tensor(2.0, dtype=torch.float64), scale[:, :C // BLK].double() - 127.0)
    return (val.view(R, C // BLK, BLK) * sc[:, :, None]).view(R, C)


def edge_blocks():
    """rows [R][64] of fp32 values; block 0 of each row is one edge block of the issue, block 1 plain randn.  Rows: 0 zeros; 1 .. 3 the
    planted ties at the scales 2^0, 2^7, 2^-9 (elements 0 .. 9 the keys of TIES, 10 .. 19 their negatives; 7.75 keeps E); 4 saturation
    from just under a power of two; 5 −0, +0 and a negative value that rounds to 0; 6 subnormal amax; 7 the largest finite amax; 8 all −0"""
    g = torch.Generator().manual_seed(404)
    rows = []

    def row(blk):
        rows.append(torch.cat([blk.float(), torch.randn(BLK, generator=g)]))
    row(torch.zeros(BLK))
    t = torch.tensor(list(TIES))
    ties = torch.cat([t, -t, torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -6.0, 0.2, -0.3, 5.5])]).float()
    assert ties.numel() == BLK
    row(ties); row(ties * 2.0 ** 7); row(ties * 2.0 ** -9)
    b = torch.randn(BLK, generator=g).clamp(-3, 3); b[9] = 7.99; b[10] = -7.99; b[11] = 6.01; row(b * 2.0 ** -5)
    b = torch.randn(BLK, generator=g); b[0] = -0.0; b[1] = 0.0; b[2] = -1e-6; row(b)
    b = torch.zeros(BLK); b[4] = 2.0 ** -130; b[5] = -(2.0 ** -128); b[6] = 2.0 ** -127; row(b)
    b = torch.randn(BLK, generator=g); b[11] = torch.finfo(torch.float32).max; b[12] = -(2.0 ** 126); row(b)
    row(torch.full((BLK,), -0.0))
    return torch.stack(rows)


#: block exponents of the planted data
PLANT_E = mx6.PLANT_E


def planted_mx4(case):
    """``layer_reference._build_exact`` (integer weight codes, zero points, bias, residual; power-of-two δw) with every input value ON its
    block's grid: x′ = g·2^E, g an E2M1 value, E per (row, block) from PLANT_E, one element of every block 4 or 6 so that
    floor(log2 amax) − 2 = E — asserted through ``mx4_reference``.  Every term is then a multiple of 2^(E_min − 1)·δw, a multiple of the
    unit of ``mxfp6_ref.mx6_exact_margin``, which therefore serves (conservatively) as this recipe's margin."""
    d = lr._build_exact(case, "perM", 4, 4, lr.PROFILES[0])
    g = torch.Generator().manual_seed(lr._seed("planted-mx4", case["name"]))
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g)
    rows = input_rows(case, d["x"])
    R, C = rows.shape
    nb = C // BLK
    E = torch.tensor(PLANT_E)[ri(0, len(PLANT_E) - 1, (R, nb))]
    mag = GRID[ri(0, 5, (R, nb, BLK))]
    mag.scatter_(2, ri(0, BLK - 1, (R, nb, 1)), GRID[ri(6, 7, (R, nb))][:, :, None])
    sign = 1.0 - 2.0 * ri(0, 1, (R, nb, BLK)).double()
    rows = (sign * mag * torch.pow(torch.tensor(2.0, dtype=torch.float64), E.double())[:, :, None]).float().reshape(R, C)
    _, scale, xhat = mx4_reference(rows)
    assert torch.equal(scale.long() - 127, E.long()) and torch.equal(xhat, rows.double())
    d["x"] = rows_to_input(case, rows, d["x"]).contiguous()
    return d


def outlier_error_mx4(c):
    """rel-L2 of the float64 layer under the MXFP4 statement against y64 of ``realtime_block_ref.outlier_case``"""
    y = mx4_reference(c["x"][0])[2] @ c["w"].double().t()
    return float((y - c["y64"]).norm() / c["y64"].norm())
