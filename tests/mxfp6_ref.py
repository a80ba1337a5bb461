"""TEST INFRASTRUCTURE — the CPU statements of the real-time MXFP6 activation mode (``real_time_format="mxfp6"``: dgq_quant_act_mx6 +
dgq_gemm_mx6) for tests/test_realtime_mxfp6_cpu.py and tests/test_gpu_realtime_mxfp6.py: a float64 / integer restatement of the
quantiser rule written independently of ``quant_layer.mx6_block`` (nearest grid value by search, not by rint), the E2M3 grid, the layer
in float64, planted exact data with its exactness margin, and the edge blocks of the issue.  Nothing here touches the GPU."""
import math

import torch
import torch.nn.functional as F

from tests import layer_reference as lr
from tests import realtime_block_ref as rb

BLK = 32


def e2m3_values():
    """the 32 E2M3 magnitudes by 5-bit code (exponent << 3 | mantissa), ascending: bias 1, subnormals m/8"""
    out = []
    for code in range(32):
        e, m = code >> 3, code & 7
        out.append(m / 8.0 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 1))
    return torch.tensor(out, dtype=torch.float64)


def mx6_reference(rows):
    """(codes uint8 [R][C], scale uint8 [R][C/32], x̂ float64 [R][C]) of fp32 rows [R][C]: per 32-block E = floor(log2 amax) − 2 in
    [−127, 127] (−127 for amax = 0), v = x·2^−E in float64, the NEAREST grid magnitude (a tie takes the even code; |v| above 7.5 has 7.5
    as its nearest), sign kept unless the magnitude is 0."""
    x = rows.detach().float().double()
    R, C = x.shape
    xb = x.view(R, C // BLK, BLK)
    amax = xb.abs().amax(dim=2)
    _, ex = torch.frexp(amax)                               # amax = m·2^ex, 0.5 <= m < 1: floor(log2 amax) = ex − 1
    E = torch.where(amax > 0, ex.to(torch.int64) - 3, torch.full_like(ex, -127, dtype=torch.int64)).clamp(-127, 127)
    v = xb * torch.pow(torch.tensor(2.0, dtype=torch.float64), -E.double())[:, :, None]
    assert float(v.abs().max()) < 8.0
    grid = e2m3_values()
    a = v.abs()
    lo = (torch.searchsorted(grid, a.reshape(-1), right=True) - 1).view(a.shape)
    hi = torch.clamp(lo + 1, max=31)
    dl, dh = a - grid[lo], grid[hi] - a
    up = (hi != lo) & ((dh < dl) | ((dh == dl) & (hi % 2 == 0)))
    mag = torch.where(up, hi, lo)
    neg = (v < 0) & (mag > 0)
    codes = (mag + 32 * neg.to(torch.int64)).to(torch.uint8).view(R, C)
    xhat = (torch.where(neg, -grid[mag], grid[mag]) * torch.pow(torch.tensor(2.0, dtype=torch.float64), E.double())[:, :, None]).view(R, C)
    return codes, (E + 127).to(torch.uint8), xhat


def decode(codes, scale):
    """x̂ float64 [R][C] from codes uint8 [R][C] and scale bytes [R][>= C/32]"""
    R, C = codes.shape
    c = codes.to(torch.int64)
    val = e2m3_values()[c & 31] * torch.where((c & 32) != 0, -1.0, 1.0).double()
    sc = torch.pow(torch.tensor(2.0, dtype=torch.float64), scale[:, :C // BLK].double() - 127.0)
    return (val.view(R, C // BLK, BLK) * sc[:, :, None]).view(R, C)


def edge_blocks():
    """rows [R][64] of fp32 values; block 0 of each row is one edge block of the issue, block 1 plain randn"""
    g = torch.Generator().manual_seed(606)
    rows = []

    def row(blk):
        rows.append(torch.cat([blk.float(), torch.randn(BLK, generator=g)]))
    row(torch.zeros(BLK))                                                   # all zeros
    b = torch.randn(BLK, generator=g).clamp(-0.9, 0.9); b[3] = 4.0; row(b)   # amax an exact power of two
    b = torch.randn(BLK, generator=g).clamp(-0.9, 0.9); b[5] = -0.25; b[6] = 0.2; row(b * 0.25)
    for top in (7.6, 7.75, 7.8, 7.99):                                      # (7.5, 7.75] and (7.75, 8): both saturate
        b = torch.randn(BLK, generator=g); b[9] = top; b[10] = -top; row(b.clamp(-top, top) * 2.0 ** -5)
    # exact ties at every step size, both ways: k + 0.5 steps with k even and odd; the block maximum 7.0 keeps E = 0 (then scaled)
    ties = torch.tensor([0.0625, 0.1875, 0.9375, 1.0625, 1.1875, 1.9375, 2.125, 2.375, 3.875, 4.25, 4.75, 7.25, 7.0,
                         -0.0625, -0.1875, -0.9375, -1.0625, -1.1875, -1.9375, -2.125, -2.375, -3.875, -4.25, -4.75, -7.25, 0.3125, 0.4375,
                         3.125, 3.375, 5.25, 5.75, 6.25])
    assert ties.numel() == BLK
    row(ties); row(ties * 2.0 ** 7); row(ties * 2.0 ** -9)
    b = torch.randn(BLK, generator=g); b[0] = -0.0; b[1] = 0.0; b[2] = -1e-6; row(b)      # negative zero, a negative value that rounds to 0
    b = torch.zeros(BLK); b[4] = 2.0 ** -130; b[5] = -(2.0 ** -131); b[6] = 2.0 ** -133; b[7] = 2.0 ** -134; row(b)        # subnormal amax
    b = torch.randn(BLK, generator=g); b[11] = 2.0 ** 100; row(b)
    b = torch.randn(BLK, generator=g) * 2.0 ** 98; b[12] = -(2.0 ** 100); row(b)
    b = torch.randn(BLK, generator=g); b[13] = 60.0; row(b)                 # one 60 among randn values
    b = torch.full((BLK,), -0.0); row(b)                                    # all negative zeros: amax = 0
    return torch.stack(rows)


# ----------------------------------------------------------------------------------------------- the layer
def input_rows(case, x):
    """the rows the quantiser sees: a Linear input's rows, a convolution input's pixels"""
    return x.reshape(-1, x.shape[-1]) if case["kind"] == "linear" else rb.pixel_rows(x)


def rows_to_input(case, rows, like):
    if case["kind"] == "linear":
        return rows.reshape(like.shape)
    B, C, H, W = like.shape
    return rows.reshape(B, H, W, C).permute(0, 3, 1, 2)


def layer_float64_w(case, xhat, w, bias, residual=None):
    """float64 layer on a dequantised input x̂ (the input's own layout, float64) with the weight w [N][...] (reference layout): nearest 2x
    upsample, then F.linear / F.conv2d"""
    N = w.shape[0]
    w = w.double()
    if case["kind"] == "linear":
        y = F.linear(xhat, w.reshape(N, -1), bias.double() if bias is not None else None)
    else:
        if case["upsample"]:
            xhat = F.interpolate(xhat, scale_factor=2.0, mode="nearest")
        y = F.conv2d(xhat, w.reshape(N, case["C"], case["k"], case["k"]), bias.double() if bias is not None else None, stride=case["stride"],
                     padding=case["pad"])
    return y if residual is None else y + residual.double()


def layer_float64(case, xhat, qw, zw, wd, bias, residual=None):
    """``layer_float64_w`` with the weight δw·(q − z) of integer codes qw [N][K_ref], zero points zw and scales wd"""
    N = qw.shape[0]
    w = wd.reshape(-1, 1).double() * (qw.double().reshape(N, -1) - zw.reshape(-1, 1).double())
    return layer_float64_w(case, xhat, w, bias, residual)


def mx6_layer_reference(case, x, qw, zw, wd, bias, residual=None):
    """y (float64) of the layer under the MXFP6 statement: the input (fp32, behind any prologue) quantised per row / pixel by
    ``mx6_reference``, then ``layer_float64``.  Also returns x̂."""
    xhat = rows_to_input(case, mx6_reference(input_rows(case, x.float()))[2], x)
    return layer_float64(case, xhat, qw, zw, wd, bias, residual), xhat


def term_magnitudes(case, xhat, qw, zw, wd, bias):
    """T = |bias| + δw·Σ|x̂·(q − z)| per output element, in the layout of the layer output"""
    N = qw.shape[0]
    cen = (qw.double().reshape(N, -1) - zw.reshape(-1, 1).double()).abs()
    return layer_float64(case, xhat.abs(), cen, torch.zeros(N), wd.abs(), bias.abs() if bias is not None else None)


#: block exponents of the planted data (E per (row, block) drawn from these)
PLANT_E = (-3, -2, -1, 0)


def mx6_exact_margin(case, xhat, qw, zw, wd, bias, residual):
    """Every term of the layer — x̂·(q − z)·δw with x̂ a multiple of 2^(E_min − 3), bias, residual (integers) — is a multiple of the
    power of two u = min(2^(E_min − 3)·δw_n, 1), and a fp32 sum of such terms is exact in ANY order (and under any intermediate
    alignment that keeps 24 bits) while the sum of their magnitudes stays below 2^24·u.  Returns max (sum of magnitudes) / (2^24·u);
    exact iff < 1."""
    T = term_magnitudes(case, xhat, qw, zw, wd, bias) + residual.double().abs()
    unit = torch.clamp(2.0 ** (min(PLANT_E) - 3) * wd.reshape(-1).double(), max=1.0)
    unit = unit.view(1, 1, -1) if case["kind"] == "linear" else unit.view(1, -1, 1, 1)
    return float((T / unit).max()) / 2.0 ** 24


def planted_mx6(case):
    """``layer_reference._build_exact`` (integer weight codes, zero points, bias, residual; power-of-two δw) with every input value ON its
    block's grid: x′ = g·2^E, g an E2M3 value, E drawn per (row, block) from PLANT_E, and one element of every block planted with a
    magnitude in [4, 7.5] so that floor(log2 amax) − 2 = E — asserted through ``mx6_reference``, which must return E and x̂ = x′.
    Returns the recipe dict with x replaced and ``E`` [rows][C/32]."""
    d = lr._build_exact(case, "perM", 6, 4, lr.PROFILES[0])
    g = torch.Generator().manual_seed(lr._seed("planted-mx6", case["name"]))
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g)
    rows = input_rows(case, d["x"])
    R, C = rows.shape
    nb = C // BLK
    grid = e2m3_values()
    E = torch.tensor(PLANT_E)[ri(0, len(PLANT_E) - 1, (R, nb))]
    mag = grid[ri(0, 19, (R, nb, BLK))]                                       # magnitudes up to 2.75 ...
    top = grid[ri(24, 31, (R, nb))]                                           # ... and one of 4 .. 7.5 per block
    mag.scatter_(2, ri(0, BLK - 1, (R, nb, 1)), top[:, :, None])
    sign = 1.0 - 2.0 * ri(0, 1, (R, nb, BLK)).double()
    xb = (sign * mag * torch.pow(torch.tensor(2.0, dtype=torch.float64), E.double())[:, :, None]).float()
    rows = xb.reshape(R, C)
    codes, scale, xhat = mx6_reference(rows)
    assert torch.equal(scale.long() - 127, E.long()), "planted blocks: the quantiser's E is not the planted one"
    assert torch.equal(xhat, rows.double()), "planted blocks: x is not on its block's grid"
    d["x"] = rows_to_input(case, rows, d["x"]).contiguous()
    d["E"] = E
    d["layout"] = "mx6"
    return d


def outlier_rows(rows, seed=0):
    """the outlier recipe on rows [R][C]: one element per row set to 60"""
    g = torch.Generator().manual_seed(lr._seed("mx6-outlier", rows.shape[0], rows.shape[1], seed))
    rows = rows.clone()
    rows[torch.arange(rows.shape[0]), torch.randint(0, rows.shape[1], (rows.shape[0],), generator=g)] = 60.0
    return rows


def outlier_error_mx6(c):
    """rel-L2 of the float64 layer under the MXFP6 statement against y64 of ``realtime_block_ref.outlier_case``"""
    xhat = mx6_reference(c["x"][0])[2]
    y = xhat @ c["w"].double().t()
    return float((y - c["y64"]).norm() / c["y64"].norm())


def _self_check():
    g = e2m3_values()
    assert g.numel() == 32 and float(g[-1]) == 7.5 and float(g[8]) == 1.0 and math.isclose(float(g[1]), 0.125)


_self_check()
