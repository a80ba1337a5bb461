"""TEST INFRASTRUCTURE — the real-time MXINT8 mode's quantiser rule restated in float64 independently of ``quant_layer.mxint8_block``
(frexp and a nearest-integer search, not the exponent field and rint), and the edge blocks of the issue.  Nothing here touches the GPU."""
import torch

BLK = 32


def mxint8_reference(rows):
    """(s int64 [R][C], scale uint8 [R][C/32], x̂ float64 [R][C]) of fp32 rows: per 32-block E = floor(log2 amax) in [−120, 127] (−120
    for amax = 0), v = x·2^(6−E) in float64, the NEAREST integer (a tie takes the even one), clamped to ±127; x̂ = s·2^(E−6)."""
    x = rows.detach().float().double()
    R, C = x.shape
    xb = x.view(R, C // BLK, BLK)
    amax = xb.abs().amax(dim=2)
    _, ex = torch.frexp(amax)                               # amax = m·2^ex, 0.5 <= m < 1: floor(log2 amax) = ex − 1
    E = torch.where(amax > 0, ex.to(torch.int64) - 1, torch.full_like(ex, -120, dtype=torch.int64)).clamp(-120, 127)
    v = xb * torch.pow(torch.tensor(2.0, dtype=torch.float64), 6.0 - E.double())[:, :, None]
    lo = torch.floor(v)
    up = (v - lo > 0.5) | ((v - lo == 0.5) & (lo % 2 != 0))
    s = torch.clamp(lo + up.double(), -127.0, 127.0)
    xhat = (s * torch.pow(torch.tensor(2.0, dtype=torch.float64), E.double() - 6.0)[:, :, None]).view(R, C)
    return s.to(torch.int64).view(R, C), (E + 127).to(torch.uint8), xhat


def edge_blocks():
    """rows [7][64] of fp32 values; block 0 of each row is one edge block of the issue, block 1 plain randn"""
    g = torch.Generator().manual_seed(808)
    below = lambda v: torch.nextafter(torch.tensor(v), torch.tensor(0.0)).item()
    small = lambda: torch.randn(BLK, generator=g).clamp(-0.9, 0.9)
    blocks = [torch.zeros(BLK), small(), small(), (torch.arange(BLK).float() - 11.5) / 8.0, small(), torch.zeros(BLK), torch.randn(BLK, generator=g) * 1e37]
    blocks[1][3] = 4.0                                                      # amax an exact power of two
    blocks[2][3], blocks[2][4] = below(4.0), -below(4.0)                    # one ulp below: 128 saturates to 127
    blocks[3][0] = 8.0                                                      # E = 3: elements 1 .. 31 are the ties −10.5 .. 19.5
    blocks[4][7], blocks[4][8] = -below(2.0), -1.0                          # the most negative value: −127, never −128
    blocks[5][4], blocks[5][5], blocks[5][6] = 2.0 ** -130, -(2.0 ** -127), 1.5 * 2.0 ** -127       # subnormal amax: the E clamp
    blocks[6][9] = torch.finfo(torch.float32).max
    return torch.stack([torch.cat([b.float(), torch.randn(BLK, generator=g)]) for b in blocks])
