"""CPU side of tests/test_gpu_groupnorm_stats.py: the data on which GroupNorm statistics kernels go wrong, the float64 reference of
the per-(batch, channel) scale / shift, the one metric both test modules use (rho: the error of x·scale + shift in units of 2^-24 of
the larger of |x|max·|scale| and |y|max, per (batch, channel)), the slice arithmetic of the standalone kernels restated, and a float64
restatement of the merge of per-(16-row block, channel) partials in which single index / factor mistakes can be switched on.
Everything here runs on the CPU."""
import torch
import torch.nn.functional as F

KINDS = ("plain", "offset", "outlier", "const", "chan")
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
EPS = 1e-5

#: (B, HW, C, G) of the standalone-kernel cases; what each one reaches is asserted by tests/test_groupnorm_stats_ref_cpu.py
GEOMS = (
    (2, 64, 320, 32),      # Cg = 10, one slice: the single launch (FINAL)
    (2, 81, 96, 32),       # Cg = 3, odd HW, one slice
    (2, 200, 64, 32),      # Cg = 2, three slices of 67, 67 and 66 rows
    (1, 1024, 32, 32),     # Cg = 1, 16 equal slices
    (1, 128, 320, 8),      # Cg = 40, two equal slices
    (1, 256, 1024, 2),     # Cg = 512: the += 256 loops, four slices
    (1, 2048, 32, 32),     # S == 32, the cap of ops.groupnorm_scale_shift
)


def slicing(B, HW, G):
    """(slices, rows_per, S, rows in the last slice): the ``slices`` expression of ops.groupnorm_scale_shift and the rows_per / S
    arithmetic of dgq_groupnorm_scale_shift, restated"""
    slices = max(1, min(32, (2048 + B * G - 1) // (B * G), HW // 64))
    return (slices,) + slicing_of(HW, slices)


def slicing_of(HW, slices):
    """(rows_per, S, rows in the last slice) of dgq_groupnorm_scale_shift for a given ``slices`` argument"""
    rows_per = (HW + slices - 1) // slices
    S = (HW + rows_per - 1) // rows_per
    return rows_per, S, HW - (S - 1) * rows_per


def group_mean_std(B, G):
    """([B][G] mean, [B][G] std) of the constructions below: every (batch, group) has its own pair"""
    i = torch.arange(B * G, dtype=torch.float64).view(B, G)
    return 3.0 * (i % 5) - 6.0, 0.5 + 0.1 * (i % 7)


def make_case(kind, B, HW, C, G, dtype, seed=0):
    """[B][HW][C] data of ``dtype``, built in float64 and cast once.  Every (batch, group) has its own mean and std and a ramp over
    the row index in [-1, 1] is added, so that a dropped or doubled slice, a wrong image pitch or a wrong channel range moves the
    statistic far outside any tolerance.
      plain    that construction
      offset   0.05·randn ± 300 (fp32) / ± 8 (16-bit types), the sign alternating with the group: |mean| >> std
      outlier  plain, + 100 at row 0 and − 100 at row HW/2 of each group's first channel (where the kernels take their shift)
      const    every group a constant of its own (M2 must come out as exactly 0)
      chan     plain without the group mean; the group's first channel + 200, its last − 150"""
    assert kind in KINDS and C % G == 0
    Cg = C // G
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + HW + C + G)
    z = torch.randn(B, HW, G, Cg, generator=g, dtype=torch.float64)
    mean, std = group_mean_std(B, G)
    mean, std = mean.view(B, 1, G, 1), std.view(B, 1, G, 1)
    ramp = torch.linspace(-1.0, 1.0, HW, dtype=torch.float64).view(1, HW, 1, 1)
    if kind == "const":
        i = torch.arange(B * G, dtype=torch.float64).view(B, 1, G, 1)
        x = (mean + 0.25 * (i % 3)).expand(B, HW, G, Cg).clone()
    elif kind == "offset":
        i = torch.arange(B * G).view(B, 1, G, 1)
        sign = 1.0 - 2.0 * (i % 2).double()
        x = 0.05 * z + sign * (300.0 if dtype == torch.float32 else 8.0)
    elif kind == "chan":
        x = std * z + ramp
        x[..., 0] += 200.0
        x[..., Cg - 1] -= 150.0
    else:
        x = mean + std * z + ramp
        if kind == "outlier":
            x[:, 0, :, 0] += 100.0
            x[:, HW // 2, :, 0] -= 100.0
    return x.reshape(B, HW, C).to(dtype)


def make_affine(C, seed=0):
    """(gamma, beta) [C] fp32: gamma in ±[0.5, 1.5] with both signs, beta ~ N(0, 1)"""
    g = torch.Generator().manual_seed(31 * seed + C)
    gamma = (0.5 + torch.rand(C, generator=g)) * (1.0 - 2.0 * (torch.arange(C) % 5 == 3).float())
    return gamma, torch.randn(C, generator=g)


def moments64(x, G):
    """([B][G] mean, [B][G] biased variance) of the values as stored, in float64"""
    B, HW, C = x.shape
    xg = x.double().view(B, HW, G, C // G)
    mean = xg.mean(dim=(1, 3))
    return mean, ((xg - mean.view(B, 1, G, 1)) ** 2).mean(dim=(1, 3))


def scale_shift_of(mean, var, G, eps, gamma, beta):
    """float64 scale / shift [B][C] of GroupNorm from [B][G] moments: scale = rstd·γ, shift = β − mean·rstd·γ"""
    Cg = gamma.numel() // G
    rstd = (var + eps).rsqrt().repeat_interleave(Cg, dim=1)
    scale = rstd * gamma.double().view(1, -1)
    return scale, beta.double().view(1, -1) - mean.repeat_interleave(Cg, dim=1) * scale


def ref_scale_shift(x, G, eps, gamma, beta):
    """(scale64, shift64) [B][C]: GN(x) = x·scale + shift in float64 from the values of x [B][HW][C] as stored, biased variance as
    F.group_norm"""
    mean, var = moments64(x, G)
    return scale_shift_of(mean, var, G, eps, gamma, beta)


def _rho(x, G, y64, scale64, y):
    B, HW, C = x.shape
    Cg = C // G
    err = (y - y64).abs().amax(dim=1)
    xmax = x.double().abs().view(B, HW, G, Cg).amax(dim=(1, 3)).repeat_interleave(Cg, dim=1)
    A = torch.maximum(xmax * scale64.abs(), y64.abs().amax(dim=1))
    r = err / (2.0 ** -24 * A).clamp_min(1e-300)
    return r, float(r.max())


def rho(x, G, eps, gamma, beta, scale, shift):
    """The metric, per (batch, channel) and never aggregated: y = x·scale + shift evaluated in float64 from the fp32 scale / shift under
    test against y64 from the float64 statistics; err[b,c] = max over the rows of |y − y64|, A[b,c] = max(|x|max of the group ·
    |scale64[b,c]|, max over the rows of |y64|), rho = err / (2^-24·A).  Returns ([B][C] rho, its maximum)."""
    scale64, shift64 = ref_scale_shift(x, G, eps, gamma, beta)
    xd = x.double()
    y64 = xd * scale64.unsqueeze(1) + shift64.unsqueeze(1)
    y = xd * scale.double().cpu().unsqueeze(1) + shift.double().cpu().unsqueeze(1)
    return _rho(x, G, y64, scale64, y)


def rho_of_y(x, G, eps, gamma, beta, y):
    """the same metric of a finished y [B][HW][C] (the yardstick: F.group_norm in fp32)"""
    scale64, shift64 = ref_scale_shift(x, G, eps, gamma, beta)
    y64 = x.double() * scale64.unsqueeze(1) + shift64.unsqueeze(1)
    return _rho(x, G, y64, scale64, y.double())


def yardstick(x, G, eps, gamma, beta):
    """rho of F.group_norm evaluated in fp32 on the CPU on the values as stored: the arithmetic the reference project runs"""
    y = F.group_norm(x.float().permute(0, 2, 1).contiguous(), G, gamma.float(), beta.float(), eps).permute(0, 2, 1)
    return rho_of_y(x, G, eps, gamma, beta, y)


def worst(r):
    """(b, c, rho) of the worst entry of a [B][C] rho tensor, for failure messages"""
    i = int(r.argmax())
    return i // r.shape[1], i % r.shape[1], float(r.flatten()[i])


# ---------------------------------------------------------------------------------------- the partials merge, restated in float64
def partials64(y, stored=None):
    """[B][HW/16][C][2] = (mean, M2) per 16-row block and channel of y [B][HW][C] in float64 — what the producers' epilogues write.
    ``stored``: the tensor the statistics are taken of instead of y (a mistake: the unrounded values instead of the stored ones)."""
    src = (y if stored is None else stored).double()
    B, HW, C = src.shape
    blk = src.view(B, HW // 16, 16, C)
    mean = blk.mean(dim=2)
    return torch.stack([mean, ((blk - mean.unsqueeze(2)) ** 2).sum(dim=2)], dim=-1)


def merge_partials64(p1, p2, G, mistake=None):
    """([B][G] mean, [B][G] biased variance) from the partial buffers p1 [B][RB][C1][2] and p2 [B][RB][C2][2] (or None) of a channel
    concat, indexed the way gn_from_partials_kernel indexes its flat buffers.  mistake: None, "pitch" (C1 as the pitch of the second
    buffer) or "factor16" (the 16· of the between-block term dropped)."""
    B, RB, C1, _ = p1.shape
    C2 = 0 if p2 is None else p2.shape[2]
    C, Cg = C1 + C2, (C1 + C2) // G
    f1 = p1.reshape(-1)
    f2 = None if p2 is None else p2.reshape(-1)
    pitch2 = C1 if mistake == "pitch" else C2
    mean = torch.zeros(B, G, dtype=torch.float64)
    var = torch.zeros(B, G, dtype=torch.float64)
    rb = torch.arange(RB).view(RB, 1)
    for b in range(B):
        for g in range(G):
            c = (g * Cg + torch.arange(Cg)).view(1, Cg)
            i1 = ((b * RB + rb) * C1 + c) * 2
            vals = []
            for first in (True, False):
                sel = (c < C1) if first else (c >= C1)
                sel = sel.expand(RB, Cg)
                if not sel.any():
                    continue
                if first:
                    idx = i1[sel]
                    vals.append((f1[idx], f1[idx + 1]))
                else:
                    idx = (((b * RB + rb) * pitch2 + (c - C1)) * 2)[sel] % f2.numel()       # (a wrong pitch stays inside the buffer)
                    vals.append((f2[idx], f2[idx + 1]))
            m = torch.cat([v[0] for v in vals])
            m2 = torch.cat([v[1] for v in vals])
            mu = m.mean()
            between = ((m - mu) ** 2).sum() * (1.0 if mistake == "factor16" else 16.0)
            mean[b, g] = mu
            var[b, g] = (m2.sum() + between) / (16.0 * m.numel())
    return mean, var
