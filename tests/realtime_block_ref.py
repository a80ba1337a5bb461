"""TEST INFRASTRUCTURE — the CPU statements of the real-time BLOCK activation quantiser (one (δ, z) per row and block of 32 consecutive
channels, ``quant_layer.block_minmax``) for tests/test_realtime_block_cpu.py and tests/test_gpu_realtime_block.py: block tables of a
Linear input and of a convolution's input pixels, their expansion to the per-element tables ``layer_reference.reference_layer`` takes,
the layer formula of dgq_gemm_blockq in float64, the exactness margin of planted data, and the outlier recipe of the issue.
Nothing here touches the GPU."""
import torch
import torch.nn.functional as F

from oracle import dgq_oracle as orc
from tests import layer_reference as lr

BLK = 32
TINY = float(torch.tensor(1e-8))                         # fp32(1e-8): δ of an all-zero block


def block_tables(rows, bits):
    """(δ, z) [R][C/32] of rows [R][C] (fp32 values): block_minmax of every block's extrema"""
    from dgq_amd.quant.quant_layer import block_minmax
    R, C = rows.shape
    xb = rows.float().reshape(R, C // BLK, BLK)
    return block_minmax(xb.min(dim=2)[0], xb.max(dim=2)[0], 2 ** bits)


def beta_of(d, z, bits):
    """β = δ·(2^(b−1) − z) as the quantiser forms it: one fp32 product"""
    return d * (float(2 ** (bits - 1)) - z)


def block_codes(rows, d, z, bits):
    """integer codes [R][C] (fp32) of rows under their block tables: the reference's fp32 divide, round half to even, clamp"""
    return orc.uaq_codes(rows.float(), d.repeat_interleave(BLK, dim=1), z.repeat_interleave(BLK, dim=1), bits)


def rho_chain(s_rows, d):
    """ρ[row] = Σ_c δ_c·rs_c as the kernel adds it: fp32 product per block, one fp32 addition per block in ascending order from 0"""
    R, C = s_rows.shape
    rs = s_rows.reshape(R, C // BLK, BLK).sum(dim=2)      # exact integers
    rho = torch.zeros(R)
    for c in range(C // BLK):
        rho = rho + d[:, c] * rs[:, c]
    return rho


def rho_float64(s_rows, d):
    R, C = s_rows.shape
    t = d.double() * s_rows.double().reshape(R, C // BLK, BLK).sum(dim=2)
    return t.sum(dim=1), t.abs().sum(dim=1)


def pixel_rows(x):
    """[B, C, H, W] -> [B·H·W][C]: the rows the quantiser sees of a convolution input"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def expand_linear(d, z):
    """block tables [M][K/32] -> per-element (1, M, K) tables for reference_layer (x [1, M, K])"""
    return d.repeat_interleave(BLK, dim=1).unsqueeze(0), z.repeat_interleave(BLK, dim=1).unsqueeze(0)


def expand_conv(d, z, shape, k, stride, pad, upsample=False):
    """per-pixel block tables [B·H·W][C/32] of an input of ``shape`` = (B, C, H, W) -> (δ, z, inside) as [B, C·k·k, L] tensors in
    F.unfold's c·k·k + tap order: what the quantiser of the unfolded operand applies per element.  A tap outside the image is a block
    of zeros: δ = fp32(1e-8), z = 0.  inside = 1.0 where the element lies in the image."""
    B, C, H, W = shape
    full = lambda t: t.repeat_interleave(BLK, dim=1).reshape(B, H, W, C).permute(0, 3, 1, 2)
    df, zf = full(d), full(z)
    if upsample:
        df, zf = F.interpolate(df, scale_factor=2.0, mode="nearest"), F.interpolate(zf, scale_factor=2.0, mode="nearest")
    unf = lambda t: F.unfold(t, kernel_size=k, dilation=1, padding=pad, stride=stride)
    inside = unf(torch.ones_like(df))
    du = torch.where(inside > 0, unf(df), torch.full((), TINY))
    return du, unf(zf), inside


def block_reference(case, d, x=None):
    """y (float64) of ``layer_reference.reference_layer`` for recipe dict d (x, w, bias, residual, abits) under the block tables the CPU
    statement gives for x (a prologue'd input overrides the recipe's); also returns the codes, the expanded (δ, z) and expand_conv's
    ``inside`` (None for a Linear layer)."""
    x = d["x"] if x is None else x
    bits = d["abits"]
    if case["kind"] == "linear":
        M, K = x.shape[-2], x.shape[-1]
        de, ze = expand_linear(*block_tables(x.reshape(M, K), bits))
        inside = None
    else:
        de, ze, inside = expand_conv(*block_tables(pixel_rows(x), bits), tuple(x.shape), case["k"], case["stride"], case["pad"], case["upsample"])
    y, q = lr.reference_layer(x, d["w"], d["bias"], de, ze, bits, case["kind"], case.get("k", 1), case.get("stride", 1), case.get("pad", 0),
                              d.get("residual"), case.get("upsample", False))
    return y, q, de, ze, inside


def natural(t, case, blocks=False):
    """an unfolded-operand tensor [B, C·k·k, L] (linear: [1, M, K]) as rows in the natural (tap, c) K order: [M][chunks][32], or
    [M][chunks] taking one value per 32-block (tables)"""
    if case["kind"] == "linear":
        rows = t.reshape(-1, t.shape[-1])
    else:
        B, CK, L = t.shape
        kk = case["k"] ** 2
        rows = t.reshape(B, CK // kk, kk, L).permute(0, 3, 2, 1).reshape(B * L, CK)
    rows = rows.reshape(rows.shape[0], -1, BLK)
    return rows[:, :, 0] if blocks else rows


def formula_float64(case, q, de, ze, inside, qw, wz, wd, bias, bits):
    """The layer formula of dgq_gemm_blockq in float64 from codes, tables and Vc:
        Y[m,n] = b[n] + δw[n]·( Σ_c ( δ[m,c]·P[m,n,c] + β[m,c]·Vc[n,c] ) − zw[n]·R[m] ),  P = Σ_{k∈c} s·qw,  R = Σ_c δ·rs
    with s = q − 2^(b−1), β = fp32(δ·(2^(b−1) − z)), Vc = Σ_{k∈c} (qw − zw); δ = β = 0 (and no term of R) on a tap outside the image.
    q / de / ze / inside: [B, C·k·k, L] (linear [1, M, K]; inside None); qw [N][K_ref] integer codes; returns [M][N]."""
    o = float(2 ** (bits - 1))
    s = natural(q - o, case).double()
    dn, zn = natural(de, case, blocks=True), natural(ze, case, blocks=True)
    beta = beta_of(dn, zn, bits)
    if inside is not None:
        m = natural(inside, case, blocks=True)
        dn, beta = dn * m, beta * m
        s = s * natural(inside, case).double()
    dn, beta = dn.double(), beta.double()
    if case["kind"] == "linear":
        qn = qw.double().reshape(qw.shape[0], -1, BLK)
    else:
        kk = case["k"] ** 2
        qn = qw.double().reshape(qw.shape[0], -1, kk).permute(0, 2, 1).reshape(qw.shape[0], -1, BLK)
    P = torch.einsum("mck,nck->mnc", s, qn)
    Vc = (qn - wz.double().view(-1, 1, 1)).sum(dim=2)
    R = (dn * s.sum(dim=2)).sum(dim=1)
    acc = (dn[:, None, :] * P).sum(dim=2) + beta @ Vc.t()
    return bias.double()[None, :] + wd.double().view(1, -1) * (acc - wz.double().view(1, -1) * R[:, None])


def rows_to_output(y_rows, case, like):
    """[M][N] rows -> the layout of reference_layer's y ([1, M, N] / [B, N, Ho, Wo])"""
    if case["kind"] == "linear":
        return y_rows.reshape(like.shape)
    B, N, Ho, Wo = like.shape
    return y_rows.reshape(B, Ho, Wo, N).permute(0, 3, 1, 2)


def block_exact_margin(case, d, q, de, ze, inside=None):
    """``layer_reference.exact_margin`` for block tables (its per-K branch with a table per ROW): every term dgq_gemm_blockq forms is a
    multiple of u = min(δ_min·wd_n, 1) — δ_c·P_c (|.| <= δ_c·Σ_{k∈c}|s||qw'|), β_c·Vc (<= Σ_{k∈c} δ|o − z||q − z|), zw'·R with R = Σ_c δ_c·rs_c
    (itself such a sum), bias and residual — and a fp32 sum of such terms is exact in any order while the sum of their magnitudes stays
    below 2^24·u.  A tap outside the image (``inside`` == 0, from expand_conv) forms no term: the kernel takes δ = β = 0 there.
    Returns max (sum of magnitudes) / (2^24·u); exact iff < 1."""
    bits, wbits = d["abits"], d["wbits"]
    o = float(2 ** (bits - 1))
    s = (lr.codes_rows(q, case) - o).double().abs()
    dk = lr.codes_rows(de.expand_as(q), case).double()
    zk = lr.codes_rows(ze.expand_as(q), case).double()
    dmin = dk.min()
    if inside is not None:
        m = lr.codes_rows(inside, case).double()
        dmin = dk[m > 0].min()
        s, dk = s * m, dk * m
    M, K = s.shape
    qw, wz, wd = d["qw"].double(), d["wzp"].reshape(-1).double(), d["wdelta"].reshape(-1).double()
    woff = 0.0 if wbits == 4 else 128.0
    qmag, zmag, cen = (qw - woff).abs(), (wz - woff).abs(), (qw - wz[:, None]).abs()
    res = d["residual"].double().abs()
    fixed = d["bias"].double().abs()[None, :] + (res.reshape(M, -1) if case["kind"] == "linear" else res.permute(0, 2, 3, 1).reshape(M, -1))
    rows = (s * dk).sum(dim=1)
    total = wd[None, :] * ((s * dk) @ qmag.t() + zmag[None, :] * rows[:, None] + (dk * (o - zk).abs()) @ cen.t()) + fixed
    unit = torch.clamp(dmin * wd, max=1.0)[None, :]
    return max(float((total / unit).max()), float(rows.max() / dmin)) / 2.0 ** 24


def planted_exact(case, abits, wbits):
    """``layer_reference._build_exact`` (integer weights, bias, residual) with the input kept INSIDE planted extremes −z·2^e and
    (2^b − 1 − z)·2^e of every (row, 32-channel block) — a Linear row's blocks, a convolution's input pixels' blocks — both planted in the
    block: block_minmax then returns δ = 2^e and z exactly (asserted), and every fp32 step of the layer is exact.  Returns the recipe
    dict with x replaced, plus e and z [rows][C/32]."""
    prof = lr.PROFILES[lr.profile_for(case, "perK", abits, wbits)]
    d = lr._build_exact(case, "perK", abits, wbits, prof)
    g = torch.Generator().manual_seed(lr._seed("planted-block", case["name"], abits, wbits))
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g)
    lin = case["kind"] == "linear"
    rows = d["x"].reshape(-1, d["x"].shape[-1]) if lin else pixel_rows(d["x"])
    R, C = rows.shape
    nb = C // BLK
    e = torch.tensor(prof["dexp"])[ri(0, len(prof["dexp"]) - 1, (R, nb))].double()
    z = (2 ** (abits - 1) + prof["zstep"] * ri(-4, 4, (R, nb))).double()
    lo, hi = (-z * 2.0 ** e).float(), ((2 ** abits - 1 - z) * 2.0 ** e).float()
    xb = (2 * ri(-prof["xr"], prof["xr"], (R, nb, BLK))).float()
    xb = torch.maximum(torch.minimum(xb, hi[:, :, None]), lo[:, :, None])
    i0, i1 = ri(0, BLK // 2 - 1, (R, nb)), ri(BLK // 2, BLK - 1, (R, nb))
    xb.scatter_(2, i0[:, :, None], lo[:, :, None])
    xb.scatter_(2, i1[:, :, None], hi[:, :, None])
    rows = xb.reshape(R, C)
    dt, zt = block_tables(rows, abits)
    assert torch.equal(dt, (2.0 ** e).float()), "planted blocks: δ is not 2^e"
    assert torch.equal(zt, z.float()), "planted blocks: z is not the planted one"
    if lin:
        d["x"] = rows.reshape(d["x"].shape)
    else:
        B, Cc, H, W = d["x"].shape
        d["x"] = rows.reshape(B, H, W, Cc).permute(0, 3, 1, 2).contiguous()
    d["layout"] = "block"
    return d


def outlier_case(M, K, N, abits, wbits=4, seed=0):
    """The data of the issue's measurement: x = randn·1.3 + 0.2 with ONE element per row set to 60, w = randn·K^-0.5 under the project's
    per-channel MINMAX weight quantiser.  Returns dict(x [1, M, K], w (dequantised), w_raw, wdelta, wzp, bias, y64 = the float64 product
    with UNQUANTISED activations)."""
    from dgq_amd import synth
    g = torch.Generator().manual_seed(lr._seed("outlier", M, K, N, seed))
    x = torch.randn(1, M, K, generator=g) * 1.3 + 0.2
    x[0, torch.arange(M), torch.randint(0, K, (M,), generator=g)] = 60.0
    w = torch.randn(N, K, generator=g) * K ** -0.5
    wd, wz = synth.channel_minmax(w, wbits)
    w_deq = orc.uaq(w, wd, wz, wbits)
    bias = torch.zeros(N)
    return dict(x=x, w=w_deq, w_raw=w, wdelta=wd, wzp=wz, bias=bias, residual=None, abits=abits, wbits=wbits,
                y64=x.double() @ w_deq.double().t())


def outlier_errors(c):
    """(row-mode error, block-mode error): rel-L2 of the float64 layer output under per-row / per-block MINMAX tables against y64"""
    from dgq_amd.quant.quant_layer import row_minmax
    x, bits = c["x"], c["abits"]
    M, K = x.shape[1], x.shape[2]
    rel = lambda y: float((y - c["y64"]).norm() / c["y64"].norm())
    dr, zr = row_minmax(x[0].min(dim=1)[0], x[0].max(dim=1)[0], 2 ** bits)
    y_row = lr.reference_layer(x, c["w"], c["bias"], dr.view(1, M, 1), zr.view(1, M, 1), bits, "linear")[0]
    y_blk = lr.reference_layer(x, c["w"], c["bias"], *expand_linear(*block_tables(x[0], bits)), bits, "linear")[0]
    return rel(y_row), rel(y_blk)
