"""CPU side of tests/test_gpu_weight_only_fused.py: the float64 value of the statement of dgq_conv2d_wq_mfma16_fused with its a-priori
per-element bound, a plain torch-fp32 restatement of the kernel's order (any one of MISTAKES can be planted in it, to show that the
bound notices), and the data of every case.  Everything here runs on the CPU; tests/test_weight_only_fused_ref_cpu.py is its self-check.

The statement (include/dgq_hip.h), rows m = (image b, ho, wo), k = (tap, c):
    x′[m,k] = act(norm(x[m,k])) for a tap inside the image, 0 exactly outside it and for k >= K;
    x̃ = x′ rounded once to the operand type (bf16 / f16 x) or its two-term bf16 split (fp32 x);
    t = δ[n]·Σ_k x̃·(q − z) + b[n] [+ bias_rows[b(m)][n]];  y = round_y(t [+ residual[m][n]])  or  round_y(t[2i]·gelu(t[2i + 1])).
The float64 value takes the SAME fp32 tables the kernel is given (scale / shift, or (mean, rstd) with γ / β): the statistics are not
part of this bound (their producers have their own tests).  Weights are in the reference's row order throughout (value rows first, gate
rows second for a GEGLU layer); the GPU test interleaves them when it packs.

The bound, u = 2^-24, per element (derivation, first order in u):
  * x′ in fp32.  GroupNorm: fl(fl(x·s) + h) — two roundings, each at most u·(|x·s| + |h|): 2u·(|x·s| + |h|).  LayerNorm:
    fl(fl(fl(fl(x − μ)·r)·γ) + β) — three roundings of the product p = (x − μ)·r·γ and one of the sum: 3u·|p| + u·(|p| + |β|)
    <= 4u·(|p| + |β|).  SiLU behind a norm: its derivative is at most 1.1 in magnitude, so the incoming error grows to at most
    2.2u·(|x·s| + |h|), and dgq_silu itself is good to about one ulp, 2u·|x′|.  All of it is inside 4u·(|x·s| + |h| + |x′|)
    (LayerNorm: |p|, |β|); the tests fold SiLU behind a GroupNorm or behind nothing, never behind a LayerNorm.
  * x̃: one rounding to the operand type, u_op·|x′| with u_op = U_OUT of the 16-bit type, or the split's 2^-16 for fp32 x.
    So e_k = u_op·|x′64| + 4u·(|x·s| + |h| + |x′64|), and it reaches y through |ŵ[n,k]|, ŵ = δ·(q − z).
    With no norm and no activation x′ = x and only the split is left: e_k = 2^-16·|x| for fp32 x, 0 for 16-bit x.
  * the K loop: x̃·(q − z) is exact in fp32 (a 16-bit value times a small integer), the fp32 sum of K terms in any order is within
    K·u·Σ|terms|, and the bias joins S′ = |b| + Σ_k |x′64·ŵ| as in the un-fused bound.
  * the epilogue: δ·acc, + b, then + bias_rows and + residual where given — r = 2 + (bias_rows given) + (residual given) <= 3
    roundings (no case gives both), each at most u·(|δΣ| + |b| + |bias_rows| + |res|).
  * the one rounding to y: u_out·|y64|.
        |y − y64| <= Σ_k e_k·|ŵ[n,k]| + K·u·S′ + r·u·(|δΣ| + |b| + |bias_rows| + |res|) + u_out·|y64|
  * geglu_out: out = a·gelu(g) with a, g the two values t above and E_a, E_g their bounds (all but the u_out term).  |gelu′| <= 1.13,
    so the two errors reach out through |gelu(g64)|·E_a + 1.13·|a64|·E_g; 0.5·g·(1 + erf(g/√2)) and the product are four more fp32
    roundings, 4u·|out64|; then the rounding to y:
        |out − out64| <= |gelu(g64)|·E_a + 1.13·|a64|·E_g + 4u·|out64| + u_out·|out64|."""
import functools

import torch
import torch.nn.functional as F

U = 2.0 ** -24
U_OUT = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}      # (tests/test_gpu_weight_only_mfma16.py)
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
TILE_ROWS = 32                    # the rows of the kernel's small tile: what a per-tile (instead of per-row) image index would use
TAIL = 64                         # k is staged in units up to a multiple of this; the lanes K .. carry weight code 0, i.e. −z

MISTAKES = ("pad_act_shift",      # a tap outside the image gets act(shift) instead of 0
            "tail_shift",         # the lanes k >= K get shift (their weight lanes hold code 0: q − z = −z)
            "neighbour_image",    # scale / shift of the image of the tile's FIRST row for every row of the tile
            "silu_before_norm",
            "table_by_k",         # the norm's tables indexed by k instead of k mod C
            "swap_value_gate",
            "bias_rows_image",    # bias_rows of the image of the tile's first row
            "packed_index")       # interleaved (geglu_rows) weight rows: the caller's residual read at the packed row index


# ------------------------------------------------------------------------------------------------------------- geometry
def _lin(M, K, N, **kw):
    return dict(x=(M, K), C=K, N=N, k=1, s=1, p=0, ups=False, **kw)


def _conv(B, C, H, W, N, k, s, p, ups=False):
    return dict(x=(B, C, H, W), C=C, N=N, k=k, s=s, p=p, ups=ups)


#: the geometries of tests/test_gpu_weight_only_mfma16.py that the fused cases use, and the new ones (the 64 x 64 form launches where
#: ceil(M/64)·ceil(N/64) >= 256: 17 x 17 tiles for the 23 x 23 convolution, 16 x 17 for the 1000-row layers)
GEOM = {
    "linear_37x320_24": _lin(37, 320, 24),
    "linear_70x360_72": _lin(70, 360, 72),
    "linear_33x64_128": _lin(33, 64, 128),
    "conv3_s1": _conv(2, 64, 8, 8, 64, 3, 1, 1),
    "conv3_s2": _conv(2, 64, 8, 8, 64, 3, 2, 1),
    "conv3_upsample_4x4": _conv(2, 64, 4, 4, 64, 3, 1, 1, ups=True),
    "conv1_3x96x5x7_40": _conv(3, 96, 5, 7, 40, 1, 1, 0),
    "conv3_3x96x5x7_40": _conv(3, 96, 5, 7, 40, 3, 1, 1),
    "conv3_c20": _conv(1, 20, 10, 11, 40, 3, 1, 1),
    "conv3_c7_s2": _conv(2, 7, 9, 10, 330, 3, 2, 1),
    "t64_conv3_2x16x23x23_1030": _conv(2, 16, 23, 23, 1030, 3, 1, 1),
    "t64_1000x72_1030": _lin(1000, 72, 1030),
    "linear_128x1280_40": _lin(128, 1280, 40),
    "conv3_128rows_k2880_40": _conv(2, 320, 8, 8, 40, 3, 1, 1),
    # the layers of the QuantLayer test (the bound is asked of every folding method's result)
    "layer_conv3_2x64x8x8_96": _conv(2, 64, 8, 8, 96, 3, 1, 1),
    "layer_conv1_2x64x6x6_64": _conv(2, 64, 6, 6, 64, 1, 1, 0),
    "layer_linear_38x320_72": _lin(38, 320, 72),
    "layer_linear_2x1280_320": _lin(2, 1280, 320),
}


@functools.lru_cache(maxsize=None)
def geometry(name):
    """index maps of the implicit im2col: b [M] (image of a row), valid [M][K], src [M][K] (source pixel, 0 where not valid), cc [K]"""
    c = GEOM[name]
    if len(c["x"]) == 2:
        M, K = c["x"]
        return dict(M=M, K=K, B=M, L=1, C=K, b=torch.arange(M), valid=torch.ones(M, K, dtype=torch.bool),
                    src=torch.arange(M)[:, None].expand(M, K), cc=torch.arange(K))
    B, C, Hs, Ws = c["x"]
    u = 1 if c["ups"] else 0
    H, W, k, s, p = Hs << u, Ws << u, c["k"], c["s"], c["p"]
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    M, K = B * Ho * Wo, k * k * C
    m = torch.arange(M)
    b, ho, wo = m // (Ho * Wo), (m % (Ho * Wo)) // Wo, m % Wo
    kk = torch.arange(K)
    tap, cc = kk // C, kk % C
    hi = (ho * s - p)[:, None] + (tap // k)[None, :]
    wi = (wo * s - p)[:, None] + (tap % k)[None, :]
    valid = (hi >= 0) & (hi < H) & (wi >= 0) & (wi < W)
    src = ((b[:, None] * Hs + (hi >> u)) * Ws + (wi >> u)) * valid
    return dict(M=M, K=K, B=B, L=Ho * Wo, C=C, b=b, valid=valid, src=src, cc=cc)


def rows_of(name, y):
    """the [M][N] rows of what the ops return for the case (logical NCHW for a 4-D x)"""
    return y.permute(0, 2, 3, 1).reshape(-1, y.shape[1]) if y.dim() == 4 else y.reshape(-1, y.shape[-1])


def nchw_of(name, rows):
    """[M][N] rows (residual) as the logical NCHW tensor the ops take for a 4-D x; the rows themselves for a Linear layer"""
    c, g = GEOM[name], geometry(name)
    if len(c["x"]) == 2:
        return rows
    Ho, Wo = _out_hw(c)
    return rows.view(g["B"], Ho, Wo, -1).permute(0, 3, 1, 2)


def _out_hw(c):
    u = 1 if c["ups"] else 0
    H, W = c["x"][2] << u, c["x"][3] << u
    return (H + 2 * c["p"] - c["k"]) // c["s"] + 1, (W + 2 * c["p"] - c["k"]) // c["s"] + 1


def weight_rows(w):
    """[N][C][k][k] (or [N][K]) -> [N][K] with k in (tap, c) order"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1) if w.dim() == 4 else w


# ------------------------------------------------------------------------------------------------------------- x′
def _gelu(g):
    return 0.5 * g * (1.0 + torch.erf(g * 0.70710678118654752))


def _xprime(name, x, fz, dt, mistake=None):
    """(x′ [M][K], mag [M][K]) evaluated in dtype dt (float64: the statement; float32: the kernel's order — the multiply and the add
    round separately, as compiled with contraction off); mag = |x·s| + |h| + |x′| (LayerNorm: |p| + |β| + |x′|), 0 with no prologue"""
    g = geometry(name)
    C, cc, valid = g["C"], g["cc"], g["valid"]
    xs = (x.permute(0, 2, 3, 1) if x.dim() == 4 else x).reshape(-1, C).to(dt)
    v = xs[g["src"], cc[None, :]]
    bsel = g["b"]
    if mistake == "neighbour_image":
        bsel = bsel[(torch.arange(g["M"]) // TILE_ROWS) * TILE_ROWS]
    cidx = cc[None, :].expand(g["M"], g["K"])
    act = fz.get("act", 0)
    if mistake == "silu_before_norm" and act:
        v = F.silu(v)
    mag = torch.zeros_like(v)
    shift_like = None
    if "scale" in fz:
        sc, sh = fz["scale"].to(dt), fz["shift"].to(dt)
        flat = bsel[:, None] * C + cidx
        if mistake == "table_by_k":
            flat = (bsel[:, None] * C + torch.arange(g["K"])[None, :]) % sc.numel()
        s_, h_ = sc.reshape(-1)[flat], sh.reshape(-1)[flat]
        prod = v * s_
        v = prod + h_
        mag, shift_like = prod.abs() + h_.abs(), h_
    elif "ln_stats" in fz:
        st, ga, be = fz["ln_stats"].to(dt), fz["gamma"].to(dt), fz["beta"].to(dt)
        kidx = torch.arange(g["K"]) % ga.numel() if mistake != "table_by_k" else (torch.arange(g["K"]) * 7 + 1) % ga.numel()
        prod = (v - st[:, 0:1]) * st[:, 1:2] * ga[kidx][None, :]
        h_ = be[kidx][None, :].expand_as(prod)
        v = prod + h_
        mag, shift_like = prod.abs() + h_.abs(), h_
    if act and mistake != "silu_before_norm":
        v = F.silu(v)
    pro = shift_like is not None or act
    if mistake == "pad_act_shift" and shift_like is not None:
        fill = F.silu(shift_like) if act else shift_like
        v = torch.where(valid, v, fill)
    else:
        v = v * valid
    mag = (mag + v.abs()) * valid if pro else torch.zeros_like(v)
    return v, mag, shift_like


def _tail(name, fz, dt, mistake):
    """the lanes K .. round_up(K, TAIL) of x′ [M][tail]: 0 — or, with the mistake planted, shift at the channel the lane would name"""
    g = geometry(name)
    n = (-g["K"]) % TAIL
    out = torch.zeros(g["M"], n, dtype=dt)
    if mistake == "tail_shift" and n:
        cidx = (torch.arange(g["K"], g["K"] + n)) % g["C"]
        if "scale" in fz:
            out = fz["shift"].to(dt)[g["b"]][:, cidx]
        elif "ln_stats" in fz:
            out = fz["beta"].to(dt)[cidx][None, :].expand(g["M"], n).clone()
    return out


# ------------------------------------------------------------------------------------------------------------- float64 value and bound
def ref64(name, x, w_int, delta, bias, fz, dtype):
    """(y64 [M][cols], bound [M][cols]) of the statement: x in its dtype, w_int = q − z [N][K] ((tap, c) order, reference rows), delta,
    bias [N], fz the fused inputs (scale / shift | ln_stats / gamma / beta, act, residual [M][N], bias_rows [B][N], geglu), dtype = x's
    and y's dtype"""
    g = geometry(name)
    K = g["K"]
    xp, mag, _ = _xprime(name, x, fz, torch.float64)
    w_hat = delta.double()[:, None] * w_int.double()
    pro = "scale" in fz or "ln_stats" in fz or fz.get("act", 0)
    u_op = 2.0 ** -16 if dtype == torch.float32 else U_OUT[dtype]
    if pro:
        e = u_op * xp.abs() + 4 * U * mag
    else:
        e = (2.0 ** -16 if dtype == torch.float32 else 0.0) * xp.abs()
    b64 = bias.double()[None, :]
    dsum = xp @ w_hat.T
    S = b64.abs() + xp.abs() @ w_hat.abs().T
    br = fz["bias_rows"].double()[g["b"]] if "bias_rows" in fz else torch.zeros_like(dsum)
    res = fz["residual"].double() if "residual" in fz else torch.zeros_like(dsum)
    assert not ("bias_rows" in fz and "residual" in fz)
    r = 2 + ("bias_rows" in fz) + ("residual" in fz)
    t = dsum + b64 + br
    E = e @ w_hat.abs().T + K * U * S + r * U * (dsum.abs() + b64.abs() + br.abs() + res.abs())
    if fz.get("geglu"):
        h = t.shape[1] // 2
        a, gt, Ea, Eg = t[:, :h], t[:, h:], E[:, :h], E[:, h:]
        out = a * _gelu(gt)
        return out, _gelu(gt).abs() * Ea + 1.13 * a.abs() * Eg + 4 * U * out.abs() + U_OUT[dtype] * out.abs()
    y = t + res
    return y, E + U_OUT[dtype] * y.abs()


def worst_ratio(y, y64, bound):
    return float(((y.double() - y64).abs() / bound.clamp_min(1e-300)).max())


# ------------------------------------------------------------------------------------------------------------- fp32 restatement
def restatement(name, x, w_int, zp, delta, bias, fz, dtype, mistake=None):
    """the kernel's order in plain torch fp32: x′ in fp32 (multiply and add rounded separately), one rounding to the operand type or the
    two-term bf16 split, an fp32 sum over k (its order is torch's, not the kernel's: both are inside K·u·S′), the epilogue term by term,
    one rounding to dtype.  mistake: one of MISTAKES, planted."""
    assert mistake is None or mistake in MISTAKES
    g = geometry(name)
    xp, _, _ = _xprime(name, x, fz, torch.float32, mistake)
    xp = torch.cat([xp, _tail(name, fz, torch.float32, mistake)], 1)
    wq = torch.cat([w_int.float(), (-zp.float())[:, None].expand(-1, xp.shape[1] - g["K"])], 1)
    if dtype == torch.float32:
        hi = xp.to(torch.bfloat16).float()
        lo = (xp - hi).to(torch.bfloat16).float()
        acc = lo @ wq.T + hi @ wq.T
    else:
        acc = xp.to(dtype).float() @ wq.T
    t = delta.float()[None, :] * acc + bias.float()[None, :]
    if "bias_rows" in fz:
        bsel = g["b"]
        if mistake == "bias_rows_image":
            bsel = bsel[(torch.arange(g["M"]) // TILE_ROWS) * TILE_ROWS]
        t = t + fz["bias_rows"].float()[bsel]
    if fz.get("geglu"):
        h = t.shape[1] // 2
        a, gt = (t[:, h:], t[:, :h]) if mistake == "swap_value_gate" else (t[:, :h], t[:, h:])
        return (a * (0.5 * gt * (1.0 + torch.erf(gt * 0.70710678118654752)))).to(dtype)
    if "residual" in fz:
        res = fz["residual"].float()
        if mistake == "packed_index":        # output column c is packed row 2c (value half) or 2(c − N/2) + 1 (gate half)
            h = res.shape[1] // 2
            cidx = torch.arange(res.shape[1])
            res = res[:, torch.where(cidx < h, 2 * cidx, 2 * (cidx - h) + 1)]
        t = t + res
    return t.to(dtype)


# ------------------------------------------------------------------------------------------------------------- data
def minmax_codes(w, bits):
    """(codes, δ, z) of a per-channel MINMAX quantiser (tests/test_gpu_weight_only_mfma16.py)"""
    qmax = 2 ** bits - 1
    flat = w.reshape(w.shape[0], -1)
    lo, hi = flat.amin(1).clamp(max=0.0), flat.amax(1).clamp(min=0.0)
    delta = ((hi - lo) / qmax).clamp_min(1e-8)
    zp = (-lo / delta).round()
    codes = (torch.round(flat / delta[:, None]) + zp[:, None]).clamp(0, qmax).to(torch.uint8)
    return codes.view(w.shape), delta, zp


def _wshape(c):
    return (c["N"], c["C"], c["k"], c["k"]) if len(c["x"]) == 4 else (c["N"], c["C"])


def groupnorm_tables64(x, groups, eps, gamma, beta):
    """(scale, shift) [B][C] fp32 of GroupNorm(x) = x·scale + shift from float64 statistics: what dgq_groupnorm_scale_shift produces to
    within its own bound — the CPU self-check's stand-in for it (the GPU test takes the real tables)"""
    B, C = x.shape[:2]
    xg = x.double().reshape(B, groups, -1)
    mu, var = xg.mean(-1), xg.var(-1, unbiased=False)
    rstd = (1.0 / torch.sqrt(var + eps)).repeat_interleave(C // groups, 1)
    sc = rstd * gamma.double()[None, :]
    return sc.float(), (beta.double()[None, :] - mu.repeat_interleave(C // groups, 1) * sc).float()


def layernorm_stats64(x2, eps):
    x64 = x2.double()
    mu = x64.mean(-1)
    return torch.stack([mu, 1.0 / torch.sqrt(x64.var(-1, unbiased=False) + eps)], 1).float()


@functools.lru_cache(maxsize=None)
def planted_case(name, kind, dtype, bits):
    """Exact data: x in {-3..3}; GroupNorm tables scale in {1, 2}, shift in ±{1, 2} — or LayerNorm statistics μ in {-2..2}, rstd in
    {1, 1/2}, γ in {1, 2}, integer β — so x′ is an integer of magnitude <= 8 (LayerNorm: <= 12), exact in every operand type; codes, δ
    in {1/2, 1/4, 1/8} and bias in quarters as in test_exact_integer_twin; residual / bias_rows in quarters.  Every partial sum is exact
    in fp32 (|Σ| <= 2880·12·255 < 2^24), so y is the float64 value rounded once.  kind: "gn", "gn_res", "gn_rows", "ln", "ln_res",
    "geglu" (gate rows with δ = 1, bias 0 and |gate| >= 9 by construction: erff saturates, dgq_geglu is a·g or ±0 exactly),
    "perm_res", "perm_rows" ("perm": the test packs the rows interleaved, geglu_rows without geglu_out, so the kernel must read the
    residual / bias_rows — which stay in the output's column order — at the column a packed row stands for).
    Returns (x, w [N][C][k][k] = δ·(q − z), codes, delta, zp, bias, fz, y64) — shared by the tests, do not modify the tensors."""
    c, g = GEOM[name], geometry(name)
    N, C, qmax = c["N"], c["C"], 2 ** bits - 1
    gen = torch.Generator().manual_seed(sum(map(ord, name + kind)) + bits)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=gen)
    codes = ri(0, qmax, _wshape(c))
    zp = ri(0, qmax, (N,)).float()
    delta = 2.0 ** -(1.0 + (torch.arange(N) % 3).float())
    bias = ri(-8, 8, (N,)).float() / 4
    x = ri(-3, 3, c["x"]).float()
    fz = {}
    if kind.startswith("gn"):
        fz["scale"] = ri(1, 2, (g["B"], C)).float()
        fz["shift"] = (ri(1, 2, (g["B"], C)) * (2 * ri(0, 1, (g["B"], C)) - 1)).float()
    elif kind.startswith("ln"):
        fz["ln_stats"] = torch.stack([ri(-2, 2, (g["M"],)).float(), 2.0 ** -ri(0, 1, (g["M"],)).float()], 1)
        fz["gamma"], fz["beta"] = ri(1, 2, (C,)).float(), ri(-2, 2, (C,)).float()
    elif kind == "geglu":
        # gate rows (the second half): codes so that q − z = ±1 on ONE column j(n) and 0 elsewhere, δ = 1, bias 0, and x = ±9·(1..3) on
        # every column: gate = ±x[m, j] with |gate| >= 9 (at 8 float64's erf is not yet ±1 and the float64 value of a·gelu(g) for
        # g = −8 is 1e-15·a, not the 0 that fp32 gives); the value rows keep the random codes, so a != g
        h = N // 2
        x = (9 * ri(1, 3, c["x"]) * (2 * ri(0, 1, c["x"]) - 1)).float()
        zp[h:] = 1.0
        codes[h:] = 1
        j = torch.arange(h) % C
        codes[h + torch.arange(h), j] = 2 * ri(0, 1, (h,))
        delta[h:] = 1.0
        bias[h:] = 0.0
        delta[:h] = 2.0 ** -(9.0 + (torch.arange(h) % 3).float())           # (keeps the value·gate product within fp16's range)
        fz["geglu"] = True
    if kind.startswith("perm"):
        fz["perm"] = True
    if kind.endswith("_res"):
        fz["residual"] = (ri(-16, 16, (g["M"], N)).float() / 4).to(dtype)
    if kind.endswith("_rows"):
        fz["bias_rows"] = (ri(-16, 16, (g["B"], N)).float() / 4).to(dtype)
    x = x.to(dtype)
    w_int = codes.float() - zp.view(-1, *([1] * (codes.dim() - 1)))
    w = delta.view(-1, *([1] * (codes.dim() - 1))) * w_int
    y64, _ = ref64(name, x, weight_rows(w_int), delta, bias, fz, dtype)
    return x, w, codes, delta, zp, bias, fz, y64


@functools.lru_cache(maxsize=None)
def random_case(name, kind, dtype, bits):
    """randn x (one GroupNorm group of image 0 moved to mean 40: |mean| >> std, so x·scale + shift cancels), MINMAX weights, randn
    residual / bias_rows; the tables here come from float64 statistics (the GPU test replaces them by the library's own and calls
    ref64 itself).  kind: "gn_silu", "gn_silu_res", "gn_silu_rows", "ln", "ln_res", "ln_geglu", "silu", "res", "geglu", "geglu_rows"
    (the GEGLU epilogue with bias_rows on both halves), "perm_res" (interleaved rows, see planted_case).
    Returns (x, w, codes, delta, zp, bias, fz) — shared, do not modify."""
    c, g = GEOM[name], geometry(name)
    N, C = c["N"], c["C"]
    gen = torch.Generator().manual_seed(100 + sum(map(ord, name + kind)) + bits)
    w = torch.randn(_wshape(c), generator=gen) / (C * c["k"] ** 2) ** 0.5
    codes, delta, zp = minmax_codes(w, bits)
    bias = torch.randn(N, generator=gen)
    x = torch.randn(c["x"], generator=gen)
    fz = {}
    if kind.startswith("gn"):
        groups = gn_groups(C)
        x[0, :C // groups] += 40.0
        x = x.to(dtype)
        gamma, beta = 1.0 + 0.2 * torch.randn(C, generator=gen), 0.3 * torch.randn(C, generator=gen)
        fz["gn"] = (groups, 1e-5, gamma, beta)
        fz["scale"], fz["shift"] = groupnorm_tables64(x, groups, 1e-5, gamma, beta)
    elif kind.startswith("ln"):
        x = (x + 3.0).to(dtype)
        fz["gamma"], fz["beta"] = 1.0 + 0.2 * torch.randn(C, generator=gen), 0.3 * torch.randn(C, generator=gen)
        fz["eps"] = 1e-5
        fz["ln_stats"] = layernorm_stats64(x.float(), 1e-5)
    x = x.to(dtype)
    if "silu" in kind:
        fz["act"] = 1
    if kind.endswith("_res") or kind == "res":
        fz["residual"] = torch.randn(g["M"], N, generator=gen).to(dtype)
    if kind.endswith("_rows"):
        fz["bias_rows"] = torch.randn(g["B"], N, generator=gen).to(dtype)
    if "geglu" in kind:
        fz["geglu"] = True
    if kind.startswith("perm"):
        fz["perm"] = True
    w_int = codes.float() - zp.view(-1, *([1] * (codes.dim() - 1)))
    return x, delta.view(-1, *([1] * (codes.dim() - 1))) * w_int, codes, delta, zp, bias, fz


def gn_groups(C):
    return next(gr for gr in (32, 16, 8, 7, 5, 4, 2, 1) if C % gr == 0 and C // gr >= 1 and gr <= C)


def kernel_inputs(fz):
    """the entries of fz that are inputs of the statement (the rest describes how the tables were made)"""
    return {k: v for k, v in fz.items() if k in ("scale", "shift", "ln_stats", "gamma", "beta", "act", "residual", "bias_rows", "geglu")}


#: (geometry, kind) of the exact planted-data test ...
PLANTED = [("conv3_s1", "gn"), ("conv3_s2", "gn_res"), ("conv3_upsample_4x4", "gn_rows"),
           ("conv1_3x96x5x7_40", "gn_rows"), ("conv3_3x96x5x7_40", "gn_rows"), ("conv3_3x96x5x7_40", "gn_res"),
           ("conv3_c20", "gn"), ("conv3_c7_s2", "gn_rows"), ("t64_conv3_2x16x23x23_1030", "gn_res"),
           ("linear_37x320_24", "ln"), ("linear_70x360_72", "ln_res"), ("t64_1000x72_1030", "ln"),
           ("linear_33x64_128", "geglu"), ("t64_1000x72_1030", "geglu"),
           ("linear_33x64_128", "perm_res"), ("linear_33x64_128", "perm_rows"), ("t64_1000x72_1030", "perm_res")]
#: ... and of the random-data test: every geometry above and the two long chains; residual, bias_rows and geglu_out each at least once
RANDOM = [("conv3_s1", "gn_silu"), ("conv3_s2", "gn_silu_res"), ("conv3_upsample_4x4", "gn_silu_rows"),
          ("conv1_3x96x5x7_40", "gn_silu_rows"), ("conv3_3x96x5x7_40", "gn_silu_res"), ("conv3_c20", "gn_silu"),
          ("conv3_c7_s2", "gn_silu_rows"), ("t64_conv3_2x16x23x23_1030", "gn_silu_res"),
          ("linear_37x320_24", "ln"), ("linear_70x360_72", "ln_res"), ("t64_1000x72_1030", "ln_geglu"), ("linear_33x64_128", "geglu"),
          ("linear_70x360_72", "silu"), ("linear_128x1280_40", "ln_res"), ("conv3_128rows_k2880_40", "gn_silu_rows"),
          ("linear_33x64_128", "geglu_rows"), ("t64_1000x72_1030", "perm_res")]
