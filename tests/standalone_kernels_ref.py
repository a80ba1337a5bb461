"""Float64 statements of the stand-alone quantiser and statistics kernels (csrc/attn_quant.hip, calib_stats.hip, adaround.hip,
weights.hip: dgq_quantize_weight), with the input builders of tests/test_gpu_standalone_kernels.py.  Checked against itself, and against
planted mistakes, by tests/test_standalone_kernels_ref_cpu.py.  Nothing here is measured on a GPU; where a figure is quoted it comes from
the CPU test of this module and says so.

The quotient rule.  Every affine quantiser here starts from t = fp32(x/δ) of two fp32 numbers (16-bit tensors are converted exactly).
``quotient32`` forms x/δ in float64 and rounds it to fp32: the float64 quotient carries 53 >= 2·24 + 2 bits, so rounding it a second
time gives the IEEE fp32 quotient (the CPU test checks ``torch.equal`` with torch's fp32 division on 4 M pairs).  From there every
step is a single fp32 operation on fp32 operands, which float64 evaluates exactly before the one rounding ``.float()`` applies:
round half to even, + z, clamp, − z, ·δ, and one rounding to the tensor's type.  The result is unique, so comparisons are on bit patterns
(``same_bits``).

No NaN anywhere: v_med3_f32 / fminf / fmaxf and torch.clamp / torch.min treat it differently and no caller produces one.
No denormal operand or result in the log2 cases (planted small values stay >= 1e-30 with δ >= 1e-3): the statement does not depend on a
denormal mode.
"""
import hashlib
import math

import torch

U = 2.0 ** -24                                       # unit round-off of fp32
INT_VIEW = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}
DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _seed(*parts):
    return int.from_bytes(hashlib.sha256("|".join(str(p) for p in ("standalone",) + parts).encode()).digest()[:6], "little")


def gen(*parts):
    return torch.Generator().manual_seed(_seed(*parts))


def same_bits(a, b):
    """torch.equal on the bit patterns (−0.0 != +0.0, inf == inf)"""
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(INT_VIEW[a.dtype]), b.view(INT_VIEW[b.dtype]))


def count_bit_mismatches(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return int((a.view(INT_VIEW[a.dtype]) != b.view(INT_VIEW[b.dtype])).sum())


def quotient32(x, d):
    """fp32(x/δ) of fp32-representable operands, through float64"""
    return (x.double() / d.double()).float()


def _rne(t32, rounding):
    if rounding == "even":
        return torch.round(t32)                      # exact on fp32: round half to even
    assert rounding == "away"                        # planted mistake
    t = t32.double()
    return (torch.sign(t) * torch.floor(t.abs() + 0.5)).float()


def affine_codes(x, d, z, qmax, rounding="even", recip=False, clamp_first=False):
    """fp32 codes clamp(rne(fp32(x/δ)) + z, 0, qmax) of broadcastable fp32 tensors.  ``recip`` / ``clamp_first`` / ``rounding="away"`` are
    the planted mistakes of the CPU test: x·fp32(1/δ) with no fallback, the clamp taken before z is added, ties away from zero."""
    if recip:
        inv = (1.0 / d.double()).float()
        t = (x.double() * inv.double()).float()
    else:
        t = quotient32(x, d)
    r = _rne(t, rounding)
    if clamp_first:
        return (torch.clamp(r.double(), 0.0, qmax) + z.double()).float()
    return torch.clamp((r.double() + z.double()).float(), 0.0, qmax)


def affine_dequant(q, d, z):
    """fp32(δ·fp32(q − z))"""
    return (d.double() * (q.double() - z.double()).float().double()).float()


# ----------------------------------------------------------------------------------------------- dgq_fakequant_rows
def table_index(rows, C, T, D, mode, skip):
    """[rows][C] index into the (δ, z) table and the mask of quantised elements: token t = row % T, quantised where t >= skip;
    mode 0: one entry, mode 1: entry t − skip (T − skip entries), mode 2: entry col % D (D entries)."""
    t = (torch.arange(rows) % T).view(-1, 1).expand(rows, C)
    col = torch.arange(C).view(1, -1).expand(rows, C)
    idx = torch.zeros(rows, C, dtype=torch.long) if mode == 0 else ((t - skip).clamp_min(0) if mode == 1 else col % D)
    return idx, t >= skip


def table_len(T, D, mode, skip):
    return 1 if mode == 0 else (T - skip if mode == 1 else D)


def fakequant_rows_ref(x, T, D, mode, delta, zp, skip, bits, rounding="even", recip=False, clamp_first=False, skip_on="tokens"):
    """dgq_fakequant_rows on x [rows][C] of any of the three types -> same type.  Rows of skipped tokens come back with their own bits."""
    rows, C = x.shape
    qmax = float(2 ** bits - 1)
    idx, live = table_index(rows, C, T, D, mode, skip)
    if skip_on == "columns":                         # planted mistake
        live = torch.arange(C).view(1, -1).expand(rows, C) >= skip
        idx = table_index(rows, C, T, D, mode, 0)[0].clamp_max(delta.numel() - 1)
    d, z = delta.float().reshape(-1)[idx], zp.float().reshape(-1)[idx]
    xf = x.float()
    q = affine_codes(xf, d, z, qmax, rounding, recip, clamp_first)
    y = affine_dequant(q, d, z).to(x.dtype)
    return torch.where(live, y, x)


FQ_SHAPES = {"t77_8x40": (2, 77, 8, 40), "t129_2x8": (2, 129, 2, 8), "t129_3x5": (2, 129, 3, 5), "stride": (2, 4100, 4, 40)}
FQ_FAMILIES = ("randn", "ties", "saturate", "bigq")


def _log_uniform(n, lo, hi, g):
    return torch.exp(torch.rand(n, generator=g, dtype=torch.float64) * (math.log(hi) - math.log(lo)) + math.log(lo)).float()


def tie_lattice(d, g, nmax=300):
    """x = fp32((n + ½)·δ), |n| <= nmax, and its ±1 / ±2 ulp neighbours, a fifth each, for the per-element δ ``d`` (fp32).  With a general
    δ the fp32 quotient of a lattice point is an exact tie only where the two roundings cancel; the CPU test measures the shares
    (on the CPU: 0.21 of the elements are exact fp32 ties, 0.39 lie just above one and 0.39 just below) and asserts that all three
    occur."""
    n = torch.randint(-nmax, nmax + 1, d.shape, generator=g).double()
    x = ((n + 0.5) * d.double()).float()
    side = torch.randint(0, 5, d.shape, generator=g)
    up, dn = torch.full_like(x, float("inf")), torch.full_like(x, float("-inf"))
    x1u, x1d = torch.nextafter(x, up), torch.nextafter(x, dn)
    x2u, x2d = torch.nextafter(x1u, up), torch.nextafter(x1d, dn)
    for k, v in ((1, x1u), (2, x1d), (3, x2u), (4, x2d)):
        x = torch.where(side == k, v, x)
    return x


def is_exact_tie(x, d):
    t = quotient32(x, d).double()
    return (t - torch.floor(t)) == 0.5


def fq_case(family, shape, mode, dtype, skip, bits):
    """One cell of the fake-quant matrix: dict(x [rows][C] of ``dtype``, T, D, delta, zp).  The tables are fp32; the data are built in fp32 and then converted,
    so a 16-bit cell holds the nearest 16-bit values (for ``ties`` those are ordinary values again: the lattice is an fp32 claim;
    for ``saturate`` fp16 turns the large magnitudes into ±inf)."""
    B, T, H, D = FQ_SHAPES[shape]
    rows, C = B * T, H * D
    g = gen("fq", family, shape, mode, skip, bits)            # (not the dtype: the three types see the same fp32 draw)
    n = table_len(T, D, mode, skip)
    qmax = 2 ** bits - 1
    mid = float(2 ** (bits - 1))
    idx, _ = table_index(rows, C, T, D, mode, skip)
    if family == "randn":
        delta = (6.0 / qmax) * (0.5 + torch.rand(n, generator=g))
        zp = mid + torch.randint(-3, 4, (n,), generator=g).float()
        x = torch.randn(rows, C, generator=g) * 1.3 + 0.1
    elif family == "ties":
        delta = _log_uniform(n, 1e-4, 10.0, g)
        zp = mid + torch.randint(-3, 4, (n,), generator=g).float()
        x = tie_lattice(delta[idx], g, nmax=300)
    elif family == "saturate":
        delta = _log_uniform(n, 1e-3, 0.3, g)
        zp = mid + torch.randint(-3, 4, (n,), generator=g).float()
        zp[0::3] = -3.0                                         # the two out-of-range zero points of layer_reference
        zp[1::3] = float(2 ** bits + 2)
        if n == 1:
            zp[0] = -3.0 if skip == 0 else float(2 ** bits + 2)
        inf = float("inf")
        vals = torch.tensor([3e38, -3e38, inf, -inf, 1e30, -1e30, 65504.0, -65504.0, 1e4, -1e4, 0.0, -0.0, 300.0, -300.0])
        pick = torch.randint(0, vals.numel() + 6, (rows, C), generator=g)
        body = torch.randn(rows, C, generator=g) * delta[idx] * qmax
        x = torch.where(pick < vals.numel(), vals[pick.clamp_max(vals.numel() - 1)], body)
    else:
        assert family == "bigq"
        # |t| from 1e5 to 3.5e6, across the 3e6 threshold above which the kernel always divides; z = −n0 brings the codes into range.
        # n0 + qmax < 2^22, so half-integers are representable and r + z is exact
        n0 = torch.round(_log_uniform(n, 1e5, 3.5e6 - qmax, g).double()) * (torch.randint(0, 2, (n,), generator=g).double() * 2 - 1)
        n0[0] = 3.0e6 - 2 ** (bits - 1)                         # one entry straddles the threshold itself
        delta = _log_uniform(n, 1e-3, 0.3, g)
        zp = (-n0).float()
        k = torch.randint(-2, qmax + 3, (rows, C), generator=g).double()
        frac = torch.tensor([0.0, 0.5, 0.25, -0.25, 0.49, -0.5])[torch.randint(0, 6, (rows, C), generator=g)].double()
        x = ((n0[idx] + k + frac) * delta.double()[idx]).float()
    if skip:                                                    # a skipped token row holds −0.0 (and the rest of its own data)
        x.view(B, T, C)[:, 0, ::7] = -0.0
    return dict(x=x.to(dtype).contiguous(), T=T, D=D, rows=rows, C=C, delta=delta.contiguous(), zp=zp.contiguous())


# ----------------------------------------------------------------------------------------------- dgq_max_f32 / dgq_logquant_f32
#: half-width of the undecided band of the log2 code.  The kernel rounds −log2f(u), u = fp32(v/δ); |log2f| < 256 there, so one ulp of the
#: result is at most 2^-16, the library documents 1 ulp for log2f, and 2·2^-16 covers it with the rounding of the exact value itself.
#: (tests/attention_quant_ref.py states a band for the fused kernels' log code, τ_log, but that one carries the score and row-sum errors
#: of the fused evaluation and is wider, not tighter: it does not apply to this kernel.)
LOG_BAND = 2.0 * 2.0 ** -16
#: at most this share of a case's elements may be undecided (the share the old golden comparison tolerates without naming them)
LOG_UNDECIDED_CAP = 1e-3


def max_ref(p, skip_cols=0, over_all=False):
    """dgq_max_f32: max(0, max over the columns >= skip_cols), exact.  ``over_all``: the planted mistake that looks at column 0 too."""
    v = p if (over_all or not skip_cols) else p[..., skip_cols:]
    return max(float(v.max()), 0.0)


def logquant_ref(p, delta, bits, skip_cols=0):
    """-> (lo, hi, decided): the two admissible outputs fp32(2^-q·δ) for q = the clamped code of t64 ∓ LOG_BAND, t64 = −log2(fp32(v/δ))
    in float64; ``decided`` where they coincide.  Columns < skip_cols carry the input in both.  v = 0: t64 = +inf, code 2^b − 1."""
    qmax = float(2 ** bits - 1)
    d = torch.as_tensor(delta, dtype=torch.float32).reshape(())
    u = quotient32(p, d).double()
    t = -torch.log2(u)
    out = []
    for s in (-LOG_BAND, LOG_BAND):
        q = torch.clamp(torch.round(t + s), 0.0, qmax)
        y = (torch.exp2(-q) * d.double()).float()
        if skip_cols:
            y[..., :skip_cols] = p[..., :skip_cols]
        out.append(y)
    return out[0], out[1], same_bits_mask(out[0], out[1])


def same_bits_mask(a, b):
    return a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)


def logquant_check(y, lo, hi):
    """the GPU test's comparison: every element equals one of its admissible values bit for bit -> number of elements that do not"""
    y = y.cpu()
    return int((~(same_bits_mask(y, lo) | same_bits_mask(y, hi))).sum())


LOG_SHAPES = {"b2h4_70x77": (2, 4, 70, 77), "odd_3x129x33": (3, 129, 33), "stride_8200x160": (8200, 160)}


def log_case(shape, skip_cols, static):
    """Softmax rows of randn·3 with: exact zeros, small values down to 1e-30, column 0 the largest of every row when skip_cols = 1,
    and for the stride shape the maximum of the counted columns in the last, partial round of the 4096 x 256-thread grid.
    -> dict(p, delta (static: a quarter of the counted maximum, so values above δ occur; None: real-time), skip_cols)"""
    g = gen("log", shape, skip_cols, static)
    dims = LOG_SHAPES[shape]
    p = torch.softmax(torch.randn(*dims, generator=g) * 3.0, dim=-1).contiguous()
    flat = p.view(-1)
    n = flat.numel()
    where = torch.randperm(n, generator=g)[:64]
    flat[where[:32]] = 0.0
    flat[where[32:]] = 10.0 ** -torch.randint(8, 31, (32,), generator=g).float()
    S = dims[-1]
    if n > 4096 * 256:
        pos = n - 3
        assert pos >= 4096 * 256 and pos % S >= skip_cols
        flat[pos] = float(flat.max()) * 1.5
    if skip_cols:
        p[..., 0] = p.max(dim=-1).values * 1.25 + 0.01
    m = max_ref(p, skip_cols)
    delta = torch.tensor([m * 0.25]) if static else None
    return dict(p=p, delta=delta, skip_cols=skip_cols)


def log_init_scores(x, deltas, bits):
    """The L2 score of T2ILogQuantizer._init_quantization_param for each candidate δ, in float64, as an interval [lo, hi]: an undecided
    element contributes the smaller of its two squared errors to lo and the larger to hi."""
    out = []
    for d in deltas:
        a, b, _ = logquant_ref(x, d, bits)
        ea, eb = (x.double() - a.double()).pow(2), (x.double() - b.double()).pow(2)
        out.append((float(torch.minimum(ea, eb).mean()), float(torch.maximum(ea, eb).mean())))
    return out


def log_init_pick(scores):
    """index of the candidate the search keeps (the strict minimum), or None where the intervals of ``log_init_scores`` do not separate
    the best from the rest by more than the fp32 evaluation of a mean of squares can move them (1e-4 relative, generously)"""
    k = min(range(len(scores)), key=lambda i: scores[i][0])
    rest = [s[0] for i, s in enumerate(scores) if i != k]
    return k if scores[k][1] * (1 + 1e-4) < min(rest) * (1 - 1e-4) else None


# ----------------------------------------------------------------------------------------------- dgq_minmax_rows_cols
MM_ROWS = (1, 63, 65, 64 * 256 + 1)
MM_COLS = (1, 40, 257)
POISON = 1e30


def minmax_case(rows, C, dtype, sliced):
    """x [rows][C]: randn with ±inf, ±0 planted (never a whole row or column of one of them except where rows or C is 1).
    ``sliced``: x is the view buf[:, 3:3 + C] of a [rows][C + 9] buffer whose other columns hold ±1e30 (fp16: ±65504): ldx > C with
    an unaligned base, and any read outside the view shows in the result."""
    g = gen("minmax", rows, C, dtype)                          # (not ``sliced``: the view holds the contiguous case's data)
    v = torch.randn(rows, C, generator=g) * 3.0
    k = max(1, rows * C // 50)
    where = torch.randperm(rows * C, generator=g)[:4 * k]
    flat = v.view(-1)
    for j, val in enumerate((float("inf"), float("-inf"), 0.0, -0.0)):
        flat[where[j * k:(j + 1) * k]] = val
    v = v.to(dtype)
    if not sliced:
        return v.contiguous(), None
    big = POISON if dtype != torch.float16 else 65504.0
    buf = torch.full((rows, C + 9), big).to(dtype)
    buf[:, 1::2] = -buf[:, 1::2]
    buf[:, 3:3 + C] = v
    return buf[:, 3:3 + C], buf


def minmax_ref(x, buf=None):
    """(rowmin, rowmax, colmin, colmax) of the fp32 values.  ``buf`` (the buffer x is a view of): the planted mistake that walks the
    storage from the view's first element as if its rows were C apart."""
    v = x.float()
    if buf is not None:
        rows, C = x.shape
        v = buf.reshape(-1)[x.storage_offset():x.storage_offset() + rows * C].reshape(rows, C).float()
    return v.min(1).values, v.max(1).values, v.min(0).values, v.max(0).values


def zero_sign_checkable(x, ext, dim):
    """mask of the extrema that are zero and whose row / column holds one kind of zero only (the sign of a zero extremum is defined)"""
    v = x.float()
    z = v == 0
    neg = z & torch.signbit(v)
    pos = z & ~torch.signbit(v)
    return (ext == 0) & ~(neg.any(dim) & pos.any(dim))


# ----------------------------------------------------------------------------------------------- adaround / dgq_quantize_weight
LN11 = math.log(11.0)                                # s·1.2 − 0.1 reaches 0 at α = −ln 11 and 1 at α = +ln 11
#: |r_device − r| of r = s·1.2 − 0.1: expf to 1 ulp (2u relative), 1 + e and the quotient one rounding each (|s| <= 1: 4u absolute), times
#: 1.2; the fp32 constant 1.1 − (−0.1), the product and the sum one rounding each of magnitude <= 1.2 (3.6u), −0.1f itself 0.1u: < 9u
ADA_DR = 9.0 * U


def adaround_case(N=640, K=640, bits=4):
    """One weight above the 1024 x 256-thread grid of the four kernels (409 600 > 262 144) with α = randn·4 and, planted, ∓ln 11 and their
    ±1 ulp neighbours (the rectifier's edges)."""
    g = gen("adaround", N, K, bits)
    w = torch.randn(N, K, generator=g) * 0.2
    lo, hi = w.min(1).values.clamp_max(0), w.max(1).values.clamp_min(0)
    delta = ((hi - lo) / (2 ** bits - 1)).clamp_min(1e-8)
    zp = torch.round(-lo / delta)
    alpha = torch.randn(N, K, generator=g) * 4.0
    e = torch.tensor([LN11, -LN11])
    up, dn = torch.nextafter(e, torch.full_like(e, 100.0)), torch.nextafter(e, torch.full_like(e, -100.0))
    edges = torch.cat([e, up, dn])
    where = torch.randperm(N * K, generator=g)[:edges.numel() * 8]
    alpha.view(-1)[where] = edges.repeat(8)
    alpha.view(-1)[-6:] = edges                       # and in the last stride round
    gout = torch.randn(N, K, generator=g)
    return dict(w=w, delta=delta, zp=zp, alpha=alpha, bits=bits, gout=gout)


def adaround_ref(c, b_list=(20.0, 7.3, 2.0), reg_weight=0.01):
    """The header comment of csrc/adaround.hip in float64 (the floor on the fp32 quotient, which is what both the reference and the kernel
    floor).  -> dict(out, galpha (mask applied), galpha_open (no mask), edge (elements where a mask is within rounding of flipping),
    reg[b] = dict(value, bound, galpha)); the regulariser's gradients are those of reg_weight·R, the
    loss weight under which test_adaround_kernels_vs_oracle_and_reference_known_answers states its tolerances."""
    w, d, z, a, gout = (c[k].double() for k in ("w", "delta", "zp", "alpha", "gout"))
    qmax = float(2 ** c["bits"] - 1)
    d, z = d.view(-1, 1), z.view(-1, 1)
    s = torch.sigmoid(a)
    r = s * 1.2 - 0.1
    h = r.clamp(0.0, 1.0)
    hmask = (r >= 0) & (r <= 1)
    dh = 1.2 * s * (1 - s)
    fl = torch.floor(quotient32(c["w"], c["delta"].view(-1, 1)).double())
    u = fl + h + z
    out = d * (u.clamp(0.0, qmax) - z)
    umask = (u >= 0) & (u <= qmax)
    g_open = gout * d * dh
    # a mask may differ from the kernel's where r is within ADA_DR of 0 or 1, or where u is within the rounding of the two fp32 additions
    # (2u·2^bits) of 0 or qmax without being on it through an exactly clamped h
    edge_r = ((r.abs() <= ADA_DR) | ((r - 1).abs() <= ADA_DR))
    du = 2 * U * (qmax + 1) + ADA_DR
    edge_u = ((u.abs() <= du) | ((u - qmax).abs() <= du)) & ~((h == 0) | (h == 1))
    reg = {}
    t = 2 * h - 1
    absd = t.abs()
    for b in b_list:
        terms = 1 - absd.pow(b)
        value = float(terms.sum())
        # per term: |t| moves by <= 2·ADA_DR + u (the clamp is 1-Lipschitz), |t|^b by b·|t|^(b−1) times that; powf to 2 ulp (4u relative);
        # 1 − p one rounding of a value <= 1
        dt = 2 * ADA_DR + U
        e_terms = float((b * (absd + dt).clamp_max(1.0).pow(b - 1) * dt + 4 * U * absd.pow(b) + U).sum())
        # the fixed tree: ceil(numel / 262144) sequential adds per thread, 6 shuffle levels, 2 LDS levels, then any order of the <= 1024
        # partials: no term passes through more than `depth` additions, so |fl(Σ) − Σ| <= γ_depth·Σ|terms| (Higham, Lemma 8.4 form)
        n = a.numel()
        blocks = min(1024, -(-n // 256))
        depth = -(-n // (blocks * 256)) + 6 + 2 + (blocks - 1)
        gamma = depth * U / (1 - depth * U)
        bound = e_terms + gamma * (value + e_terms)
        galpha_open = reg_weight * torch.where(absd > 0, -b * absd.pow(b - 1) * torch.sign(t) * 2 * dh, torch.zeros_like(t))
        galpha = torch.where(hmask, galpha_open, torch.zeros_like(t))
        reg[b] = dict(value=value, bound=bound, galpha=galpha, galpha_open=galpha_open, depth=depth)
    return dict(out=out, galpha=torch.where(hmask & umask, g_open, torch.zeros_like(g_open)), galpha_open=g_open,
                edge=edge_r | edge_u, edge_r=edge_r, reg=reg)


def weight_case(N=1280, K=2304, bits=4, with_alpha=False):
    """A weight above dgq_quantize_weight's 8192 x 256-thread grid (2 949 120 > 2 097 152), with ties of the quotient planted (w = (n + ½)·δ
    where that is exact) and α containing 0.0 and −0.0."""
    g = gen("weight", N, K, bits, with_alpha)
    w = torch.randn(N, K, generator=g) * 0.2
    lo, hi = w.min(1).values.clamp_max(0), w.max(1).values.clamp_min(0)
    delta = ((hi - lo) / (2 ** bits - 1)).clamp_min(1e-8)
    zp = torch.round(-lo / delta)
    zp[0], zp[1] = -3.0, float(2 ** bits + 2)
    sel = torch.rand(N, K, generator=g) < 0.05
    w = torch.where(sel, tie_lattice(delta.view(-1, 1).expand(N, K).contiguous(), g, nmax=2 ** (bits - 1)), w)
    alpha = None
    if with_alpha:
        alpha = torch.randn(N, K, generator=g)
        alpha[:, 0::11] = 0.0
        alpha[:, 1::11] = -0.0
        alpha.view(-1)[-2:] = torch.tensor([0.0, -0.0])
    return dict(w=w.contiguous(), delta=delta, zp=zp, alpha=alpha, bits=bits)


def quantize_weight_ref(c, rounding="even", recip=False, clamp_first=False):
    """uint8 codes: clamp(rne(fp32(w/δ_n)) + z_n, 0, 2^b − 1), or with α: clamp(floor(fp32(w/δ_n)) + [α >= 0] + z_n, 0, 2^b − 1)"""
    qmax = float(2 ** c["bits"] - 1)
    d, z = c["delta"].view(-1, 1), c["zp"].view(-1, 1)
    if c["alpha"] is None:
        return affine_codes(c["w"], d, z, qmax, rounding, recip, clamp_first).to(torch.uint8)
    r = torch.floor(quotient32(c["w"], d)) + (c["alpha"] >= 0).float()          # integers below 2^24: exact
    return torch.clamp((r.double() + z.double()).float(), 0.0, qmax).to(torch.uint8)
