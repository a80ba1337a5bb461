"""TEST INFRASTRUCTURE — a float64 reference of one quantised Linear / Conv2d layer (QuantLayer.forward: unfold -> activation
quantiser -> contraction with the dequantised weight) and the data recipes of tests/test_gpu_layer_routes.py.

Nothing here comes from ``dgq_amd``'s layer machinery: no ``plan_act``, no ``ActBinding``, no packed weight.  The activation tables go
in as a checkpoint stores them — ``(1, K, 1)`` / ``(1, 1, L)`` / scalar for a convolution (the quantiser sees the unfolded
``[B, C·kh·kw, L]`` operand), ``(1, 1, K)`` / ``(1, T, 1)`` / scalar for a Linear layer (input ``[B, T, K]``) — and the quantiser is
``oracle.dgq_oracle.uaq_codes``, the reference's own fp32 arithmetic (divide, round half to even, clamp).

``exact_case`` builds inputs on which every fp32 step of every kernel route is exact, so a GPU result must EQUAL the float64
formula; ``real_case`` builds ``torch.randn`` data under ``synth._group_params`` tables for the tolerance-based checks.
"""
import functools
import zlib

import torch
import torch.nn.functional as F

from oracle import dgq_oracle as orc

LAYOUTS = ("perK", "perM", "scalar")
G = 16                                   # DGQ groups of the per-K / per-M tables


# ----------------------------------------------------------------------------------------------- geometry
def conv_case(B, C, H, W, stride, N, k=3, upsample=False, variants=((8, 4),), gn=False, half=False):
    """H x W is the stored input; with ``upsample`` the layer sees its 2x nearest upsample."""
    name = "conv%dx%d_b%d_c%d_%dx%d_s%d_n%d%s" % (k, k, B, C, H, W, stride, N, "_ups" if upsample else "")
    return dict(name=name, kind="conv", B=B, C=C, H=H, W=W, stride=stride, N=N, k=k, pad=k // 2, upsample=upsample, variants=variants, gn=gn,
                half=half)


def linear_case(M, K, N, variants=((8, 4),), half=False):
    return dict(name="linear_m%d_k%d_n%d" % (M, K, N), kind="linear", M=M, K=K, N=N, variants=variants, half=half)


def geometry(case):
    """(B, H_in, W_in, Ho, Wo, M, K, taps) of the layer as it runs (H_in x W_in: behind the folded upsample)."""
    if case["kind"] == "linear":
        return 1, 1, 1, 1, case["M"], case["M"], case["K"], 1
    up = 2 if case["upsample"] else 1
    H, W, k, s, p = case["H"] * up, case["W"] * up, case["k"], case["stride"], case["pad"]
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    return case["B"], H, W, Ho, Wo, case["B"] * Ho * Wo, case["C"] * k * k, k * k


# ----------------------------------------------------------------------------------------------- the formula
def reference_codes(x, adelta, azp, abits, kind, k=1, stride=1, pad=0, upsample=False):
    """The integer codes (fp32, integer-valued) the layer's activation quantiser assigns: on x itself for a Linear layer, on the
    unfolded operand [B, C·k·k, L] for a convolution, for EVERY table shape (with 0 <= z <= 2^b − 1 the scalar case equals the
    reference's native F.conv2d(aqtizer(x)): a tap outside the image is 0.0 and takes the code z).  Also returns (Ho, Wo)."""
    if kind == "linear":
        return orc.uaq_codes(x, adelta, azp, abits), None
    if upsample:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    cols = F.unfold(x, kernel_size=k, dilation=1, padding=pad, stride=stride)
    Ho = (x.shape[2] + 2 * pad - k) // stride + 1
    Wo = (x.shape[3] + 2 * pad - k) // stride + 1
    return orc.uaq_codes(cols, adelta, azp, abits), (Ho, Wo)


def reference_layer(x, w_deq, bias, adelta, azp, abits, kind, k=1, stride=1, pad=0, residual=None, upsample=False):
    """y (float64) and the integer activation codes q of one quantised layer: the quantiser in the reference's fp32 arithmetic
    (``reference_codes``), the contraction with the dequantised weight, bias and residual in float64.
    Linear: x [B, T, K], w_deq [N, K] -> y [B, T, N], q [B, T, K].
    Conv:   x [B, C, H, W], w_deq [N, C, k, k] -> y [B, N, Ho, Wo], q [B, C·k·k, L] (F.unfold row order c·k·k + tap)."""
    q, out_hw = reference_codes(x, adelta, azp, abits, kind, k, stride, pad, upsample)
    deq = (adelta * (q - azp)).double()
    if kind == "linear":
        y = deq @ w_deq.double().t()
        if bias is not None:
            y = y + bias.double()
    else:
        y = (w_deq.reshape(w_deq.shape[0], -1).double() @ deq).view(x.shape[0], w_deq.shape[0], *out_hw)
        if bias is not None:
            y = y + bias.double().view(1, -1, 1, 1)
    if residual is not None:
        y = y + residual.double()
    return y, q


def reference_of(d, case, x=None):
    """``reference_layer`` on the tensors of a recipe dict (``x`` overrides the input: a prologue applied on the CPU)."""
    return reference_layer(d["x"] if x is None else x, d["w"], d["bias"], d["adelta"], d["azp"], d["abits"], case["kind"],
                           case.get("k", 1), case.get("stride", 1), case.get("pad", 0), d["residual"], case.get("upsample", False))


def codes_rows(q, case):
    """q of ``reference_layer`` as [M][K_ref] rows (row = (b, ho, wo) / (b, t); column = c·taps + tap)."""
    if case["kind"] == "linear":
        return q.reshape(-1, q.shape[-1])
    return q.permute(0, 2, 1).reshape(-1, q.shape[1])


# ----------------------------------------------------------------------------------------------- exact-integer recipe
#: ranges, widest first; ``exact_case`` takes the first under which its precondition holds (long K needs narrow ones).
#: xr: x = 2·randint(−xr, xr); dexp: activation scales 2^e; zstep: spacing of the in-range zero points around 2^(b−1);
#: wzr: weight zero points within ±wzr (W4; x8 for W8) of mid-range (wzabs: in that absolute range instead); wdexp: weight scales 2^e;
#: qwmax: weight codes in [0, qwmax] instead of the whole range; oor: share of K (or of the positions) kept in each of the two
#: groups whose zero point lies outside the code range
PROFILES = (dict(xr=4, dexp=(-2, -1, 0, 1), zstep=2, wzr=7, oor=1.0, wdexp=(-1, 0, 1), qwmax=None, wzabs=None),
            dict(xr=4, dexp=(-1, 0, 1), zstep=2, wzr=4, oor=1.0, wdexp=(-1, 0, 1), qwmax=None, wzabs=None),
            dict(xr=2, dexp=(-1, 0), zstep=1, wzr=2, oor=0.5, wdexp=(-1, 0), qwmax=None, wzabs=None),
            dict(xr=2, dexp=(-1, 0), zstep=1, wzr=1, oor=0.125, wdexp=(-1, 0), qwmax=None, wzabs=None),
            # a per-M table puts a whole ROW under an out-of-range zero point (every |s| near 2^(b−1)): the longest K then also
            # needs small weight codes and zero points
            dict(xr=2, dexp=(-1, 0), zstep=1, wzr=1, oor=0.125, wdexp=(-1, 0), qwmax=7, wzabs=(1, 2)),
            dict(xr=2, dexp=(-1, 0), zstep=1, wzr=1, oor=0.125, wdexp=(-1, 0), qwmax=3, wzabs=(1, 2)))
#: K above which the next narrower profile is taken, per-K tables / per-M and scalar tables
PROFILE_STEPS = dict(perK=(1500, 3000, 12000, 10 ** 9, 10 ** 9), perM=(600, 600, 3500, 3500, 12000), scalar=(10 ** 9,) * 5)
W8_SCALE = dict(perK=16, perM=4, scalar=1)              # W8 codes are 16x the W4 ones: the same steps at K x this
BIG = 400.0                               # |x| of the sparse lattice whose codes clamp at 0 / 2^b − 1
OOR_GROUPS = (3, 11)                      # group 3: z < 0, group 11: z > 2^b − 1


def _seed(*parts):
    return zlib.crc32("|".join(str(p) for p in parts).encode()) & 0x7FFFFFFF


def _build_tables(case, layout, abits, prof):
    """activation tables as a checkpoint stores them: G (δ, z) pairs, distinct through z; a seeded random label per K entry (per-K) or
    per position (per-M), i.e. non-contiguous groups; group 3 has z < 0, group 11 z > 2^b − 1, both present in every table"""
    g = torch.Generator().manual_seed(_seed("tables", case["name"], layout, abits))
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g)
    B, H, W, Ho, Wo, M, K, taps = geometry(case)
    lin = case["kind"] == "linear"
    mid = 2 ** (abits - 1)
    if layout == "scalar":
        return torch.tensor(2.0 ** max(prof["dexp"][0], -1)), torch.tensor(float(mid + 3))
    exps = torch.tensor(prof["dexp"])[ri(0, len(prof["dexp"]) - 1, (G,))]
    gd = (2.0 ** exps.double()).float()
    gz = (mid + prof["zstep"] * (torch.arange(G) - G // 2)).float()
    gz[OOR_GROUPS[0]] = -3.0
    gz[OOR_GROUPS[1]] = float(2 ** abits + 2)
    n_lab = K if layout == "perK" else (M if lin else Ho * Wo)
    labels = ri(0, G - 1, (n_lab,))
    if prof["oor"] < 1.0:                 # thin the two out-of-range groups: their codes all sit near ±2^(b−1)
        move = ((labels == OOR_GROUPS[0]) | (labels == OOR_GROUPS[1])) & (torch.rand(n_lab, generator=g) >= prof["oor"])
        labels = torch.where(move, labels + 1, labels)
    labels[0], labels[-1] = OOR_GROUPS
    shape = {("perK", True): (1, 1, -1), ("perM", True): (1, -1, 1), ("perK", False): (1, -1, 1), ("perM", False): (1, 1, -1)}[(layout, lin)]
    return gd[labels].view(shape), gz[labels].view(shape)


def _build_exact(case, layout, abits, wbits, prof):
    g = torch.Generator().manual_seed(_seed("exact", case["name"], layout, abits, wbits))
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g)
    B, H, W, Ho, Wo, M, K, taps = geometry(case)
    N = case["N"]
    lin = case["kind"] == "linear"
    x = (2 * ri(-prof["xr"], prof["xr"], (1, M, K) if lin else (B, case["C"], case["H"], case["W"]))).float()
    flat = x.view(-1)
    idx = torch.arange(7, flat.numel(), 61)
    flat[idx] = torch.where(idx % 2 == 0, torch.tensor(BIG), torch.tensor(-BIG))
    adelta, azp = _build_tables(case, layout, abits, prof)
    # ---- weights: w = wd_n·(q − wz_n) exactly, so the product's weight quantiser finds the codes q again
    qw = ri(0, 2 ** wbits - 1 if prof["qwmax"] is None else prof["qwmax"], (N, K))
    wd = (2.0 ** torch.tensor(prof["wdexp"])[ri(0, len(prof["wdexp"]) - 1, (N,))].double()).float()
    wzr = prof["wzr"] * (1 if wbits == 4 else 8)
    wz = (2 ** (wbits - 1) + ri(-wzr, wzr, (N,))).float() if prof["wzabs"] is None else ri(prof["wzabs"][0], prof["wzabs"][1], (N,)).float()
    w = wd[:, None] * (qw.float() - wz[:, None])
    wshape = (N, K) if lin else (N, case["C"], case["k"], case["k"])
    bias = ri(-8, 8, (N,)).float()
    residual = ri(-8, 8, (1, M, N) if lin else (B, N, Ho, Wo)).float()
    return dict(x=x, w=w.view(wshape), wdelta=wd.view((N,) + (1,) * (len(wshape) - 1)), wzp=wz.view((N,) + (1,) * (len(wshape) - 1)), qw=qw,
                bias=bias, residual=residual, adelta=adelta, azp=azp, abits=abits, wbits=wbits, layout=layout)


def exact_margin(d, case):
    """The precondition of the exact matrix, in int64 / float64 on the CPU.  Returns max over the output elements of
    (sum of term magnitudes) / (2^24 · unit); the data is exact under every route iff this is < 1.

    Every term any route forms is a multiple of one power-of-two unit per output element, u = min(δ_min·wd_n, 1) (per-K; δ_m·wd_n
    per-M / scalar; bias and residual are integers), and a fp32 sum of such terms is exact in ANY order while the sum of their
    magnitudes stays below 2^24·u.  With centred codes s = q − 2^(b−1), stored weight codes qw' (unsigned nibbles for W4, q − 128
    for W8) and zw' their zero point, the terms are
      per-K:  δ_k·s_k·qw'_k            bounded by 2·δ_max·Σ_k |s_k|·|qw'_k|, which also bounds Σ_c |coef_c·T_c| of the summation
                                        by parts over ANY chunk order, K split and clear segment (|T_c| <= Σ|s||qw'| of its
                                        segment, Σ_c |coef_c| <= 2·δ_max) — and is >= the plain Σ_k δ_k|s_k||qw'_k|;
              zw'_n·Σ_k δ_k·s_k        (the row sum the quantiser writes, Σ_k δ_k|s_k| itself being such a sum);
              U_n = Σ_k δ_k(o − z_k)(q − z)_nk      as magnitudes;
      per-M:  s_k·qw'_k, zw'_n·Σ_k s_k, (o − z_m)·vn_n with vn_n = Σ_k (q − z)_nk — integers, scaled by δ_m·wd_n at the end
    plus |bias_n| + |residual|.  Multiplying by wd_n (a power of two) never rounds."""
    abits, wbits, layout = d["abits"], d["wbits"], d["layout"]
    q, _ = reference_codes(d["x"], d["adelta"], d["azp"], abits, case["kind"], case.get("k", 1), case.get("stride", 1), case.get("pad", 0),
                           case.get("upsample", False))
    s = (codes_rows(q, case) - 2 ** (abits - 1)).double().abs()                       # [M][K]
    M, K = s.shape
    qw, wz, wd = d["qw"].double(), d["wzp"].reshape(-1).double(), d["wdelta"].reshape(-1).double()
    woff = 0.0 if wbits == 4 else 128.0
    qmag, zmag = (qw - woff).abs(), (wz - woff).abs()
    cen = qw - wz[:, None]
    o = float(2 ** (abits - 1))
    fixed = d["bias"].double().abs()[None, :] + d["residual"].double().abs().reshape(M, -1) if case["kind"] == "linear" else \
        d["bias"].double().abs()[None, :] + d["residual"].double().abs().permute(0, 2, 3, 1).reshape(M, -1)
    if layout == "perK":
        dk, zk = d["adelta"].reshape(-1).double(), d["azp"].reshape(-1).double()
        prod = 2.0 * dk.max() * (s @ qmag.t())
        rows = (s * dk[None, :]).sum(1)
        U = (cen.abs() * (dk * (o - zk).abs())[None, :]).sum(1)
        total = wd[None, :] * (prod + zmag[None, :] * rows[:, None] + U[None, :]) + fixed
        unit = torch.clamp(dk.min() * wd, max=1.0)[None, :]
        own = float(rows.max() / dk.min())                                             # the quantiser's own row sum Σ_k δ_k·s_k
    else:
        L = d["adelta"].numel()
        rows_idx = torch.arange(M) % L
        dm, zm = d["adelta"].reshape(-1).double()[rows_idx], d["azp"].reshape(-1).double()[rows_idx]
        vn = cen.sum(1).abs()
        inner = s @ qmag.t() + zmag[None, :] * s.sum(1)[:, None] + (o - zm).abs()[:, None] * vn[None, :]
        own = float(inner.max())                                                       # the integer stage before the scales
        total = dm[:, None] * wd[None, :] * inner + fixed
        unit = torch.clamp(dm[:, None] * wd[None, :], max=1.0)
    return max(float((total / unit).max()), own) / 2.0 ** 24


def profile_for(case, layout, abits, wbits):
    """index into PROFILES by the length of K: the ranges are chosen per K so that the precondition holds (exact_case asserts it)"""
    K = geometry(case)[6]
    scale = 1 if wbits == 4 else W8_SCALE[layout]
    return sum(1 for limit in PROFILE_STEPS[layout] if K * scale > limit)


@functools.lru_cache(maxsize=4)
def exact_case(case_name, layout, abits=8, wbits=4):
    """Exact-integer inputs of LAYER_CASES entry ``case_name`` in one table layout: dict(x, w, wdelta, wzp, bias, residual, adelta, azp,
    abits, wbits, layout, qw, margin, profile).  Asserts the precondition (``exact_margin`` < 1)."""
    case = CASES_BY_NAME[case_name]
    i = profile_for(case, layout, abits, wbits)
    d = _build_exact(case, layout, abits, wbits, PROFILES[i])
    d["margin"], d["profile"] = exact_margin(d, case), i
    assert d["margin"] < 1.0, ("%s/%s a%dw%d, profile %d: the term magnitudes reach %.3f x 2^24 units — the data would not be exact on every "
                               "route; narrow the ranges for this K (PROFILE_STEPS)" % (case_name, layout, abits, wbits, i, d["margin"]))
    return d


def exact_tables(case_name, layout, abits=8, wbits=4):
    """only the activation tables of ``exact_case`` (what the host planners need to name the route)"""
    case = CASES_BY_NAME[case_name]
    adelta, azp = _build_tables(case, layout, abits, PROFILES[profile_for(case, layout, abits, wbits)])
    return dict(adelta=adelta, azp=azp, layout=layout, abits=abits, wbits=wbits)


# ----------------------------------------------------------------------------------------------- real-valued recipe
def real_tables(case, layout, abits=8, wbits=4):
    """only the activation tables of ``real_case`` (what the host planners need to name the route)"""
    from dgq_amd import synth
    B, H, W, Ho, Wo, M, K, taps = geometry(case)
    lin = case["kind"] == "linear"
    if layout == "scalar":
        adelta, azp = torch.tensor(0.031), torch.tensor(float(2 ** (abits - 1) + 5))
    else:
        n = K if layout == "perK" else (M if lin else Ho * Wo)
        dl, zp = synth._group_params(n, G, abits, "layer_routes|%s|%s" % (case["name"], layout), 0)
        shape = {("perK", True): (1, 1, -1), ("perM", True): (1, -1, 1), ("perK", False): (1, -1, 1), ("perM", False): (1, 1, -1)}[(layout, lin)]
        adelta, azp = dl.view(shape), zp.view(shape)
    return dict(adelta=adelta, azp=azp, layout=layout, abits=abits, wbits=wbits)


def real_case(case, layout, abits=8, wbits=4):
    """The same shapes with torch.randn data under synth._group_params / synth.channel_minmax tables (as the F3 recipes do)."""
    from dgq_amd import synth
    g = torch.Generator().manual_seed(_seed("real", case["name"], layout, abits, wbits))
    B, H, W, Ho, Wo, M, K, taps = geometry(case)
    N = case["N"]
    lin = case["kind"] == "linear"
    x = torch.randn((1, M, K) if lin else (B, case["C"], case["H"], case["W"]), generator=g) * 1.3 + 0.2
    w = torch.randn((N, K) if lin else (N, case["C"], case["k"], case["k"]), generator=g) * K ** -0.5
    wd, wz = synth.channel_minmax(w, wbits)
    w_deq = orc.uaq(w, wd, wz, wbits)
    t = real_tables(case, layout, abits, wbits)
    adelta, azp = t["adelta"], t["azp"]
    bias = torch.randn(N, generator=g) * 0.1
    residual = torch.randn((1, M, N) if lin else (B, N, Ho, Wo), generator=g)
    return dict(x=x, w_raw=w, w=w_deq, wdelta=wd, wzp=wz, bias=bias, residual=residual, adelta=adelta, azp=azp, abits=abits, wbits=wbits,
                layout=layout)


# ----------------------------------------------------------------------------------------------- the layer cases
_A6W8 = ((8, 4), (6, 4), (8, 8))
#: the quantised layers of an SD step at 64 x 64 and 32 x 32 latents (and the small end), by the route they take — see
#: tests/test_gpu_layer_routes.py::test_route_table_is_complete for the table the planners make of it.  B = 1 where the route does not
#: depend on the batch (the float64 reference is the cost of a case).
LAYER_CASES = [
    conv_case(2, 32, 9, 9, 1, 24, variants=_A6W8),                       # the F3 fixture geometry
    conv_case(2, 64, 64, 64, 1, 64, gn=True, half=True, variants=_A6W8),
    conv_case(2, 128, 64, 64, 1, 128),
    conv_case(2, 320, 64, 64, 1, 320, gn=True, half=True),               # quantiser inside the GEMM launch
    conv_case(2, 320, 32, 32, 1, 640),
    conv_case(2, 320, 64, 64, 2, 320),
    conv_case(2, 640, 32, 32, 1, 640, gn=True, half=True),
    conv_case(1, 640, 64, 64, 1, 320),
    conv_case(1, 960, 64, 64, 1, 320),
    conv_case(2, 960, 32, 32, 1, 640),
    conv_case(2, 1280, 32, 32, 1, 640),
    conv_case(2, 640, 16, 16, 1, 1280, gn=True, half=True),
    conv_case(2, 640, 32, 32, 2, 640),
    conv_case(2, 1280, 16, 16, 1, 1280),
    conv_case(2, 1280, 8, 8, 1, 1280),
    conv_case(2, 1920, 16, 16, 1, 1280),
    conv_case(2, 2560, 16, 16, 1, 1280),
    conv_case(2, 2560, 8, 8, 1, 1280),
    conv_case(2, 1920, 32, 32, 1, 640),
    conv_case(2, 320, 46, 90, 1, 320, gn=True),                          # ragged: partial tiles on both edges
    conv_case(2, 64, 46, 90, 1, 64),
    conv_case(2, 320, 63, 63, 2, 320),
    conv_case(2, 128, 46, 90, 2, 128),
    conv_case(2, 320, 64, 64, 1, 320, k=1),
    conv_case(2, 1280, 16, 16, 1, 1280, k=1),
    conv_case(2, 640, 32, 32, 1, 640, upsample=True),
    conv_case(2, 1280, 8, 8, 1, 1280, upsample=True),
    linear_case(8192, 320, 320, half=True),
    linear_case(8192, 320, 2560),
    linear_case(8192, 1280, 320),
    linear_case(2048, 640, 640),
    linear_case(2048, 2560, 640),
    linear_case(512, 1280, 1280),
    linear_case(512, 5120, 1280),
    linear_case(154, 768, 320, variants=_A6W8),
    linear_case(2, 1280, 1280),
]
#: shapes only the real-valued prologue tests use (no cell of the exact matrix)
PROLOGUE_ONLY_CASES = [linear_case(2048, 1280, 320)]                     # the input of a GEGLU feed-forward at the 32 x 32 level
CASES_BY_NAME = {c["name"]: c for c in LAYER_CASES + PROLOGUE_ONLY_CASES}
assert len(CASES_BY_NAME) == len(LAYER_CASES) + len(PROLOGUE_ONLY_CASES)


def exact_params():
    """(case name, layout, abits, wbits) of every cell of the exact matrix"""
    return [(c["name"], lay, ab, wb) for c in LAYER_CASES for lay in LAYOUTS for (ab, wb) in c["variants"]]
