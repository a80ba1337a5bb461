"""CPU side of tests/test_gpu_attention_quant.py and tests/test_attention_quant_ref_cpu.py: adversarial operands on quantiser grids, the
float64 statement of the quantised attention (sd.py:165-201: scores·scale -> softmax -> aqtizer_w with the start-peak column bypassed ->
@ v), its tie-aware a-priori bound, and a plain fp32 restatement that stands in for the kernels on the CPU.  Nothing here imports the
extension.  Tensors are in the projection layout q [B][T][H·D], k / v [B][S][H·D].

Operands.  Every value is n·2^-3 with an integer |n| <= 50, so it lies on every quantiser grid x = δ·(c − z) whose step δ is 2^-3 or 2^-4
and whose zero point z is an integer in [126, 130] (8-bit codes 26 .. 230): aqtizer_q/k/v with such tables are the identity, and float64
sees exactly the operands every operand format of the kernels sees.  The tables themselves vary from entry to entry (``table``).

The statement.  With s2 = scale·(q·k)·log2 e, m2 = max_j s2, l = Σ_j 2^(s2 − m2), p = 2^(s2 − m2)/l and δ (mode 1: the maximum of
p[..., skip:] over the whole call; modes 2, 3: given) the quantiser's argument is
    y = (m2 − s2) + log2 l + log2 δ = −log2(p/δ)   (modes 1, 2)          y = p/δ   (mode 3),
code = clamp(rne(y), 0, 2^bits − 1) and p̂ = δ·2^-code or δ·code.  Columns below ``skip`` (and every column of mode 0) keep p.

The bound (``Ref.bound``), per output element, u = 2^-24:
    |o − o64| <= Σ_{j ambiguous} |p̂_alt,j − p̂_j|·|v_jd| + Σ_{j un-quantised} ε_p,j·p_j·|v_jd| + ε·A'_td + 2^-126·Σ_j |v_jd|.
* An entry is ambiguous when y lies within τ of a rounding tie (a half-integer); p̂_alt is what the code on the other side of that tie
  gives (equal to p̂ where both sides clamp to the same code).  τ is the fp32 error of a device's y, in the units of y:
    τ_log = E2_j + u·(4|m2 − s2| + 4|m2| + 4|log2 l| + 4|log2 δ| + 2|y| + 2(NT + 20) + 4·log2 S)  [+ τ_δ in mode 1]
    τ_uni = y·(ln 2·τ_log + 6u)
  - y_j = −s2_j + log2 Σ_i 2^(s2_i) + log2 δ does not depend on the value of the maximum, so score errors e_i (log2 units, |e_i| <=
    E_i·log2 e) move it by −e_j + Σ_i p_i·e_i to first order: E2_j = ((1 − p_j)·E_j + Σ_{i != j} p_i·E_i)·log2 e.  (With one E per row,
    as attention_mfma16_ref takes it, this is 2·E·log2 e; per key it is tighter where one key carries the row, whose own error
    cancels.)  E_i is the error of score i in nats.  bf16x3 / fp32 products: E_i = (D + 8)·u·scale·Σ_d |q_d||k_id|, the sum of
    attention_mfma16_ref.ref64 (D accumulations, the scale product and the log2 e factor; the six kept
    products of the three-term split are exact, the dropped ones are below u of the leading one).  Where an int8 contraction forms
    Σ c'q·c'k exactly (QM 1, 3), E_i = 4·u·scale·Σ_d (|q_d| + δq|z'q|)(|k_id| + δk|z'k|): the three fp32 operations of the
    zero-point algebra and the scale product, each at the magnitude of the CENTRED codes c' = c − 128, z' = z − 128.  QM 2 contracts
    centred Q codes with three K planes: the bf16x3 form with |q_d| + δq|z'q| in place of |q_d|.
  - 4|m2 − s2|: the log2 scale sl2 = scale·log2 e·δq·δk carries three roundings and the constant's; the row maximum and the score are
    multiplied by the same sl2, so this relative error acts on their difference.
  - 4|m2|: m = fl(mraw·sl2), the two additions of a0 = m + log2 l + log2 δ are rounded at the magnitude of m, and a key split merges two
    maxima once more.  (This is what a common shift of a row's scores costs in fp32: softmax does not change under it, its fp32 evaluation does.)
  - 4|log2 l|, 4|log2 δ|: log2f to 2 ulp and the additions above.  2|y|: the final fma and the magic-number add.
  - 2(NT + 20): l is a sum of 16 terms per lane, NT tiles, two half-waves and at most two key halves in fp32: relative error
    (NT + 20)·u, that is < 2(NT + 20)·u in log2 units.  4·log2 S: the sl2 error inside l's terms, Σ_j p_j·4u·|m2 − s2_j| = 4u·(H2(p) −
    log2 l) <= 4u·log2 S.
  - τ_δ (mode 1): δ_dev = 2^(m2' − m2)/l of the owning row: its log2 carries that entry's own τ_log (without the δ terms) and one
    division (2u).
  - mode 3 forms p/δ as ONE exponential of the same argument (interior tiles) or as exp2·(1/l)/δ: relative error ln 2·τ_log + 6u.
* ε_p = ln 2·τ_log + 6u (τ_log without the δ terms) is the relative error of an un-quantised probability.
* ε = (S + 16)·u + 2u [+ ln 2·τ_δ in mode 1]: the fp32 accumulation of P̂·V over S keys and the epilogue's products (worst case), the
  three-term split of a V that is not integer (exact to 24 bits: u) and the final δ product (u), the relative error of δ.
  A' = Σ_j p̂_j·(|v_jd| + δv|z'v_d|): integer-V formats accumulate centred codes and subtract z'v·Σp̂, so their roundings are at that size.
* 2^-126·Σ|v|: log codes above 127 give δ·2^-code < 2^-127, which a device may flush to zero or clamp at 2^-127 (δ <= 1).
No constant above was set by looking at a kernel's output."""
import functools
import math

import torch

U = 2.0 ** -24
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
STEP = 0.125          # 2^-3
KT = 32               # keys per tile of every kernel of the family
B = 2


def heads(x, H, D):
    """[B][N][H·D] -> [B][H][N][D]"""
    return x.view(x.shape[0], x.shape[1], H, D).transpose(1, 2)


def unheads(x):
    """[B][H][T][D] -> [B][T][H·D]"""
    return x.transpose(1, 2).reshape(x.shape[0], x.shape[2], -1)


# ------------------------------------------------------------------------------------------------------------------ operand formats
class Format:
    """one way of feeding the same tensors: the fq modes of q, k, v (None: not fused; 0 scalar, 1 per token, 2 per head-dim element) and
    what that makes of the score products (``kind``: bf = bf16x3 products, i8 = int8 contraction, q1 = centred Q plane x three K planes)"""

    def __init__(self, name, qm, km, vm, kind):
        self.name, self.qm, self.km, self.vm, self.kind = name, qm, km, vm, kind
        self.vint = vm in (0, 2)

    def __repr__(self):
        return self.name


FORMATS = {f.name: f for f in (
    Format("unfused", None, None, None, "bf"),     # fq=None
    Format("qm0", None, 1, 1, "bf"),               # QM 0: q not fused, bf16x3 products, three-plane V
    Format("qm0v", None, 2, 2, "bf"),              # QM 0 with the single integer V plane
    Format("qm1", 1, 1, 2, "i8"),                  # QM 1: per-token k table, integer V (per head-dim table)
    Format("qm3", 0, 0, 1, "i8"),                  # QM 3: scalar k table, three-plane V
    Format("qm3v", 1, 0, 0, "i8"),                 # QM 3 with the integer V plane (scalar table)
    Format("qm2", 2, 1, 1, "q1"),                  # QM 2: per-head-dim q table
    Format("qm2v", 1, 2, 2, "q1"),                 # QM 2 through a per-head-dim K table, integer V
)}
FUSED = [n for n in FORMATS if n != "unfused"]
ZLO, ZSPAN = 126, 5


def table(mode, ntok, D, seed, e=3, centred=False):
    """(δ, z) of a quantiser table of the given mode: δ alternates between 2^-e and 2^-(e+1), z walks through 126 .. 130 (``centred``:
    z = 128 throughout)"""
    n = 1 if mode == 0 else (ntok if mode == 1 else D)
    i = torch.arange(n)
    d = torch.where((i + seed) % 2 == 0, 2.0 ** -e, 2.0 ** -(e + 1)).float()
    z = torch.full((n,), 128.0) if centred else (ZLO + (3 * i + seed) % ZSPAN).float()
    return d, z


def fq_tables(fmt, T, S, D, skip, v_exp=3):
    """the ``fq`` argument of ops.attention on the CPU (None for the un-fused format): (mode, δ, z, skip, 8) per operand; the k table
    bypasses the start-peak key as aqtizer_k does (sd.py:176-180).  ``v_exp=0`` is the table of the one-hot read-out window: steps 1 and
    1/2 around z = 128, so that a zero of v is the centred code 0 and the integer-V formats add exact zeros."""
    if fmt.name == "unfused":
        return None
    out = []
    for i, (m, n, sk, e) in enumerate(((fmt.qm, T, 0, 3), (fmt.km, S, skip, 3), (fmt.vm, S, 0, v_exp))):
        out.append(None if m is None else (m,) + table(m, n - sk, D, 5 * i + 1, e, centred=(i == 2 and v_exp == 0)) + (sk, 8))
    return tuple(out)


PAD = STEP * 2.0          # δ·|z − 128| <= 2^-3·2


# ------------------------------------------------------------------------------------------------------------------ data families
class Case:
    """q, k, v: what the kernel is given.  q_ref, k_ref: what float64 is given (the un-shifted tensors of ``row_offsets``; else q, k)."""

    def __init__(self, family, shape, q, k, v, scale, q_ref=None, k_ref=None, **info):
        self.family, self.shape, self.q, self.k, self.v, self.scale = family, shape, q, k, v, scale
        self.q_ref = q if q_ref is None else q_ref
        self.k_ref = k if k_ref is None else k_ref
        self.info = info


def _grid(shape, g, amp):
    """grid-uniform values n·2^-3, |n| <= amp/2^-3"""
    n = int(round(amp / STEP))
    return torch.randint(-n, n + 1, shape, generator=g).float() * STEP


def _boost(D, scale, nats, nd=None):
    """k values on the grid for nd leading head-dim elements (|value| <= 6.25) that give 6·Σ·scale = nats to within 6·scale·2^-4 against
    q = 6 there: the total number of grid steps is rounded once and dealt out over the elements"""
    if nd is None:
        nd = max(1, math.ceil(abs(nats) / (36.0 * scale)))
    if nd > D - 2:
        raise ValueError("%g nats need %d of %d head-dim elements" % (nats, nd, D))
    steps = int(round(nats / (6.0 * scale * STEP)))
    base, extra = divmod(abs(steps), nd)
    kv = torch.full((nd,), float(base)) + (torch.arange(nd) < extra).float()
    assert float(kv.max()) <= 50
    return kv * (STEP if steps >= 0 else -STEP)


FAMILIES = ("random", "start_peak", "late_peak", "staircase_up", "staircase_down", "staircase_mid", "row_offsets", "row_offsets_deep",
            "uniform", "delta_owner")


@functools.lru_cache(maxsize=None)
def make(family, shape):
    """the operands of one (family, (D, T, S, H, B)): computed once and shared — do not modify the tensors"""
    D, T, S, H, Bn = shape
    scale = float(torch.tensor(D ** -0.5, dtype=torch.float32))
    g = torch.Generator().manual_seed(1000 * D + 7 * T + S + H + 13 * FAMILIES.index(family))
    NT = (S + KT - 1) // KT
    q = _grid((Bn, T, H, D), g, 1.0 if family == "delta_owner" else 2.0)
    k = _grid((Bn, S, H, D), g, 1.0 if family == "delta_owner" else 2.0)
    v = _grid((Bn, S, H, D), g, 2.0)
    q_ref = k_ref = None
    info = {}
    flat = lambda x: x.reshape(x.shape[0], x.shape[1], H * D).contiguous()
    if family in ("start_peak", "late_peak"):
        key = 0 if family == "start_peak" else S - 1
        kv = _boost(D, scale, 18.0)
        nd = kv.numel()
        q[..., :nd] = 6.0
        k[..., :nd] = 0.0
        k[:, key] = 0.0
        k[:, key, :, :nd] = kv
        info = dict(key=key)
    elif family.startswith("staircase"):
        # one key per tile carries the tile's maximum: level 8·(g + 1) nats (up), 8·(NT − g) (down), or a roof whose top is tile NT // 2
        top = NT // 2
        level = {"staircase_up": lambda t: 8.0 * (t + 1), "staircase_down": lambda t: 8.0 * (NT - t),
                 "staircase_mid": lambda t: 8.0 * (max(top, NT - 1 - top) + 1 - abs(t - top))}[family]
        nd = _boost(D, scale, max(level(t) for t in range(NT))).numel()
        q[..., :nd] = 6.0
        k[..., :nd] = 0.0
        keys = []
        for t in range(NT):
            j = KT * t + (5 * t + 3) % min(KT, S - KT * t)
            k[:, j] = 0.0
            k[:, j, :, :nd] = _boost(D, scale, level(t), nd)
            keys.append(j)
        info = dict(keys=keys, top=top)
    elif family.startswith("row_offsets"):
        nats = 40.0 if family == "row_offsets" else 120.0
        kv = _boost(D, scale, nats)
        nd = kv.numel()
        q[..., :nd] = 0.0
        k[..., :nd] = kv                                   # the component common to every key
        q_ref, k_ref = flat(q.clone()), flat(k)
        sign = torch.where(torch.arange(T) % 2 == 0, 1.0, -1.0).view(1, T, 1, 1)
        q[..., :nd] = 6.0 * sign
        info = dict(shift=6.0 * float(kv.sum()) * scale)
    elif family == "uniform":
        # attention_mfma16_ref.uniform_case: v = c_d + (−1)^j (c_d alone for a last odd key), so Σ_j v_jd = S·c_d exactly
        q.zero_()
        c = ((torch.arange(D) % 7) - 3).float()
        sign = torch.where(torch.arange(S) % 2 == 0, 1.0, -1.0)
        sign[2 * (S // 2):] = 0.0
        v = (c.view(1, 1, 1, D) + sign.view(1, S, 1, 1)).expand(Bn, S, H, D).contiguous()
        info = dict(c=c)
    elif family == "delta_owner":
        # the last row of the last (batch, head) meets one key >= 1 that takes all of its mass
        kv = _boost(D, scale, 14.0)
        nd = kv.numel()
        key = max(1, (S // 2) | 1) if S > 1 else 0
        q[..., :nd] = 0.0
        q[Bn - 1, T - 1, H - 1, :nd] = 6.0
        k[Bn - 1, :, H - 1, :nd] = 0.0
        k[Bn - 1, key, H - 1, :] = 0.0
        k[Bn - 1, key, H - 1, :nd] = kv
        info = dict(key=key, row=(Bn - 1, H - 1, T - 1))
    elif family != "random":
        raise ValueError(family)
    assert float(q.abs().max()) <= 50 * STEP and float(k.abs().max()) <= 50 * STEP and float(v.abs().max()) <= 50 * STEP
    return Case(family, shape, flat(q), flat(k), flat(v), scale, q_ref, k_ref, **info)


def onehot_v(shape, j0):
    """the read-out window: v[j, d] = 1 where d == j − j0 (j0 <= j < j0 + D), 0 elsewhere; then o[t, d] = p̂[t, j0 + d] exactly"""
    D, T, S, H, Bn = shape
    v = torch.zeros(Bn, S, H, D)
    for d in range(D):
        if 0 <= j0 + d < S:
            v[:, j0 + d, :, d] = 1.0
    return v.reshape(Bn, S, H * D).contiguous()


# ------------------------------------------------------------------------------------------------------------------ float64
class Ref:
    """what ``ref64`` returns, all [B][H][T][S] float64 unless noted: p, y (formed for every column; only the quantised ones use it), code, alt (the code on the
    other side of the nearest tie), dist (to that tie), tau, amb = dist <= tau, phat, palt, eps_p; delta (float), tau_delta, eps"""

    def output(self, v, H, D):
        """float64 o of the statement for this v [B][S][H·D]"""
        return unheads(torch.matmul(self.phat, heads(v.double(), H, D)))

    def bound(self, v, H, D, fmt=FORMATS["unfused"], v_exp=3):
        """the per-element bound of the module docstring for this v"""
        va = heads(v.double(), H, D).abs()
        pad = 0.0
        if fmt.vint:
            d, z = table(fmt.vm, v.shape[1], D, 11, v_exp)
            pad = (d.double() * (z.double() - 128.0).abs()).max()
        amb = torch.matmul(torch.where(self.amb, (self.palt - self.phat).abs(), torch.zeros(())), va)
        unq = torch.matmul(self.eps_p * self.p, va) if self.eps_p is not None else 0.0
        A = torch.matmul(self.phat, va + pad)
        return unheads(amb + unq + self.eps * A + 2.0 ** -126 * va.sum(-2, keepdim=True))


def _tau_log(E2, dsm, m2, log2l, log2d, y, NT, S):
    return E2 + U * (4.0 * dsm + 4.0 * m2.abs() + 4.0 * log2l.abs() + 4.0 * abs(log2d) + 2.0 * y.abs() + 2.0 * (NT + 20) + 4.0 * math.log2(max(S, 2)))


def ref64(case, mode, skip, bits, delta=None, fmt=FORMATS["unfused"]):
    """the statement in float64 on case.q_ref / case.k_ref.  ``delta``: the static δ of modes 2 and 3 (a float that fp32 holds exactly)"""
    D, T, S, H, Bn = case.shape
    NT = (S + KT - 1) // KT
    qh, kh = heads(case.q_ref.double(), H, D), heads(case.k_ref.double(), H, D)
    qa, ka = qh.abs(), kh.abs()
    if fmt.kind == "i8":
        qa, ka, nround = qa + PAD, ka + PAD, 4.0
    else:
        qa, nround = (qa + PAD if fmt.kind == "q1" else qa), D + 8.0
    Ej = (nround * U * abs(case.scale) * LOG2E) * torch.matmul(qa, ka.transpose(-2, -1))          # per score, in log2 units
    s2 = torch.matmul(qh, kh.transpose(-2, -1)) * (case.scale * LOG2E)
    m2 = s2.amax(-1, keepdim=True)
    dsm = m2 - s2
    e = torch.exp2(-dsm)
    l = e.sum(-1, keepdim=True)
    log2l = torch.log2(l)
    r = Ref()
    r.p = e / l
    E2 = Ej + (r.p * Ej).sum(-1, keepdim=True) - 2.0 * r.p * Ej                                  # (1 − p_j)·E_j + Σ_{i != j} p_i·E_i
    qmax = float(2 ** bits - 1)
    zero = torch.zeros(())
    tau_p = _tau_log(E2, dsm, m2, log2l, 0.0, dsm + log2l, NT, S)             # τ of −log2 p: no δ terms
    r.tau_delta, r.delta = 0.0, delta
    col = torch.arange(S) >= (S if mode == 0 else skip)                       # quantised columns
    r.eps_p = torch.where(col, zero, LN2 * tau_p + 6.0 * U) if not bool(col.all()) else None
    if mode == 0:
        r.y = r.code = r.alt = r.dist = r.tau = None
        r.amb = torch.zeros_like(r.p, dtype=torch.bool)
        r.phat = r.palt = r.p
        r.eps = (S + 18.0) * U
        return r
    if mode == 1:
        pq = r.p[..., skip:]
        idx = int(pq.argmax())
        r.delta = float(pq.reshape(-1)[idx])
        r.tau_delta = float(tau_p[..., skip:].reshape(-1)[idx]) + 2.0 * U
    log2d = math.log2(r.delta)
    y_log = dsm + log2l + log2d
    tau_log = tau_p + U * 4.0 * abs(log2d) + 2.0 * U * abs(log2d) + r.tau_delta      # (2|y| grows by at most 2|log2 δ|)
    if mode == 3:
        r.y = r.p / r.delta
        r.tau = r.y * (LN2 * tau_log + 6.0 * U)
    else:
        r.y, r.tau = y_log, tau_log
    fl = torch.floor(r.y)
    raw = torch.round(r.y)                                                       # rne, as rintf and the magic-number add
    r.code = raw.clamp(0.0, qmax)
    r.alt = torch.where(raw == fl, fl + 1.0, fl).clamp(0.0, qmax)
    r.dist = (r.y - (fl + 0.5)).abs()
    deq = (lambda c: r.delta * torch.exp2(-c)) if mode != 3 else (lambda c: r.delta * c)
    r.phat = torch.where(col, deq(r.code), r.p)
    r.palt = torch.where(col, deq(r.alt), r.p)
    r.amb = (r.dist <= r.tau) & col & (r.alt != r.code)
    r.eps = (S + 18.0) * U + LN2 * r.tau_delta
    return r


def worst_ratio(o, o64, bound):
    """max |o − o64| / bound; inf where o is not finite"""
    if not bool(torch.isfinite(o).all()):
        return math.inf
    return float(((o.double() - o64).abs() / bound.clamp_min(1e-300)).max())


def static_delta(case, mode, skip):
    """the static δ of the two 6-bit settings, from the float64 probabilities (a float that fp32 holds): mode 2: an eighth of the largest
    quantised probability, so the head of every row sits in the lower clamp (−log2(p/δ) < 0); mode 3: 1/200 of it, so it lies above
    qmax = 63"""
    D, T, S, H, Bn = case.shape
    p = torch.softmax(torch.matmul(heads(case.q_ref.double(), H, D), heads(case.k_ref.double(), H, D).transpose(-2, -1)) * case.scale, -1)
    pm = float(p[..., skip:].max())
    return float(torch.tensor(pm * (0.125 if mode == 2 else 0.005), dtype=torch.float32))


# ------------------------------------------------------------------------------------------------------------------ restatement
MISTAKES = ("codes_off_by_one", "delta_over_all_keys", "column0_quantised", "last_key_dropped", "pad_key_scores_zero", "max_starts_at_zero",
            "max_shared_by_row_pairs", "delta_of_batch0", "stale_delta")


def restatement(case, mode, skip, bits, delta=None, v=None, mistake=None):
    """the statement in fp32 torch on case.q / case.k (the tensors a kernel is given), tile by tile: pass 1 keeps an online maximum and
    sum per row and takes the real-time δ; pass 2 recomputes the scores, quantises with the final (m, l, δ) and accumulates p̂·v.
    ``mistake`` plants one of MISTAKES."""
    D, T, S, H, Bn = case.shape
    assert mistake is None or mistake in MISTAKES
    qh, kh, vh = (heads(x.float(), H, D) for x in (case.q, case.k, case.v if v is None else v))
    Se = S - 1 if mistake == "last_key_dropped" else S
    scale = torch.tensor(case.scale, dtype=torch.float32)
    qmax = float(2 ** bits - 1)

    def tile(s0):
        s = torch.matmul(qh, kh[:, :, s0:min(s0 + KT, Se)].transpose(-2, -1)) * scale
        if mistake == "pad_key_scores_zero" and s0 + KT > Se:
            s = torch.cat([s, torch.zeros(Bn, H, T, 1)], -1)                      # key S of the ragged tile counted with a zero score
        return s
    m = torch.full((Bn, H, T, 1), 0.0 if mistake == "max_starts_at_zero" else -math.inf)
    l = torch.zeros(Bn, H, T, 1)
    ms = torch.full((Bn, H, T, 1), -math.inf)
    for s0 in range(0, Se, KT):
        s = tile(s0)
        mn = torch.maximum(m, s.amax(-1, keepdim=True))
        l = l * torch.exp(m - mn) + torch.exp(s - mn).sum(-1, keepdim=True)
        m = mn
        lo = 0 if mistake == "delta_over_all_keys" else max(skip - s0, 0)
        if lo < min(KT, Se - s0):
            ms = torch.maximum(ms, s[..., lo:min(KT, Se - s0)].amax(-1, keepdim=True))
    if mistake == "max_shared_by_row_pairs":                                    # rows 2i and 2i + 1 use the larger of their maxima
        pair = torch.arange(T) ^ 1
        pair[pair >= T] = T - 1
        mo = torch.maximum(m, m[:, :, pair])
        l = l * torch.exp(m - mo)
        m = mo
    d = None
    if mode == 1:
        pm = torch.exp(ms - m) / l
        d = pm.amax((1, 2, 3), keepdim=True)                                    # per batch item, then over the batch
        d = d[:1].expand_as(d) if mistake == "delta_of_batch0" else d.amax(0, keepdim=True).expand_as(d)
    elif mode >= 2:
        d = torch.full((Bn, 1, 1, 1), delta, dtype=torch.float32)
    if mistake == "stale_delta":
        d = d * 0.5
    acc, accb = torch.zeros(Bn, H, T, D), torch.zeros(Bn, H, T, D)             # Σ (p̂/δ)·v — δ multiplies once at the end — and Σ p·v
    for s0 in range(0, Se, KT):
        s = tile(s0)[..., :min(KT, Se - s0)]
        p = torch.exp(s - m) / l
        vt = vh[:, :, s0:s0 + p.shape[-1]]
        if mode == 0:
            accb = accb + torch.matmul(p, vt)
            continue
        if mode == 3:
            code = torch.clamp(torch.round(p / d), 0.0, qmax)
        else:
            code = torch.clamp(torch.round((m - s) * LOG2E + torch.log2(l) + torch.log2(d)), 0.0, qmax)
        if mistake == "codes_off_by_one":                                      # every 100th entry
            n = torch.arange(code.numel()).view(code.shape)
            code = torch.where((n * 7 + s0) % 100 == 0, code + 1.0, code).clamp(0.0, qmax)
        ph = code if mode == 3 else torch.exp2(-code)
        if mistake != "column0_quantised" and s0 < skip:
            ph[..., :skip - s0] = 0.0
            accb = accb + torch.matmul(p[..., :skip - s0], vt[:, :, :skip - s0])
        acc = acc + torch.matmul(ph, vt)
    return unheads(acc * d + accb if mode else accb)


# ------------------------------------------------------------------------------------------------------------------ the GPU module's cases
#: the probability quantisers (mode, skip, bits) of the interval check
QUANTS = [(1, 0, 8), (1, 1, 8), (2, 1, 6), (3, 0, 6)]
#: launch forms: what DGQ_ATTN_ONE / DGQ_ATTN_SPLIT are set to (None: unset)
FORMS = {"w4": ("0", "0"), "one": (None, None), "split": ("0", "100000"), "wide": ("0", "0")}


def _cases():
    """(form, format, family, (D, T, S, H, B), (mode, skip, bits)) of the interval check.  Shapes, by form:
    w4    4-wave, un-split: every head dim; S = 1, 2 (half-waves without a key), 31 / 32 / 33 (one tile, ragged or full, one key past it),
          77, 257 (a single key in the last tile; NT = 9); T = 1, 33, 127 / 129 (either side of the 128-row workgroup), 200
    one   one launch: NT <= 8 and a fused format with q quantised, D in 40 / 64 / 80 / 160; T = 129 .. 300 gives two or three workgroups
          along T, whose δ has to be exchanged; S = 256 is the longest key range, 250 its ragged neighbour
    split key split: NT >= 8; S = 225 (NT = 8, halves of 4 tiles, the last holds one key), 257 (NT = 9: halves of 4 and 5), 300 (NT = 10)
    wide  8 waves: D <= 64 and ceil(T/256)·B·H >= 256; S = 77, 257: NT odd, one tile per stage; S = 256, 320: NT even and >= 8, two"""
    out = []
    qi = [0]

    def add(form, fmt, family, shape, quant=None):
        if quant is None:
            quant = QUANTS[qi[0] % len(QUANTS)]
            qi[0] += 1
        out.append((form, fmt, family, shape, quant))
    fam = ["random", "start_peak", "late_peak", "staircase_up", "staircase_down", "row_offsets", "row_offsets_deep", "uniform", "delta_owner"]
    # ---- w4: every D, S, T value of the table once, on random data, formats rotating
    w4_shapes = [(8, 1, 1, 2, B), (16, 33, 2, 2, B), (40, 127, 31, 2, B), (64, 129, 32, 2, B), (80, 200, 33, 2, B), (160, 33, 77, 2, B), (40, 129, 257, 2, B)]
    names = list(FORMATS)
    for i, sh in enumerate(w4_shapes):
        add("w4", names[i % len(names)], "random", sh)
    # ---- every family on every form; late_peak needs S % 32 == 1, staircases two tiles or more, delta_owner a ragged last query block
    per_form = {
        "w4": {"late_peak": (40, 129, 33, 2, B), "row_offsets_deep": (64, 129, 77, 2, B), None: (80, 200, 77, 2, B)},
        "one": {"late_peak": (64, 200, 33, 2, B), "staircase_up": (80, 200, 250, 2, B), "staircase_down": (64, 129, 256, 2, B),
                "row_offsets_deep": (40, 200, 250, 2, B), "uniform": (64, 300, 256, 2, B), None: (40, 200, 77, 2, B)},
        "split": {"late_peak": (80, 200, 257, 2, B), "staircase_up": (40, 129, 300, 2, B), "start_peak": (40, 200, 225, 2, B),
                  None: (64, 200, 257, 2, B)},
        "wide": {"late_peak": (8, 200, 257, 128, B), "staircase_up": (16, 300, 320, 64, B), "staircase_down": (16, 200, 256, 128, B),
                 "row_offsets_deep": (64, 300, 77, 64, B), "uniform": (16, 200, 320, 128, B), "random": (8, 300, 256, 64, B), None: (8, 200, 77, 128, B)},
    }
    fused_q = ["qm1", "qm3", "qm2", "qm3v", "qm2v"]                              # the formats the one-launch form takes
    for form, shapes in per_form.items():
        for i, f in enumerate(fam):
            fmt = fused_q[i % len(fused_q)] if form == "one" else names[(i + 3) % len(names)]
            add(form, fmt, f, shapes.get(f, shapes[None]))
    add("split", "qm1", "staircase_mid", (40, 200, 257, 2, B))                     # NT = 9: the roof's top is tile 4, the first of the second half
    add("split", "unfused", "staircase_mid", (80, 129, 300, 2, B), (1, 0, 8))
    # ---- every format on start_peak (skip 0 and 1), row_offsets, delta_owner
    forms = ["w4", "one", "split"]
    n = 0
    for fmt in names:
        for f, quants in (("start_peak", [(1, 0, 8), (1, 1, 8), (2, 1, 6)]), ("row_offsets", [(1, 1, 8), (3, 0, 6)]), ("delta_owner", [(1, 0, 8), (1, 1, 8)])):
            for qu in quants:
                form = forms[n % 3]
                n += 1
                D = (40, 64, 80, 160)[n % 4]
                S = {"w4": 77, "one": 250, "split": 257}[form]
                add("w4" if form == "one" and fmt not in fused_q else form, fmt, f, (D, 200, S, 2, B), qu)
    # ---- the static log2 quantiser without the bypass: key 0 of start_peak (p ~ 1 against δ = 1/8) sits in the lower clamp
    for form, fmt, sh in (("w4", "qm1", (40, 129, 77, 2, B)), ("one", "qm3", (80, 200, 250, 2, B)), ("split", "unfused", (64, 129, 257, 2, B))):
        add(form, fmt, "start_peak", sh, (2, 0, 6))
    return out


CASES = _cases()
#: mode 0 (the exact-fp32 kernels of attn_fused.hip): every family at D = 8, 40, 160; the deep offsets need more than 8 head-dim elements
MODE0 = [(f, (D, 129, 77 if f != "late_peak" else 33, 2, B)) for f in FAMILIES if f != "staircase_mid" for D in (8, 40, 160)
         if not (D == 8 and f == "row_offsets_deep")]
#: the read-out check: (form, format, family, (D, T, S, H, B), (mode, skip, bits), first key j0 of the window).  D = 160 covers all 77 keys
#: (first tile, ragged last tile); S = 250: keys 90 .. 249 (the ragged last tile of the longest one-launch range); S = 300 (NT = 10, the
#: halves meet at key 160): 80 .. 239 straddles the boundary, 140 .. 299 holds it and the last tile; D = 40: all 33 keys; S = 257 (NT = 9,
#: the halves meet at key 128): 0 .. 39, 110 .. 149 and 217 .. 256 (the single key of the last tile)
READOUT = [
    ("w4", "unfused", "start_peak", (160, 129, 77, 2, B), (1, 1, 8), 0), ("w4", "qm0", "start_peak", (160, 129, 77, 2, B), (2, 1, 6), 0),
    ("one", "qm1", "delta_owner", (160, 129, 77, 2, B), (1, 0, 8), 0), ("one", "qm3v", "delta_owner", (160, 200, 250, 2, B), (1, 1, 8), 90),
    ("one", "qm2", "random", (160, 200, 250, 2, B), (3, 0, 6), 90), ("split", "qm1", "delta_owner", (160, 129, 300, 2, B), (1, 1, 8), 80),
    ("split", "unfused", "delta_owner", (160, 129, 300, 2, B), (1, 0, 8), 140), ("split", "qm2v", "random", (160, 129, 300, 2, B), (3, 0, 6), 140),
    ("one", "qm3", "start_peak", (40, 200, 33, 2, B), (1, 1, 8), 0), ("w4", "qm0v", "delta_owner", (40, 129, 33, 2, B), (1, 0, 8), 0),
    ("split", "qm3", "delta_owner", (40, 200, 257, 2, B), (1, 0, 8), 110), ("split", "qm2", "random", (40, 129, 257, 2, B), (2, 1, 6), 217),
    ("w4", "qm1", "start_peak", (40, 129, 257, 2, B), (1, 1, 8), 0), ("split", "qm0", "delta_owner", (40, 200, 257, 2, B), (1, 1, 8), 217),
]
#: the exact uniform check: (form, format, shape); S = 32, 77, 256, 257
UNIFORM = [("w4", "unfused", (40, 129, 32, 2, B)), ("one", "qm1", (64, 200, 77, 2, B)), ("one", "qm3v", (160, 129, 256, 2, B)),
           ("split", "qm2", (80, 200, 257, 2, B)), ("wide", "qm0v", (16, 200, 256, 128, B)), ("w4", "qm3", (8, 33, 257, 2, B))]


@functools.lru_cache(maxsize=1)
def reference(family, shape, quant, fmt_name):
    """(case, δ or None, Ref, o64, bound) of one interval-check case, shared by the CPU and the GPU module — do not modify"""
    case = make(family, shape)
    mode, skip, bits = quant
    fmt = FORMATS[fmt_name]
    delta = static_delta(case, mode, skip) if mode >= 2 else None
    r = ref64(case, mode, skip, bits, delta, fmt)
    D, H = shape[0], shape[3]
    return case, delta, r, r.output(case.v, H, D), r.bound(case.v, H, D, fmt)


# ------------------------------------------------------------------------------------------------------------------ exact checks
def f32(x):
    """a float64 tensor rounded to fp32 and back"""
    return x.float().double()


def check_readout(o, r, shape, quant, j0, delta):
    """o: the output for v = onehot_v(shape, j0), so o[b, t, h, d] is the device's p̂[b, h, t, j0 + d].  Returns (δ_dev, problems): every
    quantised entry must equal fp32(δ_dev·2^-c) (fp32(δ_dev·c) in mode 3), c the float64 code or, where the entry is ambiguous, its
    neighbour; a value below 2^-126 may also be flushed or clamped (within 2^-126).  δ_dev is the given δ in modes 2 and 3; in mode 1 it is
    read from the largest entry with an unambiguous code, must agree with the float64 δ to ln 2·τ_δ + 2u, and every other entry of the
    call must then carry that same value.  An un-quantised column is compared with p under its relative error ε_p."""
    D, T, S, H, Bn = shape
    mode, skip, bits = quant
    n = min(D, S - j0)
    got = heads(o.double(), H, D)[..., :n]
    sl = lambda x: x[..., j0:j0 + n]
    code, alt, amb, p = sl(r.code), sl(r.alt), sl(r.amb), sl(r.p)
    problems = []
    col = (torch.arange(j0, j0 + n) >= skip).expand_as(got)
    if mode == 1:
        cand = torch.where(col & ~amb, got, torch.zeros(()).double())
        i = int(cand.argmax())
        d_dev = float(cand.reshape(-1)[i] * torch.exp2(code.reshape(-1)[i]))
        rel = abs(d_dev - r.delta) / r.delta
        if not rel <= LN2 * r.tau_delta + 2.0 * U:
            problems.append("δ_dev %.9g against float64 %.9g: relative error %.3g above %.3g" % (d_dev, r.delta, rel, LN2 * r.tau_delta + 2.0 * U))
    else:
        d_dev = delta
    deq = (lambda c: f32(d_dev * c)) if mode == 3 else (lambda c: f32(d_dev * torch.exp2(-c)))
    e0, e1 = deq(code), deq(alt)
    ok = (got == e0) | (amb & (got == e1)) | ((e0 < 2.0 ** -126) & ((got - e0).abs() <= 2.0 ** -126))
    bad = col & ~ok
    if bool(bad.any()):
        i = int(bad.reshape(-1).float().argmax())
        problems.append("%d of %d quantised entries are not fp32(δ_dev·code); first: got %.9g, expected %.9g (code %g, y %.9g, τ %.3g)"
                        % (int(bad.sum()), int(col.sum()), float(got.reshape(-1)[i]), float(e0.reshape(-1)[i]), float(code.reshape(-1)[i]),
                           float(sl(r.y).reshape(-1)[i]), float(sl(r.tau).reshape(-1)[i])))
    if j0 < skip:
        eps = sl(r.eps_p)
        badp = ~col & ~((got - p).abs() <= eps * p + 2.0 ** -126)
        if bool(badp.any()):
            problems.append("%d un-quantised entries outside ε_p·p; worst ratio %.3g" % (int(badp.sum()), float(((got - p).abs() / (eps * p + 2.0 ** -126))[~col].max())))
    return d_dev, problems


def uniform_setting(shape, mode):
    """(case, δ, expected o) of the exact uniform check.  Mode 1: p = 1/S everywhere, so δ = fp32(1/S), every code is 0 and o =
    fp32(δ·S·c_d).  Mode 3 with δ = fp32(1/(3S)): p/δ = 3 to within 1e-6, every code is 3 and o = fp32(δ·3·S·c_d)."""
    D, T, S, H, Bn = shape
    case = make("uniform", shape)
    d32 = float(torch.tensor(1.0 / S if mode == 1 else 1.0 / (3.0 * S), dtype=torch.float32))
    c = case.info["c"].double() * (S * (1.0 if mode == 1 else 3.0)) * d32
    want = c.float().view(1, 1, 1, D).expand(Bn, T, H, D).reshape(Bn, T, H * D)
    return case, (None if mode == 1 else d32), want
