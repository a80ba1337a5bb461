"""TEST INFRASTRUCTURE — a float64 statement of the GEMM family's store epilogue (include/dgq_hip.h, "the hot kernel" and
dgq_gemm_extra_t) for integer operands given directly, and the buffer images tests/test_gpu_gemm_epilogue.py compares against.

No quantiser runs in front: a case holds the centred activation codes s [M][Kp], the stored weight codes qw' [N][Kp], rowsum [M] and the
per-K (cdelta / cflush) or per-M (mdelta / mzp / L / vn) tables.  The value is formed in the header's order

    dequantised value  ->  fq_mode (the fused attention-side quantiser)  ->  + residual[(m / res_div)·ldr + n]  ->  GEGLU pairing

in float64 and rounded ONCE to the output dtype.  ``images`` returns the expected content of the WHOLE allocation each output view is
carved out of (SENTINEL everywhere outside the [M][cols] window), so a store outside the window is seen as well as a wrong value.

Exactness.  alpha, cdelta, mdelta, fq_delta are powers of two; zw, gamma, mzp, vn, the residual and fq_zp are integers; the codes are
small.  Every term any kernel forms is then a multiple of one power-of-two unit per output element, and fp32 arithmetic on such terms
is exact in any order while the sum of their magnitudes stays below 2^24 units: ``margin`` computes that ratio, every case asserts
``< 1`` (tests/test_gemm_epilogue_ref_cpu.py), and ``emulate_f32`` — the epilogue's own operation order with every step rounded to
fp32 — must then equal the float64 value bit for bit.  The GPU assertion is therefore equality.

GEGLU.  dgq_geglu(a, g) = a·(0.5·g·(1 + erff(g/√2))) is exact where erff saturates: every gate column (odd weight row) carries a bias of
±(bound + GATE_FLOOR) over an accumulator bounded by ``bound``, both signs mixed within a row, so |g| >= GATE_FLOOR = 16 and the output
is a·g (positive gate) or 0 (negative gate).  ``make_case`` asserts that the float64 GELU of the same gates rounds to those fp32 values.
"""
import functools
import math

import torch

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
#: quiet-NaN bit patterns with a payload: no finite result, and no NaN a kernel could form, has these bits
SENTINEL = {torch.float32: 0x7FC5A5A5, torch.bfloat16: 0x7FA5, torch.float16: 0x7DA5}
CLASSES = ("A", "B", "C", "D")
GATE_FLOOR = 16.0
FQ_T, FQ_D, FQ_QMAX = 7, 5, 255.0
OFFSET = 128.0
L_PER_M = 5
MISTAKES = ("res_row_m", "res_before_fq", "skip_ignored", "mode3_by_m", "mode2_no_skip", "half_away", "geglu_swapped", "geglu_col_nb",
            "y2_pitch_ldy", "double_round16", "ragged_alpha")


# ----------------------------------------------------------------------------------------------- buffer layout
def view_layout(cls, rows, cols, dtype):
    """(element offset, row pitch, elements of the allocation) of a [rows][cols] view of alignment class ``cls`` inside an allocation
    whose base is 16-byte aligned:  A base on 16 bytes, pitch a multiple of 16 bytes (and of 4 elements);  B base off by one element;
    C base aligned, odd pitch;  D base on 8 bytes only.  Every class leaves elements in front, a pitch gap and a tail."""
    es = torch.empty(0, dtype=dtype).element_size()
    front = 32 // es                                         # 32 bytes in front of an aligned base
    pitch = (cols // 8 + 1) * 8                              # > cols, a multiple of 8 elements = 16 / 32 bytes
    off = front
    if cls == "B":
        off = front + 1
    elif cls == "C":
        pitch = (cols + 1) | 1
    elif cls == "D":
        off = front + 8 // es
    else:
        assert cls == "A", cls
    assert pitch > cols and (off * es) % 16 == {"A": 0, "B": es, "C": 0, "D": 8}[cls]
    return off, pitch, off + (rows - 1) * pitch + cols + pitch + 8


def carve(alloc, off, pitch, rows, cols):
    """the [rows][cols] view at element ``off`` with row pitch ``pitch`` of a 1-d allocation"""
    return alloc.as_strided((rows, cols), (pitch, 1), off)


def image(window, dtype, off, pitch, total):
    """integer image of an allocation of ``total`` elements of ``dtype`` holding ``window`` (of that dtype, or already its integer view) at
    (off, pitch) and SENTINEL elsewhere; window elements that fall outside the allocation are clipped (planted mistakes only)"""
    w = window.contiguous().view(INT_VIEW[dtype]) if window.dtype == dtype else window
    img = torch.full((total,), SENTINEL[dtype], dtype=torch.int64).to(INT_VIEW[dtype])
    rows, cols = w.shape
    idx = off + torch.arange(rows)[:, None] * pitch + torch.arange(cols)[None, :]
    ok = idx < total
    img[idx[ok]] = w[ok]
    return img


def first_mismatch(got_img, want_img, dtype, off, pitch, rows, cols):
    """None, or (row, column, inside / outside the window, got, want) of the first differing element of two integer images of ``dtype``"""
    bad = (got_img != want_img).nonzero()
    if bad.numel() == 0:
        return None
    i = int(bad[0])
    r, col = divmod(i - off, pitch) if i >= off else (-1, i - off)
    inside = 0 <= r < rows and 0 <= col < cols
    val = lambda t: "%r (0x%x)" % (float(t[i:i + 1].view(dtype)), int(t[i]) & (0xFFFFFFFF if dtype == torch.float32 else 0xFFFF))
    return (r, col, "inside" if inside else "outside", val(got_img), val(want_img))


# ----------------------------------------------------------------------------------------------- operands
def _operands(M, N, Kp, wbits, small, seed):
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g)
    nch = Kp // 32
    if small:                                               # the GEGLU cases: a·g must be exact, so both stay narrow
        s, qw = ri(-2, 2, (M, Kp)), ri(0, 7, (N, Kp))
        cd = torch.ones(nch, dtype=torch.float64)
        alpha = torch.tensor([2.0 ** (n // 2 % 2) for n in range(N)], dtype=torch.float64)
        zw = torch.tensor([float((n * 3) % 8) for n in range(N)], dtype=torch.float64)
    else:
        s = ri(-6, 6, (M, Kp))
        s[::7, ::53] = -128                                 # int8 extremes, sparsely (16-bit outputs must stay finite)
        s[3::11, 5::47] = 127
        if wbits == 4:
            qw = ri(0, 15, (N, Kp))
            zw = torch.tensor([float((n * 7) % 16) for n in range(N)], dtype=torch.float64)
        else:                                               # W8: stored codes q − 128
            qw = ri(-12, 12, (N, Kp))
            qw[::5, ::61] = -128
            qw[2::9, 3::67] = 127
            zw = torch.tensor([float((n * 7) % 16 - 8) for n in range(N)], dtype=torch.float64)
        cd = torch.tensor([2.0 ** ((i % 3) - 1) for i in range(nch)], dtype=torch.float64)
        alpha = torch.tensor([2.0 ** ((n % 3) - 1) for n in range(N)], dtype=torch.float64)
    gend = torch.tensor([(i % 3 == 1 or i == nch - 1) for i in range(nch)])
    fl = gend.to(torch.uint8)
    fl[3::12] = 2                                           # clears behind every third K tile; marks off a tile's last chunk are ignored
    fl[6::16] = 2
    for i in range(nch - 2, -1, -1):                        # every chunk carries its group's scale
        if not gend[i]:
            cd[i] = cd[i + 1]
    rowsum = torch.tensor([float((m * 3) % 17 - 8) for m in range(M)], dtype=torch.float64)
    # gamma: small integers, and in two columns of five ±2304 so that 16-bit outputs are rounded, not trivially exact
    gamma = torch.tensor([float(n % 11 - 5) + (2304.0 if n % 5 == 2 else (-2304.0 if n % 5 == 4 else 0.0)) for n in range(N)], dtype=torch.float64)
    if small:
        gamma = torch.tensor([float(n % 11 - 5) for n in range(N)], dtype=torch.float64)
    md = torch.tensor([2.0 ** (i - 4) for i in range(L_PER_M)], dtype=torch.float64)
    if small:
        md = torch.tensor([2.0 ** (i % 2) for i in range(L_PER_M)], dtype=torch.float64)
    mz = torch.tensor([float(120 + 3 * i) for i in range(L_PER_M)], dtype=torch.float64)
    vn = torch.tensor([float((n * 5) % 23 - 11) for n in range(N)], dtype=torch.float64)
    return dict(s=s, qw=qw, cdelta=cd, cflush=fl, alpha=alpha, zw=zw, gamma=gamma, rowsum=rowsum, mdelta=md, mzp=mz, vn=vn)


def _bare(c):
    """(per-K: Σ_c cdelta_c·P_c − zw·rowsum;  per-M: mdelta·(Σ s·qw' − zw·rowsum + (offset − mzp)·vn)) [M][N] float64, before alpha"""
    s, qw = c["s"].double(), c["qw"].double()
    M = c["M"]
    if c["per_m"]:
        mi = torch.arange(M) % L_PER_M
        t = s @ qw.t() - c["zw"][None, :] * c["rowsum"][:, None] + (OFFSET - c["mzp"][mi])[:, None] * c["vn"][None, :]
        return c["mdelta"][mi][:, None] * t
    acc = torch.zeros(M, c["N"], dtype=torch.float64)
    for ch in range(c["Kp"] // 32):
        acc += c["cdelta"][ch] * (s[:, 32 * ch:32 * ch + 32] @ qw[:, 32 * ch:32 * ch + 32].t())
    return acc - c["zw"][None, :] * c["rowsum"][:, None]


def _fq_tables(mode):
    """(delta, zp, skip): T entries each so that every planted index mistake stays inside the table; neighbours differ"""
    delta = torch.tensor([2.0 ** e for e in (1, 2, 0, 3, 1, 2, 0)], dtype=torch.float64)
    zp = torch.tensor([128.0, 100.0, 140.0, 120.0, 133.0, 90.0, 150.0], dtype=torch.float64)
    return delta, zp, {1: 0, 2: 2, 3: 1}[mode]


def make_case(name, M, N, Kp, wbits=4, per_m=0, out="f32", ycls="A", res=None, y2cls=None, fq=0, geglu=False, gn=False, seed=1):
    """One cell's operands, layout and extras.  res = (dtype name, class, res_div) or None; fq = 0 / 1 / 2 / 3; y2cls: class of the second
    copy or None.  The dict is shared between tests: do not modify its tensors."""
    c = dict(name=name, M=M, N=N, Kp=Kp, wbits=wbits, per_m=per_m, out=out, dtype=DTYPES[out], ycls=ycls, res=res, y2cls=y2cls, fq=fq,
             geglu=geglu, gn=gn, seed=seed)
    c.update(_operands(M, N, Kp, wbits, geglu, seed * 1000 + N * 7 + Kp + wbits))
    if geglu:
        # gates: bias ±(bound + floor) over the bounded rest of the dequantised value (sign alternates along the row)
        gam = c["gamma"]
        gam[1::2] = 0.0
        bound = float((c["alpha"][None, :] * _bare(c))[:, 1::2].abs().max())
        sign = torch.tensor([1.0 if (i % 3) != 1 else -1.0 for i in range(N // 2)], dtype=torch.float64)
        gam[1::2] = sign * (bound + GATE_FLOOR)
        c["gate_bound"] = bound
    return _finish_case(c)


def make_layer_case(name, y0, unit, base_margin, K, out="f32", ycls="A", res=None, y2cls=None, fq=0, geglu=False, gn=False, seed=1, layer=None):
    """A cell of a kernel that runs its own quantiser (panel, conv, real-time block, MXFP6): ``y0`` [M][N] float64 is the layer's
    dequantised value (bias included) from that family's float64 reference on exact data, ``unit`` the power of two every term is a
    multiple of, ``base_margin`` that family's own exactness ratio; the extras are applied by the same code as for ``make_case``.
    ``layer``: whatever the GPU test needs to launch it (the recipe dict)."""
    M, N = y0.shape
    c = dict(name=name, M=M, N=N, Kp=K, wbits=4, per_m=0, out=out, dtype=DTYPES[out], ycls=ycls, res=res, y2cls=y2cls, fq=fq, geglu=geglu,
             gn=gn, seed=seed, y0=y0.double(), unit=float(unit), base_margin=float(base_margin), layer=layer)
    return _finish_case(c)


def _finish_case(c):
    M, N, seed, res = c["M"], c["N"], c["seed"], c["res"]
    cols = N // 2 if c["geglu"] else N
    c["cols"] = cols
    c["y_layout"] = view_layout(c["ycls"], M, cols, c["dtype"])
    if c["y2cls"] is not None:
        c["y2_layout"] = view_layout(c["y2cls"], M, N, c["dtype"])
        if c["y2_layout"][1] == c["y_layout"][1]:            # the two pitches must differ, or a copy written at pitch ldy goes unseen
            off, pitch, total = c["y2_layout"]
            c["y2_layout"] = (off, pitch + (2 if c["y2cls"] == "C" else 8), total + 8 * M)
    if res is not None:
        rdt, rcls, div = res
        rows = (M + div - 1) // div
        g = torch.Generator().manual_seed(seed * 77 + M + N)
        r = torch.randint(-127, 128, (rows, N), generator=g).double()
        r = torch.where((torch.arange(rows)[:, None] + torch.arange(N)[None, :]) % 3 == 0, r * 32.0, r)
        assert torch.equal(r.to(DTYPES[rdt]).double(), r), "the residual must be exact in its dtype"
        c["residual"] = r
        c["res_layout"] = view_layout(rcls, rows, N, DTYPES[rdt])
    if c["fq"]:
        c["fq_delta"], c["fq_zp"], c["fq_skip"] = _fq_tables(c["fq"])
    if c["geglu"]:
        _assert_gelu_saturates(c)
    # 16-bit outputs: finite, and large enough that the final rounding is exercised
    big = float(expected(c).double().abs().max())
    assert math.isfinite(big) and (c["out"] == "f32" or c["fq"] or big > {"bf16": 2.0 ** 8, "f16": 2.0 ** 11}[c["out"]]), (c["name"], big)
    return c


def _dequant(c, alpha=None):
    """the dequantised value [M][N] in float64: the header's formula on the cell's operands, or the layer family's own reference"""
    if "y0" in c:
        return c["y0"].clone()
    return (c["alpha"] if alpha is None else alpha)[None, :] * _bare(c) + c["gamma"][None, :]


def _assert_gelu_saturates(c):
    h = _dequant(c)
    a, g = h[:, 0::2], h[:, 1::2]
    assert float(g.abs().min()) >= GATE_FLOOR and bool((g > 0).any(1).all()) and bool((g < 0).any(1).all())
    gelu64 = a * (0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0))))
    want = torch.where(g > 0, a * g, torch.zeros_like(a))
    assert torch.equal(gelu64.float(), want.float()), "the float64 GELU of the planted gates must round to a·g / 0 in fp32"


# ----------------------------------------------------------------------------------------------- the formula
def _rne(x):
    return torch.round(x)                                   # round half to even


def _fake_quant(c, y, mistakes):
    M, N = y.shape
    m, n = torch.arange(M)[:, None].expand(M, N), torch.arange(N)[None, :].expand(M, N)
    t = m % FQ_T
    skip = c["fq_skip"]
    if c["fq"] == 1:
        idx = torch.zeros_like(t)
    elif c["fq"] == 2:
        idx = t if "mode2_no_skip" in mistakes else t - skip
    else:
        idx = (m if "mode3_by_m" in mistakes else n) % FQ_D
    live = torch.ones_like(t, dtype=torch.bool) if "skip_ignored" in mistakes else t >= skip
    idx = idx.clamp(0, FQ_T - 1)
    d, z = c["fq_delta"][idx], c["fq_zp"][idx]
    q = y / d
    r = torch.where(q >= 0, torch.floor(q + 0.5), torch.ceil(q - 0.5)) if "half_away" in mistakes else _rne(q)
    code = torch.clamp(r + z, 0.0, FQ_QMAX)
    return torch.where(live, d * (code - z), y)


def expected(c, mistakes=()):
    """the [M][cols] window of the output in the output dtype: float64 throughout, one rounding at the end"""
    M, N = c["M"], c["N"]
    alpha = None
    if "ragged_alpha" in mistakes and N % 4 != 0 and "y0" not in c:
        alpha = c["alpha"].clone()
        alpha[N - 1] = alpha[N - 2]
    y = _dequant(c, alpha)
    r = None
    if c["res"] is not None:
        rows = torch.arange(M) if "res_row_m" in mistakes else torch.arange(M) // c["res"][2]
        r = c["residual"][rows.clamp(max=c["residual"].shape[0] - 1)]
        if "res_before_fq" in mistakes and c["fq"]:
            y, r = y + r, None
    if c["fq"]:
        y = _fake_quant(c, y, mistakes)
    if r is not None:
        if "double_round16" in mistakes:
            y = y.to(c["dtype"]).double()
        y = y + r
    if c["geglu"]:
        a, g = (y[:, 1::2], y[:, 0::2]) if "geglu_swapped" in mistakes else (y[:, 0::2], y[:, 1::2])
        y = a * (0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0))))
    return y.to(c["dtype"])


def images(c, mistakes=()):
    """dict(y=, y2=) of integer images of the whole allocations (y2 only where the case has one)"""
    win = expected(c, mistakes)
    off, pitch, total = c["y_layout"]
    out = {}
    if "geglu_col_nb" in mistakes and c["geglu"]:
        # a lane's two outputs stored at columns nb, nb + 1 instead of nb/2, nb/2 + 1 (clipped to the row's N columns)
        it = INT_VIEW[c["dtype"]]
        wide = torch.full((c["M"], c["N"]), SENTINEL[c["dtype"]], dtype=torch.int64).to(it)
        i = torch.arange(c["cols"])
        wide[:, 4 * (i // 2) + i % 2] = win.view(it)
        out["y"] = image(wide, c["dtype"], off, pitch, total)
    else:
        out["y"] = image(win, c["dtype"], off, pitch, total)
    if c["y2cls"] is not None:
        off2, pitch2, total2 = c["y2_layout"]
        out["y2"] = image(win, c["dtype"], off2, pitch if "y2_pitch_ldy" in mistakes else pitch2, total2)
    return out


# ----------------------------------------------------------------------------------------------- the exactness argument
def margin(c):
    """max over the output elements of (sum of the magnitudes of every term a kernel forms) / (2^24 units); the fp32 result equals the
    float64 one in any summation order iff this is < 1.  unit = the smallest power of two any term of the element is a multiple of."""
    M, N = c["M"], c["N"]
    if "y0" in c:
        own = c["base_margin"] * 2.0 ** 24
        total, unit = c["y0"].abs(), torch.full((M, N), min(c["unit"], 1.0), dtype=torch.float64)
        return _extras_margin(c, total, unit, own)
    s, qw = c["s"].double().abs(), c["qw"].double().abs()
    al = c["alpha"][None, :]
    if c["per_m"]:
        mi = torch.arange(M) % L_PER_M
        inner = s @ qw.t() + c["zw"].abs()[None, :] * c["rowsum"].abs()[:, None] + (OFFSET - c["mzp"][mi]).abs()[:, None] * c["vn"].abs()[None, :]
        own = float(inner.max())                            # the integer stage
        total = al * c["mdelta"][mi][:, None] * inner
        unit = torch.clamp(al * c["mdelta"][mi][:, None], max=1.0)
    else:
        # summation by parts over any chunk order, K split and clear segment: Σ_c |coef_c·T_c| <= 2·δ_max·Σ|s||qw'|
        own = float((s @ qw.t()).max())
        total = al * (2.0 * c["cdelta"].max() * (s @ qw.t()) + c["zw"].abs()[None, :] * c["rowsum"].abs()[:, None])
        unit = torch.clamp(al * c["cdelta"].min(), max=1.0)
    total = total + c["gamma"].abs()[None, :]
    return _extras_margin(c, total, unit * torch.ones(M, N, dtype=torch.float64), own)


def _extras_margin(c, total, unit, own):
    if c["fq"]:                                             # the quantiser's own steps: integers |r| + |z|, then δ·(code − z)
        total = total + float((c["fq_delta"] * (FQ_QMAX + c["fq_zp"])).max())
        unit = torch.clamp(unit, max=float(c["fq_delta"].min()))
    if c["res"] is not None:
        total = total + float(c["residual"].abs().max())
    ratio = float((total / unit).max())
    if c["geglu"]:                                          # the one product of two results: a·g = a·odd(g)·2^k, exact iff a·odd(g) fits
        h = _dequant(c).abs() / unit
        gi = h[:, 1::2].round().long()
        assert torch.equal(gi.double(), h[:, 1::2])
        odd = (gi // (gi & -gi).clamp(min=1)).double()
        ratio = max(ratio, float((h[:, 0::2] * odd).max()))
    return max(ratio, own) / 2.0 ** 24


def _f32(x):
    return x.float().double()


def emulate_f32(c):
    """The epilogue in the kernels' operation order with EVERY step rounded to fp32 (gemm_device.h dgq_dequant / dgq_extra, dgq_geglu;
    the per-K accumulator by summation by parts with the clear marks): equals ``expected`` bit for bit on exact data."""
    M, N, Kp = c["M"], c["N"], c["Kp"]
    if "y0" in c:
        return _emulate_extras(c, _f32(c["y0"]))
    s, qw = c["s"].double(), c["qw"].double()
    al, zw, ga, rs = c["alpha"][None, :], c["zw"][None, :], c["gamma"][None, :], c["rowsum"][:, None]
    if c["per_m"]:
        mi = torch.arange(M) % L_PER_M
        md, mz = c["mdelta"][mi][:, None], c["mzp"][mi][:, None]
        acc = _f32(s @ qw.t())                              # (float)int32
        r0, r1, r2 = md, _f32(md * rs), _f32(md * _f32(OFFSET - mz))
        t = _f32(r0 * acc - _f32(zw * r1))
        t = _f32(r2 * c["vn"][None, :] + t)
        y = _f32(al * t + ga)
    else:
        nch = Kp // 32
        cd, fl = c["cdelta"], c["cflush"]
        T = torch.zeros(M, N, dtype=torch.float64)
        acc = torch.zeros(M, N, dtype=torch.float64)
        for ch in range(nch):
            T = T + s[:, 32 * ch:32 * ch + 32] @ qw[:, 32 * ch:32 * ch + 32].t()
            clear = ch % 4 == 3 and int(fl[ch]) == 2
            coef = cd[ch] if (ch == nch - 1 or clear) else _f32(cd[ch] - cd[ch + 1])
            acc = _f32(coef * _f32(T) + acc)
            if clear:
                T = torch.zeros_like(T)
        y = _f32(al * _f32(acc - zw * rs) + ga)
    return _emulate_extras(c, y)


def _emulate_extras(c, y):
    M, N = y.shape
    if c["fq"]:
        m, n = torch.arange(M)[:, None].expand(M, N), torch.arange(N)[None, :].expand(M, N)
        t = m % FQ_T
        idx = {1: torch.zeros_like(t), 2: (t - c["fq_skip"]).clamp(min=0), 3: n % FQ_D}[c["fq"]]
        d, z = c["fq_delta"][idx], c["fq_zp"][idx]
        code = torch.clamp(_f32(torch.round(_f32(y / d)) + z), 0.0, FQ_QMAX)
        y = torch.where(t >= c["fq_skip"], _f32(d * _f32(code - z)), y)
    if c["res"] is not None:
        y = _f32(y + c["residual"][torch.arange(M) // c["res"][2]])
    if c["geglu"]:
        a, g = y[:, 0::2], y[:, 1::2]
        erf = torch.where(g > 0, torch.ones_like(g), -torch.ones_like(g))          # erff saturated: |g| >= GATE_FLOOR (asserted)
        y = _f32(a * _f32(_f32(0.5 * g) * _f32(1.0 + erf)))
    return y.float().to(c["dtype"])


def edge_report(c):
    """what the fq data reaches: exact ties with even and odd k, clamps at 0 and at qmax, bypassed tokens — the CPU self-check asserts
    every one of them over the fq cases"""
    y = _dequant(c)
    M, N = y.shape
    m, n = torch.arange(M)[:, None].expand(M, N), torch.arange(N)[None, :].expand(M, N)
    t = m % FQ_T
    idx = {1: torch.zeros_like(t), 2: (t - c["fq_skip"]).clamp(min=0), 3: n % FQ_D}[c["fq"]]
    live = t >= c["fq_skip"]
    q = y / c["fq_delta"][idx]
    u = torch.round(q) + c["fq_zp"][idx]
    tie = live & (q - torch.floor(q) == 0.5) & (u > 0) & (u < FQ_QMAX)
    k = torch.floor(q)
    return dict(tie_even=int((tie & (k % 2 == 0)).sum()), tie_odd=int((tie & (k % 2 == 1)).sum()), clamp_lo=int((live & (u < 0)).sum()),
                clamp_hi=int((live & (u > FQ_QMAX)).sum()), bypass=int((~live).sum()))


# ----------------------------------------------------------------------------------------------- the cells
def _cells(M):
    """the (extras, dtype, classes) cells every wxa8 kernel family runs, as make_case keyword sets.  N walks 68..71 (N % 4 = 0..3, a full
    64-wide column tile and a ragged one), per-K / per-M and Kp = 128 / 384 alternate; every class of y, y2 and the residual occurs, and
    the pairs (y vector, y2 scalar), (y scalar, y2 vector), (residual vector, stores scalar), (residual scalar, stores vector)."""
    out = []

    def add(tag, **kw):
        i = len(out)
        if kw.get("N") is None:
            kw["N"] = 68 + i % 4
        kw.setdefault("per_m", (i // 2) % 2)
        kw.setdefault("Kp", 128 if (i // 4) % 2 else 384)
        out.append(dict(name="%s-%s-%s" % (tag, kw.get("out", "f32"), kw.get("ycls", "A")), M=M, seed=1 + i % 3, **kw))
    for dt in DTYPES:
        for cls in CLASSES:
            add("none", out=dt, ycls=cls)
    # residual: every dtype in every class; vector stores over scalar residuals and the reverse; res_div 7 (M % 7 != 0)
    for rdt in DTYPES:
        for rcls, ycls in (("A", "B"), ("B", "A"), ("C", "A"), ("D", "C")):
            add("res_%s%s" % (rdt, rcls), out=rdt, ycls=ycls, res=(rdt, rcls, 7 if rcls in "AC" else 1), N=68 if rcls in "AD" else None)
    add("res_f32A_under_bf16", out="bf16", ycls="A", res=("f32", "A", 1), N=68)
    add("res_bf16A_under_f32", out="f32", ycls="A", res=("bf16", "A", 7), N=68)
    add("res_f32B_under_bf16", out="bf16", ycls="C", res=("f32", "B", 7), N=71)
    add("res_f16D_under_f32", out="f32", ycls="B", res=("f16", "D", 1), N=68)
    # y2 alone and with a residual
    for dt, ycls, y2cls in (("f32", "A", "B"), ("f32", "C", "A"), ("bf16", "A", "C"), ("bf16", "B", "A"), ("f16", "D", "A"), ("f16", "A", "D"),
                            ("f32", "A", "A"), ("bf16", "D", "D")):
        add("y2%s" % y2cls, out=dt, ycls=ycls, y2cls=y2cls, N=68 if len(out) % 2 else 70)
    add("y2A_resB", out="f32", ycls="C", y2cls="A", res=("f32", "B", 1), N=68)
    add("y2C_resA", out="bf16", ycls="A", y2cls="C", res=("bf16", "A", 7), N=68)
    add("y2B_resD", out="f16", ycls="A", y2cls="B", res=("f16", "D", 1), N=71)
    # the fused quantiser: each mode alone, mode 2 with a residual (the order of the two)
    for mode in (1, 2, 3):
        for dt, cls in (("f32", "A"), ("bf16", "C"), ("f16", "B")):
            add("fq%d" % mode, out=dt, ycls=cls, fq=mode)
    add("fq2_resA", out="f32", ycls="A", fq=2, res=("f32", "A", 1), N=68)
    add("fq2_resC", out="bf16", ycls="B", fq=2, res=("bf16", "C", 7), N=70)
    add("fq2_resB", out="f16", ycls="A", fq=2, res=("f32", "B", 1), N=69)
    # GEGLU: pitch classes A, C, D (and B) in fp32 and bf16; N % 4 == 0 is the header's condition
    for dt in ("f32", "bf16"):
        for cls in ("A", "C", "D", "B"):
            add("geglu", out=dt, ycls=cls, geglu=True, N=68)
    return out


#: (M, wbits, Kp override) of every variant of the cells a GPU test runs: the tile family, the 256-row kernel, W8, the K-split plans
VARIANTS = ((83, 4, None), (300, 4, None), (83, 8, None), (83, 4, 384))


@functools.lru_cache(maxsize=None)
def cells(M=83, wbits=4, Kp=None):
    """the shared cells at M rows (W4 / W8; Kp: every cell at this K instead of alternating), built once; read-only"""
    return tuple(make_case(**dict(kw, wbits=wbits, **({"Kp": Kp} if Kp else {}))) for kw in _cells(M))


def describe(c):
    """(extras, dtype, class of y / y2 / residual) of a cell, for the coverage table"""
    ex = []
    if c["res"] is not None:
        ex.append("res[%s,div%d]" % (c["res"][0], c["res"][2]))
    if c["y2cls"] is not None:
        ex.append("y2")
    if c["fq"]:
        ex.append("fq%d" % c["fq"])
    if c["geglu"]:
        ex.append("geglu")
    if c["gn"]:
        ex.append("gn")
    return "+".join(ex) or "none", c["out"], c["ycls"], c["y2cls"] or "-", c["res"][1] if c["res"] is not None else "-"


def paths(c, split=False):
    """which side of each vector / scalar choice of the epilogue the cell's full column groups take (the ragged last group is always
    element by element): dict of 'vec' / 'scalar' / '-'"""
    es = 4 if c["out"] == "f32" else 2

    def store(layout, cols):
        off, pitch, _ = layout
        return "vec" if (off * es) % 16 == 0 and (pitch * es) % 16 == 0 and (es == 4 or pitch % 4 == 0) and cols >= 4 else "scalar"
    p = dict(y="-", y2="-", res="-", geglu="-", slab="-", combine="-")
    if c["geglu"]:
        off, pitch, _ = c["y_layout"]
        p["geglu"] = "vec" if pitch % 2 == 0 and (off * es) % 8 == 0 else "scalar"
        return p
    p["y"] = store(c["y_layout"], c["N"])
    if c["y2cls"] is not None:
        p["y2"] = store(c["y2_layout"], c["N"])
    if c["res"] is not None:
        res_es = 4 if c["res"][0] == "f32" else 2
        off, pitch, _ = c["res_layout"]
        p["res"] = "vec" if pitch % 4 == 0 and (off * res_es) % (4 * res_es) == 0 else "scalar"
    if split:
        p["slab"] = "vec" if c["N"] % 4 == 0 else "scalar"
        ok = c["N"] % 4 == 0 and p["y"] == "vec" and p["y2"] in ("-", "vec") and not c["fq"] and p["res"] in ("-", "vec")
        p["combine"] = "vec" if ok else "scalar"
    return p


# ----------------------------------------------------------------------------------------------- kernels that run their own quantiser
#: the extras every such family runs on its one Linear cell (M = 83, K = 128): every class of y, y2 and the residual, the four
#: vector / scalar pairs, the three fused-quantiser modes, GEGLU in pitch classes A, C, D (fp32 and bf16)
LAYER_SPECS = (
    dict(tag="none", out="f32", ycls="A", N=68), dict(tag="none", out="bf16", ycls="B", N=69), dict(tag="none", out="f16", ycls="C", N=70),
    dict(tag="none", out="f32", ycls="D", N=71),
    dict(tag="res", out="f32", ycls="B", res=("f32", "A", 1), N=68), dict(tag="res", out="bf16", ycls="A", res=("bf16", "B", 7), N=69),
    dict(tag="res", out="f16", ycls="A", res=("f16", "C", 1), N=70), dict(tag="res", out="f32", ycls="C", res=("bf16", "D", 7), N=68),
    dict(tag="res", out="bf16", ycls="D", res=("f32", "A", 1), N=68), dict(tag="res", out="f16", ycls="B", res=("f16", "A", 7), N=68),
    dict(tag="y2", out="f32", ycls="A", y2cls="B", N=68), dict(tag="y2", out="bf16", ycls="C", y2cls="A", N=68),
    dict(tag="y2", out="f16", ycls="A", y2cls="C", N=71), dict(tag="y2", out="f32", ycls="B", y2cls="D", N=68),
    dict(tag="y2res", out="f16", ycls="D", y2cls="A", res=("f16", "D", 1), N=68),
    dict(tag="fq1", out="f32", ycls="A", fq=1, N=69), dict(tag="fq2", out="bf16", ycls="C", fq=2, N=70), dict(tag="fq3", out="f16", ycls="B", fq=3, N=71),
    dict(tag="fq2res", out="f32", ycls="A", fq=2, res=("f32", "B", 1), N=68),
    dict(tag="geglu", out="f32", ycls="A", geglu=True, N=68), dict(tag="geglu", out="f32", ycls="C", geglu=True, N=68),
    dict(tag="geglu", out="f32", ycls="D", geglu=True, N=68), dict(tag="geglu", out="bf16", ycls="A", geglu=True, N=68),
    dict(tag="geglu", out="bf16", ycls="C", geglu=True, N=68), dict(tag="geglu", out="bf16", ycls="D", geglu=True, N=68),
)
LAYER_M, LAYER_K = 83, 128


def _zero_gates(d):
    """GEGLU on a layer recipe: the gate rows (odd n) get the weight q = z (no accumulator: bound = 0) and a bias of ±16, ±32 or ±64 by
    column, signs mixed along the row — a·g is then exact whatever a is (these families' planted values are wide; a gate with more
    significant bits would round the product).  The tile family's cells carry the gates with a live accumulator."""
    N = d["qw"].shape[0]
    odd = torch.arange(1, N, 2)
    wz = d["wzp"].reshape(-1)
    assert bool((wz == wz.round()).all()) and float(wz.min()) >= 0
    d["qw"][odd] = wz[odd].long()[:, None]
    w2 = d["w"].reshape(N, -1)
    w2[odd] = 0.0
    d["w"] = w2.reshape(d["w"].shape)
    sign = torch.tensor([1.0 if (i % 4) < 2 else -1.0 for i in range(N // 2)])
    d["bias"][odd] = sign * GATE_FLOOR * 2.0 ** (torch.arange(N // 2) % 3).float()
    return d


@functools.lru_cache(maxsize=None)
def layer_recipe(family, N, geglu, layout="perK"):
    """(recipe dict d, layer case, y0 [M][N] float64 without residual, unit, the family's own exactness margin) of one Linear cell of
    ``family`` in {"panel", "blockq", "mx6"} — its planted exact data, the family's float64 reference"""
    from tests import layer_reference as lr
    case = lr.linear_case(LAYER_M, LAYER_K, N)
    case = dict(case, name="%s_%s%s" % (case["name"], family, "_geglu" if geglu else ""))
    if family == "panel":
        d = lr._build_exact(case, layout, 8, 4, lr.PROFILES[0])
    elif family == "blockq":
        from tests import realtime_block_ref as rb
        d = rb.planted_exact(case, 8, 4)
    else:
        from tests import mxfp6_ref as mx
        d = mx.planted_mx6(case)
    d["residual"] = torch.zeros_like(d["residual"])
    if geglu:
        d = _zero_gates(d)
    else:                                                   # two columns of five far out, so that 16-bit outputs are rounded
        n = torch.arange(N)
        d["bias"] = d["bias"] + 2304.0 * (n % 5 == 2).float() - 2304.0 * (n % 5 == 4).float()
    if family == "panel":
        y0 = lr.reference_layer(d["x"], d["w"], d["bias"], d["adelta"], d["azp"], 8, "linear")[0]
        base = lr.exact_margin(d, case)
        unit = float(d["adelta"].min()) * float(d["wdelta"].min())
    elif family == "blockq":
        y0, q, de, ze, inside = rb.block_reference(case, d)
        base = rb.block_exact_margin(case, d, q, de, ze, inside)
        unit = float(de.min()) * float(d["wdelta"].min())
    else:
        y0, xhat = mx.mx6_layer_reference(case, d["x"], d["qw"], d["wzp"], d["wdelta"], d["bias"], None)
        base = mx.mx6_exact_margin(case, xhat, d["qw"], d["wzp"], d["wdelta"], d["bias"], d["residual"])
        unit = 2.0 ** (min(mx.PLANT_E) - 3) * float(d["wdelta"].min())
    return d, case, y0.reshape(LAYER_M, N).double(), unit, base


@functools.lru_cache(maxsize=None)
def layer_cells(family, layout="perK"):
    out = []
    for i, spec in enumerate(LAYER_SPECS):
        kw = {k: v for k, v in spec.items() if k not in ("tag", "N")}
        d, case, y0, unit, base = layer_recipe(family, spec["N"], bool(spec.get("geglu")), layout)
        out.append(make_layer_case("%s-%s-%s" % (spec["tag"], spec["out"], spec["ycls"]), y0, unit, base, LAYER_K, seed=1 + i % 3,
                                   layer=dict(d=d, case=case, layout=layout), **kw))
    return tuple(out)


#: the conv kernel with its quantiser inside at its smallest geometry, B x 32 x 4 x 8 -> 160: N is fixed (no ragged column group), the
#: header refuses GEGLU and the fused quantiser there; res_div = Ho·Wo = 32 is the bias_rows broadcast
CONVQ_SPECS = (
    dict(tag="none", out="f32", ycls="A"), dict(tag="none", out="bf16", ycls="B"), dict(tag="none", out="f16", ycls="C"), dict(tag="none", out="f32", ycls="D"),
    dict(tag="res", out="f32", ycls="B", res=("f32", "A", 1)), dict(tag="res", out="bf16", ycls="A", res=("bf16", "B", 1)),
    dict(tag="res", out="f16", ycls="A", res=("f16", "C", 32)), dict(tag="res", out="f32", ycls="C", res=("bf16", "D", 32)),
    dict(tag="res", out="bf16", ycls="D", res=("f32", "A", 32)),
    dict(tag="y2", out="f32", ycls="A", y2cls="B"), dict(tag="y2", out="bf16", ycls="C", y2cls="A"), dict(tag="y2", out="f16", ycls="A", y2cls="C"),
    dict(tag="y2res", out="f32", ycls="B", y2cls="D", res=("f32", "D", 32)),
)


@functools.lru_cache(maxsize=None)
def convq_recipe(B, layout):
    from tests import layer_reference as lr
    case = lr.conv_case(B, 32, 4, 8, 1, 160)
    d = lr._build_exact(case, layout, 8, 4, lr.PROFILES[0])
    d["residual"] = torch.zeros_like(d["residual"])
    y0 = lr.reference_layer(d["x"], d["w"], d["bias"], d["adelta"], d["azp"], 8, "conv", 3, 1, 1)[0]
    y0 = y0.permute(0, 2, 3, 1).reshape(B * 32, 160).double()
    return d, case, y0, float(d["adelta"].min()) * float(d["wdelta"].min()), lr.exact_margin(d, case)


@functools.lru_cache(maxsize=None)
def convq_cells():
    out = []
    for i, spec in enumerate(CONVQ_SPECS):
        kw = {k: v for k, v in spec.items() if k != "tag"}
        layout, B = ("perK", "perM")[i % 2], 1 + (i // 2) % 2
        d, case, y0, unit, base = convq_recipe(B, layout)
        out.append(make_layer_case("%s-%s-%s" % (spec["tag"], spec["out"], spec["ycls"]), y0, unit, base, 288, seed=1 + i % 3,
                                   layer=dict(d=d, case=case, layout=layout), **kw))
    return tuple(out)


# ----------------------------------------------------------------------------------------------- the batched small-M Linear
def smallm_case(M, K, N, wbits, seed):
    """dgq_linear_smallm_batch on exact data: integer input codes under a power-of-two scalar δ, the per-M formula with L = 1 and the
    row sums the kernel forms itself.  x = δ·(code − z) is exact in fp32, bf16 and fp16 (|code − z| <= 135: 8 significant bits)."""
    g = torch.Generator().manual_seed(seed * 131 + M * 7 + K + N + wbits)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g)
    s = ri(-6, 6, (M, K))
    s[:, 5::97] = -128
    s[:, 11::89] = 127
    md, mz = 0.25, 120.0
    x = md * (s.double() + OFFSET - mz)
    if wbits == 4:
        qw = ri(0, 15, (N, K))
        zw = torch.tensor([float((n * 7) % 16) for n in range(N)], dtype=torch.float64)
    else:
        qw = ri(-12, 12, (N, K))
        qw[::5, ::61] = -128
        qw[2::9, 3::67] = 127
        zw = torch.tensor([float((n * 7) % 16 - 8) for n in range(N)], dtype=torch.float64)
    alpha = torch.tensor([2.0 ** ((n % 3) - 1) for n in range(N)], dtype=torch.float64)
    gamma = torch.tensor([float(n % 11 - 5) + (2304.0 if n % 5 == 2 else (-2304.0 if n % 5 == 4 else 0.0)) for n in range(N)], dtype=torch.float64)
    vn = torch.tensor([float((n * 5) % 23 - 11) for n in range(N)], dtype=torch.float64)
    return dict(M=M, K=K, N=N, wbits=wbits, x=x, s=s, qw=qw, zw=zw, alpha=alpha, gamma=gamma, vn=vn, mdelta=md, mzp=mz)


def smallm_expected(c, dtype):
    s, qw = c["s"].double(), c["qw"].double()
    t = s @ qw.t() - c["zw"][None, :] * s.sum(1)[:, None] + (OFFSET - c["mzp"]) * c["vn"][None, :]
    return (c["alpha"][None, :] * c["mdelta"] * t + c["gamma"][None, :]).to(dtype)


def smallm_margin(c):
    s, qw = c["s"].double().abs(), c["qw"].double().abs()
    inner = s @ qw.t() + c["zw"].abs()[None, :] * s.sum(1)[:, None] + abs(OFFSET - c["mzp"]) * c["vn"].abs()[None, :]
    total = c["alpha"][None, :] * c["mdelta"] * inner + c["gamma"].abs()[None, :]
    unit = torch.clamp(c["alpha"] * c["mdelta"], max=1.0)[None, :]
    return max(float((total / unit).max()), float(inner.max())) / 2.0 ** 24


def smallm_emulate_f32(c, dtype):
    """linear_smallm_kernel's arithmetic with every step rounded to fp32: the quantiser (x/δ, round half even, + z, clamp, − 2^(b−1)),
    the row sum, the three fmas of the per-M epilogue"""
    md, mz = c["mdelta"], c["mzp"]
    x = c["x"].to(dtype).double()
    code = torch.clamp(torch.round(_f32(x / md)) + mz, 0.0, 255.0) - OFFSET
    assert torch.equal(code, c["s"].double()), "the quantiser must find the planted codes"
    rs = _f32(code.sum(1))[:, None]
    acc = _f32(code @ c["qw"].double().t())
    r0, r1, r2 = md, _f32(md * rs), md * (OFFSET - mz)             # (δ and z are fp32 values: the scalar products are exact)
    t = _f32(r0 * acc - _f32(c["zw"][None, :] * r1))
    t = _f32(r2 * c["vn"][None, :] + t)
    return _f32(c["alpha"][None, :] * t + c["gamma"][None, :]).float().to(dtype)


#: (M, K, wbits) of the small-M cells: odd M (the pair walk's clamped second row), K off a multiple of 32 (the guarded second half of
#: a lane's 32-code slice: 72 = 2·32 + 8, 1000 = 31·32 + 8), K = 1280 on the multiple; W8 at K = 1100, the second trip of its K loop
SMALLM_CELLS = tuple((M, K, 4) for M in (1, 3, 5) for K in (72, 1000, 1280)) + ((3, 1100, 8),)
SMALLM_N = (77, 64, 77, 64)                       # one batch of four problems, each with its own ldy
