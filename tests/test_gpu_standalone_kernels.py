"""The stand-alone quantiser and statistics kernels against the float64 statements of tests/standalone_kernels_ref.py (checked on the CPU
by tests/test_standalone_kernels_ref_cpu.py): dgq_fakequant_rows, dgq_max_f32 / dgq_logquant_f32 and the static-δ search built on them,
dgq_minmax_rows_cols, the four AdaRound kernels and dgq_quantize_weight — at the shapes where each takes another path: every table mode,
type and token skip, C no multiple of 4, a strided view, ragged row slices, and one tensor per kernel family above the kernel's grid cap,
so that its grid-stride loop runs a second, partial round.

Bit-exact (``same_bits`` / ``torch.equal``): the affine fake-quant, the maximum, min / max, the weight codes.  The log2 code is held to the
decided / undecided rule of ``logquant_ref``; the AdaRound kernels to the tolerances test_adaround_kernels_vs_oracle_and_reference_known_answers
states, against float64, plus the a-priori summation bound of the regulariser."""
import functools

import pytest
import torch

from tests import standalone_kernels_ref as sk

pytestmark = pytest.mark.gpu

DT_IDS = ["fp32", "fp16", "bf16"]


@pytest.fixture(scope="module")
def dev():
    from dgq_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


# ----------------------------------------------------------------------------------------------- dgq_fakequant_rows
def _run_fakequant(dev, c, mode, skip, bits, what):
    from dgq_amd import ops
    want = sk.fakequant_rows_ref(c["x"], c["T"], c["D"], mode, c["delta"], c["zp"], skip, bits)
    d, z = c["delta"].to(dev), c["zp"].to(dev)
    x = c["x"].to(dev)
    y = ops.fakequant_rows(x, c["T"], c["D"], mode, d, z, skip, bits)                      # in place
    assert y.data_ptr() == x.data_ptr()
    bad = sk.count_bit_mismatches(y, want)
    assert bad == 0, "%s in place: %d of %d elements differ in their bits" % (what, bad, want.numel())
    x = c["x"].to(dev)
    out = torch.full_like(x, 7.0)
    y = ops.fakequant_rows(x, c["T"], c["D"], mode, d, z, skip, bits, out=out)
    assert y.data_ptr() == out.data_ptr() and sk.same_bits(x, c["x"]), "%s out=: the input changed" % what
    bad = sk.count_bit_mismatches(y, want)
    assert bad == 0, "%s out=: %d of %d elements differ in their bits" % (what, bad, want.numel())


@pytest.mark.parametrize("dtype", sk.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("family", sk.FQ_FAMILIES)
def test_fakequant_rows_bit_for_bit(family, mode, dtype, dev):
    """every data family x table mode x type, each with skip 0 / 1, bits 4 / 6 / 8, the three small shapes, in place and out="""
    for shape in ("t77_8x40", "t129_2x8", "t129_3x5"):
        for skip in (0, 1):
            for bits in (4, 6, 8):
                c = sk.fq_case(family, shape, mode, dtype, skip, bits)
                _run_fakequant(dev, c, mode, skip, bits, "%s %s mode %d skip %d b%d %s" % (family, shape, mode, skip, bits, dtype))


@pytest.mark.parametrize("dtype", sk.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_fakequant_rows_second_stride_round(mode, dtype, dev):
    """8200 x 160 = 1 312 000 elements > 4096 x 256 threads: the grid-stride loop takes a second, partial round.  Ties (the fp32 claim) for
    fp32, randn for the 16-bit types; token skip 1, so the skipped rows recur in both rounds."""
    family = "ties" if dtype == torch.float32 else "randn"
    c = sk.fq_case(family, "stride", mode, dtype, 1, 8)
    assert c["rows"] * c["C"] > 4096 * 256
    _run_fakequant(dev, c, mode, 1, 8, "%s stride mode %d %s" % (family, mode, dtype))


# ----------------------------------------------------------------------------------------------- dgq_max_f32 / dgq_logquant_f32
@pytest.mark.parametrize("static", [False, True], ids=["realtime", "static"])
@pytest.mark.parametrize("skip_cols", [0, 1])
@pytest.mark.parametrize("shape", list(sk.LOG_SHAPES))
def test_max_and_logquant_tie_aware(shape, skip_cols, static, dev):
    from dgq_amd import ops
    c = sk.log_case(shape, skip_cols, static)
    p = c["p"]
    m = sk.max_ref(p, skip_cols)
    pd = p.to(dev)
    got_m = ops.max_f32(pd, skip_cols)
    assert float(got_m.cpu()) == m, (float(got_m.cpu()), m)
    assert sk.same_bits(pd, p)
    delta = c["delta"] if static else torch.tensor([m])
    dd = delta.to(dev) if static else got_m
    for bits in (6, 8):
        lo, hi, decided = sk.logquant_ref(p, delta, bits, skip_cols)
        share = 1.0 - float(decided.double().mean())
        assert share <= sk.LOG_UNDECIDED_CAP, share
        what = "%s skip %d %s b%d" % (shape, skip_cols, "static" if static else "real-time", bits)
        x = p.to(dev)
        out = torch.full_like(x, -1.0)
        y = ops.logquant_f32(x, dd, bits, skip_cols, out=out)
        assert y.data_ptr() == out.data_ptr() and sk.same_bits(x, p), "%s out=: the input changed" % what
        bad = sk.logquant_check(y, lo, hi)
        assert bad == 0, "%s out=: %d elements equal neither admissible value (%d undecided of %d)" % (what, bad, int((~decided).sum()), p.numel())
        y2 = ops.logquant_f32(x, dd, bits, skip_cols)                                       # in place
        assert y2.data_ptr() == x.data_ptr()
        assert sk.same_bits(y2, y.cpu()), "%s: in place and out= differ" % what
        yc = y.cpu()
        live, ylive = p[..., skip_cols:], yc[..., skip_cols:]
        zero_val = (torch.exp2(torch.tensor(-float(2 ** bits - 1), dtype=torch.float64)) * delta.double()).float()
        assert bool((ylive[live == 0] == zero_val).all()), "%s: a zero does not take the last code" % what
        if static:
            assert bool((ylive[live > delta] == delta).all()), "%s: a value above δ does not take code 0" % what
        if skip_cols:
            assert sk.same_bits(yc[..., 0].contiguous(), p[..., 0].contiguous()), "%s: column 0 was touched" % what


@pytest.mark.parametrize("bits", [6, 8])
def test_static_log_delta_search_picks_the_reference_quantile(bits, dev, monkeypatch):
    """T2ILogQuantizer._init_quantization_param on one of the cases: the three candidate δ are read back from its own logquant_f32 calls (the
    quantile is torch's, on the device); with those, the reference's float64 scores must name the δ it returns."""
    from dgq_amd import ops
    from dgq_amd.quant.quant_layer_text import T2ILogQuantizer
    p = sk.log_case("b2h4_70x77", 0, False)["p"]
    seen = []
    orig = ops.logquant_f32

    def spy(x, delta, *a, **kw):
        seen.append(delta.detach().cpu().reshape(-1).clone())
        return orig(x, delta, *a, **kw)
    monkeypatch.setattr(ops, "logquant_f32", spy)
    q = T2ILogQuantizer(bits=bits, always_zero=True, real_time=False)
    got = q._init_quantization_param(p.to(dev))
    assert len(seen) == 3 and all(s.numel() == 1 for s in seen), seen
    cands = [s[0] for s in seen]
    assert cands[0] < cands[1] < cands[2] <= p.max()
    scores = sk.log_init_scores(p, cands, bits)
    k = sk.log_init_pick(scores)
    print("static log δ search b%d: candidates %s, float64 score intervals %s, reference picks %s, device %.9g" % (
        bits, [float(c) for c in cands], scores, k, float(got)))
    assert k is not None, scores
    assert float(got.cpu()) == float(cands[k]), (float(got.cpu()), [float(c) for c in cands], k)


# ----------------------------------------------------------------------------------------------- dgq_minmax_rows_cols
def _check_minmax(got, x, what):
    want = sk.minmax_ref(x)
    for name, g, w, dim in (("rowmin", got[0], want[0], 1), ("rowmax", got[1], want[1], 1), ("colmin", got[2], want[2], 0), ("colmax", got[3], want[3], 0)):
        if g is None:
            continue
        g = g.cpu()
        assert g.dtype == torch.float32 and g.shape == w.shape
        assert bool((g == w).all()), "%s %s: %d of %d differ, first at %d" % (what, name, int((g != w).sum()), w.numel(), int((g != w).nonzero()[0]))
        ok = sk.zero_sign_checkable(x, w, dim)
        assert bool((torch.signbit(g[ok]) == torch.signbit(w[ok])).all()), "%s %s: sign of a zero extremum" % (what, name)


@pytest.mark.parametrize("dtype", sk.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("C", sk.MM_COLS)
@pytest.mark.parametrize("rows", sk.MM_ROWS)
def test_minmax_rows_cols_edges(rows, C, dtype, dev):
    """contiguous and as the column slice buf[:, 3:3 + C] of a poisoned buffer (ldx > C, unaligned base); rows 1 / 63 / 65 (one row slice,
    fewer and more than 64 rows), 64·256 + 1 (256 slices asked, 65 rows each: 253 used, the last one ragged with 5 rows); C = 1, 40 and 257
    (one column past a 256-column block); ±inf and ±0 inside (rows = 1: a column that holds nothing but +inf or −inf); rows-only and
    cols-only requests"""
    from dgq_amd import ops
    for sliced in (False, True):
        x, buf = sk.minmax_case(rows, C, dtype, sliced)
        if sliced:
            bd = buf.to(dev)
            xd = bd[:, 3:3 + C]
            assert xd.stride(0) == C + 9 and xd.stride(1) == 1
        else:
            xd = x.to(dev)
        what = "%d x %d %s%s" % (rows, C, dtype, " sliced" if sliced else "")
        _check_minmax(ops.minmax_rows_cols(xd), x, what)
        r = ops.minmax_rows_cols(xd, rows=True, cols=False)
        assert r[2] is None and r[3] is None
        _check_minmax(r, x, what + " rows only")
        r = ops.minmax_rows_cols(xd, rows=False, cols=True)
        assert r[0] is None and r[1] is None
        _check_minmax(r, x, what + " cols only")
        assert sk.same_bits(xd.contiguous(), x.contiguous())


# ----------------------------------------------------------------------------------------------- adaround / dgq_quantize_weight
@functools.lru_cache(maxsize=None)
def _adaround():
    c = sk.adaround_case()
    return c, sk.adaround_ref(c)


def _masked_allclose(got, want, want_open, edge, rtol, atol, what):
    """allclose outside ``edge``; on an edge element (a clamp mask within rounding of flipping) either 0 or the open formula"""
    got = got.detach().cpu().double()
    ok = ~edge
    assert torch.allclose(got[ok], want[ok], rtol=rtol, atol=atol), "%s: worst %.3g" % (what, float((got[ok] - want[ok]).abs().max()))
    e = got[edge]
    close = lambda a, b: (a - b).abs() <= atol + rtol * b.abs()
    assert bool((close(e, want_open[edge]) | (e == 0)).all()), "%s: an edge element is neither 0 nor the formula" % what


def test_adaround_kernels_above_the_grid_cap(dev):
    """640 x 640 = 409 600 elements > 1024 x 256 threads, α with the rectifier's edges planted; float64 formulas of csrc/adaround.hip's header
    under the tolerances of test_adaround_kernels_vs_oracle_and_reference_known_answers (copied from there, with its 0.01 loss weight)"""
    from dgq_amd import ops
    c, r = _adaround()
    assert c["alpha"].numel() > 1024 * 256
    w, d, z, gout = (c[k].to(dev) for k in ("w", "delta", "zp", "gout"))
    a = c["alpha"].to(dev).requires_grad_(True)
    out = ops.adaround_soft(w, d, z, a, c["bits"])
    (out * gout).sum().backward()
    assert torch.allclose(out.detach().cpu().double(), r["out"], rtol=0, atol=1e-6 * float(c["delta"].max()) * 2 ** c["bits"])
    _masked_allclose(a.grad, r["galpha"], r["galpha_open"], r["edge"], 2e-5, 1e-9, "soft backward")
    ok = ~r["edge"]
    assert ((a.grad.cpu() == 0)[ok]).eq((r["galpha"] == 0)[ok]).float().mean() > 0.9999
    for b, rb in r["reg"].items():
        a.grad = None
        v = ops.adaround_reg(a, b)
        (0.01 * v).backward()
        got = float(v.detach().cpu())
        print("adaround_reg b=%g: device %.6f, float64 %.6f, off by %.3g, summation bound %.3g" % (b, got, rb["value"], abs(got - rb["value"]), rb["bound"]))
        assert abs(got - rb["value"]) <= 2e-5 * abs(rb["value"]) + 1e-4, (b, got, rb["value"])
        assert abs(got - rb["value"]) <= rb["bound"], (b, got, rb["value"], rb["bound"])
        _masked_allclose(a.grad, rb["galpha"], rb["galpha_open"], r["edge_r"], 1e-4, 1e-8, "reg backward b=%g" % b)


@pytest.mark.parametrize("with_alpha", [False, True], ids=["rne", "alpha"])
@pytest.mark.parametrize("bits", [4, 8])
def test_quantize_weight_above_the_grid_cap(bits, with_alpha, dev):
    """1280 x 2304 = 2 949 120 elements > 8192 x 256 threads; quotient ties planted, zero points outside the code range, α with ±0.0"""
    from dgq_amd import ops
    c = sk.weight_case(bits=bits, with_alpha=with_alpha)
    assert c["w"].numel() > 8192 * 256
    want = sk.quantize_weight_ref(c)
    got = ops.quantize_weight(c["w"].to(dev), c["delta"].to(dev), c["zp"].to(dev), c["alpha"].to(dev) if with_alpha else None, bits).cpu()
    assert got.dtype == torch.uint8 and got.shape == want.shape
    assert torch.equal(got, want), "%d of %d codes differ, first at %s" % (int((got != want).sum()), want.numel(), (got != want).nonzero()[0].tolist())
