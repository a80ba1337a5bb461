"""tests/standalone_kernels_ref.py against itself, against the oracle's fp32 formulas where they state the same thing, and against
planted mistakes: each wrong variant must be rejected by the very comparison tests/test_gpu_standalone_kernels.py makes, on the very
inputs it uses.  No GPU."""
import pytest
import torch

from oracle import dgq_oracle as orc
from tests import standalone_kernels_ref as sk


def test_quotient_identity():
    """fp32(float64(x)/float64(δ)) is torch's fp32 x/δ (IEEE) on 4 M pairs, magnitudes across the formats' range, ties included"""
    g = sk.gen("quotient")
    n = 1 << 22
    x = torch.randn(n, generator=g) * torch.exp(torch.randn(n, generator=g) * 8)
    d = sk._log_uniform(n, 1e-6, 1e3, g)
    x[: n // 8] = sk.tie_lattice(d[: n // 8], g)
    assert torch.equal(sk.quotient32(x, d), x / d)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_tie_lattice_holds_ties_and_both_neighbours(mode):
    for bits in (4, 8):
        c = sk.fq_case("ties", "t77_8x40", mode, torch.float32, 0, bits)
        idx, _ = sk.table_index(c["rows"], c["C"], c["T"], c["D"], mode, 0)
        d = c["delta"][idx]
        t = sk.quotient32(c["x"], d).double()
        f = t - torch.floor(t)
        tie, above, below = (f == 0.5), (f > 0.5) & (f < 0.5 + 1e-3), (f < 0.5) & (f > 0.5 - 1e-3)
        share = [float(m.double().mean()) for m in (tie, above, below)]
        print("ties mode %d b%d: exact fp32 ties %.3f, just above %.3f, just below %.3f of %d elements" % (mode, bits, *share, t.numel()))
        assert share[0] > 0 and share[1] > 0 and share[2] > 0, share
        assert int(tie.sum()) >= 100, "too few exact ties to carry the claim"
        # and inside the kernel's fast-path band, where the IEEE division decides: the product with fp32(1/δ) disagrees somewhere
        assert not torch.equal(sk.affine_codes(c["x"], d, torch.zeros_like(d), 1e9, recip=True), sk.affine_codes(c["x"], d, torch.zeros_like(d), 1e9))


def test_bigq_lattice_straddles_the_division_threshold_inside_the_code_range():
    for mode in (0, 1, 2):
        c = sk.fq_case("bigq", "t77_8x40", mode, torch.float32, 0, 8)
        idx, _ = sk.table_index(c["rows"], c["C"], c["T"], c["D"], mode, 0)
        t = sk.quotient32(c["x"], c["delta"][idx]).abs()
        assert float(t.min()) >= 9e4 and float(t.max()) <= 3.6e6
        assert bool((t < 3e6).any()) and bool((t >= 3e6).any())
        q = sk.affine_codes(c["x"], c["delta"][idx], c["zp"][idx], 255.0)
        inside = ((q > 0) & (q < 255)).double().mean()
        assert inside > 0.9, inside


def test_fakequant_reference_agrees_with_the_oracle_formula():
    """fp32 cells, the reference's own uaq (torch fp32 arithmetic): equal bit for bit on every family (no NaN in any of them)"""
    for family in sk.FQ_FAMILIES:
        for mode in (0, 1, 2):
            c = sk.fq_case(family, "t77_8x40", mode, torch.float32, 0, 8)
            idx, _ = sk.table_index(c["rows"], c["C"], c["T"], c["D"], mode, 0)
            want = orc.uaq(c["x"], c["delta"][idx], c["zp"][idx], 8)
            got = sk.fakequant_rows_ref(c["x"], c["T"], c["D"], mode, c["delta"], c["zp"], 0, 8)
            assert not torch.isnan(want).any()
            assert sk.same_bits(got, want), (family, mode, sk.count_bit_mismatches(got, want))


@pytest.mark.parametrize("dtype", sk.DTYPES, ids=["fp32", "fp16", "bf16"])
def test_fakequant_planted_mistakes_are_caught(dtype):
    def ref(c, mode, skip, bits, **kw):
        return sk.fakequant_rows_ref(c["x"], c["T"], c["D"], mode, c["delta"], c["zp"], skip, bits, **kw)
    for mode in (0, 1, 2):
        for shape in ("t77_8x40", "t129_2x8"):
            if dtype == torch.float32:                                   # the lattice is an fp32 claim
                c = sk.fq_case("ties", shape, mode, dtype, 0, 8)
                assert not sk.same_bits(ref(c, mode, 0, 8, rounding="away"), ref(c, mode, 0, 8)), ("away", mode, shape)
                assert not sk.same_bits(ref(c, mode, 0, 8, recip=True), ref(c, mode, 0, 8)), ("recip", mode, shape)
                c = sk.fq_case("bigq", shape, mode, dtype, 0, 8)
                # (mode 0 has a single δ, and for a single δ the product may happen to round like the quotient on a short lattice)
                assert mode == 0 or not sk.same_bits(ref(c, mode, 0, 8, recip=True), ref(c, mode, 0, 8)), ("recip bigq", mode, shape)
            c = sk.fq_case("saturate", shape, mode, dtype, 0, 6)
            assert not sk.same_bits(ref(c, mode, 0, 6, clamp_first=True), ref(c, mode, 0, 6)), ("clamp first", mode, shape)
            for family in ("randn", "saturate"):
                c = sk.fq_case(family, shape, mode, dtype, 1, 8)
                assert not sk.same_bits(ref(c, mode, 1, 8, skip_on="columns"), ref(c, mode, 1, 8)), ("skip", mode, shape)
                # the skipped rows keep their bits, −0.0 among them
                y = ref(c, mode, 1, 8).view(-1, c["T"], c["C"])
                x = c["x"].view(-1, c["T"], c["C"])
                assert sk.same_bits(y[:, 0], x[:, 0]) and bool(torch.signbit(x[:, 0].float())[x[:, 0] == 0].any())


LOG_CELLS = [(s, k, st, b) for s in sk.LOG_SHAPES for k in (0, 1) for st in (False, True) for b in (6, 8)]


@pytest.mark.parametrize("shape,skip_cols,static,bits", LOG_CELLS)
def test_log_cases_hold_the_undecided_cap_and_their_edges(shape, skip_cols, static, bits):
    c = sk.log_case(shape, skip_cols, static)
    p = c["p"]
    m = sk.max_ref(p, skip_cols)
    delta = c["delta"] if static else torch.tensor([m])
    assert float(delta) >= 1e-3 and not torch.isnan(p).any() and float(p.min()) >= 0
    lo, hi, decided = sk.logquant_ref(p, delta, bits, skip_cols)
    share = 1.0 - float(decided.double().mean())
    print("log case %s skip %d %s b%d: undecided share %.2e (CPU)" % (shape, skip_cols, "static" if static else "real-time", bits, share))
    assert share <= sk.LOG_UNDECIDED_CAP, share
    qmax = 2 ** bits - 1
    live = p[..., skip_cols:]
    # zeros take the last code (0 for 8 bits: 2^-255 is below the format), values above a static δ take code 0
    zero_val = (torch.exp2(torch.tensor(-float(qmax), dtype=torch.float64)) * delta.double()).float()
    assert bool((live == 0).any()) and bool((lo[..., skip_cols:][live == 0] == zero_val).all())
    if bits == 8:
        assert float(zero_val) == 0.0
    if static:
        above = live > delta
        assert bool(above.any()) and bool((lo[..., skip_cols:][above] == delta).all())
    if skip_cols:
        assert sk.same_bits(lo[..., 0].contiguous(), p[..., 0].contiguous())
        assert sk.max_ref(p, skip_cols, over_all=True) != m, "the planted mistake (column 0 counted) gives the same maximum"
        assert bool((p[..., 0] >= p.max(-1).values).all())
    if p.numel() > 4096 * 256:
        counted = p.clone()
        counted[..., :skip_cols] = 0.0
        first = int(torch.where(counted.view(-1) == m)[0][0])
        assert first >= 4096 * 256 and float(counted.view(-1)[:4096 * 256].max()) < m, "the maximum is not in the last round alone"
    # the comparison rejects a neighbouring code on a decided element, and the oracle's fp32 formula passes it
    assert sk.logquant_check(lo, lo, hi) == 0 and sk.logquant_check(hi, lo, hi) == 0
    wrong = lo.clone()
    k = int(torch.where(decided.view(-1) & (lo.view(-1) > 0))[0][5])
    wrong.view(-1)[k] *= 0.5
    assert sk.logquant_check(wrong, lo, hi) == 1
    o = orc.log_quant(live, delta.reshape(()), bits)
    assert sk.logquant_check(torch.cat([p[..., :skip_cols], o], -1), lo, hi) == 0


def test_log_init_scores_separate_the_candidates():
    """the static-δ search test reads the device's three candidates back; here: the quantiles of the CPU, and that the reference's scores
    differ by more than the undecided elements could move them (``log_init_pick`` returns None otherwise)"""
    c = sk.log_case("b2h4_70x77", 0, False)
    x = c["p"]
    deltas = [torch.quantile(x.reshape(-1), q) for q in (0.999, 0.9999, 0.99999)]
    for bits in (6, 8):
        scores = sk.log_init_scores(x, deltas, bits)
        k = sk.log_init_pick(scores)
        print("log init b%d: score intervals %s, pick %s" % (bits, scores, k))
        assert k is not None, scores
        assert abs(float(orc.log_quant_init_delta(x, bits)) - float(deltas[k])) == 0.0


@pytest.mark.parametrize("dtype", sk.DTYPES, ids=["fp32", "fp16", "bf16"])
def test_minmax_cases_and_the_ldx_mistake(dtype):
    for rows in sk.MM_ROWS[:3]:
        for C in sk.MM_COLS:
            x, buf = sk.minmax_case(rows, C, dtype, True)
            assert x.stride(0) == C + 9 and x.stride(1) == 1 and x.storage_offset() == 3
            assert not torch.isnan(x.float()).any() and bool(torch.isinf(x.float()).any()) or rows * C < 4
            good, bad = sk.minmax_ref(x), sk.minmax_ref(x, buf=buf)
            if rows > 1:
                assert not all(torch.equal(a, b) for a, b in zip(good, bad)), (rows, C)
            flat, _ = sk.minmax_case(rows, C, dtype, False)
            assert all(torch.equal(a, b) for a, b in zip(good, sk.minmax_ref(flat)))      # the view holds the contiguous case's data


def test_adaround_reference_vs_oracle_and_summation_bound():
    """float64 formulas against the oracle's fp32 autograd under the tolerances of test_adaround_kernels_vs_oracle_and_reference_known_answers
    (masks: outside the elements the reference itself calls undecided), and the a-priori bound of the regulariser's sum against an fp32 sum"""
    c = sk.adaround_case()
    r = sk.adaround_ref(c)
    a = c["alpha"].clone().requires_grad_(True)
    out = orc.adaround_soft(c["w"], c["delta"].view(-1, 1), c["zp"].view(-1, 1), a, c["bits"])
    (out * c["gout"]).sum().backward()
    assert torch.allclose(out.detach().double(), r["out"], rtol=0, atol=1e-6 * float(c["delta"].max()) * 2 ** c["bits"])
    ok = ~r["edge"]
    assert int(r["edge_r"].sum()) >= 54, "the planted rectifier edges are not recognised"
    assert float(r["edge"].double().mean()) < 1e-3
    assert torch.allclose(a.grad.double()[ok], r["galpha"][ok], rtol=2e-5, atol=1e-9)
    for b, rb in r["reg"].items():
        a.grad = None
        v = orc.adaround_round_loss(a, b)
        (0.01 * v).backward()
        v = v.detach()
        assert abs(float(v) - rb["value"]) <= rb["bound"], (b, float(v), rb["value"], rb["bound"])
        assert rb["bound"] <= 2e-4 * rb["value"], "the bound says nothing: %g of %g" % (rb["bound"], rb["value"])
        assert torch.allclose(a.grad.double()[ok], rb["galpha"][ok], rtol=1e-4, atol=1e-8), b
        print("adaround reg b=%g: Σ %.6f, bound %.3g (depth %d), fp32 torch sum off by %.3g" % (b, rb["value"], rb["bound"], rb["depth"], abs(float(v) - rb["value"])))


@pytest.mark.parametrize("bits", [4, 8])
def test_quantize_weight_reference_vs_oracle_and_planted_mistakes(bits):
    c = sk.weight_case(bits=bits)
    d, z = c["delta"].view(-1, 1), c["zp"].view(-1, 1)
    want = sk.quantize_weight_ref(c)
    assert torch.equal(want, orc.uaq_codes(c["w"], d, z, bits).to(torch.uint8))
    assert int(sk.is_exact_tie(c["w"], d).sum()) > 1000
    assert not torch.equal(sk.quantize_weight_ref(c, rounding="away"), want)
    assert not torch.equal(sk.quantize_weight_ref(c, clamp_first=True).to(torch.uint8), want)
    ca = sk.weight_case(bits=bits, with_alpha=True)
    al = ca["alpha"]
    assert bool(((al == 0) & torch.signbit(al)).any()) and bool(((al == 0) & ~torch.signbit(al)).any())
    d = ca["delta"].view(-1, 1)
    hard = orc.adaround_hard(ca["w"], d, ca["zp"].view(-1, 1), al, bits) / d + ca["zp"].view(-1, 1)
    assert torch.equal(sk.quantize_weight_ref(ca), torch.round(hard).to(torch.uint8))
    assert ca["w"].numel() > 8192 * 256
