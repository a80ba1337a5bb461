"""The block-staged convolution quantisers (quant_act_conv_kernel, and gemm_convq_kernel which quantises inside the GEMM launch) with
their gather tables resolved once per workgroup (csrc/quant_common.h: dgq_conv_tables_resolve / dgq_conv_quant_round): codes and row
sums must EQUAL the reference quantiser of tests/layer_reference.py (fp32 divide, round half to even, clamp — independent of the kernels).

Every per-K / per-M table here has power-of-two δ, so a row sum Σ δ·s is exact in fp32 in any order and ``check_codes`` (imported from
tests/test_gpu_layer_routes.py) can demand equality of the sums as well.  The geometries are the smallest that reach what the shared
step can get wrong: group sizes that are no multiple of 4 (packed dwords that are partly padding), partial tiles, stride 2, the folded
2x upsample, K past one 1024-code round (a partial last round), each of the three tiles, A6 / A8, 16-bit inputs, and inputs on the
rounding ties (n + ½)·δ_k, where the IEEE-division fallback of the tie band decides the code.

The block-staged path takes a layer only where its tile grid covers the chip (>= 256 tiles and >= 2048 rows, csrc/quant_act.hip:
conv_block_pays), so the small images come in batches that reach that; the B = 1 cells of the 8 x 8 images run too — on whatever variant
the planner gives them, which the spy records — next to the batch at which the tile in question launches.
"""
import functools
import math

import pytest
import torch

from tests import layer_reference as lr
from tests.test_gpu_layer_routes import Spy, build_layer, check_codes, host_route, rel_l2, run_layer, run_quantiser

G = 16


@pytest.fixture(scope="module")
def dev():
    from dgq_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def _gen(*parts):
    return torch.Generator().manual_seed(lr._seed("conv_tables", *parts))


def pow2_tables(case, layout, abits):
    """16 (δ, z) pairs with δ = 2^e, e in −2 .. 1, distinct through z (two of them outside the code range), dealt at random over the K
    entries (per-K: group sizes are no multiples of 4, asserted) or over the output positions (per-M)."""
    g = _gen("tables", case["name"], layout, abits)
    B, H, W, Ho, Wo, M, K, taps = lr.geometry(case)
    mid = 2 ** (abits - 1)
    gd = 2.0 ** torch.randint(-2, 2, (G,), generator=g).float()
    gz = (mid + 2.0 * (torch.arange(G) - G // 2)).float()
    gz[3], gz[11] = -3.0, float(2 ** abits + 2)
    n = K if layout == "perK" else Ho * Wo
    labels = torch.randint(0, G, (n,), generator=g)
    labels[:G] = torch.arange(G)[:n]
    if layout == "perK":
        assert any(int(c) % 4 for c in torch.bincount(labels, minlength=G)), "every group size is a multiple of 4"
        return gd[labels].view(1, -1, 1), gz[labels].view(1, -1, 1)
    return gd[labels].view(1, 1, -1), gz[labels].view(1, 1, -1)


def tie_input(case, adelta, g):
    """x on (n + ½)·δ of the element's centre tap (per-K) and one ulp either side, a third each: under the other taps' power-of-two δ
    the same value is a tie or a whole number as well."""
    B, C, H, W = case["B"], case["C"], case["H"], case["W"]
    taps = case["k"] ** 2
    d = adelta.reshape(-1)
    dc = d.view(C, taps)[:, taps // 2] if d.numel() == C * taps else torch.full((C,), float(d[0]))
    n = torch.randint(-9, 10, (B, C, H, W), generator=g).float()
    x = (n + 0.5) * dc.view(1, C, 1, 1)
    side = torch.randint(0, 3, (B, C, H, W), generator=g)
    up, down = torch.nextafter(x, torch.full_like(x, 1e9)), torch.nextafter(x, torch.full_like(x, -1e9))
    return torch.where(side == 1, up, torch.where(side == 2, down, x))


@functools.lru_cache(maxsize=None)
def cell(B, C, H, W, stride, upsample, layout, abits, dtype, ties, N=32):
    """One layer (weights included: ActBinding wants them) with its reference codes, computed once per distinct cell."""
    from dgq_amd import synth
    from oracle import dgq_oracle as orc
    case = lr.conv_case(B, C, H, W, stride, N, upsample=upsample)
    g = _gen("data", case["name"], layout, abits, dtype, ties)
    adelta, azp = pow2_tables(case, layout, abits)
    if ties:
        x = tie_input(case, adelta, g)
    else:
        x = torch.randn(B, C, H, W, generator=g) * 1.7 + 0.3
    x = x.to(dtype)                                            # the kernel reads these very values
    w = torch.randn(N, C, 3, 3, generator=g) * (9 * C) ** -0.5
    wd, wz = synth.channel_minmax(w, 4)
    Bq, Hq, Wq, Ho, Wo, M, K, taps = lr.geometry(case)
    d = dict(x=x, w_raw=w, w=orc.uaq(w, wd, wz, 4), wdelta=wd, wzp=wz, bias=torch.randn(N, generator=g) * 0.1,
             residual=torch.randn(B, N, Ho, Wo, generator=g), adelta=adelta, azp=azp, abits=abits, wbits=4, layout=layout)
    q, _ = lr.reference_codes(x.float(), adelta, azp, abits, "conv", 3, stride, 1, upsample)
    return case, d, lr.codes_rows(q, case)


def quantise_and_check(dev, monkeypatch, case, d, q_rows, want_variant=None, want_tile=None):
    from dgq_amd import _lib, ops
    lay, ab = build_layer(ops, case, d, dev)
    route = host_route(case, d)
    spy = Spy(ops, _lib)
    monkeypatch.setattr(ops, "_lib_call", spy)
    codes, rowsum, folded = run_quantiser(ops, case, ab, d["x"].to(dev))
    torch.cuda.synchronize()
    qc = [c for c in spy.take() if c["name"] == "dgq_quant_act_batch"]
    assert len(qc) == 1, qc
    assert qc[0]["variant"] == route["variant"], (qc, route)
    tile = route["tile"] if qc[0]["variant"] == 5 else 0
    print("%s %s a%d: variant %d tile %d%s Kp %d, %d rows" % (case["name"], d["layout"], d["abits"], qc[0]["variant"], tile,
                                                               " (partial)" if route["partial"] else "", route["Kp"], route["M"]))
    if want_variant is not None:
        assert qc[0]["variant"] == want_variant, "quantiser variant %d ran, the case is about variant %d; route %s" % (qc[0]["variant"], want_variant, route)
    if want_tile is not None:
        assert tile == want_tile, "tile %d ran, expected %d; route %s" % (tile, want_tile, route)
    if case["upsample"]:
        assert folded, "the 2x upsample was materialised, not folded into the load"
    check_codes(case, lay, codes, rowsum, q_rows, d, tile, "%s/%s a%d variant %d" % (case["name"], d["layout"], d["abits"], qc[0]["variant"]))
    return route


# C = 20 on 5 x 7: K = 180 in 16 groups (sizes no multiples of 4), every 4 x 8 tile partial; the batch makes the tile grid cover the chip
SMALL = [pytest.param(128, 20, 5, 7, 1, False, id="c20_5x7"),
         pytest.param(256, 20, 5, 7, 2, False, id="c20_5x7_stride2"),
         pytest.param(44, 20, 5, 7, 1, True, id="c20_5x7_upsampled"),
         pytest.param(128, 128, 6, 6, 1, False, id="c128_6x6_partial_last_round")]


@pytest.mark.gpu
@pytest.mark.parametrize("B,C,H,W,stride,ups", SMALL)
def test_per_k_small_geometries(B, C, H, W, stride, ups, dev, monkeypatch):
    case, d, q_rows = cell(B, C, H, W, stride, ups, "perK", 8, torch.float32, False)
    route = quantise_and_check(dev, monkeypatch, case, d, q_rows, want_variant=5, want_tile=1)
    if C == 128:
        assert route["Kp"] > 1024 and route["Kp"] % 1024, "the last 1024-code round is not partial"
    else:
        assert route["partial"], "no partial tile"


@pytest.mark.gpu
@pytest.mark.parametrize("B,C,H,W,stride,ups", [SMALL[0], SMALL[3]])
def test_per_m(B, C, H, W, stride, ups, dev, monkeypatch):
    case, d, q_rows = cell(B, C, H, W, stride, ups, "perM", 8, torch.float32, False)
    quantise_and_check(dev, monkeypatch, case, d, q_rows, want_variant=5, want_tile=1)


# the library's tile rule (csrc/quant_act.hip: conv_tile / conv_tile_geo) on 8 x 8 images: C = 320 fits the 4 x 4 tile (id 2) twice per CU
# and so takes it, unless that leaves the grid below 256 tiles — then, as for C = 640 and 1280 whose patches only fit it, the 2 x 4 tile
# (id 3).  B = 1 (64 rows) is below what the block-staged path takes at all: those cells run on the planner's other variant.
@pytest.mark.gpu
@pytest.mark.parametrize("C,B,tile", [(320, 1, 0), (640, 1, 0), (1280, 1, 0), (320, 64, 2), (320, 32, 3), (640, 32, 3), (1280, 32, 3)])
def test_tiles_at_8x8(C, B, tile, dev, monkeypatch):
    case, d, q_rows = cell(B, C, 8, 8, 1, False, "perK", 8, torch.float32, False)
    quantise_and_check(dev, monkeypatch, case, d, q_rows, want_variant=5 if tile else None, want_tile=tile)


@pytest.mark.gpu
@pytest.mark.parametrize("abits", [6, 8])
def test_a6_a8(abits, dev, monkeypatch):
    case, d, q_rows = cell(128, 20, 5, 7, 1, False, "perK", abits, torch.float32, False)
    quantise_and_check(dev, monkeypatch, case, d, q_rows, want_variant=5, want_tile=1)
    case, d, q_rows = cell(128, 20, 5, 7, 1, False, "perM", abits, torch.float32, False)
    quantise_and_check(dev, monkeypatch, case, d, q_rows, want_variant=5, want_tile=1)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_16_bit_input(dtype, dev, monkeypatch):
    case, d, q_rows = cell(128, 128, 6, 6, 1, False, "perK", 8, dtype, False)
    quantise_and_check(dev, monkeypatch, case, d, q_rows, want_variant=5, want_tile=1)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["perK", "perM"])
def test_rounding_ties(layout, dev, monkeypatch):
    """x on (n + ½)·δ_k and one ulp either side: the fast path's product with 1/δ cannot decide these, the fallback's division does"""
    case, d, q_rows = cell(128, 20, 5, 7, 1, False, layout, 8, torch.float32, True)
    quantise_and_check(dev, monkeypatch, case, d, q_rows, want_variant=5, want_tile=1)
    case, d, q_rows = cell(128, 128, 6, 6, 1, False, layout, 8, torch.float32, True)
    quantise_and_check(dev, monkeypatch, case, d, q_rows, want_variant=5, want_tile=1)


# ---- general-δ ties.  With δ = 2^e the product x·(1/δ) of the quantisers' fast path is exact, so test_rounding_ties cannot see a wrong tie
# band (dgq_affine_code_fast, dgq_common.h; dgq_affine_code4_fast, quant_common.h).  Here δ is log-uniform and x = fp32((n + ½)·δ) with its
# ±1 / ±2 ulp neighbours: about a fifth of such values are exact ties of the fp32 quotient, the others lie one or two of ITS ulps beside
# one (shares measured on the CPU by tests/test_standalone_kernels_ref_cpu.py) — inside the band, where only the IEEE division decides.
def general_tables(case, layout, abits):
    """``pow2_tables`` with δ log-uniform in [0.05, 2) instead of powers of two; Linear cases take their per-K table over K and their
    per-M table over the M rows, in the shapes layer_reference.real_tables gives them."""
    g = _gen("general tables", case["name"], layout, abits)
    B, H, W, Ho, Wo, M, K, taps = lr.geometry(case)
    lin = case["kind"] == "linear"
    mid = 2 ** (abits - 1)
    gd = torch.exp(torch.rand(G, generator=g, dtype=torch.float64) * (math.log(2.0) - math.log(0.05)) + math.log(0.05)).float()
    gz = (mid + 2.0 * (torch.arange(G) - G // 2)).float()
    gz[3], gz[11] = -3.0, float(2 ** abits + 2)
    n = K if layout == "perK" else (M if lin else Ho * Wo)
    labels = torch.randint(0, G, (n,), generator=g)
    labels[:G] = torch.arange(G)[:n]
    shape = {("perK", True): (1, 1, -1), ("perM", True): (1, -1, 1), ("perK", False): (1, -1, 1), ("perM", False): (1, 1, -1)}[(layout, lin)]
    return gd[labels].view(shape), gz[labels].view(shape)


def general_tie_input(case, layout, adelta, g):
    """x on fp32((n + ½)·δ), |n| <= 9, and one or two ulps either side, a fifth each.  δ is the element's own (Linear), the one of the
    element's centre tap (conv, per-K) or of the output position centred on the pixel (conv, per-M, stride 1): every value is on the
    lattice of at least one of the quantisers that read it, and an ordinary value under the others."""
    d = adelta.reshape(-1)
    if case["kind"] == "linear":
        M, K = case["M"], case["K"]
        dc = (d.view(1, 1, K) if layout == "perK" else d.view(1, M, 1)).expand(1, M, K)
    else:
        B, C, H, W = case["B"], case["C"], case["H"], case["W"]
        taps = case["k"] ** 2
        assert case["stride"] == 1 and not case["upsample"]
        dc = (d.view(1, C, taps, 1, 1)[:, :, taps // 2] if layout == "perK" else d.view(1, 1, H, W)).expand(B, C, H, W)
    n = torch.randint(-9, 10, dc.shape, generator=g).double()
    x = ((n + 0.5) * dc.double()).float()
    side = torch.randint(0, 5, dc.shape, generator=g)
    up, down = torch.full_like(x, float("inf")), torch.full_like(x, float("-inf"))
    x1u, x1d = torch.nextafter(x, up), torch.nextafter(x, down)
    for k, v in ((1, x1u), (2, x1d), (3, torch.nextafter(x1u, up)), (4, torch.nextafter(x1d, down))):
        x = torch.where(side == k, v, x)
    return x


@functools.lru_cache(maxsize=None)
def general_cell(kind, dims, layout, abits=8, N=32):
    """One layer under ``general_tables`` on ``general_tie_input`` with its reference codes; asserts that exact ties of the fp32 quotient
    and both kinds of neighbour occur among the codes inside the range."""
    from dgq_amd import synth
    from oracle import dgq_oracle as orc
    case = lr.linear_case(*dims, N) if kind == "linear" else lr.conv_case(*dims, N)
    g = _gen("general data", case["name"], layout, abits)
    adelta, azp = general_tables(case, layout, abits)
    x = general_tie_input(case, layout, adelta, g)
    B, H, W, Ho, Wo, M, K, taps = lr.geometry(case)
    lin = kind == "linear"
    w = torch.randn((N, K) if lin else (N, case["C"], 3, 3), generator=g) * K ** -0.5
    wd, wz = synth.channel_minmax(w, 4)
    d = dict(x=x, w_raw=w, w=orc.uaq(w, wd, wz, 4), wdelta=wd, wzp=wz, bias=torch.randn(N, generator=g) * 0.1,
             residual=torch.randn((1, M, N) if lin else (B, N, Ho, Wo), generator=g), adelta=adelta, azp=azp, abits=abits, wbits=4, layout=layout)
    q, _ = lr.reference_codes(x, adelta, azp, abits, kind, case.get("k", 1), case.get("stride", 1), case.get("pad", 0), False)
    cols = x if lin else torch.nn.functional.unfold(x, kernel_size=3, padding=1, stride=1)
    t = (cols.double() / adelta.double()).float().double()
    f = t - torch.floor(t)
    live = (q > 0) & (q < 2 ** abits - 1)
    for name, mask in (("exact ties", f == 0.5), ("values just above a tie", (f > 0.5) & (f < 0.5 + 1e-4)), ("values just below a tie", (f < 0.5) & (f > 0.5 - 1e-4))):
        assert int((mask & live).sum()) >= 8, "%s %s: %d %s inside the code range" % (case["name"], layout, int((mask & live).sum()), name)
    return case, d, lr.codes_rows(q, case)


def quantise_and_check_codes(dev, monkeypatch, case, d, q_rows, want_variant):
    """as test_real_layer_codes_and_output compares codes: torch.equal through kperm — no row-sum and no output claim (Σ δ·s is not exact
    under a general δ)"""
    from dgq_amd import _lib, ops
    from dgq_amd.plan import natural_kperm
    from tests.test_gpu_layer_routes import describe_code_mismatch
    lay, ab = build_layer(ops, case, d, dev)
    route = host_route(case, d)
    assert route["variant"] == want_variant, "the planners send %s %s to variant %d, the cell is about variant %d: %s" % (
        case["name"], d["layout"], route["variant"], want_variant, route)
    spy = Spy(ops, _lib)
    monkeypatch.setattr(ops, "_lib_call", spy)
    codes, rowsum, folded = run_quantiser(ops, case, ab, d["x"].to(dev))
    torch.cuda.synchronize()
    qc = [c for c in spy.take() if c["name"] == "dgq_quant_act_batch"]
    assert len(qc) == 1 and qc[0]["variant"] == want_variant, (qc, route)
    B, H, W, Ho, Wo, M, K, taps = lr.geometry(case)
    kperm = lay.kperm if lay.mode == "perK" else natural_kperm(K // taps, taps)
    m = kperm >= 0
    got, want = codes.cpu().int()[:, m], (q_rows[:, kperm[m].long()] - 2 ** (d["abits"] - 1)).int()
    if not torch.equal(got, want):
        raise AssertionError("%s %s variant %d: %s" % (case["name"], d["layout"], want_variant,
                                                        describe_code_mismatch(case, got, want, kperm[m], route["tile"] if want_variant == 5 else 0)))
    assert int(codes.cpu().int()[:, ~m].abs().sum()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["perK", "perM"])
def test_rounding_ties_general_delta_conv(layout, dev, monkeypatch):
    """conv variant 5 (c20_5x7, as test_rounding_ties) under a general δ"""
    case, d, q_rows = general_cell("conv", (128, 20, 5, 7, 1), layout)
    quantise_and_check_codes(dev, monkeypatch, case, d, q_rows, 5)


#: one Linear cell per quantiser variant a Linear input can take (test_route_table_is_complete lists 0 .. 5; 5 is the block-staged conv
#: path above): (variant, layout, M, K) with the smallest K at which quantiser_route gives the variant under ``general_tables`` (searched on
#: the CPU: K in steps of 2 for variants 1 / 2, of 4 for the others; the route does not depend on M at these K — 1, 16, 64 and 256 rows give
#: the same — and 64 rows make the lattice long enough to hold ties).  The cell's own host_route and the Spy confirm the variant.
#:   1  per-K, K no multiple of 4: the table gather from global;  2  per-M: the natural order (K = 2 is refused: K % 4);
#:   3  per-K, K % 4 == 0, padding of the groups >= K / 4;        0  per-K, K % 4 == 0, less padding than that: the staged strip;
#:   4  per-K, K > 4096: too wide for a staged strip.
LINEAR_VARIANT_CELLS = [(1, "perK", 64, 2), (2, "perM", 64, 4), (3, "perK", 64, 4), (0, "perK", 64, 824), (4, "perK", 64, 4100)]


@pytest.mark.gpu
@pytest.mark.parametrize("variant,layout,M,K", LINEAR_VARIANT_CELLS, ids=lambda v: str(v))
def test_rounding_ties_general_delta_linear(variant, layout, M, K, dev, monkeypatch):
    case, d, q_rows = general_cell("linear", (M, K), layout)
    quantise_and_check_codes(dev, monkeypatch, case, d, q_rows, variant)


@pytest.mark.gpu
@pytest.mark.parametrize("B,C,H,W,N", [(2, 32, 4, 8, 160), (1, 128, 8, 8, 320)])
@pytest.mark.parametrize("layout", ["perK", "perM"])
def test_convq_against_two_launch_form(B, C, H, W, N, layout, dev, monkeypatch):
    """The quantiser inside the GEMM launch against quantise launch + GEMM launch, on tables with padded group tails (per-K: asserted by
    pow2_tables).  Per-M: the integer contraction and one scale per row — the two outputs are EQUAL.  Per-K: the fused form flushes
    its group totals in another order than the two-launch GEMM, so both are held to the suite's bound against the float64 formula
    (2e-5 relative L2, test_real_layer_codes_and_output)."""
    from dgq_amd import _lib, ops
    monkeypatch.delenv("DGQ_GEMM_FORCE", raising=False)
    monkeypatch.delenv("DGQ_GEMM_FUSE_ALL", raising=False)
    case, d, _ = cell(B, C, H, W, 1, False, layout, 8, torch.float32, False, N)
    y_ref, _ = lr.reference_of(d, case)
    lay, ab = build_layer(ops, case, d, dev)
    route = host_route(case, d)
    assert route["conv_act_fuses"], "the library does not take this geometry in the fused form: %s" % route
    spy = Spy(ops, _lib)
    monkeypatch.setattr(ops, "_lib_call", spy)
    x, res = d["x"].to(dev), d["residual"].to(dev)
    out = {}
    for label, fuse in (("fused", True), ("two-launch", False)):
        monkeypatch.setattr(ops, "CONV_FUSE", fuse)
        spy.take()
        y = run_layer(ops, case, ab, x, res)
        torch.cuda.synchronize()
        calls = spy.take()
        gemm = [c for c in calls if c["name"] == "dgq_gemm_wxa8"]
        assert len(gemm) == 1 and gemm[0]["fused"] == fuse, (label, calls)
        assert len([c for c in calls if c["name"] == "dgq_quant_act_batch"]) == (0 if fuse else 1), (label, calls)
        out[label] = y.cpu()
        err = rel_l2(out[label], y_ref)
        print("%s %s %s: rel L2 against the float64 formula %.3g" % (case["name"], layout, label, err))
        assert err <= 2e-5, (label, err)
    if layout == "perM":
        assert torch.equal(out["fused"], out["two-launch"]), "%d elements differ" % int((out["fused"] != out["two-launch"]).sum())
