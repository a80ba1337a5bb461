"""CPU self-check of tests/gemm_epilogue_ref.py: the data of every cell is exact (margin < 1, and an fp32 emulation of the epilogue's own
operation order equals the float64 value bit for bit), the fused-quantiser data reaches every edge on purpose, every alignment class
and both sides of every vector / scalar choice occur, and each planted mistake changes a compared element of some cell."""
import pytest
import torch

from tests import gemm_epilogue_ref as er


def all_groups():
    """(label, cells) of everything the GPU file runs through the shared extras code"""
    for v in er.VARIANTS:
        yield "wxa8 M=%d W%d Kp=%s" % v, er.cells(*v)
    for fam, lay in (("panel", "perK"), ("panel", "perM"), ("blockq", "perK"), ("mx6", "perK")):
        yield "%s %s" % (fam, lay), er.layer_cells(fam, lay)
    yield "convq", er.convq_cells()



def _bits(t):
    return t.contiguous().view(er.INT_VIEW[t.dtype])


@pytest.mark.parametrize("label,cs", list(all_groups()), ids=lambda v: v if isinstance(v, str) else "")
def test_every_cell_is_exact(label, cs):
    for c in cs:
        assert er.margin(c) < 1.0, (label, c["name"], er.margin(c))
        want, emu = er.expected(c), er.emulate_f32(c)
        # (bit for bit, up to the sign of a zero: a negative GEGLU gate gives a·(−0))
        assert torch.equal(want.double(), emu.double()) and bool(torch.isfinite(want.double()).all()), c["name"]
        if not c["geglu"]:
            assert torch.equal(_bits(want), _bits(emu)), c["name"]


def test_sixteen_bit_outputs_are_rounded_not_trivially_exact():
    for c in er.cells(83):
        if c["out"] == "f32" or c["fq"] == 1:
            continue
        y64 = er.expected(dict(c, dtype=torch.float32)).double()            # the exact value (fp32 holds it: margin < 1)
        assert int((er.expected(c).double() != y64).sum()) > 0, c["name"]


def test_fused_quantiser_data_hits_its_edges():
    seen = {1: False, 2: False, 3: False}
    for c in er.cells(83):
        if not c["fq"]:
            continue
        e = er.edge_report(c)
        assert min(e["tie_even"], e["tie_odd"], e["clamp_lo"], e["clamp_hi"]) > 0, (c["name"], e)
        assert (e["bypass"] > 0) == (c["fq"] != 1), (c["name"], e)
        seen[c["fq"]] = True
    assert all(seen.values())
    assert 83 % er.FQ_T != 0 and 64 % er.FQ_T != 0 and 64 % er.FQ_D != 0 and 32 % er.FQ_D != 0


@pytest.mark.parametrize("mistake", er.MISTAKES)
def test_planted_mistake_is_noticed(mistake):
    hits = []
    for c in er.cells(83):
        good, bad = er.images(c), er.images(c, (mistake,))
        if any(not torch.equal(good[k], bad[k]) for k in good):
            hits.append(c["name"])
    assert hits, "no cell notices the planted mistake %r: the data is too weak" % mistake


def test_every_class_and_both_sides_of_every_choice_occur():
    cs = er.cells(83)
    for key, col in (("y", 2), ("y2", 3), ("res", 4)):
        assert {er.describe(c)[col] for c in cs} >= set(er.CLASSES), key
    for split in (False, True):
        ps = [er.paths(c, split) for c in cs]
        for k in ("y", "y2", "res", "geglu") + (("slab", "combine") if split else ()):
            assert {p[k] for p in ps} >= {"vec", "scalar"}, (k, split)
    pairs = {(p["y"], p["y2"]) for p in (er.paths(c) for c in cs)} | {("res", p["res"], p["y"]) for p in (er.paths(c) for c in cs)}
    assert {("vec", "scalar"), ("scalar", "vec"), ("res", "vec", "scalar"), ("res", "scalar", "vec")} <= pairs
    assert {c["N"] % 4 for c in cs} == {0, 1, 2, 3} and {c["Kp"] for c in cs} == {128, 384} and {c["per_m"] for c in cs} == {0, 1}
    res = [c["res"] for c in cs if c["res"] is not None]
    assert {r[2] for r in res} == {1, 7} and 83 % 7 != 0 and 300 % 7 != 0
    assert any(c["out"] == "bf16" and c["res"] and c["res"][0] == "f32" for c in cs) and any(c["out"] == "f32" and c["res"] and c["res"][0] == "bf16" for c in cs)


def test_images_mark_everything_outside_the_window():
    c = [x for x in er.cells(83) if x["y2cls"] is not None][0]
    for key, lay, cols in (("y", c["y_layout"], c["cols"]), ("y2", c["y2_layout"], c["N"])):
        off, pitch, total = lay
        img = er.images(c)[key]
        inside = torch.zeros(total, dtype=torch.bool)
        idx = off + torch.arange(c["M"])[:, None] * pitch + torch.arange(cols)[None, :]
        inside[idx.reshape(-1)] = True
        assert off > 0 and pitch > cols and total > int(idx.max()) + 1
        assert bool((img[~inside] == er.SENTINEL[c["dtype"]]).all()) and not bool((img[inside] == er.SENTINEL[c["dtype"]]).any())
        bad = img.clone()
        bad[off + pitch + cols] += 1                                           # one element of the pitch gap of row 1
        assert er.first_mismatch(bad, img, c["dtype"], off, pitch, c["M"], cols)[:3] == (1, cols, "outside")


def test_layer_family_cells_cover_every_class_and_choice():
    for label, cs in list(all_groups())[len(er.VARIANTS):]:
        for col in (2, 3, 4):
            assert {er.describe(c)[col] for c in cs} >= set(er.CLASSES), (label, col)
        ps = [er.paths(c) for c in cs]
        for k in ("y", "y2", "res") + (() if label == "convq" else ("geglu",)):
            assert {p[k] for p in ps} >= {"vec", "scalar"}, (label, k)


def test_small_m_cells_are_exact_and_reach_their_edges():
    for (M, K, wbits) in er.SMALLM_CELLS:
        for N in set(er.SMALLM_N):
            c = er.smallm_case(M, K, N, wbits, 1)
            assert er.smallm_margin(c) < 1.0
            for dt in er.DTYPES.values():
                want, emu = er.smallm_expected(c, dt), er.smallm_emulate_f32(c, dt)
                assert torch.equal(_bits(want), _bits(emu)) and bool(torch.isfinite(want.double()).all())
                assert dt == torch.float32 or float(want.double().abs().max()) > 2.0 ** 11
    Ms, Ks = {c[0] for c in er.SMALLM_CELLS}, {c[1] for c in er.SMALLM_CELLS}
    assert Ms == {1, 3, 5} and any(K % 32 not in (0,) and ((K + 15) & ~15) % 32 == 16 for K in Ks) and any(K % 32 == 0 for K in Ks)
    assert any(w == 8 and K > 1024 for (_, K, w) in er.SMALLM_CELLS)          # W8: a second trip of the 1024-code K loop
