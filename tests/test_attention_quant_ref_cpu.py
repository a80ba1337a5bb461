"""The float64 reference of the quantised attention family (tests/attention_quant_ref.py) checked by itself, on the CPU: the conditions
under which its tie-aware bound means something, and the mistakes it has to see.  tests/test_gpu_attention_quant.py trusts the bound, not
the kernels; this module is why it may."""
import math

import pytest
import torch

from tests import attention_quant_ref as ar

IDS = ["%s-%s-%s-D%d_T%d_S%d_H%d-m%ds%db%d" % ((form, fmt, fam) + sh[:4] + qu) for form, fmt, fam, sh, qu in ar.CASES]


@pytest.mark.parametrize("form,fmt,family,shape,quant", ar.CASES, ids=IDS)
def test_ambiguity_caps_and_restatement(form, fmt, family, shape, quant):
    """few entries are ambiguous (<= 2^-8 of them, at least half of the rows have none), so the bound is tight almost everywhere; and the
    fp32 restatement of the statement stays inside it"""
    case, delta, r, o64, bound = ar.reference(family, shape, quant, fmt)
    share, rows = float(r.amb.float().mean()), float(r.amb.any(-1).float().mean())
    worst = ar.worst_ratio(ar.restatement(case, *quant, delta=delta), o64, bound)
    print("AQCPU|%s|%s|%s|%s|%s|share %.3e|rows %.3f|restatement %.3f" % (form, fmt, family, shape, quant, share, rows, worst))
    assert share <= 2.0 ** -8
    assert rows <= 0.5
    assert worst <= 1.0


@pytest.mark.parametrize("family,shape", ar.MODE0, ids=["%s-D%d_T%d_S%d" % ((f,) + sh[:3]) for f, sh in ar.MODE0])
def test_mode0_restatement(family, shape):
    case, delta, r, o64, bound = ar.reference(family, shape, (0, 0, 8), "unfused")
    assert not bool(r.amb.any())
    assert ar.worst_ratio(ar.restatement(case, 0, 0, 8), o64, bound) <= 1.0


def _scores(case):
    D, T, S, H, Bn = case.shape
    return torch.matmul(ar.heads(case.q.double(), H, D), ar.heads(case.k.double(), H, D).transpose(-2, -1)) * case.scale


SHAPES = sorted({(fam, sh) for _, _, fam, sh, _ in ar.CASES} | set(ar.MODE0))


@pytest.mark.parametrize("family,shape", [c for c in SHAPES if c[0] in ("start_peak", "late_peak")], ids=str)
def test_peaks_are_peaked(family, shape):
    """the peak key beats every other key of every row by 10 to 25 nats"""
    case = ar.make(family, shape)
    s = _scores(case)
    key = case.info["key"]
    assert key == (0 if family == "start_peak" else shape[2] - 1) and (family == "start_peak" or shape[2] % 32 == 1)
    others = torch.cat([s[..., :key], s[..., key + 1:]], -1).amax(-1)
    margin = s[..., key] - others
    print(family, shape, "margin %.2f .. %.2f nats" % (float(margin.min()), float(margin.max())))
    assert float(margin.min()) >= 10.0 and float(margin.max()) <= 25.0


@pytest.mark.parametrize("family,shape", [c for c in SHAPES if c[0].startswith("staircase")], ids=str)
def test_staircases_step_by_eight_nats(family, shape):
    """the maximum of tile g is its marked key; from tile to tile it moves by 8 nats (within the grid's rounding of the key) in the
    family's direction: every stage rescales (up), none after the first does (down), or the top is the first tile of the second half"""
    case = ar.make(family, shape)
    S = shape[2]
    s = _scores(case)
    NT = (S + ar.KT - 1) // ar.KT
    tmax = torch.stack([s[..., ar.KT * g:ar.KT * (g + 1)].amax(-1) for g in range(NT)], -1)
    marked = torch.stack([s[..., j] for j in case.info["keys"]], -1)
    assert torch.equal(tmax, marked)
    step = tmax[..., 1:] - tmax[..., :-1]
    sign = {"staircase_up": [1.0] * (NT - 1), "staircase_down": [-1.0] * (NT - 1),
            "staircase_mid": [1.0 if g < case.info["top"] else -1.0 for g in range(NT - 1)]}[family]
    err = (step - 8.0 * torch.tensor(sign, dtype=torch.float64)).abs().max()
    assert float(err) <= 1.0, float(err)
    if family == "staircase_mid":
        assert case.info["top"] == NT // 2                    # tile NT // 2 opens the second key half of a split launch


@pytest.mark.parametrize("family,shape", [c for c in SHAPES if c[0].startswith("row_offsets")], ids=str)
def test_row_offsets_shift_and_leave_softmax_alone(family, shape):
    case = ar.make(family, shape)
    want = 40.0 if family == "row_offsets" else 120.0
    D, T, S, H, Bn = shape
    s = _scores(case)
    s0 = torch.matmul(ar.heads(case.q_ref.double(), H, D), ar.heads(case.k_ref.double(), H, D).transpose(-2, -1)) * case.scale
    shift = s - s0
    sign = torch.where(torch.arange(T) % 2 == 0, 1.0, -1.0).double().view(1, 1, T, 1)
    assert float((shift - sign * case.info["shift"]).abs().max()) <= 1e-9 * want       # the same for every key of a row
    assert abs(case.info["shift"] - want) <= 0.05 * want
    if T > 1:
        assert float(s[:, :, 1::2].max()) < -0.5 * want                                  # half of the rows: every score far below zero


@pytest.mark.parametrize("family,shape", [c for c in SHAPES if c[0] == "delta_owner"], ids=str)
@pytest.mark.parametrize("skip", [0, 1])
def test_delta_owner_owns_delta(family, shape, skip):
    """one row — the last of the last (batch, head), in the ragged last query block — holds a probability of a key >= skip that is at
    least twice every other row's largest"""
    case = ar.make(family, shape)
    D, T, S, H, Bn = shape
    p = torch.softmax(_scores(case), -1)[..., skip:]
    rowmax = p.amax(-1)
    b, h, t = case.info["row"]
    assert (b, h, t) == (Bn - 1, H - 1, T - 1) and T % 128 != 0 and case.info["key"] >= skip
    own = float(rowmax[b, h, t])
    rowmax[b, h, t] = 0.0
    assert own >= 2.0 * float(rowmax.max()), (own, float(rowmax.max()))


#: mistake -> (family, shape, (mode, skip, bits)) on which the bound has to see it
PLANTED = {
    "codes_off_by_one": ("random", (40, 129, 77, 2, 2), (1, 0, 8)),
    "delta_over_all_keys": ("start_peak", (40, 129, 77, 2, 2), (1, 1, 8)),
    "column0_quantised": ("start_peak", (40, 129, 77, 2, 2), (1, 1, 8)),
    "last_key_dropped": ("late_peak", (40, 129, 33, 2, 2), (1, 0, 8)),
    "pad_key_scores_zero": ("row_offsets", (40, 129, 77, 2, 2), (1, 0, 8)),
    "max_starts_at_zero": ("row_offsets_deep", (40, 129, 77, 2, 2), (1, 0, 8)),
    "max_shared_by_row_pairs": ("row_offsets_deep", (40, 129, 77, 2, 2), (1, 0, 8)),
    "delta_of_batch0": ("delta_owner", (40, 129, 77, 2, 2), (1, 0, 8)),
    "stale_delta": ("random", (40, 129, 77, 2, 2), (1, 0, 8)),
}


@pytest.mark.parametrize("mistake", ar.MISTAKES)
def test_planted_mistake_is_detected(mistake):
    """each mistake, planted in the restatement, leaves the bound on the named family (the restatement without it stays inside)"""
    family, shape, quant = PLANTED[mistake]
    case, delta, r, o64, bound = ar.reference(family, shape, quant, "unfused")
    clean = ar.worst_ratio(ar.restatement(case, *quant, delta=delta), o64, bound)
    worst = ar.worst_ratio(ar.restatement(case, *quant, delta=delta, mistake=mistake), o64, bound)
    print("AQPLANT|%s|%s|clean %.3f|planted %.3g" % (mistake, family, clean, worst))
    assert clean <= 1.0 < worst


def test_planted_mistakes_are_all_named():
    assert set(PLANTED) == set(ar.MISTAKES)


@pytest.mark.parametrize("form,fmt,family,shape,quant,j0", ar.READOUT, ids=["%s-%s-%s-D%d_S%d-j%d" % (a, b, c, s[0], s[2], j) for a, b, c, s, _, j in ar.READOUT])
def test_readout_of_the_restatement(form, fmt, family, shape, quant, j0):
    """the read-out check accepts the restatement — and refuses it with a stale δ or shifted codes"""
    case = ar.make(family, shape)
    delta = ar.static_delta(case, *quant[:2]) if quant[0] >= 2 else None
    r = ar.ref64(case, *quant, delta=delta, fmt=ar.FORMATS[fmt])
    v = ar.onehot_v(shape, j0)
    d_dev, problems = ar.check_readout(ar.restatement(case, *quant, delta=delta, v=v), r, shape, quant, j0, delta)
    assert not problems, problems
    # (a log2 quantiser with half the δ gives every code one less and the same p̂, except at code 0: a window without one cannot tell)
    n = min(shape[0], shape[2] - j0)
    head = bool((r.code[..., max(j0, quant[1]):j0 + n] == 0).any())
    for mistake in ("stale_delta", "codes_off_by_one") if head else ("codes_off_by_one",):
        assert ar.check_readout(ar.restatement(case, *quant, delta=delta, v=v, mistake=mistake), r, shape, quant, j0, delta)[1]


@pytest.mark.parametrize("mode", [1, 3])
@pytest.mark.parametrize("form,fmt,shape", ar.UNIFORM, ids=["%s-%s-D%d_S%d" % (a, b, s[0], s[2]) for a, b, s in ar.UNIFORM])
def test_uniform_expectation_is_what_the_restatement_gives(form, fmt, shape, mode):
    case, delta, want = ar.uniform_setting(shape, mode)
    assert torch.equal(ar.restatement(case, mode, 0, 8 if mode == 1 else 6, delta=delta), want)
