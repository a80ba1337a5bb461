"""The quantised attention family behind dgq_attention (attn_fused.hip, attn_bf16x3.hip + attn_bf16x3_dev.h, attn_one.hip) against the
float64 statement of tests/attention_quant_ref.py, per element, on peaked and edge data.

  * interval check: |o − o64| within the tie-aware a-priori bound, for every launch form (4 waves un-split, one launch, key split, 8 waves
    wide with one and two tiles per stage), every operand format (un-fused, QM 0 / 1 / 2 / 3, integer V on and off) and every data family;
    mode 0 (the exact-fp32 kernels) under the un-quantised bound;
  * read-out check: with a one-hot window as V the output IS the device's p̂, and every entry must be fp32(δ_dev·2^-code) bit for bit;
  * uniform data: the output is exact;
  * the refusal of a non-positive scale, determinism, finite outputs and an unchanged count of given-up δ exchanges.
tests/test_attention_quant_ref_cpu.py checks the reference itself (ambiguity caps, restatement, planted mistakes) without a GPU.
The forms are selected as the sibling tests select them: DGQ_ATTN_ONE / DGQ_ATTN_SPLIT, read per call; DGQ_ATTN_I8 stays unset."""
import math

import pytest
import torch

from dgq_amd import ops
from tests import attention_quant_ref as ar

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _no_exchange_gave_up():
    before = ops.attention_sync_timeouts()
    yield
    assert ops.attention_sync_timeouts() == before, "a workgroup of a one-launch call gave up the wait for δ"


def _form(monkeypatch, form):
    one, split = ar.FORMS[form]
    monkeypatch.delenv("DGQ_ATTN_I8", raising=False)
    for name, val in (("DGQ_ATTN_ONE", one), ("DGQ_ATTN_SPLIT", split)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)


def _run(case, fmt, quant, delta, v=None, v_exp=3, scale=None):
    D, T, S, H, Bn = case.shape
    mode, skip, bits = quant
    dev = torch.device("cuda:0")
    fq = ar.fq_tables(ar.FORMATS[fmt], T, S, D, skip, v_exp)
    if fq is not None:
        fq = tuple(None if f is None else (f[0], f[1].to(dev), f[2].to(dev), f[3], f[4]) for f in fq)
    d = torch.tensor([delta], dtype=torch.float32, device=dev) if delta is not None else None
    o = ops.attention(case.q.to(dev), case.k.to(dev), (case.v if v is None else v).to(dev), H, D, case.scale if scale is None else scale,
                      mode, skip, d, bits, fq=fq)
    torch.cuda.synchronize()
    o = o.cpu()
    assert o.shape == case.q.shape and o.dtype == torch.float32 and bool(torch.isfinite(o).all())
    return o


def _id(form, fmt, fam, sh, qu):
    return "%s-%s-%s-D%d_T%d_S%d_H%d-m%ds%db%d" % ((form, fmt, fam) + sh[:4] + qu)


# ------------------------------------------------------------------------------------------------------------------ interval check
@pytest.mark.parametrize("form,fmt,family,shape,quant", ar.CASES, ids=[_id(*c) for c in ar.CASES])
def test_quantised_attention_inside_the_float64_bound(form, fmt, family, shape, quant, monkeypatch):
    """row_offsets: the kernel is given the shifted tensors, the reference and its bound are those of the un-shifted ones"""
    case, delta, r, o64, bound = ar.reference(family, shape, quant, fmt)
    _form(monkeypatch, form)
    o = _run(case, fmt, quant, delta)
    worst = ar.worst_ratio(o, o64, bound)
    print("AQ|%s|%s|%s|%s|%s|ratio %.4f|rel-L2 %.3e" % (form, fmt, family, shape, quant, worst, float((o.double() - o64).norm() / o64.norm())))
    assert worst <= 1.0


@pytest.mark.parametrize("family,shape", ar.MODE0, ids=["%s-D%d_T%d_S%d" % ((f,) + sh[:3]) for f, sh in ar.MODE0])
def test_mode0_inside_the_unquantised_bound(family, shape, monkeypatch):
    case, delta, r, o64, bound = ar.reference(family, shape, (0, 0, 8), "unfused")
    _form(monkeypatch, "w4")
    o = _run(case, "unfused", (0, 0, 8), None)
    worst = ar.worst_ratio(o, o64, bound)
    print("AQ|fp32|unfused|%s|%s|(0, 0, 8)|ratio %.4f|rel-L2 %.3e" % (family, shape, worst, float((o.double() - o64).norm() / o64.norm())))
    assert worst <= 1.0


def test_mode0_negative_scale():
    """mode 0 multiplies by the scale before it takes the maximum: a negative scale is served, and is the softmax of the negated scores"""
    shape = (40, 129, 77, 2, ar.B)
    base = ar.make("random", shape)
    case = ar.Case("random", shape, base.q, base.k, base.v, -base.scale)
    r = ar.ref64(case, 0, 0, 8)
    o = _run(case, "unfused", (0, 0, 8), None)
    assert ar.worst_ratio(o, r.output(case.v, 2, 40), r.bound(case.v, 2, 40)) <= 1.0


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_quantised_modes_refuse_a_scale_that_is_not_positive(mode, monkeypatch):
    """their running maxima are taken over the unscaled scores: scale <= 0, nan and inf are refused before anything is launched"""
    case = ar.make("random", (40, 129, 77, 2, ar.B))
    _form(monkeypatch, "w4")
    for scale in (0.0, -case.scale, math.nan, math.inf, -math.inf):
        with pytest.raises(RuntimeError, match="scale"):
            _run(case, "unfused", (mode, 0, 8), 0.01 if mode >= 2 else None, scale=scale)
    _run(case, "unfused", (mode, 0, 8), 0.01 if mode >= 2 else None)


# ------------------------------------------------------------------------------------------------------------------ read-out
@pytest.mark.parametrize("form,fmt,family,shape,quant,j0", ar.READOUT, ids=["%s-%s-%s-D%d_S%d-m%ds%d-j%d" % (a, b, c, s[0], s[2], q[0], q[1], j) for a, b, c, s, q, j in ar.READOUT])
def test_every_probability_bit_for_bit(form, fmt, family, shape, quant, j0, monkeypatch):
    case = ar.make(family, shape)
    delta = ar.static_delta(case, *quant[:2]) if quant[0] >= 2 else None
    r = ar.ref64(case, *quant, delta=delta, fmt=ar.FORMATS[fmt])
    _form(monkeypatch, form)
    o = _run(case, fmt, quant, delta, v=ar.onehot_v(shape, j0), v_exp=0)
    d_dev, problems = ar.check_readout(o, r, shape, quant, j0, delta)
    print("AQREAD|%s|%s|%s|%s|%s|j0 %d|δ_dev %.9g|δ64 %.9g" % (form, fmt, family, shape, quant, j0, d_dev, r.delta))
    assert not problems, problems


# ------------------------------------------------------------------------------------------------------------------ uniform
@pytest.mark.parametrize("mode", [1, 3])
@pytest.mark.parametrize("form,fmt,shape", ar.UNIFORM, ids=["%s-%s-D%d_S%d" % (a, b, s[0], s[2]) for a, b, s in ar.UNIFORM])
def test_uniform_is_exact(form, fmt, shape, mode, monkeypatch):
    case, delta, want = ar.uniform_setting(shape, mode)
    _form(monkeypatch, form)
    o = _run(case, fmt, (mode, 0, 8 if mode == 1 else 6), delta)
    if not torch.equal(o, want):
        d = (o.double() - want.double()).abs()
        raise AssertionError("%d of %d elements differ, max |diff| %.3g" % (int((o != want).sum()), d.numel(), float(d.max())))


# ------------------------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("form,fmt,family,shape,quant", [
    ("w4", "qm0", "random", (80, 200, 77, 2, ar.B), (1, 1, 8)), ("one", "qm1", "delta_owner", (40, 200, 250, 2, ar.B), (1, 1, 8)),
    ("split", "qm2", "start_peak", (64, 200, 257, 2, ar.B), (1, 1, 8)), ("wide", "qm3", "random", (8, 300, 256, 64, ar.B), (1, 0, 8))],
    ids=["w4", "one", "split", "wide"])
def test_twice_gives_equal_bits(form, fmt, family, shape, quant, monkeypatch):
    case = ar.make(family, shape)
    _form(monkeypatch, form)
    assert torch.equal(_run(case, fmt, quant, None), _run(case, fmt, quant, None))
