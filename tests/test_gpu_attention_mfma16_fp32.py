"""Un-quantised attention of the fp32 state on the bf16 matrix cores (dgq_attention_mfma16_f32, ops.attention_mfma16_f32, the attention
modules' attention_mfma16_fp32 flag, QuantModel.set_attention_mfma16_fp32, inference_qmodel --attn_mfma16_fp32).

The contract, as for the 16-bit entry (tests/test_gpu_attention_mfma16.py):
  * on data where every value the kernel forms is exact (one-hot scores: attention is a gather of 16-bit-significand values that the
    two planes carry whole; zero scores: a mean of small integers, which pins the IEEE division) the output is the expected tensor
    bit for bit;
  * on random fp32 data every element satisfies the a-priori bound of tests/attention_split_ref.py against float64,
        |o − o64| <= (2E + 2^-15)·A + 2^-24·|o64|,   E = (3·2^-18 + 3·D·2^-24)·G,
    which a plain torch restatement of the kernel's statement stays inside on the CPU — and which the same restatement with any one
    cross term left out exceeds (the first four tests need no GPU)."""
import pytest
import torch

from dgq_amd import ops, _lib
from tests import attention_mfma16_ref as ar
from tests import attention_split_ref as sr

gpu = pytest.mark.gpu
cases = pytest.mark.parametrize("case", ar.CASES, ids=["D%d_T%d_S%d_H%d" % c for c in ar.CASES])
RANDOM = [(c, ar.B) for c in ar.CASES] + [(ar.LONG, 1)]
random_cases = pytest.mark.parametrize("case,Bn", RANDOM, ids=["D%d_T%d_S%d_H%d" % c for c, _ in RANDOM])
qmuls = pytest.mark.parametrize("qmul", [1.0, 6.0], ids=["q1", "q6"])
ENTRY = "dgq_attention_mfma16_f32"


# ------------------------------------------------------------------------------------------------------------- 1. - 4. no GPU
def test_export_and_argument_checks():
    lib = _lib.load()
    assert lib.dgq_version() == 123
    f = getattr(lib, ENTRY)
    ptr = 1 << 20                        # never dereferenced: every call below is refused before a launch
    args = dict(q=ptr, k=ptr, v=ptr, o=ptr, B=1, H=2, T=5, S=7, D=40)

    def call(**kw):
        a = dict(args, **kw)
        return f(a["q"], a["k"], a["v"], a["o"], a["B"], a["H"], a["T"], a["S"], a["D"], 0.5, None)
    bad = [(dict(q=None), "null"), (dict(k=None), "null"), (dict(v=None), "null"), (dict(o=None), "null"),
           (dict(B=0), "geometry"), (dict(H=0), "geometry"), (dict(T=0), "geometry"), (dict(S=-1), "geometry"),
           (dict(D=32), "D=32"), (dict(D=0), "D=0"),
           (dict(q=ptr + 4), "aligned"), (dict(k=ptr + 8), "aligned"), (dict(v=ptr + 4), "aligned"), (dict(o=ptr + 12), "aligned")]
    for kw, what in bad:
        assert call(**kw) == -1, kw                                                    # DGQ_EINVAL
        assert ENTRY in _lib.last_error() and what in _lib.last_error(), (kw, _lib.last_error())


def test_setter_and_cli_refusals():
    from dgq_amd import inference_qmodel
    from dgq_amd.diffusers_rewrite import UNet2DConditionModel
    from dgq_amd.diffusers_rewrite.unet import Attention
    from dgq_amd.quant import QuantModel, Scaler, QMODE
    qnn = QuantModel(model=UNet2DConditionModel("tiny"), wq_params={"bits": 4, "channel_wise": True, "scaler": Scaler.MINMAX},
                     aq_params={"bits": 8, "channel_wise": False, "scaler": Scaler.MINMAX, "leaf_param": False},
                     softmax_aq_params={"softmax_a_bit": 8, "t2i_log_quant": False, "t2i_real_time": False, "t2i_start_peak": False,
                                        "log_max_1": False},
                     aq_mode=[QMODE.NORMAL.value, QMODE.QDIFF.value], tib_recon=False)
    attns = [m for m in qnn.modules() if isinstance(m, Attention)]
    assert len(attns) == 12 and Attention.attention_mfma16_fp32 is False and not any(m.attention_mfma16_fp32 for m in attns)
    qnn.set_attention_mfma16_fp32()
    assert all(m.attention_mfma16_fp32 is True for m in attns) and not any(m.attention_mfma16 for m in attns)
    qnn.set_attention_mfma16(True)                          # the 16-bit switch does not touch the fp32 one, either way
    qnn.set_attention_mfma16(False)
    assert all(m.attention_mfma16_fp32 is True for m in attns)
    qnn.set_attention_mfma16_fp32(False)
    assert not any(m.attention_mfma16_fp32 for m in attns)
    qnn.set_attention_mfma16(True)
    qnn.set_attention_mfma16_fp32(True)
    qnn.set_attention_mfma16_fp32(False)
    assert all(m.attention_mfma16 is True for m in attns) and not any(m.attention_mfma16_fp32 for m in attns)
    assert inference_qmodel.parse_args([]).attn_mfma16_fp32 is False
    assert inference_qmodel.parse_args(["--attn_mfma16_fp32"]).attn_mfma16_fp32 is True
    with pytest.raises(SystemExit) as e:                    # both are refused before anything is built
        inference_qmodel.main(["--attn_mfma16_fp32", "--use_aq", "--model_type", "tiny"])
    assert "--attn_mfma16_fp32" in str(e.value) and "--use_aq" in str(e.value)
    with pytest.raises(SystemExit) as e:
        inference_qmodel.main(["--attn_mfma16_fp32", "--fp16", "--model_type", "tiny"])
    assert "--attn_mfma16_fp32" in str(e.value) and "--fp16" in str(e.value)


@random_cases
@qmuls
def test_statement_is_inside_the_bound_on_cpu(case, Bn, qmul):
    """the bound, not the kernel, is what the GPU test trusts: the kernel's statement in plain torch stays inside it"""
    D, T, S, H = case
    q, k, v, scale, o64, A, G = sr.random_case(case, qmul, Bn)
    o = sr.restatement(q, k, v, H, D, scale)
    worst = sr.worst_ratio(o, o64, A, G, D)
    print("%s q x%g: restatement max |err| / bound = %.3f, rel-L2 %.3e" % (case, qmul, worst, float((o.double() - o64).norm() / o64.norm())))
    assert o.dtype == torch.float32 and worst <= 1.0


@pytest.mark.parametrize("term", sr.TERMS)
def test_the_bound_has_teeth(term):
    """a kernel that loses any one of the four cross terms is outside the bound"""
    case = (8, 70, 77, 3)
    D, T, S, H = case
    q, k, v, scale, o64, A, G = sr.random_case(case, 1.0)
    worst = sr.worst_ratio(sr.restatement(q, k, v, H, D, scale, omit=term), o64, A, G, D)
    print("%s without %s: max |err| / bound = %.1f" % (case, term, worst))
    assert worst > 1.0


# ------------------------------------------------------------------------------------------------------------- 5. / 6. exact data
def _run(q, k, v, H, D, scale):
    return ops.attention_mfma16_f32(q.cuda(), k.cuda(), v.cuda(), H, D, scale).cpu()


def _assert_equal(o, want, what):
    assert o.dtype == want.dtype == torch.float32 and o.shape == want.shape
    if not torch.equal(o, want):
        d = (o.double() - want.double()).abs()
        raise AssertionError("%s: %d of %d elements differ, max |diff| %.3g" % (what, int((o != want).sum()), d.numel(), float(d.max())))


@gpu
@cases
def test_onehot_attention_is_a_gather(case):
    D, T, S, H = case
    q, k, v, scale, want = sr.onehot_case(case)
    v_hi, v_lo = sr.split(v)
    assert torch.equal(v_hi + v_lo, v) and all(float(sr.split(x)[1].abs().max()) == 0.0 for x in (q, k))
    _assert_equal(_run(q, k, v, H, D, scale), want, "one-hot")


@gpu
@cases
def test_uniform_attention_counts_exactly_S_keys(case):
    """acc = S·c_d and l = S exactly; only an IEEE division returns c_d for every S (c·(1/S) does not)"""
    D, T, S, H = case
    q, k, v, scale, want = sr.uniform_case(case)
    _assert_equal(_run(q, k, v, H, D, scale), want, "uniform")


@gpu
@cases
@pytest.mark.parametrize("form", [0, 1, 2])
def test_every_lds_form_is_a_gather_too(case, form, monkeypatch):
    """the forms the entry does not take by default (DGQ_ATTN16F_FORM, read per call: 64- / 32-key stages, one buffer) stay measurable
    only while they stay right"""
    D, T, S, H = case
    q, k, v, scale, want = sr.onehot_case(case)
    monkeypatch.setenv("DGQ_ATTN16F_FORM", str(form))
    _assert_equal(_run(q, k, v, H, D, scale), want, "one-hot, form %d" % form)


# ------------------------------------------------------------------------------------------------------------- 7. random data
@gpu
@random_cases
@qmuls
def test_random_against_float64_per_element(case, Bn, qmul):
    D, T, S, H = case
    q, k, v, scale, o64, A, G = sr.random_case(case, qmul, Bn)
    o = _run(q, k, v, H, D, scale)
    assert o.dtype == torch.float32 and o.shape == q.shape and torch.isfinite(o).all()
    worst = sr.worst_ratio(o, o64, A, G, D)
    print("%s q x%g: max |err| / bound = %.3f, rel-L2 %.3e" % (case, qmul, worst, float((o.double() - o64).norm() / o64.norm())))
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------- 8. tiny UNet
class _Spy:
    """counts the library entries that ops calls"""

    def __init__(self, monkeypatch):
        self.names = []
        orig = ops._lib_call

        def call(name, *a):
            self.names.append(name)
            return orig(name, *a)
        monkeypatch.setattr(ops, "_lib_call", call)

    def take(self):
        n = self.names.count(ENTRY)
        self.names.clear()
        return n


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@gpu
def test_tiny_unet_routing_graphs_and_accuracy(monkeypatch, tmp_path):
    """Weight-only state of arch ``tiny`` (12 attention modules; no shape rule: every one is admitted).  An fp32 forward takes the entry
    once per attention with the new flag and never without — not with set_attention_mfma16 either; the 16-bit states and the
    quantised state never take it; a graph replay equals the eager run bit for bit and the setter drops a captured graph.  Accuracy
    against the project's own alternative to the exact route: e_split = rel-L2(flag on, exact fp32 route) <= 0.1·e_f16 = 0.1·rel-L2(f16
    state on the torch formulation, exact fp32 route)."""
    from dgq_amd import synth
    from tests import test_gpu_realtime_act as rta
    from tests.test_gpu_weight_only_mfma16 import _tiny_qnn
    spy = _Spy(monkeypatch)
    qnn = _tiny_qnn(4)
    inp = synth.synth_inputs("tiny", 2, 1, 16)
    x, ctx, t = inp["sample"].cuda(), inp["encoder_hidden_states"].cuda(), torch.tensor(999)
    N = 12
    with torch.no_grad():
        y_exact = qnn(x, t, ctx)[0].clone()
        assert spy.take() == 0
        qnn.set_attention_mfma16(True)
        y_16flag = qnn(x, t, ctx)[0].clone()
        assert spy.take() == 0 and torch.equal(y_16flag, y_exact)      # the 16-bit switch leaves the fp32 state on its exact kernel
        qnn.set_attention_mfma16(False)
        qnn.set_attention_mfma16_fp32(True)
        y_split = qnn(x, t, ctx)[0].clone()
        assert spy.take() == N
        assert y_split.dtype == torch.float32 and torch.isfinite(y_split).all()
        # graph replay == eager, bit for bit; the setter after a capture gives the other route, not a stale replay
        qnn.enable_graphs(True)
        qnn(x, t, ctx)
        assert spy.take() == 2 * N                              # warmed up and captured
        y_graph = qnn(x, t, ctx)[0].clone()
        assert spy.take() == 0                                  # a replay: no entry is called
        qnn.set_attention_mfma16_fp32(False)
        y_flip = qnn(x, t, ctx)[0].clone()
        y_flip_replay = qnn(x, t, ctx)[0].clone()
        assert spy.take() == 0
        qnn.set_attention_mfma16_fp32(True)
        y_back = qnn(x, t, ctx)[0].clone()
        assert spy.take() == 2 * N
        qnn.enable_graphs(False)
        assert torch.equal(y_graph, y_split) and torch.equal(y_back, y_split)
        assert torch.equal(y_flip, y_exact) and torch.equal(y_flip_replay, y_exact)
        assert not torch.equal(y_split, y_exact)
        # the 16-bit states never read the flag (f16 first: its torch-formulation output is e_f16's)
        qnn = qnn.half()
        y_f16 = qnn(x.half(), t, ctx.half())[0].float()
        assert spy.take() == 0
        qnn = qnn.to(torch.bfloat16)
        y_bf16 = qnn(x.bfloat16(), t, ctx.bfloat16())[0]
        assert spy.take() == 0 and torch.isfinite(y_bf16.float()).all()
        # nor does the quantised state
        path = str(tmp_path / "wonly.pth")
        synth.write_cali_ckpt(path, "tiny", 4, 8, 1, num_slots=1, seed=0, batch=2, res=16, start_peak=True, with_act=False)
        qq = rta._build_qnn(path, x.device)
        qq.set_quant_state(True, True)
        qq.set_attention_mfma16_fp32(True)
        yq = qq(x, t, ctx)[0]
        assert spy.take() == 0 and torch.isfinite(yq.float()).all()
    e_split, e_f16 = _rel(y_split, y_exact), _rel(y_f16, y_exact)
    print("tiny UNet, weight-only W4: rel-L2 to the exact fp32 route: dgq_attention_mfma16_f32 %.4e, f16 state on the torch formulation %.4e"
          % (e_split, e_f16))
    assert e_split <= 0.1 * e_f16


# ------------------------------------------------------------------------------------------------------------- 9. op and CLI
@gpu
def test_op_equals_direct_call_and_cli(tmp_path):
    from dgq_amd import inference_qmodel
    D, T, S, H = 40, 200, 333, 2
    q, k, v, scale = (x.cuda() if torch.is_tensor(x) else x for x in sr.random_case((D, T, S, H), 1.0)[:4])
    o = ops.attention_mfma16_f32(q, k, v, H, D, scale)
    o2 = torch.full_like(q, float("nan"))
    rc = getattr(_lib.load(), ENTRY)(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(o2), q.shape[0], H, T, S, D, scale, _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(o, o2)
    out = str(tmp_path / "lat_{rank}.pt")
    inference_qmodel.main(["--model_type", "tiny", "--attn_mfma16_fp32", "--num_inference_steps", "2", "--out", out])
    d = torch.load(out.format(rank=0))
    assert sorted(d) == [0, 1] and all(torch.isfinite(v).all() for v in d.values())
