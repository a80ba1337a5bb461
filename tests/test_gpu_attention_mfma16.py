"""Un-quantised attention on the 16-bit matrix cores (dgq_attention_mfma16, ops.attention_mfma16, the attention modules'
attention_mfma16 flag, QuantModel.set_attention_mfma16, inference_qmodel --attn_mfma16).

The contract has two halves:
  * on data where every value the kernel forms is exact (one-hot scores: attention is a gather; zero scores: attention is a mean of
    small integers) the output is the expected tensor bit for bit — a wrong lane map, key permutation, head or batch offset, a padded
    key counted in the row sum or a dropped tail key shows as a wrong number, not as noise;
  * on random data every element satisfies the a-priori bound of tests/attention_mfma16_ref.py against float64,
        |o − o64| <= (2u + 2E + 2^-16)·A + u·|o64|,
    which a plain torch restatement of the kernel's statement is checked against on the CPU (the first three tests need no GPU)."""
import pytest
import torch

from dgq_amd import ops, _lib
from tests import attention_mfma16_ref as ar

gpu = pytest.mark.gpu
IDS = {torch.bfloat16: "bf16", torch.float16: "f16"}
dtypes = pytest.mark.parametrize("dtype", ar.DTYPES, ids=[IDS[d] for d in ar.DTYPES])
cases = pytest.mark.parametrize("case", ar.CASES, ids=["D%d_T%d_S%d_H%d" % c for c in ar.CASES])
RANDOM = [(c, ar.B) for c in ar.CASES] + [(ar.LONG, 1)]
random_cases = pytest.mark.parametrize("case,Bn", RANDOM, ids=["D%d_T%d_S%d_H%d" % c for c, _ in RANDOM])


# ------------------------------------------------------------------------------------------------------------- 1. - 3. no GPU
def test_attention_mfma16_export_and_argument_checks():
    lib = _lib.load()
    assert lib.dgq_version() == 123
    f = lib.dgq_attention_mfma16
    ptr = 1 << 20                        # never dereferenced: every call below is refused before a launch
    args = dict(q=ptr, k=ptr, v=ptr, o=ptr, dtype=2, B=1, H=2, T=5, S=7, D=40)

    def call(**kw):
        a = dict(args, **kw)
        return f(a["q"], a["k"], a["v"], a["o"], a["dtype"], a["B"], a["H"], a["T"], a["S"], a["D"], 0.5, None)
    bad = [(dict(q=None), "null"), (dict(k=None), "null"), (dict(v=None), "null"), (dict(o=None), "null"),
           (dict(B=0), "geometry"), (dict(H=0), "geometry"), (dict(T=0), "geometry"), (dict(S=-1), "geometry"),
           (dict(D=32), "D=32"), (dict(D=0), "D=0"), (dict(dtype=3), "dtype"), (dict(dtype=-1), "dtype")]
    for kw, what in bad:
        assert call(**kw) == -1, kw                                                    # DGQ_EINVAL
        assert "dgq_attention_mfma16" in _lib.last_error() and what in _lib.last_error(), (kw, _lib.last_error())
    assert call(dtype=0) == -2 and "dgq_attention_mfma16" in _lib.last_error()         # DGQ_F32: DGQ_EUNSUPPORTED


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
    assert len(attns) == 12 and not any(m.attention_mfma16 for m in attns)
    qnn.set_attention_mfma16()
    assert all(m.attention_mfma16 is True for m in attns)
    qnn.set_attention_mfma16(False)
    assert not any(m.attention_mfma16 for m in attns)
    assert inference_qmodel.parse_args([]).attn_mfma16 is False and inference_qmodel.parse_args(["--attn_mfma16"]).attn_mfma16 is True
    with pytest.raises(SystemExit) as e:                    # both are refused before anything is built
        inference_qmodel.main(["--attn_mfma16", "--use_aq", "--fp16", "--model_type", "tiny"])
    assert "--use_aq" in str(e.value)
    with pytest.raises(SystemExit) as e:
        inference_qmodel.main(["--attn_mfma16", "--model_type", "tiny"])
    assert "--fp16" in str(e.value)


@dtypes
@random_cases
@pytest.mark.parametrize("qmul", [1.0, 6.0], ids=["q1", "q6"])
def test_statement_is_inside_the_bound_on_cpu(case, Bn, dtype, qmul):
    """the bound, not the kernel, is what the GPU test trusts: the kernel's statement in plain torch stays inside it"""
    D, T, S, H = case
    q, k, v, scale, o64, A, E = ar.random_case(case, dtype, qmul, Bn)
    o = ar.restatement(q, k, v, H, D, scale)
    worst = ar.worst_ratio(o, o64, A, E, dtype)
    print("%s %s q x%g: restatement max |err| / bound = %.3f" % (case, IDS[dtype], qmul, worst))
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------- 4. / 5. exact data
def _run(q, k, v, H, D, scale):
    return ops.attention_mfma16(q.cuda(), k.cuda(), v.cuda(), H, D, scale).cpu()


def _assert_equal(o, want, what):
    assert o.dtype == want.dtype and o.shape == want.shape
    if not torch.equal(o, want):
        d = (o.double() - want.double()).abs()
        raise AssertionError("%s: %d of %d elements differ, max |diff| %.3g" % (what, int((o != want).sum()), d.numel(), float(d.max())))


@gpu
@dtypes
@cases
def test_onehot_attention_is_a_gather(case, dtype):
    D, T, S, H = case
    q, k, v, scale, want = ar.onehot_case(case, dtype)
    _assert_equal(_run(q, k, v, H, D, scale), want, "one-hot")


@gpu
@dtypes
@cases
def test_uniform_attention_counts_exactly_S_keys(case, dtype):
    D, T, S, H = case
    q, k, v, scale, want = ar.uniform_case(case, dtype)
    _assert_equal(_run(q, k, v, H, D, scale), want, "uniform")


@gpu
@dtypes
@cases
def test_the_32_key_form_is_a_gather_and_counts_too(case, dtype, monkeypatch):
    """the form the entry does not take by default below D = 160 (DGQ_ATTN16_KT=32, read per call) stays measurable only while it stays
    right"""
    D, T, S, H = case
    monkeypatch.setenv("DGQ_ATTN16_KT", "32")
    q, k, v, scale, want = ar.onehot_case(case, dtype)
    _assert_equal(_run(q, k, v, H, D, scale), want, "one-hot, 32-key stages")
    q, k, v, scale, want = ar.uniform_case(case, dtype)
    _assert_equal(_run(q, k, v, H, D, scale), want, "uniform, 32-key stages")


# ------------------------------------------------------------------------------------------------------------- 6. random data
@gpu
@dtypes
@random_cases
@pytest.mark.parametrize("qmul", [1.0, 6.0], ids=["q1", "q6"])
def test_random_against_float64_per_element(case, Bn, dtype, qmul):
    D, T, S, H = case
    q, k, v, scale, o64, A, E = ar.random_case(case, dtype, qmul, Bn)
    o = _run(q, k, v, H, D, scale)
    assert o.dtype == dtype and o.shape == q.shape and torch.isfinite(o.float()).all()
    worst = ar.worst_ratio(o, o64, A, E, dtype)
    print("%s %s q x%g: max |err| / bound = %.3f, rel-L2 %.3e" % (case, IDS[dtype], qmul, worst,
                                                                 float((o.double() - o64).norm() / o64.norm())))
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------- 7. tiny UNet
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
        n = self.names.count("dgq_attention_mfma16")
        self.names.clear()
        return n


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@gpu
@dtypes
def test_tiny_unet_routing_graphs_and_accuracy(dtype, monkeypatch, tmp_path):
    """Weight-only state of arch ``tiny`` (12 attention modules).  The fp32 state and the quantised state never take the entry, flag
    or not; a 16-bit forward takes it once per attention with the flag and never without; a graph replay equals the eager run bit for
    bit and the setter drops a captured graph.  Accuracy against the parent route, measured here: with y32 the fp32-state output,
    e_new = rel-L2(new route, y32) <= 1.25·e_old = rel-L2(torch formulation, y32) — both are dominated by the layers' own 16-bit
    roundings, and the new route rounds less (fp32 scores), so they differ by rounding noise only."""
    from dgq_amd import synth
    from tests import test_gpu_realtime_act as rta
    from tests.test_gpu_weight_only_mfma16 import _tiny_qnn
    spy = _Spy(monkeypatch)
    qnn = _tiny_qnn(4)
    inp = synth.synth_inputs("tiny", 2, 1, 16)
    x, ctx, t = inp["sample"].cuda(), inp["encoder_hidden_states"].cuda(), torch.tensor(999)
    N = 12
    with torch.no_grad():
        qnn.set_attention_mfma16(True)
        y32 = qnn(x, t, ctx)[0].clone()
        assert spy.take() == 0                                  # the fp32 state keeps its exact kernel
        qnn.set_attention_mfma16(False)
        qnn = qnn.to(dtype)
        xd, cd = x.to(dtype), ctx.to(dtype)
        y_old = qnn(xd, t, cd)[0].clone()
        assert spy.take() == 0
        qnn.set_attention_mfma16(True)
        y_new = qnn(xd, t, cd)[0].clone()
        assert spy.take() == N
        assert y_new.dtype == dtype and torch.isfinite(y_new.float()).all()
        # graph replay == eager, bit for bit; the setter after a capture gives the other route, not a stale replay
        qnn.enable_graphs(True)
        qnn(xd, t, cd)
        assert spy.take() == 2 * N                              # warmed up and captured
        y_graph = qnn(xd, t, cd)[0].clone()
        assert spy.take() == 0                                  # a replay: no entry is called
        qnn.set_attention_mfma16(False)
        y_flip = qnn(xd, t, cd)[0].clone()
        y_flip_replay = qnn(xd, t, cd)[0].clone()
        assert spy.take() == 0
        qnn.set_attention_mfma16(True)
        y_back = qnn(xd, t, cd)[0].clone()
        assert spy.take() == 2 * N
        qnn.enable_graphs(False)
        assert torch.equal(y_graph, y_new) and torch.equal(y_back, y_new)
        assert torch.equal(y_flip, y_old) and torch.equal(y_flip_replay, y_old)
        assert not torch.equal(y_new, y_old)
        # the quantised state never reads the flag, 16-bit tensors or not
        path = str(tmp_path / "wonly.pth")
        synth.write_cali_ckpt(path, "tiny", 4, 8, 1, num_slots=1, seed=0, batch=2, res=16, start_peak=True, with_act=False)
        qq = rta._build_qnn(path, x.device).to(dtype)
        qq.set_quant_state(True, True)
        qq.set_attention_mfma16(True)
        yq = qq(xd, t, cd)[0]
        assert spy.take() == 0 and torch.isfinite(yq.float()).all()
    e_old, e_new = _rel(y_old.float(), y32), _rel(y_new.float(), y32)
    print("tiny UNet, weight-only W4, %s state: rel-L2 to the fp32 state: torch formulation %.4e, dgq_attention_mfma16 %.4e" % (IDS[dtype], e_old, e_new))
    assert e_new <= 1.25 * e_old


# ------------------------------------------------------------------------------------------------------------- 8. op and CLI
@gpu
def test_op_equals_direct_call_and_cli(tmp_path):
    from dgq_amd import inference_qmodel
    D, T, S, H = 40, 200, 333, 2
    q, k, v, scale = (x.cuda() if torch.is_tensor(x) else x for x in ar.random_case((D, T, S, H), torch.float16, 1.0)[:4])
    o = ops.attention_mfma16(q, k, v, H, D, scale)
    o2 = torch.full_like(q, float("nan"))
    rc = _lib.load().dgq_attention_mfma16(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(o2), _lib.DTYPE_CODE[q.dtype], q.shape[0], H, T, S, D,
                                          scale, _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(o, o2)
    out = str(tmp_path / "lat_{rank}.pt")
    inference_qmodel.main(["--model_type", "tiny", "--fp16", "--attn_mfma16", "--num_inference_steps", "2", "--out", out])
    d = torch.load(out.format(rank=0))
    assert sorted(d) == [0, 1] and all(torch.isfinite(v).all() for v in d.values())
