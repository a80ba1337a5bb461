"""F4 block goldens on the HIP path: the reference's own ``QuantBasicTransformerBlock`` (with its
``Attention_forward``: aqtizer_q/k/v, log2 / uniform aqtizer_w, start-peak) and ``QuantResnetBlock2D`` outputs, stored in
tests/golden/f4_blocks.pt by make_golden.py `small`, against this package's blocks running on libdgq_hip.so — directly, not
through the oracle.  Both graph forms: the unfused sequence of layer calls and the fused one bench.py times (LayerNorm / SiLU /
GroupNorm prologues, residual / GEGLU epilogues, batched q/k/v, fused attention).

Tolerance.  A block is a chain of 5-10 quantizers; the integer GEMMs differ from the reference's fp32 GEMMs by ~3e-7 per layer,
which flips an isolated activation code now and then (error = one quantisation step of one element).  Asserted: rel-L2 of the
block output <= 5e-3 and at least 95 % of the output elements within 1e-4 (of the reference's largest value) of the reference
(measured: transformer blocks 2e-7 / 100 %, the resnet block — two 3x3 convs behind GroupNorm — 1.6e-4 / 97.8 %)."""
import os
import sys

import pytest
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from tests.golden import recipes  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(HERE, "golden")


def _wrap_layers(root, wq, aq, kinds):
    from dgq_amd.quant.quant_layer import QuantLayer
    for _, mod in list(root.named_modules()):
        for cname, child in list(mod.named_children()):
            if isinstance(child, kinds):
                setattr(mod, cname, QuantLayer(child, dict(wq), dict(aq)))


def _install(qb, gold, act_suffix=""):
    """the reference's stored quantizer parameters -> this package's quantizer modules (what load_cali_model does for a ckpt)"""
    from dgq_amd.quant.quant_layer import QuantLayer
    for name, m in qb.named_modules():
        if isinstance(m, QuantLayer) and name in gold["wq"]:
            d, z = gold["wq"][name]
            m.wqtizer.delta, m.wqtizer.zero_point, m.wqtizer.init = d.cuda(), z.cuda(), True
    for name, (d, z) in gold["act"].items():
        q = qb.get_submodule(name + act_suffix)
        q.delta, q.zero_point, q.init = d.cuda(), z.cuda(), True


def _check(y, ref, what):
    y, ref = y.float().cpu().double(), ref.double()
    e = ((y - ref).norm() / ref.norm()).item()
    close = ((y - ref).abs() <= 1e-4 * ref.abs().max()).double().mean().item()
    print("%s: rel-L2 %.3g, %.2f %% of the elements within 1e-4 of the reference" % (what, e, 100 * close))
    assert e <= 5e-3 and close >= 0.95, (what, e, close)


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
@pytest.mark.parametrize("case", recipes.f4_tblock_cases(), ids=lambda c: c["name"])
def test_f4_transformer_block_hip_vs_reference(case, fused, monkeypatch):
    """diffusers_rewrite/sd.py:151-268 + quant/quant_block.py:121-186 (reference) == dgq_amd QuantBasicTransformerBlock on the GPU"""
    from dgq_amd.diffusers_rewrite.unet import BasicTransformerBlock
    from dgq_amd.quant import quant_block as qbm
    from dgq_amd.quant.quant_layer import Scaler
    monkeypatch.setattr(qbm, "FUSION", fused)
    gold = torch.load(os.path.join(GOLD, "f4_blocks.pt"))["tblock_" + case["name"]]
    inp = recipes.f4_tblock_inputs(case)
    blk = BasicTransformerBlock(recipes.F4_HIDDEN, 768, heads=8)
    blk.load_state_dict(inp["fp_sd"])
    wq = {"bits": 4, "channel_wise": True, "scaler": Scaler.MINMAX}
    aq = {"bits": case["abits"], "channel_wise": False, "scaler": Scaler.MINMAX, "leaf_param": True}
    sm = {"softmax_a_bit": case["abits"], "t2i_log_quant": case["log"], "t2i_real_time": case["rt"],
          "t2i_start_peak": case["sp"], "log_max_1": False}
    _wrap_layers(blk, wq, aq, (nn.Linear,))
    qb = qbm.QuantBasicTransformerBlock(blk, dict(aq), sm).cuda().eval()
    _install(qb, gold)
    qb.set_quant_state(True, True)
    with torch.no_grad():
        y = qb(inp["x"].cuda(), inp["ctx"].cuda())
    torch.cuda.synchronize()
    _check(y, gold["y"], "transformer block %s (%s)" % (case["name"], "fused" if fused else "unfused"))


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
@pytest.mark.parametrize("case", recipes.f4_tblock_cases(), ids=lambda c: c["name"])
def test_f4_transformer_block_materialised_attention(case, fused, monkeypatch):
    """The same blocks with no head dim in ops.ATTN_HEAD_DIMS, so that both attentions take the materialised branch of
    quant_block.attention_forward (matmul -> softmax -> dgq_max_f32 / dgq_logquant_f32 or dgq_fakequant_rows -> matmul, q/k/v through
    dgq_fakequant_rows): what calibration, reconstruction with gradients and other head dims run.  Same bound against f4_blocks.pt; the
    spies prove the branch — the test cannot pass through the fused kernel.  The distance to the fused path's output is printed only."""
    from dgq_amd import ops
    from dgq_amd.diffusers_rewrite.unet import BasicTransformerBlock
    from dgq_amd.quant import quant_block as qbm
    from dgq_amd.quant.quant_layer import Scaler
    monkeypatch.setattr(qbm, "FUSION", fused)
    gold = torch.load(os.path.join(GOLD, "f4_blocks.pt"))["tblock_" + case["name"]]
    inp = recipes.f4_tblock_inputs(case)
    blk = BasicTransformerBlock(recipes.F4_HIDDEN, 768, heads=8)
    blk.load_state_dict(inp["fp_sd"])
    wq = {"bits": 4, "channel_wise": True, "scaler": Scaler.MINMAX}
    aq = {"bits": case["abits"], "channel_wise": False, "scaler": Scaler.MINMAX, "leaf_param": True}
    sm = {"softmax_a_bit": case["abits"], "t2i_log_quant": case["log"], "t2i_real_time": case["rt"],
          "t2i_start_peak": case["sp"], "log_max_1": False}
    _wrap_layers(blk, wq, aq, (nn.Linear,))
    qb = qbm.QuantBasicTransformerBlock(blk, dict(aq), sm).cuda().eval()
    _install(qb, gold)
    qb.set_quant_state(True, True)
    x, ctx = inp["x"].cuda(), inp["ctx"].cuda()
    calls = {}

    def spy(name):
        orig = getattr(ops, name)

        def wrapped(*a, **kw):
            calls[name] = calls.get(name, 0) + 1
            return orig(*a, **kw)
        monkeypatch.setattr(ops, name, wrapped)
    for name in ("attention", "fakequant_rows", "logquant_f32", "max_f32"):
        spy(name)
    head_dims = ops.ATTN_HEAD_DIMS
    monkeypatch.setattr(ops, "ATTN_HEAD_DIMS", ())
    with torch.no_grad():
        y = qb(x, ctx)
    torch.cuda.synchronize()
    seen = dict(calls)
    calls.clear()
    monkeypatch.setattr(ops, "ATTN_HEAD_DIMS", head_dims)
    with torch.no_grad():
        y_fused_attn = qb(x, ctx)
    torch.cuda.synchronize()
    assert calls.get("attention", 0) == 2, calls                         # the comparison run did take the fused kernel
    calls = seen
    what = "transformer block %s (%s), materialised attention" % (case["name"], "fused" if fused else "unfused")
    print("%s: ops calls %s" % (what, calls))
    assert "attention" not in calls, calls
    assert calls.get("fakequant_rows", 0) >= 6, calls                    # q, k, v of both attentions
    if case["log"]:
        assert calls.get("logquant_f32", 0) == 2, calls
    if case["log"] and case["rt"]:
        assert calls.get("max_f32", 0) == 2, calls
    if not case["log"]:
        assert calls.get("fakequant_rows", 0) == 8, calls                # ... and the uniform softmax quantiser of both
    d = ((y.double() - y_fused_attn.double()).norm() / y_fused_attn.double().norm()).item()
    print("%s: rel-L2 to the fused attention path's output %.3g (not asserted)" % (what, d))
    _check(y, gold["y"], what)


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
def test_f4_resnet_block_hip_vs_reference(fused, monkeypatch):
    """quant/quant_block.py:79-119 (reference QuantResnetBlock2D, grouped conv inputs) == dgq_amd QuantResnetBlock2D on the GPU"""
    from dgq_amd.diffusers_rewrite.unet import ResnetBlock2D
    from dgq_amd.quant import quant_block as qbm
    from dgq_amd.quant.quant_layer import Scaler
    monkeypatch.setattr(qbm, "FUSION", fused)
    gold = torch.load(os.path.join(GOLD, "f4_blocks.pt"))["resnet_w4a8g8"]
    inp = recipes.f4_resnet_inputs()
    rb = ResnetBlock2D(64, 96)
    rb.load_state_dict(inp["fp_sd"])
    wq = {"bits": 4, "channel_wise": True, "scaler": Scaler.MINMAX}
    aq = {"bits": 8, "channel_wise": False, "scaler": Scaler.MINMAX, "leaf_param": True}
    _wrap_layers(rb, wq, aq, (nn.Linear, nn.Conv2d))
    qr = qbm.QuantResnetBlock2D(rb, dict(aq)).cuda().eval()
    _install(qr, gold, act_suffix=".aqtizer")
    for n in ("conv1", "conv2", "conv_shortcut"):
        getattr(qr, n).use_group_num = True
    qr.set_quant_state(True, True)
    with torch.no_grad():
        y = qr(inp["x"].cuda(), inp["temb"].cuda())
    torch.cuda.synchronize()
    _check(y, gold["y"], "resnet block (%s)" % ("fused" if fused else "unfused"))
