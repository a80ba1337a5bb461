"""Block wrappers — mirror of the reference's ``quant/quant_block.py``.

``QuantBasicTransformerBlock`` (quant_block.py:121-186) attaches ``aqtizer_{q,k,v,w}`` to both attentions and
owns the quantized attention forward (the reference swaps in ``Attention.Attention_forward``,
diffusers_rewrite/sd.py:151-207); ``QuantResnetBlock2D`` (quant_block.py:79-119) re-hosts the resnet
submodules.  Wrapping is by duck-typing, so both this package's UNet and the reference's
``diffusers_rewrite`` UNet classes are accepted.
"""
import os as _os
from typing import Dict

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .quant_layer import QuantLayer, UniformAffineQuantizer, StraightThrough
from .quant_layer_text import T2ILogQuantizer


#: Fold elementwise neighbours of a quantized layer into its two kernels (SiLU/GEGLU/GroupNorm in the quantise-on-load
#: pass; aqtizer_{q,k,v} and residual adds in the GEMM epilogue).  The teacher-forced parity test switches this off to
#: observe every intermediate tensor of the reference graph; tests/test_gpu_unet.py::test_fused_equals_unfused compares both.
FUSION = True
#: GroupNorm folding rounds differently from F.group_norm (x·(rstd·γ) + (β − mean·rstd·γ)); separate switch for tests.
FUSE_NORM = True
# Kernel-level fusions, each measured A/B on one MI355X box with bench.py (SD1.4 step, all bit-identical to the unfused
# sequence, tests/test_gpu_unet.py::test_fused_equals_unfused):
#   residual / temb-broadcast adds in the GEMM epilogue (residual tile prefetched as 16-byte loads)   +3.3 %
#   GEGLU a·gelu(g) inside ff.net.2's quantise-on-load pass                                           +1.5 %
#   SiLU(temb), GroupNorm(+SiLU), LayerNorm folded into the load pass                                 (see FUSE_NORM)
#   aqtizer_{q,k,v} in the attention pre-pass                                                         +0.3 %
#   aqtizer_{q,k,v} in the projection GEMM's epilogue (exact division per output inside under-filled grids)  slower: off
_F_RES = True
_F_FQ = False
_F_GEGLU = True
# ... or (round 3) in ff.net.0's GEMM epilogue: half the stores of the widest layer, no GEGLU pass in front of ff.net.2
_F_GEGLU_EPI = True
_F_SILU = True
# norm1/2/3 of the transformer block folded into the quantise-on-load pass of the layers that consume them
_F_LN = True
# layers that consume the same tensor share their launches (dgq_quant_act_batch / dgq_gemm_wxa8_batch): to_q/to_k/to_v of a
# self-attention (one input, three quantizer tables) and the to_k/to_v of EVERY cross-attention (one text context)
_F_QKV_BATCH = True
_F_CTX_BATCH = True
# the time_emb_proj(SiLU(temb)) projections of ALL resnet blocks in one launch (they depend on temb only): 46 launches -> 1
_F_TEMB_BATCH = True
# aqtizer_{q,k,v} applied inside the attention pre-pass (K/V while they are split into bf16 planes, Q into a scratch
# copy by extra blocks of the same launch): three launches per attention saved, nothing added to a GEMM grid
_F_ATTN_FQ = True


class BaseQuantBlock(nn.Module):
    def __init__(self, aq_params: dict = {}) -> None:
        super().__init__()
        self.use_wq = False
        self.use_aq = False
        self.act_func = StraightThrough()
        self.ignore_recon = False

    def set_quant_state(self, use_wq: bool = False, use_aq: bool = False) -> None:
        """quant_block.py:25-33: QuantLayers follow both flags; attentions only ``use_aq``."""
        for m in self.modules():
            if isinstance(m, QuantLayer):
                m.set_quant_state(use_wq=use_wq, use_aq=use_aq)
            if hasattr(m, "aqtizer_q") and hasattr(m, "to_q"):
                m.use_aq = use_aq


class TembGroup:
    """The time_emb_proj layers of one QuantModel.  The first resnet block that asks for its projection of a given
    ``temb`` tensor triggers ONE batched launch (ops.linear_smallm_batch) for every layer of the group; the others pick
    their result up.  Keyed by tensor identity, so it holds within one forward (and one graph capture) only."""

    def __init__(self, layers, epoch):
        self.layers = list(layers)
        self.epoch = epoch
        self._src, self._seen = None, -1
        self._out = {}

    def eligible(self, temb):
        return (temb.is_cuda and temb.dim() == 2 and temb.shape[0] <= ops.SMALLM_MAX_M and temb.shape[1] <= ops.SMALLM_MAX_K
                and temb.dtype in ops.FLOAT_DTYPES and temb.stride(1) == 1
                and all(l.on_integer_path(temb) and not l.aqtizer.calibrating() for l in self.layers))

    def get(self, layer, temb):
        if self._src is not temb or self._seen != self.epoch[0]:
            binds = [l._binding() for l in self.layers]
            if any(b.mode == "perK" or b.L != 1 for b in binds):
                return None                                   # a grouped table on a 2-D input does not occur; be safe
            self._out = dict(zip((id(l) for l in self.layers), ops.linear_smallm_batch(temb, binds, pre_act=1)))
            self._src, self._seen = temb, self.epoch[0]
        return self._out[id(layer)]


class CtxGroup:
    """The attn2.to_k / attn2.to_v layers of one QuantModel: they all project the same encoder_hidden_states tensor, so the
    first cross-attention of a forward computes every one of them with shared launches (ops.quant_linear_multi)."""

    def __init__(self, layers, epoch):
        self.layers = list(layers)
        self.epoch = epoch                # [n]: bumped by QuantModel before every run of the UNet (eager, warm-up, capture)
        self._src, self._seen = None, -1
        self._out = {}

    def eligible(self, ctx):
        return (torch.is_tensor(ctx) and ctx.is_cuda and ctx.dtype in ops.FLOAT_DTYPES
                and all(l.on_integer_path(ctx) and not l.aqtizer.calibrating() for l in self.layers))

    def get(self, layer, ctx):
        # valid for ONE run of the UNet only: the pipeline passes the same prompt_embeds object every step (other
        # contents under graph replay, other tables under time-aware slots), and a graph capture must contain the launches
        if self._src is not ctx or self._seen != self.epoch[0]:
            binds = [l._binding() for l in self.layers]
            self._out = dict(zip((id(l) for l in self.layers), ops.quant_linear_multi(ctx, binds)))
            self._src, self._seen = ctx, self.epoch[0]
        return self._out[id(layer)]


class QuantResnetBlock2D(BaseQuantBlock):
    def __init__(self, resnet: nn.Module, aq_params: dict = {}) -> None:
        super().__init__(aq_params)
        self.norm1 = resnet.norm1
        self.conv1 = resnet.conv1
        self.time_emb_proj = resnet.time_emb_proj
        self.norm2 = resnet.norm2
        self.dropout = resnet.dropout
        self.conv2 = resnet.conv2
        self.nonlinearity = resnet.nonlinearity
        self.conv_shortcut = resnet.conv_shortcut

    def _norm_act_conv(self, norm, conv, x, residual=None, bias_rows=None, final=False):
        """conv(SiLU(norm(x))) + residual (same shape) or + bias_rows[:, :, None, None] ([B, C_out]); final: the block's own result"""
        if FUSION and FUSE_NORM and isinstance(conv, QuantLayer) and isinstance(norm, nn.GroupNorm) and conv.can_fuse_prenorm(x):
            if _F_RES:
                return conv.forward_prenorm(x, norm, silu=True, residual=residual, bias_rows=bias_rows, final=final)
            y = conv.forward_prenorm(x, norm, silu=True)
        else:
            h = F.silu(norm(x))
            if residual is not None and FUSION and _F_RES and isinstance(conv, QuantLayer):
                return conv.forward_residual(h, residual)
            y = conv(h)
        if bias_rows is not None:
            y = y + bias_rows[:, :, None, None]
        return y if residual is None else residual + y

    def forward(self, input_tensor, temb):
        grp = getattr(self.time_emb_proj, "_temb_group", None)
        te = None
        if FUSION and _F_SILU and _F_TEMB_BATCH and grp is not None and grp.eligible(temb):
            te = grp.get(self.time_emb_proj, temb)                            # all resnet blocks' projections: one launch
            if te is not None:
                from .quant_layer import _tap
                te = _tap(self.time_emb_proj, te, x=temb, prologue=True)
        if te is not None:
            pass
        elif FUSION and _F_SILU and isinstance(self.time_emb_proj, QuantLayer):
            te = self.time_emb_proj.forward_fused(temb, pre_act=1)            # SiLU(temb) folded into the load
        else:
            te = self.time_emb_proj(F.silu(temb))
        h = self._norm_act_conv(self.norm1, self.conv1, input_tensor, bias_rows=te)   # + temb in conv1's epilogue
        sc = self.conv_shortcut(input_tensor) if self.conv_shortcut is not None else input_tensor
        return self._norm_act_conv(self.norm2, self.conv2, h, residual=sc, final=True)     # shortcut + conv2(...) in the epilogue


def _qparams_real_time(specs):
    """(mode 1, δ, z) of real-time attention-side quantizers for THIS call's projection outputs: one (δ, z) per token over batch and
    heads — the rows b·T + t of the [B·T][H·D] tensor folded over b (dgq_act_row_params with fold_T = T), the (1, T, 1) layout with the
    ``skip`` bypassed leading tokens dropped.  specs: [(tensor [B, T, H·D] contiguous, skip, bits)]; q, k and v of one attention share
    the launches."""
    tabs = ops.act_row_params_multi([(t, (t.shape[0] * t.shape[1], 1, 1, t.shape[2], 1, 1, 1, 0), bits, None, None, False, t.shape[1])
                                     for t, _skip, bits in specs])
    return [(1, d[skip:], z[skip:]) for (d, z), (_t, skip, _bits) in zip(tabs, specs)]


def _qparams(q: UniformAffineQuantizer, dev):
    """(mode, δ, z) of an attention-side quantizer for dgq_fakequant_rows on the [B·T, H·D] layout:
    () -> scalar; (1,T,1) -> per token; (1,1,D) -> per head-dim (quant_layer.py:311-313, 391-402)."""
    d = q.delta.detach()
    z = torch.as_tensor(q.zero_point).detach()
    cache = getattr(q, "_dev_cache", None)
    key = (d.data_ptr(), d._version, z.data_ptr() if z.numel() else 0, z._version, str(dev))
    if cache is not None and cache[0] == key:
        return cache[1]
    if d.numel() == 1:
        mode = 0
    elif d.dim() == 3 and d.shape[2] == 1:
        mode = 1
    elif d.dim() == 3 and d.shape[1] == 1:
        mode = 2
    else:
        raise NotImplementedError("attention quantizer δ shape %s" % (tuple(d.shape),))
    dd = d.reshape(-1).float().to(dev).contiguous()
    zz = z.reshape(-1).float().to(dev)
    zz = (zz.expand_as(dd) if zz.numel() == 1 else zz).contiguous()
    q._dev_cache = (key, (mode, dd, zz))
    return mode, dd, zz


class PreLN:
    """A tensor with an nn.LayerNorm pending.  QuantLayers on the integer path fold the norm into their quantise-on-load
    pass (``forward_fused(x, ln=norm)``), and so do weight-only matrix-core layers under ``QuantLayer.weight_only_fused``, from the
    row statistics cached here; anything else gets the materialised LayerNorm output (computed once)."""

    def __init__(self, x, norm):
        self.x, self.norm, self._y, self._stats = x, norm, None, None
        self.shape, self.device, self.dtype, self.is_cuda = x.shape, x.device, x.dtype, x.is_cuda

    def materialise(self):
        if self._y is None:
            self._y = self.norm(self.x)
        return self._y

    def row_stats(self):
        """(mean, rstd) of the rows, for the layers that fold the norm on the weight-only matrix-core route (QuantLayer.takes_fused):
        one launch for every consumer of the tensor — to_q, to_k and to_v of a self-attention share it"""
        if self._stats is None:
            self._stats = ops.layernorm_row_stats(self.x.reshape(-1, self.x.shape[-1]).contiguous(), float(self.norm.eps))
        return self._stats


def _fusable_ln(norm):
    return (FUSION and FUSE_NORM and _F_LN and isinstance(norm, nn.LayerNorm) and norm.elementwise_affine
            and norm.bias is not None and len(norm.normalized_shape) == 1)


def _prenorm(x, norm):
    return PreLN(x, norm) if (_fusable_ln(norm) and x.is_cuda and x.dtype in ops.FLOAT_DTYPES) else norm(x)


def _apply(layer, inp, **kw):
    """layer(inp) where inp may carry a pending LayerNorm"""
    if isinstance(inp, PreLN):
        if isinstance(layer, QuantLayer) and not layer.is_conv:
            if layer.takes_fused(inp.x) and ops.layernorm_row_stats_ok(inp.x.shape[-1]) and not kw.get("pre_act") and kw.get("fq") is None:
                kw = dict(kw, ln_stats=inp.row_stats())
            return layer.forward_fused(inp.x, ln=inp.norm, **kw)
        inp = inp.materialise()
    if kw:
        return layer.forward_fused(inp, **kw)
    return layer(inp)


class QuantBasicTransformerBlock(BaseQuantBlock):
    def __init__(self, tran: nn.Module, aq_params: dict = {}, softmax_aq_params: dict = {}) -> None:
        super().__init__(aq_params)
        self.norm1 = tran.norm1
        self.attn1 = tran.attn1
        self.norm2 = tran.norm2
        self.attn2 = tran.attn2
        self.norm3 = tran.norm3
        self.ff = tran.ff
        net = self.ff.net
        if (_F_GEGLU_EPI and len(net) == 3 and hasattr(net[0], "proj") and isinstance(net[0].proj, QuantLayer)
                and net[0].proj.w.shape[0] % 4 == 0):
            net[0].proj.geglu_rows = True                      # packed rows (value, gate) interleaved: see QuantLayer
        aq_params_qkv = dict(aq_params)
        aq_params_qkv.pop("real_time_format", None)            # (a layer-side format: the attention-side quantizers keep their integer per-token form)
        for attn in (self.attn1, self.attn2):
            attn.aqtizer_q = UniformAffineQuantizer(**aq_params_qkv)
            attn.aqtizer_k = UniformAffineQuantizer(**aq_params_qkv)
            attn.aqtizer_v = UniformAffineQuantizer(**aq_params_qkv)
        aq_params_w = dict(aq_params)
        aq_params_w.pop("real_time", None)                     # (the layer-side flag: aqtizer_w keeps t2i_log_quant / t2i_real_time)
        aq_params_w.pop("real_time_block", None)
        aq_params_w.pop("real_time_format", None)
        aq_params_w["bits"] = softmax_aq_params["softmax_a_bit"]
        aq_params_w["symmetric"] = False
        aq_params_w["always_zero"] = True
        if softmax_aq_params["t2i_log_quant"]:
            aq_params_w["real_time"] = softmax_aq_params["t2i_real_time"]
            aq_params_w["log_max_1"] = softmax_aq_params["log_max_1"]
            self.attn1.aqtizer_w = T2ILogQuantizer(**aq_params_w)
            self.attn2.aqtizer_w = T2ILogQuantizer(**aq_params_w)
        else:
            self.attn1.aqtizer_w = UniformAffineQuantizer(**aq_params_w)
            self.attn2.aqtizer_w = UniformAffineQuantizer(**aq_params_w)
        if softmax_aq_params["t2i_start_peak"]:
            self.attn2.start_peak = True                       # only ever set on attn2 (quant_block.py:157-158)
        self.attn1.use_aq = False
        self.attn2.use_aq = False
        self.attn1.forward = lambda hidden_states, encoder_hidden_states=None, _a=self.attn1: \
            quant_attention_forward(_a, hidden_states, encoder_hidden_states)
        self.attn2.forward = lambda hidden_states, encoder_hidden_states=None, _a=self.attn2: \
            quant_attention_forward(_a, hidden_states, encoder_hidden_states)

    def forward(self, x, encoder_hidden_states=None):
        if not FUSION:
            x = x + self.attn1(self.norm1(x))
            x = x + self.attn2(self.norm2(x), encoder_hidden_states=encoder_hidden_states)
            return x + self.ff(self.norm3(x))
        x = quant_attention_forward(self.attn1, _prenorm(x, self.norm1), None, residual=x)
        x = quant_attention_forward(self.attn2, _prenorm(x, self.norm2), encoder_hidden_states, residual=x)
        net = self.ff.net
        if len(net) == 3 and hasattr(net[0], "proj") and isinstance(net[1], nn.Dropout):
            if isinstance(net[0].proj, QuantLayer) and net[0].proj.geglu_rows and isinstance(net[2], QuantLayer):
                h2 = _apply(net[0].proj, _prenorm(x, self.norm3), geglu=True)   # value·gelu(gate) in ff.net.0's epilogue
                return net[2].forward_fused(h2, residual=x)
            h = _apply(net[0].proj, _prenorm(x, self.norm3))  # GEGLU projection (sd.py:210-236)
            if _F_GEGLU and isinstance(net[2], QuantLayer):
                return net[2].forward_fused(h, pre_act=2, residual=x)   # a·gelu(g) happens in ff.net.2's load
            a, g = h.chunk(2, dim=-1)
            h2 = net[1](a * F.gelu(g))
            if _F_RES and isinstance(net[2], QuantLayer):
                return net[2].forward_fused(h2, residual=x)             # x + ff(x) in the epilogue
            return x + net[2](h2)
        return x + self.ff(self.norm3(x))


def quant_attention_forward(attn, hidden_states, encoder_hidden_states=None, residual=None):
    """Quantized attention (replaces Attention.Attention_forward, sd.py:151-207).

    q/k/v quantizers run in place on the projection outputs in their [B·T, H·D] layout (a per-token or
    per-head-dim table addresses the same elements as the reference's [B,H,T,D] broadcast); the start-peak
    bypass of key token 0 / probability column 0 (sd.py:176-180,191-195) is a ``skip`` argument of the kernels
    instead of slice + concat."""
    start_peak = bool(getattr(attn, "start_peak", False))
    src = hidden_states if encoder_hidden_states is None else encoder_hidden_states
    H, D = attn.num_heads, attn.head_dim
    use_aq = bool(getattr(attn, "use_aq", False))

    # softmax-quantiser mode of dgq_attention_f32; where that kernel applies aqtizer_q/k/v itself on load, the three
    # separate fake-quant passes are skipped (pending[...] carries their tables instead)
    mode_w = 0
    if use_aq:
        wq_ = attn.aqtizer_w
        mode_w = (1 if wq_.real_time else 2) if isinstance(wq_, T2ILogQuantizer) else 3
    calibrating = use_aq and any(getattr(attn, n).calibrating() for n in ("aqtizer_q", "aqtizer_k", "aqtizer_v"))
    defer = (FUSION and _F_ATTN_FQ and use_aq and not calibrating and hidden_states.is_cuda
             and hidden_states.dtype in ops.FLOAT_DTYPES
             and D in ops.ATTN_HEAD_DIMS and (mode_w == 1 or attn.aqtizer_w.init)
             and ops.attention_fuses_fakequant(D, mode_w))
    pending = {}
    pending_rt = {}                                                  # real-time quantizers: name -> (tensor, skip, bits), resolved together

    # projections that share their launches: q/k/v of a self-attention (same input, LayerNorm folded once per problem) ...
    pre = {}
    from .quant_layer import _tap
    if (FUSION and _F_QKV_BATCH and not _F_FQ and encoder_hidden_states is None and not calibrating
            and all(isinstance(l, QuantLayer) and not l.is_conv for l in (attn.to_q, attn.to_k, attn.to_v))):
        xin = hidden_states.x if isinstance(hidden_states, PreLN) else hidden_states
        lnm = hidden_states.norm if isinstance(hidden_states, PreLN) else None
        if (all(l.on_integer_path(xin) for l in (attn.to_q, attn.to_k, attn.to_v)) and xin.dtype in ops.FLOAT_DTYPES
                and (lnm is None or (xin.shape[-1] % 4 == 0 and xin.shape[-1] <= 2048))):
            ys = ops.quant_linear_multi(xin, [l._binding() for l in (attn.to_q, attn.to_k, attn.to_v)],
                                        ln=(lnm.weight, lnm.bias, float(lnm.eps)) if lnm is not None else None)
            for nm, l, y in zip(("aqtizer_q", "aqtizer_k", "aqtizer_v"), (attn.to_q, attn.to_k, attn.to_v), ys):
                pre[nm] = _tap(l, y, x=xin, prologue=lnm is not None)
    # ... and the k/v projections of the text context, shared by every cross-attention of the model
    grp = getattr(attn.to_k, "_ctx_group", None)
    if (FUSION and _F_CTX_BATCH and not _F_FQ and encoder_hidden_states is not None and not calibrating and grp is not None
            and not isinstance(src, PreLN) and grp.eligible(src)):
        for nm, l in (("aqtizer_k", attn.to_k), ("aqtizer_v", attn.to_v)):
            pre[nm] = _tap(l, grp.get(l, src), x=src, prologue=False)

    def project(layer, name, inp, skip):
        """projection + its attention-side quantizer (fused into the attention kernel's loads when possible)"""
        qz = getattr(attn, name) if use_aq else None
        ntok = inp.shape[1]
        if name in pre:
            ten = pre[name]
            if defer and qz.real_time:
                ten = ten.contiguous()
                pending_rt[name] = (ten, skip, qz.bits)
                return ten
            if defer and qz.init:
                mode, dd, zz = _qparams(qz, ten.device)
                pending[name] = (mode, dd, zz, skip, qz.bits)
                return ten
            layer = lambda _x, _t=ten: _t                             # already projected: only the quantizer is left
            inp = ten
        if defer and qz.real_time:
            ten = _apply(layer, inp).contiguous()
            pending_rt[name] = (ten, skip, qz.bits)
            return ten
        if defer and qz.init:
            mode, dd, zz = _qparams(qz, inp.device)
            pending[name] = (mode, dd, zz, skip, qz.bits)
            return _apply(layer, inp)
        if (FUSION and _F_FQ and qz is not None and qz.init and not qz.real_time and isinstance(layer, QuantLayer)
                and layer.on_integer_path(inp.x if isinstance(inp, PreLN) else inp) and inp.dtype in ops.FLOAT_DTYPES):
            mode, dd, zz = _qparams(qz, inp.device)
            return _apply(layer, inp, fq=(mode + 1, dd, zz, ntok, D, skip, qz.bits))
        ten = _apply(layer, inp)
        if use_aq:
            bb, ntok, cc = ten.shape
            if not qz.init:                                          # first-forward scalar self-init
                view = ten.view(bb, ntok, H, D)
                qz.init_from(view[:, skip:] if skip else view)
            if qz.calibrating():                                     # DGQ calibration: the quantizer sees [B,H,T−skip,D]
                view = ten.view(bb, ntok, H, D)
                qz.observe((view[:, skip:] if skip else view).transpose(1, 2))
            ten = ten.contiguous()
            mode, dd, zz = _qparams_real_time([(ten, skip, qz.bits)])[0] if qz.real_time else _qparams(qz, ten.device)
            ops.fakequant_rows(ten.view(bb * ntok, cc), ntok, D, mode, dd, zz, skip, qz.bits)
        return ten

    q = project(attn.to_q, "aqtizer_q", hidden_states, 0)
    k = project(attn.to_k, "aqtizer_k", src, 1 if start_peak else 0)
    v = project(attn.to_v, "aqtizer_v", src, 0)
    if pending_rt:                                                   # one dgq_act_row_params_batch call for q, k and v
        names = list(pending_rt)
        for nm, (mode, dd, zz) in zip(names, _qparams_real_time([pending_rt[nm] for nm in names])):
            pending[nm] = (mode, dd, zz, pending_rt[nm][1], pending_rt[nm][2])
    b, t, c = q.shape
    s = k.shape[1]
    # weight reconstruction (reconstruction.py) differentiates through the block: the fused kernels have no backward, so a
    # forward that records a graph takes the materialised torch formulation below
    needs_grad = torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad)
    if (not use_aq and getattr(attn, "attention_mfma16_fp32", False) and q.is_cuda and q.dtype == k.dtype == v.dtype == torch.float32
            and D in ops.ATTN_HEAD_DIMS and not needs_grad):
        # opt-in (QuantModel.set_attention_mfma16_fp32): the un-quantised attention of the fp32 state in one launch on the bf16 matrix
        # cores (two-term bf16 splits, fp32 softmax: DESIGN.md §8) instead of the exact fp32 MFMA kernel below
        o = ops.attention_mfma16_f32(q.contiguous(), k.contiguous(), v.contiguous(), H, D, float(attn.scale))
        return _attn_out(attn, o, residual)
    if (D in ops.ATTN_HEAD_DIMS and q.is_cuda and q.dtype == k.dtype == v.dtype and not needs_grad
            and (q.dtype == torch.float32
                 or (q.dtype in ops.FLOAT_DTYPES and use_aq and ops.attention_fuses_fakequant(D, mode_w)))):
        # fused two-pass attention (dgq_attention_f32): probabilities are never materialised
        mode, delta, bits = 0, None, 8
        skip = 1 if (start_peak and use_aq) else 0
        if use_aq:
            wq = attn.aqtizer_w
            bits = wq.bits
            if isinstance(wq, T2ILogQuantizer):
                if wq.real_time:
                    mode = 1
                else:
                    if not wq.init:
                        _init_static_softmax_delta(attn, wq, q, k, b, t, s, H, D, skip)
                    mode, delta = 2, wq.delta.detach().reshape(1).float().to(q.device)
            else:
                if not wq.init:
                    _init_static_softmax_delta(attn, wq, q, k, b, t, s, H, D, skip)
                mode, delta = 3, wq.delta.detach().reshape(1).float().to(q.device)
        fq = tuple(pending.get(n) for n in ("aqtizer_q", "aqtizer_k", "aqtizer_v")) if pending else None
        o = ops.attention(q.contiguous(), k.contiguous(), v.contiguous(), H, D, float(attn.scale), mode, skip,
                              delta, bits, fq)
        return _attn_out(attn, o, residual)
    if (not use_aq and getattr(attn, "attention_mfma16", False) and q.is_cuda and q.dtype in (torch.float16, torch.bfloat16)
            and q.dtype == k.dtype == v.dtype and D in ops.ATTN_HEAD_DIMS and not needs_grad):
        # opt-in (QuantModel.set_attention_mfma16): the un-quantised attention of the 16-bit states in one launch on the bf16 / f16
        # matrix cores instead of matmul -> softmax -> matmul below (fp32 scores, probabilities never written out: DESIGN.md §8)
        o = ops.attention_mfma16(q.contiguous(), k.contiguous(), v.contiguous(), H, D, float(attn.scale))
        return _attn_out(attn, o, residual)
    qh = q.view(b, t, H, D).transpose(1, 2)
    kh = k.view(b, s, H, D).transpose(1, 2)
    vh = v.view(b, s, H, D).transpose(1, 2)
    scores = torch.matmul(qh, kh.transpose(-2, -1)) * attn.scale
    p = torch.softmax(scores, dim=-1)
    del scores
    if use_aq:
        p = p.float().contiguous()                                    # softmax quantisation in fp32 (sd.py:189)
        wq = attn.aqtizer_w
        skip = 1 if start_peak else 0
        if isinstance(wq, T2ILogQuantizer):
            if wq.real_time:
                delta = ops.max_f32(p, skip)
            else:
                if not wq.init:
                    wq.forward(p.clone(), skip)                       # quantile search on first use
                delta = wq.delta.detach().reshape(1).float().to(p.device)
            ops.logquant_f32(p, delta, wq.bits, skip)
        else:
            if not wq.init:
                wq.init_from(p[..., skip:] if skip else p)
            dd = wq.delta.detach().reshape(1).float().to(p.device)
            zz = torch.as_tensor(wq.zero_point).detach().reshape(1).float().to(p.device)
            if skip:
                pv = p.view(-1, s)
                # column bypass is not a row/token skip: quantise all, then restore column 0
                col0 = pv[:, 0].clone()
                ops.fakequant_rows(pv, 1, s, 0, dd, zz, 0, wq.bits)
                pv[:, 0] = col0
            else:
                ops.fakequant_rows(p.view(-1, s), 1, s, 0, dd, zz, 0, wq.bits)
        p = p.to(vh.dtype)
    o = torch.matmul(p, vh).transpose(1, 2).reshape(b, t, c)
    return _attn_out(attn, o, residual)


def _attn_out(attn, o, residual):
    """to_out[0] (+ residual in its GEMM epilogue), to_out[1] = Dropout(p=0)."""
    first = attn.to_out[0]
    if residual is not None and FUSION and _F_RES and isinstance(first, QuantLayer):
        o = first.forward_fused(o, residual=residual)
        residual = None
    else:
        o = first(o)
    for layer in list(attn.to_out)[1:]:
        o = layer(o)
    return o if residual is None else residual + o


def _init_static_softmax_delta(attn, wq, q, k, b, t, s, H, D, skip):
    """First-use initialisation of a static softmax quantizer (T2ILogQuantizer quantile search,
    quant_layer_text.py:49-76, or always_zero min/max): materialises the probabilities once, at load time only."""
    qh = q.view(b, t, H, D).transpose(1, 2)
    kh = k.view(b, s, H, D).transpose(1, 2)
    p = torch.softmax(torch.matmul(qh, kh.transpose(-2, -1)) * attn.scale, dim=-1).float()
    view = p[..., skip:] if skip else p
    if isinstance(wq, T2ILogQuantizer):
        d = wq._init_quantization_param(view.contiguous())
        wq.delta = nn.Parameter(d) if wq.leaf_param else d
        wq.init = True
    else:
        wq.init_from(view)


def b2qb() -> Dict[str, type]:
    return {"ResnetBlock2D": QuantResnetBlock2D, "BasicTransformerBlock": QuantBasicTransformerBlock}
