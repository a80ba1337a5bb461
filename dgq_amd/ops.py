"""Thin Python wrappers, one per C-ABI entry point of libdgq_hip.so, plus the per-layer objects
(`PackedWeight`, `ActBinding`) that own the device-resident tables.  No arithmetic happens in Python on the
hot path: a quantized layer call is `dgq_quant_act` + `dgq_gemm_wxa8`."""
import ctypes
import os
import threading
from typing import Optional

import torch
import torch.nn.functional as F

from . import _lib
from .plan import (ActLayout, natural_kperm, natural_ksrc, ksrc_index, ksrc_inverse, round_up, KTILE, act_offset, mark_clears,
                   flush_coefficients)

_c = ctypes


def _lib_call(name, *args):
    _lib.check(getattr(_lib.load(), name)(*args), name)


# ------------------------------------------------------------------------------------------ weights
def quantize_weight(w: torch.Tensor, delta: torch.Tensor, zp: torch.Tensor, alpha: Optional[torch.Tensor], bits: int):
    """Integer codes (uint8 [N][K_ref]) of wqtizer(w); K_ref = w.view(N,-1) order."""
    _lib.require_gpu()
    N = w.shape[0]
    w2 = w.detach().reshape(N, -1).contiguous().float()
    K = w2.shape[1]
    d = delta.detach().reshape(-1).contiguous().float()
    z = zp.detach().reshape(-1).contiguous().float()
    assert d.numel() == N and z.numel() == N, "weight quantizer must be per output channel"
    a = alpha.detach().reshape(N, -1).contiguous().float() if alpha is not None else None
    codes = torch.empty((N, K), dtype=torch.uint8, device=w.device)
    _lib_call("dgq_quantize_weight", _lib.ptr(w2), _lib.ptr(d), _lib.ptr(z), _lib.ptr(a), N, K, bits,
              _lib.ptr(codes), _lib.stream())
    return codes


class _AdaRoundSoft(torch.autograd.Function):
    """ŵ(α) of the AdaRound soft quantiser (adaptive_rounding.py:39-70, soft_tgt) — dgq_adaround_soft_fwd / _bwd.
    Only α receives a gradient: it is the only tensor the reconstruction optimiser owns (reconstruction.py:37-41)."""

    @staticmethod
    def forward(ctx, w2, d, z, alpha2, bits):
        N, K = w2.shape
        out = torch.empty_like(w2)
        _lib_call("dgq_adaround_soft_fwd", _lib.ptr(w2), _lib.ptr(d), _lib.ptr(z), _lib.ptr(alpha2), N, K, bits,
                  _lib.ptr(out), _lib.stream())
        ctx.save_for_backward(w2, d, z, alpha2)
        ctx.bits = bits
        return out

    @staticmethod
    def backward(ctx, gout):
        w2, d, z, alpha2 = ctx.saved_tensors
        N, K = w2.shape
        g = gout.contiguous().float()
        galpha = torch.empty_like(alpha2)
        _lib_call("dgq_adaround_soft_bwd", _lib.ptr(g), _lib.ptr(w2), _lib.ptr(d), _lib.ptr(z), _lib.ptr(alpha2), N, K,
                  ctx.bits, _lib.ptr(galpha), _lib.stream())
        return None, None, None, galpha, None


def adaround_soft(w: torch.Tensor, delta: torch.Tensor, zp: torch.Tensor, alpha: torch.Tensor, bits: int):
    """δ·(clamp(floor(w/δ) + h(α) + z, 0, 2^bits−1) − z) with h the rectified sigmoid; differentiable in α (fp32)."""
    _lib.require_gpu()
    N = w.shape[0]
    w2 = w.detach().reshape(N, -1).contiguous().float()
    d = delta.detach().reshape(-1).contiguous().float()
    z = torch.as_tensor(zp).detach().reshape(-1).float().to(w.device)
    z = (z.expand(N) if z.numel() == 1 else z).contiguous()
    assert d.numel() == N and z.numel() == N, "weight quantizer must be per output channel"
    a2 = alpha.reshape(N, -1)
    if a2.dtype != torch.float32 or not a2.is_contiguous():
        a2 = a2.float().contiguous()
    return _AdaRoundSoft.apply(w2, d, z, a2, bits).view(w.shape)


class _AdaRoundReg(torch.autograd.Function):
    """Σ (1 − |2h(α) − 1|^b) (reconstruction_util.py:68-70) — dgq_adaround_reg_fwd / _bwd."""

    @staticmethod
    def forward(ctx, alpha, b):
        a = alpha.contiguous()
        n = a.numel()
        part = torch.empty((_lib.load().dgq_adaround_reg_blocks(n),), dtype=torch.float32, device=a.device)
        _lib_call("dgq_adaround_reg_fwd", _lib.ptr(a), n, _c.c_float(b), _lib.ptr(part), _lib.stream())
        ctx.save_for_backward(a)
        ctx.b = b
        return part.sum()

    @staticmethod
    def backward(ctx, g):
        (a,) = ctx.saved_tensors
        gs = g.reshape(1).float().contiguous()
        galpha = torch.empty_like(a)
        _lib_call("dgq_adaround_reg_bwd", _lib.ptr(a), a.numel(), _c.c_float(ctx.b), _lib.ptr(gs), _lib.ptr(galpha),
                  _lib.stream())
        return galpha.view_as(a), None


def adaround_reg(alpha: torch.Tensor, b: float):
    """The rounding regulariser Σ (1 − |2h(α) − 1|^b) as a 0-d tensor, differentiable in α."""
    _lib.require_gpu()
    assert alpha.dtype == torch.float32
    return _AdaRoundReg.apply(alpha, float(b))


#: dgq_pack_w4 layout every kernel of this package reads (rows with bit 4 set: 8-byte halves of a 32-chunk exchanged)
W4_LAYOUT = 1


#: dgq_pack_w4 layout of the short-K kernel's weight image (gemm_panel.hip): fragment-major, N padded to 32-column tiles
W4_FRAG_LAYOUT = 2
#: keep a fragment-major copy of every W4 weight beside the row-major one, so that dgq_gemm_wxa8 may take its short-K kernel
#: (DGQ_GEMM_PANEL=0: never — the tile family alone, as in round 4)
GEMM_PANEL = True


def pack_weight(codes: torch.Tensor, kperm: Optional[torch.Tensor], Kp: int, bits: int, layout: int = W4_LAYOUT):
    N, K = codes.shape
    kp = kperm.to(codes.device, torch.int32).contiguous() if kperm is not None else None
    if bits == 4:
        rows = (N + 31) // 32 * 32 if layout == W4_FRAG_LAYOUT else N
        out = torch.empty((rows, Kp // 2), dtype=torch.uint8, device=codes.device)
        _lib_call("dgq_pack_w4", _lib.ptr(codes), N, K, _lib.ptr(kp), Kp, layout, _lib.ptr(out), _lib.stream())
    elif bits == 8:
        out = torch.empty((N, Kp), dtype=torch.int8, device=codes.device)
        _lib_call("dgq_pack_w8", _lib.ptr(codes), N, K, _lib.ptr(kp), Kp, _lib.ptr(out), _lib.stream())
    else:
        raise NotImplementedError("weight bits %d: the HIP path implements W4 and W8" % bits)
    return out


def unpack_w4(packed: torch.Tensor, Kp: int, layout: int = W4_LAYOUT):
    N = packed.shape[0]
    out = torch.empty((N, Kp), dtype=torch.uint8, device=packed.device)
    _lib_call("dgq_unpack_w4", _lib.ptr(packed), N, Kp, layout, _lib.ptr(out), _lib.stream())
    return out


class PackedWeight:
    """One quantized layer's weight, frozen to integer codes once (the reference re-derives them from fp32
    ``w`` on every call, quant_layer.py:642-643)."""

    def __init__(self, w, delta, zp, alpha, bias, bits, C, taps):
        self.bits, self.C, self.taps = bits, C, taps
        self.N = w.shape[0]
        self.K = C * taps
        dev = w.device
        self.codes = quantize_weight(w, delta, zp, alpha, bits)           # [N][K_ref] u8
        woff = 0.0 if bits == 4 else 128.0
        self.alpha = delta.detach().reshape(-1).float().contiguous().to(dev)
        self.zp_true = zp.detach().reshape(-1).float().contiguous().to(dev)
        self.zw = (self.zp_true - woff).contiguous()                       # zero point in the stored code domain
        self.bias = (bias.detach().float().contiguous().to(dev) if bias is not None
                     else torch.zeros(self.N, device=dev))
        self._natural = None
        self._natural_frag = None
        self._vn = None
        self._vc = None
        self._mfma16 = None
        self._mx6 = None
        self._mx6_ok = None

    @property
    def mx6_eligible(self):
        """True when dgq_gemm_mx6 may take this weight: W4, integer zero points and |q − z| <= 15 (the arithmetic of check_mfma16), so
        that every (q − z)/2 is an FP6 E2M3 value.  Computed once per packed weight."""
        if self._mx6_ok is None:
            self._mx6_ok = self.bits == 4 and self.check_mfma16(self.codes, self.zp_true, 4)
        return self._mx6_ok

    def mx6(self):
        """(image, Kp): the E2M3 codes of (q − z)/2 in the natural K order, [N][Kp/32][24] bytes (dgq_pack_w_mx6) — cached, one extra
        image per layer at 0.75 bytes per weight"""
        if self._mx6 is None:
            assert self.mx6_eligible, "PackedWeight.mx6: W4 with integer zero points and |q - z| <= 15"
            Kp = round_up(self.K, KTILE)
            img = torch.empty((self.N, Kp // 32, 24), dtype=torch.uint8, device=self.codes.device)
            _lib_call("dgq_pack_w_mx6", _lib.ptr(self.codes), _lib.ptr(self.zp_true), self.N, self.C, self.taps, Kp, _lib.ptr(img), _lib.stream())
            self._mx6 = (img, Kp)
        return self._mx6

    def mfma16_eligible(self):
        """True when dgq_conv2d_wq_mfma16 may take this weight: the zero points are integers and every q − z fits the bound (15 for
        W4, 255 for W8), so that q − z is exact in bf16 and f16 — MINMAX and AdaRound checkpoints (their z is a rounded value inside
        the code range).  Computed once per packed weight."""
        if self._mfma16 is None:
            self._mfma16 = self.check_mfma16(self.codes, self.zp_true, self.bits)
        return self._mfma16

    @staticmethod
    def check_mfma16(codes, zp, bits):
        """the rule of mfma16_eligible on codes [N][K] (u8) and zero points [N] (any device)"""
        z = zp.reshape(-1).float()
        lim = 15 if bits == 4 else 255
        if not (bool(torch.isfinite(z).all()) and bool((z == z.round()).all())):
            return False
        return bool(((codes.float() - z[:, None]).abs() <= lim).all())

    def natural_frag(self):
        """the natural-order weights fragment-major (dgq_pack_w4 layout 2), W4 only; None otherwise"""
        if self._natural_frag is None and self.bits == 4 and GEMM_PANEL:
            perm = natural_kperm(self.C, self.taps)
            self._natural_frag = pack_weight(self.codes, perm, perm.numel(), 4, W4_FRAG_LAYOUT)
        return self._natural_frag

    def natural(self):
        if self._natural is None:
            perm = natural_kperm(self.C, self.taps)
            self._natural = (pack_weight(self.codes, perm, perm.numel(), self.bits), perm.numel())
        return self._natural

    def centered(self):
        """(q − z) as float64 [N][K_ref] — load-time helper for the epilogue constants."""
        return self.codes.double() - self.zp_true.double()[:, None]

    def vn(self):
        if self._vn is None:
            self._vn = self.centered().sum(dim=1).float().contiguous()
        return self._vn

    def vc(self):
        """Vc[n][c] = Σ_{k∈c} (q − z) per 32-chunk c of the natural K order, fp32 [N][Kp/32] (integer-valued, 0 on the chunks of the
        K padding) — the load-time table of dgq_gemm_blockq"""
        if self._vc is None:
            perm = natural_kperm(self.C, self.taps).to(self.codes.device).long()
            cen = self.centered()
            nat = torch.where(perm >= 0, cen[:, perm.clamp(min=0)], torch.zeros((), dtype=cen.dtype, device=cen.device))
            self._vc = nat.view(self.N, -1, 32).sum(dim=2).float().contiguous()
        return self._vc


class ActBinding:
    """Device-resident tables of one (layer, timestep-slot) activation quantizer."""

    #: True on a DynamicActBinding whose row tables are not set yet (see there)
    dynamic = False
    #: True on a BlockActBinding (see there): the layer runs dgq_quant_act_block + dgq_gemm_blockq
    block = False
    #: True on a MxActBinding (a block binding; see there): the layer runs dgq_quant_act_mx6 + dgq_gemm_mx6
    mx = False

    def _table(self, key, make):
        if key not in self._koff:
            self._koff[key] = make()
        return self._koff[key]

    def koff(self, W, ldc):
        """ksrc resolved to element offsets (dh*W + dw)*ldc + c for one input geometry (cached)."""
        return None if self.ksrc is None else self._table(("off", W, ldc), lambda: ksrc_index(self.ksrc, W, ldc))

    def klds(self, kw, C):
        """ksrc resolved to indices (dh*kw + dw)*C + c into the [tap][C] strip a wave stages in LDS (cached)."""
        return None if self.ksrc is None else self._table(("lds", kw, C), lambda: ksrc_index(self.ksrc, kw, C))

    def kdst(self, kw, C, taps):
        """inverse of ksrc: packed position kp of element (tap, c), [taps*C] int32 (cached) — dgq_quant_act's scatter path"""
        return None if self.ksrc is None else self._table(("dst", kw, C, taps), lambda: ksrc_inverse(self.ksrc, kw, C, taps))

    def conv_patch_width(self, kh, kw, C, stride):
        """width in pixels of the input patch dgq_quant_act's block-staged path stages for this geometry (dgq_quant_act_conv_tile);
        0 where the geometry has no such path (cached)"""
        def ask():
            pw = _c.c_int(0)
            return pw.value if _lib.load().dgq_quant_act_conv_tile(C, kh, kw, stride, self.Kp, _c.byref(pw)) else 0
        return self._table(("patw", kh, kw, C, stride), ask)

    def kpat(self, kh, kw, C, pw):
        """(dh·pw + dw)·C + c of every packed position inside an input patch pw pixels wide, -1 for padding (cached): dgq_quant_act's
        block-staged path (pw from dgq_quant_act_conv_tile) and dgq_gemm_act_t.kpat of the conv form of quantise-on-load
        (csrc/gemm_convq.hip: 4 x 8 output positions per workgroup, pw = 8 + kw − 1).  Per-M / scalar layers: the natural order."""
        def make():
            e = self.ksrc if self.ksrc is not None else natural_ksrc(C, kh, kw, self.Kp).to(self.pw.codes.device)
            return ksrc_index(e, pw, C)
        return self._table(("pat", kh, kw, C, pw), make)

    def input_binding(self, C):
        """This (scalar) quantizer applied to the conv's INPUT tensor as a 1x1 layer in natural order: what dgq_quant_act needs to
        write the int8 NHWC code tensor of the implicit-im2col path (cached)."""
        hit = self._koff.get(("input", C))
        if hit is None:
            import copy
            hit = copy.copy(self)
            hit.Kp = round_up(C, KTILE)
            hit._koff = {}
            self._koff[("input", C)] = hit
        return hit

    def conv_zero_code(self):
        """centred int8 code of the value 0.0 under this scalar quantizer, z − offset (set at construction); None when z is not a
        code of the b-bit range (no implicit operand for such a layer)"""
        return self._zc

    def conv_fill(self):
        """32 bytes: 16 x the code of 0.0 (a tap outside the image), 16 x 0 (the K padding) — dgq_gemm_conv_t.fill"""
        return self._fill

    def __init__(self, layout: ActLayout, pw: PackedWeight, abits: int):
        dev = pw.codes.device
        self.mode, self.abits, self.offset = layout.mode, abits, act_offset(abits)
        self.pw = pw
        if layout.mode == "perK":
            self.Kp = layout.Kp
            self.ksrc = layout.ksrc.to(dev)
            self._koff = {}
            self.cdelta = layout.cdelta.to(dev)
            self.czp = layout.czp.to(dev)
            cfl = mark_clears(layout.cflush, abits, pw.bits)                     # + where the GEMM clears its running total
            self.cflush = cfl.to(dev)
            self.ccoef = flush_coefficients(layout.cdelta, cfl).to(dev)          # the same information as scalar-loadable coefficients
            self.wpacked = pack_weight(pw.codes, layout.kperm, layout.Kp, pw.bits)
            self.wfrag = pack_weight(pw.codes, layout.kperm, layout.Kp, 4, W4_FRAG_LAYOUT) if (pw.bits == 4 and GEMM_PANEL) else None
            U = (pw.centered() @ layout.kcoef.to(dev)).float()             # Σ_k δ_k(o − z_k)(qw − zw)
            self.gamma = (pw.bias + pw.alpha * U).contiguous()
            self.n_groups = layout.n_groups
        else:
            self.wpacked, self.Kp = pw.natural()
            self.wfrag = pw.natural_frag()
            self.ksrc = None
            self._koff = {}
            self.mdelta = layout.mdelta.to(dev).contiguous()
            self.mzp = layout.mzp.to(dev).contiguous()
            self.L = layout.L
            self.gamma = pw.bias
            self.vn = pw.vn()
            if layout.mode == "scalar":                    # implicit-im2col convolutions: the code of 0.0 and the DMA fill line
                # The reference's scalar-δ convolution is the native F.conv2d(aqtizer(x), ŵ, padding) (quant_layer.py:659): it pads with
                # exact 0.0 BEHIND the quantizer, i.e. with the code z.  That is a code of the b-bit range only while 0 <= z <= 2^b − 1
                # (always, for the min/max-derived scales of every DGQ recipe; a Scaler.MSE range of a one-signed input could leave it).
                # Outside it neither this path nor the materialised one can represent the padding value: no implicit operand then
                # (``conv_zero_code() is None``), the layer takes the materialising pass and its documented pad-then-quantise form.
                z = float(layout.mzp.reshape(-1)[0])
                if 0.0 <= round(z) <= 2.0 ** abits - 1.0:
                    self._zc = float(round(z) - self.offset)
                    self._fill = torch.tensor([int(self._zc)] * 16 + [0] * 16, dtype=torch.int8, device=dev)
                else:
                    self._zc, self._fill = None, None


class DynamicActBinding(ActBinding):
    """The binding of a real-time activation quantizer (UniformAffineQuantizer(real_time=True)): mode ``perM`` on the natural-order
    weight image — one copy per layer, no K permutation, no timestep slots — whose row tables do not exist until the layer sees its
    input.  quant_linear / quant_conv2d / quant_linear_multi / gemm_act ask dgq_act_row_params for one (δ, z) per row of THIS call's
    operand and continue with ``bound(mdelta, mzp)``: a shallow copy with L = M and those tables, which every per-M route then reads as
    mdelta[m % L] like a calibrated per-token table."""

    dynamic = True

    def __init__(self, pw: PackedWeight, abits: int):
        self.mode, self.abits, self.offset = "perM", abits, act_offset(abits)
        self.pw = pw
        self.wpacked, self.Kp = pw.natural()
        self.wfrag = pw.natural_frag()
        self.ksrc = None
        self._koff = {}
        self.mdelta = self.mzp = None
        self.L = 0
        self.gamma = pw.bias
        self.vn = pw.vn()

    def bound(self, mdelta: torch.Tensor, mzp: torch.Tensor):
        import copy
        ab = copy.copy(self)                                # shares the weight images and the (geometry-keyed) table cache
        ab.dynamic = False
        ab.mdelta, ab.mzp, ab.L = mdelta, mzp, mdelta.numel()
        return ab


class BlockActBinding(ActBinding):
    """The binding of a real-time BLOCK activation quantizer (UniformAffineQuantizer(real_time=True, real_time_block=32)): the
    natural-order weight image and Vc (PackedWeight.vc), no tables, no timestep slots, one binding per layer.  quant_linear /
    quant_conv2d / quant_linear_multi run such a layer as dgq_quant_act_block on its INPUT (once per row / pixel: codes, {δ, β} per
    32-channel block, ρ) + dgq_gemm_blockq (a convolution gathers the taps; the unfolded operand never exists)."""

    block = True

    def __init__(self, pw: PackedWeight, abits: int):
        assert pw.C % 32 == 0, "real-time block quantizer: C % 32 == 0"
        self.mode, self.abits, self.offset = "block", abits, act_offset(abits)
        self.pw = pw
        self.wpacked, self.Kp = pw.natural()
        self.wfrag = None
        self.ksrc = None
        self._koff = {}
        self.L = 0
        self.gamma = pw.bias
        self.vc = pw.vc()


class MxActBinding(BlockActBinding):
    """The binding of a real-time MXFP6 activation quantizer (UniformAffineQuantizer(real_time=True, real_time_block=32,
    real_time_format="mxfp6")) on a layer whose weight is exact in FP6 E2M3 (PackedWeight.mx6_eligible): the MX weight image, bias and δw —
    no tables, no timestep slots, one binding per layer.  The routes of a block binding run it as dgq_quant_act_mx6 on the layer INPUT
    (once per row / pixel: 24 code bytes and one E8M0 scale byte per 32-channel block) + dgq_gemm_mx6."""

    mx = True

    def __init__(self, pw: PackedWeight):
        assert pw.C % 32 == 0, "real-time MXFP6 quantizer: C % 32 == 0"
        self.mode, self.abits, self.offset = "block", 6, 0.0
        self.pw = pw
        self.wpacked, self.Kp = pw.mx6()
        self.wfrag = None
        self.ksrc = None
        self._koff = {}
        self.L = 0
        self.gamma = pw.bias


# ------------------------------------------------------------------------------------------ hot path
def act_ksplits(M, Kp):
    """K splits of the activation pre-pass: aim for >= 8192 waves (one per row x split) on low-M layers."""
    ks = max(1, min(16, 8192 // max(M, 1), Kp // 512))
    return _lib.load().dgq_quant_act_parts(Kp, ks)


FLOAT_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
def as_f32(t: torch.Tensor) -> torch.Tensor:
    """fp32 copy of a small parameter vector (norm γ/β ...) of a model that was cast with .half(): the kernels take
    their per-channel vectors in fp32.  The copy is cached ON the tensor object (pass the Parameter, not ``.data``) and
    refreshed when the tensor is modified in place or moved; nothing is keyed by address, so a later model that
    happens to reuse the same device memory can never see a stale vector."""
    if t.dtype == torch.float32:
        return t.detach()
    key = (t._version, t.data_ptr(), t.dtype)
    hit = t.__dict__.get("_dgq_f32")
    if hit is None or hit[0] != key:
        hit = (key, t.detach().float().contiguous())
        t.__dict__["_dgq_f32"] = hit
    return hit[1]


def groupnorm_scale_shift(x_cl: torch.Tensor, B, HW, C, groups, eps, gamma, beta):
    """GN(x) = x*scale + shift with scale/shift [B][C] (see dgq_groupnorm_scale_shift)."""
    dev = x_cl.device
    # enough (batch, group, slice) blocks to fill the chip; one block per (batch, group) — a single launch — only at 8x8
    # (measured: one block per group at 64x64 costs +1.1 ms per step)
    slices = max(1, min(32, (2048 + B * groups - 1) // (B * groups), HW // 64))
    scale = torch.empty((B, C), dtype=torch.float32, device=dev)
    shift = torch.empty((B, C), dtype=torch.float32, device=dev)
    part = torch.empty((B * groups * slices * 3,), dtype=torch.float32, device=dev)
    _lib_call("dgq_groupnorm_scale_shift", _lib.ptr(x_cl), _lib.DTYPE_CODE[x_cl.dtype], B, HW, C, groups,
              _c.c_float(eps), _lib.ptr(as_f32(gamma)), _lib.ptr(as_f32(beta)), _lib.ptr(scale), _lib.ptr(shift),
              _lib.ptr(part), slices, _lib.stream())
    return scale, shift


#: GroupNorm statistics out of the producing GEMM's epilogue (dgq_gemm_extra_t.gn_partial + dgq_groupnorm_from_partials) instead
#: of a pass over the tensor.  A conv output carries its partials as a tensor attribute (``_dgq_gn``); a GroupNorm folded
#: into the next layer's load uses them when the very same tensor object (or a channel concat of two such tensors,
#: ``cat_channels``) reaches it.  DGQ_GN_FROM_GEMM=0 restores the standalone statistics kernels.
GN_FROM_GEMM = True
#: ... also where the producing GEMM is K-split: its combine kernel writes the partials (=0: statistics pass for those tensors)
GN_FROM_SPLITK = True


#: convolutions whose activation quantizer is one (δ, z) pair (config C5 / C2U; the reference's native conv path) take the
#: implicit-im2col GEMM (dgq_gemm_conv_t): the input is quantised once per pixel and the unfolded operand never exists.
#: DGQ_CONV_IMPLICIT=0: the materialising pass of every other conv layer.
CONV_IMPLICIT = True


class OutputRedirect:
    """Where the NEXT "final" layer call of a module may put its output: ``out`` — an [M][N] row view it stores INTO (its result tensor is
    then a view of that memory), ``out2`` — one it stores into AS WELL.  The UNet sets it (``ops.set_redirect``) around the call of a module whose
    output is one half of an up-path concatenation (diffusers_rewrite/sd.py:558-613), both halves being row slices [:, :C1] / [:, C1:] of
    one [M][C1 + C2] buffer; a layer call made with ``final=True`` (the call whose result IS the module's result, residual included)
    takes it.  Nobody taking it is fine: the caller then finds its tensors elsewhere and concatenates as before."""

    def __init__(self, out=None, out2=None):
        self.out, self.out2, self.taken = out, out2, False


_REDIRECT_TLS = threading.local()                      # per thread: two threads running a model each never see the other's redirect


def set_redirect(rd):
    _REDIRECT_TLS.rd = rd


def pending_redirect():
    return getattr(_REDIRECT_TLS, "rd", None)


#: DGQ_CAT_INPLACE=0 (A/B runs): torch.cat for every skip concatenation
CAT_INPLACE = os.environ.get("DGQ_CAT_INPLACE", "1") != "0"


def take_redirect(M, N, dtype):
    """the pending OutputRedirect's (out, out2) if its views have this layer's output shape and dtype, else (None, None)"""
    rd = pending_redirect()
    if rd is None or rd.taken:
        return None, None
    for v in (rd.out, rd.out2):
        if v is not None and (tuple(v.shape) != (M, N) or v.dtype != dtype or v.stride(1) != 1):
            return None, None
    rd.taken = True
    return rd.out, rd.out2


def cat_channels(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """torch.cat([a, b], dim=1) of two NCHW tensors that keeps the GroupNorm partials of both sources (the skip concatenation in
    front of an up block's norm1): dgq_groupnorm_from_partials takes the two partial buffers as one channel range."""
    y = torch.cat([a, b], dim=1)
    ga, gb = _gn_of(a), _gn_of(b)
    if ga is not None and gb is not None and len(ga["parts"]) == 1 and len(gb["parts"]) == 1 and ga["B"] == gb["B"] and ga["HW"] == gb["HW"]:
        y._dgq_gn = dict(parts=ga["parts"] + gb["parts"], B=ga["B"], HW=ga["HW"], C=ga["C"] + gb["C"], ver=y._version)
    return y


def _gn_of(x: torch.Tensor):
    """The GroupNorm partials a producing GEMM attached to x — only while x is still the tensor it wrote: an in-place op in
    between (``x += ...``, a hook that mutates and returns its output) bumps ``_version`` and the statistics are stale."""
    gn = getattr(x, "_dgq_gn", None) if GN_FROM_GEMM else None
    return gn if (gn is not None and gn.get("ver") == x._version) else None


def groupnorm_from_partials(gn, groups, eps, gamma, beta):
    """scale / shift [B][C] of GN(x) from the partial statistics the producer(s) of x wrote (see dgq_groupnorm_from_partials)"""
    parts = gn["parts"]
    B, HW, C = gn["B"], gn["HW"], gn["C"]
    dev = parts[0][0].device
    scale = torch.empty((B, C), dtype=torch.float32, device=dev)
    shift = torch.empty((B, C), dtype=torch.float32, device=dev)
    p2, c2 = (parts[1][0], parts[1][1]) if len(parts) > 1 else (None, 0)
    _lib_call("dgq_groupnorm_from_partials", _lib.ptr(parts[0][0]), parts[0][1], _lib.ptr(p2), c2, B, HW, groups, _c.c_float(eps),
              _lib.ptr(as_f32(gamma)), _lib.ptr(as_f32(beta)), _lib.ptr(scale), _lib.ptr(shift), _lib.stream())
    return scale, shift


def _quant_input(x, geom, bits, pre=None, ln=None, ups=False):
    """(dgq_quant_act_args_t, the tensors it points to) with the INPUT description of the layer input x (channels-last storage) of
    geometry geom = (B, H, W, C, kh, kw, stride, pad) set — x, dtype, geometry, bits, the folded prologue — and nothing else: what
    dgq_act_row_params reads, and what _quant_args completes with a binding's tables.  pre / ln / ups as in quant_act."""
    B, H, W, C, kh, kw, stride, pad = geom
    a = _lib.QuantActArgs()
    a.x, a.x_dtype, a.B, a.H, a.W, a.C, a.kh, a.kw, a.stride, a.pad = x.data_ptr(), _lib.DTYPE_CODE[x.dtype], B, H, W, C, kh, kw, stride, pad
    a.bits = bits
    keep = [x]
    if pre and pre[0] is not None:
        a.pre_scale, a.pre_shift = pre[0].data_ptr(), pre[1].data_ptr()
        keep += [pre[0], pre[1]]
    a.pre_act = pre[2] if pre else 0
    if ln:
        g, b = as_f32(ln[0]), as_f32(ln[1])
        a.ln_gamma, a.ln_beta, a.ln_eps = g.data_ptr(), b.data_ptr(), float(ln[2])
        keep += [g, b]
    a.ups = 1 if ups else 0
    return a, keep


def _quant_args(x, geom, ab: ActBinding, pre=None, ln=None, ups=False):
    """(dgq_quant_act_args_t, the tensors it points to) for the layer input x (channels-last storage) of geometry geom = (B, H, W, C,
    kh, kw, stride, pad) under ab's tables — with one K split and placeholder outputs: the caller settles the split (quant_splits),
    allocates and sets ``codes`` / ``rowsum``.  pre / ln / ups as in quant_act."""
    B, H, W, C, kh, kw, stride, pad = geom
    per_m = 0 if ab.mode == "perK" else 1
    ldc = 2 * C if (pre and pre[2] == 2) else C
    a, keep = _quant_input(x, geom, ab.abits, pre, ln, ups)
    a.ksrc, a.koff, a.klds, a.kdst = _dp(ab.ksrc), _dp(ab.koff(W, ldc)), _dp(ab.klds(kw, C)), _dp(ab.kdst(kw, C, kh * kw))
    if kh * kw > 1 and C % 4 == 0:                           # the block-staged conv path, where the geometry has one
        pw = ab.conv_patch_width(kh, kw, C, stride)
        a.kpat = _dp(ab.kpat(kh, kw, C, pw)) if pw else None
    a.Kp, a.per_m = ab.Kp, per_m
    a.delta, a.zp = (ab.cdelta.data_ptr(), ab.czp.data_ptr()) if not per_m else (ab.mdelta.data_ptr(), ab.mzp.data_ptr())
    a.L = 1 if not per_m else ab.L
    a.ksplits = 1
    a.codes = a.rowsum = 1                                   # placeholders: dgq_quant_act_variant only validates non-NULL
    return a, keep


def act_row_params_multi(problems):
    """dgq_act_row_params_batch: the real-time row tables of up to 4 inputs of one dtype in shared launches.  problems: dicts / tuples
    (x, geom, bits, pre, ln, ups, fold_T) — x the channels-last storage and geom = (B, H, W, C, kh, kw, stride, pad) as for quant_act,
    fold_T > 0 folds the rows r with equal r % fold_T (Linear inputs).  Returns [(δ, z)] fp32 device tensors, [M] or [fold_T] each.
    At most two launches, no synchronisation: capture-safe (the scratch comes from torch's allocator like every other temporary)."""
    n = len(problems)
    ins = (_lib.QuantActArgs * n)()
    outs = (_lib.RowParamsOut * n)()
    keep, res = [], []
    for i, (x, geom, bits, pre, ln, ups, fold_T) in enumerate(problems):
        B, H, W, C, kh, kw, stride, pad = geom
        a, k = _quant_input(x, geom, bits, pre, ln, ups)
        ins[i] = a
        M = B * ((H + 2 * pad - kh) // stride + 1) * ((W + 2 * pad - kw) // stride + 1)
        entries = fold_T if fold_T else M
        d = torch.empty((entries,), dtype=torch.float32, device=x.device)
        z = torch.empty((entries,), dtype=torch.float32, device=x.device)
        o = outs[i]
        o.fold_T, o.delta, o.zp = fold_T, d.data_ptr(), z.data_ptr()
        if fold_T or (kh, kw, stride, pad) != (1, 1, 1, 0):
            ws = torch.empty((2 * B * (H >> (1 if ups else 0)) * (W >> (1 if ups else 0)),), dtype=torch.float32, device=x.device)
            o.ws, o.ws_floats = ws.data_ptr(), ws.numel()
            k.append(ws)
        keep += k
        res.append((d, z))

    def issue(_keep=keep):
        _lib_call("dgq_act_row_params_batch", n, _c.cast(ins, _c.c_void_p), _c.cast(outs, _c.c_void_p), _lib.stream())
    issue()
    if ROWPARAMS_LAUNCH_HOOK is not None:
        ROWPARAMS_LAUNCH_HOOK(issue, problems)
    return res


def act_row_params(x, geom, bits, pre=None, ln=None, ups=False, fold_T=0):
    """(δ, z) of the real-time activation quantizer for every row of one layer input — see act_row_params_multi"""
    return act_row_params_multi([(x, geom, bits, pre, ln, ups, fold_T)])[0]


def _bind_rows(ab: ActBinding, x, geom, pre=None, ln=None, ups=False):
    """ab itself, or — a DynamicActBinding — ab bound to the row tables of this call's operand"""
    if not ab.dynamic:
        return ab
    return ab.bound(*act_row_params(x, geom, ab.abits, pre, ln, ups))


def quant_splits(a, M):
    """Settles ``a.ksplits`` of a quantiser problem of M rows and returns it.  The LDS-scatter and block-staged variants (3 / 4 / 5:
    per-K convs, per-K Linear inputs with short groups, convs whose input patch fits the LDS) take the whole row in one wave / block:
    they are asked for with one K split first; every other problem is split by act_ksplits.  None where ``a.ups`` is set and the
    problem takes none of those variants (the folded upsample exists on the scatter / block-staged paths only).  One accepted set
    serves convolutions and Linear inputs alike: quant_act_variant (csrc/quant_act.hip) answers 5 only with ``kpat`` and more than
    one tap, and a Linear struct has neither."""
    a.ksplits = 1
    if (a.kdst is None and a.kpat is None) or _lib.load().dgq_quant_act_variant(_c.byref(a)) not in (3, 4, 5):
        if a.ups:
            return None
        a.ksplits = act_ksplits(M, a.Kp)
    return a.ksplits


def quant_act(x_cl: torch.Tensor, B, H, W, C, kh, kw, stride, pad, ab: ActBinding, pre=None, ln=None, ups=False):
    """x_cl: contiguous channels-last storage [B][H][W][C] (any fp dtype). Returns (codes, rowsum[parts][M], M).
    pre = (scale [B][C], shift [B][C], act) folds a GroupNorm (+SiLU when act == 1) into the load;
    ln = (gamma [C], beta [C], eps) folds a LayerNorm over each row's C elements (Linear inputs).
    ups: x_cl holds [B][H/2][W/2][C] and is read through a 2x nearest upsample (Upsample2D's interpolate folded into the load);
    returns None when the layer's quantise variant has no such form."""
    Ho = (H + 2 * pad - kh) // stride + 1
    Wo = (W + 2 * pad - kw) // stride + 1
    M = B * Ho * Wo
    a, keep = _quant_args(x_cl, (B, H, W, C, kh, kw, stride, pad), ab, pre, ln, ups)
    parts = quant_splits(a, M)
    if parts is None:
        return None
    codes = torch.empty((M, ab.Kp), dtype=torch.int8, device=x_cl.device)
    rowsum = torch.empty((parts, M), dtype=torch.float32, device=x_cl.device)
    a.codes, a.rowsum = codes.data_ptr(), rowsum.data_ptr()

    def issue(_keep=keep):
        _lib_call("dgq_quant_act_batch", 1, _c.byref(a), _lib.stream())
    issue()
    if QUANT_LAUNCH_HOOK is not None:
        ldc = 2 * C if a.pre_act == 2 else C
        QUANT_LAUNCH_HOOK(issue, B * H * W * ldc * x_cl.element_size() >> (2 if ups else 0), M * ab.Kp + 4 * parts * M)
    return codes, rowsum, M


def _dp(t):
    return t.data_ptr() if t is not None else None


_WORKSPACE = {}
WORKSPACE_BYTES = 128 << 20
#: slabs kept for user streams (other than the default / capture stream): least recently
#: used first out, so a program that keeps creating streams does not leak 128 MB per handle
_STREAM_SLABS_MAX = 4


def workspace(device):
    """Persistent split-K scratch (caller-owned; one per device AND stream, so that layers running concurrently on
    different streams never share it): the library never allocates."""
    cur = torch.cuda.current_stream(device).cuda_stream
    # the default stream and torch's graph-capture stream of a device are one serial chain (a capture runs while the
    # default stream is idle) and share the "main" slab; any OTHER user stream gets a slab of its own, keyed by handle,
    # so two user streams can never race on one split-K workspace
    is_main = cur == torch.cuda.default_stream(device).cuda_stream or torch.cuda.is_current_stream_capturing()
    branch = "main" if is_main else ("stream", cur)
    key = (str(device), branch)
    if key not in _WORKSPACE:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("dgq_amd: the split-K workspace must exist before graph capture (run the model once eagerly)")
        if isinstance(branch, tuple):                       # a user stream: bounded, least recently used first out
            old = [k for k in _WORKSPACE if k[0] == str(device) and isinstance(k[1], tuple)]
            while len(old) >= _STREAM_SLABS_MAX:
                _WORKSPACE.pop(old.pop(0))
        _WORKSPACE[key] = torch.empty(WORKSPACE_BYTES, dtype=torch.uint8, device=device)
    elif isinstance(branch, tuple):
        _WORKSPACE[key] = _WORKSPACE.pop(key)               # most recently used last
    return _WORKSPACE[key]


def make_extra(residual=None, fq=None, res_div=1, geglu=False, gn_partial=None, conv=None, y2=None):
    """dgq_gemm_extra_t: residual [M / res_div][N] fp32 (row stride = its stride(0); res_div > 1 broadcasts each row
    over res_div consecutive output rows); fq = (mode, delta, zp, T, D, skip, bits) with mode 1 scalar / 2 per token /
    3 per head-dim; geglu = the pair epilogue of a row-interleaved ff.net.0.  Keeps the tensors alive on the returned object."""
    if residual is None and fq is None and not geglu and gn_partial is None and conv is None and y2 is None:
        return None
    ex = _lib.GemmExtra()
    ex.res_div = 1
    if y2 is not None:                                      # a second copy of the output rows ([M][N] view, its own row pitch)
        assert y2.dim() == 2 and y2.stride(1) == 1
        ex.y2, ex.ldy2 = y2.data_ptr(), y2.stride(0)
        ex._y2_keep = y2
    ex.conv = None
    ex.flush_coef = None
    if conv is not None:                                    # (dgq_gemm_conv_t, tensors it points to)
        ex.conv = _c.cast(_c.pointer(conv[0]), _c.c_void_p)
        ex._conv_keep = conv
    ex.geglu = 1 if geglu else 0
    ex.gn_partial = gn_partial.data_ptr() if gn_partial is not None else None
    keep = []
    if residual is not None:
        assert residual.dtype in _lib.DTYPE_CODE and residual.stride(-1) == 1
        ex.residual, ex.ldr, ex.res_div = residual.data_ptr(), residual.stride(0), res_div
        ex.res_dtype = _lib.DTYPE_CODE[residual.dtype]
        keep.append(residual)
    if gn_partial is not None:
        keep.append(gn_partial)
    if fq is not None:
        mode, delta, zp, T, D, skip, bits = fq
        ex.fq_mode, ex.fq_delta, ex.fq_zp = mode, delta.data_ptr(), zp.data_ptr()
        ex.fq_T, ex.fq_D, ex.fq_skip, ex.fq_qmax = T, D, skip, float(2 ** bits - 1)
        keep += [delta, zp]
    else:
        ex.fq_T = ex.fq_D = 1
    ex._keep = keep
    return ex


#: measurement hooks (bench.py's roofline leg), None in production.  QUANT_LAUNCH_HOOK(issue, algorithmic_bytes, overhead_bytes): every
#: dgq_quant_act_batch launch — algorithmic = the layer input read once, un-unfolded; overhead = the int8 code matrix
#: and the row sums it writes, which the algorithm does not need; ATTN_LAUNCH_HOOK(issue, flops, bytes): every dgq_attention call (its two or three kernels).
QUANT_LAUNCH_HOOK = None
ATTN_LAUNCH_HOOK = None
#: ROWPARAMS_LAUNCH_HOOK(issue, problems): every dgq_act_row_params_batch call (the real-time row tables; problems as act_row_params_multi takes them)
ROWPARAMS_LAUNCH_HOOK = None
#: when set, every GEMM launch of the dgq_gemm_wxa8 family is issued through
#: ``GEMM_LAUNCH_HOOK(issue, problems)`` — ``issue()`` launches it (again) on the current stream, ``problems`` lists the
#: (M, ActBinding, out_element_size, input_bytes) of the layers the launch computes — input_bytes > 0 where the launch quantises its own
#: operand (the fp input it reads), 0 where it reads a code matrix a dgq_quant_act launch wrote.  None in production.
GEMM_LAUNCH_HOOK = None


def with_layer_tables(extra, ab: "ActBinding", M):
    """extra (or a blank one) carrying the layer's optional operand images: the flush-coefficient table for the shapes the 256-row
    kernel may take, the fragment-major weights for the short-K kernel"""
    need_coef = ab.mode == "perK" and M >= 2048 and ab.pw.N >= 128
    wfrag = getattr(ab, "wfrag", None)
    if not need_coef and wfrag is None:
        return extra
    if extra is None:
        extra = _lib.GemmExtra()
        extra.res_div, extra.fq_T, extra.fq_D, extra._keep = 1, 1, 1, []
    if need_coef:
        extra.flush_coef = ab.ccoef.data_ptr()
    if wfrag is not None:
        extra.wfrag = wfrag.data_ptr()
    return extra


#: Linear / 1x1 layers whose whole padded K fits the short-K kernel's LDS panel run as ONE launch: the GEMM quantises its own rows
#: (dgq_gemm_act_t) instead of reading the codes a dgq_quant_act launch wrote.  DGQ_GEMM_FUSE=0: the two-launch form everywhere.
GEMM_FUSE = True
#: ... also for the 3x3 convolutions whose input patch fits the LDS (csrc/gemm_convq.hip); False: quantise launch + GEMM launch
CONV_FUSE = os.environ.get("DGQ_CONV_FUSE", "1") != "0"         # (this round's A/B switch: DGQ_CONV_FUSE=0)


def _act_operand_ok(x2):
    """what dgq_gemm_wxa8 requires of a quantise-on-load operand (fill_gemm): 16-byte aligned base, row pitch a multiple of 8 bytes"""
    return x2 is None or (x2.data_ptr() % 16 == 0 and (x2.stride(0) * x2.element_size()) % 8 == 0 and x2.stride(-1) == 1)


def act_fuses(ab: "ActBinding", M, K, dtype, n_problems=1, x2=None, N=None, Kp=None):
    """True where quant_linear / quant_conv2d (1x1) may hand the layer to dgq_gemm_wxa8 with quantise-on-load.  x2: the [M][K] operand
    view the launch would read — a view the kernel cannot address (an unaligned slice) keeps the layer on the two-launch form instead
    of failing the call.  N / Kp: what the library plans a shared launch with (problem 0's N, the widest Kp of the launch)."""
    if not (GEMM_FUSE and GEMM_PANEL) or getattr(ab, "wfrag", None) is None or ab.pw.taps != 1 or K % 4 != 0 or dtype not in _lib.DTYPE_CODE:
        return False
    if not _act_operand_ok(x2):
        return False
    dt = _lib.DTYPE_CODE[dtype]
    return bool(_lib.load().dgq_gemm_act_fuses(M, ab.pw.N if N is None else N, K, ab.Kp if Kp is None else Kp, ab.pw.bits,
                                               0 if ab.mode == "perK" else 1, n_problems, dt, dt))


def _multi_fuses(bindings, M, Kin, dtype, x2):
    """quant_linear_multi: every shared quantise-on-load launch of _gemm_batches (one per scale mode and 8 layers) must take quantise-on-load
    with the shape the library plans it by — problem 0's N and the launch's widest Kp (dgq_gemm_wxa8_batch)"""
    groups = {}
    for i, ab in enumerate(bindings):
        if ab.pw.K != Kin:
            return False
        groups.setdefault(0 if ab.mode == "perK" else 1, []).append(ab)
    for abs_ in groups.values():
        for j0 in range(0, len(abs_), 8):
            chunk = abs_[j0:j0 + 8]
            kp = max(ab.Kp for ab in chunk)
            if not all(act_fuses(ab, M, Kin, dtype, len(chunk), x2, N=chunk[0].pw.N, Kp=kp) for ab in chunk):
                return False
    return True


def conv_act_fuses(ab: "ActBinding", B, H, W, C, kh, kw, stride, pad, dtype, x_store=None):
    """True where quant_conv2d may hand a k x k convolution to dgq_gemm_wxa8 with its activation quantiser inside the launch
    (csrc/gemm_convq.hip: no int8 code matrix in HBM)."""
    if not (GEMM_FUSE and CONV_FUSE) or getattr(ab, "wfrag", None) is None or ab.mode == "scalar" or dtype not in _lib.DTYPE_CODE:
        return False
    if x_store is not None and not (x_store.is_contiguous() and x_store.data_ptr() % 16 == 0 and (C * x_store.element_size()) % 8 == 0):
        return False
    dt = _lib.DTYPE_CODE[dtype]
    return bool(_lib.load().dgq_gemm_conv_act_fuses(B, H, W, C, kh, kw, stride, pad, ab.pw.N, ab.Kp, ab.pw.bits,
                                                    0 if ab.mode == "perK" else 1, dt, dt))


def make_act(x2: torch.Tensor, ab: "ActBinding", pre=None, ln=None, rows_per_image=1, conv=None):
    """dgq_gemm_act_t for the rows x2 [M][K] (row stride = stride(0)) under the layer's activation quantizer; pre = (scale, shift,
    act) a folded GroupNorm (+ SiLU), ln = (gamma, beta, eps) a folded LayerNorm.  conv = (B, H, W, C, kh, kw, stride, pad): the conv
    form (csrc/gemm_convq.hip) — x2 is the contiguous [B][H][W][C] storage and the launch stages input patches of it.  Keeps its
    tensors alive on the struct."""
    a = _lib.GemmAct()
    a.x, a.x_dtype = x2.data_ptr(), _lib.DTYPE_CODE[x2.dtype]
    keep = [x2]
    if conv is None:
        a.ldx, a.K = x2.stride(0), ab.pw.K
        if ab.mode == "perK":
            kd = ab.kdst(1, ab.pw.K, 1)
            a.kdst = kd.data_ptr()
            keep.append(kd)
    else:
        B, H, W, C, kh, kw, stride, pad = conv
        kp = ab.kpat(kh, kw, C, 8 + kw - 1)
        a.ldx = a.K = C
        a.kpat = kp.data_ptr()
        a.B, a.H, a.W, a.kh, a.kw, a.stride, a.pad = B, H, W, kh, kw, stride, pad
        keep.append(kp)
    if ab.mode == "perK":
        a.czp = ab.czp.data_ptr()
    a.bits = ab.abits
    a.rows_per_image, a.pre_act = rows_per_image, 0
    if pre is not None:
        if pre[0] is not None:
            a.pre_scale, a.pre_shift = pre[0].data_ptr(), pre[1].data_ptr()
            keep += [pre[0], pre[1]]
        a.pre_act = pre[2]
    if ln is not None:
        g, b = as_f32(ln[0]), as_f32(ln[1])
        a.ln_gamma, a.ln_beta, a.ln_eps = g.data_ptr(), b.data_ptr(), float(ln[2])
        keep += [g, b]
    a._keep = keep
    return a


def _with_act(extra, ab: "ActBinding", M, act):
    """extra (see with_layer_tables) carrying the quantise-on-load descriptor ``act``"""
    extra = with_layer_tables(extra, ab, M)
    extra.act = _c.cast(_c.pointer(act), _c.c_void_p)
    extra._act_keep = act
    return extra


def gemm_act(x2, M, ab: "ActBinding", out_dtype, extra=None, pre=None, ln=None, rows_per_image=1, out=None):
    """one launch: aqtizer(x2) @ Wᵀ with the layer's epilogue — dgq_gemm_wxa8 with quantise-on-load (see act_fuses)"""
    if ab.dynamic:                                       # (a caller that did not bind the row tables itself)
        assert x2.is_contiguous()
        ab = _bind_rows(ab, x2, (M // rows_per_image, rows_per_image, 1, ab.pw.K, 1, 1, 1, 0), pre, ln)
    extra = _with_act(extra, ab, M, make_act(x2, ab, pre, ln, rows_per_image))
    return gemm_wxa8(None, None, M, ab, out_dtype, out=out, extra=extra, _fused_bytes=x2.element_size() * M * ab.pw.K)


def _gemm_args(ab: ActBinding, M, codes, rowsum, parts, out, extra):
    """dgq_gemm_args_t of one layer: codes [M][Kp] and rowsum [parts][M] as a dgq_quant_act launch wrote them — or None for both
    where extra.act makes the launch quantise its own operand: both are ignored then and only have to be device pointers, with
    one row-sum part.  The scale tables follow the layer's mode: cdelta / cflush per-K, mdelta / mzp / vn and L per-M and scalar."""
    pw = ab.pw
    per_m = 0 if ab.mode == "perK" else 1
    g = _lib.GemmArgs()
    if codes is None:
        g.codes = g.rowsum = ab.wfrag.data_ptr()
        g.rowsum_parts = 1
    else:
        g.codes, g.rowsum, g.rowsum_parts = codes.data_ptr(), rowsum.data_ptr(), parts
    g.M, g.Kp, g.wpacked, g.w_bits, g.N, g.per_m = M, ab.Kp, ab.wpacked.data_ptr(), pw.bits, pw.N, per_m
    if per_m:
        g.mdelta, g.mzp, g.L, g.vn = ab.mdelta.data_ptr(), ab.mzp.data_ptr(), ab.L, ab.vn.data_ptr()
    else:
        g.cdelta, g.cflush, g.L = ab.cdelta.data_ptr(), ab.cflush.data_ptr(), 1
    g.offset = ab.offset
    g.alpha, g.zw, g.gamma = pw.alpha.data_ptr(), pw.zw.data_ptr(), ab.gamma.data_ptr()
    g.y, g.y_dtype, g.ldy = out.data_ptr(), _lib.DTYPE_CODE[out.dtype], out.stride(0)
    if extra is not None:
        g.extra = _c.cast(_c.pointer(extra), _c.c_void_p)
        g._extra_keep = extra
    return g


def gemm_wxa8(codes, rowsum, M, ab: ActBinding, out_dtype, out: Optional[torch.Tensor] = None, extra=None, _fused_bytes=0):
    """One dgq_gemm_wxa8 launch (split-K, the implicit-conv tiles and the conv-quantiser kernel are this entry's alone).  codes =
    rowsum = None where extra.act makes the launch quantise its own operand.  _fused_bytes: the fp input such a launch reads, for
    GEMM_LAUNCH_HOOK only."""
    assert codes is not None or (extra is not None and extra.act), "dgq gemm_wxa8: no code matrix and no quantise-on-load descriptor"
    dev = ab.wpacked.device
    ws = workspace(dev)
    extra = with_layer_tables(extra, ab, M)
    if out is None:
        out = torch.empty((M, ab.pw.N // 2 if (extra is not None and extra.geglu) else ab.pw.N), dtype=out_dtype, device=dev)
    g = _gemm_args(ab, M, codes, rowsum, rowsum.shape[0] if (rowsum is not None and rowsum.dim() == 2) else 1, out, None)
    head = [getattr(g, name) for name, _ in _lib.GemmArgs._fields_[:22]]      # (the entry's first 22 parameters, in its order)

    def issue(_keep=(codes, rowsum, out, g, ab)):
        _lib_call("dgq_gemm_wxa8", *head, _lib.ptr(ws), ws.numel(), _c.byref(extra) if extra is not None else None, _lib.stream())
    issue()
    if GEMM_LAUNCH_HOOK is not None:
        GEMM_LAUNCH_HOOK(issue, [(M, ab, out.element_size(), _fused_bytes)])
    return out


#: BLOCK_LAUNCH_HOOK(issue, kind, info): every launch of the real-time block mode — kind "quant" (dgq_quant_act_block; info = rows, C)
#: or "gemm" (dgq_gemm_blockq; info = M, N, K).  A measurement hook (tools/profile_realtime_act.py), None in production.
BLOCK_LAUNCH_HOOK = None


def _block_quant_launch(entry, x_cl, geom, bits, pre, ln, ups, pitch, outputs):
    """One launch of a block quantiser entry on the layer INPUT x_cl: rows = the input's rows / pixels (the SOURCE pixels with ``ups``),
    pitch = per-block entries of a row (default C/32).  outputs(rows, C, pitch, device) -> (the entry's output struct, its tensors);
    returns the tensors."""
    B, H, W, C = geom[:4]
    sh = 1 if ups else 0
    rows = B * (H >> sh) * (W >> sh)
    a, keep = _quant_input(x_cl, geom, bits, pre, ln, ups)
    o, res = outputs(rows, C, C // 32 if pitch is None else pitch, x_cl.device)

    def issue(_keep=(keep, res)):
        _lib_call(entry, _c.byref(a), _c.byref(o), _lib.stream())
    issue()
    if BLOCK_LAUNCH_HOOK is not None:
        BLOCK_LAUNCH_HOOK(issue, "quant", (rows, C))
    return res


def _block_gemm_launch(entry, k, q, geom, ab, out_dtype, out, extra, ups, **own):
    """One launch of a block GEMM entry on q = its quantiser's result (q[0]: the codes): the dgq_gemm_args_t of a block-mode layer —
    ``own``: the fields the format adds — and the geometry of k, the format's struct carrying its own fields.  Returns y."""
    B, H, W, C, kh, kw, stride, pad = geom
    M = B * ((H + 2 * pad - kh) // stride + 1) * ((W + 2 * pad - kw) // stride + 1)
    pw = ab.pw
    if out is None:
        out = torch.empty((M, pw.N // 2 if (extra is not None and extra.geglu) else pw.N), dtype=out_dtype, device=q[0].device)
    g = _lib.GemmArgs()
    g.codes, g.rowsum_parts = q[0].data_ptr(), 1
    g.M, g.Kp, g.wpacked, g.N, g.per_m, g.L = M, ab.Kp, ab.wpacked.data_ptr(), pw.N, 0, 1
    g.alpha, g.gamma = pw.alpha.data_ptr(), ab.gamma.data_ptr()
    g.y, g.y_dtype, g.ldy = out.data_ptr(), _lib.DTYPE_CODE[out.dtype], out.stride(0)
    for name, value in own.items():
        setattr(g, name, value)
    if extra is not None:
        g.extra = _c.cast(_c.pointer(extra), _c.c_void_p)
    k.B, k.H, k.W, k.C, k.kh, k.kw, k.stride, k.pad, k.ups = B, H, W, C, kh, kw, stride, pad, 1 if ups else 0

    def issue(_keep=(q, out, extra, ab)):
        _lib_call(entry, _c.byref(g), _c.byref(k), _lib.stream())
    issue()
    if BLOCK_LAUNCH_HOOK is not None:
        BLOCK_LAUNCH_HOOK(issue, "gemm", (M, pw.N, pw.K))
    return out


def quant_act_block(x_cl: torch.Tensor, geom, bits, pre=None, ln=None, ups=False, ldt=None):
    """dgq_quant_act_block on the layer INPUT x_cl (channels-last storage, geom = (B, H, W, C, kh, kw, stride, pad) as for quant_act):
    one launch.  Returns (codes int8 [rows][C], table fp32 [rows][ldt][2] = {δ, β} per 32-channel block, ρ fp32 [rows]) with rows =
    the input's rows / pixels (the SOURCE pixels with ``ups``); ldt (default C/32) > C/32 adds zeroed entries (a Linear layer's K
    padding).  pre / ln / ups as in quant_act."""
    def outputs(rows, C, ldt, dev):
        codes = torch.empty((rows, C), dtype=torch.int8, device=dev)
        table = torch.empty((rows, ldt, 2), dtype=torch.float32, device=dev)
        rho = torch.empty((rows,), dtype=torch.float32, device=dev)
        o = _lib.ActBlockOut()
        o.codes, o.table, o.ldt, o.rho = codes.data_ptr(), table.data_ptr(), ldt, rho.data_ptr()
        return o, (codes, table, rho)
    return _block_quant_launch("dgq_quant_act_block", x_cl, geom, bits, pre, ln, ups, ldt, outputs)


def dequant_act_block(codes, table, out):
    """out [rows][C] = δ·(q − z) from quant_act_block's codes and table (dgq_dequant_act_block)"""
    rows, C = codes.shape
    _lib_call("dgq_dequant_act_block", _lib.ptr(codes), _lib.ptr(table), table.shape[1], rows, C, _lib.ptr(out), _lib.DTYPE_CODE[out.dtype],
              _lib.stream())
    return out


def gemm_blockq(q, geom, ab: "BlockActBinding", out_dtype, out=None, extra=None, ups=False):
    """One dgq_gemm_blockq launch on q = quant_act_block(...) of the layer input; geom = (B, H, W, C, kh, kw, stride, pad) of the layer
    (H, W: behind a folded upsample).  Returns y [M][N] (N/2 columns with the GEGLU epilogue)."""
    _, table, rho = q
    k = _lib.GemmBlock()
    k.table, k.ldt, k.vc = table.data_ptr(), table.shape[1], ab.vc.data_ptr()
    return _block_gemm_launch("dgq_gemm_blockq", k, q, geom, ab, out_dtype, out, extra, ups, w_bits=ab.pw.bits, rowsum=rho.data_ptr(),
                              offset=ab.offset, zw=ab.pw.zw.data_ptr())


def quant_act_mx6(x_cl: torch.Tensor, geom, pre=None, ln=None, ups=False, lds=None):
    """dgq_quant_act_mx6 on the layer INPUT x_cl (channels-last storage, geom as for quant_act_block): one launch.  Returns (codes uint8
    [rows][C/32][24], scale uint8 [rows][lds] = E + 127 per 32-channel block) with rows = the input's rows / pixels (the SOURCE pixels
    with ``ups``); lds (default C/32) > C/32 adds entries of 127 (a Linear layer's K padding).  pre / ln / ups as in quant_act."""
    def outputs(rows, C, lds, dev):
        codes = torch.empty((rows, C // 32, 24), dtype=torch.uint8, device=dev)
        scale = torch.empty((rows, lds), dtype=torch.uint8, device=dev)
        o = _lib.ActMx6Out()
        o.codes, o.scale, o.lds = codes.data_ptr(), scale.data_ptr(), lds
        return o, (codes, scale)
    return _block_quant_launch("dgq_quant_act_mx6", x_cl, geom, 6, pre, ln, ups, lds, outputs)


def dequant_act_mx6(codes, scale, out):
    """out [rows][C] = x̂ from quant_act_mx6's codes and scales (dgq_dequant_act_mx6)"""
    rows, C = codes.shape[0], codes.shape[1] * 32
    _lib_call("dgq_dequant_act_mx6", _lib.ptr(codes), _lib.ptr(scale), scale.shape[1], rows, C, _lib.ptr(out), _lib.DTYPE_CODE[out.dtype],
              _lib.stream())
    return out


def gemm_mx6(q, geom, ab: "MxActBinding", out_dtype, out=None, extra=None, ups=False):
    """One dgq_gemm_mx6 launch on q = quant_act_mx6(...) of the layer input; geom = (B, H, W, C, kh, kw, stride, pad) of the layer
    (H, W: behind a folded upsample).  Returns y [M][N] (N/2 columns with the GEGLU epilogue)."""
    k = _lib.GemmMx6()
    k.scale, k.lds = q[1].data_ptr(), q[1].shape[1]
    return _block_gemm_launch("dgq_gemm_mx6", k, q, geom, ab, out_dtype, out, extra, ups, w_bits=4)


def _block_quant(ab, x_cl, geom, pre=None, ln=None, ups=False, pad_k=False):
    """the input of a block binding quantised by its format's entry; pad_k: table / scale entries up to Kp/32 (Linear layers)"""
    if ab.mx:
        return quant_act_mx6(x_cl, geom, pre, ln, ups, lds=ab.Kp // 32 if pad_k else None)
    return quant_act_block(x_cl, geom, ab.abits, pre, ln, ups, ldt=ab.Kp // 32 if pad_k else None)


def _block_gemm(ab, q, geom, out_dtype, out=None, extra=None, ups=False):
    return (gemm_mx6 if ab.mx else gemm_blockq)(q, geom, ab, out_dtype, out=out, extra=extra, ups=ups)


def quant_linear(x: torch.Tensor, ab: ActBinding, pre_act=0, residual=None, fq=None, ln=None, geglu=False):
    """x [..., K] -> [..., N].  pre_act: 0 none, 1 SiLU(x), 2 GEGLU (x is [..., 2K]: x[:K]·gelu(x[K:])) folded into the
    quantise-on-load pass; residual [..., N] and fq (see make_extra) folded into the GEMM epilogue.  geglu: the weight rows
    are (value, gate) interleaved and the epilogue writes value·gelu(gate), [..., N/2]."""
    Kin = x.shape[-1]
    K = Kin // 2 if pre_act == 2 else Kin
    x2 = x.reshape(-1, Kin)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    rows = x2.shape[0]
    pre = (None, None, pre_act) if pre_act else None
    res2 = None
    if residual is not None:
        res2 = residual.reshape(-1, ab.pw.N)
        if not res2.is_contiguous():
            res2 = res2.contiguous()
    if ab.block:                                         # real-time block mode: quantise the rows once, one GEMM
        geom = (rows, 1, 1, K, 1, 1, 1, 0)
        y = _block_gemm(ab, _block_quant(ab, x2, geom, pre, ln, pad_k=True), geom, x.dtype, extra=make_extra(res2, fq, geglu=geglu))
        return y.view(*x.shape[:-1], y.shape[-1])
    ab = _bind_rows(ab, x2, (rows, 1, 1, K, 1, 1, 1, 0), pre, ln)
    if pre_act != 2 and act_fuses(ab, rows, K, x.dtype, x2=x2):
        y = gemm_act(x2, rows, ab, x.dtype, extra=make_extra(res2, fq, geglu=geglu), pre=pre, ln=ln)
        return y.view(*x.shape[:-1], y.shape[-1])
    codes, rowsum, M = quant_act(x2, rows, 1, 1, K, 1, 1, 1, 0, ab, pre, ln)
    y = gemm_wxa8(codes, rowsum, M, ab, x.dtype, extra=make_extra(res2, fq, geglu=geglu))
    return y.view(*x.shape[:-1], y.shape[-1])


def _gemm_batches(bindings, M, outs, key, problem):
    """The dgq_gemm_wxa8_batch launches of a quant_linear_multi call: the layers grouped by key(i), 8 problems per launch;
    problem(i, j) -> (codes, rowsum, parts, extra, input_bytes) of layer i as problem j of its launch (see _gemm_args and
    GEMM_LAUNCH_HOOK)."""
    groups = {}
    for i in range(len(bindings)):
        groups.setdefault(key(i), []).append(i)
    for idxs in groups.values():
        for j0 in range(0, len(idxs), 8):
            chunk = idxs[j0:j0 + 8]
            probs = [problem(i, j) for j, i in enumerate(chunk)]
            gs = [_gemm_args(bindings[i], M, p[0], p[1], p[2], outs[i], p[3]) for i, p in zip(chunk, probs)]
            arr = (_lib.GemmArgs * len(gs))(*gs)

            def issue(arr=arr, n_chunk=len(gs), _keep=gs):
                _lib_call("dgq_gemm_wxa8_batch", n_chunk, _c.cast(arr, _c.c_void_p), _lib.stream())
            issue()
            if GEMM_LAUNCH_HOOK is not None:
                GEMM_LAUNCH_HOOK(issue, [(M, bindings[i], outs[i].element_size(), p[4]) for i, p in zip(chunk, probs)])


def quant_linear_multi(x: torch.Tensor, bindings, ln=None):
    """[quant_linear(x, ab, ln=ln) for ab in bindings] with the launches shared: layers that consume the SAME input — the
    q / k / v projections of a self-attention, the to_k / to_v of every cross-attention (one text context) — are quantised
    by one dgq_quant_act_batch per (kernel variant, scale mode) and multiplied by one dgq_gemm_wxa8_batch per scale mode,
    8 problems per launch — or, where every such launch may quantise its own rows (_multi_fuses), by the latter alone.  Same
    kernels, same arithmetic, same results as the one-layer calls."""
    Kin = x.shape[-1]
    x2 = x.reshape(-1, Kin)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    M = x2.shape[0]
    dev = x2.device
    if any(ab.block for ab in bindings):                # real-time block layers: the shared input is quantised ONCE per bit width, one GEMM each
        geom = (M, 1, 1, Kin, 1, 1, 1, 0)
        quants, res = {}, {}
        for i, ab in enumerate(bindings):
            if ab.block:
                assert ab.pw.K == Kin and ab.pw.taps == 1
                fmt = (ab.mx, ab.abits)                 # (one padded K per input width: every binding's Kp / 32 is the same)
                if fmt not in quants:
                    quants[fmt] = _block_quant(ab, x2, geom, None, ln, pad_k=True)
                res[i] = _block_gemm(ab, quants[fmt], geom, x.dtype)
                res[i] = res[i].view(*x.shape[:-1], res[i].shape[-1])
        rest = [i for i in range(len(bindings)) if i not in res]
        if rest:
            for i, y in zip(rest, quant_linear_multi(x, [bindings[i] for i in rest], ln=ln)):
                res[i] = y
        return [res[i] for i in range(len(bindings))]
    if any(ab.dynamic for ab in bindings):              # real-time layers of one input (and one bit width) share their row tables
        tables = {}
        for ab in bindings:
            if ab.dynamic and ab.abits not in tables:
                tables[ab.abits] = act_row_params(x2, (M, 1, 1, Kin, 1, 1, 1, 0), ab.abits, None, ln)
        bindings = [ab.bound(*tables[ab.abits]) if ab.dynamic else ab for ab in bindings]
    outs = [torch.empty((M, ab.pw.N), dtype=x.dtype, device=dev) for ab in bindings]
    per_m = [0 if ab.mode == "perK" else 1 for ab in bindings]
    if _multi_fuses(bindings, M, Kin, x.dtype, x2):
        def fused(i, j):                               # (one shared input: its bytes are counted on the launch's first problem)
            ab = bindings[i]
            return None, None, 1, _with_act(None, ab, 0, make_act(x2, ab, None, ln)), (M * Kin * x2.element_size() if j == 0 else 0)
        _gemm_batches(bindings, M, outs, lambda i: per_m[i], fused)
        return [o.view(*x.shape[:-1], o.shape[-1]) for o in outs]
    lib = _lib.load()
    qa = []
    for ab in bindings:
        assert ab.pw.K == Kin and ab.pw.taps == 1
        a, keep = _quant_args(x2, (M, 1, 1, Kin, 1, 1, 1, 0), ab, None, ln)
        parts = quant_splits(a, M)
        codes = torch.empty((M, ab.Kp), dtype=torch.int8, device=dev)
        rowsum = torch.empty((parts, M), dtype=torch.float32, device=dev)
        a.codes, a.rowsum = codes.data_ptr(), rowsum.data_ptr()
        qa.append((lib.dgq_quant_act_variant(_c.byref(a)), a, codes, rowsum, parts, keep))
    groups = {}
    for i, q in enumerate(qa):
        groups.setdefault((q[0], per_m[i]), []).append(i)
    for idxs in groups.values():
        for j0 in range(0, len(idxs), 8):
            chunk = idxs[j0:j0 + 8]
            arr = (_lib.QuantActArgs * len(chunk))(*[qa[i][1] for i in chunk])

            def issue_q(arr=arr, n_chunk=len(chunk), _keep=[qa[i] for i in chunk]):
                _lib_call("dgq_quant_act_batch", n_chunk, _c.cast(arr, _c.c_void_p), _lib.stream())
            issue_q()
            if QUANT_LAUNCH_HOOK is not None:          # one shared input, one code matrix + row sums per problem
                QUANT_LAUNCH_HOOK(issue_q, M * Kin * x2.element_size(), sum(M * bindings[i].Kp + 4 * qa[i][4] * M for i in chunk))
    _gemm_batches(bindings, M, outs, lambda i: (per_m[i], bindings[i].pw.bits),
                  lambda i, j: (qa[i][2], qa[i][3], qa[i][4], with_layer_tables(None, bindings[i], 0), 0))
    return [o.view(*x.shape[:-1], o.shape[-1]) for o in outs]


def _gn_input(x, x_store, norm):
    """(scale, shift) [B][C] of the GroupNorm norm = (groups, eps, gamma, beta, act) of x (logical NCHW; x_store its [B][H][W][C]
    storage): from the partials the producing GEMM(s) left on x, else by a statistics pass"""
    groups, eps, gamma, beta, _act = norm
    B, C, H, W = x.shape
    gn = _gn_of(x)
    if gn is not None and gn["B"] == B and gn["HW"] == H * W and gn["C"] == C and C % groups == 0:
        return groupnorm_from_partials(gn, groups, eps, gamma, beta)
    return groupnorm_scale_shift(x_store, B, H * W, C, groups, eps, gamma, beta)


def _gn_partial(want, M, N, HW, device):
    """the [M/16][N][2] buffer a launch writes the GroupNorm partials of its [M][N] output (HW rows per image) into, for whoever
    normalises it next — where the caller wants them (its own condition) and the epilogues can form them; else None"""
    if want and GN_FROM_GEMM and HW % 16 == 0 and N % 4 == 0:
        return torch.empty((M // 16, N, 2), dtype=torch.float32, device=device)
    return None


def _gn_tagged(y, part, B, Ho, Wo, N):
    """the [M][N] rows y as the logical NCHW output, carrying its GroupNorm partials (if any) as ``_dgq_gn``"""
    out = y.view(B, Ho, Wo, N).permute(0, 3, 1, 2)
    if part is not None:
        out._dgq_gn = dict(parts=[(part, N)], B=B, HW=Ho * Wo, C=N, ver=out._version)
    return out


def quant_conv2d(x: torch.Tensor, ab: ActBinding, kh, kw, stride, pad, norm=None, residual=None, bias_rows=None, gn_out=True, upsample=False,
                 out=None, out2=None):
    """x logical NCHW (any strides; made channels-last) -> logical NCHW output in channels-last storage.
    norm = (groups, eps, gamma, beta, act): GroupNorm (+SiLU) of x folded into the quantise-on-load pass;
    residual (logical NCHW, same shape as the output) is added in the GEMM epilogue; bias_rows [B][N] likewise, one row
    per image (conv1(...) + time_emb_proj(...)[:, :, None, None]).
    upsample: the layer's input is F.interpolate(x, scale_factor=2, mode="nearest") (Upsample2D.forward); where the quantise
    variant of the layer can read x through that mapping the 4x tensor is never written, otherwise it is materialised here.
    out / out2: [M][N] row views (own row pitch) the output is stored into / stored into AS WELL (OutputRedirect: the halves of a
    channel-concatenation buffer); the returned tensor is a view of ``out`` then."""
    if upsample and (norm is not None or ab.mode == "scalar" or kh * kw == 1):
        x, upsample = F.interpolate(x, scale_factor=2.0, mode="nearest"), False
    B, C, H, W = x.shape
    if upsample:
        H, W = 2 * H, 2 * W                           # the layer's input geometry; x stays the (H/2) x (W/2) source
    xc = x.contiguous(memory_format=torch.channels_last)
    x_store = xc.permute(0, 2, 3, 1)                  # [B,H,W,C] view over the same storage, contiguous
    pre = (*_gn_input(x, x_store, norm), norm[4]) if norm is not None else None
    if not ab.block:
        ab = _bind_rows(ab, x_store, (B, H, W, C, kh, kw, stride, pad), pre, ups=upsample)      # (real-time: this operand's row tables)
    Ho = (H + 2 * pad - kh) // stride + 1
    Wo = (W + 2 * pad - kw) // stride + 1
    M = B * Ho * Wo
    N = ab.pw.N
    res2, res_div = None, 1
    if residual is not None:
        res2 = residual.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1).reshape(M, N)
    elif bias_rows is not None:                       # [B][N]: one row per image, broadcast over its Ho*Wo positions
        res2, res_div = bias_rows.contiguous(), M // B

    def extra_with(part, conv=None):
        return make_extra(res2, res_div=res_div, gn_partial=part, conv=conv, y2=out2)
    if ab.block:
        # real-time block mode: every input pixel (the SOURCE pixel of a folded upsample; a pixel's block parameters do not depend on
        # the taps that read it) is quantised once, the GEMM gathers the taps
        geom = (B, H, W, C, kh, kw, stride, pad)
        q = _block_quant(ab, x_store, geom, pre, ups=upsample)
        part = _gn_partial(gn_out, M, N, Ho * Wo, x.device)
        y = _block_gemm(ab, q, geom, x.dtype, out=out, extra=extra_with(part), ups=upsample)
        return _gn_tagged(y, part, B, Ho, Wo, N)
    if kh == 1 and kw == 1 and stride == 1 and pad == 0 and act_fuses(ab, M, C, x.dtype, x2=x_store.reshape(M, C)):
        # a 1x1 convolution is a Linear layer over the pixels: one launch, the GEMM quantises its own rows (dgq_gemm_act_t)
        part = _gn_partial(gn_out, M, N, Ho * Wo, x.device)
        y = gemm_act(x_store.reshape(M, C), M, ab, x.dtype, extra=extra_with(part), pre=pre, rows_per_image=H * W, out=out)
        return _gn_tagged(y, part, B, Ho, Wo, N)
    if kh * kw > 1 and not upsample and conv_act_fuses(ab, B, H, W, C, kh, kw, stride, pad, x.dtype, x_store):
        # the unfolded operand is quantised INSIDE the GEMM launch from a staged input patch (dgq_gemm_act_t with kh > 1): one launch,
        # no code matrix (QuantLayer.forward, quant_layer.py:626-661, as one kernel)
        part = _gn_partial(gn_out, M, N, Ho * Wo, x.device)
        act = make_act(x_store, ab, pre, rows_per_image=H * W, conv=(B, H, W, C, kh, kw, stride, pad))
        y = gemm_wxa8(None, None, M, ab, x.dtype, out=out, extra=_with_act(extra_with(part), ab, M, act),
                      _fused_bytes=x.element_size() * B * H * W * C)
        return _gn_tagged(y, part, B, Ho, Wo, N)
    implicit = CONV_IMPLICIT and ab.mode == "scalar" and kh * kw > 1 and C % 16 == 0 and ab.pw.bits == 4 and ab.conv_zero_code() is not None
    conv_desc = None
    if implicit:
        # ONE (δ, z) for the whole operand (the reference's native path F.conv2d(aqtizer(x), ŵ), quant_layer.py:659): every input
        # pixel is quantised once, as a 1x1 layer in natural order, and the GEMM gathers the taps from that int8 NHWC tensor
        # (dgq_gemm_conv_t) — the 9x unfolded operand is never written
        abi = ab.input_binding(C)
        codes, pixsum, _ = quant_act(x_store, B, H, W, C, 1, 1, 1, 0, abi, pre)
        rowsum = torch.empty((1, M), dtype=torch.float32, device=x.device)
        cv = _lib.GemmConv()
        cv.codes_in, cv.pixsum, cv.fill = codes.data_ptr(), pixsum.data_ptr(), ab.conv_fill().data_ptr()
        cv.B, cv.H, cv.W, cv.C, cv.ldc, cv.kh, cv.kw, cv.stride, cv.pad, cv.Ho, cv.Wo = B, H, W, C, abi.Kp, kh, kw, stride, pad, Ho, Wo
        cv.zero_code, cv.pixsum_parts = ab.conv_zero_code(), pixsum.shape[0]
        conv_desc = (cv, pixsum)
    else:
        qa = quant_act(x_store, B, H, W, C, kh, kw, stride, pad, ab, pre, ups=upsample)
        if qa is None:                                # no folded form for this layer's quantise variant: materialise the upsample
            return quant_conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), ab, kh, kw, stride, pad, norm=norm, residual=residual,
                                bias_rows=bias_rows, gn_out=gn_out, out=out, out2=out2)
        codes, rowsum, M = qa
    # GroupNorm partials of the output: from the GEMM's own epilogue, or — a K-split launch — from its combine kernel
    # (DGQ_GN_FROM_SPLITK=0: only unsplit launches, the tensor gets a statistics pass otherwise)
    part = _gn_partial(gn_out and (GN_FROM_SPLITK or _lib.load().dgq_gemm_plan_splits(M, N, ab.Kp, ab.pw.bits, 0 if ab.mode == "perK" else 1,
                                                                                      WORKSPACE_BYTES) == 1), M, N, Ho * Wo, x.device)
    y = gemm_wxa8(codes, rowsum, M, ab, x.dtype, out=out, extra=extra_with(part, conv_desc))
    return _gn_tagged(y, part, B, Ho, Wo, N)


def _weight_only_operand(x, K, kh, kw, stride, pad, upsample, what):
    """What the weight-only kernels read of x for a weight of K columns: (storage, (B, H, W, C, kh, kw, stride, pad), rows -> result).
    x logical NCHW with K = kh·kw·C (made channels-last; ``upsample``: seen through a 2x nearest upsample), or [..., K] for a
    Linear layer (kh = kw = 1, any rank: the rows are everything but the last dimension)."""
    if x.dim() == 4 and K == kh * kw * x.shape[1]:
        B, C, H, W = x.shape
        if upsample:
            H, W = 2 * H, 2 * W
        Ho = (H + 2 * pad - kh) // stride + 1
        Wo = (W + 2 * pad - kw) // stride + 1
        return (x.contiguous(memory_format=torch.channels_last), (B, H, W, C, kh, kw, stride, pad),
                lambda y: y.view(B, Ho, Wo, -1).permute(0, 3, 1, 2))
    assert K == x.shape[-1] and kh == kw == 1 and not upsample, "dgq %s: weight [N][%d] does not match input %s" % (what, K, tuple(x.shape))
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    return x2, (x2.shape[0], 1, 1, K, 1, 1, 1, 0), lambda y: y.view(*x.shape[:-1], -1)


def conv2d_f32w(x: torch.Tensor, w_nat: torch.Tensor, bias, kh, kw, stride, pad, norm=None, out2=None, gn_out=False):
    """Weight-only state: conv2d / linear of UNQUANTISED activations with the dequantised weight, exact fp32 MFMA with the
    im2col folded into the load (dgq_conv2d_f32w).  x logical NCHW (made channels-last) or [..., K] for a Linear layer
    (kh = kw = 1); w_nat [N][kh·kw·C] fp32 with K in (tap, c) order; bias [N] fp32 or None.
    norm = (groups, eps, gamma, beta, act) folds GroupNorm (+SiLU) of a 4-D x into the load, as in quant_conv2d."""
    N = w_nat.shape[0]
    xs, geom, result = _weight_only_operand(x, w_nat.shape[1], kh, kw, stride, pad, False, "conv2d_f32w")
    is_conv = xs.dim() == 4
    assert is_conv or norm is None
    if not is_conv:
        out2 = None                                     # (a Linear call has never honoured it)
    sc, sh = _gn_input(x, xs.permute(0, 2, 3, 1), norm) if norm is not None else (None, None)
    B, H, W = geom[:3]
    Ho = (H + 2 * pad - kh) // stride + 1
    Wo = (W + 2 * pad - kw) // stride + 1
    M = B * Ho * Wo
    y = torch.empty((M, N), dtype=x.dtype, device=x.device)
    part = _gn_partial(gn_out and is_conv and N > 8, M, N, Ho * Wo, x.device)
    _lib_call("dgq_conv2d_f32w", _lib.ptr(xs), _lib.DTYPE_CODE[x.dtype], *geom,
              _lib.ptr(w_nat), _lib.ptr(bias), N, _lib.ptr(y), _lib.DTYPE_CODE[y.dtype], N,
              _lib.ptr(sc), _lib.ptr(sh), int(norm[4]) if norm is not None else 0,
              _lib.ptr(out2), out2.stride(0) if out2 is not None else 0, _lib.ptr(part), _lib.stream())
    return _gn_tagged(y, part, B, Ho, Wo, N) if is_conv else result(y)


def conv2d_wq(x: torch.Tensor, pw: PackedWeight, kh, kw, stride, pad, upsample=False, geglu_rows=False):
    """Weight-only state from the packed codes (dgq_conv2d_wq): bit for bit ``conv2d_f32w(x, δ·(q − z) in natural order, pw.bias)``,
    without an fp32 copy of the weight — each element is dequantised as the kernel stages it.  Inputs and returned views as in
    conv2d_f32w: x logical NCHW (made channels-last) or [..., K] for a Linear layer (kh = kw = 1).  ``upsample``: the layer sees
    F.interpolate(x, scale_factor=2, mode="nearest"), read through the (h/2, w/2) mapping and never written.  ``geglu_rows``: pw's
    rows are interleaved (QuantLayer.geglu_rows) and the output comes back in the reference's column order.  N > 8."""
    w_img, Kp = pw.natural()
    N = pw.N
    xs, geom, result = _weight_only_operand(x, pw.K, kh, kw, stride, pad, upsample, "conv2d_wq")
    B, H, W = geom[:3]
    M = B * ((H + 2 * pad - kh) // stride + 1) * ((W + 2 * pad - kw) // stride + 1)
    y = torch.empty((M, N), dtype=x.dtype, device=x.device)
    _lib_call("dgq_conv2d_wq", _lib.ptr(xs), _lib.DTYPE_CODE[x.dtype], *geom, int(upsample),
              _lib.ptr(w_img), pw.bits, Kp, _lib.ptr(pw.alpha), _lib.ptr(pw.zp_true), _lib.ptr(pw.bias), N, int(geglu_rows),
              _lib.ptr(y), _lib.DTYPE_CODE[y.dtype], N, _lib.stream())
    return result(y)


def conv2d_wq_mfma16(x: torch.Tensor, pw: PackedWeight, kh, kw, stride, pad, upsample=False, geglu_rows=False):
    """Weight-only state on the bf16 / f16 matrix cores (dgq_conv2d_wq_mfma16), beside conv2d_wq: the same operands, arguments and
    returned views, NOT the same bits — y = b + δ·Σ_k x̃·(q − z) with the integer q − z as the 16-bit operand, fp32 accumulation in
    the kernel's own order and δ in the epilogue.  bf16 / f16 x enter as they are; fp32 x as two bf16 terms (|x − x̃| <= 2^-16·|x|).
    pw.mfma16_eligible() must hold (the caller's check: QuantLayer routes an ineligible weight to conv2d_wq)."""
    assert pw.mfma16_eligible(), "dgq conv2d_wq_mfma16: q − z is not an integer within the operand's exact range"
    w_img, Kp = pw.natural()
    N = pw.N
    xs, geom, result = _weight_only_operand(x, pw.K, kh, kw, stride, pad, upsample, "conv2d_wq_mfma16")
    B, H, W = geom[:3]
    M = B * ((H + 2 * pad - kh) // stride + 1) * ((W + 2 * pad - kw) // stride + 1)
    y = torch.empty((M, N), dtype=x.dtype, device=x.device)
    _lib_call("dgq_conv2d_wq_mfma16", _lib.ptr(xs), _lib.DTYPE_CODE[x.dtype], *geom, int(upsample),
              _lib.ptr(w_img), pw.bits, Kp, _lib.ptr(pw.alpha), _lib.ptr(pw.zp_true), _lib.ptr(pw.bias), N, int(geglu_rows),
              _lib.ptr(y), _lib.DTYPE_CODE[y.dtype], N, _lib.stream())
    return result(y)


def layernorm_row_stats(x2d: torch.Tensor, eps):
    """[rows][2] fp32 (mean, rstd) of the rows of x2d [rows][C] (dgq_layernorm_row_stats: two passes over the row in
    registers, sums and final arithmetic in fp64, each value rounded to fp32 once) — the ``ln`` input of conv2d_wq_mfma16_fused.  C % 4 == 0 and C <= 2048, else the library refuses."""
    assert x2d.dim() == 2 and x2d.is_contiguous()
    rows, C = x2d.shape
    out = torch.empty((rows, 2), dtype=torch.float32, device=x2d.device)
    _lib_call("dgq_layernorm_row_stats", _lib.ptr(x2d), _lib.DTYPE_CODE[x2d.dtype], rows, C, _c.c_float(eps), _lib.ptr(out), _lib.stream())
    return out


def layernorm_row_stats_ok(C):
    """what dgq_layernorm_row_stats accepts (a caller with another width keeps the nn.LayerNorm module)"""
    return C % 4 == 0 and C <= 2048


def _table16(t: torch.Tensor) -> torch.Tensor:
    """t as a contiguous fp32 table on a 16-byte boundary, as the fused kernel's vector loads of it need: the tensor itself where it
    already is one (every fresh allocation), else a copy — a γ / β that is a view at an odd offset of a larger buffer"""
    t = as_f32(t).contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def conv2d_wq_mfma16_fused(x: torch.Tensor, pw: PackedWeight, kh, kw, stride, pad, upsample=False, geglu_rows=False, norm=None, ln=None,
                           pre_act=0, residual=None, bias_rows=None, geglu=False):
    """conv2d_wq_mfma16 with the layer's element-wise neighbours folded into the launch (dgq_conv2d_wq_mfma16_fused): operands and
    returned views as there, and with nothing to fold the same bits.
    norm: GroupNorm of a 4-D x folded into the load — (groups, eps, gamma, beta, act) as in quant_conv2d (statistics from the partials x
          carries, else by a pass; act 1 = SiLU behind it), or the fp32 tables themselves, (scale, shift) [B][C];
    ln:   LayerNorm of a Linear x likewise — (stats, gamma, beta) with stats = layernorm_row_stats(x rows, eps);
    pre_act 1: SiLU(x) (behind the norm);  residual (the output's shape) and bias_rows [B][N] (one row per image) are added in fp32 before
    the one rounding — both in the output's column order, with geglu_rows too (the kernel reads them at the column a packed row stands
    for);  geglu (needs geglu_rows): the result is value·gelu(gate), [..., N/2], bias_rows then [B][N] with the value columns first."""
    assert pw.mfma16_eligible(), "dgq conv2d_wq_mfma16_fused: q − z is not an integer within the operand's exact range"
    w_img, Kp = pw.natural()
    N = pw.N
    xs, geom, result = _weight_only_operand(x, pw.K, kh, kw, stride, pad, upsample, "conv2d_wq_mfma16_fused")
    B, H, W = geom[:3]
    M = B * ((H + 2 * pad - kh) // stride + 1) * ((W + 2 * pad - kw) // stride + 1)
    f = _lib.Wq16Fuse()
    keep = []
    if norm is not None:
        if len(norm) == 5:
            sc, sh = _gn_input(x, xs.permute(0, 2, 3, 1), norm)
            pre_act = int(norm[4])
        else:
            sc, sh = (_table16(t) for t in norm)
        keep += [sc, sh]
        f.pre_scale, f.pre_shift = sc.data_ptr(), sh.data_ptr()
    if ln is not None:
        st, ga, be = ln[0], _table16(ln[1]), _table16(ln[2])
        assert st.dtype == torch.float32 and st.is_contiguous() and tuple(st.shape) == (M, 2)
        keep += [st, ga, be]
        f.ln_stats, f.ln_gamma, f.ln_beta = st.data_ptr(), ga.data_ptr(), be.data_ptr()
    f.pre_act = int(pre_act)
    if residual is not None:
        if xs.dim() == 4:
            residual = residual.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
        res2 = residual.reshape(M, N).to(x.dtype).contiguous()
        keep.append(res2)
        f.residual, f.ldr = res2.data_ptr(), N
    if bias_rows is not None:
        br = bias_rows.reshape(B if xs.dim() == 4 else M, N).to(x.dtype).contiguous()
        keep.append(br)
        f.bias_rows = br.data_ptr()
    f.geglu_out = int(bool(geglu))
    ncols = N // 2 if geglu else N
    y = torch.empty((M, ncols), dtype=x.dtype, device=x.device)
    _lib_call("dgq_conv2d_wq_mfma16_fused", _lib.ptr(xs), _lib.DTYPE_CODE[x.dtype], *geom, int(upsample),
              _lib.ptr(w_img), pw.bits, Kp, _lib.ptr(pw.alpha), _lib.ptr(pw.zp_true), _lib.ptr(pw.bias), N, int(geglu_rows),
              _lib.ptr(y), _lib.DTYPE_CODE[y.dtype], ncols, _c.byref(f), _lib.stream())
    del keep                                             # (the launch is enqueued on the tensors' stream: the allocator keeps their memory until it ran)
    return result(y)


# ------------------------------------------------------------------------------------------ attention side
def fakequant_rows(x2d: torch.Tensor, T, D, mode, delta, zp, skip, bits, out=None):
    """x2d [rows][C] contiguous; see dgq_fakequant_rows."""
    assert x2d.is_contiguous()
    rows, C = x2d.shape
    out = x2d if out is None else out
    _lib_call("dgq_fakequant_rows", _lib.ptr(x2d), _lib.ptr(out), _lib.DTYPE_CODE[x2d.dtype], rows, C, T, D, mode,
              _lib.ptr(delta), _lib.ptr(zp), skip, bits, _lib.stream())
    return out


def timestep_embedding(timesteps: torch.Tensor, dim: int, out_dtype=torch.float32):
    """Timesteps.forward (diffusers_rewrite/sd.py:19-39) as one launch: ``timesteps`` [rows] int64 or fp32 (any stride: the expanded
    single timestep has stride 0) -> [rows, dim] = cat(cos, sin)."""
    assert timesteps.dim() == 1 and timesteps.dtype in (torch.int64, torch.float32) and dim % 2 == 0
    rows = timesteps.shape[0]
    out = torch.empty((rows, dim), dtype=out_dtype, device=timesteps.device)
    _lib_call("dgq_timestep_embedding", _lib.ptr(timesteps), 1 if timesteps.dtype == torch.float32 else 0, int(timesteps.stride(0)), rows, dim,
              _lib.ptr(out), _lib.DTYPE_CODE[out_dtype], _lib.stream())
    return out


def _dense_layout(t):
    """0: [N,C,H,W] contiguous, 1: channels-last dense, None: neither (4-D tensors; 2-/3-D contiguous counts as 0)"""
    if t.is_contiguous():
        return 0
    if t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last):
        return 1
    return None


def cfg_ddim_step(eps_uncond, eps_cond, sample, guidance, s1, inv_s2, s3, s4):
    """eps = e_u + guidance·(e_c − e_u) (``eps_cond`` None: eps = e_u), then the DDIM update s3·((x − s1·eps)·inv_s2) + s4·eps in the
    order of the eager chain (pipeline_stable_diffusion.py:1037-1044, scheduling_ddim.py); fp32 / fp16 / bf16 tensors (one dtype; a 16-bit
    chain rounds after every statement as the eager one does); ``sample`` contiguous, the eps halves in
    the same layout or channels-last (what the UNet returns).  Returns None when the layouts are not of that kind."""
    lay = _dense_layout(eps_uncond)
    if (lay is None or not sample.is_contiguous() or sample.dim() < 2 or eps_uncond.shape != sample.shape
            or (eps_cond is not None and (eps_cond.shape != sample.shape or _dense_layout(eps_cond) != lay))):
        return None
    for t in (eps_uncond, eps_cond):
        assert t is None or t.dtype == sample.dtype
    C = sample.shape[1]
    HW = sample.numel() // (sample.shape[0] * C)
    out = torch.empty_like(sample)
    _lib_call("dgq_cfg_ddim_step", _lib.ptr(eps_uncond), _lib.ptr(eps_cond), _lib.ptr(sample), _lib.ptr(out), _lib.DTYPE_CODE[sample.dtype], sample.numel(), C, HW, lay,
              _c.c_float(guidance), _c.c_float(s1), _c.c_float(inv_s2), _c.c_float(s3), _c.c_float(s4), _lib.stream())
    return out


def max_f32(p: torch.Tensor, skip_cols=0):
    assert p.is_contiguous() and p.dtype == torch.float32
    S = p.shape[-1]
    rows = p.numel() // S
    out = torch.zeros((1,), dtype=torch.float32, device=p.device)
    _lib_call("dgq_max_f32", _lib.ptr(p), rows, S, skip_cols, _lib.ptr(out), _lib.stream())
    return out


def logquant_f32(p: torch.Tensor, delta: torch.Tensor, bits, skip_cols=0, out=None):
    assert p.is_contiguous() and p.dtype == torch.float32
    S = p.shape[-1]
    rows = p.numel() // S
    out = p if out is None else out
    _lib_call("dgq_logquant_f32", _lib.ptr(p), _lib.ptr(out), rows, S, skip_cols, _lib.ptr(delta), bits, _lib.stream())
    return out


SMALLM_MAX_M, SMALLM_MAX_K, SMALLM_MAX_PROBLEMS = 16, 2048, 24


def linear_smallm_batch(x2d: torch.Tensor, bindings, pre_act=0):
    """[ab.pw(aqtizer(act(x2d))) for ab in bindings] for scalar-quantizer Linear layers sharing the input x2d [M <= 16][K]
    in ONE launch per 24 layers (dgq_linear_smallm_batch): the time-embedding projections of a UNet forward."""
    assert x2d.dim() == 2 and x2d.stride(1) == 1 and x2d.dtype in _lib.DTYPE_CODE
    M, K = x2d.shape
    outs = []
    for i0 in range(0, len(bindings), SMALLM_MAX_PROBLEMS):
        chunk = bindings[i0:i0 + SMALLM_MAX_PROBLEMS]
        probs = (_lib.SmallMProblem * len(chunk))()
        keep = []
        for j, ab in enumerate(chunk):
            pw = ab.pw
            assert ab.mode != "perK" and ab.L == 1 and pw.K == K and pw.taps == 1
            y = torch.empty((M, pw.N), dtype=x2d.dtype, device=x2d.device)
            q = probs[j]
            q.wpacked, q.alpha, q.zw = ab.wpacked.data_ptr(), pw.alpha.data_ptr(), pw.zw.data_ptr()
            q.gamma, q.vn = ab.gamma.data_ptr(), ab.vn.data_ptr()
            q.mdelta, q.mzp = ab.mdelta.data_ptr(), ab.mzp.data_ptr()
            q.y, q.ldy, q.N, q.Kp, q.w_bits, q.a_bits = y.data_ptr(), y.stride(0), pw.N, ab.Kp, pw.bits, ab.abits
            keep.append(y)
        _lib_call("dgq_linear_smallm_batch", _lib.ptr(x2d), _lib.DTYPE_CODE[x2d.dtype], M, K, x2d.stride(0), pre_act,
                  len(chunk), _c.cast(probs, _c.c_void_p), _lib.DTYPE_CODE[x2d.dtype], _lib.stream())
        outs += keep
    return outs


def minmax_rows_cols(x2d: torch.Tensor, rows=True, cols=True):
    """Row-wise and column-wise (min, max) of a contiguous [R][C] view — the statistics of DGQ's calibration producer
    (dgq_minmax_rows_cols).  Returns (rowmin, rowmax, colmin, colmax), fp32, None for a pair that was not requested."""
    assert x2d.dim() == 2 and x2d.stride(1) == 1 and x2d.dtype in _lib.DTYPE_CODE
    R, C = x2d.shape
    dev = x2d.device
    rmin = rmax = cmin = cmax = part = None
    slices = max(1, min(256, R // 64))
    if rows:
        rmin = torch.empty((R,), dtype=torch.float32, device=dev)
        rmax = torch.empty((R,), dtype=torch.float32, device=dev)
    if cols:
        cmin = torch.empty((C,), dtype=torch.float32, device=dev)
        cmax = torch.empty((C,), dtype=torch.float32, device=dev)
        part = torch.empty((2 * slices * C,), dtype=torch.float32, device=dev)
    _lib_call("dgq_minmax_rows_cols", _lib.ptr(x2d), _lib.DTYPE_CODE[x2d.dtype], R, C, x2d.stride(0),
              _lib.ptr(rmin), _lib.ptr(rmax), _lib.ptr(cmin), _lib.ptr(cmax), _lib.ptr(part), slices, _lib.stream())
    return rmin, rmax, cmin, cmax


ATTN_HEAD_DIMS = (8, 16, 40, 64, 80, 160)
_ATTN_WS = {}


def _attn_workspace(device, nbytes):
    """The attention kernels' scratch (δ scalar, row statistics, K / V tile images): one grow-only buffer per device and
    stream chain instead of an allocation per call — attentions of one forward run back to back on one stream, each fully
    overwrites what it reads.  Under graph capture a buffer allocated here belongs to the graph's pool like any other."""
    cap = torch.cuda.is_current_stream_capturing()
    key = (str(device), torch.cuda.current_stream(device).cuda_stream if not cap else "capture")
    buf = _ATTN_WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty((max(nbytes, 1 << 20),), dtype=torch.uint8, device=device)      # caching allocator: 512-byte aligned
        if not cap:
            _ATTN_WS[key] = buf
    return buf


def attention_fuses_fakequant(D, mode):
    """True where dgq_attention_f32 applies the q/k/v fake-quantizers itself (``fq=``)."""
    return bool(_lib.load().dgq_attention_fuses_fakequant(D, mode))


def attention(q, k, v, H, D, scale, mode, skip, delta, bits, fq=None):
    """q [B,T,H*D], k/v [B,S,H*D] contiguous (fp32; fp16 / bf16 in the quantised modes) -> o [B,T,H*D]; see dgq_attention.
    fq: optional 3-tuple for q, k, v of None | (mode, delta, zp, skip, bits) — the aqtizer_q/k/v quantizers applied on
    load (only where ``attention_fuses_fakequant(D, mode)``)."""
    assert q.dtype in _lib.DTYPE_CODE and k.dtype == q.dtype and v.dtype == q.dtype
    assert q.is_contiguous() and k.is_contiguous() and v.is_contiguous()
    B, T, _ = q.shape
    S = k.shape[1]
    nbytes = _lib.load().dgq_attention_workspace_bytes(B, H, T, S, D)
    ws = _attn_workspace(q.device, nbytes)
    desc = None
    if fq is not None and any(f is not None for f in fq):
        desc = (_lib.AttnFq * 3)()
        for i, f in enumerate(fq):
            if f is None:
                desc[i].mode = -1
                continue
            fmode, fd, fz, fskip, fbits = f
            ntok = (T if i == 0 else S) - fskip
            need = 1 if fmode == 0 else (ntok if fmode == 1 else D)
            assert fd.numel() == need and fz.numel() == need and fd.dtype == torch.float32 and fd.is_contiguous(), \
                "q/k/v quantizer table has %d entries, kernel addresses %d" % (fd.numel(), need)
            desc[i].mode, desc[i].skip, desc[i].bits = fmode, fskip, fbits
            desc[i].delta, desc[i].zero_point = _lib.ptr(fd), _lib.ptr(fz)
    o = torch.empty_like(q)

    def issue():
        _lib_call("dgq_attention", _lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(o), _lib.DTYPE_CODE[q.dtype], B, H, T, S, D,
                  _c.c_float(scale), mode, skip, _lib.ptr(delta), bits,
                  _c.cast(desc, _c.c_void_p) if desc is not None else None, _lib.ptr(ws), nbytes, _lib.stream())
    issue()
    if ATTN_LAUNCH_HOOK is not None:                   # Q·Kᵀ and P·V: 4·T·S·D flops per (batch, head); q, k, v read and o written once
        ATTN_LAUNCH_HOOK(issue, 4.0 * T * S * D * B * H, (2 * B * T + 2 * B * S) * H * D * q.element_size())
    return o


attention_f32 = attention


def attention_mfma16(q, k, v, H, D, scale):
    """Un-quantised attention of the 16-bit states on the bf16 / f16 matrix cores (dgq_attention_mfma16), beside ``attention``: q [B,T,H*D],
    k/v [B,S,H*D] contiguous fp16 / bf16 of one dtype -> o [B,T,H*D].  One launch, no workspace; fp32 scores and accumulation, the
    probabilities never leave the registers.  Opt-in through the attention modules' ``attention_mfma16`` flag."""
    assert q.dtype in (torch.float16, torch.bfloat16) and k.dtype == q.dtype and v.dtype == q.dtype
    assert q.is_contiguous() and k.is_contiguous() and v.is_contiguous()
    B, T, _ = q.shape
    S = k.shape[1]
    o = torch.empty_like(q)

    def issue():
        _lib_call("dgq_attention_mfma16", _lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(o), _lib.DTYPE_CODE[q.dtype], B, H, T, S, D,
                  _c.c_float(scale), _lib.stream())
    issue()
    if ATTN_LAUNCH_HOOK is not None:                   # the accounting of ``attention``
        ATTN_LAUNCH_HOOK(issue, 4.0 * T * S * D * B * H, (2 * B * T + 2 * B * S) * H * D * q.element_size())
    return o


def attention_mfma16_f32(q, k, v, H, D, scale):
    """Un-quantised attention of the fp32 state on the bf16 matrix cores (dgq_attention_mfma16_f32), beside ``attention`` mode 0: q [B,T,H*D],
    k/v [B,S,H*D] contiguous fp32 -> fp32 o [B,T,H*D].  One launch, no workspace; q, k, v and the probabilities enter the matrix cores
    as two-term bf16 splits, softmax and accumulation in fp32, an IEEE division at the end.  Opt-in through the attention
    modules' ``attention_mfma16_fp32`` flag."""
    assert q.dtype == torch.float32 and k.dtype == q.dtype and v.dtype == q.dtype
    assert q.is_contiguous() and k.is_contiguous() and v.is_contiguous()
    B, T, _ = q.shape
    S = k.shape[1]
    o = torch.empty_like(q)

    def issue():
        _lib_call("dgq_attention_mfma16_f32", _lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(o), B, H, T, S, D, _c.c_float(scale), _lib.stream())
    issue()
    if ATTN_LAUNCH_HOOK is not None:                   # the accounting of ``attention``
        ATTN_LAUNCH_HOOK(issue, 4.0 * T * S * D * B * H, (2 * B * T + 2 * B * S) * H * D * q.element_size())
    return o


def attention_sync_timeouts():
    """Workgroups of single-launch attention calls (csrc/attn_one.hip) that ever gave up the wait for the real-time δ exchange
    in this process; synchronises.  0 unless a grid was not resident as a whole."""
    n = _lib.load().dgq_attention_sync_timeouts()
    if n < 0:
        raise RuntimeError("dgq_attention_sync_timeouts failed")
    return n
