"""Host-side mirror of the reference's ``quant/quant_layer.py`` operator interface, executing on MI355X.

Same public names and argument meaning (``Scaler``, ``UniformAffineQuantizer``, ``QuantLayer``, ``QMODE``,
``StraightThrough``), different execution model:

  reference (quant_layer.py:626-661)                      here
  ---------------------------------------------------    -----------------------------------------------------
  fake-quant weights from fp32 on EVERY call (:642-643)   integer codes frozen once -> int4/int8 packed in HBM
  F.unfold materialises im2col in fp32 (:630-638)         gather + quantise straight to int8 codes (dgq_quant_act)
  6 elementwise fp passes per activation (:297-299)       fused into that single pre-pass
  fp32 F.linear / matmul / F.conv2d (:562,:659)           V_MFMA_I32_16X16X64_I8 GEMM, dequant in the epilogue
  ~750 host->device δ/z copies per step when time-aware   all timestep slots resident on the device

There is no CPU execution path: a quantized forward on a CPU tensor raises.
"""
import logging
import os
from enum import Enum
from typing import List, Optional, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..plan import plan_act

logger = logging.getLogger(__name__)


class StraightThrough(nn.Module):
    def forward(self, x):
        return x


def minmax(x: torch.Tensor, symmetric: bool = False, level: int = 256, always_zero: bool = False):
    """Scalar min/max scale initialiser — same arithmetic as quant_layer.py:22-38 (python-double range,
    δ clamped to ≥1e-8, z = rne(−min/δ))."""
    x_min, x_max = min(x.min().item(), 0.0), max(x.max().item(), 0.0)
    delta = torch.tensor(float(x_max - x_min) / (level - 1))
    if symmetric:
        m = max(abs(x_min), x_max)
        x_min, x_max = -m, m
        delta = torch.tensor(float(x_max - x_min) / (level - 2))
    if always_zero:
        delta = torch.tensor(float(x_max) / (level - 1))
    if delta < 1e-8:
        delta = torch.tensor(1e-8)
    if symmetric or always_zero:
        zero_point = torch.tensor(0.0)
    else:
        zero_point = torch.round(-torch.tensor(float(x_min)) / delta)
    return delta.to(device=x.device, dtype=x.dtype), zero_point.to(device=x.device, dtype=x.dtype)


def lp_loss(pred: torch.Tensor, tgt: torch.Tensor, p: float = 2.0):
    """quant_layer.py:198-209 with reduction ALL: mean |pred − tgt|^p over every element."""
    return (pred - tgt).abs().pow(p).mean()


def channel_mse(w: torch.Tensor, level: int):
    """``mse`` for every output channel at once (asymmetric weights): what quant_layer.py:253-264 computes with a python loop of
    80 full passes per channel.  Same arithmetic per channel — ranges shrunk in double precision and rounded to fp32 once,
    z = rne(fp32(−min)/δ), error = mean |·|^2.4 — the candidates of all channels evaluated together; a channel keeps the
    FIRST candidate with the smallest error, as the reference's strict ``<`` does."""
    flat = w.detach().reshape(w.shape[0], -1).float()
    mn64, mx64 = flat.min(dim=1)[0].double(), flat.max(dim=1)[0].double()
    best = torch.full((flat.shape[0],), 1e+10, device=flat.device)
    delta = torch.zeros_like(best)
    zp = torch.zeros_like(best)
    for i in range(80):
        f = 1. - (i * 0.01)
        new_min, new_max = mn64 * f, mx64 * f
        nd = ((new_max - new_min) / (level - 1)).float()
        nz = torch.round((-new_min).float() / nd)
        x_q = torch.clamp(torch.round(flat / nd[:, None]) + nz[:, None], 0, level - 1)
        err = (nd[:, None] * (x_q - nz[:, None]) - flat).abs().pow(2.4).mean(dim=1)
        better = err < best
        best = torch.where(better, err, best)
        delta = torch.where(better, nd, delta)
        zp = torch.where(better, nz, zp)
    shape = (-1,) + (1,) * (w.dim() - 1)
    return delta.view(shape).to(w.dtype), zp.view(shape).to(w.dtype)


def mse(x: torch.Tensor, symmetric: bool = False, level: int = 256, always_zero: bool = False):
    """The scalar L2.4 range search (quant_layer.py:62-86) = ``channel_mse`` of the tensor taken as ONE channel: all 80 shrink
    candidates are ranked by the same batched evaluation; 0-d (δ, z) like the reference returns."""
    if symmetric or always_zero:
        return _mse_flagged(x, symmetric, level, always_zero)
    d, z = channel_mse(x.reshape(1, -1), level)
    return d.reshape(()), z.reshape(())


def _mse_flagged(x: torch.Tensor, symmetric: bool, level: int, always_zero: bool):
    """The same search under the quantizer flags (quant_layer.py:72-80): ``always_zero`` (the uniform softmax quantizer aqtizer_w,
    quant_block.py:145-156: δ = max/(level − 1), z = 0, codes in [0, level − 1]) and ``symmetric`` (δ = 2·max|range|/(level − 2),
    z = 0, codes in [−level/2, level/2 − 1]).  The 80 shrink candidates are evaluated eight at a time over the flattened tensor;
    the first candidate with the smallest error wins (the reference's strict ``<``)."""
    flat = x.detach().reshape(-1).float()
    x_min, x_max = float(flat.min()), float(flat.max())
    f = 1.0 - 0.01 * torch.arange(80, dtype=torch.float64)
    new_min, new_max = x_min * f, x_max * f
    if always_zero:
        deltas = (new_max / (level - 1)).float()                     # torch.tensor(python double): rounded to fp32 once
        nb, pb = 0, level - 1
    else:
        m = torch.maximum(new_min.abs(), new_max)
        deltas = (m + m) / (level - 2)                               # stays a python double in the reference: the division below
        nb, pb = -level // 2, level // 2 - 1                         # rounds it to fp32 when it meets the fp32 tensor
    deltas = deltas.to(flat.device)
    best, best_d = None, None
    for i0 in range(0, 80, 8):
        d = deltas[i0:i0 + 8].float()[:, None]
        x_q = torch.clamp(torch.round(flat[None, :] / d), nb, pb)
        err = (d * x_q - flat[None, :]).abs().pow(2.4).mean(dim=1)
        for j in range(err.numel()):
            if best is None or float(err[j]) < best:
                best, best_d = float(err[j]), deltas[i0 + j]
    delta = best_d.float() if always_zero else best_d                # (symmetric: the reference returns the python double)
    return torch.as_tensor(delta).to(dtype=x.dtype, device=x.device).reshape(()), torch.tensor(0.0, dtype=x.dtype, device=x.device)


def _outside_scope(name):
    def scaler(x, symmetric=False, level=256, always_zero=False):
        raise NotImplementedError("Scaler.%s is not selected by any DGQ recipe (SURVEY.md §2: out of scope); use MINMAX or MSE" % name)
    scaler.__name__ = name.lower()
    return scaler


class Scaler(Enum):
    """Same member names as the reference enum (quant_layer.py:187-193); the DGQ recipes select MINMAX (``--fast``) or MSE."""
    MINMAX = minmax
    MSE = mse
    KL = _outside_scope("KL")
    HIST = _outside_scope("HIST")
    OMSE = _outside_scope("OMSE")
    LOGMINMAX = _outside_scope("LOGMINMAX")


QMODE = Enum("QMODE", ("QDIFF", "NORMAL", "PTQD"))


def channel_minmax(w: torch.Tensor, level: int):
    """Vectorised per-output-channel ``minmax`` (what quant_layer.py:253-264 computes with a python loop
    over channels — the dominant cost of the reference's load)."""
    flat = w.detach().reshape(w.shape[0], -1)
    mn = torch.clamp(flat.min(dim=1)[0], max=0.0).double()
    mx = torch.clamp(flat.max(dim=1)[0], min=0.0).double()
    delta = ((mx - mn) / float(level - 1)).float()
    delta = torch.where(delta < 1e-8, torch.full_like(delta, 1e-8), delta)
    zp = torch.round(-mn.float() / delta)
    shape = (-1,) + (1,) * (w.dim() - 1)
    return delta.view(shape), zp.view(shape)


def row_minmax(row_min: torch.Tensor, row_max: torch.Tensor, level: int):
    """``minmax`` of many rows at once from their fp32 minima / maxima — the statement dgq_act_row_params reproduces bit for bit (the
    real-time activation quantizer): lo = min(row_min, 0), hi = max(row_max, 0), δ = fp32((double(hi) − double(lo)) / (level − 1)),
    fp32(1e-8) when smaller, z = rne(fp32(−lo) / δ) with an fp32 IEEE division.  Equal to the scalar ``minmax`` of each row
    (tests/test_realtime_act_cpu.py)."""
    lo = torch.clamp(row_min.float(), max=0.0)
    hi = torch.clamp(row_max.float(), min=0.0)
    delta = ((hi.double() - lo.double()) / float(level - 1)).float()
    delta = torch.where(delta < 1e-8, torch.full_like(delta, 1e-8), delta)
    zp = torch.round(-lo / delta)
    return delta, zp


#: channels per block of the real-time block mode (``real_time_block``): DGQ_KCHUNK, the depth of one mfma_i32_32x32x32_i8
REAL_TIME_BLOCK = 32


def block_minmax(blk_min: torch.Tensor, blk_max: torch.Tensor, level: int):
    """``minmax`` of many (row, 32-channel block) cells at once from their fp32 minima / maxima — ``row_minmax`` applied to block
    extrema, the statement dgq_quant_act_block reproduces bit for bit (real-time block mode).  An all-zero block (a convolution tap
    outside the image) gives δ = fp32(1e-8), z = 0: code 0, dequantised to exactly 0."""
    return row_minmax(blk_min, blk_max, level)


#: E2M3 magnitudes by 5-bit code (exponent << 3 | mantissa): subnormals m/8, then (1 + m/8)·2^(e−1)
E2M3_MAGNITUDES = tuple(m / 8.0 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 1) for e in range(4) for m in range(8))


def mx6_block(rows: torch.Tensor):
    """The MXFP6 statement dgq_quant_act_mx6 reproduces bit for bit (``real_time_format="mxfp6"``): rows [R][C] fp32 (C % 32 == 0, finite,
    behind any folded prologue), every 32 consecutive channels one block.  With amax = max |x′| of the block, E = floor(log2 amax) − 2
    — the OCP MX rule for E2M3 (emax 2), read off the exponent field of amax — clamped to [−127, 127], −127 for amax = 0; v = x′·2^−E (an
    exact scaling, |v| < 8) is rounded to nearest, ties to even, onto the E2M3 grid (steps 0.125 below 2, 0.25 below 4, 0.5 above) and
    saturates at ±7.5; a zero magnitude is the code +0.  Returns (codes uint8 [R][C] = sign << 5 | exponent << 3 | mantissa, scale uint8
    [R][C/32] = E + 127, x̂ fp32 [R][C] = value(code)·2^E)."""
    x = rows.detach().float()
    R, C = x.shape
    assert C % REAL_TIME_BLOCK == 0
    xb = x.view(R, C // REAL_TIME_BLOCK, REAL_TIME_BLOCK)
    amax = xb.abs().amax(dim=2)
    field = (amax.contiguous().view(torch.int32) >> 23) & 0xFF              # 0 for zero and subnormal amax
    E = torch.clamp(field - 129, min=-127)                                     # (finite amax: at most 125)
    inv = torch.ldexp(torch.ones_like(amax), -E)                               # 2^−E, a normal float
    v = xb * inv[:, :, None]
    a = v.abs()
    step = torch.where(a < 2.0, torch.full_like(a, 0.125), torch.where(a < 4.0, torch.full_like(a, 0.25), torch.full_like(a, 0.5)))
    q = torch.clamp(torch.round(a / step) * step, max=7.5)                     # torch.round: half to even; a / step is exact
    qe = torch.floor(torch.log2(torch.clamp(q, min=1.0))).to(torch.int32)      # 0, 1, 2 for the normal ranges (exact at powers of two)
    mag = torch.where(q < 1.0, (q * 8.0).to(torch.int32), ((qe + 1) << 3) | ((q / torch.ldexp(torch.ones_like(q), qe) - 1.0) * 8.0).to(torch.int32))
    sign = torch.where((v < 0) & (mag > 0), 32, 0).to(torch.int32)
    codes = (mag | sign).to(torch.uint8).view(R, C)
    xhat = (torch.where(v < 0, -q, q) * torch.ldexp(torch.ones_like(amax), E)[:, :, None]).view(R, C)
    return codes, (E + 127).to(torch.uint8), xhat


def mx6_pack(codes: torch.Tensor):
    """6-bit codes [R][C] (uint8) -> [R][C/32][24] bytes: element j of a block at bits 6j .. 6j + 5 of its 192-bit little-endian string
    (four codes per three bytes) — the FP6 operand image"""
    R, C = codes.shape
    c = codes.view(R, C // 4, 4).to(torch.int32)
    w = c[..., 0] | (c[..., 1] << 6) | (c[..., 2] << 12) | (c[..., 3] << 18)
    out = torch.stack([w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 0xFF], dim=-1).to(torch.uint8)
    return out.view(R, C // REAL_TIME_BLOCK, 24)


def mx6_unpack(packed: torch.Tensor):
    """inverse of ``mx6_pack``: [R][C/32][24] bytes -> codes uint8 [R][C]"""
    R = packed.shape[0]
    b = packed.reshape(R, -1, 3).to(torch.int32)
    w = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    return torch.stack([(w >> (6 * j)) & 63 for j in range(4)], dim=-1).to(torch.uint8).view(R, -1)


def group_params_from_ranges(in_min, in_max, out_min, out_max, group_num, mode, level, force_in_channel=None):
    """The host half of ``done_group_num`` (quant_layer.py:338-418) as a pure function of the folded range vectors —
    returns (δ, z, in_channel_wise) in the checkpoint's broadcast shapes.  Arithmetic follows the reference line by
    line: numpy float32 ranges -> float64 K-Means -> per-cluster range in float64 -> δ rounded to fp32 by
    ``torch.tensor`` -> z = rne(−min/δ) in fp32."""
    import os
    import numpy as np
    from sklearn.cluster import KMeans
    imin, imax = in_min.detach().cpu().numpy().flatten(), in_max.detach().cpu().numpy().flatten()
    omin, omax = out_min.detach().cpu().numpy().flatten(), out_max.detach().cpu().numpy().flatten()
    in_spread = imax.max() - imax.min() + imin.max() - imin.min()
    out_spread = omax.max() - omax.min() + omin.max() - omin.min()
    in_channel_wise = bool(in_spread > out_spread or os.environ.get("IN_CHANNEL_WISE", False))
    if force_in_channel is not None:
        in_channel_wise = force_in_channel
    data = np.column_stack((imin, imax)) if in_channel_wise else np.column_stack((omin, omax))
    km = KMeans(n_clusters=group_num, random_state=0).fit(data)
    labels = km.labels_
    if mode == "mean":
        center = km.cluster_centers_
    elif mode == "minmax":
        center = []
        for i in range(group_num):
            cl = data[labels == i]
            center.append([cl.min(), cl.max()] if cl.size else [0.0, 1.0])
        center = np.array(center)
    else:
        raise NotImplementedError(mode)
    base = (in_min if in_channel_wise else out_min).detach().clone().cpu().float().flatten()
    delta, zero_point = base.clone(), base.clone()
    lab = torch.from_numpy(labels.astype("int64"))
    for i in range(group_num):
        d = torch.tensor((center[i, 1] - center[i, 0]) / (level - 1))
        if d < 1e-8:
            d = torch.tensor(1e-8)
        d = d.float()
        delta[lab == i] = d
        zero_point[lab == i] = torch.round(torch.tensor(-center[i, 0]).float() / d)
    shape = (1, 1, -1) if in_channel_wise else (1, -1, 1)
    return delta.view(shape), zero_point.view(shape), in_channel_wise


class UniformAffineQuantizer(nn.Module):
    """δ·(clamp(rne(x/δ)+z, 0, 2^b−1) − z)  — quant_layer.py:216-299 (inference branch; the calibration branches of
    :284-293 are ``observe``).

    ``real_time=True`` (a mode of this library; the reference has it for the softmax quantizer only): no stored (δ, z) — every row
    the quantizer sees gets its own pair from ``Scaler.MINMAX`` applied to that row at run time (dgq_act_row_params; ``row_minmax``
    below is the statement).  The row of a Linear layer is a row of its [M][K] input, the row of a convolution one output position's
    row of the unfolded operand, both behind any folded prologue; an attention-side quantizer (aqtizer_q/k/v) takes one pair per
    token over batch and heads.  Needs no activation calibration; ``init_from`` is a no-op and the quantizer is always ``init``.

    ``real_time_block=32`` (with ``real_time``): a second granularity — one pair per row AND block of 32 consecutive channels
    (``block_minmax``), so an outlier sets the step of its own 32 channels only.  A convolution row has, for every tap, the C/32 blocks
    of that tap's input pixel (a tap outside the image is a block of zeros and contributes exactly 0), so its input is quantised
    once per pixel (dgq_quant_act_block + dgq_gemm_blockq).  Layers with C % 32 != 0 and the attention-side quantizers keep the
    per-row / per-token form.

    ``real_time_format="mxfp6"`` (with ``real_time_block=32`` and 6 bits): the block is an OCP MXFP6 block instead — one power-of-two
    scale and 32 FP6 E2M3 codes (``mx6_block``), the operand of the block-scaled matrix cores (dgq_quant_act_mx6 + dgq_gemm_mx6).  W4
    layers with integer zero points and C % 32 == 0 take it; every other layer runs as with ``real_time_block=32`` alone."""

    def __init__(self, bits: int = 8, symmetric: bool = False, channel_wise: bool = False,
                 scaler: Scaler = Scaler.MINMAX, leaf_param: bool = False, always_zero: bool = False,
                 quant_emb: bool = False, real_time: bool = False, real_time_block: int = 0, real_time_format: str = "int") -> None:
        super().__init__()
        if symmetric:
            raise NotImplementedError("symmetric quantizers are not used by the DGQ inference path")
        if real_time and (channel_wise or always_zero or scaler is not Scaler.MINMAX):
            raise ValueError("a real-time activation quantizer is Scaler.MINMAX per row: not channel_wise, not always_zero")
        if real_time_block not in (0, REAL_TIME_BLOCK) or (real_time_block and not real_time):
            raise ValueError("real_time_block is 0 (one pair per row) or %d (one pair per row and block of %d consecutive channels), and a "
                             "granularity of real_time=True" % (REAL_TIME_BLOCK, REAL_TIME_BLOCK))
        if real_time_format not in ("int", "mxfp6"):
            raise ValueError("real_time_format is \"int\" or \"mxfp6\", not %r" % (real_time_format,))
        if real_time_format == "mxfp6" and not (real_time and real_time_block == REAL_TIME_BLOCK and bits == 6):
            raise ValueError("real_time_format=\"mxfp6\" is a format of real_time=True with real_time_block=%d and bits=6" % REAL_TIME_BLOCK)
        self.real_time = bool(real_time)
        self.real_time_block = int(real_time_block)
        self.real_time_format = real_time_format
        self.level = 2 ** bits
        self.symmetric = symmetric
        self.channel_wise = channel_wise
        self.scaler = scaler
        self.leaf_param = leaf_param
        if leaf_param:
            self.x_min, self.x_max = None, None
        self.running_stat = False
        self.always_zero = always_zero
        self.delta = None
        self.zero_point = None
        self.init = self.real_time                 # nothing to initialise: the parameters come from each call's rows
        self.quant_emb = quant_emb
        self.group_num = -1
        # calibration producer state (quant_layer.py:247-248): one (min, max) pair of vectors per observed batch
        self.min_max_per_in_channel = []
        self.min_max_per_out_channel = []

    @property
    def bits(self):
        return int(self.level).bit_length() - 1

    # -- calibration producer (DGQ activation calibration, quant_layer.py:284-293, 301-446) ------------------------
    def calibrating(self) -> bool:
        return self.running_stat or self.group_num != -1

    def observe(self, x: torch.Tensor) -> None:
        """The statistics side of the reference's forward (quant_layer.py:284-293), called with the tensor the quantizer
        sees (the unfolded operand for grouped convs; [B,H,T,D] for the attention-side quantizers)."""
        if not self.init:
            self.init_from(x)
        if self.running_stat:
            self.act_momentum_update(x)
        if 1 < self.group_num:
            if x.dim() > 2:
                self.record_min_max_ema(x)
        elif self.group_num != -1:
            self.act_momentum_update(x)

    def record_min_max_ema(self, x: torch.Tensor, act_range_momentum: float = 0.95) -> None:
        """quant_layer.py:301-313: per-"in-channel" (last dim) and per-"out-channel" (second-to-last dim; the token /
        unfolded-row axis) minima and maxima of this batch, reduced over everything else — one pass of
        dgq_minmax_rows_cols over the tensor viewed as [rows][C] plus a fold of the batch (/head) index."""
        if x.dim() not in (3, 4):
            raise NotImplementedError("DGQ statistics are defined for 3-D (Linear / unfolded conv) and 4-D (attention) inputs")
        xc = x.detach().contiguous()
        C, T = xc.shape[-1], xc.shape[-2]
        rmin, rmax, cmin, cmax = ops.minmax_rows_cols(xc.view(-1, C))
        self.min_max_per_in_channel.append((cmin, cmax))
        self.min_max_per_out_channel.append((rmin.view(-1, T).min(dim=0)[0], rmax.view(-1, T).max(dim=0)[0]))

    def act_momentum_update(self, x: torch.Tensor, act_range_momentum: float = 0.95) -> None:
        """quant_layer.py:431-446: EMA of the scalar range, δ/z from the EMA range (the reference builds a clipped copy
        of x whose min / max ARE the EMA values and feeds it to Scaler.MINMAX; the result depends on those two only)."""
        assert self.init and self.leaf_param
        x_min, x_max = x.data.min().float(), x.data.max().float()
        self.x_min = self.x_min * act_range_momentum + x_min * (1.0 - act_range_momentum)
        self.x_max = self.x_max * act_range_momentum + x_max * (1.0 - act_range_momentum)
        rng = torch.stack([self.x_min, self.x_max]).to(x.dtype)
        delta, self.zero_point = self.scaler(rng, self.symmetric, self.level, self.always_zero)
        self.delta = nn.Parameter(delta)

    def done_group_num(self, group_num, mode):
        """quant_layer.py:315-429: fold the recorded batches (min of mins / max of maxes), pick the axis with the larger
        spread, K-Means(group_num, random_state=0) on the (min, max) pairs (host, scikit-learn like the reference), one
        (δ, z) per cluster from the cluster's range ('minmax') or centre ('mean'), broadcast shape (1,1,X) / (1,X,1)."""
        if self.min_max_per_in_channel == []:
            self.group_num = -1
            return None
        import numpy as np
        from sklearn.cluster import KMeans
        in_min = torch.stack([m[0] for m in self.min_max_per_in_channel]).min(dim=0)[0]
        in_max = torch.stack([m[1] for m in self.min_max_per_in_channel]).max(dim=0)[0]
        out_min = torch.stack([m[0] for m in self.min_max_per_out_channel]).min(dim=0)[0]
        out_max = torch.stack([m[1] for m in self.min_max_per_out_channel]).max(dim=0)[0]
        delta, zero_point, _ = group_params_from_ranges(in_min, in_max, out_min, out_max, group_num, mode, self.level)
        self.last_ranges = tuple(t.detach().cpu() for t in (in_min, in_max, out_min, out_max))    # kept for inspection / tests
        dev = in_min.device
        self.delta.data = delta.to(dev)
        self.zero_point = zero_point.to(dev)
        self.group_num = -1
        self.min_max_per_in_channel = []
        self.min_max_per_out_channel = []
        return self.delta.data, self.zero_point

    # -- initialisation -------------------------------------------------------------------------
    def _init_quantization_param(self, x: torch.Tensor, channel_wise: bool = False):
        if channel_wise:
            if self.scaler is Scaler.MINMAX:
                return channel_minmax(x, self.level)
            if self.scaler is Scaler.MSE and not self.symmetric and not self.always_zero:
                return channel_mse(x, self.level)
            # any other scaler: the reference's loop over output channels (quant_layer.py:253-264)
            dz = [self.scaler(x[c].detach(), self.symmetric, self.level, self.always_zero) for c in range(x.shape[0])]
            shape = (-1,) + (1,) * (x.dim() - 1)
            delta = torch.stack([torch.as_tensor(d, dtype=x.dtype, device=x.device).reshape(()) for d, _ in dz]).view(shape)
            zp = torch.stack([torch.as_tensor(z, dtype=x.dtype, device=x.device).reshape(()) for _, z in dz]).view(shape)
            return delta, zp
        if self.leaf_param:
            self.x_min, self.x_max = x.data.min(), x.data.max()
        return self.scaler(x, self.symmetric, self.level, self.always_zero)

    def init_from(self, x: torch.Tensor):
        if self.real_time:
            return
        delta, zp = self._init_quantization_param(x, self.channel_wise)
        self.delta = nn.Parameter(delta) if self.leaf_param else delta
        self.zero_point = zp
        self.init = True

    # -- forward --------------------------------------------------------------------------------
    def layout(self, x: torch.Tensor):
        """(x2d, mode, T, D) for dgq_fakequant_rows given this quantizer's δ shape and a contiguous x:
        scalar; (1,1,X) = last dim; (1,X,1) = second-to-last dim (token); [N,1(,1,1)] = dim 0 (weights)."""
        d = self.delta
        C = x.shape[-1]
        if d.numel() == 1:
            return x.view(-1, C), 0, 1, C
        if d.dim() == x.dim() and d.shape[0] == x.shape[0] and d.numel() == x.shape[0]:   # per output channel
            return x.view(x.shape[0], -1), 1, x.shape[0], x[0].numel()
        if d.dim() == 3 and d.shape[0] == 1 and d.shape[1] == 1 and d.shape[2] == C:
            return x.view(-1, C), 2, 1, C
        if d.dim() == 3 and d.shape[0] == 1 and d.shape[2] == 1 and x.dim() >= 2 and d.shape[1] == x.shape[-2]:
            return x.view(-1, C), 1, x.shape[-2], C
        raise NotImplementedError("quantizer δ shape %s on input %s" % (tuple(d.shape), tuple(x.shape)))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not self.init:
            self.init_from(x)
        if not x.is_cuda:
            raise RuntimeError("dgq_amd: quantizers execute on the GPU only (no CPU fallback)")
        xc = x.contiguous()
        if self.real_time:
            # stand-alone (fake-quant) form: the rows of the last dimension, their tables from dgq_act_row_params, then
            # dgq_fakequant_rows with one table entry per row.  A convolution's rows exist only inside the layer (unfolded operand).
            if x.dim() == 4 or x.shape[-1] % 4 != 0 or x.dtype not in ops.FLOAT_DTYPES:
                raise NotImplementedError("stand-alone real-time quantizer: [..., C] inputs with C % 4 == 0 (a convolution's rows are "
                                          "those of its unfolded operand: use the QuantLayer)")
            x2d = xc.view(-1, x.shape[-1])
            if self.real_time_block:
                # block form: the new quantiser's codes and {δ, β} tables, then a dequantise
                if x.shape[-1] % self.real_time_block != 0:
                    raise NotImplementedError("stand-alone real-time block quantizer: [..., C] inputs with C %% %d == 0" % self.real_time_block)
                if self.real_time_format == "mxfp6":
                    codes, scale = ops.quant_act_mx6(x2d, (x2d.shape[0], 1, 1, x2d.shape[1], 1, 1, 1, 0))
                    out = torch.empty_like(xc)
                    ops.dequant_act_mx6(codes, scale, out.view(x2d.shape))
                    return out
                codes, table, _rho = ops.quant_act_block(x2d, (x2d.shape[0], 1, 1, x2d.shape[1], 1, 1, 1, 0), self.bits)
                out = torch.empty_like(xc)
                ops.dequant_act_block(codes, table, out.view(x2d.shape))
                return out
            d, z = ops.act_row_params(x2d, (x2d.shape[0], 1, 1, x2d.shape[1], 1, 1, 1, 0), self.bits)
            out = torch.empty_like(xc)
            ops.fakequant_rows(x2d, x2d.shape[0], x2d.shape[1], 1, d, z, 0, self.bits, out=out.view(x2d.shape))
            return out
        x2d, mode, T, D = self.layout(xc)
        d = self.delta.detach().reshape(-1).float().to(x.device)
        z = torch.as_tensor(self.zero_point).detach().reshape(-1).float().to(x.device)
        if z.numel() == 1 and d.numel() > 1:
            z = z.expand_as(d).contiguous()
        out = torch.empty_like(xc)
        ops.fakequant_rows(x2d, T, D, mode, d, z, 0, self.bits, out=out.view(x2d.shape))
        return out

    def bitwidth_refactor(self, bits: int = 8) -> None:
        self.level = 2 ** bits

    def extra_repr(self) -> str:
        return "level=%d, channel_wise=%s, leaf_param=%s, always_zero=%s%s" % (
            self.level, self.channel_wise, self.leaf_param, self.always_zero,
            (", real_time=True" + (", real_time_block=%d" % self.real_time_block if self.real_time_block else "")
             + (", real_time_format=%s" % self.real_time_format if self.real_time_format != "int" else "")) if self.real_time else "")

    def half(self):
        super().half()
        if self.delta is not None and not isinstance(self.delta, nn.Parameter):
            self.delta = self.delta.half()
        if torch.is_tensor(self.zero_point) and not isinstance(self.zero_point, nn.Parameter):
            self.zero_point = self.zero_point.half()
        return self

    def float(self):
        super().float()
        if self.delta is not None and not isinstance(self.delta, nn.Parameter):
            self.delta = self.delta.float()
        if torch.is_tensor(self.zero_point) and not isinstance(self.zero_point, nn.Parameter):
            self.zero_point = self.zero_point.float()
        return self


#: Test instrumentation (tests/test_gpu_unet.py::teacher-forced checks).  When set to a callable, every call of a quantized
#: layer that runs on the integer path — the plain ``forward`` and the fused entry points the blocks use
#: (``forward_fused`` / ``forward_prenorm`` / ``forward_residual``) — reports
#: ``LAYER_TAP(layer, y, x=..., prologue=bool, residual=..., bias_rows=...)`` and continues with the tensor it returns,
#: so a test can compare every operator of the FUSED graph with the oracle and teacher-force it.  None in production.
LAYER_TAP = None
#: weight-only state on the library's own exact-fp32 kernel (dgq_conv2d_f32w); =0: F.linear / F.conv2d on the dequantised weight
WEIGHT_ONLY_HIP = True
#: ... computed from the packed W4 / W8 codes (dgq_conv2d_wq: the same bits, no fp32 copy of the weight) for every layer with N > 8;
#: False: dgq_conv2d_f32w on dequantized_weight_natural()
WEIGHT_ONLY_PACKED = True
#: ... and the FP state (unquantised layers: conv_in / conv_out of a quantized model) too, outside autograd; =0: MIOpen / rocBLAS
FP_STATE_HIP = True


def _tap(layer, y, **info):
    if LAYER_TAP is None:
        return y
    # (a tensor the tap REPLACES carries no GroupNorm partials: they describe the tensor the GEMM wrote, and the next
    # GroupNorm then takes its statistics from the replacement itself — tests/test_gpu_kernels.py pins the partials path)
    return LAYER_TAP(layer, y, **info)


class SlotRef:
    """Shared by every layer of one QuantModel: which timestep slot's activation tables are live
    (time-aware mode, calibration.py:297-312). ``None`` = use the quantizer modules' own δ/z."""

    def __init__(self):
        self.slot = None


class QuantLayer(nn.Module):
    """Drop-in for the reference's QuantLayer (quant_layer.py:577-702) around nn.Linear / nn.Conv2d."""

    QMAP = {nn.Conv2d: F.conv2d, nn.Linear: F.linear}
    #: opt-in, read at call time: where forward / forward_upsampled would run dgq_conv2d_wq, run dgq_conv2d_wq_mfma16 instead (the
    #: 16-bit matrix cores: not bit-identical to the exact route) — see takes_mfma16.  QuantModel.set_weight_only_mfma16
    #: sets it on every layer.
    weight_only_mfma16 = False
    #: opt-in beside weight_only_mfma16, read at call time: the methods that fold a layer's element-wise neighbours on the integer path
    #: (forward_prenorm, forward_residual, forward_fused, the *_tokens pair) fold them on the weight-only matrix-core route too
    #: (dgq_conv2d_wq_mfma16_fused: norm, SiLU, GEGLU, residual and time-embedding rows in the one launch) instead of
    #: running them as torch operators around dgq_conv2d_wq_mfma16 — see takes_fused.  QuantModel.set_weight_only_fused sets it.
    weight_only_fused = False

    def __init__(self, layer: Union[nn.Conv2d, nn.Linear], wq_params: dict = {}, aq_params: dict = {},
                 disable_aq: bool = False, aq_mode: List[int] = [QMODE.QDIFF.value], quant_emb: bool = False) -> None:
        super().__init__()
        self.wq_params = dict(wq_params)
        self.aq_params = dict(aq_params)
        self.fwd_kwargs = {}
        self.is_conv = isinstance(layer, nn.Conv2d)
        if self.is_conv:
            if layer.groups != 1 or layer.dilation != (1, 1):
                raise NotImplementedError("grouped/dilated convolutions do not occur in the SD/SDXL UNets")
            self.fwd_kwargs = dict(stride=layer.stride, padding=layer.padding, dilation=layer.dilation,
                                   groups=layer.groups)
        self.kwd_func = self.QMAP[type(layer)]
        self.w = layer.weight
        self.original_w = self.w.data.clone()
        self.b = None
        self.original_b = None
        if layer.bias is not None:
            self.b = layer.bias
            self.original_b = self.b.data.clone()
        self.use_wq = False
        self.use_aq = False
        self.disable_aq = disable_aq
        self.aq_mode = aq_mode
        self.quant_emb = quant_emb
        self.wq_params["quant_emb"] = quant_emb
        self.wqtizer = UniformAffineQuantizer(**self.wq_params)
        self.aqtizer = UniformAffineQuantizer(**self.aq_params)
        self.split = 0
        self.act_func = StraightThrough()
        self.ignore_recon = False
        self.extra_repr = layer.extra_repr
        self.use_group_num = False
        # device-side state (not part of the state-dict)
        self._pw = None
        self._pw_key = None
        self._wdq = None
        self._wnat = None
        self._bindings = {}
        self._act_tables = {}            # slot -> (δ, z) CPU tensors from the cali_ckpt
        self._slot_ref: Optional[SlotRef] = None
        #: ff.net.0 of a GEGLU feed-forward (set by QuantBasicTransformerBlock): the packed weight keeps its rows interleaved
        #: (2i = value column i, 2i+1 = gate column i) so that dgq_gemm_wxa8's pair epilogue can form value·gelu(gate)
        self.geglu_rows = False

    # -- geometry ---------------------------------------------------------------------------------
    @property
    def in_channels(self):
        return self.w.shape[1]

    @property
    def taps(self):
        return self.w.shape[2] * self.w.shape[3] if self.is_conv else 1

    def _conv_geom(self):
        """(kh, kw, stride, pad) as the library entries take them; (1, 1, 1, 0) for a Linear layer"""
        if not self.is_conv:
            return 1, 1, 1, 0
        return self.w.shape[2], self.w.shape[3], self.fwd_kwargs["stride"][0], self.fwd_kwargs["padding"][0]

    def _plain(self) -> bool:
        """a Linear layer, or a convolution with dilation 1 and groups 1 (what the library's conv entries compute)"""
        return not self.is_conv or (tuple(self.fwd_kwargs.get("dilation", (1, 1)))[0] == 1 and self.fwd_kwargs.get("groups", 1) == 1)

    def _has_act_table(self) -> bool:
        """the activation quantizer is initialised, or the live timestep slot has a table"""
        return bool(self.aqtizer.init or (self._slot_ref is not None and self._slot_ref.slot in self._act_tables))   # (real-time: always init)

    # -- weights ------------------------------------------------------------------------------------
    def _weight_key(self):
        q = self.wqtizer
        alpha = getattr(q, "alpha", None)
        return (self.w.data_ptr(), self.w._version, str(self.w.device),
                q.delta.data_ptr() if torch.is_tensor(q.delta) else None,
                q.delta._version if torch.is_tensor(q.delta) else None,
                q.zero_point._version if torch.is_tensor(q.zero_point) else None,
                alpha._version if alpha is not None else None,
                self.b._version if self.b is not None else None)

    def packed_weight(self) -> ops.PackedWeight:
        """Freeze the weight to integer codes (once; re-done only if a parameter was modified)."""
        q = self.wqtizer
        if not q.init:
            q.init_from(self.w.data)
        key = self._weight_key()
        if self._pw is None or key != self._pw_key:
            dev = self.w.device
            w, d, z = self.w.data.float(), q.delta.data.to(dev), torch.as_tensor(q.zero_point).data.to(dev)
            alpha, b = getattr(q, "alpha", None), (self.b.data if self.b is not None else None)
            if self.geglu_rows:
                rp = self._row_perm(dev)
                w, d, z = w[rp], d.reshape(w.shape[0], -1)[rp], z.reshape(w.shape[0], -1)[rp]
                alpha = alpha.data[rp] if alpha is not None else None
                b = b[rp] if b is not None else None
            self._pw = ops.PackedWeight(w, d, z, alpha, b, q.bits, self.in_channels, self.taps)
            self._pw_key = key
            self._bindings = {}
            self._wdq = None
            self._wnat = None
        return self._pw

    def _row_perm(self, dev):
        """packed row 2i = reference row i (value half), 2i+1 = reference row i + N/2 (gate half)"""
        N = self.w.shape[0]
        return torch.stack([torch.arange(N // 2, device=dev), torch.arange(N // 2, device=dev) + N // 2], 1).flatten()

    def _row_unperm(self, dev):
        return torch.argsort(self._row_perm(dev))

    def dequantized_weight(self, dtype):
        """δ·(q − z) as a tensor: weight-only mode feeds it to the library GEMM/conv."""
        pw = self.packed_weight()
        if self._wdq is None or self._wdq.dtype != dtype:
            w = pw.alpha[:, None] * (pw.codes.float() - pw.zp_true[:, None])
            if self.geglu_rows:
                w = w[self._row_unperm(w.device)]
            w = w.view(self.w.shape)
            self._wdq = w.to(dtype)
            if self.is_conv:
                self._wdq = self._wdq.contiguous(memory_format=torch.channels_last)
        return self._wdq

    def dequantized_weight_natural(self):
        """(δ·(q − z) as fp32 [N][taps·C] with K in (tap, c) order, bias as fp32 or None) — the operands of dgq_conv2d_f32w."""
        self.packed_weight()                              # (re-packs, and drops the caches below, when the weight state changed)
        if self._wnat is None:
            w = self.dequantized_weight(torch.float32).float()
            if self.is_conv:
                w = w.permute(0, 2, 3, 1)                    # [N][kh][kw][C]
            self._wnat = (w.reshape(w.shape[0], -1).contiguous(), self.b.float().contiguous() if self.b is not None else None)
        return self._wnat

    # -- activation tables ----------------------------------------------------------------------------
    def set_act_table(self, slot, delta, zero_point):
        self._act_tables[slot] = (delta, zero_point)
        self._bindings.pop(slot, None)

    def _binding(self) -> ops.ActBinding:
        pw = self.packed_weight()
        if self.aqtizer.real_time:                # no tables, no slots: one natural-order binding, its row tables made per call
            if "real_time" not in self._bindings:
                # block granularity where the input channels split into whole 32-blocks; the per-row mode otherwise
                # (MXFP6 blocks where the format asks for them and the weight is exact in E2M3)
                blk = self.aqtizer.real_time_block
                whole = blk and self.in_channels % blk == 0
                if whole and self.aqtizer.real_time_format == "mxfp6" and pw.mx6_eligible:
                    self._bindings["real_time"] = ops.MxActBinding(pw)
                else:
                    self._bindings["real_time"] = (ops.BlockActBinding(pw, self.aqtizer.bits) if whole
                                                   else ops.DynamicActBinding(pw, self.aqtizer.bits))
            return self._bindings["real_time"]
        slot = self._slot_ref.slot if self._slot_ref is not None else None
        if slot is not None and slot in self._act_tables:
            key = slot
            if key not in self._bindings:
                d, z = self._act_tables[slot]
                lay = plan_act(d, z, "conv" if self.is_conv else "linear", self.in_channels, self.taps, self.aqtizer.bits,
                               kw=self.w.shape[3] if self.is_conv else 1)
                self._bindings[key] = ops.ActBinding(lay, pw, self.aqtizer.bits)
            return self._bindings[key]
        a = self.aqtizer
        d = a.delta
        z = torch.as_tensor(a.zero_point)
        key = ("live", d.data_ptr(), d._version, z.data_ptr() if z.numel() else 0, z._version)
        if key not in self._bindings:
            self._bindings = {k: v for k, v in self._bindings.items() if not (isinstance(k, tuple) and k[0] == "live")}
            lay = plan_act(d.data, z.data, "conv" if self.is_conv else "linear", self.in_channels, self.taps, a.bits,
                           kw=self.w.shape[3] if self.is_conv else 1)
            self._bindings[key] = ops.ActBinding(lay, pw, a.bits)
        return self._bindings[key]

    # -- forward ----------------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor, split: int = 0) -> torch.Tensor:
        quant_act = self.use_aq and not self.disable_aq
        if not self.use_wq:
            w = self.original_w.to(device=x.device, dtype=x.dtype)
            b = self.original_b.to(device=x.device, dtype=x.dtype) if self.original_b is not None else None
            if quant_act:
                x = self.aqtizer(x)
            if (FP_STATE_HIP and x.is_cuda and x.dtype in ops.FLOAT_DTYPES and not torch.is_grad_enabled() and self._plain()):
                # FP state on the GPU without autograd (conv_in / conv_out of every quantized model, quant_model.py:66-73): the
                # library's exact-fp32 kernel instead of MIOpen / rocBLAS (conv_out's four output channels take its N <= 8 form;
                # step 9.537 vs 9.559 ms with MIOpen)
                self._fp_natural(x.device)
                # (gn_out: conv_in's output carries its GroupNorm partials on this path too — with or without an output redirect
                # the first resnet's norm1 and the last up resnet's see the same statistics)
                return ops.conv2d_f32w(x, self._wnat_fp[1], self._wnat_fp[2], *self._conv_geom(), gn_out=self.is_conv)
            if self.is_conv:
                return F.conv2d(x, w, b, stride=self.fwd_kwargs["stride"], padding=self.fwd_kwargs["padding"])
            return F.linear(x, w, b)
        if not x.is_cuda:
            raise RuntimeError("dgq_amd.QuantLayer: the quantized path runs only through the HIP kernels on the GPU "
                               "(no CPU fallback); got a %s tensor" % x.device)
        if not quant_act:
            if getattr(self.wqtizer, "soft_tgt", False):
                # weight reconstruction in progress (reconstruction.py:37-41): the differentiable soft-rounded weight,
                # re-evaluated every call like the reference's wqtizer(self.w) (quant_layer.py:642-643)
                if not self.wqtizer.init:
                    self.wqtizer.init_from(self.w.data)
                w = self.wqtizer(self.w)
                if self.is_conv:
                    w = w.contiguous(memory_format=torch.channels_last)
            else:
                # inference in the weight-only state: exact-fp32 MFMA kernel of this library, not F.linear / F.conv2d of the
                # vendor libraries — from the packed codes (dgq_conv2d_wq), or on the dequantised fp32 weight (dgq_conv2d_f32w)
                if self.on_packed_weight_only_path(x):
                    return self._weight_only_op()(x, self.packed_weight(), *self._conv_geom(), geglu_rows=self.geglu_rows)
                if self._weight_only_hip(x):
                    return ops.conv2d_f32w(x, *self.dequantized_weight_natural(), *self._conv_geom())
                w = self.dequantized_weight(x.dtype)
            b = self.b.to(x.dtype) if self.b is not None else None
            if self.is_conv:
                return F.conv2d(x, w, b, stride=self.fwd_kwargs["stride"], padding=self.fwd_kwargs["padding"])
            return F.linear(x, w, b)
        if not self._has_act_table():
            self.aqtizer.init_from(x)           # first-forward self-initialisation (quant_layer.py:274-278)
        if self.aqtizer.calibrating():          # DGQ calibration: statistics of what the quantizer sees (:284-293, :630-641)
            seen = x
            if self.is_conv and self.use_group_num:
                seen = F.unfold(x, kernel_size=tuple(self.w.shape[2:]), dilation=1, padding=self.fwd_kwargs["padding"][0],
                                stride=self.fwd_kwargs["stride"][0])
            self.aqtizer.observe(seen)
        ab = self._binding()
        if self.is_conv:
            return _tap(self, ops.quant_conv2d(x, ab, *self._conv_geom()), x=x, prologue=False)
        y = ops.quant_linear(x, ab)
        if self.geglu_rows:                     # the plain path returns the reference's column order
            y = y.index_select(-1, self._row_unperm(y.device))
        return _tap(self, y, x=x, prologue=False)

    def _take_redirect(self, x: torch.Tensor, scale: int = 1):
        """(out, out2) of a pending ops.OutputRedirect for this convolution's output on input x (spatially scaled by ``scale``), or
        (None, None): asked only by the calls whose result IS their module's result (``final=True``)."""
        if ops.pending_redirect() is None or not self.is_conv or x.dim() != 4:
            return None, None
        kh, kw, st, pd = self._conv_geom()
        Ho = (x.shape[2] * scale + 2 * pd - kh) // st + 1
        Wo = (x.shape[3] * scale + 2 * pd - kw) // st + 1
        return ops.take_redirect(x.shape[0] * Ho * Wo, self.w.shape[0], x.dtype)

    def forward_final(self, x: torch.Tensor) -> torch.Tensor:
        """``self(x)`` where the result is the calling module's own result (Downsample2D.conv, the UNet's conv_in): the one place a
        pending ops.OutputRedirect is honoured on the plain path — integer path or FP state of a convolution, no tap, no hooks."""
        if (ops.pending_redirect() is not None and self.is_conv and x.is_cuda and x.dtype in ops.FLOAT_DTYPES and LAYER_TAP is None and not self.aqtizer.calibrating()
                and not self._forward_hooks and not self._forward_pre_hooks and not torch.is_grad_enabled()):
            if self.on_integer_path(x):
                out, out2 = self._take_redirect(x)
                return ops.quant_conv2d(x, self._binding(), *self._conv_geom(), out=out, out2=out2)
            if (not self.use_wq and not (self.use_aq and not self.disable_aq) and FP_STATE_HIP and self._plain()):
                out, out2 = self._take_redirect(x)
                if out is None:                                   # (the FP kernel takes the second copy only)
                    self._fp_natural(x.device)
                    return ops.conv2d_f32w(x, self._wnat_fp[1], self._wnat_fp[2], *self._conv_geom(), out2=out2, gn_out=True)
                ops.pending_redirect().taken = False
        return self(x)

    def forward_upsampled(self, x: torch.Tensor, final: bool = False) -> torch.Tensor:
        """``self(F.interpolate(x, scale_factor=2.0, mode="nearest"))`` — Upsample2D.forward (diffusers_rewrite/sd.py).  On the integer
        path of a k x k convolution the quantise-on-load pass reads x through the (h/2, w/2) mapping and the upsampled tensor is
        never written (ops.quant_conv2d(upsample=True)); with a layer tap installed, during calibration or in any other state the
        interpolate runs as written.  In the weight-only state the packed-code kernel reads x through the same mapping
        (ops.conv2d_wq(upsample=True)), under the same conditions."""
        if (LAYER_TAP is None and self.is_conv and self.on_packed_weight_only_path(x) and not self.aqtizer.calibrating()
                and not self._forward_hooks and not self._forward_pre_hooks):
            return self._weight_only_op()(x, self.packed_weight(), *self._conv_geom(), upsample=True)
        if (LAYER_TAP is None and self.is_conv and self.on_integer_path(x) and x.dtype in ops.FLOAT_DTYPES and not self.aqtizer.calibrating()
                and not self._forward_hooks and not self._forward_pre_hooks and self.taps > 1):
            out, out2 = self._take_redirect(x, 2) if final else (None, None)
            return ops.quant_conv2d(x, self._binding(), *self._conv_geom(), upsample=True, out=out, out2=out2)
        return self(F.interpolate(x, scale_factor=2.0, mode="nearest"))

    def on_packed_weight_only_path(self, x: torch.Tensor) -> bool:
        """True when forward(x) would run dgq_conv2d_wq (weight-only state from the packed codes, GPU, outside autograd)."""
        return (WEIGHT_ONLY_PACKED and self.use_wq and not (self.use_aq and not self.disable_aq) and x.is_cuda
                and not getattr(self.wqtizer, "soft_tgt", False) and self.w.shape[0] > 8 and self._weight_only_hip(x))

    def takes_mfma16(self) -> bool:
        """True when a call on the packed weight-only path runs dgq_conv2d_wq_mfma16 instead of dgq_conv2d_wq: the switch is set and
        the weight is eligible (PackedWeight.mfma16_eligible: integral zero points, q − z within the operand's exact range; a weight
        that is not stays on the exact route).  There is no rule on the shape: every row of profiles/r13_weight_only_mfma16.txt is
        faster on the new kernel, the M = batch time-embedding layers (time_embedding, time_emb_proj) included, so they take it too."""
        return self.weight_only_mfma16 and self.packed_weight().mfma16_eligible()

    def _weight_only_op(self):
        return ops.conv2d_wq_mfma16 if self.takes_mfma16() else ops.conv2d_wq

    def takes_fused(self, x: torch.Tensor) -> bool:
        """True when the folding methods run dgq_conv2d_wq_mfma16_fused on x: the switch is set, the call is on the packed weight-only
        path and takes the matrix-core entry, and nothing has to see the un-fused pieces (no layer tap, no hooks, no calibration —
        the conditions of forward_upsampled; autograd is excluded by the packed path itself)."""
        return (self.weight_only_fused and LAYER_TAP is None and self.on_packed_weight_only_path(x) and self.takes_mfma16()
                and not self.aqtizer.calibrating() and not self._forward_hooks and not self._forward_pre_hooks)

    def _fused(self, x, **kw):
        return ops.conv2d_wq_mfma16_fused(x, self.packed_weight(), *self._conv_geom(), geglu_rows=self.geglu_rows, **kw)

    def _weight_only_hip(self, x: torch.Tensor) -> bool:
        """what the weight-only state asks of x and of the layer before it leaves F.conv2d / F.linear for this library's kernels"""
        return WEIGHT_ONLY_HIP and x.dtype in ops.FLOAT_DTYPES and not (torch.is_grad_enabled() and x.requires_grad) and self._plain()

    def on_integer_path(self, x: torch.Tensor) -> bool:
        """True when forward(x) would run dgq_quant_act + dgq_gemm_wxa8 (weights and activations quantised, GPU)."""
        return self.use_wq and self.use_aq and not self.disable_aq and x.is_cuda and self._has_act_table()

    def forward_fused(self, x: torch.Tensor, pre_act: int = 0, residual=None, fq=None, ln=None, geglu: bool = False, ln_stats=None) -> torch.Tensor:
        """``fq(self(act(x))) + residual`` with the elementwise pieces folded into the two kernels of the layer:
        pre_act 1 = SiLU(x), 2 = GEGLU (x[..., :K]·gelu(x[..., K:])) inside the quantise-on-load pass; ``fq`` (an
        attention-side quantizer, see ops.make_extra) and ``residual`` inside the GEMM epilogue.  Linear layers on the
        integer path only; anything else falls back to the unfused sequence of the same kernels/ops.  ``ln`` = an
        nn.LayerNorm module applied to x first, folded into the same load pass (per-row statistics in the kernel).
        ``geglu``: the layer is the GEGLU projection ff.net.0 and the result is value·gelu(gate), [..., N/2] — formed in the
        GEMM epilogue when the packed rows are interleaved (``geglu_rows``).
        On the weight-only matrix-core route with ``weight_only_fused`` (takes_fused) a Linear layer folds ln, SiLU, the residual and
        the GEGLU into its one launch; ``ln_stats``: the rows' (mean, rstd) where the caller already has them
        (ops.layernorm_row_stats; PreLN shares one launch among the consumers of a normalised tensor)."""
        if (not self.is_conv and fq is None and pre_act in (0, 1) and self.takes_fused(x)
                and (ln is None or (not pre_act and ops.layernorm_row_stats_ok(x.shape[-1])))):
            lnp = None
            if ln is not None:
                st = ln_stats if ln_stats is not None else ops.layernorm_row_stats(x.reshape(-1, x.shape[-1]).contiguous(), float(ln.eps))
                lnp = (st, ln.weight, ln.bias)
            if geglu and not self.geglu_rows:                     # rows not interleaved: GEGLU as its own step
                a, g = self._fused(x, ln=lnp, pre_act=pre_act).chunk(2, dim=-1)
                y = a * F.gelu(g)
                return y if residual is None else y + residual
            if geglu and residual is not None:                    # (no caller asks for both: the kernel's GEGLU epilogue takes no residual)
                return self._fused(x, ln=lnp, pre_act=pre_act, geglu=True) + residual
            return self._fused(x, ln=lnp, pre_act=pre_act, residual=residual, geglu=geglu)
        if ln is not None and (self.is_conv or not self.on_integer_path(x) or x.dtype not in ops.FLOAT_DTYPES or pre_act
                               or x.shape[-1] % 4 or x.shape[-1] > 2048):
            x = ln(x)                                           # nn.LayerNorm module: unfused
            ln = None
        if self.is_conv or not self.on_integer_path(x) or x.dtype not in ops.FLOAT_DTYPES:
            if pre_act == 1:
                x = F.silu(x)
            elif pre_act == 2:
                a, g = x.chunk(2, dim=-1)
                x = a * F.gelu(g)
            y = self(x)                                           # through __call__: forward hooks (data_utill.py) see it
            if geglu:
                a, g = y.chunk(2, dim=-1)
                y = a * F.gelu(g)
            if fq is not None:
                mode, dd, zz, T, D, skip, bits = fq
                y = y.contiguous()
                ops.fakequant_rows(y.view(-1, y.shape[-1]), T, D, mode - 1, dd, zz, skip, bits)
            return y if residual is None else y + residual
        lnp = (ln.weight, ln.bias, float(ln.eps)) if ln is not None else None
        if geglu and not self.geglu_rows:                         # rows not interleaved: GEGLU as its own step
            y = self.forward_fused(x, pre_act=pre_act, ln=ln)
            a, g = y.chunk(2, dim=-1)
            return a * F.gelu(g)
        return _tap(self, ops.quant_linear(x, self._binding(), pre_act=pre_act, residual=residual, fq=fq, ln=lnp, geglu=geglu),
                    x=x, prologue=bool(pre_act or lnp is not None), residual=residual, fq=fq, geglu=geglu)

    def can_fuse_prenorm(self, x: torch.Tensor) -> bool:
        """True when this layer runs on the integer path, so a preceding GroupNorm(+SiLU) can be folded into its
        quantise-on-load pass (dgq_groupnorm_scale_shift + dgq_quant_act prologue) — or on the weight-only matrix-core route with
        ``weight_only_fused``, where it folds into that kernel's load (takes_fused)."""
        return self.is_conv and x.dtype in ops.FLOAT_DTYPES and (self.on_integer_path(x) or self.takes_fused(x))

    def forward_prenorm(self, x: torch.Tensor, norm: nn.GroupNorm, silu: bool = True, residual=None, bias_rows=None, final: bool = False) -> torch.Tensor:
        """conv(act(GroupNorm(x))) [+ residual | + bias_rows[b, :, None, None]] without materialising the normalised tensor.
        final: the result is the calling module's own result (a pending ops.OutputRedirect may place it; not on the weight-only route)."""
        if self.takes_fused(x):                                   # the weight-only matrix-core route
            return self._fused(x, norm=(norm.num_groups, norm.eps, norm.weight, norm.bias, 1 if silu else 0), residual=residual, bias_rows=bias_rows)
        ab = self._binding()
        out, out2 = self._take_redirect(x) if (final and LAYER_TAP is None) else (None, None)
        return _tap(self, ops.quant_conv2d(x, ab, *self._conv_geom(),
                                           norm=(norm.num_groups, norm.eps, norm.weight, norm.bias, 1 if silu else 0),
                                           residual=residual, bias_rows=bias_rows, out=out, out2=out2),
                    x=x, prologue=True, residual=residual, bias_rows=bias_rows)

    # -- Linear projections of a Transformer2D with use_linear_projection (SDXL, sdxl.py: proj_in / proj_out are nn.Linear over the
    #    channels of an NCHW tensor): on the integer path they are 1x1 convolutions of the channels-last tensor, so the
    #    GroupNorm in front of proj_in folds into its quantise-on-load pass, the residual behind proj_out into its GEMM epilogue,
    #    and proj_out leaves GroupNorm partials for the next resnet block — as the Conv2d projections of SD do.
    def can_fuse_tokens(self, x: torch.Tensor) -> bool:
        return not self.is_conv and self.w.dim() == 2 and x.dtype in ops.FLOAT_DTYPES and (self.on_integer_path(x) or self.takes_fused(x))

    def forward_prenorm_tokens(self, x: torch.Tensor, norm: nn.GroupNorm) -> torch.Tensor:
        """Linear(GroupNorm(x).permute(0, 2, 3, 1).reshape(B, HW, C)) for x [B, C, H, W] -> [B, HW, N]."""
        if self.takes_fused(x):                                   # the weight-only matrix-core route
            y = self._fused(x, norm=(norm.num_groups, norm.eps, norm.weight, norm.bias, 0))
            b, n, hh, ww = y.shape
            return y.permute(0, 2, 3, 1).reshape(b, hh * ww, n)
        y = ops.quant_conv2d(x, self._binding(), 1, 1, 1, 0, norm=(norm.num_groups, norm.eps, norm.weight, norm.bias, 0), gn_out=False)
        b, n, hh, ww = y.shape
        return _tap(self, y.permute(0, 2, 3, 1).reshape(b, hh * ww, n), x=x, prologue=True)

    def forward_residual_tokens(self, h: torch.Tensor, residual: torch.Tensor, final: bool = False) -> torch.Tensor:
        """Linear(h).reshape(B, H, W, N).permute(0, 3, 1, 2) + residual for tokens h [B, HW, C] and residual [B, N, H, W].
        final: the result is the calling module's own result (a pending ops.OutputRedirect may place it)."""
        b, n, hh, ww = residual.shape
        x = h.reshape(b, hh, ww, h.shape[-1]).permute(0, 3, 1, 2)
        if self.takes_fused(h):                                   # the weight-only matrix-core route
            return self._fused(x, residual=residual)
        o1, o2 = ops.take_redirect(b * hh * ww, n, x.dtype) if (final and LAYER_TAP is None) else (None, None)
        y = ops.quant_conv2d(x, self._binding(), 1, 1, 1, 0, residual=residual, out=o1, out2=o2)
        yt = y.permute(0, 2, 3, 1).reshape(b, hh * ww, n)
        rt = residual.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1).reshape(b, hh * ww, n)
        out = _tap(self, yt, x=h, prologue=False, residual=rt)
        if out is yt:
            return y                                        # (keeps the GroupNorm partials attached by quant_conv2d)
        return out.reshape(b, hh, ww, n).permute(0, 3, 1, 2)

    def can_fuse_prenorm_fp(self, x: torch.Tensor) -> bool:
        """FP-state conv on the GPU outside autograd (conv_out of a quantized model): GroupNorm + SiLU fold into the load of
        dgq_conv2d_f32w."""
        return (FP_STATE_HIP and self.is_conv and not self.use_wq and not (self.use_aq and not self.disable_aq) and x.is_cuda
                and not self._forward_hooks and not self._forward_pre_hooks     # (data capture hooks must see a plain call)
                and x.dtype in ops.FLOAT_DTYPES and not torch.is_grad_enabled() and self._plain())

    def forward_prenorm_fp(self, x: torch.Tensor, norm: nn.GroupNorm, silu: bool = True) -> torch.Tensor:
        wn, bn = self._fp_natural(x.device)
        return ops.conv2d_f32w(x, wn, bn, *self._conv_geom(), norm=(norm.num_groups, norm.eps, norm.weight, norm.bias, 1 if silu else 0))

    def _fp_natural(self, device):
        key = (self.original_w.data_ptr(), self.original_w._version, str(device))
        if getattr(self, "_wnat_fp", None) is None or self._wnat_fp[0] != key:
            wf = self.original_w.detach().to(device=device, dtype=torch.float32)
            if self.is_conv:
                wf = wf.permute(0, 2, 3, 1)
            bf = self.original_b.detach().to(device=device, dtype=torch.float32).contiguous() if self.original_b is not None else None
            self._wnat_fp = (key, wf.reshape(wf.shape[0], -1).contiguous(), bf)
        return self._wnat_fp[1], self._wnat_fp[2]

    def forward_residual(self, x: torch.Tensor, residual, final: bool = False) -> torch.Tensor:
        """conv(x) + residual with the add in the GEMM epilogue (integer path), else unfused.
        final: the result is the calling module's own result (a pending ops.OutputRedirect may place it)."""
        if self.is_conv and self.on_integer_path(x) and x.dtype in ops.FLOAT_DTYPES:
            out, out2 = self._take_redirect(x) if (final and LAYER_TAP is None) else (None, None)
            return _tap(self, ops.quant_conv2d(x, self._binding(), *self._conv_geom(), residual=residual, out=out, out2=out2),
                        x=x, prologue=False, residual=residual)
        if self.takes_fused(x):                                   # weight-only matrix-core route: the add in that kernel's epilogue
            return self._fused(x, residual=residual)
        return self(x) + residual

    # -- state switches (quant_layer.py:663-686) -----------------------------------------------------------
    def set_quant_state(self, use_wq: bool = False, use_aq: bool = False) -> None:
        self.use_wq = use_wq if not self.ignore_recon else False
        self.use_aq = use_aq if not self.ignore_recon else False

    def set_running_stat(self, running_stat: bool) -> None:
        self.aqtizer.running_stat = running_stat

    def set_group_num(self, group_num: int = 1) -> None:
        """quant_layer.py:604-608: start collecting DGQ statistics; convs switch to the unfolded-operand semantics."""
        self.aqtizer.group_num = group_num
        self.use_group_num = True

    def done_group_num(self, group_num, mode) -> None:
        self.aqtizer.done_group_num(group_num, mode)
        self._bindings = {}

    def half(self):
        super().half()
        self.original_w = self.original_w.half()
        if self.original_b is not None:
            self.original_b = self.original_b.half()
        return self

    def float(self):
        super().float()
        self.original_w = self.original_w.float()
        if self.original_b is not None:
            self.original_b = self.original_b.float()
        return self

    def _apply(self, fn, *a, **k):
        super()._apply(fn, *a, **k)
        self.original_w = fn(self.original_w)
        if self.original_b is not None:
            self.original_b = fn(self.original_b)
        return self
