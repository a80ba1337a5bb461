"""CPU side of tests/test_gpu_attention_mfma16_fp32.py: the float64 reference of un-quantised attention on fp32 tensors with the
a-priori bound of dgq_attention_mfma16_f32, a plain torch restatement of that kernel's statement (two-term bf16 splits; any single
cross term can be left out, to show that the bound notices), and the exact-data constructions.  Cases, layout and helpers are those of
tests/attention_mfma16_ref.py; everything here runs on the CPU."""
import functools
import math

import torch

from tests import attention_mfma16_ref as ar

TERMS = ("q_lo*k_hi", "q_hi*k_lo", "p_lo*v_hi", "p_hi*v_lo")


def split(x):
    """hi = bf16_rn(x), lo = bf16_rn(x − hi) as fp32 tensors (x − hi is exact in fp32)"""
    hi = x.to(torch.bfloat16).float()
    return hi, (x - hi).to(torch.bfloat16).float()


def ref64(q, k, v, H, D, scale):
    """(o64, A, G) in the layout of o: float64 softmax attention on the given fp32 values, A = Σ_j p_j·|v_j| per element and
    G = |scale|·max_j Σ_d |q_d·k_{j,d}| per query row (broadcast over the head dim)"""
    qh, kh, vh = (ar.heads(x.double(), H, D) for x in (q, k, v))
    p = torch.softmax(torch.matmul(qh, kh.transpose(-2, -1)) * scale, dim=-1)
    o = torch.matmul(p, vh)
    A = torch.matmul(p, vh.abs())
    G = abs(scale) * torch.matmul(qh.abs(), kh.abs().transpose(-2, -1)).amax(-1, keepdim=True)
    back = lambda x: x.transpose(1, 2).reshape(q.shape[0], q.shape[1], -1)
    return back(o), back(A), back(G.expand_as(o))


def bound(o64, A, G, D):
    """|o − o64| <= (2E + 2^-15)·A + 2^-24·|o64|, E = (3·2^-18 + 3·D·2^-24)·G: the two truncations and the dropped lo·lo of a score
    product (3·2^-18), the fp32 accumulation of 3D products (3·D·2^-24), that score error shifted into p and into l (2E), the split
    of p and v (2^-16) plus exp / rescales / fp32 sums (2^-16), the final division (2^-24)"""
    E = (3 * 2.0 ** -18 + 3 * D * 2.0 ** -24) * G
    return (2 * E + 2.0 ** -15) * A + 2.0 ** -24 * o64.abs()


def worst_ratio(o, o64, A, G, D):
    return float(((o.double() - o64).abs() / bound(o64, A, G, D).clamp_min(1e-300)).max())


def restatement(q, k, v, H, D, scale, tile=32, omit=None):
    """the statement of dgq_attention_mfma16_f32 in plain torch: split operands (their products are exact in fp32), fp32 sums with the
    small terms first, online softmax over 32-key tiles, l sums the unrounded p, an fp32 division at the end.  omit: one of TERMS,
    left out of its sum."""
    assert omit is None or omit in TERMS
    qh, kh, vh = (ar.heads(x.float(), H, D) for x in (q, k, v))
    (q_hi, q_lo), (k_hi, k_lo), (v_hi, v_lo) = split(qh), split(kh), split(vh)
    Bn, _, T, _ = qh.shape
    S = kh.shape[2]
    zero = lambda a, b: torch.zeros(a.shape[:-1] + b.shape[-1:])
    mm = lambda name, a, b: zero(a, b) if omit == name else torch.matmul(a, b)
    m = torch.full((Bn, H, T, 1), -math.inf)
    l = torch.zeros(Bn, H, T, 1)
    acc = torch.zeros(Bn, H, T, D)
    for s0 in range(0, S, tile):
        sl = slice(s0, s0 + tile)
        kth, ktl = k_hi[:, :, sl].transpose(-2, -1), k_lo[:, :, sl].transpose(-2, -1)
        s = (mm("q_lo*k_hi", q_lo, kth) + mm("q_hi*k_lo", q_hi, ktl) + torch.matmul(q_hi, kth)) * scale
        mn = torch.maximum(m, s.amax(-1, keepdim=True))
        alpha = torch.exp(m - mn)
        p = torch.exp(s - mn)
        p_hi, p_lo = split(p)
        l = l * alpha + p.sum(-1, keepdim=True)
        acc = acc * alpha + (mm("p_lo*v_hi", p_lo, v_hi[:, :, sl]) + mm("p_hi*v_lo", p_hi, v_lo[:, :, sl]) + torch.matmul(p_hi, v_hi[:, :, sl]))
        m = mn
    return (acc / l).transpose(1, 2).reshape(Bn, T, H * D)


@functools.lru_cache(maxsize=None)
def random_case(case, qmul, Bn=ar.B):
    """the fp32 tensors of ar.random_case (q, k ~ N(0, 1), q times qmul, v ~ 1.3·N(0, 1) + 0.2, NOT rounded to 16 bits) with the
    float64 reference and the bound's terms: (q, k, v, scale, o64, A, G), computed once per (case, variant) and shared by the CPU and
    the GPU test — do not modify the tensors"""
    D, T, S, H = case
    g = torch.Generator().manual_seed(1000 * D + T + S + H + int(qmul))
    q = torch.randn(Bn, T, H * D, generator=g) * qmul
    k = torch.randn(Bn, S, H * D, generator=g)
    v = 1.3 * torch.randn(Bn, S, H * D, generator=g) + 0.2
    scale = D ** -0.5
    return (q, k, v, scale) + ref64(q, k, v, H, D, scale)


def onehot_case(case, Bn=ar.B):
    """(q, k, v, scale, expected): the one-hot geometry of ar.onehot_case in fp32 (q = ±128 and k = ±1 are exact in bf16, their lo
    terms are zero) with v = m·2^-8, integer |m| < 2^15: 16 significant bits, so v_hi + v_lo == v and o[b,t,h] = v[b,π(t),h] exactly"""
    D, T, S, H = case
    q, k, _, scale, _ = ar.onehot_case(case, torch.float32, Bn)
    m = torch.randint(-(2 ** 15) + 1, 2 ** 15, (Bn, S, H, D), generator=torch.Generator().manual_seed(S + D))
    v = m.float() * 2.0 ** -8
    want = torch.gather(v, 1, ar.perm(case, Bn).unsqueeze(-1).expand(Bn, T, H, D))
    flat = lambda x: x.reshape(x.shape[0], x.shape[1], H * D).contiguous()
    return q, k, flat(v), scale, flat(want)


def uniform_case(case, Bn=ar.B):
    """ar.uniform_case in fp32: q = 0, every real key has probability 1/S, the values are small integers: acc = S·c_d and l = S
    exactly, so o = c_d exactly under an IEEE division (a multiplication by 1/S does not give it)"""
    return ar.uniform_case(case, torch.float32, Bn)
