"""CPU side of tests/test_gpu_attention_mfma16.py: the float64 reference of un-quantised attention with the a-priori bound of
dgq_attention_mfma16, a plain torch restatement of that kernel's statement, and the exact-data constructions.  Everything here runs
on the CPU; tensors are in the projection layout q [B][T][H·D], k / v [B][S][H·D]."""
import functools
import math

import torch

U = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -11}
DTYPES = [torch.bfloat16, torch.float16]

#: (D, T, S, H): every head dim; T and S ragged against the 128-query workgroup, the 32-query wave and the 32-key tile; S below one
#: tile, a single key past a tile (257), and many tiles with the maximum arriving late (1100)
CASES = [(8, 70, 77, 3), (16, 130, 40, 3), (40, 200, 333, 2), (64, 96, 77, 2), (80, 257, 257, 2), (160, 64, 77, 2), (40, 64, 1100, 1)]
LONG = (40, 128, 4100, 1)                    # B = 1: 129 key tiles
B = 2


def heads(x, H, D):
    """[B][N][H·D] -> [B][H][N][D]"""
    return x.view(x.shape[0], x.shape[1], H, D).transpose(1, 2)


def ref64(q, k, v, H, D, scale):
    """(o64, A, E): float64 softmax attention on the given 16-bit values in the layout of o, A = Σ_j p_j·|v_j| per element and
    E = max_j D·2^-24·scale·Σ_d |q_d·k_{j,d}| per row (broadcast over the head dim)"""
    qh, kh, vh = (heads(x.double(), H, D) for x in (q, k, v))
    p = torch.softmax(torch.matmul(qh, kh.transpose(-2, -1)) * scale, dim=-1)
    o = torch.matmul(p, vh)
    A = torch.matmul(p, vh.abs())
    E = D * 2.0 ** -24 * abs(scale) * torch.matmul(qh.abs(), kh.abs().transpose(-2, -1)).amax(-1, keepdim=True)
    back = lambda x: x.transpose(1, 2).reshape(q.shape[0], q.shape[1], -1)
    return back(o), back(A), back(E.expand_as(o))


def bound(o64, A, E, dtype):
    """|o − o64| <= (2u + 2E + 2^-16)·A + u·|o64|: one rounding of p (u·A), the normaliser (u·A; it vanishes where l sums the
    unrounded p), the fp32 accumulation of a score shifted into p and into l (2E·A), exp / rescale factors / fp32 sums of <= 2^12
    terms (2^-16·A), the final store (u·|o64|)"""
    u = U[dtype]
    return (2 * u + 2 * E + 2.0 ** -16) * A + u * o64.abs()


def worst_ratio(o, o64, A, E, dtype):
    return float(((o.double() - o64).abs() / bound(o64, A, E, dtype).clamp_min(1e-300)).max())


def restatement(q, k, v, H, D, scale, tile=32):
    """the statement of dgq_attention_mfma16 in plain torch: fp32 scores, online softmax over 32-key tiles, p rounded to the dtype
    for P·V only (l sums the unrounded p), fp32 accumulation, one rounding at the end"""
    dtype = q.dtype
    qh, kh, vh = (heads(x.float(), H, D) for x in (q, k, v))
    Bn, _, T, _ = qh.shape
    S = kh.shape[2]
    m = torch.full((Bn, H, T, 1), -math.inf)
    l = torch.zeros(Bn, H, T, 1)
    acc = torch.zeros(Bn, H, T, D)
    for s0 in range(0, S, tile):
        s = torch.matmul(qh, kh[:, :, s0:s0 + tile].transpose(-2, -1)) * scale
        mn = torch.maximum(m, s.amax(-1, keepdim=True))
        alpha = torch.exp(m - mn)
        p = torch.exp(s - mn)
        l = l * alpha + p.sum(-1, keepdim=True)
        acc = acc * alpha + torch.matmul(p.to(dtype).float(), vh[:, :, s0:s0 + tile])
        m = mn
    return (acc / l).to(dtype).transpose(1, 2).reshape(Bn, T, H * D)


@functools.lru_cache(maxsize=None)
def random_case(case, dtype, qmul, Bn=B):
    """q, k ~ N(0, 1) (q times qmul), v ~ 1.3·N(0, 1) + 0.2, rounded to the dtype, with the float64 reference and the bound's terms:
    computed once per (case, dtype, variant) and shared by the CPU and the GPU test — do not modify the tensors"""
    D, T, S, H = case
    g = torch.Generator().manual_seed(1000 * D + T + S + H + int(qmul))
    q = (torch.randn(Bn, T, H * D, generator=g) * qmul).to(dtype)
    k = torch.randn(Bn, S, H * D, generator=g).to(dtype)
    v = (1.3 * torch.randn(Bn, S, H * D, generator=g) + 0.2).to(dtype)
    scale = D ** -0.5
    return (q, k, v, scale) + ref64(q, k, v, H, D, scale)


def perm(case, Bn=B):
    """π_{b,h}(t) = (7t + 3 + 11(bH + h)) mod S as an index tensor [B][T][H]"""
    D, T, S, H = case
    t = torch.arange(T).view(1, T, 1)
    bh = (torch.arange(Bn).view(Bn, 1, 1) * H + torch.arange(H).view(1, 1, H))
    return (7 * t + 3 + 11 * bh) % S


def onehot_case(case, dtype, Bn=B):
    """(q, k, v, scale, expected): k[b,j,h,:nb] = ±1 is the binary code of j, q[b,t,h,:nb] = 128·code(π_{b,h}(t)), scale 1 — the
    matching key scores 128·nb and every other key at least 256 less, so its probability is exactly 0 and o[b,t,h] = v[b,π(t),h]"""
    D, T, S, H = case
    nb = max(1, math.ceil(math.log2(S)))
    assert nb <= D and 2 ** nb >= S
    code = lambda idx: ((idx.unsqueeze(-1) >> torch.arange(nb)) & 1).float() * 2 - 1          # [..., nb]
    k = torch.zeros(Bn, S, H, D)
    k[..., :nb] = code(torch.arange(S)).view(1, S, 1, nb)
    pi = perm(case, Bn)
    q = torch.zeros(Bn, T, H, D)
    q[..., :nb] = 128.0 * code(pi)
    v = torch.randn(Bn, S, H, D, generator=torch.Generator().manual_seed(S + D)).to(dtype)
    want = torch.gather(v, 1, pi.unsqueeze(-1).expand(Bn, T, H, D))
    flat = lambda x: x.reshape(x.shape[0], x.shape[1], H * D).to(dtype).contiguous()
    return flat(q), flat(k), flat(v), 1.0, flat(want)


def uniform_case(case, dtype, Bn=B):
    """(q, k, v, scale, expected): q = 0, so every real key has probability 1/S; v[b,j,h,d] = c_d + (−1)^j for j < 2⌊S/2⌋ and c_d for
    a last odd key, c_d small integers: every sum is exact and o = c_d exactly"""
    D, T, S, H = case
    c = ((torch.arange(D) % 7) - 3).float()
    sign = torch.where(torch.arange(S) % 2 == 0, 1.0, -1.0)
    sign[2 * (S // 2):] = 0.0
    v = (c.view(1, 1, 1, D) + sign.view(1, S, 1, 1)).expand(Bn, S, H, D)
    k = torch.randn(Bn, S, H * D, generator=torch.Generator().manual_seed(S)).to(dtype)
    q = torch.zeros(Bn, T, H * D, dtype=dtype)
    want = c.view(1, 1, 1, D).expand(Bn, T, H, D)
    flat = lambda x: x.reshape(x.shape[0], x.shape[1], H * D).to(dtype).contiguous()
    return q, k, flat(v), D ** -0.5, flat(want)
