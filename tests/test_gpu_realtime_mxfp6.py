"""Real-time MXFP6 activations on the block-scaled matrix cores (UniformAffineQuantizer(real_time=True, real_time_block=32,
real_time_format="mxfp6"): dgq_quant_act_mx6 + dgq_gemm_mx6, W4A6) — a mode of this library.

The statement the quantiser must reproduce BIT FOR BIT is ``quant_layer.mx6_block`` (== the independent float64 restatement of
tests/mxfp6_ref.py, tests/test_realtime_mxfp6_cpu.py).  The operand maps of V_MFMA_SCALE_F32_32X32X64_F8F6F4 (which lane holds which
(row, k), which scale byte goes with which K block) are pinned by one-hot operands whose output is a gather, bit for bit; layers on
planted exact data EQUAL the float64 reference; real-valued layers stay inside a per-element bound whose constant C_SUM was measured."""
import pytest
import torch
import torch.nn.functional as F

from tests import layer_reference as lr
from tests import mxfp6_ref as mx
from tests import realtime_block_ref as rb
from tests import test_gpu_groupnorm_stats as gs
from tests import test_gpu_layer_routes as routes
from tests import test_gpu_realtime_act as rta
from tests.test_gpu_realtime_act import rt_inputs, rel_l2          # noqa: F401  (module-scoped fixture of the row mode)

pytestmark = pytest.mark.gpu

#: c of the real-data bound |y − y64| <= c·K·2^-24·T + u_out·|y64|: 4 x the worst ratio |y − y64| / (K·2^-24·T) measured over
#: REAL_CASES (randn and the outlier recipe), rounded up to a power of two — profiles/r17_realtime_mxfp6.txt.  A fp32 chain gives
#: c <= 1; a wrong element, block or scale shows at about 2^24 / K.
C_SUM_MEASURED = 0.002163          # conv3x3_b2_c32_9x9_s1_n24, outlier recipe (the output rounding 2^-25·|y| dominates every case)
C_SUM = 2.0 ** -6


@pytest.fixture(scope="module")
def dev():
    from dgq_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def unpacked(got, C):
    """(codes uint8 [R][C], scale uint8 [R][lds]) on the CPU of a quant_act_mx6 result"""
    from dgq_amd.quant.quant_layer import mx6_unpack
    codes, scale = (t.cpu() for t in got)
    assert codes.dtype == torch.uint8 and codes.shape[1:] == (C // 32, 24)
    return mx6_unpack(codes), scale


def check_quantiser(got, rows, lds, what):
    """codes and scale bytes of a dgq_quant_act_mx6 launch against the statement on ``rows`` [R][C] (fp32 values), torch.equal"""
    from dgq_amd.quant.quant_layer import mx6_block
    R, C = rows.shape
    codes, scale = unpacked(got, C)
    want_c, want_s, xhat = mx6_block(rows)
    assert scale.shape == (R, lds)
    assert torch.equal(scale[:, :C // 32], want_s), "%s: scale differs at %s" % (what, (scale[:, :C // 32] != want_s).nonzero()[:4].tolist())
    assert lds == C // 32 or bool((scale[:, C // 32:] == 127).all()), "%s: the padding entries must read 127" % what
    bad = codes != want_c
    assert not bool(bad.any()), "%s: %d codes differ, first at %s: got %d, want %d" % (
        what, int(bad.sum()), bad.nonzero()[0].tolist(), int(codes[bad][0]), int(want_c[bad][0]))
    return want_c, want_s, xhat


# ----------------------------------------------------------------------------------------------- 1. the quantiser, bit exact
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=lambda d: str(d).replace("torch.", ""))
@pytest.mark.parametrize("M,K", [(154, 768), (37, 320)])
def test_quantiser_linear_bit_exact(M, K, dtype, dev):
    from dgq_amd import ops
    from dgq_amd.plan import round_up, KTILE
    g = torch.Generator().manual_seed(M * 1000 + K)
    x = rta.special_rows(torch.randn(M, K, generator=g) * 1.3 + 0.2)
    x[7, 40] = 1e4
    x[6, 32:64] = 0.0
    x = x.to(dtype)
    lds = round_up(K, KTILE) // 32
    assert lds == (24 if K == 768 else 12)                # (37, 320): Kp = 384, two padding entries
    got = ops.quant_act_mx6(x.to(dev), (M, 1, 1, K, 1, 1, 1, 0), lds=lds)
    torch.cuda.synchronize()
    _, s, _ = check_quantiser(got, x.float(), lds, "linear %dx%d %s" % (M, K, dtype))
    assert int(s[6, 1]) == 0                              # the all-zero block: E = −127


@pytest.mark.parametrize("B,C,H,W", [(2, 32, 9, 9), (2, 64, 11, 13)])
def test_quantiser_conv_input_per_pixel_bit_exact(B, C, H, W, dev):
    from dgq_amd import ops
    g = torch.Generator().manual_seed(C + H)
    x = rta.special_image(torch.randn(B, C, H, W, generator=g) * 1.3 + 0.2)
    xs = x.to(dev).contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
    got = ops.quant_act_mx6(xs, (B, H, W, C, 3, 3, 1, 1))
    torch.cuda.synchronize()
    check_quantiser(got, rb.pixel_rows(x), C // 32, "conv input %dx%dx%dx%d" % (B, C, H, W))


def test_quantiser_edge_blocks_and_dequant_bit_exact(dev):
    """the edge blocks of the CPU test (zeros, powers of two, both saturating bands, ties at every step size, −0, subnormal and huge
    amax, one 60 among randn), and dgq_dequant_act_mx6 == x̂ bit for bit in fp32 (16-bit outputs: x̂ rounded once)"""
    from dgq_amd import ops
    rows = mx.edge_blocks()
    R, C = rows.shape
    got = ops.quant_act_mx6(rows.to(dev), (R, 1, 1, C, 1, 1, 1, 0))
    torch.cuda.synchronize()
    _, _, xhat = check_quantiser(got, rows, C // 32, "edge blocks")
    y = ops.dequant_act_mx6(got[0], got[1], torch.empty(R, C, device=dev))
    assert torch.equal(y.cpu(), xhat)
    for dt in (torch.float16, torch.bfloat16):
        y16 = ops.dequant_act_mx6(got[0], got[1], torch.empty(R, C, device=dev, dtype=dt))
        assert torch.equal(y16.cpu(), xhat.to(dt))


def test_standalone_quantizer_forward(dev):
    from dgq_amd.quant.quant_layer import UniformAffineQuantizer, mx6_block
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(2 * 37, 320, generator=g) * 1.3 + 0.2).view(2, 37, 320)
    x[1, 3, 17] = 60.0
    q = UniformAffineQuantizer(bits=6, real_time=True, real_time_block=32, real_time_format="mxfp6")
    y = q(x.to(dev))
    assert torch.equal(y.cpu(), mx6_block(x.view(-1, 320))[2].view(x.shape))
    with pytest.raises(NotImplementedError):
        q(torch.zeros(1, 4, 8, 8, device=dev))


def test_quantiser_groupnorm_scale_shift_bit_exact(dev):
    """a folded GroupNorm without activation is x·scale + shift, one fp32 product and one fp32 sum: x′ is reproducible on the CPU from
    the very scale / shift rows the launch reads, and the codes are the statement's on it, bit for bit"""
    from dgq_amd import ops
    B, C, H, W = 2, 64, 6, 5
    g = torch.Generator().manual_seed(21)
    x = torch.randn(B, C, H, W, generator=g) * 1.3 + 0.2
    sc, sh = 1 + 0.3 * torch.randn(B, C, generator=g), 0.5 * torch.randn(B, C, generator=g)
    xs = x.to(dev).contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
    got = ops.quant_act_mx6(xs, (B, H, W, C, 3, 3, 1, 1), pre=(sc.to(dev), sh.to(dev), 0))
    torch.cuda.synchronize()
    xp = x * sc[:, :, None, None] + sh[:, :, None, None]
    check_quantiser(got, rb.pixel_rows(xp), C // 32, "GroupNorm scale / shift")


def check_quantiser_behind_prologue(got, rows, tol, what):
    """SiLU, GEGLU (erf) and the LayerNorm statistics are evaluated by the device's own approximations, so the kernel's x′ is the CPU's
    only to within ``tol`` [R][C] — not reproducible bit for bit off the device.  The statement is monotone in x′ under a fixed E, so the
    check that remains exact is an interval: with lo / hi the statement on x′ − tol / x′ + tol, every block whose two E agree must carry
    that E and every code's VALUE must lie in [value(lo), value(hi)]; blocks whose amax sits within tol of a power of two (the two E
    differ) may carry either E and are few."""
    R, C = rows.shape
    codes, scale = unpacked(got, C)
    (_, s_lo, x_lo), (_, s_hi, x_hi) = mx.mx6_reference(rows - tol), mx.mx6_reference(rows + tol)
    am_lo = mx.mx6_reference(torch.clamp(rows.abs() - tol, min=0.0))[1]
    am_hi = mx.mx6_reference(rows.abs() + tol)[1]
    firm = am_lo == am_hi
    assert float(firm.float().mean()) > 0.98, "%s: %d of %d blocks sit on a power of two" % (what, int((~firm).sum()), firm.numel())
    assert torch.equal(scale[:, :C // 32][firm], am_hi[firm]), "%s: scale bytes differ" % what
    assert bool(((scale[:, :C // 32] == am_lo) | (scale[:, :C // 32] == am_hi)).all())
    got_x = mx.decode(codes, scale)
    fe = firm.repeat_interleave(32, dim=1)
    # under a firm E both interval ends were rounded with that E: the kernel's value lies between them
    ok = (got_x >= torch.minimum(x_lo, x_hi)) & (got_x <= torch.maximum(x_lo, x_hi))
    assert bool(ok[fe].all()), "%s: %d codes outside the statement's interval, first at %s" % (what, int((~ok & fe).sum()), (~ok & fe).nonzero()[0].tolist())
    same = got_x == mx.mx6_reference(rows)[2]
    assert float(same[fe].float().mean()) > 0.995, "%s: only %.4f of the codes equal the statement on the CPU's x′" % (what, float(same[fe].float().mean()))


@pytest.mark.parametrize("fold", ["gn_silu", "ln", "geglu"])
def test_quantiser_folded_prologue(fold, dev):
    from dgq_amd import ops
    g = torch.Generator().manual_seed(31)
    if fold == "gn_silu":
        B, C, H, W = 2, 64, 8, 8
        x = torch.randn(B, C, H, W, generator=g) * 1.3 + 0.2
        gam, bet = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
        xs = x.to(dev).contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
        sc, sh = ops.groupnorm_scale_shift(xs, B, H * W, C, 32, 1e-5, gam.to(dev), bet.to(dev))
        got = ops.quant_act_mx6(xs, (B, H, W, C, 3, 3, 1, 1), pre=(sc, sh, 1))
        pre = x * sc.cpu()[:, :, None, None] + sh.cpu()[:, :, None, None]          # (exact: the launch's own scale / shift)
        rows = rb.pixel_rows(F.silu(pre))
        tol = 4e-6 * rows.abs() + 1e-7
    elif fold == "ln":
        M, K = 77, 320
        x = torch.randn(M, K, generator=g) * 1.3 + 0.2
        gam, bet = 1 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
        got = ops.quant_act_mx6(x.to(dev), (M, 1, 1, K, 1, 1, 1, 0), ln=(gam.to(dev), bet.to(dev), 1e-5))
        rows = F.layer_norm(x.double(), (K,), gam.double(), bet.double(), 1e-5).float()
        # (x − μ)·rstd·γ + β in fp32: μ and rstd to a few ulp, the difference against |x| + |μ| — 2^-20 of the row's largest value
        tol = (2.0 ** -20 * (x.abs().amax(dim=1, keepdim=True) + 1.0)).expand_as(rows).contiguous()
    else:
        M, K = 77, 320
        x = torch.randn(M, 2 * K, generator=g) * 1.3 + 0.2
        got = ops.quant_act_mx6(x.to(dev), (M, 1, 1, K, 1, 1, 1, 0), pre=(None, None, 2))
        rows = (x[:, :K].double() * F.gelu(x[:, K:].double())).float()
        tol = 4e-6 * rows.abs() + 1e-6 * x[:, :K].abs()
    torch.cuda.synchronize()
    check_quantiser_behind_prologue(got, rows, tol, fold)


# ----------------------------------------------------------------------------------------------- 2. operand maps
def _asym_weight(N, K):
    """integer codes, zero points and power-of-two scales, asymmetric in (n, k): no two (n, k) cells of a tile confuse"""
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    qw = (3 * n + 5 * k + (n * k) % 7 + (k // 32) * 2) % 16
    zw = (1 + (5 * torch.arange(N)) % 14).float()
    wd = (2.0 ** ((torch.arange(N) % 3) - 1).double()).float()
    return qw, zw, wd


def _packed_weight(ops, dev, qw, zw, wd, bias=None):
    N, K = qw.shape
    w = wd[:, None] * (qw.float() - zw[:, None])
    pw = ops.PackedWeight(w.to(dev), wd.view(N, 1).to(dev), zw.view(N, 1).to(dev), None, bias.to(dev) if bias is not None else None, 4, K, 1)
    assert torch.equal(pw.codes.cpu().long(), qw) and pw.mx6_eligible
    return pw


def _handmade(ops, dev, codes, E, lds):
    """(codes, scale) on the device as dgq_quant_act_mx6 writes them, from 6-bit codes [M][K] and exponents E [M][K/32]"""
    from dgq_amd.quant.quant_layer import mx6_pack
    M = codes.shape[0]
    scale = torch.full((M, lds), 127, dtype=torch.uint8)
    scale[:, :E.shape[1]] = (E + 127).to(torch.uint8)
    return mx6_pack(codes.to(torch.uint8)).contiguous().to(dev), scale.to(dev)


@pytest.mark.parametrize("M,K,N", [(64, 64, 64), (37, 320, 24)])
def test_operand_map_one_hot_activations(M, K, N, dev):
    """row m holds the code of 1.0 at ONE k_m (distinct per row), every (row, block) its own E: y[m, n] must be δw[n]·(q − z)[n, k_m]·
    2^E[m, k_m / 32] — a gather, bit for bit.  A wrong lane map reads another k or n; a wrong scale byte another block's E."""
    from dgq_amd import ops
    qw, zw, wd = _asym_weight(N, K)
    ab = ops.MxActBinding(_packed_weight(ops, dev, qw, zw, wd))
    km = (torch.arange(M) * 7 + 3) % K
    assert km.unique().numel() == M
    codes = torch.zeros(M, K, dtype=torch.int64)
    codes[torch.arange(M), km] = 8                                        # 1.0
    g = torch.Generator().manual_seed(M + K)
    E = torch.randint(-6, 7, (M, K // 32), generator=g)
    E[:, 1:] = torch.where(E[:, 1:] == E[:, :-1], E[:, 1:] + 1, E[:, 1:])     # neighbouring blocks differ
    geom = (M, 1, 1, K, 1, 1, 1, 0)
    y = ops.gemm_mx6(_handmade(ops, dev, codes, E, ab.Kp // 32), geom, ab, torch.float32)
    torch.cuda.synchronize()
    want = (wd[None, :].double() * (qw.double() - zw[:, None].double())[:, km].t() * (2.0 ** E[torch.arange(M), km // 32].double())[:, None])
    got = y.cpu().double()
    bad = got != want
    assert not bool(bad.any()), "%d of %d elements differ, first at %s: got %r, want %r" % (
        int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist(), float(got[bad][0]), float(want[bad][0]))


@pytest.mark.parametrize("M,K,N", [(64, 64, 64), (37, 320, 24)])
def test_operand_map_one_hot_weights(M, K, N, dev):
    """the transpose: column n holds q − z = 2 (the E2M3 value 1.0 under the constant scale 2^1) at ONE k_n, activations asymmetric in
    (m, k) with their own E per (row, block): y[m, n] = δw[n]·2·x̂[m, k_n], bit for bit"""
    from dgq_amd import ops
    kn = (torch.arange(N) * 5 + 1) % K
    assert kn.unique().numel() == N
    zw = (1 + (5 * torch.arange(N)) % 13).float()                          # 1 .. 13: z + 2 is a code
    qw = zw.long()[:, None].repeat(1, K)
    qw[torch.arange(N), kn] += 2
    wd = (2.0 ** ((torch.arange(N) % 3) - 1).double()).float()
    ab = ops.MxActBinding(_packed_weight(ops, dev, qw, zw, wd))
    m, k = torch.arange(M)[:, None], torch.arange(K)[None, :]
    codes = (7 * m + 11 * k + (m * k) % 5) % 64
    g = torch.Generator().manual_seed(N + K)
    E = torch.randint(-6, 7, (M, K // 32), generator=g)
    geom = (M, 1, 1, K, 1, 1, 1, 0)
    y = ops.gemm_mx6(_handmade(ops, dev, codes, E, ab.Kp // 32), geom, ab, torch.float32)
    torch.cuda.synchronize()
    xhat = mx.decode(codes.to(torch.uint8), (E + 127).to(torch.uint8))
    want = 2.0 * wd[None, :].double() * xhat[:, kn]
    got = y.cpu().double()
    bad = got != want
    assert not bool(bad.any()), "%d of %d elements differ, first at %s: got %r, want %r" % (
        int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist(), float(got[bad][0]), float(want[bad][0]))


def test_weight_image_is_the_statement(dev):
    """dgq_pack_w_mx6: the E2M3 codes of (q − z)/2 in the natural (tap, c) order, the K padding as code 0 — a 3x3 layer with Kp > K"""
    from dgq_amd import ops
    from dgq_amd.quant.quant_layer import mx6_unpack
    N, C, taps = 24, 32, 9
    K = C * taps
    qw, zw, wd = _asym_weight(N, K)
    w = (wd[:, None] * (qw.float() - zw[:, None])).view(N, C, 3, 3)
    pw = ops.PackedWeight(w.to(dev), wd.view(N, 1, 1, 1).to(dev), zw.view(N, 1, 1, 1).to(dev), None, None, 4, C, taps)
    img, Kp = pw.mx6()
    assert Kp == 384 and tuple(img.shape) == (N, Kp // 32, 24) and pw.mx6()[0] is img
    got = mx.decode(mx6_unpack(img.cpu()), torch.full((N, Kp // 32), 127, dtype=torch.uint8))
    nat = (qw.double() - zw[:, None].double()).view(N, C, taps).permute(0, 2, 1).reshape(N, K) / 2.0
    assert torch.equal(got[:, :K], nat) and float(got[:, K:].abs().max()) == 0.0
    assert int(mx6_unpack(img.cpu())[:, K:].max()) == 0


def test_bad_arguments_are_refused(dev):
    from dgq_amd import ops
    qw, zw, wd = _asym_weight(24, 64)
    pw = _packed_weight(ops, dev, qw, zw, wd)
    ab = ops.MxActBinding(pw)
    x = torch.randn(8, 64, device=dev)
    q = ops.quant_act_mx6(x, (8, 1, 1, 64, 1, 1, 1, 0), lds=ab.Kp // 32)
    ex = ops._lib.GemmExtra()
    ex.res_div, ex.act = 1, 256                                            # (a non-null pointer value: refused before anything reads it)
    with pytest.raises(RuntimeError, match="dgq_gemm_mx6"):                # a quantise-on-load descriptor
        ops.gemm_mx6(q, (8, 1, 1, 64, 1, 1, 1, 0), ab, torch.float32, extra=ex)
    with pytest.raises(RuntimeError, match="dgq_gemm_mx6"):                # a folded upsample of an odd-sized image
        ops.gemm_mx6(q, (1, 3, 3, 64, 3, 3, 1, 1), ab, torch.float32, ups=True)
    with pytest.raises(RuntimeError, match="dgq_quant_act_mx6"):           # C % 32
        ops.quant_act_mx6(torch.randn(8, 48, device=dev), (8, 1, 1, 48, 1, 1, 1, 0))
    w8 = ops.PackedWeight(torch.randn(8, 64, device=dev), torch.full((8, 1), 0.01, device=dev), torch.full((8, 1), 128.0, device=dev), None, None, 8, 64, 1)
    assert not w8.mx6_eligible
    half = ops.PackedWeight(torch.randn(8, 64, device=dev), torch.full((8, 1), 0.3, device=dev), torch.full((8, 1), 7.5, device=dev), None, None, 4, 64, 1)
    assert not half.mx6_eligible


# ----------------------------------------------------------------------------------------------- 3. exact layers
EXACT_CASES = [
    lr.linear_case(154, 768, 320),                                        # ragged M
    lr.conv_case(2, 64, 7, 9, 1, 64, k=1),
    lr.conv_case(2, 32, 9, 9, 1, 24),                                     # N < tile, Kp = 384 > K = 288
    lr.conv_case(2, 64, 11, 13, 2, 64),
    lr.conv_case(2, 64, 8, 8, 1, 64, upsample=True),
    lr.linear_case(37, 320, 24),                                          # ragged M and N, Kp = 384
]


def _exact_layer(ops, case, dev):
    d = mx.planted_mx6(case)
    y_ref, xhat = mx.mx6_layer_reference(case, d["x"], d["qw"], d["wzp"], d["wdelta"], d["bias"], d["residual"])
    margin = mx.mx6_exact_margin(case, xhat, d["qw"], d["wzp"], d["wdelta"], d["bias"], d["residual"])
    assert margin < 1.0, "%s: the term magnitudes reach %.3f x 2^24 units — narrow the ranges" % (case["name"], margin)
    B, H, W, Ho, Wo, M, K, taps = lr.geometry(case)
    pw = ops.PackedWeight(d["w"].to(dev), d["wdelta"].to(dev), d["wzp"].to(dev), None, d["bias"].to(dev), 4, K // taps, taps)
    assert torch.equal(pw.codes.cpu().long(), d["qw"]) and pw.mx6_eligible
    return d, y_ref, ops.MxActBinding(pw)


@pytest.mark.parametrize("case", EXACT_CASES, ids=lambda c: c["name"])
def test_exact_layers_equal_the_reference(case, dev, monkeypatch):
    from dgq_amd import _lib, ops
    d, y_ref, ab = _exact_layer(ops, case, dev)
    spy = routes.Spy(ops, _lib)
    monkeypatch.setattr(ops, "_lib_call", spy)
    y = routes.run_layer(ops, case, ab, d["x"].to(dev), d["residual"].to(dev))
    torch.cuda.synchronize()
    names = [c["name"] for c in spy.take()]
    assert names.count("dgq_quant_act_mx6") == 1 and names.count("dgq_gemm_mx6") == 1, names
    assert not any(n.startswith("dgq_act_row_params") or n in ("dgq_quant_act_batch", "dgq_quant_act_block", "dgq_gemm_blockq")
                   or n.startswith("dgq_gemm_wxa8") for n in names), names
    got = y.cpu().double()
    if not torch.equal(got, y_ref):
        bad = got != y_ref
        idx = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: y differs from the reference on %d of %d elements, first at %s: got %r, want %r"
                             % (case["name"], int(bad.sum()), bad.numel(), idx, float(got[idx]), float(y_ref[idx])))


# ----------------------------------------------------------------------------------------------- 4. real-valued layers
REAL_CASES = ["linear_m154_k768_n320", "linear_m2048_k640_n640", "conv3x3_b2_c32_9x9_s1_n24"]


def real_layer_ratio(ops, case, d, x, dev):
    """runs the layer on x (no residual) and returns (worst |y − y64| / (K·2^-24·T) over the elements, y, y64, T) with y64 the float64
    layer on the KERNEL's own codes and scales"""
    B, H, W, Ho, Wo, M, K, taps = lr.geometry(case)
    pw = ops.PackedWeight(d["w_raw"].to(dev), d["wdelta"].to(dev), d["wzp"].to(dev), None, d["bias"].to(dev), 4, K // taps, taps)
    assert pw.mx6_eligible
    ab = ops.MxActBinding(pw)
    y = routes.run_layer(ops, case, ab, x.to(dev), None).cpu().double()
    lin = case["kind"] == "linear"
    C = K // taps
    xs = x.to(dev).reshape(-1, C) if lin else x.to(dev).contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
    got = ops.quant_act_mx6(xs, (M, 1, 1, C, 1, 1, 1, 0) if lin else (B, H, W, C, case["k"], case["k"], case["stride"], case["pad"]))
    torch.cuda.synchronize()
    codes, scale = unpacked(got, C)
    xhat = mx.rows_to_input(case, mx.decode(codes, scale), x)
    qw, zw, wd = pw.codes.cpu().long(), pw.zp_true.cpu(), pw.alpha.cpu()
    y64 = mx.layer_float64(case, xhat, qw, zw, wd, d["bias"])
    T = mx.term_magnitudes(case, xhat, qw, zw, wd, d["bias"])
    return float(((y - y64).abs() / (K * 2.0 ** -24 * T)).max()), y, y64, T, K


@pytest.mark.parametrize("data", ["randn", "outlier"])
@pytest.mark.parametrize("name", REAL_CASES)
def test_real_layers_inside_the_bound(name, data, dev, capsys):
    """per element |y − y64| <= C_SUM·K·2^-24·T + 2^-24·|y64|, T = |bias| + δw·Σ|x̂·(q − z)|, y64 from the kernel's own codes"""
    from dgq_amd import ops
    case = lr.CASES_BY_NAME[name]
    d = lr.real_case(case, "perM", 6, 4)
    x = d["x"]
    if data == "outlier":
        x = mx.rows_to_input(case, mx.outlier_rows(mx.input_rows(case, x)), x).contiguous()
    ratio, y, y64, T, K = real_layer_ratio(ops, case, d, x, dev)
    with capsys.disabled():
        print("\nREAL-TIME MXFP6 %s %s: worst |y - y64| / (K 2^-24 T) = %.4g; rel-L2 %.3g" % (name, data, ratio, rel_l2(y, y64)))
    bound = C_SUM * K * 2.0 ** -24 * T + 2.0 ** -24 * y64.abs()
    bad = (y - y64).abs() > bound
    assert not bool(bad.any()), "%s %s: %d elements outside the bound, worst ratio %.4g" % (name, data, int(bad.sum()), ratio)


# ----------------------------------------------------------------------------------------------- 5. epilogues
@pytest.fixture(scope="module")
def epi(dev):
    from dgq_amd import ops
    case = lr.linear_case(154, 768, 320)
    d, y_ref, ab = _exact_layer(ops, case, dev)
    x = d["x"].to(dev)
    return dict(case=case, d=d, ab=ab, x=x, y0=ops.quant_linear(x, ab))


def test_epilogue_residual(epi, dev):
    from dgq_amd import ops
    res = epi["d"]["residual"].to(dev)
    assert torch.equal(ops.quant_linear(epi["x"], epi["ab"], residual=res), epi["y0"] + res)


def test_epilogue_geglu(epi, dev):
    """packed rows (value, gate) interleaved: column i of the GEGLU output is y[2i]·gelu(y[2i+1]).  The projection values are the plain
    call's bit for bit; the erf of the kernel and of the host differ in their last bits: 1e-6 rel-L2, the bound of
    test_gemm_geglu_epilogue_equals_projection_then_geglu for fp32"""
    from dgq_amd import ops
    y = ops.quant_linear(epi["x"], epi["ab"], geglu=True)
    y0 = epi["y0"].double()
    a, gt = y0[..., 0::2], y0[..., 1::2]
    want = a * (0.5 * gt * (1.0 + torch.erf(gt * 0.70710678118654752)))
    assert y.shape == want.shape
    assert rel_l2(y.cpu(), want.cpu()) < 1e-6


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=lambda d: str(d).replace("torch.", ""))
def test_epilogue_16bit_output(epi, dtype, dev):
    """the planted grid values are 16-bit representable: the same codes and sums, the fp32 result rounded once"""
    from dgq_amd import ops
    x16 = epi["x"].to(dtype)
    assert torch.equal(x16.float(), epi["x"])
    y = ops.quant_linear(x16, epi["ab"])
    assert y.dtype == dtype and torch.equal(y, epi["y0"].to(dtype))


def test_epilogue_second_copy(epi, dev):
    from dgq_amd import ops
    ab, x = epi["ab"], epi["x"]
    M, K, N = 154, 768, 320
    geom = (M, 1, 1, K, 1, 1, 1, 0)
    buf = torch.zeros(M, N + 72, device=dev)
    q = ops.quant_act_mx6(x.view(M, K), geom, lds=ab.Kp // 32)
    y = ops.gemm_mx6(q, geom, ab, torch.float32, extra=ops.make_extra(y2=buf[:, 40:40 + N]))
    assert torch.equal(y, epi["y0"].view(M, N)) and torch.equal(buf[:, 40:40 + N], y)
    assert float(buf[:, :40].abs().max()) == 0.0 and float(buf[:, 40 + N:].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=gs.ids_dtype)
@pytest.mark.parametrize("k,upsample", [(3, False), (3, True), (1, False)])
def test_groupnorm_partials(k, upsample, dtype, dev, monkeypatch):
    """the partials dgq_gemm_mx6's epilogue leaves against the float64 statistics of the tensor AS STORED: the metric, the data kinds and
    the tolerance of tests/test_gpu_groupnorm_stats.py's "partials" family (the epilogue is the family's gemm_store_tile)"""
    from dgq_amd import ops, synth
    B, C, Hs, N, G = 2, 64, 8, 64, 8
    H = 2 * Hs if upsample else Hs
    gen = torch.Generator().manual_seed(11)
    w = torch.randn(N, C, k, k, generator=gen) * 0.05
    wd, wz = synth.channel_minmax(w, 4)
    ab = ops.MxActBinding(ops.PackedWeight(w.to(dev), wd.to(dev), wz.to(dev), None, gs.chan_bias(N, G, 11).to(dev), 4, C, k * k))
    x = gs.image(B, C, Hs, Hs, dtype, dev, 12)
    spy = gs.spied(ops, monkeypatch)
    for kind in gs.RES_KINDS:
        y = ops.quant_conv2d(x, ab, k, k, 1, k // 2, residual=gs.residual(kind, B, H, H, N, G, dtype, dev), gn_out=True, upsample=upsample)
        names = [c["name"] for c in spy.take()]
        assert names.count("dgq_gemm_mx6") == 1 and "dgq_gemm_blockq" not in names, names
        assert tuple(y.shape) == (B, N, H, H)
        gs.check_partials(ops, dev, kind, "mx6 %dx%d%s %s" % (k, k, " upsample" if upsample else "", gs.NAME[dtype]), y, G)


# ----------------------------------------------------------------------------------------------- 6. row independence
def test_rows_are_independent(dev):
    """changing one row changes only that output row; a permutation of the rows permutes the output"""
    from dgq_amd import ops
    M, K, N = 154, 768, 320
    g = torch.Generator().manual_seed(M + N)
    x = (torch.randn(M, K, generator=g) * 1.3 + 0.2).to(dev)
    ab = ops.MxActBinding(rta._packed(ops, dev, N, K, 1, 9))
    y = ops.quant_linear(x, ab)
    x2 = x.clone()
    x2[77] = x2[77] * 3.0 + 1.0
    y2 = ops.quant_linear(x2, ab)
    keep = torch.arange(M, device=dev) != 77
    assert torch.equal(y2[keep], y[keep]) and not torch.equal(y2[77], y[77])
    perm = torch.randperm(M, generator=g).to(dev)
    assert torch.equal(ops.quant_linear(x[perm].contiguous(), ab), y[perm])


# ----------------------------------------------------------------------------------------------- 7. public API
def test_quant_layer_mxfp6_beats_row_on_outliers(dev, capsys):
    """a QuantLayer under the MXFP6 quantiser against the same layer under the row quantiser at A6, on the outlier data of the CPU test:
    at most half the error against the float64 product with unquantised activations"""
    from dgq_amd import ops
    from dgq_amd.quant import QuantLayer, Scaler
    c = rb.outlier_case(64, 768, 320, 6)
    errs = {}
    for fmt in ("row", "mxfp6"):
        lin = torch.nn.Linear(768, 320, bias=False)
        lin.weight.data.copy_(c["w_raw"])
        aq = {"bits": 6, "channel_wise": False, "scaler": Scaler.MINMAX, "leaf_param": True, "real_time": True}
        if fmt == "mxfp6":
            aq.update(real_time_block=32, real_time_format="mxfp6")
        layer = QuantLayer(lin, {"bits": 4, "channel_wise": True, "scaler": Scaler.MINMAX}, aq).to(dev)
        layer.set_quant_state(True, True)
        with torch.no_grad():
            y = layer(c["x"].to(dev))
        assert isinstance(layer._bindings["real_time"], ops.MxActBinding if fmt == "mxfp6" else ops.DynamicActBinding)
        y64 = c["x"].double() @ layer.dequantized_weight(torch.float32).double().cpu().t()
        errs[fmt] = rel_l2(y.cpu(), y64)
    with capsys.disabled():
        print("\nREAL-TIME MXFP6 outliers 64x768->320 A6: row %.3g mxfp6 %.3g (%.2fx)" % (errs["row"], errs["mxfp6"], errs["row"] / errs["mxfp6"]))
    assert errs["mxfp6"] <= 0.5 * errs["row"], errs


# ----------------------------------------------------------------------------------------------- 8. model level
@pytest.fixture(scope="module")
def mx_ckpts(tmp_path_factory):
    """a weight-only synthetic W4A6 checkpoint, and the same weights with act_* blocks (which the real-time modes ignore)"""
    from dgq_amd import synth
    d = tmp_path_factory.mktemp("mx_ck")
    wonly, full = str(d / "wonly.pth"), str(d / "full.pth")
    synth.write_cali_ckpt(wonly, "tiny", 4, 6, 1, num_slots=1, seed=0, batch=2, res=16, start_peak=True, with_act=False)
    synth.write_cali_ckpt(full, "tiny", 4, 6, 4, num_slots=2, seed=0, batch=2, res=16, start_peak=True, with_act=True)
    return wonly, full


def _build_qnn(path, dev, steps=25, time_aware=False, fmt="mxfp6"):
    import types
    from dgq_amd import synth
    from dgq_amd.diffusers_rewrite import UNet2DConditionModel
    from dgq_amd.quant import get_qmodel, Scaler
    from dgq_amd.runtime import quant_params
    unet = UNet2DConditionModel("tiny")
    unet.load_state_dict(synth.state_dict_from_ckpt(path))
    wq, aq, sm = quant_params(Scaler, 4, 6, True, True, True, True)
    aq["real_time"], aq["real_time_block"], aq["real_time_format"] = True, 32, fmt
    qnn = get_qmodel("tiny", types.SimpleNamespace(unet=unet), path, wq, True, aq, sm, False, steps, time_aware, device=dev)
    qnn = qnn.float().to(dev)
    qnn.disable_out_quantization()
    return qnn


@pytest.fixture(scope="module")
def mx_qnn(mx_ckpts, dev):
    return _build_qnn(mx_ckpts[0], dev)


def _model_case(layer, x_in):
    if layer.is_conv:
        kh, kw, st, pd = layer._conv_geom()
        return dict(kind="conv", C=x_in.shape[1], k=kh, stride=st, pad=pd, upsample=False)
    return dict(kind="linear")


def test_model_teacher_forced_vs_reference(mx_qnn, rt_inputs, capsys, monkeypatch):
    """arch ``tiny`` from a WEIGHT-ONLY checkpoint, the fused graph: every quantised layer reports once through LAYER_TAP; every layer
    is eligible here, so one layer's weight is made to report itself ineligible (as a W8 or fractional-z weight does) and is checked,
    with the call spy, to have taken the block route.  Teacher-forced, a layer without a folded prologue is inside the real-data
    bound, per element, against mx6_layer_reference of its own input (the codes are the statement's, bit for bit); a layer behind a
    folded prologue — whose x′ the CPU reproduces to a few ulp only — within 2e-3 rel-L2, the bound of the block mode's model test."""
    from dgq_amd import _lib, ops
    from dgq_amd.quant import quant_layer
    qnn = mx_qnn
    inner = rta._inner_layers(qnn)
    names = {id(m): n for n, m in inner.items()}
    mods = dict(qnn.model.named_modules())
    odd_name = sorted(n for n, m in inner.items() if not m.is_conv and n.endswith("to_out.0"))[0]
    odd = inner[odd_name]
    odd._bindings.clear()
    odd.packed_weight()._mx6_ok = False                                   # as a W8 or fractional-z weight reports itself
    spy = routes.Spy(ops, _lib)
    monkeypatch.setattr(ops, "_lib_call", spy)
    seen, worst_ratio, worst_pro, routes_of = [], (0.0, None), (0.0, None), {}

    def tap(layer, y, x=None, prologue=False, residual=None, bias_rows=None, fq=None, geglu=False):
        nonlocal worst_ratio, worst_pro
        name = names[id(layer)]
        seen.append(name)
        routes_of[name] = [c["name"] for c in spy.take() if c["name"].startswith(("dgq_gemm", "dgq_quant_act", "dgq_act_row"))]
        assert fq is None
        x_in = x.detach().float().cpu()
        if prologue:
            x_in = rta._prologue_input(mods, name, x_in)
        case = _model_case(layer, x_in)
        w = layer.dequantized_weight(torch.float32).float().cpu()
        b = layer.b.detach().float().cpu() if layer.b is not None else None
        if layer is odd:
            from tests import test_gpu_realtime_block as tb
            ref = tb._layer_reference(layer, x_in)
        else:
            xin2 = x_in if layer.is_conv else x_in.reshape(1, -1, x_in.shape[-1])
            xhat = mx.rows_to_input(case, mx.mx6_reference(mx.input_rows(case, xin2))[2], xin2)
            ref = mx.layer_float64_w(case, xhat, w, b)
            T = mx.layer_float64_w(case, xhat.abs(), w.abs(), b.abs() if b is not None else None)
            if not layer.is_conv:
                ref, T = ref.reshape(*x_in.shape[:-1], -1), T.reshape(*x_in.shape[:-1], -1)
        plain = ref
        if geglu:
            a, gte = ref.chunk(2, dim=-1)
            ref = a * F.gelu(gte)
        ref = ref.reshape(y.shape)
        if residual is not None:
            ref = ref + residual.detach().double().cpu().reshape(y.shape)
        if bias_rows is not None:
            ref = ref + bias_rows.detach().double().cpu()[:, :, None, None]
        got = y.detach().cpu().double()
        if layer is odd or prologue or geglu:
            e = rel_l2(got, ref)
            if e > worst_pro[0]:
                worst_pro = (e, name)
        else:
            K = layer.in_channels * layer.taps
            slack = 2.0 ** -24 * (plain.reshape(y.shape).abs() + ref.abs())     # the rounding of the result, and of the sum with a residual
            ratio = float((((got - ref).abs() - slack).clamp_min(0.0) / (K * 2.0 ** -24 * T.reshape(y.shape))).max())
            if ratio > worst_ratio[0]:
                worst_ratio = (ratio, name)
        return ref.to(y.device, y.dtype)

    quant_layer.LAYER_TAP = tap
    try:
        with torch.no_grad():
            out = qnn(rt_inputs[0], torch.tensor(999), rt_inputs[1])[0]
    finally:
        quant_layer.LAYER_TAP = None
    assert torch.isfinite(out).all()
    assert sorted(seen) == sorted(inner), "layers not seen exactly once: %s" % (set(inner) ^ set(seen) or [n for n in seen if seen.count(n) > 1])
    assert len(inner) == 119
    n_mx = sum(isinstance(m._bindings.get("real_time"), ops.MxActBinding) for m in inner.values())
    assert n_mx == len(inner) - 1 and isinstance(odd._bindings["real_time"], ops.BlockActBinding) and not odd._bindings["real_time"].mx
    assert "dgq_gemm_blockq" in routes_of[odd_name] and "dgq_gemm_mx6" not in routes_of[odd_name], routes_of[odd_name]
    others = [n for n in routes_of if n != odd_name and routes_of[n]]
    assert others and all("dgq_gemm_blockq" not in routes_of[n] and not any(c.startswith("dgq_gemm_wxa8") for c in routes_of[n]) for n in others)
    assert sum(c == "dgq_gemm_mx6" for n in others for c in routes_of[n]) == n_mx
    with capsys.disabled():
        print("\nREAL-TIME MXFP6 MODEL tiny: %d MX layers; worst bound ratio without a prologue %.4g (%s); worst rel-L2 behind one %.3g (%s)"
              % (n_mx, *worst_ratio, *worst_pro))
    assert worst_ratio[0] <= C_SUM, worst_ratio
    assert worst_pro[0] < 2e-3, worst_pro


def test_model_graph_replay_images_and_loader(mx_ckpts, rt_inputs, dev):
    from dgq_amd import ops
    qnn = _build_qnn(mx_ckpts[0], dev)
    x, ctx = rt_inputs
    with torch.no_grad():
        y_e = qnn(x, torch.tensor(999), ctx)[0].clone()
        y_e2 = qnn(x, torch.tensor(499), ctx)[0].clone()
        qnn.enable_graphs(True)
        y_g = qnn(x, torch.tensor(999), ctx)[0].clone()
        y_g_again = qnn(x, torch.tensor(999), ctx)[0].clone()
        qnn.enable_graphs(False)
    assert torch.isfinite(y_e).all() and not torch.equal(y_e, y_e2)
    assert torch.equal(y_g, y_e) and torch.equal(y_g_again, y_e), "graph replay differs from the eager run"
    inner = rta._inner_layers(qnn)
    for name, layer in inner.items():
        assert list(layer._bindings) == ["real_time"], name
        ab, pw = layer._bindings["real_time"], layer._pw
        assert isinstance(ab, ops.MxActBinding) and ab.wpacked is pw._mx6[0] and not layer._act_tables, name
    # the int block mode of the same checkpoint computes something else (the format is live), a 50-step model from the checkpoint WITH
    # act_* blocks the same (they are ignored)
    with torch.no_grad():
        y_int = _build_qnn(mx_ckpts[0], dev, fmt="int")(x, torch.tensor(999), ctx)[0]
        y50 = _build_qnn(mx_ckpts[1], dev, steps=50)(x, torch.tensor(999), ctx)[0]
    assert not torch.equal(y_int, y_e)
    assert torch.equal(y50, y_e), "the act_* blocks of the checkpoint changed the result"
    # two loader refusals: per-timestep tables, and the format without its block granularity
    with pytest.raises(ValueError):
        _build_qnn(mx_ckpts[0], dev, time_aware=True)
    with pytest.raises(ValueError):
        from dgq_amd.quant import Scaler
        from dgq_amd.quant.quant_layer import UniformAffineQuantizer
        UniformAffineQuantizer(bits=6, scaler=Scaler.MINMAX, real_time=True, real_time_format="mxfp6")


# ----------------------------------------------------------------------------------------------- 9. CLI
def test_cli_aq_real_time_format(tmp_path):
    from dgq_amd import inference_qmodel as cli
    out = str(tmp_path / "lat_{rank}.pt")
    cli.main(["--model_type", "tiny", "--use_aq", "--aq", "6", "--aq_real_time", "--aq_real_time_block", "32", "--aq_real_time_format", "mxfp6",
              "--t2i_log_quant", "--t2i_real_time", "--num_inference_steps", "2", "--out", out])
    d = torch.load(out.format(rank=0))
    assert sorted(d) == [0, 1] and all(torch.isfinite(v).all() for v in d.values())
    with pytest.raises(SystemExit) as e:
        cli.main(["--model_type", "tiny", "--use_aq", "--aq_real_time", "--aq_real_time_block", "32", "--aq_real_time_format", "mxfp6",
                  "--num_inference_steps", "2", "--out", out])
    assert "mxfp6" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(["--model_type", "tiny", "--use_aq", "--aq", "6", "--aq_real_time", "--aq_real_time_format", "mxfp6", "--num_inference_steps", "2",
                  "--out", out])
    assert "mxfp6" in str(e.value)
