"""ops.gemm_mx_rows (dgq_gemm_mx_rows: quantiser and MX GEMM of a Linear layer in one launch) against the two-launch route, bit for bit,
and against float64 under the MX GEMM tests' a-priori bound |y − y64| <= c·K·2^-24·S + u_out·|y64|, S = |bias| + δw·Σ|x̂·(q − z)| over the
statement's own codes, c = 1 (2 for MXINT8: two MFMA terms per product) — derived, not measured."""
import ctypes
import pytest
import torch

from tests import test_gpu_realtime_mxfp6 as t6
from tests import test_gpu_smallm_mx_batch as sm
from tests.test_gpu_realtime_act import dev, rt_inputs          # noqa: F401  (module-scoped fixtures of the row mode)

pytestmark = pytest.mark.gpu
FORMATS = sm.FORMATS
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
_LAYERS = {}


def _layer(ops, dev, fmt, K, N):
    if (fmt, K, N) not in _LAYERS:
        _LAYERS[(fmt, K, N)] = sm._layers(ops, dev, fmt, K, (N,))[0]
    return _LAYERS[(fmt, K, N)]


def _rows(M, K, dev, dtype=torch.float32):
    """the project's outlier data: random rows with one 60 per row"""
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(M + K))
    x[torch.arange(M), (torch.arange(M) * 7 + 3) % K] = 60.0
    return x.to(dev, dtype)


@pytest.fixture
def two_launch():
    """run(f): f() on the two-launch route un-split; the switches are put back afterwards"""
    from dgq_amd import ops
    saved = ops.MX_ROWS_FUSED, ops.MX_KSPLIT

    def run(f, fused=False):
        ops.MX_ROWS_FUSED, ops.MX_KSPLIT = fused, 1
        try:
            return f()
        finally:
            ops.MX_ROWS_FUSED, ops.MX_KSPLIT = saved
    return run


@DTYPES
@pytest.mark.parametrize("fmt", FORMATS)
def test_bits_of_the_two_launch_route_and_the_float64_bound(fmt, dtype, dev, two_launch, capsys):
    """M: one row, a full panel, a ragged second panel, several; K: one block, Kp = 384 with a part-filled K tile, the LDS limit (MXINT8:
    the 32-row panel); N: a ragged single tile, several tiles with a ragged last, a column split"""
    from dgq_amd import ops
    worst = 0.0
    for K in (32, 320, 1280):
        for M in (1, 64, 65, 200):
            x = _rows(M, K, dev, dtype)
            xhat = sm._xhat(ops, fmt, x, 0)
            for N in (24, 200, 640):
                layer = _layer(ops, dev, fmt, K, N)
                y = ops.gemm_mx_rows(x, [layer[0]])[0]
                assert torch.equal(y, two_launch(lambda: ops.quant_linear(x, layer[0]))), (M, K, N)
                _, d, wd, bias = layer
                y64, S = bias + wd * (xhat @ d.t()), bias.abs() + wd * (xhat.abs() @ d.abs().t())
                bound = (2 if fmt == "mxint8" else 1) * K * 2.0 ** -24 * S + sm.U_OUT[dtype] * y64.abs()
                worst = max(worst, float(((y.cpu().double() - y64).abs() / bound).max()))
    with capsys.disabled():
        print("\nMX ROWS %s %s: worst |y - y64| / bound = %.4g" % (fmt, dtype, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("case", ["ln", "silu", "geglu_in", "residual", "geglu_out"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_prologues_and_epilogues_through_quant_linear(fmt, case, dev, two_launch):
    from dgq_amd import ops
    M, K, N = 65, 320, 200
    layer = _layer(ops, dev, fmt, K, N)[0]
    x = _rows(M, 2 * K if case == "geglu_in" else K, dev)
    g = torch.Generator().manual_seed(1)
    kw = {"ln": dict(ln=((torch.rand(K, generator=g) + 0.5).to(dev), torch.randn(K, generator=g).to(dev), 1e-5)), "silu": dict(pre_act=1),
          "geglu_in": dict(pre_act=2), "residual": dict(residual=torch.randn(M, N, generator=g).to(dev)), "geglu_out": dict(geglu=True)}[case]
    seen = []
    ops.BLOCK_LAUNCH_HOOK = lambda issue, kind, info: seen.append(kind)
    try:
        y_on = two_launch(lambda: ops.quant_linear(x, layer, **kw), fused=True)
    finally:
        ops.BLOCK_LAUNCH_HOOK = None
    assert seen == ["rows"] and torch.equal(y_on, two_launch(lambda: ops.quant_linear(x, layer, **kw)))


@pytest.mark.parametrize("fmt", FORMATS)
def test_column_splits_and_batching_change_nothing(fmt, dev, two_launch):
    from dgq_amd import ops
    M, K = 65, 320
    x = _rows(M, K, dev)
    abs_ = [_layer(ops, dev, fmt, K, N)[0] for N in (200, 24, 640)]
    ref = two_launch(lambda: ops.quant_linear_multi(x, abs_))
    for s in (1, 2, 3):
        assert torch.equal(ops.gemm_mx_rows(x, [abs_[2]], col_splits=s)[0], ref[2]), s
        for y, r in zip(ops.gemm_mx_rows(x, abs_, col_splits=s), ref):
            assert torch.equal(y, r), s
    for y, r in zip(two_launch(lambda: ops.quant_linear_multi(x, abs_), fused=True), ref):
        assert torch.equal(y, r)


@pytest.mark.parametrize("fmt", FORMATS)
def test_exact_data_equals_float64(fmt, dev):
    """x in {−2 .. 2} (exact in every format), integer q − z and bias, power-of-two δw: every partial sum is an integer below 2^24"""
    from dgq_amd import ops
    M, K, N = 65, 320, 200
    qw, zw, wd = t6._asym_weight(N, K)
    bias = ((torch.arange(N) % 9) - 4).float()
    ab = ops.MxActBinding(t6._packed_weight(ops, dev, qw, zw, wd, bias), fmt)
    m, k = torch.arange(M)[:, None], torch.arange(K)[None, :]
    x = (((3 * m + 7 * k + (m * k) % 3) % 5) - 2).float()
    y64 = bias.double() + wd.double() * (x.double() @ (qw.double() - zw.double()[:, None]).t())
    assert torch.equal(ops.gemm_mx_rows(x.to(dev), [ab])[0].cpu().double(), y64)


@pytest.mark.parametrize("fmt", FORMATS)
def test_unet_routes_its_linear_layers(fmt, tmp_path, rt_inputs, dev):
    """arch ``tiny``: flag on = the same bits in fewer launches, some of kind "rows"; flag off = none of that kind"""
    from dgq_amd import ops, synth
    path = str(tmp_path / "wonly.pth")
    synth.write_cali_ckpt(path, "tiny", 4, ops.MX_FORMAT_BITS[fmt], 1, num_slots=1, seed=0, batch=2, res=16, start_peak=True, with_act=False)
    qnn = sm._build_qnn(path, dev, fmt)
    x, ctx = rt_inputs

    def run(on):
        seen = []
        ops.MX_ROWS_FUSED, ops.BLOCK_LAUNCH_HOOK = on, lambda issue, kind, info: seen.append(kind)
        with torch.no_grad():
            return qnn(x, torch.tensor(999), ctx)[0].clone(), seen
    try:
        (y_off, off), (y_on, on) = run(False), run(True)
    finally:
        ops.MX_ROWS_FUSED, ops.BLOCK_LAUNCH_HOOK = False, None
    assert torch.equal(y_on, y_off)
    assert "rows" not in off and on.count("rows") > 0 and len(on) < len(off), (len(on), len(off))


def test_refusals(dev):
    from dgq_amd import ops, _lib
    lib = _lib.load()
    ab = _layer(ops, dev, "mxfp6", 32, 24)[0]

    def call(n=1, C=32, kh=1, Kps=(ab.Kp,) * 5):
        x = torch.zeros(2, C, device=dev)
        y = torch.empty(2, 24, device=dev)
        a, _ = ops._quant_input(x, (2, 1, 1, C, kh, kh, 1, 0), 6)
        gs = (_lib.GemmArgs * 5)()
        for g, Kp in zip(gs, Kps):
            g.rowsum_parts, g.M, g.Kp, g.wpacked, g.w_bits, g.N, g.L = 1, 2, Kp, ab.wpacked.data_ptr(), 4, 24, 1
            g.alpha, g.gamma, g.y, g.y_dtype, g.ldy = ab.pw.alpha.data_ptr(), ab.gamma.data_ptr(), y.data_ptr(), _lib.DTYPE_CODE[y.dtype], 24
        return lib.dgq_gemm_mx_rows(ctypes.byref(a), 6, n, ctypes.cast(gs, ctypes.c_void_p), 0, _lib.stream())
    assert call() == 0
    for kw in (dict(C=5120, Kps=(5120,) * 5), dict(C=48), dict(kh=3), dict(n=5), dict(n=2, Kps=(ab.Kp, 2 * ab.Kp))):
        assert call(**kw) == -1 and "dgq_gemm_mx_rows" in _lib.last_error(), (kw, _lib.last_error())
    assert lib.dgq_gemm_mx_rows_plan(64, 640, 5120, 6) == 0 and lib.dgq_gemm_mx_rows_plan(64, 640, 1280, 8) > 0
