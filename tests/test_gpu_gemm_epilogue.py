"""The GEMM family's store epilogue (csrc/gemm_tile.h gemm_store_tile, csrc/gemm_wxa8.hip splitk_epilogue_kernel) against the float64
statement of tests/gemm_epilogue_ref.py, in every form and alignment, by EQUALITY.

Every output view (y, y2) is carved out of a larger allocation pre-filled with a sentinel bit pattern, at the element offset and row
pitch of its alignment class; after the launch the WHOLE allocation is compared as integers with the expected image: the window must
hold the reference, everything else (the elements in front of the base, the pitch gap of every row, the tail) still the sentinel.  The
residual sits in such an allocation too (a read outside its window returns a NaN), and it and every table are compared with a clone
taken before the launch.  The data are exact (tests/test_gemm_epilogue_ref_cpu.py), so no tolerance appears anywhere.

Each test prints one line per cell — family, extras, output dtype, alignment class of y / y2 / residual, and the side of every vector /
scalar choice the cell's full column groups take — and asserts at its end that the family met every class for every operand it accepts."""
import ctypes
import types

import pytest
import torch

from tests import gemm_epilogue_ref as er

pytestmark = pytest.mark.gpu

RING_TILES = ["32,64,1", "32,128,1", "64,64,1", "64,128,1", "128,64,1", "128,128,1"]
W8_TILES = ["32,64,1", "128,128,1"]
SPLIT_PLANS = ["32,64,3", "64,128,2"]


@pytest.fixture(scope="module")
def dev():
    from dgq_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


# ----------------------------------------------------------------------------------------------- buffers and comparison
def sentinel_alloc(total, dtype, dev):
    a = torch.full((total,), er.SENTINEL[dtype], dtype=torch.int64).to(er.INT_VIEW[dtype]).to(dev).view(dtype)
    assert a.data_ptr() % 16 == 0
    return a


def place(window, layout, dev):
    """``window`` (CPU, its final dtype) inside a sentinel allocation at ``layout``: (allocation, the strided device view)"""
    off, pitch, total = layout
    a = sentinel_alloc(total, window.dtype, dev)
    v = er.carve(a, off, pitch, *window.shape)
    v.copy_(window.to(dev))
    return a, v


def check_image(what, alloc, want_img, dtype, layout, rows, cols):
    got = alloc.view(er.INT_VIEW[dtype]).cpu()
    if not torch.equal(got, want_img):
        off, pitch, _ = layout
        r, c, where, g, w = er.first_mismatch(got, want_img, dtype, off, pitch, rows, cols)
        raise AssertionError("%s: %d elements differ, first at row %d column %d, %s the window: got %s, want %s"
                             % (what, int((got != want_img).sum()), r, c, where, g, w))


class Table:
    """the coverage table of one test: printed line by line, checked at the end"""

    def __init__(self, family):
        self.family, self.rows = family, []

    def add(self, c, split=False):
        d, p = er.describe(c), er.paths(c, split)
        self.rows.append((d, p))
        print("EPILOGUE | %-14s | %-22s | %-4s | y %s y2 %s res %s | N %d Kp %d %s | %s" % (
            self.family, d[0], d[1], d[2], d[3], d[4], c["N"], c["Kp"], "perM" if c["per_m"] else "perK",
            " ".join("%s:%s" % kv for kv in p.items() if kv[1] != "-")))

    def check(self, operands=("y", "y2", "res"), choices=("y", "y2", "res", "geglu"), classes=er.CLASSES):
        col = dict(y=2, y2=3, res=4)
        for k in operands:
            assert {d[col[k]] for d, _ in self.rows} >= set(classes), "%s: classes of %s" % (self.family, k)
        for k in choices:
            assert {p[k] for _, p in self.rows} >= {"vec", "scalar"}, "%s: both sides of the %s choice" % (self.family, k)


# ----------------------------------------------------------------------------------------------- the wxa8 family on direct operands
def wxa8_binding(c, dev):
    """what ops.gemm_wxa8 reads of an ActBinding, from the cell's tables directly (no plan_act, no quantiser)"""
    f = lambda t: t.float().to(dev).contiguous()
    from dgq_amd import ops
    codes = c["s"].to(torch.int8).to(dev)
    wp = ops.pack_weight(c["qw"].to(torch.uint8).to(dev), None, c["Kp"], 4) if c["wbits"] == 4 else c["qw"].to(torch.int8).to(dev)
    pw = types.SimpleNamespace(N=c["N"], bits=c["wbits"], alpha=f(c["alpha"]), zw=f(c["zw"]), K=c["Kp"])
    ab = types.SimpleNamespace(pw=pw, Kp=c["Kp"], wpacked=wp, mode="perM" if c["per_m"] else "perK", cdelta=f(c["cdelta"]),
                               cflush=c["cflush"].to(dev), mdelta=f(c["mdelta"]), mzp=f(c["mzp"]), L=er.L_PER_M, vn=f(c["vn"]),
                               offset=er.OFFSET, gamma=f(c["gamma"]))
    return ab, codes, f(c["rowsum"])


def cell_extra(ops, c, dev, gn_partial=None):
    """(the dgq_gemm_extra_t of the cell, its output allocations and views, the tensors a launch must leave unchanged)"""
    dt = c["dtype"]
    bufs, frozen = {}, []
    off, pitch, total = c["y_layout"]
    bufs["y"] = sentinel_alloc(total, dt, dev)
    out = er.carve(bufs["y"], off, pitch, c["M"], c["cols"])
    kw = {}
    if c["y2cls"] is not None:
        off2, pitch2, total2 = c["y2_layout"]
        bufs["y2"] = sentinel_alloc(total2, dt, dev)
        kw["y2"] = er.carve(bufs["y2"], off2, pitch2, c["M"], c["N"])
    if c["res"] is not None:
        ra, rv = place(c["residual"].to(er.DTYPES[c["res"][0]]), c["res_layout"], dev)
        kw["residual"], kw["res_div"] = rv, c["res"][2]
        frozen.append(ra)
    if c["fq"]:
        fd, fz = c["fq_delta"].float().to(dev), c["fq_zp"].float().to(dev)
        kw["fq"] = (c["fq"], fd, fz, er.FQ_T, er.FQ_D, c["fq_skip"], 8)
        frozen += [fd, fz]
    if c["geglu"]:
        kw["geglu"] = True
    if gn_partial is not None:
        kw["gn_partial"] = gn_partial
    return ops.make_extra(**kw), bufs, out, frozen


def check_cell(what, c, bufs, frozen, before):
    torch.cuda.synchronize()
    want = er.images(c)
    check_image(what + " y", bufs["y"], want["y"], c["dtype"], c["y_layout"], c["M"], c["cols"])
    if "y2" in bufs:
        check_image(what + " y2", bufs["y2"], want["y2"], c["dtype"], c["y2_layout"], c["M"], c["N"])
    for t, b in zip(frozen, before):
        assert torch.equal(t.view(torch.uint8), b), "%s: the launch changed one of its inputs" % what


def snapshot(tensors):
    return [t.view(torch.uint8).clone() for t in tensors]


def run_wxa8_cell(ops, c, dev, label, gn_partial=None):
    ab, codes, rowsum = wxa8_binding(c, dev)
    extra, bufs, out, frozen = cell_extra(ops, c, dev, gn_partial)
    frozen += [codes, rowsum, ab.wpacked, ab.pw.alpha, ab.pw.zw, ab.gamma, ab.vn, ab.cdelta, ab.mdelta, ab.mzp]
    before = snapshot(frozen)
    ops.gemm_wxa8(codes, rowsum, c["M"], ab, c["dtype"], out=out, extra=extra)
    check_cell("%s %s" % (label, c["name"]), c, bufs, frozen, before)


@pytest.mark.parametrize("tile", RING_TILES)
def test_ring_tiles_unsplit(tile, dev, monkeypatch):
    """every cell of er.cells on each ring tile shape (32x64 runs WVK = 2: the two K halves of a tile added behind a barrier)"""
    from dgq_amd import ops
    monkeypatch.setenv("DGQ_GEMM_FORCE", tile)
    monkeypatch.setattr(ops, "GEMM_FUSE", False)
    tab = Table("ring " + tile)
    for c in er.cells(83):
        run_wxa8_cell(ops, c, dev, tile)
        tab.add(c)
    tab.check()


@pytest.mark.parametrize("tile", W8_TILES)
def test_ring_tiles_w8(tile, dev, monkeypatch):
    from dgq_amd import ops
    monkeypatch.setenv("DGQ_GEMM_FORCE", tile)
    tab = Table("ring W8 " + tile)
    for c8 in er.cells(83, 8):
        run_wxa8_cell(ops, c8, dev, "W8 " + tile)
        tab.add(c8)
    tab.check()


@pytest.mark.parametrize("plan", SPLIT_PLANS)
def test_split_plans_slab_store_and_combine(plan, dev, monkeypatch):
    """K-split launches: the slab store (vector iff N % 4 == 0) and the combine kernel on and off its vec4 row.  Kp = 384 on every cell
    (one K tile cannot split); the GEGLU cells run unsplit, as the header says."""
    from dgq_amd import _lib, ops
    monkeypatch.setenv("DGQ_GEMM_FORCE", plan)
    tab = Table("split " + plan)
    ws = ops.workspace(dev)
    for c3 in er.cells(83, 4, 384):
        splits = _lib.load().dgq_gemm_plan_splits(c3["M"], c3["N"], 384, 4, c3["per_m"], ctypes.c_size_t(ws.numel()))
        assert splits == int(plan.split(",")[2])
        run_wxa8_cell(ops, c3, dev, plan)
        tab.add(c3, split=not c3["geglu"])
    tab.check(choices=("y", "y2", "res", "geglu", "slab", "combine"))


def test_rows256_kernel(dev, monkeypatch):
    """the 256-row kernel at M = 300: both staged halves of every wave tile (EPH = 2, a residual prefetch per half) and a second,
    ragged row tile"""
    from dgq_amd import ops
    monkeypatch.setenv("DGQ_GEMM_FORCE", "256,256,1")
    tab = Table("rows256")
    for c in er.cells(300):
        run_wxa8_cell(ops, c, dev, "256,256,1")
        tab.add(c)
    tab.check()


# ----------------------------------------------------------------------------------------------- refusals the header documents
def test_documented_refusals_are_refusals(dev, monkeypatch):
    """GEGLU with N % 4 != 0, with a residual, with the fused quantiser or with y2; GroupNorm partials with M % 16 != 0, N % 4 != 0 or
    the fused quantiser; ldr < N; ldy2 < N; ldy < N — each refused by the host check, nothing written"""
    from dgq_amd import ops
    monkeypatch.setenv("DGQ_GEMM_FORCE", "64,64,1")
    base = dict(name="refusal", M=83, N=68, Kp=128)

    def refused(match, gn_rows=None, shrink=None, **kw):
        c = er.make_case(**dict(base, **kw))
        ab, codes, rowsum = wxa8_binding(c, dev)
        gn = torch.zeros((gn_rows, c["N"], 2), device=dev) if gn_rows else None
        extra, bufs, out, frozen = cell_extra(ops, c, dev, gn)
        if shrink == "ldr":
            extra.ldr = c["N"] - 1
        elif shrink == "ldy2":
            extra.ldy2 = c["N"] - 1
        elif shrink == "ldy":
            out = out.as_strided(out.shape, (c["N"] - 1, 1), out.storage_offset())
        with pytest.raises(RuntimeError, match=match):
            ops.gemm_wxa8(codes, rowsum, c["M"], ab, c["dtype"], out=out, extra=extra)
        torch.cuda.synchronize()
        for k, a in bufs.items():
            assert bool((a.view(er.INT_VIEW[c["dtype"]]) == er.SENTINEL[c["dtype"]]).all()), "a refused call wrote %s" % k

    geglu70 = dict(geglu=True, N=68)
    refused("GEGLU", **geglu70, res=("f32", "A", 1))
    refused("GEGLU", **geglu70, fq=1)
    refused("GEGLU|y2", **geglu70, y2cls="A")
    c = er.make_case(**dict(base, N=70))                               # N % 4 != 0 under GEGLU
    ab, codes, rowsum = wxa8_binding(c, dev)
    out = cell_extra(ops, c, dev)[2]
    with pytest.raises(RuntimeError, match="GEGLU"):
        ops.gemm_wxa8(codes, rowsum, 83, ab, torch.float32, out=out, extra=ops.make_extra(geglu=True))
    refused("GroupNorm partials", gn_rows=6, M=83)
    refused("GroupNorm partials", gn_rows=6, M=96, N=70)
    refused("GroupNorm partials", gn_rows=6, M=96, fq=2)
    refused("residual", res=("bf16", "A", 1), shrink="ldr")
    refused("y2", y2cls="A", shrink="ldy2")
    refused("ldy", shrink="ldy")


# ----------------------------------------------------------------------------------------------- GroupNorm partials beside y2 and a misaligned residual
@pytest.mark.parametrize("plan", ["64,64,1", "32,64,3"])
def test_groupnorm_partials_with_second_copy_and_misaligned_residual(plan, dev, monkeypatch):
    """gn_partial with y2 and a residual off its vector alignment, on an unsplit tile and through the combine kernel of a K-split plan:
    the outputs are still exact; the partials are checked by tests/test_gpu_groupnorm_stats.check under ITS bound (family "partials")"""
    from dgq_amd import ops
    from tests import groupnorm_stats_ref as gr
    from tests import test_gpu_groupnorm_stats as gs
    monkeypatch.setenv("DGQ_GEMM_FORCE", plan)
    tab = Table("gn " + plan)
    for out, rcls, y2cls in (("f32", "B", "C"), ("bf16", "D", "A"), ("f32", "C", "A")):
        M, N, G = 96, 68, 4
        c = er.make_case("gn_y2%s_res%s" % (y2cls, rcls), M, N, 384, out=out, ycls="A", y2cls=y2cls, res=(out if out != "f32" else "f16", rcls, 1),
                         gn=True, seed=2)
        assert er.margin(c) < 1.0
        part = torch.zeros((M // 16, N, 2), device=dev)
        run_wxa8_cell(ops, c, dev, plan, gn_partial=part)
        tab.add(c, split=plan.endswith(",3"))
        gamma, beta = gr.make_affine(N)
        sc, sh = ops.groupnorm_from_partials(dict(parts=[(part, N)], B=2, HW=M // 2, C=N), G, gr.EPS, gamma.to(dev), beta.to(dev))
        gs.check("partials", "offset", "%s %s" % (plan, c["name"]), er.expected(c).view(2, M // 2, N), G, gamma, beta, sc, sh)


# ----------------------------------------------------------------------------------------------- one batch launch
def test_batch_of_three_problems_with_their_own_extras(dev, monkeypatch):
    """dgq_gemm_wxa8_batch, three problems sharing the codes as q / k / v do: fq_mode 2 into a class-B output (N = 68), fq_mode 3 into
    class C (N = 71), residual + y2 in class A (N = 70) — a workgroup that reads another problem's extras, N or pitch fails"""
    from dgq_amd import ops
    monkeypatch.setenv("DGQ_GEMM_FORCE", "64,64,1")
    M, Kp = 83, 384
    specs = (dict(N=68, fq=2, ycls="B"), dict(N=71, fq=3, ycls="C"), dict(N=70, res=("f32", "A", 1), y2cls="A", ycls="A"))
    tab = Table("batch 64,64")
    for per_m, out in ((0, "f32"), (1, "bf16")):
        cs = [er.make_case("batch%d" % i, M, Kp=Kp, per_m=per_m, out=out, seed=5, **s) for i, s in enumerate(specs)]
        s0 = cs[0]["s"]
        codes = s0.to(torch.int8).to(dev)
        gs, keep, checks = [], [], []
        for c in cs:
            c["s"] = s0                                              # one code matrix for the three
            assert er.margin(c) < 1.0
            ab, _, rowsum = wxa8_binding(c, dev)
            extra, bufs, outv, frozen = cell_extra(ops, c, dev)
            frozen += [codes, rowsum, ab.wpacked]
            gs.append(ops._gemm_args(ab, M, codes, rowsum, 1, outv, extra))
            keep.append((ab, codes, rowsum, extra, outv))
            checks.append((c, bufs, frozen, snapshot(frozen)))
        arr = (type(gs[0]) * 3)(*gs)
        ops._lib_call("dgq_gemm_wxa8_batch", 3, ctypes.cast(arr, ctypes.c_void_p), ops._lib.stream())
        for c, bufs, frozen, before in checks:
            check_cell("batch " + c["name"], c, bufs, frozen, before)
            tab.add(c)


# ----------------------------------------------------------------------------------------------- kernels that run their own quantiser
def run_layer_cell(ops, c, dev, label, launch, gn_partial=None):
    extra, bufs, out, frozen = cell_extra(ops, c, dev, gn_partial)
    before = snapshot(frozen)
    launch(out, extra)
    check_cell("%s %s" % (label, c["name"]), c, bufs, frozen, before)


def packed_weight(ops, d, case, dev):
    from tests import layer_reference as lr
    K, taps = lr.geometry(case)[6:8]
    pw = ops.PackedWeight(d["w"].to(dev), d["wdelta"].to(dev), d["wzp"].to(dev), None, d["bias"].to(dev), 4, K // taps, taps)
    assert torch.equal(pw.codes.cpu().long(), d["qw"]), "the weight quantiser did not find the recipe's codes"
    return pw


@pytest.mark.parametrize("layout", ["perK", "perM"])
@pytest.mark.parametrize("plan", ["", "F1,5,1,1", "F1,10,1,1"])
def test_panel_kernel_quantise_on_load(plan, layout, dev, monkeypatch):
    """the short-K panel kernel (gemm_panel.hip) with its quantiser inside, on an exact Linear cell of layer_reference._build_exact
    (M = 83, K = 128): the planner's configuration under DGQ_GEMM_FUSE_ALL and the two one-K-wave F plans; x has the output's dtype"""
    from dgq_amd import ops
    from tests import test_gpu_layer_routes as routes
    monkeypatch.setattr(ops, "GEMM_FUSE", True)
    monkeypatch.setenv("DGQ_GEMM_FUSE_ALL", "1")
    monkeypatch.setenv("DGQ_GEMM_FORCE", plan) if plan else monkeypatch.delenv("DGQ_GEMM_FORCE", raising=False)
    tab = Table("panel %s %s" % (plan or "planner", layout))
    for c in er.layer_cells("panel", layout):
        d, case = c["layer"]["d"], c["layer"]["case"]
        lay, ab = routes.build_layer(ops, case, d, dev)
        assert torch.equal(ab.pw.codes.cpu().long(), d["qw"])
        x2 = d["x"].reshape(c["M"], er.LAYER_K).to(c["dtype"]).to(dev)
        assert torch.equal(x2.cpu().float(), d["x"].reshape(c["M"], er.LAYER_K)) and ops.act_fuses(ab, c["M"], er.LAYER_K, c["dtype"], x2=x2)
        run_layer_cell(ops, c, dev, "panel", lambda out, extra: ops.gemm_act(x2, c["M"], ab, c["dtype"], extra=extra, out=out))
        tab.add(c)
    tab.check()


@pytest.mark.parametrize("family", ["blockq", "mx6"])
def test_realtime_block_and_mxfp6_gemms(family, dev):
    """dgq_gemm_blockq and dgq_gemm_mx6 (2 x 2 x 2 waves: the two K halves of a tile added behind a barrier) on one Linear cell each of
    their planted exact data; fp32 input, every output dtype"""
    from dgq_amd import ops
    tab = Table(family)
    geom = (er.LAYER_M, 1, 1, er.LAYER_K, 1, 1, 1, 0)
    for c in er.layer_cells(family):
        d, case = c["layer"]["d"], c["layer"]["case"]
        pw = packed_weight(ops, d, case, dev)
        x2 = d["x"].reshape(c["M"], er.LAYER_K).to(dev)
        if family == "blockq":
            ab = ops.BlockActBinding(pw, 8)
            q = ops.quant_act_block(x2, geom, 8, ldt=ab.Kp // 32)
            launch = lambda out, extra: ops.gemm_blockq(q, geom, ab, c["dtype"], out=out, extra=extra)
        else:
            assert pw.mx6_eligible
            ab = ops.MxActBinding(pw)
            q = ops.quant_act_mx6(x2, geom, lds=ab.Kp // 32)
            launch = lambda out, extra: ops.gemm_mx6(q, geom, ab, c["dtype"], out=out, extra=extra)
        run_layer_cell(ops, c, dev, family, launch)
        tab.add(c)
    tab.check()


def test_conv_kernel_with_quantiser_inside(dev, monkeypatch):
    """gemm_convq (TILED rows: a workgroup's 32 rows are a 4 x 8 tile of output positions) at its smallest geometry, 1 or 2 x 32 x 4 x 8
    -> 160, per-K and per-M: strided out / out2 views, residuals of every class and dtype, res_div = Ho·Wo (the bias_rows broadcast);
    GEGLU and the fused quantiser are refused there.  One cell more goes through ops.quant_conv2d with bias_rows, out and out2."""
    from dgq_amd import _lib, ops
    from tests import test_gpu_layer_routes as routes
    monkeypatch.setattr(ops, "GEMM_FUSE", True)
    monkeypatch.setattr(ops, "CONV_FUSE", True)
    monkeypatch.delenv("DGQ_GEMM_FORCE", raising=False)
    tab = Table("convq")

    def operands(c):
        d, case = c["layer"]["d"], c["layer"]["case"]
        lay, ab = routes.build_layer(ops, case, d, dev)
        assert torch.equal(ab.pw.codes.cpu().long(), d["qw"])
        x = d["x"].to(c["dtype"]).to(dev)
        assert torch.equal(x.cpu().float(), d["x"])
        xs = x.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
        B = case["B"]
        assert ops.conv_act_fuses(ab, B, 4, 8, 32, 3, 3, 1, 1, c["dtype"], xs)
        return ab, x, xs, B

    for c in er.convq_cells():
        ab, x, xs, B = operands(c)

        def launch(out, extra):
            act = ops.make_act(xs, ab, None, rows_per_image=32, conv=(B, 4, 8, 32, 3, 3, 1, 1))
            ops.gemm_wxa8(None, None, c["M"], ab, c["dtype"], out=out, extra=ops._with_act(extra, ab, c["M"], act))
        run_layer_cell(ops, c, dev, "convq", launch)
        tab.add(c)
    tab.check(choices=("y", "y2", "res"))

    # through the layer call: bias_rows [B][N] is the residual with res_div = Ho·Wo
    c = [x for x in er.convq_cells() if x["res"] is not None and x["res"][2] == 32 and x["y2cls"] is not None][0]
    ab, x, xs, B = operands(c)
    spy = routes.Spy(ops, _lib)
    monkeypatch.setattr(ops, "_lib_call", spy)

    _, bufs, out, _ = cell_extra(ops, c, dev)                          # (the views; quant_conv2d builds the struct itself)
    y2 = er.carve(bufs["y2"], c["y2_layout"][0], c["y2_layout"][1], c["M"], c["N"])
    ops.quant_conv2d(x, ab, 3, 3, 1, 1, bias_rows=c["residual"].to(er.DTYPES[c["res"][0]]).to(dev), gn_out=False, out=out, out2=y2)
    calls = [k for k in spy.take() if k["name"] == "dgq_gemm_wxa8"]
    assert len(calls) == 1 and calls[0]["fused"], calls
    check_cell("convq quant_conv2d " + c["name"], c, bufs, [], [])

    # refusals of this form: GEGLU and the fused quantiser
    c = er.convq_cells()[0]
    ab, x, xs, B = operands(c)
    fd = torch.ones(7, device=dev)
    for kw in (dict(geglu=True), dict(fq=(1, fd, fd, 7, 5, 0, 8))):
        act = ops.make_act(xs, ab, None, rows_per_image=32, conv=(B, 4, 8, 32, 3, 3, 1, 1))
        out = torch.zeros((c["M"], 160), device=dev)
        with pytest.raises(RuntimeError, match="does not take quantise-on-load"):
            ops.gemm_wxa8(None, None, c["M"], ab, torch.float32, out=out, extra=ops._with_act(ops.make_extra(**kw), ab, c["M"], act))


# ----------------------------------------------------------------------------------------------- the batched small-M Linear
@pytest.mark.parametrize("dtype", list(er.DTYPES), ids=str)
@pytest.mark.parametrize("M,K,wbits", er.SMALLM_CELLS)
def test_linear_smallm_exact_on_its_edges(M, K, wbits, dtype, dev):
    """dgq_linear_smallm_batch against the float64 per-M formula on exact data: odd M (the clamped second row of the pair walk, M = 1
    included), K off a multiple of 32 (the guarded second half of a lane's slice), W8 on the second trip of its K loop, bf16; one
    batch of four problems, N = 77 and 64, each with its own ldy, every output inside a sentinel allocation"""
    from dgq_amd import _lib, ops
    dt = er.DTYPES[dtype]
    Kp = (K + 127) // 128 * 128
    probs = (_lib.SmallMProblem * len(er.SMALLM_N))()
    cases, keep, bufs = [], [], []
    x = None
    for j, N in enumerate(er.SMALLM_N):
        c = er.smallm_case(M, K, N, wbits, 1)                       # (the codes depend on N through the seed: share problem 0's)
        if j == 0:
            s0 = c["s"]
            x = c["x"].to(dt).to(dev)
            assert torch.equal(x.cpu().double(), c["x"])
        c = dict(c, s=s0, qw=torch.roll(c["qw"], j, 0))
        assert er.smallm_margin(c) < 1.0
        f = lambda v: v.float().to(dev).contiguous()
        if wbits == 4:
            wp = ops.pack_weight(c["qw"].to(torch.uint8).to(dev), None, Kp, 4)
        else:
            wp = torch.zeros((N, Kp), dtype=torch.int8, device=dev)
            wp[:, :K] = c["qw"].to(torch.int8).to(dev)
        tabs = [f(c[k]) for k in ("alpha", "zw", "gamma", "vn")] + [torch.tensor([c["mdelta"]], device=dev), torch.tensor([c["mzp"]], device=dev)]
        layout = er.view_layout("ABCD"[j], M, N, dt)
        a = sentinel_alloc(layout[2], dt, dev)
        q = probs[j]
        q.wpacked, q.alpha, q.zw, q.gamma, q.vn, q.mdelta, q.mzp = [v.data_ptr() for v in [wp] + tabs]
        q.y, q.ldy, q.N, q.Kp, q.w_bits, q.a_bits = a.data_ptr() + layout[0] * a.element_size(), layout[1], N, Kp, wbits, 8
        cases.append((c, layout))
        keep.append((wp, tabs))
        bufs.append(a)
    ops._lib_call("dgq_linear_smallm_batch", _lib.ptr(x), _lib.DTYPE_CODE[dt], M, K, x.stride(0), 0, len(er.SMALLM_N),
                  ctypes.cast(probs, ctypes.c_void_p), _lib.DTYPE_CODE[dt], _lib.stream())
    torch.cuda.synchronize()
    for j, ((c, layout), a) in enumerate(zip(cases, bufs)):
        want = er.image(er.smallm_expected(c, dt), dt, layout[0], layout[1], layout[2])
        check_image("smallm M=%d K=%d W%d %s problem %d" % (M, K, wbits, dtype, j), a, want, dt, layout, M, c["N"])
