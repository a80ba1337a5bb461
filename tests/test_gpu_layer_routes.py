"""Every route a quantised Linear / Conv2d layer can take (quantiser variant, conv tile, quantiser inside the GEMM launch, GEMM tile
family, K splits) at the shapes an SD step runs, against the float64 formula of tests/layer_reference.py — not against another
route of this library.

* ``test_route_table_is_complete`` (host only): which route the library's planners give every LAYER_CASES cell, and that the
  cells together reach every route; a planner change that re-routes a case shows here as the route that lost its coverage.
* ``test_exact_layer_matrix`` (GPU): on exact-integer data (``layer_reference.exact_case``: every fp32 step of every route is
  exact) the layer output EQUALS the formula on the planner's route and on every alternative the library's switches reach; the
  code matrix and the row sums of ``ops.quant_act`` equal the reference codes, with the first wrong code located in the image.
* ``test_real_layer_*`` (GPU): real-valued tables at the same shapes within the tolerances the suite already states.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import layer_reference as lr

LAYER_CASES = lr.LAYER_CASES
TILE_DIMS = {1: (4, 8), 2: (4, 4), 3: (2, 4)}
FUSED_PLANS = ["F1,10,1,1", "F1,5,1,1", "F1,5,1,2", "F1,4,1,2"]
DUMMY = 256                                      # a non-null pointer value for the host planners (never dereferenced)


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


@pytest.fixture(scope="module")
def dev():
    from dgq_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


# ----------------------------------------------------------------------------------------------- host planners
def _conv_tile_geo(lib, B, Ho, Wo, C, k, stride, Kp):
    """(tile id, has a partial tile) of the block-staged conv quantiser: dgq_quant_act_conv_tile, and the 2 x 4 tile where the
    4 x 4 one leaves the grid below 256 workgroups.  That second rule is a COPY of csrc/quant_act.hip: conv_tile_geo — the library
    exports the tile of a channel count, not of a geometry, and the spy can confirm variant 5 but not the tile that launched.  Whoever
    changes conv_tile_geo changes this function with it; an export of the geometry's tile would replace it."""
    pw = ctypes.c_int(0)
    t = lib.dgq_quant_act_conv_tile(C, k, k, stride, Kp, ctypes.byref(pw))
    tiles = lambda th, tw: B * (-(-Ho // th)) * (-(-Wo // tw))
    if t == 2 and tiles(4, 4) < 256 and tiles(2, 4) >= 256:
        t = 3
    if t == 0:
        return 0, False
    th, tw = TILE_DIMS[t]
    return t, bool(Ho % th or Wo % tw)


def quantiser_route(B, H, W, C, k, stride, pad, Kp, per_k, L, bits, ups=False, pre_act=0, ln=False, pre_scale=False):
    """What ops.quant_act asks the library before it allocates: (variant, K splits, conv tile, partial) — None where the folded
    upsample has no form for the variant."""
    from dgq_amd import _lib, ops
    lib = _lib.load()
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    M = B * Ho * Wo
    a = _lib.QuantActArgs()
    a.x, a.x_dtype, a.B, a.H, a.W, a.C, a.kh, a.kw, a.stride, a.pad = DUMMY, 0, B, H, W, C, k, k, stride, pad
    if per_k:
        a.ksrc = a.koff = a.klds = a.kdst = DUMMY
    tile, partial = _conv_tile_geo(lib, B, Ho, Wo, C, k, stride, Kp) if k > 1 else (0, False)
    if k > 1 and C % 4 == 0 and tile:
        a.kpat = DUMMY
    a.Kp, a.per_m, a.delta, a.zp, a.L, a.bits = Kp, 0 if per_k else 1, DUMMY, DUMMY, 1 if per_k else L, bits
    a.pre_act = pre_act
    if pre_scale:
        a.pre_scale = a.pre_shift = DUMMY
    if ln:
        a.ln_gamma, a.ln_beta, a.ln_eps = DUMMY, DUMMY, 1e-5
    a.ups, a.ksplits, a.codes, a.rowsum = 1 if ups else 0, 1, DUMMY, DUMMY
    parts = ops.quant_splits(a, M)                 # the rule of ops.quant_act and ops.quant_linear_multi itself
    if parts is None:
        return None
    v = lib.dgq_quant_act_variant(ctypes.byref(a))
    return v, parts, (tile if v == 5 else 0), (partial if v == 5 else False)


def host_route(case, d, dtype=torch.float32):
    """The route of one LAYER_CASES cell as the library's host planners give it (no GPU): dict(M, K, Kp, variant, act_ksplits, tile,
    partial, act_fuses, conv_act_fuses, implicit, gemm_splits).  ``variant`` is the quantiser of the two-launch form (the fused forms
    make no quantiser launch)."""
    from dgq_amd import _lib, ops
    from dgq_amd.plan import plan_act, round_up, KTILE
    lib = _lib.load()
    B, H, W, Ho, Wo, M, K, taps = lr.geometry(case)
    lin = case["kind"] == "linear"
    C, k, stride, pad = (K, 1, 1, 0) if lin else (case["C"], case["k"], case["stride"], case["pad"])
    N, layout, abits, wbits = case["N"], d["layout"], d["abits"], d["wbits"]
    per_k = layout == "perK"
    Kp = plan_act(d["adelta"], d["azp"], case["kind"], C, taps, abits).Kp if per_k else round_up(K, KTILE)
    dt = _lib.DTYPE_CODE[dtype]
    L = 1 if per_k else d["adelta"].numel()
    r = dict(M=M, K=K, Kp=Kp, per_k=per_k, implicit=False, act_fuses=False, conv_act_fuses=False)
    folded = (not lin) and case["upsample"] and layout != "scalar" and taps > 1
    if lin:
        Bq, Hq, Wq = M, 1, 1
    else:
        Bq, Hq, Wq = B, H, W
    q = quantiser_route(Bq, Hq, Wq, C, k, stride, pad, Kp, per_k, L, abits, ups=folded)
    if q is None:                                  # the folded upsample has no form here: the layer materialises it
        folded = False
        q = quantiser_route(Bq, Hq, Wq, C, k, stride, pad, Kp, per_k, L, abits)
    r["folded_upsample"] = folded
    if wbits == 4 and ops.GEMM_PANEL and ops.GEMM_FUSE:
        if taps == 1 and C % 4 == 0 and stride == 1 and pad == 0:
            r["act_fuses"] = bool(lib.dgq_gemm_act_fuses(M, N, C, Kp, wbits, 0 if per_k else 1, 1, dt, dt))
        if taps > 1 and not folded and layout != "scalar" and ops.CONV_FUSE:
            r["conv_act_fuses"] = bool(lib.dgq_gemm_conv_act_fuses(B, H, W, C, k, k, stride, pad, N, Kp, wbits, 0 if per_k else 1, dt, dt))
    z = float(d["azp"].reshape(-1)[0])
    if layout == "scalar" and taps > 1 and C % 16 == 0 and wbits == 4 and ops.CONV_IMPLICIT and 0 <= round(z) <= 2 ** abits - 1:
        r["implicit"] = True                       # the input is quantised once per pixel, as a 1x1 layer in natural order
        r["materialised"] = q[:2]                  # (variant, K splits) of the unfolded operand's quantiser with CONV_IMPLICIT off
        q = quantiser_route(B, H, W, C, 1, 1, 0, round_up(C, KTILE), False, 1, abits)
    r["variant"], r["act_ksplits"], r["tile"], r["partial"] = q
    r["gemm_splits"] = lib.dgq_gemm_plan_splits(M, N, Kp, wbits, 0 if per_k else 1, ops.WORKSPACE_BYTES)
    return r


def forced_tile_plans(route, N, wbits, workspace_bytes):
    """the DGQ_GEMM_FORCE tile plans the exact matrix runs on a cell: the 256-row kernel (W4), a 64- and a 128-row tile, and a K split
    where K has four tiles to split and the slabs fit the workspace.  Every one of them must run: none is optional."""
    plans = (["256,256,1"] if wbits == 4 else []) + ["64,64,1", "128,128,1"]
    if route["Kp"] // 128 >= 4 and 4 * route["M"] * N * 4 <= workspace_bytes:
        plans.append("64,64,4")
    return plans


def f_plans_apply(case, route, wbits):
    """the F plans of FUSED_PLANS run where the layer is Linear-like, W4, and the library takes quantise-on-load at all for the shape
    (dgq_gemm_act_fuses under DGQ_GEMM_FUSE_ALL=1, which the caller has set)"""
    from dgq_amd import _lib
    if wbits != 4 or lr.geometry(case)[7] != 1:
        return False
    K = lr.geometry(case)[6]
    return K % 4 == 0 and bool(_lib.load().dgq_gemm_act_fuses(route["M"], case["N"], K, route["Kp"], 4, 0 if route["per_k"] else 1, 1, 0, 0))


def test_route_table_is_complete(monkeypatch):
    """Host only.  Over LAYER_CASES x layouts the planners must reach: quantiser variants 0 .. 5 (variant 1 through the GEGLU prologue
    at K = 5120, which only the real-valued tests can run), conv tiles 1 .. 3 each with and without a partial tile, a K-split
    quantiser, the conv and the Linear quantise-inside-the-GEMM forms taken and declined, GEMM K splits 1 and > 1."""
    monkeypatch.delenv("DGQ_GEMM_FORCE", raising=False)
    monkeypatch.delenv("DGQ_GEMM_FUSE_ALL", raising=False)
    rows = []
    for name, layout, abits, wbits in lr.exact_params():
        if (abits, wbits) != (8, 4):
            continue
        case = lr.CASES_BY_NAME[name]
        rows.append((name, layout, host_route(case, lr.exact_tables(name, layout, abits, wbits))))
    print("\n%-34s %-6s %6s %6s %6s  v ks tile part lin-fuse conv-fuse implicit gemm-splits" % ("case", "layout", "M", "K", "Kp"))
    for name, layout, r in rows:
        print("%-34s %-6s %6d %6d %6d  %d %2d %4d %4s %8s %9s %8s %d" % (name, layout, r["M"], r["K"], r["Kp"], r["variant"], r["act_ksplits"], r["tile"],
                                                                       "yes" if r["partial"] else "-", r["act_fuses"], r["conv_act_fuses"], r["implicit"],
                                                                       r["gemm_splits"]))
    geglu = prologue_route("geglu", lr.CASES_BY_NAME["linear_m512_k5120_n1280"], lr.real_tables(lr.CASES_BY_NAME["linear_m512_k5120_n1280"], "perK"))
    print("GEGLU prologue, 512 x (2 x 5120), per-K table of the GPU case: variant %d, %d K splits" % geglu[:2])
    variants = {r["variant"] for _, _, r in rows} | {geglu[0]}
    assert variants >= {0, 1, 2, 3, 4, 5}, "quantiser variants without a case: %s" % sorted({0, 1, 2, 3, 4, 5} - variants)
    assert geglu[0] == 1, "the GEGLU prologue case of test_real_layer_folded_prologue no longer takes variant 1: %s" % (geglu,)
    tiles = {(r["tile"], r["partial"]) for _, _, r in rows if r["variant"] == 5}
    want = {(t, p) for t in (1, 2, 3) for p in (False, True)}
    assert tiles >= want, "conv tiles (id, partial) without a case: %s" % sorted(want - tiles)
    assert any(r["act_ksplits"] > 1 for _, _, r in rows), "no case with a K-split quantiser"
    for key in ("conv_act_fuses", "act_fuses", "implicit"):
        assert {r[key] for _, _, r in rows} == {False, True}, "%s is %s on every case" % (key, {r[key] for _, _, r in rows})
    assert {r["gemm_splits"] > 1 for _, _, r in rows} == {False, True}, "GEMM K splits: every case on one side"
    assert any(r.get("folded_upsample") for _, _, r in rows), "no case reads its input through the folded 2x upsample"
    # every forced plan of the exact matrix runs on at least one cell (they are never optional where they apply)
    from dgq_amd import ops
    forced = {p for name, _, r in rows for p in forced_tile_plans(r, lr.CASES_BY_NAME[name]["N"], 4, ops.WORKSPACE_BYTES)}
    assert forced == {"256,256,1", "64,64,1", "128,128,1", "64,64,4"}, forced
    monkeypatch.setenv("DGQ_GEMM_FUSE_ALL", "1")
    n_f = sum(1 for name, _, r in rows if f_plans_apply(lr.CASES_BY_NAME[name], r, 4))
    print("the F plans %s run on %d cells" % (FUSED_PLANS, n_f))
    assert n_f >= 3, "the quantise-on-load plans run on %d cells" % n_f


def prologue_route(fold, case, tables):
    """(variant, K splits, ...) of the quantiser of a layer with a folded prologue, for the very table the GPU test runs under"""
    from dgq_amd.plan import plan_act, round_up, KTILE
    B, H, W, Ho, Wo, M, K, taps = lr.geometry(case)
    lin = case["kind"] == "linear"
    C, k, stride, pad = (K, 1, 1, 0) if lin else (case["C"], case["k"], case["stride"], case["pad"])
    per_k = tables["layout"] == "perK"
    Kp = plan_act(tables["adelta"], tables["azp"], case["kind"], C, taps, tables["abits"]).Kp if per_k else round_up(K, KTILE)
    L = 1 if per_k else tables["adelta"].numel()
    Bq, Hq, Wq = (M, 1, 1) if lin else (B, H, W)
    return quantiser_route(Bq, Hq, Wq, C, k, stride, pad, Kp, per_k, L, tables["abits"], pre_act={"gn_silu": 1, "ln": 0, "geglu": 2}[fold],
                           ln=(fold == "ln"), pre_scale=(fold == "gn_silu"))


# ----------------------------------------------------------------------------------------------- GPU helpers
class Spy:
    """ops._lib_call wrapper: the entry points a layer call makes; for dgq_quant_act_batch the variant dgq_quant_act_variant reports
    for the very argument struct, for dgq_gemm_wxa8 whether the launch carries its own quantiser / the implicit-conv descriptor."""

    def __init__(self, ops, _lib):
        self.orig, self.lib, self.calls = ops._lib_call, _lib.load(), []

    def __call__(self, name, *args):
        rec = dict(name=name)
        if name == "dgq_quant_act_batch":
            a = args[1]._obj
            rec.update(variant=self.lib.dgq_quant_act_variant(ctypes.byref(a)), ksplits=int(a.ksplits))
        elif name == "dgq_gemm_wxa8":
            ex = args[24]
            rec.update(fused=bool(ex is not None and ex._obj.act), implicit=bool(ex is not None and ex._obj.conv))
        self.calls.append(rec)
        return self.orig(name, *args)

    def take(self):
        out, self.calls = self.calls, []
        return out


def build_layer(ops, case, d, dev):
    from dgq_amd.plan import plan_act
    B, H, W, Ho, Wo, M, K, taps = lr.geometry(case)
    C = K if case["kind"] == "linear" else case["C"]
    pw = ops.PackedWeight(d.get("w_raw", d["w"]).to(dev), d["wdelta"].to(dev), d["wzp"].to(dev), None, d["bias"].to(dev), d["wbits"], C, taps)
    lay = plan_act(d["adelta"], d["azp"], case["kind"], C, taps, d["abits"])
    return lay, ops.ActBinding(lay, pw, d["abits"])


def run_layer(ops, case, ab, x, res, **kw):
    if case["kind"] == "linear":
        return ops.quant_linear(x, ab, residual=res, **kw)
    return ops.quant_conv2d(x, ab, case["k"], case["k"], case["stride"], case["pad"], residual=res, upsample=case["upsample"], **kw)


def run_quantiser(ops, case, ab, x, pre=None, ln=None):
    """ops.quant_act on the layer input as quant_linear / quant_conv2d hand it over -> (codes, rowsum, folded)"""
    B, H, W, Ho, Wo, M, K, taps = lr.geometry(case)
    if case["kind"] == "linear":
        xs = x.reshape(M, -1).contiguous()
        return ops.quant_act(xs, M, 1, 1, K, 1, 1, 1, 0, ab, pre, ln)[:2] + (False,)
    k, s, p = case["k"], case["stride"], case["pad"]
    xc = x.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
    if case["upsample"]:
        qa = ops.quant_act(xc, B, H, W, case["C"], k, k, s, p, ab, pre, ups=True) if (k > 1 and ab.mode != "scalar") else None
        if qa is not None:
            return qa[:2] + (True,)
        xc = F.interpolate(x, scale_factor=2.0, mode="nearest").contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
    return ops.quant_act(xc, B, H, W, case["C"], k, k, s, p, ab, pre)[:2] + (False,)


def describe_code_mismatch(case, got, want, kref, tile):
    """the first wrong code of a [M][K_ref] comparison, in the image: row -> (b, ho, wo), column -> (c, dh, dw)"""
    bad = (got != want).nonzero()
    m, j = int(bad[0, 0]), int(bad[0, 1])
    kr = int(kref[j])
    msg = "%d of %d codes differ; first at row %d, k_ref %d: got %d, want %d" % (bad.shape[0], got.numel(), m, kr, int(got[m, j]), int(want[m, j]))
    if case["kind"] == "conv":
        B, H, W, Ho, Wo, M, K, taps = lr.geometry(case)
        k, s, p = case["k"], case["stride"], case["pad"]
        b, l = divmod(m, Ho * Wo)
        ho, wo = divmod(l, Wo)
        c, tap = divmod(kr, taps)
        dh, dw = divmod(tap, k)
        hi, wi = ho * s - p + dh, wo * s - p + dw
        outside = not (0 <= hi < H and 0 <= wi < W)
        msg += " = (b %d, ho %d, wo %d) x (c %d, dh %d, dw %d): input pixel (%d, %d) %s the image" % (b, ho, wo, c, dh, dw, hi, wi,
                                                                                                    "OUTSIDE" if outside else "inside")
        if tile:
            th, tw = TILE_DIMS[tile]
            part = (ho // th == Ho // th and Ho % th) or (wo // tw == Wo // tw and Wo % tw)
            msg += ", %s tile of the %d x %d grid" % ("a PARTIAL" if part else "a full", th, tw)
    return msg


def check_codes(case, lay, codes, rowsum, q_rows, d, tile, what):
    """centred codes == q − 2^(b−1) through kperm (natural order for per-M / scalar), padding columns zero, row sums exact"""
    from dgq_amd.plan import natural_kperm
    B, H, W, Ho, Wo, M, K, taps = lr.geometry(case)
    C = K if case["kind"] == "linear" else case["C"]
    off = 2 ** (d["abits"] - 1)
    kperm = lay.kperm if lay.mode == "perK" else natural_kperm(C, taps)
    m = kperm >= 0
    got = codes.cpu().int()
    want = (q_rows[:, kperm[m].long()] - off).int()
    if not torch.equal(got[:, m], want):
        raise AssertionError("%s: %s" % (what, describe_code_mismatch(case, got[:, m], want, kperm[m], tile)))
    assert int(got[:, ~m].abs().sum()) == 0, "%s: padding columns are not zero" % what
    s = (q_rows - off).double()
    want_sum = (s * d["adelta"].reshape(1, -1).double()).sum(1) if lay.mode == "perK" else s.sum(1)
    got_sum = rowsum.cpu().double().sum(0)
    assert torch.equal(got_sum, want_sum), "%s: row sums differ on %d rows, first %d" % (what, int((got_sum != want_sum).sum()),
                                                                                          int((got_sum != want_sum).nonzero()[0]))


# ----------------------------------------------------------------------------------------------- the exact matrix
@pytest.mark.gpu
@pytest.mark.parametrize("name,layout,abits,wbits", lr.exact_params(), ids=lambda v: str(v))
def test_exact_layer_matrix(name, layout, abits, wbits, dev, monkeypatch, capsys):
    """One LAYER_CASES cell on exact-integer data (layer_reference.exact_case asserts the precondition): through PackedWeight, plan_act,
    ActBinding and quant_linear / quant_conv2d with bias, residual and ``upsample=``, y must EQUAL the float64 formula on
    the planner's route, the two-launch form, the materialised form of a scalar convolution, the 256-row GEMM, a 64- and a 128-row
    tile, a K-split plan and (fused Linear) the F plans; the spy asserts that the route the host planners name is the one that ran.
    16-bit tensors in and out on the ``half`` cases: y == the formula rounded once.  ops.quant_act's codes and row sums against the
    reference codes, also behind an exact GroupNorm-style prologue (``gn`` cases): a tap outside the image is the code of 0.0."""
    from dgq_amd import _lib, ops
    monkeypatch.delenv("DGQ_GEMM_FORCE", raising=False)
    monkeypatch.delenv("DGQ_GEMM_FUSE_ALL", raising=False)
    case = lr.CASES_BY_NAME[name]
    d = lr.exact_case(name, layout, abits, wbits)
    assert d["margin"] < 1.0
    y_ref, q = lr.reference_of(d, case)
    q_rows = lr.codes_rows(q, case)
    lay, ab = build_layer(ops, case, d, dev)
    assert torch.equal(ab.pw.codes.cpu().long(), d["qw"]), "the weight quantiser did not find the recipe's codes"
    route = host_route(case, d)
    spy = Spy(ops, _lib)
    monkeypatch.setattr(ops, "_lib_call", spy)
    M, N = route["M"], case["N"]
    ran = []

    def run(label, dtype=torch.float32, fused=None, implicit=None, quantiser=None):
        x, res = d["x"].to(dev).to(dtype), d["residual"].to(dev).to(dtype)
        spy.take()
        y = run_layer(ops, case, ab, x, res)                       # a plan the library refuses fails the test: none is optional
        torch.cuda.synchronize()
        calls = spy.take()
        gemm = [c for c in calls if c["name"] == "dgq_gemm_wxa8"]
        quant = [c for c in calls if c["name"] == "dgq_quant_act_batch"]
        assert len(gemm) == 1, (label, calls)
        if fused is not None:
            assert gemm[0]["fused"] == fused, "%s: quantiser inside the GEMM launch: %s, expected %s" % (label, gemm[0]["fused"], fused)
            assert len(quant) == (0 if fused else 1), "%s: %d quantiser launches" % (label, len(quant))
        if implicit is not None:
            assert gemm[0]["implicit"] == implicit, (label, gemm[0])
        if quant:
            want_q = quantiser if quantiser is not None else (route["variant"], route["act_ksplits"])
            assert (quant[0]["variant"], quant[0]["ksplits"]) == want_q, (label, quant[0], want_q, route)
        want = y_ref if dtype == torch.float32 else y_ref.to(dtype)
        got = y.cpu().double() if dtype == torch.float32 else y.cpu()
        if not torch.equal(got, want):
            bad = (got != want)
            idx = [int(v) for v in bad.nonzero()[0]]
            raise AssertionError("%s/%s %s [%s]: y differs from the formula on %d of %d elements, first at %s: got %r, want %r; route %s"
                                 % (name, layout, label, dtype, int(bad.sum()), bad.numel(), idx, float(got[tuple(idx)]), float(want[tuple(idx)]), route))
        ran.append(label if dtype == torch.float32 else "%s/%s" % (label, str(dtype).replace("torch.", "")))

    fused = route["act_fuses"] or route["conv_act_fuses"]
    run("planner", fused=fused, implicit=route["implicit"])
    if case.get("half") and (abits, wbits) == (8, 4):
        for dtype in (torch.bfloat16, torch.float16):
            rh = host_route(case, d, dtype)
            run("planner", dtype, fused=rh["act_fuses"] or rh["conv_act_fuses"], implicit=rh["implicit"])
    monkeypatch.setattr(ops, "GEMM_FUSE", False)
    monkeypatch.setattr(ops, "CONV_FUSE", False)
    if fused:
        run("two-launch", fused=False, implicit=route["implicit"])
        if case.get("half") and (abits, wbits) == (8, 4):
            for dtype in (torch.bfloat16, torch.float16):
                run("two-launch", dtype, fused=False)
    if route["implicit"]:
        monkeypatch.setattr(ops, "CONV_IMPLICIT", False)
        run("materialised", fused=False, implicit=False, quantiser=route["materialised"])
        monkeypatch.setattr(ops, "CONV_IMPLICIT", True)
    for plan in forced_tile_plans(route, N, wbits, ops.WORKSPACE_BYTES):
        monkeypatch.setenv("DGQ_GEMM_FORCE", plan)
        run(plan, fused=False)
    monkeypatch.delenv("DGQ_GEMM_FORCE")
    monkeypatch.setattr(ops, "GEMM_FUSE", True)
    monkeypatch.setattr(ops, "CONV_FUSE", True)
    monkeypatch.setenv("DGQ_GEMM_FUSE_ALL", "1")
    if f_plans_apply(case, route, wbits):
        assert ops.act_fuses(ab, M, lr.geometry(case)[6], torch.float32)
        run("fuse-all", fused=True)
        for plan in FUSED_PLANS:
            monkeypatch.setenv("DGQ_GEMM_FORCE", plan)
            run(plan, fused=True)
        monkeypatch.delenv("DGQ_GEMM_FORCE")
    monkeypatch.delenv("DGQ_GEMM_FUSE_ALL")

    # ---- the code matrix and the row sums of the quantiser launch itself
    x = d["x"].to(dev)
    spy.take()
    codes, rowsum, folded = run_quantiser(ops, case, ab, x)
    torch.cuda.synchronize()
    qc = [c for c in spy.take() if c["name"] == "dgq_quant_act_batch"]
    if not route["implicit"]:
        assert (qc[0]["variant"], qc[0]["ksplits"], folded) == (route["variant"], route["act_ksplits"], route["folded_upsample"]), (qc, route)
    tile = route["tile"] if qc[0]["variant"] == 5 else 0
    check_codes(case, lay, codes, rowsum, q_rows, d, tile, "%s/%s quantiser variant %d" % (name, layout, qc[0]["variant"]))
    ran.append("codes(v%d)" % qc[0]["variant"])
    if case.get("gn") and (abits, wbits) == (8, 4):
        g = torch.Generator().manual_seed(5)
        B, C = case["B"], case["C"]
        scale = (2.0 ** torch.randint(0, 2, (B, C), generator=g).double()).float()
        shift = (2 * torch.randint(-3, 4, (B, C), generator=g)).float()
        xn = d["x"] * scale[:, :, None, None] + shift[:, :, None, None]
        _, qn = lr.reference_of(d, case, x=xn)                      # F.unfold pads with 0.0 BEHIND the norm
        spy.take()
        codes, rowsum, _ = run_quantiser(ops, case, ab, x, pre=(scale.to(dev), shift.to(dev), 0))
        torch.cuda.synchronize()
        v = [c for c in spy.take() if c["name"] == "dgq_quant_act_batch"][0]["variant"]
        check_codes(case, lay, codes, rowsum, lr.codes_rows(qn, case), d, route["tile"] if v == 5 else 0,
                    "%s/%s quantiser variant %d behind a scale / shift prologue" % (name, layout, v))
        ran.append("prologue-codes(v%d)" % v)
    with capsys.disabled():
        print("\nROUTES %s %s a%dw%d profile %d margin %.2f: %s | asserted: variant %d ks %d tile %d%s lin-fuse %s conv-fuse %s implicit %s splits %d"
              % (name, layout, abits, wbits, d["profile"], d["margin"], ", ".join(ran), route["variant"], route["act_ksplits"], route["tile"],
                 "p" if route["partial"] else "", route["act_fuses"], route["conv_act_fuses"], route["implicit"], route["gemm_splits"]))


# ----------------------------------------------------------------------------------------------- real-valued tables
REAL_CELLS = [("conv3x3_b2_c64_64x64_s1_n64", "perK"), ("conv3x3_b2_c64_64x64_s1_n64", "perM"), ("conv3x3_b2_c320_64x64_s1_n320", "perK"),
              ("conv3x3_b2_c320_64x64_s1_n320", "perM"), ("conv3x3_b2_c640_32x32_s1_n640", "perK"), ("conv3x3_b2_c640_16x16_s1_n1280", "perK"),
              ("conv3x3_b2_c320_46x90_s1_n320", "perK"), ("conv3x3_b2_c320_63x63_s2_n320", "perK"), ("conv3x3_b2_c640_32x32_s1_n640_ups", "perK"),
              ("conv3x3_b2_c320_64x64_s1_n320", "scalar"), ("linear_m8192_k320_n320", "perK"), ("linear_m8192_k320_n320", "perM"),
              ("linear_m2048_k2560_n640", "perK"), ("linear_m512_k5120_n1280", "perK")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,layout", REAL_CELLS)
def test_real_layer_codes_and_output(name, layout, dev, monkeypatch, capsys):
    """torch.randn data under synth._group_params tables: the codes of ops.quant_act EQUAL orc.uaq_codes (the claim of
    test_f3_layers_vs_reference, here on the production variants) and y is within 2e-5 relative L2 of the float64 formula on the
    planner's route and on the two-launch form (the bound of test_f3_layers_vs_reference)."""
    from dgq_amd import _lib, ops
    monkeypatch.delenv("DGQ_GEMM_FORCE", raising=False)
    monkeypatch.delenv("DGQ_GEMM_FUSE_ALL", raising=False)
    case = lr.CASES_BY_NAME[name]
    d = lr.real_case(case, layout)
    y_ref, q = lr.reference_of(d, case)
    lay, ab = build_layer(ops, case, d, dev)
    route = host_route(case, d)
    spy = Spy(ops, _lib)
    monkeypatch.setattr(ops, "_lib_call", spy)
    x, res = d["x"].to(dev), d["residual"].to(dev)
    codes, rowsum, _ = run_quantiser(ops, case, ab, x)
    torch.cuda.synchronize()
    v = [c for c in spy.take() if c["name"] == "dgq_quant_act_batch"][0]["variant"]
    if not route["implicit"]:
        assert v == route["variant"], (v, route)
    from dgq_amd.plan import natural_kperm
    B, H, W, Ho, Wo, M, K, taps = lr.geometry(case)
    kperm = lay.kperm if lay.mode == "perK" else natural_kperm(K // taps, taps)
    m = kperm >= 0
    got, want = codes.cpu().int()[:, m], (lr.codes_rows(q, case)[:, kperm[m].long()] - 2 ** (d["abits"] - 1)).int()
    if not torch.equal(got, want):
        raise AssertionError(describe_code_mismatch(case, got, want, kperm[m], route["tile"] if v == 5 else 0))
    errs = []
    for fuse in (True, False):
        monkeypatch.setattr(ops, "GEMM_FUSE", fuse)
        monkeypatch.setattr(ops, "CONV_FUSE", fuse)
        y = run_layer(ops, case, ab, x, res)
        torch.cuda.synchronize()
        errs.append(rel_l2(y.cpu(), y_ref))
    with capsys.disabled():
        print("\nREAL %s %s: variant %d, rel-L2 vs float64 planner %.3g two-launch %.3g" % (name, layout, v, errs[0], errs[1]))
    assert max(errs) < 2e-5, errs


PROLOGUE_CELLS = [("gn_silu", "conv3x3_b2_c64_64x64_s1_n64", "perK"), ("gn_silu", "conv3x3_b2_c320_64x64_s1_n320", "perK"),
                  ("gn_silu", "conv3x3_b2_c320_64x64_s1_n320", "perM"), ("gn_silu", "conv3x3_b2_c640_32x32_s1_n640", "perK"),
                  ("gn_silu", "conv3x3_b2_c640_16x16_s1_n1280", "perK"), ("gn_silu", "conv1x1_b2_c320_64x64_s1_n320", "perK"),
                  ("ln", "linear_m8192_k320_n320", "perK"), ("ln", "linear_m2048_k640_n640", "perK"), ("ln", "linear_m512_k1280_n1280", "perM"),
                  ("geglu", "linear_m2048_k1280_n320", "perK"), ("geglu", "linear_m512_k5120_n1280", "perK")]


@pytest.mark.gpu
@pytest.mark.parametrize("fold,name,layout", PROLOGUE_CELLS)
def test_real_layer_folded_prologue(fold, name, layout, dev, monkeypatch, capsys):
    """GroupNorm + SiLU (``norm=``), LayerNorm (``ln=``) and the GEGLU prologue (``pre_act=2``) folded into the quantiser, against
    F.group_norm / F.silu / F.layer_norm / F.gelu in fp32 on the CPU followed by the float64 formula: codes differ by at most one step
    on < 1e-3 of the elements and y is within 2e-3 (the bounds of test_fused_groupnorm_silu_quant_codes /
    test_fused_layernorm_quant_codes); planner's route and the two-launch form."""
    from dgq_amd import _lib, ops
    monkeypatch.delenv("DGQ_GEMM_FORCE", raising=False)
    monkeypatch.delenv("DGQ_GEMM_FUSE_ALL", raising=False)
    case = lr.CASES_BY_NAME[name]
    d = lr.real_case(case, layout)
    want_v = prologue_route(fold, case, d)[:2]
    g = torch.Generator().manual_seed(17)
    B, H, W, Ho, Wo, M, K, taps = lr.geometry(case)
    x, res = d["x"], d["residual"]
    kw, pre, ln = {}, None, None
    if fold == "gn_silu":
        C = case["C"]
        gam, bet = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
        x_in = F.silu(F.group_norm(x, 32, gam, bet, 1e-5))
        kw = dict(norm=(32, 1e-5, gam.to(dev), bet.to(dev), 1))
    elif fold == "ln":
        gam, bet = 1 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
        x_in = F.layer_norm(x, (K,), gam, bet, 1e-5)
        ln = (gam.to(dev), bet.to(dev), 1e-5)
        kw = dict(ln=ln)
    else:
        x = torch.cat([x, torch.randn(x.shape, generator=g)], dim=-1)                 # [1, M, 2K]: value ‖ gate
        x_in = x[..., :K] * F.gelu(x[..., K:])
        pre = (None, None, 2)
        kw = dict(pre_act=2)
    y_ref, q = lr.reference_of(d, case, x=x_in)
    lay, ab = build_layer(ops, case, d, dev)
    spy = Spy(ops, _lib)
    monkeypatch.setattr(ops, "_lib_call", spy)
    xg, rg = x.to(dev), res.to(dev)
    if fold == "gn_silu":
        xc = xg.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
        sc, sh = ops.groupnorm_scale_shift(xc, B, H * W, case["C"], 32, 1e-5, kw["norm"][2], kw["norm"][3])
        pre = (sc, sh, 1)
    spy.take()
    codes, rowsum, _ = run_quantiser(ops, case, ab, xg, pre=pre, ln=ln)
    torch.cuda.synchronize()
    qc = [c for c in spy.take() if c["name"] == "dgq_quant_act_batch"][0]
    v = qc["variant"]
    assert (v, qc["ksplits"]) == want_v, "the quantiser that ran (variant, K splits) %s is not the host planners' %s" % ((v, qc["ksplits"]), want_v)
    from dgq_amd.plan import natural_kperm
    kperm = lay.kperm if lay.mode == "perK" else natural_kperm(K // taps, taps)
    m = kperm >= 0
    diff = (codes.cpu().int()[:, m] - (lr.codes_rows(q, case)[:, kperm[m].long()] - 2 ** (d["abits"] - 1)).int()).abs()
    share = float((diff > 0).float().mean())
    errs = []
    for fuse in (True, False):
        monkeypatch.setattr(ops, "GEMM_FUSE", fuse)
        monkeypatch.setattr(ops, "CONV_FUSE", fuse)
        y = run_layer(ops, case, ab, xg, rg, **kw)
        torch.cuda.synchronize()
        errs.append(rel_l2(y.cpu(), y_ref))
    with capsys.disabled():
        print("\nPROLOGUE %s %s %s: variant %d, share of differing codes %.3g (max step %d), rel-L2 planner %.3g two-launch %.3g"
              % (fold, name, layout, v, share, int(diff.max()), errs[0], errs[1]))
    assert int(diff.max()) <= 1 and share < 1e-3, (int(diff.max()), share)
    assert max(errs) < 2e-3, errs
