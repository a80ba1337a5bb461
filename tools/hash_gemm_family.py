"""Bit identity of the GEMM family across two library builds: prints `name sha256(output bytes)` for a few seconds of small cases that
reach every kernel of gemm_wxa8.hip / gemm_wxa8_big.hip / gemm_panel.hip / gemm_convq.hip (and one attention call per kernel file
that uses the XCD tile order) with REAL plan_act tables — flush coefficients that are not powers of two, which the exact-integer tests
cannot see reordered; a last section runs the real-time block family (gemm_blockq.hip, gemm_mx6.hip behind their quantisers) on random
data.  Run it under each build (tools/ab_libs.sh "python tools/hash_gemm_family.py" old.so -) and diff the listings.
usage: python tools/hash_gemm_family.py"""
import hashlib, os, sys
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from dgq_amd import ops, synth          # noqa: E402
from dgq_amd.plan import plan_act       # noqa: E402

dev = torch.device("cuda")
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def emit(name, *tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    print("%-72s %s" % (name, h.hexdigest()), flush=True)


def env(**kv):
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def binding(N, C, taps, mode, rows, seed, wbits=4, kind="linear", w=None):
    g = torch.Generator().manual_seed(seed)
    if w is None:
        w = torch.randn(N, C, *((3, 3) if taps == 9 else ()), generator=g) * 0.05
    wd, wz = synth.channel_minmax(w.cpu(), wbits)
    pw = ops.PackedWeight(w.to(dev), wd.to(dev), wz.to(dev), None, torch.randn(N, generator=g).to(dev), wbits, C, taps)
    K = C * taps
    pk, pm = ((1, 1, -1), (1, -1, 1)) if kind == "linear" else ((1, -1, 1), (1, 1, -1))
    if mode == "perK":
        d, z = synth._group_params(K, 16, 8, "hash|%d|%d" % (K, seed), 0)
        lay = plan_act(d.view(*pk), z.view(*pk), kind, C, taps, 8)
    elif mode == "perM":
        d, z = synth._group_params(rows, 16, 8, "hash|%d|%d" % (rows, seed), 0)
        lay = plan_act(d.view(*pm), z.view(*pm), kind, C, taps, 8)
    else:
        lay = plan_act(torch.tensor(0.037), torch.tensor(97.0), kind, C, taps, 8)
    return ops.ActBinding(lay, pw, 8)


def linear(tag, M, N, K, plans, wbits=4, modes=("perK", "perM"), dtypes=("f32", "bf16"), x=None, w=None):
    for mode in modes:
        ab = binding(N, K, 1, mode, M, M + N + K, wbits, w=w)
        for dt in dtypes:
            g = torch.Generator().manual_seed(K + M)
            xx = (torch.randn(1, M, K, generator=g) * 1.5 if x is None else x).to(dev, DT[dt])
            for plan in plans:
                env(DGQ_GEMM_FORCE=plan)
                emit("%s M%d N%d K%d W%d %s %s plan %s" % (tag, M, N, K, wbits, mode, dt, plan), ops.quant_linear(xx, ab))
    env(DGQ_GEMM_FORCE=None)


def block_layers():
    """the real-time block family (quantiser + GEMM of each format: blockq W4 / W8, mx6) on random data — δ and scales that are no
    powers of two: Linear layers (a K-padding tail; several row and column tiles), the convolution geometries of
    tests/test_block_gather_cpu.py, the three output dtypes, each epilogue extra at one shape"""
    g = torch.Generator().manual_seed(77)
    dts = dict(DT, f16=torch.float16)

    def formats(N, C, kh, kw):
        out = []
        for wbits in (4, 8):
            w = torch.randn(N, C, *((kh, kw) if kh * kw > 1 else ()), generator=g) * 0.05
            wd, wz = synth.channel_minmax(w, wbits)
            pw = ops.PackedWeight(w.to(dev), wd.to(dev), wz.to(dev), None, torch.randn(N, generator=g).to(dev), wbits, C, kh * kw)
            out.append(("blockq W%d" % wbits, ops.BlockActBinding(pw, 8)))
            if wbits == 4:
                out.append(("mx6", ops.MxActBinding(pw)))
        return out

    def run(ab, x, geom, ups, dtype, extra=None):
        q = ops._block_quant(ab, x, geom, ups=ups, pad_k=geom[4:] == (1, 1, 1, 0))
        return ops._block_gemm(ab, q, geom, dtype, extra=extra, ups=ups)

    geoms = [("linear 37x320", (37, 1, 1, 320, 1, 1, 1, 0), 0), ("linear 154x768", (154, 1, 1, 768, 1, 1, 1, 0), 0),
             ("conv 3x3 s1 p1 2x9x9x32", (2, 9, 9, 32, 3, 3, 1, 1), 0), ("conv 3x3 s2 p1 2x11x13x64", (2, 11, 13, 64, 3, 3, 2, 1), 0),
             ("conv 3x3 ups 2x8x8x32", (2, 8, 8, 32, 3, 3, 1, 1), 1), ("conv 1x1 s2 p0 1x7x9x64", (1, 7, 9, 64, 1, 1, 2, 0), 0),
             ("conv 3x3 p0 1x5x5x32", (1, 5, 5, 32, 3, 3, 1, 0), 0)]
    for name, geom, ups in geoms:
        B, H, W, C, kh, kw = geom[:6]
        x = (torch.randn(B, H >> ups, W >> ups, C, generator=g) * 1.3 + 0.2).to(dev)
        for N in ((24,) if name == "linear 37x320" else (320,) if name == "linear 154x768" else (24, 64)):
            for fmt, ab in formats(N, C, kh, kw):
                for dn, dt in dts.items():
                    emit("block %s N%d %s %s" % (name, N, fmt, dn), run(ab, x, geom, ups, dt))
    # ---- the extras: Linear 154 x 768 -> 320; GroupNorm partials on the ups convolution (M = 128)
    M, K, N = 154, 768, 320
    geom = (M, 1, 1, K, 1, 1, 1, 0)
    x = (torch.randn(M, K, generator=g) * 1.3 + 0.2).to(dev)
    res, res2 = torch.randn(M, N, generator=g).to(dev), torch.randn(M // 2, N, generator=g).to(dev)
    cgeom = (2, 8, 8, 32, 3, 3, 1, 1)
    xc = (torch.randn(2, 4, 4, 32, generator=g) * 1.3 + 0.2).to(dev)
    for (fmt, ab), (_, abc) in zip(formats(N, K, 1, 1), formats(64, 32, 3, 3)):
        emit("block extras %s residual" % fmt, run(ab, x, geom, 0, torch.float32, ops.make_extra(residual=res)))
        emit("block extras %s residual res_div 2" % fmt, run(ab, x, geom, 0, torch.float32, ops.make_extra(residual=res2, res_div=2)))
        emit("block extras %s GEGLU" % fmt, run(ab, x, geom, 0, torch.float32, ops.make_extra(geglu=True)))
        buf = torch.zeros(M, N + 72, device=dev)
        emit("block extras %s y2" % fmt, run(ab, x, geom, 0, torch.float32, ops.make_extra(y2=buf[:, 40:40 + N])), buf)
        part = torch.zeros(128 // 16, 64, 2, device=dev)
        emit("block extras %s GroupNorm partials" % fmt, run(abc, xc, cgeom, 1, torch.float32, ops.make_extra(gn_partial=part)), part)


def main():
    ops.GEMM_FUSE = False
    # ---- tile family: 18+ K tiles, a clear inside, ragged edges
    linear("tile", 203, 332, 2304, ["32,64,1", "32,64,3", "32,128,1", "64,64,1", "64,128,2", "128,64,1", "128,128,1"])
    linear("tile", 203, 332, 2304, ["32,64,1", "128,128,1"], wbits=8)
    # ---- long-K table tail (more table entries than threads): the wide golden layer's input, cut to 64 x 128
    from golden import recipes
    case = [c for c in recipes.f3_wide_cases() if c["layout"] == "perK"][0]
    inp = recipes.f3_inputs(case)
    linear("tail", 64, 128, 9216, ["128,128,1"], modes=("perK",), x=inp["x"][:1, :64], w=inp["w"][:128])
    # ---- 256-row kernel, with the caller's coefficient table bound and with its own LDS table
    table = ops.with_layer_tables
    for bound in (True, False):
        def tables(extra, ab, M, bound=bound):
            extra = table(extra, ab, M)
            if ab.mode == "perK":
                if extra is None:
                    extra = ops._lib.GemmExtra()
                    extra.res_div, extra.fq_T, extra.fq_D, extra._keep = 1, 1, 1, []
                extra.flush_coef = ab.ccoef.data_ptr() if bound else None
            return extra
        ops.with_layer_tables = tables
        linear("rows256 ccoef=%d" % bound, 300, 700, 2304, ["256,256,1"])
    ops.with_layer_tables = table
    # ---- panel (quantise-on-load): every configuration, and a three-problem launch
    ops.GEMM_FUSE = True
    env(DGQ_GEMM_FUSE_ALL="1")
    for (M, N, K) in ((203, 332, 320), (97, 1290, 1280)):
        linear("panel", M, N, K, ["F1,10,1,1", "F1,5,1,1", "F1,5,1,2", "F1,4,1,2"])
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 77, 768, generator=g).to(dev)
    binds = [binding(320, 768, 1, "perK", 77, 40 + i) for i in range(3)]
    assert ops._multi_fuses(binds, 154, 768, x.dtype, x.reshape(-1, 768))
    emit("panel multi M154 K768 x3 perK f32", *ops.quant_linear_multi(x, binds))
    env(DGQ_GEMM_FUSE_ALL=None)
    # ---- 3x3 convolution with the quantiser inside (NW = 5, 10), GroupNorm prologue + residual + partials
    ops.CONV_FUSE = True
    for (B, C, H, W) in ((2, 64, 16, 24), (1, 320, 32, 32)):
        for N in (160, 320):
            for mode in ("perK", "perM"):
                ab = binding(N, C, 9, mode, H * W, B + C + N, kind="conv")
                for dt in ("f32", "bf16"):
                    g = torch.Generator().manual_seed(C + N)
                    x = (torch.randn(B, C, H, W, generator=g) * 1.3 + 0.2).to(dev, DT[dt])
                    res = torch.randn(B, N, H, W, generator=g).to(dev, DT[dt])
                    norm = (32, 1e-5, torch.randn(C, generator=g).to(dev), torch.randn(C, generator=g).to(dev), 1)
                    assert ops.conv_act_fuses(ab, B, H, W, C, 3, 3, 1, 1, DT[dt])
                    y = ops.quant_conv2d(x, ab, 3, 3, 1, 1, norm=norm, residual=res)
                    sc, sh = ops.groupnorm_from_partials(ops._gn_of(y), 32, 1e-5, torch.ones(N, device=dev), torch.zeros(N, device=dev))
                    emit("convq %dx%dx%dx%d N%d %s %s" % (B, C, H, W, N, mode, dt), y, sc, sh)
    # ---- implicit-im2col A operand
    env(DGQ_GEMM_FORCE="64,128,1")
    ab = binding(320, 320, 9, "scalar", 256, 9, kind="conv")
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(1, 320, 16, 16, generator=g) * 1.5 + 0.3).to(dev)
    emit("implicit conv 1x320x16x16 N320 plan 64,128,1", ops.quant_conv2d(x, ab, 3, 3, 1, 1))
    # ---- split-K combine with GroupNorm partials
    env(DGQ_GEMM_FORCE="32,64,3")
    ab = binding(72, 64, 9, "perK", 256, 11, kind="conv")
    x = torch.randn(2, 64, 16, 16, generator=g).to(dev)
    y = ops.quant_conv2d(x, ab, 3, 3, 1, 1, gn_out=True)
    sc, sh = ops.groupnorm_from_partials(y._dgq_gn, 8, 1e-5, torch.ones(72, device=dev), torch.zeros(72, device=dev))
    emit("splitk + gn partials 2x64x16x16 N72 plan 32,64,3", y, sc, sh)
    env(DGQ_GEMM_FORCE=None)
    # ---- attention: the three-launch kernels (int8 and bf16x3 scores) and the one-launch kernel
    tab = lambda n: (torch.rand(n, generator=g).to(dev) * 0.02 + 0.02, torch.randint(100, 156, (n,), generator=g).float().to(dev))
    B, H, D, T, S = 2, 8, 8, 70, 77
    q, k, v = (torch.randn(B, n, H * D, generator=g).to(dev) for n in (T, S, S))
    fq = ((1,) + tab(T) + (0, 8), (1,) + tab(S - 1) + (1, 8), (2,) + tab(D) + (0, 8))
    for i8 in ("1", "0"):
        env(DGQ_ATTN_I8=i8)
        emit("attention three launches D8 T70 S77 i8=%s" % i8, ops.attention_f32(q, k, v, H, D, D ** -0.5, 1, 1, None, 8, fq=fq))
    env(DGQ_ATTN_I8=None)
    D, T, S = 160, 64, 64
    q, k, v = ((torch.randn(B, n, H * D, generator=g) * 1.1).to(dev) for n in (T, S, S))
    fq = ((1,) + tab(T) + (0, 8), (1,) + tab(S) + (0, 8), (2,) + tab(D) + (0, 8))
    for one in ("1", "0"):
        env(DGQ_ATTN_ONE=None if one == "1" else "0", DGQ_ATTN_SPLIT=None if one == "1" else "0")
        emit("attention D160 T64 S64 one-launch=%s" % one, ops.attention(q, k, v, H, D, D ** -0.5, 1, 0, None, 8, fq=fq))
    env(DGQ_ATTN_ONE=None, DGQ_ATTN_SPLIT=None)
    block_layers()


main()
