"""Bit identity of the activation-quantiser family across two library builds: prints `name sha256(output bytes)` for a few seconds of
small cases that reach every kernel of quant_act.hip (each case asks dgq_quant_act_variant first and asserts the kernel it is named
for), act_rowparams.hip, quant_block.hip and quant_mx6.hip, with REAL plan_act tables whose δ are no powers of two — a reordered per-K
row sum shows.  Hashed: codes and row sums; the (δ, z) tables of the row mode; codes, {δ, β} table, ρ and the dequantised x̂ of the block
mode; codes, scales and x̂ of the MXFP6 mode.
Run it under each build (tools/ab_libs.sh "python tools/hash_quant_family.py" old.so -) and diff the listings.
usage: python tools/hash_quant_family.py [--plan]      --plan: print every case's kernel variant and launch nothing (needs no GPU)"""
import ctypes, hashlib, os, sys, types
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgq_amd import _lib, ops, synth                                   # noqa: E402
from dgq_amd.plan import plan_act, natural_kperm, natural_ksrc    # noqa: E402

PLAN = "--plan" in sys.argv
dev = torch.device("cpu" if PLAN else "cuda")
DTYPES = (("f32", torch.float32), ("f16", torch.float16), ("bf16", torch.bfloat16))
F32 = DTYPES[:1]


def emit(name, *tensors):
    if PLAN:
        print(name, flush=True)
        return
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    print("%-84s %s" % (name, h.hexdigest()), flush=True)


class Tables(ops.ActBinding):
    """The quantiser side of an ActBinding — plan_act's tables on the device and the cached gather tables — without a weight."""

    def __init__(self, mode, kind, C, taps, rows, abits, key, G=16):
        pk, pm = ((1, 1, -1), (1, -1, 1)) if kind == "linear" else ((1, -1, 1), (1, 1, -1))
        if mode == "perK":
            d, z = synth._group_params(C * taps, G, abits, "hq|%s" % key, 0)
            lay = plan_act(d.view(*pk), z.view(*pk), kind, C, taps, abits)
            self.Kp, self.ksrc, self.cdelta, self.czp = lay.Kp, lay.ksrc.to(dev), lay.cdelta.to(dev), lay.czp.to(dev)
        else:
            if mode == "perM":
                d, z = synth._group_params(rows, 16, abits, "hq|%s" % key, 0)
                lay = plan_act(d.view(*pm), z.view(*pm), kind, C, taps, abits)
            else:
                lay = plan_act(torch.tensor(0.037), torch.tensor(float(2 ** (abits - 1) - 31)), kind, C, taps, abits)
            self.Kp, self.ksrc = natural_kperm(C, taps).numel(), None
            self.mdelta, self.mzp, self.L = lay.mdelta.to(dev).contiguous(), lay.mzp.to(dev).contiguous(), lay.L
        self.mode, self.abits, self._koff = lay.mode, abits, {}
        self.pw = types.SimpleNamespace(codes=torch.empty(0, device=dev))


def data(shape, seed, dtype, scale=1.5, shift=0.2):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).to(dev, dtype)


def groupnorm(B, C, seed, act=1):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(B, C, generator=g) + 0.5).to(dev), (torch.randn(B, C, generator=g) * 0.1).to(dev), act)


def layernorm(C, seed):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(C, generator=g) + 0.5).to(dev), (torch.randn(C, generator=g) * 0.1).to(dev), 1e-5)


def conv_tile(a, M):
    """the tile of the block-staged path for a problem (quant_act.hip: conv_tile_geo)"""
    t = _lib.load().dgq_quant_act_conv_tile(a.C, a.kh, a.kw, a.stride, a.Kp, None)
    Ho, Wo = (a.H + 2 * a.pad - a.kh) // a.stride + 1, (a.W + 2 * a.pad - a.kw) // a.stride + 1
    if t == 2 and a.B * -(-Ho // 4) * -(-Wo // 4) < 256 <= a.B * -(-Ho // 2) * -(-Wo // 4):
        t = 3
    return t


def quantise(name, want, problems, drop=(), tile=None, splits=None):
    """One dgq_quant_act_batch launch of `problems` = (x, geom, tables, pre, ln, ups); `drop`: gather tables withheld from the library
    (what the legacy entry dgq_quant_act does), `splits`: K splits asked for instead of the planner's, `want`: the kernel variant every
    problem must take."""
    n = len(problems)
    args = (_lib.QuantActArgs * n)()
    keep, outs = [], []
    for i, (x, geom, ab, pre, ln, ups) in enumerate(problems):
        B, H, W, C, kh, kw, stride, pad = geom
        M = B * ((H + 2 * pad - kh) // stride + 1) * ((W + 2 * pad - kw) // stride + 1)
        a, k = ops._quant_args(x, geom, ab, pre, ln, ups)
        for f in drop:
            setattr(a, f, None)
        parts = ops.quant_splits(a, M)
        if splits is not None:
            a.ksplits = parts = _lib.load().dgq_quant_act_parts(ab.Kp, splits)
        v = _lib.load().dgq_quant_act_variant(ctypes.byref(a))
        assert parts is not None and v == want, "%s: problem %d takes variant %s, the case is about %d" % (name, i, v, want)
        assert tile is None or conv_tile(a, M) == tile, "%s: tile %d, the case is about %d" % (name, conv_tile(a, M), tile)
        codes = torch.zeros((M, ab.Kp), dtype=torch.int8, device=dev)
        rowsum = torch.zeros((parts, M), dtype=torch.float32, device=dev)
        a.codes, a.rowsum = codes.data_ptr(), rowsum.data_ptr()
        args[i] = a
        keep.append(k)
        outs += [codes, rowsum]
        if i == 0:
            name += " | variant %d%s Kp %d parts %d" % (v, "" if tile is None else " tile %d" % tile, ab.Kp, parts)
    if not PLAN:
        ops._lib_call("dgq_quant_act_batch", n, ctypes.cast(args, ctypes.c_void_p), _lib.stream())
    emit(name, *outs)


def lin(M, C):
    return (1, M, 1, C, 1, 1, 1, 0)


def natural_cases():
    # ---- variant 2, natural order: per-M and scalar, a K-padding tail (320 -> Kp 384), one K split
    M, C = 203, 320
    for mode in ("perM", "scalar"):
        for dn, dt in DTYPES:
            for abits in ((8, 6) if dn == "f32" else (8,)):
                quantise("natural linear M%d C%d %s %s a%d" % (M, C, mode, dn, abits), 2,
                         [(data((M, C), 1, dt), lin(M, C), Tables(mode, "linear", C, 1, M, abits, "n1"), None, None, False)])
    quantise("natural linear M203 C320 perM f32 LayerNorm", 2,
             [(data((M, C), 2, torch.float32), lin(M, C), Tables("perM", "linear", C, 1, M, 8, "n2"), None, layernorm(C, 2), False)])
    quantise("natural linear M203 C320 perM f32 GEGLU", 2,
             [(data((M, 2 * C), 3, torch.float32), lin(M, C), Tables("perM", "linear", C, 1, M, 8, "n3"), (None, None, 2), None, False)])
    # several K splits at low M
    quantise("natural linear M64 C2560 perM f32 K splits", 2,
             [(data((64, 2560), 4, torch.float32), lin(64, 2560), Tables("perM", "linear", 2560, 1, 64, 8, "n4"), None, None, False)])
    # a convolution in natural order (border taps), GroupNorm + SiLU folded
    geom = (2, 9, 9, 32, 3, 3, 1, 1)
    for dn, dt in DTYPES:
        quantise("natural conv 2x9x9x32 3x3 perM %s GroupNorm+SiLU" % dn, 2,
                 [(data((2, 9, 9, 32), 5, dt), geom, Tables("perM", "conv", 32, 9, 81, 8, "n5"), groupnorm(2, 32, 5), None, False)])
    # shared-input launches of 2, 3, 4 problems (one x, LayerNorm folded: q / k / v), and an 8-problem launch
    for dn, dt in DTYPES:
        x, ln = data((M, C), 6, dt), layernorm(C, 6)
        for n in (2, 3, 4, 8):
            quantise("natural linear M203 C320 perM %s LayerNorm x%d problems" % (dn, n), 2,
                     [(x, lin(M, C), Tables("perM", "linear", C, 1, M, 8, "n6|%d" % i), None, ln, False) for i in range(n)])


def gather_cases():
    # ---- variant 1, the table gather from global memory: the library is given ksrc / koff alone, or C % 4 != 0
    nat = ("klds", "kdst", "kpat")
    geom = (2, 9, 9, 32, 3, 3, 1, 1)                        # interior rows (koff) and border rows (ksrc)
    for dn, dt in DTYPES:
        for abits in ((8, 6) if dn == "f32" else (8,)):
            for pre in (None, groupnorm(2, 32, 7)):
                quantise("gather conv 2x9x9x32 3x3 perK %s a%d%s" % (dn, abits, " GroupNorm+SiLU" if pre else ""), 1,
                         [(data((2, 9, 9, 32), 7, dt), geom, Tables("perK", "conv", 32, 9, 81, abits, "g1"), pre, None, False)], drop=nat)
        quantise("gather linear M77 C320 perK %s GEGLU" % dn, 1,
                 [(data((77, 640), 8, dt), lin(77, 320), Tables("perK", "linear", 320, 1, 77, 8, "g2"), (None, None, 2), None, False)], drop=nat)
        quantise("gather linear M77 C320 perK %s LayerNorm" % dn, 1,
                 [(data((77, 320), 9, dt), lin(77, 320), Tables("perK", "linear", 320, 1, 77, 8, "g3"), None, layernorm(320, 9), False)], drop=nat)
    quantise("gather conv 2x9x9x6 3x3 perK f32 (C not a multiple of 4)", 1,
             [(data((2, 9, 9, 6), 10, torch.float32), (2, 9, 9, 6, 3, 3, 1, 1), Tables("perK", "conv", 6, 9, 81, 8, "g4"), None, None, False)])
    # per-M tables behind a gather table (the natural order written out as ksrc)
    for dn, dt in DTYPES:
        ab = Tables("perM", "conv", 32, 9, 81, 8, "g5")
        ab.ksrc = natural_ksrc(32, 3, 3, ab.Kp).to(dev)
        quantise("gather conv 2x9x9x32 3x3 perM %s GroupNorm+SiLU" % dn, 1,
                 [(data((2, 9, 9, 32), 11, dt), geom, ab, groupnorm(2, 32, 11), None, False)], drop=nat)


def staged_cases():
    # ---- variant 0, LDS-staged strips: conv C = 320 3x3 (below what the block-staged path takes), Linear with few groups
    geom = (1, 8, 8, 320, 3, 3, 1, 1)
    for dn, dt in DTYPES:
        for abits in ((8, 6) if dn == "f32" else (8,)):
            quantise("staged conv 1x8x8x320 3x3 perK %s a%d GroupNorm+SiLU" % (dn, abits), 0,
                     [(data((1, 8, 8, 320), 12, dt), geom, Tables("perK", "conv", 320, 9, 64, abits, "s1"), groupnorm(1, 320, 12), None, False)], splits=1)
    for dn, dt in DTYPES:
        quantise("staged linear M77 C320 perK(2 groups) %s LayerNorm" % dn, 0,
                 [(data((77, 320), 13, dt), lin(77, 320), Tables("perK", "linear", 320, 1, 77, 8, "s2", G=2), None, layernorm(320, 13), False)])
        quantise("staged linear M77 C320 perK(2 groups) %s GEGLU" % dn, 0,
                 [(data((77, 640), 14, dt), lin(77, 320), Tables("perK", "linear", 320, 1, 77, 8, "s3", G=2), (None, None, 2), None, False)])
    # per-M tables behind a gather table: the staged kernel's per-M form
    ab = Tables("perM", "conv", 320, 9, 64, 8, "s4")
    ab.ksrc = natural_ksrc(320, 3, 3, ab.Kp).to(dev)
    quantise("staged conv 1x8x8x320 3x3 perM f32", 0, [(data((1, 8, 8, 320), 15, torch.float32), geom, ab, None, None, False)], splits=1)


def scatter_cases():
    # ---- variant 3, four rows per block: short-group per-K Linear with LayerNorm; a 3x3 behind a folded 2x upsample
    for dn, dt in DTYPES:
        for abits in ((8, 6) if dn == "f32" else (8,)):
            quantise("scatter linear M203 C320 perK(16 groups) %s a%d LayerNorm" % (dn, abits), 3,
                     [(data((203, 320), 16, dt), lin(203, 320), Tables("perK", "linear", 320, 1, 203, abits, "c1"), None, layernorm(320, 16), False)])
    quantise("scatter conv 4x32x32x460 3x3 perK f32 ups GroupNorm+SiLU", 3,
             [(data((4, 16, 16, 460), 17, torch.float32), (4, 32, 32, 460, 3, 3, 1, 1), Tables("perK", "conv", 460, 9, 1024, 8, "c2"),
               groupnorm(4, 460, 17), None, True)], drop=("kpat",))
    # ---- variant 4, one row per block: 16 waves (rows x problems <= 2048), with ups; 8 waves; a wide Linear
    for dn, dt in DTYPES:
        for ups in (False, True):
            quantise("scatter conv 1x8x8x460 3x3 perK %s 16 waves%s" % (dn, " ups" if ups else ""), 4,
                     [(data((1, 4, 4, 460) if ups else (1, 8, 8, 460), 18, dt), (1, 8, 8, 460, 3, 3, 1, 1), Tables("perK", "conv", 460, 9, 64, 8, "c3"),
                       groupnorm(1, 460, 18), None, ups)])
        x = data((5, 16, 16, 460), 19, dt)
        quantise("scatter conv 5x16x16x460 3x3 perK %s 8 waves x2 problems" % dn, 4,
                 [(x, (5, 16, 16, 460, 3, 3, 1, 1), Tables("perK", "conv", 460, 9, 256, 8, "c4|%d" % i), groupnorm(5, 460, 19), None, False)
                  for i in range(2)])
    quantise("scatter linear M77 C5120 perK f32 (wide)", 4,
             [(data((77, 5120), 20, torch.float32), lin(77, 5120), Tables("perK", "linear", 5120, 1, 77, 8, "c5"), None, None, False)])
    quantise("scatter linear M77 C5120 perK f32 a6 SiLU (wide)", 4,
             [(data((77, 5120), 20, torch.float32), lin(77, 5120), Tables("perK", "linear", 5120, 1, 77, 6, "c5"), (None, None, 1), None, False)])


def conv_block_cases():
    # ---- variant 5, block-staged: the smallest shapes conv_block_pays admits (>= 256 tiles, M >= 2048), each tile
    small = [(1, 128, 20, 5, 7, 1, False), (1, 256, 20, 5, 7, 2, False), (1, 44, 20, 10, 14, 1, True), (2, 64, 320, 8, 8, 1, False),
             (3, 32, 320, 8, 8, 1, False)]
    for tile, B, C, H, W, stride, ups in small:
        Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
        shape = (B, H >> ups, W >> ups, C)
        for mode in ("perK", "perM"):
            for dn, dt in (DTYPES if (stride == 1 and not ups) else F32):
                for abits in ((8, 6) if (dn == "f32" and C == 20) else (8,)):
                    for pre in ((None, groupnorm(B, C, 21)) if dn == "f32" else (groupnorm(B, C, 21),)):
                        quantise("block conv %dx%dx%dx%d 3x3 s%d%s %s %s a%d%s" % (B, H, W, C, stride, " ups" if ups else "", mode, dn, abits,
                                                                              " GroupNorm+SiLU" if pre else ""), 5,
                                 [(data(shape, 21, dt), (B, H, W, C, 3, 3, stride, 1), Tables(mode, "conv", C, 9, Ho * Wo, abits, "b%d" % C),
                                   pre, None, ups)], tile=tile)


def row_params_cases():
    # ---- dgq_act_row_params_batch: plain Linear with each fold, conv 3x3 (pad, stride 2, ups: the finish kernel), fold_T, a 4-problem batch
    M, C = 203, 320
    for dn, dt in DTYPES:
        folds = (("none", (M, C), None, None), ("LayerNorm", (M, C), None, layernorm(C, 30)), ("GEGLU", (M, 2 * C), (None, None, 2), None),
                 ("SiLU", (M, C), (None, None, 1), None))
        for fn, shape, pre, ln in folds:
            for bits in ((8, 6) if (dn == "f32" and fn == "none") else (8,)):
                emit("rowparams linear M%d C%d %s a%d %s" % (M, C, dn, bits, fn),
                     *(() if PLAN else ops.act_row_params(data(shape, 30, dt), lin(M, C), bits, pre, ln)))
        for (H, stride, ups) in ((9, 1, False), (9, 2, False), (10, 1, True)):
            x = data((2, H >> ups, H >> ups, 64), 31, dt)
            emit("rowparams conv 2x%dx%dx64 3x3 s%d%s %s GroupNorm+SiLU" % (H, H, stride, " ups" if ups else "", dn),
                 *(() if PLAN else ops.act_row_params(x, (2, H, H, 64, 3, 3, stride, 1), 8, groupnorm(2, 64, 31), None, ups)))
        emit("rowparams linear M210 C320 %s fold_T 70" % dn, *(() if PLAN else ops.act_row_params(data((210, C), 32, dt), lin(210, C), 8, fold_T=70)))
        if not PLAN:
            res = ops.act_row_params_multi([(data((M, C), 33 + i, dt), lin(M, C), 8, None, layernorm(C, 33 + i), False, 0) for i in range(4)])
        emit("rowparams linear M203 C320 %s LayerNorm x4 problems" % dn, *(() if PLAN else [t for r in res for t in r]))


def block_cases():
    # ---- dgq_quant_act_block + dgq_dequant_act_block: C = 32, 320, 2048; ldt > C/32; each fold; ups
    def run(name, x, geom, bits=8, pre=None, ln=None, ups=False, ldt=None):
        if PLAN:
            return emit(name)
        codes, table, rho = ops.quant_act_block(x, geom, bits, pre, ln, ups, ldt)
        xhat = ops.dequant_act_block(codes, table, torch.empty(codes.shape, dtype=x.dtype, device=dev))
        emit(name, codes, table, rho, xhat)
    for dn, dt in DTYPES:
        for C in (32, 320, 2048):
            run("block linear M203 C%d %s" % (C, dn), data((203, C), 40, dt), lin(203, C))
            run("block linear M203 C%d %s LayerNorm" % (C, dn), data((203, C), 40, dt), lin(203, C), ln=layernorm(C, 40))
        run("block linear M203 C320 %s a6 ldt 12" % dn, data((203, 320), 41, dt), lin(203, 320), bits=6, ldt=12)
        run("block linear M203 C320 %s GEGLU" % dn, data((203, 640), 42, dt), lin(203, 320), pre=(None, None, 2))
        run("block linear M203 C320 %s SiLU" % dn, data((203, 320), 43, dt), lin(203, 320), pre=(None, None, 1))
        run("block conv 2x9x9x64 3x3 %s GroupNorm+SiLU" % dn, data((2, 9, 9, 64), 44, dt), (2, 9, 9, 64, 3, 3, 1, 1), pre=groupnorm(2, 64, 44))
        run("block conv 2x10x10x64 3x3 %s ups GroupNorm+SiLU" % dn, data((2, 5, 5, 64), 45, dt), (2, 10, 10, 64, 3, 3, 1, 1),
            pre=groupnorm(2, 64, 45), ups=True)


def mx6_cases():
    # ---- dgq_quant_act_mx6 + dgq_dequant_act_mx6: block_cases' shapes and folds; lds > C/32; rows 3 and 7 carry an all-zero first block
    def run(name, x, geom, pre=None, ln=None, ups=False, lds=None):
        if PLAN:
            return emit(name)
        x = x.clone()
        x.view(-1, x.shape[-1])[3:8:4, :32] = 0
        codes, scale = ops.quant_act_mx6(x, geom, pre, ln, ups, lds)
        xhat = ops.dequant_act_mx6(codes, scale, torch.empty((codes.shape[0], codes.shape[1] * 32), dtype=x.dtype, device=dev))
        emit(name, codes, scale, xhat)
    for dn, dt in DTYPES:
        for C in (32, 320, 2048):
            run("mx6 linear M203 C%d %s" % (C, dn), data((203, C), 50, dt), lin(203, C))
            run("mx6 linear M203 C%d %s LayerNorm" % (C, dn), data((203, C), 50, dt), lin(203, C), ln=layernorm(C, 50))
        run("mx6 linear M203 C320 %s lds 12" % dn, data((203, 320), 51, dt), lin(203, 320), lds=12)
        run("mx6 linear M203 C320 %s GEGLU" % dn, data((203, 640), 52, dt), lin(203, 320), pre=(None, None, 2))
        run("mx6 linear M203 C320 %s SiLU" % dn, data((203, 320), 53, dt), lin(203, 320), pre=(None, None, 1))
        run("mx6 conv 2x9x9x64 3x3 %s GroupNorm+SiLU" % dn, data((2, 9, 9, 64), 54, dt), (2, 9, 9, 64, 3, 3, 1, 1), pre=groupnorm(2, 64, 54))
        run("mx6 conv 2x10x10x64 3x3 %s ups GroupNorm+SiLU" % dn, data((2, 5, 5, 64), 55, dt), (2, 10, 10, 64, 3, 3, 1, 1),
            pre=groupnorm(2, 64, 55), ups=True)


if __name__ == "__main__":
    for cases in (natural_cases, gather_cases, staged_cases, scatter_cases, conv_block_cases, row_params_cases, block_cases, mx6_cases):
        cases()
