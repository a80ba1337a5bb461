"""Bit identity of the bf16x3 attention family across two library builds: prints `name sha256(output bytes)` for small cases that reach
every path of attn3_stats_kernel / attn3_pv_kernel / attn3_merge_kernel (csrc/attn_bf16x3.hip) and attn3_one_kernel (csrc/attn_one.hip)
— their tile bodies are written out twice and must stay equal: the four score forms (QM 0-3), integer and three-plane V, the four softmax modes,
the three tensor types, ragged tiles and rows, the key split, the 8-wave blocks with one and two tiles per ring stage, one launch.
A second section does the same for am16_kernel (csrc/attn_mfma16.hip: un-quantised attention on the 16-bit matrix cores, one body for
16-bit and fp32 tensors) on RANDOM data, where a reordered sum shows: every head dim, ragged T and S, a one-key last stage, 129 stages;
bf16 / f16 with 64- and 32-key stages, fp32 in its three LDS forms — every instantiated kernel.
Run it once under each build (DGQ_HIP_LIB=old.so, then the tree's own) and diff the listings.
usage: python tools/hash_attention_family.py"""
import hashlib, os, sys
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgq_amd import ops          # noqa: E402

dev = torch.device("cuda")
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
# aqtizer_q / aqtizer_k modes of the score forms (None: not fused; 0 scalar, 1 per token, 2 per head-dim)
QM = {0: (None, None), 1: (1, 1), 3: (1, 0), 2: (2, 1)}
VF = {"vscalar": 0, "vperd": 2, "vpertok": 1}          # integer V (one plane), integer V, three planes
MODES = [(1, 1), (1, 0), (2, 1), (3, 0)]               # (softmax quantiser mode, start-peak skip)


def emit(name, t):
    torch.cuda.synchronize()
    print("%-84s %s" % (name, hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()), flush=True)


def env(**kv):
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def case(tag, seed, D, T, S, qm, vf, mode, skip, dt, B=2, H=2):
    g = torch.Generator().manual_seed(seed)
    q, k, v = ((torch.randn(B, n, H * D, generator=g) * 1.1).to(dev).to(DT[dt]) for n in (T, S, S))
    delta = None if mode == 1 else torch.tensor([1.0 / 255.0 if mode == 3 else 0.8], device=dev)
    tab = lambda n: (torch.rand(n, generator=g).to(dev) * 0.02 + 0.02, torch.randint(100, 156, (n,), generator=g).float().to(dev))
    ntab = lambda m, ntok: 1 if m == 0 else (ntok if m == 1 else D)
    fq = None
    if vf is not None:
        qmode, kmode = QM[qm]
        fq = (None if qmode is None else (qmode,) + tab(ntab(qmode, T)) + (0, 8),
              None if kmode is None else (kmode,) + tab(ntab(kmode, S - skip)) + (skip, 8),
              (VF[vf],) + tab(ntab(VF[vf], S)) + (0, 8))
    emit("%s D%d T%d S%d QM%d %s mode%d skip%d %s" % (tag, D, T, S, qm, vf or "fq=None", mode, skip, dt),
         ops.attention(q, k, v, H, D, D ** -0.5, mode, skip, delta, 8, fq=fq))


def main():
    n = 0
    # ---- three launches, 4-wave blocks: three tiles, a ragged last tile, ragged rows; every (QM, V form, mode) at every D
    env(DGQ_ATTN_ONE="0", DGQ_ATTN_SPLIT="0")
    for D in (8, 16, 40, 64, 80, 160):
        for qm in (0, 1, 3, 2):
            for vf in VF:
                for mode, skip in MODES:
                    case("three-launch", n, D, 70, 77, qm, vf, mode, skip, ("f32", "bf16", "f16")[n % 3])
                    n += 1
        for dt in DT:
            case("three-launch", n, D, 70, 77, 0, None, 1, 1, dt)
            n += 1
    # ---- key split: the partial statistics, the merge kernel, the fp32 part stores
    env(DGQ_ATTN_SPLIT="100000")
    for D in (40, 80):
        for mode, skip in ((1, 1), (3, 0)):
            for dt in ("f32", "bf16"):
                for qm, vf in ((1, "vperd"), (2, "vpertok"), (3, "vscalar"), (0, None)):
                    case("key-split", n, D, 130, 300, qm, vf, mode, skip, dt)
                    n += 1
    # ---- 8-wave blocks: one tile per stage (S = 77), two (S = 256: eight tiles), and a tail block
    env(DGQ_ATTN_SPLIT="0")
    for D in (40, 64):
        for S in (77, 256):
            for T in (2048, 2048 - 37):
                for qm, vf, mode, skip in ((1, "vperd", 1, 1), (2, "vpertok", 3, 0), (3, "vscalar", 2, 1), (0, None, 1, 0)):
                    case("wide", n, D, T, S, qm, vf, mode, skip, ("f32", "bf16")[n % 2], H=16)
                    n += 1
    # ---- one launch (the default environment)
    env(DGQ_ATTN_ONE=None, DGQ_ATTN_SPLIT=None)
    j = 0                                                  # mode, tensor type and V form advance at different rates: every pairing of two of them occurs
    for D in (40, 64, 80, 160):
        for S in (20, 77, 256, 250):
            for T in (64, 200):
                for qm in (1, 2, 3):
                    mode, skip = MODES[j % 4]
                    case("one-launch", n, D, T, S, qm, ("vperd", "vpertok", "vscalar")[(j // 5) % 3], mode, skip, ("f32", "bf16")[(j // 4) % 2])
                    n += 1
                    j += 1
    print("attention_sync_timeouts %d" % ops.attention_sync_timeouts(), flush=True)
    mfma16()


def mfma16():
    """ops.attention_mfma16 / ops.attention_mfma16_f32 on the shapes of tests/attention_mfma16_ref.py; q, k ~ N(0, 1.1), v ~ 1.3·N(0, 1) + 0.2"""
    from tests import attention_mfma16_ref as ar
    for n, ((D, T, S, H), B) in enumerate([(c, ar.B) for c in ar.CASES] + [(ar.LONG, 1)]):
        g = torch.Generator().manual_seed(7000 + n)
        q, k = ((torch.randn(B, m, H * D, generator=g) * 1.1).to(dev) for m in (T, S))
        v = (1.3 * torch.randn(B, S, H * D, generator=g) + 0.2).to(dev)
        shape = "D%d T%d S%d H%d B%d" % (D, T, S, H, B)
        for dt in ("bf16", "f16"):
            for kt in (None, "32"):
                env(DGQ_ATTN16_KT=kt)
                emit("mfma16 %s %s kt%s" % (shape, dt, kt or "-default"), ops.attention_mfma16(q.to(DT[dt]), k.to(DT[dt]), v.to(DT[dt]), H, D, D ** -0.5))
        env(DGQ_ATTN16_KT=None)
        for form in ("0", "1", "2"):
            env(DGQ_ATTN16F_FORM=form)
            emit("mfma16_f32 %s form%s" % (shape, form), ops.attention_mfma16_f32(q, k, v, H, D, D ** -0.5))
        env(DGQ_ATTN16F_FORM=None)


main()
