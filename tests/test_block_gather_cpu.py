"""The tap gather of the real-time block GEMMs (dgq_amd/csrc/gemm_gather.h), checked on a CPU: the header both kernels stage their
operands through is compiled into a stand-alone host program (tests/host/block_gather_main.cpp, address + UB sanitizers where they
link) and run as a child process; the expected table is F.unfold of an index image."""
import os
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gather_prog(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    assert hipcc, "hipcc not found"
    out = str(tmp_path_factory.mktemp("block_gather") / "block_gather")
    # the host compiler as the Makefile's abi.o rule uses it
    base = [hipcc, "-O2", "-std=c++17", "-x", "c++", "-I", os.path.join(ROOT, "dgq_amd", "csrc"),
            os.path.join(ROOT, "tests", "host", "block_gather_main.cpp"), "-o", out]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if san.returncode != 0:
        print("sanitizers do not link here, building without:\n" + san.stderr[-2000:])
        subprocess.run(base, check=True, capture_output=True, text=True)
    return out


def _kp(K):
    return -(-K // 128) * 128


#: name -> (B, H, W, C, kh, kw, stride, pad, ups); H, W behind the folded upsample
GEOMETRIES = {
    "linear M37 C320 (plain)": (37, 1, 1, 320, 1, 1, 1, 0, 0),
    "3x3 s1 p1 2x9x9": (2, 9, 9, 32, 3, 3, 1, 1, 0),
    "3x3 s2 p1 2x11x13": (2, 11, 13, 64, 3, 3, 2, 1, 0),
    "3x3 ups 2x8x8": (2, 8, 8, 32, 3, 3, 1, 1, 1),
    "1x1 s2 p0 7x9 (not plain)": (1, 7, 9, 64, 1, 1, 2, 0, 0),
    "3x3 p0 5x5": (1, 5, 5, 32, 3, 3, 1, 0, 0),
}


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_gather_equals_unfold_of_an_index_image(gather_prog, name):
    """For every output row m and chunk cc in [0, nchp): `in` is exactly "cc < nch and the tap lies in the image", `pix` is the stored
    pixel wherever `in` holds, cb = cc mod cpb for every real chunk (cc < nch) and `in` is false for every chunk of the K padding.
    (cb of a padding chunk is not pinned: nothing reads it, and the plain case returns cc itself there.)"""
    B, H, W, C, kh, kw, stride, pad, ups = GEOMETRIES[name]
    Kp = _kp(kh * kw * C)
    r = subprocess.run([gather_prog], input="%d %d %d %d %d %d %d %d %d %d\n" % (B, H, W, C, kh, kw, stride, pad, ups, Kp),
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = r.stdout.split("\n")
    M, nch, nchp = (int(v) for v in rows[0].split())
    got = torch.tensor([[int(v) for v in l.split()] for l in rows[1:] if l], dtype=torch.int64).view(M, nchp, 3)

    Hs, Ws, cpb = H >> ups, W >> ups, C // 32
    img = (1 + torch.arange(B * Hs * Ws, dtype=torch.float64)).view(B, 1, Hs, Ws)
    if ups:
        img = img.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    taps = F.unfold(img, kernel_size=(kh, kw), padding=pad, stride=stride)             # [B][kh·kw (dh·kw + dw)][L]
    L = taps.shape[2]
    assert M == B * L and nch == kh * kw * cpb and nchp == Kp // 32
    if name.startswith("linear"):
        assert (nch, nchp) == (10, 12)
    val = taps.permute(0, 2, 1).reshape(M, kh * kw).to(torch.int64)                    # 0: outside, else pixel + 1
    cc = torch.arange(nchp)
    real = cc < nch
    tap = (cc // cpb).clamp(max=kh * kw - 1)
    want_in = real[None, :] & (val[:, tap] != 0)
    want_pix = val[:, tap] - 1

    got_pix, got_cb, got_in = got[..., 0], got[..., 1], got[..., 2].bool()
    assert torch.equal(got_in, want_in)
    assert not got_in[:, ~real].any()
    assert torch.equal(got_pix[want_in], want_pix[want_in])
    assert torch.equal(got_cb[:, real], (cc % cpb)[real][None, :].expand(M, -1))
    assert want_in.any(dim=0)[real].all()                                              # every real chunk is read by some row
    if pad:
        assert not want_in[:, real].all()                                              # ... and the border is in the case
