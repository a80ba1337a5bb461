"""The reference side of tests/test_gpu_groupnorm_stats.py, checked without a GPU: the metric rho leaves a correct fp32 algorithm
(F.group_norm in fp32, the arithmetic the reference project runs) a wide margin below the ceiling of the GPU tests, it sees every
index mistake a statistics kernel can make, and the case list reaches the index edges of the kernels."""
import pytest
import torch

from tests import groupnorm_stats_ref as gr

NAME = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "f16"}


@pytest.mark.parametrize("geom", gr.GEOMS + ((1, 6400, 4, 2), (1, 6376, 4, 2)), ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("dtype", gr.DTYPES, ids=lambda d: NAME[d])
def test_fp32_group_norm_stays_far_below_the_ceiling(geom, dtype):
    """rho of F.group_norm in fp32 is <= 16 on every kind, dtype and geometry of the GPU tests (measured: <= 4.6, const 1.0): the
    ceiling of 256 leaves a correct fp32 algorithm a factor of 16 or more"""
    B, HW, C, G = geom
    gamma, beta = gr.make_affine(C)
    for kind in gr.KINDS:
        x = gr.make_case(kind, B, HW, C, G, dtype)
        r, rmax = gr.yardstick(x, G, gr.EPS, gamma, beta)
        print("yardstick %-8s %-5s %-16s rho %.2f" % (kind, NAME[dtype], geom, rmax))
        assert rmax <= 16.0, (kind, gr.worst(r))


@pytest.mark.parametrize("dtype", gr.DTYPES, ids=lambda d: NAME[d])
def test_the_metric_sees_what_it_must(dtype):
    """rho of the float64-exact scale / shift is <= 1 (<= 3 once both are rounded to fp32); statistics with one slice's rows left out, with the first
    slice counted twice, with the channel range moved by one channel, or with image 1's rows taken for image 0 push it above 4096"""
    B, HW, C, G = 2, 200, 64, 32
    _, rows_per, S, last = gr.slicing(B, HW, G)
    assert S == 3 and last < rows_per
    gamma, beta = gr.make_affine(C)
    x = gr.make_case("plain", B, HW, C, G, dtype)
    sc, sh = gr.ref_scale_shift(x, G, gr.EPS, gamma, beta)
    assert gr.rho(x, G, gr.EPS, gamma, beta, sc, sh)[1] <= 1.0
    # rounded to fp32: 2^-24·|x·scale| + 2^-24·|shift| with |shift| <= |y64| + |x·scale| <= 2A
    assert gr.rho(x, G, gr.EPS, gamma, beta, sc.float(), sh.float())[1] <= 3.0
    wrong = {"last slice dropped": x[:, :HW - last], "a middle slice dropped": torch.cat([x[:, :rows_per], x[:, 2 * rows_per:]], 1),
             "first slice twice": torch.cat([x[:, :rows_per], x], 1), "channels moved by one": torch.roll(x, -1, dims=2),
             "image 1 for image 0": x[[1, 1]]}
    for what, xs in wrong.items():
        sc, sh = gr.ref_scale_shift(xs, G, gr.EPS, gamma, beta)
        r, rmax = gr.rho(x, G, gr.EPS, gamma, beta, sc.float(), sh.float())
        assert rmax > 4096.0, (what, rmax)
        if what != "image 1 for image 0":
            assert float(r.min()) > 4096.0, (what, float(r.min()))            # every (batch, channel) moves, not only the worst one


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=lambda d: NAME[d])
def test_the_metric_sees_the_mistakes_of_a_partials_merge(dtype):
    """the merge of per-(16-row block, channel) partials restated in float64 (two buffers, C1 = 68 and C2 = 60 with G = 8: group 4
    spans both): exact it gives rho <= 1 (<= 3 rounded to fp32); with C1 as the pitch of the second buffer, without the 16· of the between-block term, or
    with partials of the unrounded values where the tensor is stored in 16 bits, rho passes the ceiling of the GPU tests"""
    B, HW, C1, C2, G = 2, 64, 68, 60, 8
    C = C1 + C2
    gamma, beta = gr.make_affine(C)
    x64 = gr.make_case("plain", B, HW, C, G, torch.float64)
    x = x64.to(dtype)
    p1, p2 = gr.partials64(x[..., :C1].contiguous()), gr.partials64(x[..., C1:].contiguous())
    sc, sh = gr.scale_shift_of(*gr.merge_partials64(p1, p2, G), G, gr.EPS, gamma, beta)
    assert gr.rho(x, G, gr.EPS, gamma, beta, sc, sh)[1] <= 1.0 and gr.rho(x, G, gr.EPS, gamma, beta, sc.float(), sh.float())[1] <= 3.0
    for mistake in ("pitch", "factor16"):
        sc, sh = gr.scale_shift_of(*gr.merge_partials64(p1, p2, G, mistake), G, gr.EPS, gamma, beta)
        assert gr.rho(x, G, gr.EPS, gamma, beta, sc.float(), sh.float())[1] > 4096.0, mistake
    if dtype != torch.float32:
        for kind in ("plain", "offset"):
            u = gr.make_case(kind, B, HW, C, G, torch.float64).float()              # what an epilogue holds before it rounds
            x = u.to(dtype)                                                         # what it stores
            q1, q2 = gr.partials64(None, u[..., :C1].contiguous()), gr.partials64(None, u[..., C1:].contiguous())
            sc, sh = gr.scale_shift_of(*gr.merge_partials64(q1, q2, G), G, gr.EPS, gamma, beta)
            assert gr.rho(x, G, gr.EPS, gamma, beta, sc.float(), sh.float())[1] > 256.0, kind


def test_the_case_list_covers_the_index_edges():
    """via slicing(): S == 1, S > 1 with equal slices, S > 1 with a shorter last slice, S == 32, Cg in {1, 2, 3, 10, 40, 512}; and
    the direct-entry case reaches the second trip of gn_finalize_kernel's loop (S > 64) with a shorter last slice"""
    seen, cgs = set(), set()
    for (B, HW, C, G) in gr.GEOMS:
        slices, rows_per, S, last = gr.slicing(B, HW, G)
        assert 1 <= S <= slices <= 32 and (S - 1) * rows_per + last == HW and 0 < last <= rows_per
        cgs.add(C // G)
        seen.add("one" if S == 1 else ("equal" if last == rows_per else "short"))
        if S == 32:
            seen.add("cap")
    assert seen == {"one", "equal", "short", "cap"} and cgs == {1, 2, 3, 10, 40, 512}
    assert gr.slicing(2, 200, 32) == (3, 67, 3, 66)
    rows_per, S, last = gr.slicing_of(6400, 100)
    assert (rows_per, S, last) == (64, 100, 64)
    rows_per, S, last = gr.slicing_of(6400 - 24, 100)
    assert S == 100 and last == 40
