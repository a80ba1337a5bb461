"""Self-check of tests/weight_only_fused_ref.py, on the CPU: the a-priori bound of dgq_conv2d_wq_mfma16_fused must hold for a plain
torch-fp32 restatement of the kernel's order on every case the GPU test runs, and must notice each planted mistake on a named case —
a bound that a wrong kernel also meets would prove nothing on the GPU."""
import pytest
import torch

from tests import weight_only_fused_ref as fr


def _ratio(name, kind, dtype, bits, planted, mistake=None):
    if planted:
        x, _w, codes, delta, zp, bias, fz, _ = fr.planted_case(name, kind, dtype, bits)
    else:
        x, _w, codes, delta, zp, bias, fz = fr.random_case(name, kind, dtype, bits)
    fz = fr.kernel_inputs(fz)
    w_int = fr.weight_rows(codes.float() - zp.view(-1, *([1] * (codes.dim() - 1))))
    y64, bound = fr.ref64(name, x, w_int, delta, bias, fz, dtype)
    y = fr.restatement(name, x, w_int, zp, delta, bias, fz, dtype, mistake)
    assert y.shape == y64.shape and y.dtype == dtype
    return fr.worst_ratio(y, y64, bound), y, y64


@pytest.mark.parametrize("dtype", fr.DTYPES, ids=["fp32", "bf16", "f16"])
def test_restatement_is_under_the_bound_on_every_case(dtype):
    worst = 0.0
    for name, kind in fr.RANDOM:
        for bits in (4, 8):
            r, _, _ = _ratio(name, kind, dtype, bits, planted=False)
            print("%s %s W%d %s: restatement max |err| / bound = %.3f" % (name, kind, bits, dtype, r))
            assert r <= 1.0, (name, kind, bits)
            worst = max(worst, r)
    print("worst ratio of the fp32 restatement, %s: %.3f" % (dtype, worst))


@pytest.mark.parametrize("dtype", fr.DTYPES, ids=["fp32", "bf16", "f16"])
def test_restatement_gives_the_exact_value_on_planted_data(dtype):
    """on the planted data every operation of the restatement is exact, so it equals the float64 value rounded once — the property the
    GPU test asks of the kernel"""
    for name, kind in fr.PLANTED:
        _, y, y64 = _ratio(name, kind, dtype, 4, planted=True)
        assert torch.equal(y, y64.to(dtype)), (name, kind)
        assert y64.abs().max() < (60000 if dtype == torch.float16 else 2 ** 24)          # (the construction stays inside the type's range)


#: mistake -> the case that shows it (geometry, kind, planted data?)
NAMED = {
    "pad_act_shift": ("conv3_s1", "gn_silu", False),                    # 3x3, pad 1: every border row has taps outside the image
    "tail_shift": ("conv3_c7_s2", "gn_silu_rows", False),               # K = 63: lane 63 names channel 0, whose shift is the large one
    "neighbour_image": ("conv3_3x96x5x7_40", "gn_silu_res", False),     # 35 rows per image: 32-row tiles straddle two images
    "silu_before_norm": ("conv3_c20", "gn_silu", False),
    "table_by_k": ("conv3_s2", "gn_silu_res", False),                   # K = 9·C: k and k mod C differ from the second tap on
    "swap_value_gate": ("linear_33x64_128", "geglu", False),
    "bias_rows_image": ("conv1_3x96x5x7_40", "gn_silu_rows", False),
    "packed_index": ("t64_1000x72_1030", "perm_res", False),            # N = 1030 interleaved rows, a residual in the output's order
}


@pytest.mark.parametrize("mistake", fr.MISTAKES)
@pytest.mark.parametrize("dtype", fr.DTYPES, ids=["fp32", "bf16", "f16"])
def test_bound_notices_each_planted_mistake(mistake, dtype):
    name, kind, planted = NAMED[mistake]
    for bits in (4, 8):
        clean, _, _ = _ratio(name, kind, dtype, bits, planted)
        wrong, _, _ = _ratio(name, kind, dtype, bits, planted, mistake)
        print("%s on %s %s W%d %s: ratio %.3f clean, %.3g with the mistake" % (mistake, name, kind, bits, dtype, clean, wrong))
        assert clean <= 1.0 < wrong


def test_mistakes_are_all_named():
    assert set(NAMED) == set(fr.MISTAKES)
