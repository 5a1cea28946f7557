"""The cases of tests/inference_cases.py, checked without a GPU on the oracle alone: tests/test_gpu_inference_shapes.py compares arg-max
indices with the fp64 oracle's, which means something only where the oracle's own top-2 margin is clear of the error bound.  Here: the
oracle is finite at every shape (N = 1 included: a cloud of one point normalises to the origin), every class margin exceeds twice the
widest class bound, and at most 3 % of the points have a part margin within twice the widest part bound -- the cap under which the GPU
test may leave points out of its index comparison.  A change of a seed, a shape or a bound that breaks one of these fails here first."""
import pytest
import torch

import inference_cases as IC


@pytest.mark.parametrize("vanilla", [False, True])
@pytest.mark.parametrize("B,N", IC.SHAPES, ids=IC.IDS)
def test_inference_case_is_finite_and_clear_of_ties(B, N, vanilla):
    case = (B, N, vanilla)
    exp = IC.expected(case)
    cls, seg, R = exp["fp64"]
    assert cls.shape == (B, 23) and seg.shape == (B, N, 12) and R.shape == (B, 3, 3) and cls.dtype == torch.float64
    for kind in ("fp64", "bf16", "fp32"):
        assert all(bool(torch.isfinite(t).all()) for t in exp[kind]), kind
    assert float((cls.sum(-1) - 1).abs().max()) < 1e-12 and float((seg.sum(-1) - 1).abs().max()) < 1e-12
    # the floors are what they are called: fp32 arithmetic is far below the bf16 operand rounding, which is below the bounds' scale
    assert max(exp["floor_fp32"]) < 1e-4 and max(exp["floor_fp32"]) < max(exp["floor_bf16"]) < 1e-2, (exp["floor_fp32"], exp["floor_bf16"])
    cls_margin, part_margin = IC.top2_margin(cls), IC.top2_margin(seg)
    for precision in ("bf16x3", "bf16"):
        b_cls, b_part, _ = IC.bounds(case, precision)
        assert b_cls >= IC.T_X3[0] and b_part >= IC.T_X3[1]
        assert float(cls_margin.min()) > 2 * b_cls, (precision, float(cls_margin.min()), b_cls)
        share = float((part_margin > 2 * b_part).double().mean())
        assert share >= IC.SAFE_SHARE, (precision, share, b_part)
    print(f"inference case B={B} N={N} vanilla={vanilla}: bf16 floor {exp['floor_bf16']} fp32 floor {exp['floor_fp32']} class margin "
          f"{float(cls_margin.min()):.3e} part safe share {float((part_margin > 2 * IC.bounds(case, 'bf16')[1]).double().mean()):.4f}")


def test_the_case_list_is_the_one_the_kernels_need():
    """the shapes on both sides of every row count at which an inference kernel takes another path"""
    shapes = set(IC.SHAPES)
    assert len(IC.SHAPES) == len(shapes) == 9
    assert min(N for _, N in shapes) == 1                                     # a single row
    assert any(N < 32 for _, N in shapes)                                     # less than a 32-row block
    assert any(N == 64 for _, N in shapes) and any(N % 64 == 1 and N > 64 for _, N in shapes)      # a whole slot; a one-row slot behind one
    assert any(N == 127 for _, N in shapes) and any(N == 129 for _, N in shapes)                   # either side of the 128-row tile
    assert any(32 < B <= 128 and B % 32 for B, _ in shapes) and any(B > 128 for B, _ in shapes)    # dense layers: a ragged second chunk; B > 128
    assert any(B == 1 and N > 2048 and N % 64 for B, N in shapes)             # long and ragged
    assert max(B * N for B, N in shapes) == 5200                              # every case stays small
    assert set(IC.INDEPENDENT) <= shapes
