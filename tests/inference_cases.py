"""The shapes `PointNet(..., training=False)` is tested at beyond the BASELINE configurations, their weights, clouds, oracle results and
error bounds -- TEST INFRASTRUCTURE, shared by tests/test_cpu_inference_cases.py (no GPU: the conditions under which the GPU test is
allowed to judge) and tests/test_gpu_inference_shapes.py (the HIP path against the fp64 oracle).  The checker is
oracle/pointnet_oracle.py; nothing of the package under test is imported here.

Inference runs two kernels a training step never runs -- chain_max_kernel (pn_panel.hip: a max-pooled chain in one launch, 64 rows per
panel) and seg_head_fused (pn_segout.hip: the segmentation head in one launch, 64 or 128 rows per tile) -- and the per-cloud dense
layers with moving statistics (bn_mode 2) on B rows, 32 rows per register chunk.  A cluster-labelling call hands them one cloud of
whatever the sampler kept, or a batch of small clusters: the list below is those shapes.
"""
from __future__ import annotations

import functools

import torch

from oracle import pointnet_oracle as O   # checker only

from parity_harness import CCLS, CSEG, make_inputs

# (B, N, what the shape reaches)
CASES = [
    (1, 1, "one row in every per-point kernel; the pool over a single row"),
    (5, 31, "one ragged slot, shorter than a 32-row block"),
    (2, 64, "exactly one 64-row slot"),
    (3, 65, "a whole slot plus a one-row slot"),
    (1, 127, "one row short of the 128-row GEMM tile"),
    (2, 129, "one row past it"),
    (40, 72, "more than 32 clouds: the dense layers' second register chunk, ragged (8 rows)"),
    (130, 40, "more than 128 clouds, each shorter than a slot"),
    (1, 2100, "long and ragged (32 slots plus 52 rows), a single cloud"),
]
SHAPES = [(B, N) for B, N, _ in CASES]
IDS = [f"{B}x{N}" for B, N in SHAPES]
INDEPENDENT = [(5, 31), (40, 72)]         # every cloud is also run alone at B = 1

PARAM_SEED, INPUT_SEED, INPUT_KIND = 23, 20260003, "shapes"
OUTPUTS = ("class", "part", "R")
# 'bf16x3': the mode's stated bound (tests/test_gpu_model.py) for all three outputs.  'bf16': per output max(T_BF16, FLOOR_FACTOR x the
# bf16 floor of the case), T_BF16 as tests/test_gpu_parity_configs.py::test_inference_at_baseline_size has it, the widening rule as
# parity_harness.check_training_step has it.
T_X3 = (2e-4, 2e-4, 2e-4)
T_BF16 = (1e-3, 1e-3, 1.5e-3)
FLOOR_FACTOR = 4.0
SAFE_SHARE = 0.97                         # at least this share of the points must have a part top-2 margin above twice the bound


def weights(vanilla):
    return O.init_params(CCLS, CSEG, seed=PARAM_SEED, vanilla=vanilla, randomize_bn=True)


def clouds(B, N):
    return make_inputs(B, N, INPUT_SEED, INPUT_KIND)[0]


def _max_abs(a, b):
    return tuple(float((x.double() - y.double()).abs().max()) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def expected(case):
    """case = (B, N, vanilla) -> the oracle's [class (B, 23), part (B, N, 12), R (B, 3, 3)] three times, computed once per case and to be
    left unchanged by its users:

    fp64        O.forward on double weights: what the device is compared with
    bf16        the same with both operands of every per-point matmul with K >= 64 rounded to bf16 (quant=O.bf16_round): what the
                'bf16' mode's operand rounding alone does to the fp64 result
    fp32        O.forward on float weights: what fp32 arithmetic alone does to it
    floor_bf16  |bf16 - fp64| per output, max over entries: what ANY correct implementation of the mode shows against fp64
    floor_fp32  |fp32 - fp64| likewise"""
    B, N, vanilla = case
    p, pc = weights(vanilla), clouds(B, N)
    p64 = {k: v.double() for k, v in p.items()}
    with torch.no_grad():
        f64 = O.forward(p64, pc.double(), training=False, vanilla=vanilla)
        b16 = O.forward(p64, pc.double(), training=False, vanilla=vanilla, quant=O.bf16_round)
        f32 = O.forward(p, pc, training=False, vanilla=vanilla)
    return dict(fp64=f64, bf16=b16, fp32=f32, floor_bf16=_max_abs(b16, f64), floor_fp32=_max_abs(f32, f64))


def bounds(case, precision):
    """the three max-abs error bounds (class, part, R) of `precision` at `case`"""
    if precision == "bf16x3":
        return T_X3
    assert precision == "bf16", precision
    return tuple(max(t, FLOOR_FACTOR * f) for t, f in zip(T_BF16, expected(case)["floor_bf16"]))


def top2_margin(probs):
    """(...,) the gap between the two largest entries of every row"""
    top2 = probs.topk(2, dim=-1).values
    return top2[..., 0] - top2[..., 1]
