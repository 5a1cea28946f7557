"""Whole training steps on long clouds with a ragged end, and on batches of more than 128 clouds.

Long ragged clouds.  From 2048 points on the scatter of the max-pool backward (pn_maxbwd.hip: maxbwd_scatter_body<2>, in the default plan
inside maxbwd_scatter_reduce) works on 64-row tiles of two 32-row MFMA blocks.  Every other training shape at or above that size is a
multiple of 64 (2048, 4096), so the ragged last tile of that form -- fewer than 64 rows, a second block wholly outside the cloud, the
count of 16-byte stores -- and the ragged ends of the other per-tile kernels on a long cloud (128-row statistics tiles, 64-row panel
slots, 64-row weight-gradient slabs, 32-row resolve blocks) ran in no training step.  Real scans are not multiples of 64.
    N = 2049  one row in the last 64-row tile, 32-row block and 128-row tile
    N = 2080  the last scatter tile is exactly one 32-row block: the second block is empty
    N = 2100  52 rows, in both blocks
The clouds are make_inputs' shape-diverse ones with the points farthest from each centroid moved into the ragged tile, the farthest to row N - 1
(parity_harness.farthest_point_last): as drawn, no maximum of any max-pooled layer falls into the one-row tile at N = 2049 and the
tile would be exercised with zeros.  WITNESS, asserted on the GPU's own rows of the maxima: every cloud of every max-pooled layer has
at least 64 of its 1024 maxima in the ragged tile (the fp64 oracle: at least 153, tests/test_cpu_long_cloud_inputs.py).  Two or three
clouds leave the batch statistics of the per-cloud dense layers ill-conditioned (as a batch of one, tests/test_gpu_large_batch.py), so
those cases are teacher-forced only; four clouds are also held end to end.

Large batches.  maxbwd_dw_kernel stages 128 clouds per pass, maxbwd_prep_body 32 per round; mse_kernel, fold3_bwd_slabs_kernel and
cloud_bias_grad_kernel have grids and loops that grow with B.  No other training step has more than 64 clouds: the second 128-cloud
pass never ran.  B = 130 (two clouds into the second pass) is held teacher-forced and end to end, B = 257 (one cloud into the third)
teacher-forced.

Every step here also writes the per-launch lines of the Gram-form backward (tests/teacher_forced.py: max_bwd_launches) to the report.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from parity_harness import BF16, X3, check_training_step, farthest_point_last, ragged_tile_hits, report   # noqa: E402

TOL = {"bf16x3": X3, "bf16": BF16}
# (B, N, vanilla, end to end)
RAGGED = [(2, 2049, False, False), (3, 2080, False, False), (4, 2100, False, True), (4, 2100, True, True)]
MAX_WS = {False: ("mm23", "iT.m3", "fT.m3"), True: ("mm23",)}


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("B,N,vanilla,end_to_end", RAGGED)
def test_training_step_on_long_ragged_clouds(dev, B, N, vanilla, end_to_end, precision):
    tag = f"long-ragged[all,vanilla={vanilla},{precision},B={B},N={N}]"
    _, m = check_training_step(dev, B, N, "all", vanilla=vanilla, precision=precision, seed_params=21, seed_inputs=20260003, inputs="shapes",
                               damp_tnet=0.1, end_to_end=end_to_end, pc_hook=farthest_point_last, tag=tag, **TOL[precision])
    for wn in MAX_WS[vanilla]:
        hits = ragged_tile_hits(m.workspace_tensor(wn + ".arg", B, N, True, torch.int32).view(B, 1024).cpu(), N)
        report(f"{tag} witness: maxima of {wn} in rows >= {64 * (N // 64)} (the ragged 64-row tile), per cloud: {hits.tolist()}")
        assert int(hits.min()) >= 64, (wn, hits.tolist())


@pytest.mark.parametrize("B,N,profile,precision,end_to_end", [
    (130, 136, "all", "bf16x3", True), (130, 136, "all", "bf16", True), (130, 136, "final", "bf16x3", True),
    (257, 33, "all", "bf16x3", False), (257, 33, "all", "bf16", False)])
def test_training_step_with_more_than_128_clouds(dev, B, N, profile, precision, end_to_end):
    tag = f"huge-batch[{profile},{precision},B={B},N={N}]"
    worst, _ = check_training_step(dev, B, N, profile, precision=precision, seed_params=21, seed_inputs=20260003, inputs="shapes",
                                   damp_tnet=0.1, end_to_end=end_to_end, tag=tag, **TOL[precision])
    report(f"{tag}: worst relative gradient error {worst:.3e}")
