"""The inputs of tests/test_gpu_long_clouds.py, checked without a GPU, on the fp64 oracle alone: with the farthest point of every cloud
moved to row N - 1 and the next farthest in front of it (parity_harness.farthest_point_last), every cloud of every max-pooled layer has maxima in the ragged last 64-row
tile -- so a later edit of make_inputs or of the hook cannot leave the GPU cases running that tile on zeros.  The GPU test asserts
at least 64 of the GPU's own rows; the oracle has at least 153 at these shapes, asserted here as at least 128."""
import pytest
import torch

from oracle import pointnet_oracle as O
from parity_harness import CCLS, CSEG, farthest_point_last, make_inputs, ragged_tile_hits

LAYERS = {False: ("mlp_2_3", "input_transform.conv3", "feature_transform.conv3"), True: ("mlp_2_3",)}


def oracle_hits(B, N, vanilla, hook):
    params = O.init_params(CCLS, CSEG, seed=21, vanilla=vanilla, randomize_bn=True)
    if not vanilla:
        for k in ("input_transform.w", "feature_transform.w"):
            params[k] = params[k] * 0.1
    pc, _, y_seg, _, keep = make_inputs(B, N, 20260003, "shapes")
    if hook is not None:
        pc, y_seg = hook(pc, y_seg)
    with torch.no_grad():
        _, ctx = O.forward({k: v.double() for k, v in params.items()}, pc.double(), return_ctx=True, training=True, vanilla=vanilla,
                           dropout_masks=keep)
    return {on: ragged_tile_hits(ctx.taps[on + ".y"].argmax(1), N) for on in LAYERS[vanilla]}


@pytest.mark.parametrize("B,N,vanilla", [(2, 2049, False), (3, 2080, False), (4, 2100, False), (4, 2100, True)])
def test_the_ragged_tile_of_a_long_cloud_receives_maxima(B, N, vanilla):
    for on, hits in oracle_hits(B, N, vanilla, farthest_point_last).items():
        assert hits.shape == (B,) and int(hits.min()) >= 128, (on, hits.tolist())


@pytest.mark.parametrize("N", [2049, 2080, 2100])
def test_the_hook_fills_the_ragged_tile_with_the_farthest_points(N):
    """the last N % 64 rows hold the N % 64 farthest points, the farthest last; labels travel with their points; a row that neither
    gives nor receives a point is untouched (at N = 2049: one swap)"""
    B, nr = 3, N % 64
    pc, _, y_seg, _, _ = make_inputs(B, N, 20260003, "shapes")
    y_seg = y_seg * N + torch.arange(N)                       # a label that names its point
    pc2, y2 = farthest_point_last(pc, y_seg)
    dist = (pc - pc.mean(1, keepdim=True)).double().norm(dim=-1)
    for b in range(B):
        src = y2[b] % N                                       # where each row's point came from
        assert torch.equal(src.sort().values, torch.arange(N)) and torch.equal(pc2[b], pc[b][src]) and torch.equal(y2[b], y_seg[b][src])
        tail = dist[b][src[N - nr:]]
        assert bool((tail[1:] >= tail[:-1]).all()) and float(tail[0]) >= float(dist[b][src[: N - nr]].max())
        moved = src != torch.arange(N)
        assert int(moved[: N - nr].sum()) <= nr and (nr > 1 or int(moved.sum()) in (0, 2))


def test_without_the_hook_the_one_row_tile_is_empty():
    """why the hook exists: as drawn, row 2048 of these clouds holds no maximum of any max-pooled layer"""
    hits = oracle_hits(2, 2049, False, None)
    assert sum(int(h.sum()) for h in hits.values()) == 0, {k: v.tolist() for k, v in hits.items()}
