"""pn_fps on the MI355X beyond one block and one cloud, bit for bit against the NumPy oracle (oracle/sampling_oracle.py): clouds split
over several blocks with several clouds per launch and several launches per call, the round tag of the cross-block granule
wrapping, the largest cloud, a last block of one point, distance ties between blocks, a start index other than 0 on every
kernel, M = 1, M > N, and the pruned kernel with two clouds.  Inputs: tests/sampler_cases.py (checked on the oracle alone in
tests/test_cpu_sampler_cases.py).  Every cross-block wait is bounded and ends in the error flag, which ops raises: a lost peer
fails the test, it does not hang it."""
import numpy as np
import pytest
import torch

import sampler_cases as SC
from oracle import sampling_oracle as SO

pytestmark = pytest.mark.gpu


def _compare(dev, xyz, M, start):
    from pointcloudprocessing_amd import ops
    idx, md = ops.farthest_point_sample(torch.from_numpy(xyz).to(dev), M, start_idx=start, return_mindist=True)
    idx, md = idx.cpu().numpy(), md.cpu().numpy()
    assert idx.shape == (xyz.shape[0], M) and md.shape == xyz.shape[:2]
    refs = []
    for b in range(xyz.shape[0]):
        ri, rmd = SO.fps(xyz[b], M, start)
        assert np.array_equal(idx[b], ri), (b, np.flatnonzero(idx[b] != ri)[:5])
        assert np.array_equal(md[b].view(np.uint32), rmd.view(np.uint32)), (b, np.flatnonzero(md[b] != rmd)[:5])
        refs.append((ri, rmd))
    return refs


@pytest.mark.parametrize("name", list(SC.FPS_CASES))
def test_fps_case(dev, name):
    B, N, M, start = SC.FPS_CASES[name]
    xyz = SC.fps_cloud(name)
    assert xyz.shape == (B, N, 3)
    refs = _compare(dev, xyz, M, start)
    if name == "tag_wrap":
        assert M - 1 > SC.FPS_TAG_PERIOD and N > SC.FPS_SINGLE_BLOCK_MAX
    if name == "cross_block_ties":
        twins = dict(SC.FPS_TIE_PAIRS)
        hit = [i for i in refs[0][0] if i in twins]
        assert len(hit) >= 4 and all(np.array_equal(xyz[0, i], xyz[0, twins[i]]) for i in hit)
        assert all(SC.fps_block_of(i) != SC.fps_block_of(twins[i]) for i in hit)
    if M == 1:
        assert all(np.isposinf(rmd).all() for _, rmd in refs)
    if M > N:
        assert all((ri[N:] == 0).all() for ri, _ in refs)


@pytest.mark.parametrize("mode", ["1", "2"])
def test_fps_pruned_kernel_two_clouds(dev, monkeypatch, mode):
    monkeypatch.setenv("PN_FPS_PRUNE", mode)
    B, N, M, start = SC.FPS_PRUNED_CASE
    xyz = SC.fps_ordered_grid()
    refs = _compare(dev, xyz, M, start)
    assert not np.array_equal(refs[0][0], refs[1][0])                          # the second cloud is its own problem
