"""The global start of the semantic ICP without a GPU: the declared surface, the argument checks that run before any HIP call,
ops.rotation_grid, and the NumPy oracle pipeline (tests/icp_global_oracle.py) on the kc-46 cases the GPU tests share: it must
recover the true pose from rotations up to 171 degrees, full view and one-sided, where the local solver alone does not."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
import icp_global_oracle as GO
import icp_oracle as IO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pn_part_moments_workspace_bytes", "pn_part_moments", "pn_icp_seed_poses", "pn_icp_score_workspace_bytes", "pn_icp_score_poses")
NP = len(helpers.F15_PARTS)
FAKE = C.c_void_p(0x1000)        # never dereferenced: the checks run before any HIP call
WS = 1 << 30


def test_surface_is_declared_and_exported():
    from pointcloudprocessing_amd import _lib, ops
    from pointcloudprocessing_amd.pointnet.PointNet import PointNet
    hdr = open(os.path.join(ROOT, "include", "pointnet_hip.h")).read()
    for name in NEW:
        assert f"{name}(" in hdr and name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert "#define PN_ABI_VERSION 6" in hdr and _lib.lib().pn_abi_version() == 6 and _lib.ABI_VERSION == 6
    for f in (ops.rotation_grid, ops.part_moments, ops.icp_part_moments, ops.icp_seed_poses, ops.icp_score_poses, ops.global_pose):
        assert callable(f)
    assert "global" in PointNet.predict_pose.__doc__
    L = _lib.lib()
    assert L.pn_part_moments_workspace_bytes(0, 10) == 0 and L.pn_part_moments_workspace_bytes(2, 1000) > 0
    assert L.pn_icp_score_workspace_bytes(1, 10, 0) == 0 and L.pn_icp_score_workspace_bytes(1, 10, 4097) == 0
    # the scorer's workspace holds the bucketing and one partial per block of 256 samples and block of poses
    assert L.pn_icp_score_workspace_bytes(2, 5000, 37) > L.pn_icp_score_workspace_bytes(2, 5000, 5) >= 2 * 5000 * 4


def _seg(*v):
    return (C.c_int32 * len(v))(*v)


def _moments(p=None, B=1, N=64, n_parts=2, ws=WS):
    from pointcloudprocessing_amd import _lib
    g = lambda k: (p or {}).get(k, FAKE)                                      # noqa: E731
    return _lib.lib().pn_part_moments(g("scan"), g("labels"), B, N, n_parts, g("out"), g("ws"), ws, None)


def _seeds(p=None, B=1, n_parts=2, K=4):
    from pointcloudprocessing_amd import _lib
    g = lambda k: (p or {}).get(k, FAKE)                                      # noqa: E731
    return _lib.lib().pn_icp_seed_poses(g("mom"), g("rmom"), B, n_parts, g("rot"), K, g("out"), None)


def _score(p=None, B=1, N=64, seg=None, M=8, n_parts=2, K=5, stride=1, max_d2=4.0, ws=WS):
    from pointcloudprocessing_amd import _lib
    g = lambda k: (p or {}).get(k, FAKE)                                      # noqa: E731
    return _lib.lib().pn_icp_score_poses(g("scan"), g("labels"), B, N, g("ref"), seg or _seg(0, 4, M), M, n_parts, g("poses"), K,
                                         stride, max_d2, g("score"), g("order"), g("ws"), ws, None)


def test_argument_checks_without_gpu():
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    cases = [
        (lambda: _moments({"scan": None}), b"null pointer"), (lambda: _moments({"out": None}), b"moments_out"),
        (lambda: _moments({"ws": None}), b"workspace"), (lambda: _moments(B=0), b"B=0"), (lambda: _moments(N=0), b"N=0"),
        (lambda: _moments(n_parts=0), b"n_parts=0"), (lambda: _moments(n_parts=17), b"n_parts=17"),
        (lambda: _moments(ws=L.pn_part_moments_workspace_bytes(1, 64) - 1), b"workspace"),
        (lambda: _seeds({"mom": None}), b"null pointer"), (lambda: _seeds({"rmom": None}), b"ref_moments"),
        (lambda: _seeds({"out": None}), b"poses_out"), (lambda: _seeds({"rot": None}), b"rotations"), (lambda: _seeds(K=-1), b"K=-1"),
        (lambda: _seeds(n_parts=17), b"n_parts=17"), (lambda: _seeds(B=0), b"B=0"),
        (lambda: _score({"scan": None}), b"null pointer"), (lambda: _score({"ref": None}), b"null pointer"),
        (lambda: _score({"poses": None}), b"poses"), (lambda: _score({"score": None}), b"score_out"),
        (lambda: _score({"order": None}), b"order_out"), (lambda: _score(K=0), b"K=0"), (lambda: _score(K=4097), b"K=4097"),
        (lambda: _score(stride=0), b"stride=0"), (lambda: _score(max_d2=0.0), b"max_d2"), (lambda: _score(max_d2=-1.0), b"max_d2"),
        (lambda: _score(max_d2=float("inf")), b"max_d2"), (lambda: _score(max_d2=float("nan")), b"max_d2"),
        (lambda: _score(B=0), b"B=0"), (lambda: _score(N=0), b"N=0"), (lambda: _score(M=0, seg=_seg(0, 0, 0)), b"M=0"),
        (lambda: _score(n_parts=17), b"n_parts=17"), (lambda: _score(seg=_seg(0, 5, 4), M=4), b"not monotone"),
        (lambda: _score(seg=_seg(0, 4, 7)), b"end at M"),
        (lambda: _score(ws=L.pn_icp_score_workspace_bytes(1, 64, 5) - 1), b"workspace"),
    ]
    for call, msg in cases:
        assert call() == -1
        assert msg in L.pn_last_error(), (msg, L.pn_last_error())


def test_errors_raise_through_ops_without_gpu():
    import torch
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd._lib import PointNetHipError
    scan, lab = torch.zeros(1, 8, 3), torch.zeros(1, 8, dtype=torch.int32)
    ref = ops.icp_reference(np.zeros((4, 3), np.float32), np.zeros(4), 1, device=torch.device("cpu"))
    for md in (float("inf"), float("nan"), 0.0):
        with pytest.raises(PointNetHipError, match="max_dist"):
            ops.global_pose(scan, lab, ref, md)
    with pytest.raises(PointNetHipError, match="top"):
        ops.global_pose(scan, lab, ref, 3.0, top=0)
    with pytest.raises(PointNetHipError):                         # no CPU fallback
        ops.global_pose(scan, lab, ref, 3.0)
    with pytest.raises(PointNetHipError):
        ops.part_moments(scan, lab, 1)
    with pytest.raises(PointNetHipError):
        ops.icp_score_poses(scan, lab, ref, torch.eye(4, dtype=torch.float64)[None, None], 3.0)
    with pytest.raises(PointNetHipError):
        ops.icp_part_moments(object())
    with pytest.raises(PointNetHipError):
        ops.rotation_grid(0)


@pytest.mark.parametrize("n", [1, 7, 256])
def test_rotation_grid(n):
    from pointcloudprocessing_amd import ops
    R = ops.rotation_grid(n)
    assert tuple(R.shape) == (n, 3, 3) and str(R.dtype) == "torch.float64" and not R.is_cuda
    R = R.numpy()
    assert np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)).max() < 1e-14
    assert np.abs(np.linalg.det(R) - 1.0).max() < 1e-14
    assert np.abs(R - GO.rotation_grid(n)).max() < 1e-14
    if n == 256:
        ang = np.array([[IO.rotation_angle(R[i], R[j]) for j in range(n)] for i in range(0, n, 16)])
        ang[np.arange(len(ang)), np.arange(0, n, 16)] = np.inf
        # pairwise distinct, and spread: SO(3) has volume 8 pi^2 in the rotation-angle metric, so 256 uniform rotations sit about
        # (8 pi^2 / 256)^(1/3) = 0.68 rad apart; a third of that is asked of the nearest pair
        assert ang.min() > 0.2
        d = np.abs(R[:, None] - R[None]).max((2, 3))
        d[np.arange(n), np.arange(n)] = np.inf
        assert d.min() > 1e-2


def test_oracle_moments_seeds_and_score_agree_with_their_definitions():
    xyz, part, ref, seg = GO.kc46(NP)
    scan, lab, T = GO.case(2, False, NP)
    mom = GO.part_moments(scan[None], lab[None], NP)
    assert mom[0, :, 0].sum() == (lab >= 0).sum() and np.allclose(mom[0, :, 1:].sum(0), scan[lab >= 0].astype(np.float64).sum(0))
    rmom = GO.ref_moments_cloud(ref, seg, NP)
    assert rmom[:, 0].tolist() == np.diff(seg).tolist()
    seeds = GO.seed_poses(mom, rmom, GO.rotation_grid(5))
    assert seeds.shape == (1, 6, 4, 4) and np.array_equal(seeds[0, :, 3], np.tile([0, 0, 0, 1.0], (6, 1)))
    # pose K: the fit of the part centroids is an independent Horn fit of the same weighted centroid pairs
    sh = np.flatnonzero((mom[0, :, 0] > 0) & (rmom[:, 0] > 0))
    w = mom[0, sh, 0].astype(int)
    Rh, th = IO.horn(np.repeat(rmom[sh, 1:] / rmom[sh, :1], w, 0), np.repeat(mom[0, sh, 1:] / mom[0, sh, :1], w, 0))
    assert np.abs(seeds[0, 5, :3, :3] - Rh).max() < 1e-9 and np.abs(seeds[0, 5, :3, 3] - th).max() < 1e-8
    assert IO.pose_error(seeds[0, 5], T)[0] < np.deg2rad(15)          # full view: the centroid fit lands near the truth
    # one pose, stride 1: count and cost follow icp_oracle.correspond's d2
    md = np.float32(4.0)
    score, order = GO.score_poses(scan[None], lab[None], ref, seg, NP, seeds[:, 5:6], 1, md)
    d2 = IO.correspond(scan[None], lab[None], ref, seg, NP, seeds[:, 5].astype(np.float32))[1][0]
    act = IO.active(scan[None], lab[None], seg, NP)[0]
    assert score[0, 0, 0] == (d2[act] <= md).sum() and order.tolist() == [[0]]
    assert abs(score[0, 0, 1] - np.minimum(d2[act], md).astype(np.float64).sum()) < 1e-9
    # a NaN pose scores the worst cost, every sampled point at max_d2
    bad = seeds[:, :2].copy()
    bad[0, 0, 0, 0] = np.nan
    s2, o2 = GO.score_poses(scan[None], lab[None], ref, seg, NP, bad, 3, md)
    n_s = len(GO.sample(scan, lab, seg, NP, 3))
    assert s2[0, 0].tolist() == [0.0, float(md) * n_s] and o2.tolist() == [[1, 0]]


@pytest.mark.parametrize("seed,one_sided", GO.CASES)
def test_oracle_pipeline_recovers_the_pose(seed, one_sided):
    """moments -> 256 + 1 seeds -> score (stride 4) -> refine the best 4 (40 iterations, max_dist 3 m) -> select: within
    1e-2 rad and 5e-2 m of the truth (a cap; a throwaway restatement measured at most 6.5e-4 rad and 8.1e-3 m on these cases), and
    the top-4 set is separated from the fifth candidate, which the comparison of the device's top set with this one needs."""
    r = GO.solved(seed, one_sided, NP)
    _, _, T = GO.case(seed, one_sided, NP)
    ang, dt = IO.pose_error(r["pose"][0], T)
    c = r["coarse"][0, r["order"][0], 1]
    gap = (c[4] - c[3]) / c[4]
    print(f"seed {seed} one-sided {one_sided}: true angle {np.rad2deg(IO.rotation_angle(T[:3, :3], np.eye(3))):.1f} deg, winner "
          f"{int(r['winner'][0])}, {ang:.3e} rad, {dt:.3e} m, gap between the 4th and 5th coarse cost {gap:.3e}")
    assert ang < GO.CAP_ROT and dt < GO.CAP_T, (ang, dt)
    assert gap > 1e-6
    assert r["top"].shape == (1, 4) and r["winner"][0] in r["top"][0] and r["cost"][0] == r["fine"][0].min()


def test_local_solver_alone_fails_on_the_171_degree_case():
    """full view, seed 1: the true rotation is 171 degrees; icp_oracle.icp from [I | c_s - c_r] does not reach the bound"""
    _, _, ref, seg = GO.kc46(NP)
    scan, lab, T = GO.case(1, False, NP)
    assert IO.rotation_angle(T[:3, :3], np.eye(3)) > np.deg2rad(170)
    mom, rmom = GO.part_moments(scan[None], lab[None], NP), GO.ref_moments_cloud(ref, seg, NP)
    start = GO.seed_poses(mom, rmom, np.eye(3)[None])[:, 0]                       # [I | c_s - c_r]
    assert np.array_equal(start[0, :3, :3], np.eye(3))
    pose = IO.icp(scan[None], lab[None], ref, seg, NP, start, max_iters=GO.PARAMS["max_iters"], max_d2=GO.max_d2_of(GO.MAX_DIST))[0]
    ang, dt = IO.pose_error(pose[0], T)
    print(f"plain ICP from the centroid start: {ang:.3e} rad, {dt:.3e} m from the truth")
    assert not (ang < GO.CAP_ROT and dt < GO.CAP_T)
