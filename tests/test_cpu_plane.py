"""pn_plane_segment / ops.plane_segment / ops.plane_mask / remove_planes= without a GPU: the declared surface, the argument checks
(they run before any HIP call), and the NumPy oracle's own facts (tests/plane_oracle.py): exact integer arithmetic on a lattice, the
inclusive threshold, the tie rule, collinear clouds, the stop rules of the loop, and the four conditions the scene fixture must meet."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import plane_oracle as PO
from helpers import ROOT

F32 = np.float32
INVALID = -1


# ---- the library on the CPU -----------------------------------------------------------------------------------------
def test_surface_is_declared_and_exported():
    from pointcloudprocessing_amd import _lib, ops
    from pointcloudprocessing_amd.pointnet.PointNet import PointNet
    hdr = open(os.path.join(ROOT, "include", "pointnet_hip.h")).read()
    for decl in ("size_t pn_plane_segment_workspace_bytes(int N, int hypotheses, int max_planes);", "int pn_plane_segment(const float* xyz, int N,",
                 "#define PN_PLANE_TILE 1024", "#define PN_PLANE_MAX_HYPOTHESES 4096", "#define PN_PLANE_MAX_PLANES 8", "0x504C414E",
                 "s*s <= t2", "the lowest h among ties"):
        assert decl in hdr, decl
    assert "#define PN_ABI_VERSION 6" in hdr and _lib.lib().pn_abi_version() == 6 == _lib.ABI_VERSION      # additive: the version stays
    for name in ("pn_plane_segment_workspace_bytes", "pn_plane_segment"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert len(_lib.SIGNATURES["pn_plane_segment"][1]) == 16 and _lib.SIGNATURES["pn_plane_segment"][1][6] is C.c_uint64
    assert (_lib.PN_PLANE_TILE, _lib.PN_PLANE_MAX_HYPOTHESES, _lib.PN_PLANE_MAX_PLANES) == (PO.TILE, PO.MAX_H, PO.MAX_P) == (1024, 4096, 8)
    par = inspect.signature(ops.plane_segment).parameters
    assert list(par) == ["xyz", "threshold", "max_planes", "hypotheses", "min_inliers", "seed", "axis", "max_angle_deg", "return_hypotheses"]
    assert [par[k].default for k in list(par)[2:]] == [1, 1024, 3, 0, None, None, False]
    assert callable(ops.plane_mask)
    for fn in (PointNet.predict_scan, PointNet.predict_pose):
        assert inspect.signature(fn).parameters["remove_planes"].default is None


def _call(xyz=0x1000, N=8, threshold=0.1, H=16, P=2, min_inliers=3, seed=0, axis=None, cos=0.5, planes=0x1000, counts=0x1000, plane_id=0x1000,
          hyp=0, ws=0x1000, ws_bytes=None):
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    p = lambda a: C.c_void_p(a) if a else None      # noqa: E731  (never dereferenced: the checks run before any HIP call)
    if ws_bytes is None:
        ws_bytes = L.pn_plane_segment_workspace_bytes(N, H, P)
    rc = L.pn_plane_segment(p(xyz), N, threshold, H, P, min_inliers, seed, (C.c_float * 3)(*axis) if axis else None, cos, p(planes), p(counts),
                            p(plane_id), p(hyp), p(ws), ws_bytes, None)
    return rc, L.pn_last_error()


@pytest.mark.parametrize("kw,msg", [
    (dict(xyz=0), b"null pointer"), (dict(planes=0), b"null pointer"), (dict(counts=0), b"null pointer"), (dict(plane_id=0), b"null pointer"),
    (dict(N=0, ws_bytes=1 << 20), b"N=0"), (dict(N=-3, ws_bytes=1 << 20), b"N=-3"), (dict(N=(1 << 24) + 1, ws_bytes=1 << 30), b"outside [1, 2^24]"),
    (dict(H=0, ws_bytes=1 << 20), b"hypotheses=0"), (dict(H=4097, ws_bytes=1 << 20), b"hypotheses=4097"),
    (dict(P=0, ws_bytes=1 << 20), b"max_planes=0"), (dict(P=9, ws_bytes=1 << 20), b"max_planes=9"),
    (dict(threshold=-0.1), b"threshold"), (dict(threshold=float("nan")), b"threshold"), (dict(threshold=float("inf")), b"threshold"),
    (dict(threshold=1e20), b"threshold * threshold"),
    (dict(axis=(0.0, 0.0, 0.0)), b"zero vector"), (dict(axis=(0.0, float("nan"), 1.0)), b"axis must be finite"),
    (dict(axis=(float("inf"), 0.0, 1.0)), b"axis must be finite"), (dict(axis=(0.0, 0.0, 1.0), cos=1.5), b"cos_max_angle"),
    (dict(axis=(0.0, 0.0, 1.0), cos=-0.1), b"cos_max_angle"), (dict(axis=(0.0, 0.0, 1.0), cos=float("nan")), b"cos_max_angle"),
    (dict(ws=0), b"workspace"), (dict(ws_bytes=64), b"workspace too small"), (dict(ws=0x1008), b"16-byte aligned"),
])
def test_argument_checks_without_gpu(kw, msg):
    rc, err = _call(**kw)
    assert rc == INVALID and msg in err, err


def test_workspace_size():
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    sizes = [L.pn_plane_segment_workspace_bytes(n, 256, 3) for n in (1, 2, 1023, 1024, 1025, 4096, 100000, 1 << 20, 1 << 24)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
    assert all(L.pn_plane_segment_workspace_bytes(n, 4096, 8) >= 16 * n + 4 * 4096 * 8 for n in (1, 4096, 131072))       # the list and the counts
    for bad in ((0, 16, 1), (-1, 16, 1), ((1 << 24) + 1, 16, 1), (8, 0, 1), (8, 4097, 1), (8, 16, 0), (8, 16, 9)):
        assert L.pn_plane_segment_workspace_bytes(*bad) == 0


def test_ops_wrappers_refuse_cpu_tensors_and_bad_keywords():
    import torch
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd._lib import PointNetHipError
    with pytest.raises(PointNetHipError):
        ops.plane_segment(torch.zeros(8, 3), 0.1)                           # no CPU fallback
    with pytest.raises(PointNetHipError):
        ops.plane_segment(np.zeros((8, 3), F32), 0.1)
    pid = torch.tensor([-1, 0, 2, -1, 1], dtype=torch.int32)
    assert ops.plane_mask(pid).tolist() == [True, False, False, True, False]


# ---- the oracle's own facts -----------------------------------------------------------------------------------------
def test_draws_are_a_function_of_seed_round_and_list_length():
    a = PO.draws(1000, 0, 64, 0)
    assert a.shape == (64, 3) and a.min() >= 0 and a.max() < 1000
    assert np.array_equal(a, PO.draws(1000, 0, 64, 0)) and np.array_equal(a[:16], PO.draws(1000, 0, 16, 0))
    for other in (PO.draws(1000, 1, 64, 0), PO.draws(1000, 0, 64, 1), PO.draws(1000, 0, 64, 1 << 32)):
        assert not np.array_equal(a, other)
    assert np.array_equal(PO.draws(1, 0, 64, 5), np.zeros((64, 3), np.int64))          # one row: every hypothesis draws it three times
    assert PO.draws((1 << 24), 3, 64, 9).max() < 1 << 24


@pytest.mark.parametrize("threshold,num,den", [(1.0, 1, 1), (0.5, 1, 4)])
def test_lattice_scores_are_exact_and_the_threshold_is_inclusive(threshold, num, den):
    x = PO.lattice()
    act = np.ones(len(x), bool)
    hyp = PO.hypotheses(x, act, 0, 256, threshold)
    assert hyp["valid"].sum() > 200 and np.abs(hyp["c"]).max() <= 98 and np.array_equal(hyp["c"], np.rint(hyp["c"]))
    counts = PO.score(x, act, hyp)
    exact = PO.lattice_counts_exact(x, hyp)(num, den)
    assert np.array_equal(counts, exact)                                      # fp32 == integer arithmetic: every product is exact
    # points at exactly the threshold distance exist and count: with `<` in place of `<=` the scores drop
    xi, p0, c = x.astype(np.int64), hyp["p0"].astype(np.int64), hyp["c"].astype(np.int64)
    on_edge = sum(int((den * ((xi - p0[h]) @ c[h]) ** 2 == num * int(c[h] @ c[h])).sum()) for h in np.flatnonzero(hyp["valid"]))
    # (no lattice point lies at exactly 1/2 from a lattice plane: s = |c| / 2 needs a primitive normal of even length, whose squared
    # length would be 0 mod 4 with an odd component)
    assert on_edge > 50 if threshold == 1.0 else on_edge == 0
    # massive ties, and the winner is the lowest h among them
    win = PO.select(counts)
    assert win == int(np.flatnonzero(counts == counts.max())[0]) and (threshold != 1.0 or (counts == counts.max()).sum() >= 2)
    assert len(np.unique(counts[hyp["valid"]])) < hyp["valid"].sum() // 2


def test_the_tie_rule_picks_the_lowest_h():
    assert PO.select(np.array([3, 7, 7, -1, 7], np.int32)) == 1
    assert PO.select(np.array([-1, -1, 4, 4], np.int32)) == 2
    assert PO.select(np.array([-1, -1, -1], np.int32)) == -1
    # two copies of one plane's points: every hypothesis that hits the plane scores the same
    x = np.array([[i, j, 0] for i in range(6) for j in range(6)] * 2, F32)
    counts, win, plane, mask = PO.round(x, np.ones(len(x), bool), 0, 0.5, 64)
    assert counts.max() == 72 and (counts == 72).sum() > 10 and win == int(np.flatnonzero(counts == 72)[0])
    assert np.allclose(np.abs(plane), [0, 0, 1, 0], atol=1e-12) and mask.all()


def test_collinear_clouds_have_no_valid_hypothesis():
    x = PO.collinear()
    counts, win, plane, mask = PO.round(x, np.ones(len(x), bool), 0, 0.5, 128)
    assert (counts == -1).all() and win == -1 and plane is None and mask is None
    planes, cnt, pid, hc = PO.segment(x, 0.5, 3, 128)
    assert not planes.any() and not cnt.any() and (pid == -1).all() and (hc[0] == -1).all() and (hc[1:] == -1).all()


def test_small_and_bad_inputs():
    for n in (1, 2):
        planes, cnt, pid, hc = PO.segment(PO.random_cloud(n), 0.05, 2, 16)
        assert not planes.any() and not cnt.any() and (pid == -1).all() and (hc == -1).all()
    x = PO.random_cloud(500, seed=2)
    x[[0, 250, 499]] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]]
    act = PO.active_rows(x)
    assert act.sum() == 497
    counts, win, plane, mask = PO.round(x, act, 0, 0.05, 64)
    assert win >= 0 and not mask[[0, 250, 499]].any() and mask.sum() > 100
    # the axis constraint only ever invalidates hypotheses
    free = PO.hypotheses(x, act, 0, 64, 0.05)
    tied = PO.hypotheses(x, act, 0, 64, 0.05, axis=(0, 0, 1), cos_max_angle=np.cos(np.radians(10.0)))
    assert (tied["valid"] <= free["valid"]).all() and 0 < tied["valid"].sum() < free["valid"].sum()


def test_min_inliers_voids_a_round_and_stops_the_rest():
    x, tag = PO.floor_and_wall()
    planes, cnt, pid, hc = PO.segment(x, 0.03, 3, 128, min_inliers=1000)
    assert cnt[0] >= 1500 and cnt[1] >= 1400 and cnt[2] == 0 and not planes[2].any() and (hc[2] >= -1).all() and hc[2].max() > 0
    assert set(np.unique(pid)) == {-1, 0, 1}
    planes, cnt, pid, hc = PO.segment(x, 0.03, 3, 128, min_inliers=5000)
    assert not planes.any() and not cnt.any() and (pid == -1).all() and hc[0].max() > 1000 and (hc[1:] == -1).all()


def test_axis_constraint_picks_floor_or_wall():
    x, tag = PO.floor_and_wall()
    cos = np.cos(np.radians(10.0))
    for axis, want in (((0, 0, 1), 0), ((1, 0, 0), 1)):
        planes, cnt, pid, hc = PO.segment(x, 0.03, 1, 128, 3, 0, axis, cos)
        assert abs(planes[0][:3] @ np.asarray(axis, float)) > 0.999 and (pid[tag == want] == 0).all() and (pid[tag == 1 - want] == 0).mean() < 0.05


def test_the_scene_fixture_meets_its_conditions():
    """two planes and a void third round, every floor and wall row labelled, no aircraft row labelled, and the largest cluster of
    the untouched scene holds the floor: conditions on the fixture, checked with the oracle alone"""
    import cluster_oracle as CO
    scene, air, floor, wall, clean = PO.floor_scene()
    assert (len(air), len(floor), len(wall)) == (4096, 6000, 3000) and np.array_equal(scene[air], clean)
    S = PO.SCENE
    planes, cnt, pid, hc = PO.segment(scene, S["threshold"], S["max_planes"], S["hypotheses"], S["min_inliers"])
    assert cnt[0] >= S["min_inliers"] and cnt[1] >= S["min_inliers"] and cnt[2] == 0 and not planes[2].any() and hc[2].max() > 0
    assert (pid[floor] >= 0).all() and (pid[wall] >= 0).all() and (pid[air] == -1).all() and cnt[:2].sum() == 9000
    cl = CO.voxel_clusters(scene, PO.SCENE_CLUSTER_LEAF, scene.min(0), 26)
    big = int(np.flatnonzero(cl[2] == cl[2].max())[0])
    assert (cl[0][floor] == big).sum() > 0
    rest = scene[pid < 0]
    cl2 = CO.voxel_clusters(rest, PO.SCENE_CLUSTER_LEAF, rest.min(0), 26)
    big2 = int(np.flatnonzero(cl2[2] == cl2[2].max())[0])
    assert np.array_equal(rest[cl2[0] == big2], clean)
