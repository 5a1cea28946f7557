"""Point-to-plane semantic ICP without a GPU: the declared surface, argument checks that run before any HIP call, metric="plane"
without normals, and the NumPy oracle (tests/icp_plane_oracle.py): normals of planes and spheres, the sign rule, the linear terms
against a finite difference, a noise-free pose, and the unobservable directions of a single planar part."""
import ctypes as C
import os

import numpy as np
import pytest

import icp_oracle as IO
import icp_plane_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pn_icp_normals", "pn_icp_plane_workspace_bytes", "pn_icp_plane_sums", "pn_icp_plane_solve", "pn_semantic_icp_plane")


def test_surface_is_declared_and_exported():
    from pointcloudprocessing_amd import _lib, ops
    from pointcloudprocessing_amd.pointnet.PointNet import PointNet
    hdr = open(os.path.join(ROOT, "include", "pointnet_hip.h")).read()
    for name in NEW:
        assert f"{name}(" in hdr and name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert "#define PN_ICP_DEGENERATE 4" in hdr and "#define PN_ABI_VERSION 6" in hdr and _lib.lib().pn_abi_version() == 6
    for f in (ops.icp_normals, ops.icp_plane_sums, ops.icp_plane_solve):
        assert callable(f)
    assert "metric" in PointNet.predict_pose.__doc__
    L = _lib.lib()
    assert L.pn_icp_plane_workspace_bytes(2, 131072, 490, 12) > L.pn_icp_workspace_bytes(2, 131072, 490, 12)
    assert L.pn_icp_plane_workspace_bytes(0, 10, 4, 1) == 0


def _seg(*v):
    return (C.c_int32 * len(v))(*v)


FAKE = C.c_void_p(0x1000)        # never dereferenced: the checks run before any HIP call
WS = 1 << 30


@pytest.mark.parametrize("kw,msg", [
    (dict(k=2), b"k=2"), (dict(k=17), b"k=17"), (dict(M=0, seg=_seg(0, 0, 0)), b"M=0"), (dict(n_parts=0, seg=_seg(0)), b"n_parts=0"),
    (dict(seg=_seg(0, 9, 8)), b"not monotone"), (dict(seg=_seg(0, 4, 7)), b"end at M"), (dict(ref=None), b"null pointer"),
    (dict(out=None), b"null pointer"),
])
def test_normals_argument_checks_without_gpu(kw, msg):
    from pointcloudprocessing_amd import _lib
    a = dict(ref=FAKE, seg=_seg(0, 4, 8), M=8, n_parts=2, k=4, out=FAKE)
    a.update(kw)
    assert _lib.lib().pn_icp_normals(a["ref"], a["seg"], a["M"], a["n_parts"], a["k"], a["out"], FAKE, FAKE, None) == -1
    assert msg in _lib.lib().pn_last_error(), _lib.lib().pn_last_error()


def _sums_call(ptrs=None, seg=None, M=8, n_parts=2, ws=WS, max_d2=float("inf")):
    from pointcloudprocessing_amd import _lib
    p = ptrs or {}
    g = lambda k: p.get(k, FAKE)                                              # noqa: E731
    return _lib.lib().pn_icp_plane_sums(g("scan"), g("labels"), 1, 64, g("ref"), seg or _seg(0, 4, M), M, n_parts, g("pose32"), max_d2,
                                        g("normals"), g("pose64"), g("idx"), g("d2"), g("sums"), g("ws"), ws, None)


def _loop_call(ptrs=None, max_iters=5, max_d2=float("inf"), tol=(1e-6, 1e-6), ws=WS):
    from pointcloudprocessing_amd import _lib
    p = ptrs or {}
    g = lambda k: p.get(k, FAKE)                                              # noqa: E731
    return _lib.lib().pn_semantic_icp_plane(g("scan"), g("labels"), 1, 64, g("ref"), _seg(0, 4, 8), 8, 2, g("init"), max_iters, max_d2,
                                            tol[0], tol[1], g("normals"), g("pose"), g("rmse"), g("pairs"), g("iters"), g("status"),
                                            g("ws"), ws, None)


def test_plane_argument_checks_without_gpu():
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    short = L.pn_icp_plane_workspace_bytes(1, 64, 8, 2) - 1
    assert L.pn_icp_workspace_bytes(1, 1024, 8, 2) < L.pn_icp_plane_workspace_bytes(1, 1024, 8, 2)    # 29 sums per block, not 18
    cases = [
        (lambda: _sums_call({"normals": None}), b"ref_normals"), (lambda: _sums_call({"pose64": None}), b"pose64"),
        (lambda: _sums_call({"sums": None}), b"sums_out"), (lambda: _sums_call(ws=short), b"workspace"),
        (lambda: _sums_call(seg=_seg(0, 5, 4), M=4), b"not monotone"), (lambda: _sums_call(max_d2=float("nan")), b"max_d2 is NaN"),
        (lambda: _loop_call({"normals": None}), b"ref_normals"), (lambda: _loop_call(max_iters=0), b"max_iters=0"),
        (lambda: _loop_call(max_d2=float("nan")), b"max_d2 is NaN"), (lambda: _loop_call(tol=(-1.0, 0.0)), b"tolerances"),
        (lambda: _loop_call(ws=short), b"workspace"), (lambda: _loop_call({"status": None}), b"null pointer"),
        (lambda: L.pn_icp_plane_solve(None, 1, FAKE, FAKE, FAKE, None), b"null pointer"),
        (lambda: L.pn_icp_plane_solve(FAKE, 0, FAKE, FAKE, FAKE, None), b"B=0"),
    ]
    for call, msg in cases:
        assert call() == -1
        assert msg in L.pn_last_error(), (msg, L.pn_last_error())


def test_plane_metric_needs_normals():
    import torch
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd._lib import PointNetHipError
    xyz = np.arange(24, dtype=np.float32).reshape(8, 3)
    lab = np.array([0, 0, 0, 0, 1, 1, 1, 1])
    ref = ops.icp_reference(xyz, lab, 2, device=torch.device("cpu"))
    assert ref.normals is None
    scan, labels, init = torch.zeros(1, 8, 3), torch.zeros(1, 8, dtype=torch.int32), torch.eye(4)[None].double()
    with pytest.raises(PointNetHipError, match="normals"):
        ops.semantic_icp(scan, labels, ref, init, metric="plane")
    with pytest.raises(PointNetHipError, match="metric"):
        ops.semantic_icp(scan, labels, ref, init, metric="planar")
    with pytest.raises(PointNetHipError):
        ops.icp_plane_solve(torch.zeros(1, 29, dtype=torch.float64), torch.eye(4)[None].double())


def test_icp_reference_groups_normals():
    import torch
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd._lib import PointNetHipError
    xyz = np.arange(24, dtype=np.float32).reshape(8, 3)
    nrm = -np.arange(24, dtype=np.float32).reshape(8, 3)
    lab = np.array([2, 0, -1, 2, 0, 5, 1, 0])
    r = ops.icp_reference(xyz, lab, 3, device=torch.device("cpu"), normals=nrm)
    assert r.normals.dtype == torch.float32 and np.array_equal(r.normals.numpy(), nrm[[1, 4, 7, 6, 0, 3]])
    with pytest.raises(PointNetHipError):
        ops.icp_reference(xyz, lab, 3, device=torch.device("cpu"), normals=nrm[:5])


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------
def _pose(R, t):
    P = np.eye(4)
    P[:3, :3] = R
    P[:3, 3] = t
    return P


def _plate(rng, n, origin, e1, e2):
    s, t = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    return (np.asarray(origin) + s[:, None] * np.asarray(e1, np.float64) + t[:, None] * np.asarray(e2, np.float64)).astype(np.float32)


def test_oracle_normals_of_a_plane_and_a_sphere():
    rng = np.random.default_rng(0)
    e1, e2 = np.array([3.0, -1.0, 2.0]), np.array([0.5, 2.0, -4.0])
    true_n = np.cross(e1, e2) / np.linalg.norm(np.cross(e1, e2))
    plate = _plate(rng, 300, [1.0, 2.0, 3.0], e1, e2)
    v = rng.normal(size=(800, 3))
    sphere = (5.0 * v / np.linalg.norm(v, axis=1, keepdims=True) + [10.0, -3.0, 2.0]).astype(np.float32)
    ref = np.concatenate([plate, sphere])
    seg = np.array([0, 300, 1100])
    nrm, curv, nbr = PO.normals(ref, seg, 2, 10)
    assert np.isfinite(nrm).all() and nbr.shape == (1100, 10) and (nbr >= 0).all()
    assert (nbr[:300] < 300).all() and (nbr[300:] >= 300).all()                 # the same label only
    assert (nbr[:, 0] == np.arange(1100)).all()                                  # the point itself is the nearest
    assert np.abs(np.abs(nrm[:300] @ true_n) - 1).max() < 1e-5 and np.abs(curv[:300]).max() < 1e-6
    radial = (sphere - [10.0, -3.0, 2.0]) / 5.0
    assert np.abs(np.abs((nrm[300:] * radial).sum(1))).min() > 0.98
    assert (curv[300:] > 1e-4).all() and (curv[300:] < 0.05).all()


def test_oracle_sign_rule_and_degenerate_points():
    rng = np.random.default_rng(1)
    # plane with normal (0.36, -0.8, 0.48): the largest component is y, so the normal is (-0.36, 0.8, -0.48)
    n = np.array([0.36, -0.8, 0.48])
    e1 = np.cross(n, [1.0, 0.0, 0.0])
    e2 = np.cross(n, e1)
    plate = _plate(rng, 50, [0.0, 0.0, 0.0], e1 * 3, e2 * 3)
    line = (np.arange(6, dtype=np.float64)[:, None] * [1.0, 2.0, 3.0]).astype(np.float32)     # collinear
    pair = np.array([[0, 0, 0], [1, 1, 1]], np.float32)                                      # fewer than 3 neighbours
    same = np.ones((4, 3), np.float32)                                                       # coincident
    ref = np.concatenate([plate, line, pair, same])
    seg = np.array([0, 50, 56, 58, 62])
    nrm, curv, nbr = PO.normals(ref, seg, 4, 8)
    assert np.abs(nrm[:50] - (-n)).max() < 1e-6 and (nrm[:50, 1] > 0).all()
    assert np.isnan(nrm[50:]).all() and np.isnan(curv[50:]).all()
    assert nbr[56].tolist() == [56, 57, -1, -1, -1, -1, -1, -1]
    assert nbr[58].tolist() == [58, 59, 60, 61, -1, -1, -1, -1]                             # ties -> lowest index


def test_oracle_linear_terms_match_finite_difference():
    rng = np.random.default_rng(2)
    pose = _pose(IO.rot([0.2, 1.0, -0.4], 0.8), [3.0, -2.0, 5.0])
    p = rng.normal(size=(20, 3)) * 4
    q = rng.normal(size=(20, 3)) * 4
    n = rng.normal(size=(20, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    r0, a = PO.pair_terms(p, q, n, pose)
    for k in range(6):
        for h in (1e-6, -1e-6):
            x = np.zeros(6)
            x[k] = h
            r1, _ = PO.pair_terms(p, q, n, PO.apply(pose, x))
            assert np.abs((r1 - r0) / h - a[:, k]).max() < 1e-5 * (1 + np.abs(a[:, k]).max())


def _box_scene(n_ref, n_scan, pose, seed):
    """three non-parallel plates, one label each: a noise-free pose is observable and the residual is 0 at it"""
    rng = np.random.default_rng(seed)
    plates = [([0.0, 0.0, 0.0], [6.0, 0.0, 0.0], [0.0, 5.0, 0.0]), ([0.0, 0.0, 0.0], [0.0, 5.0, 0.0], [0.0, 0.0, 4.0]),
              ([0.0, 0.0, 0.0], [6.0, 0.0, 0.0], [1.0, 0.0, 4.0])]
    ref = np.concatenate([_plate(rng, n_ref, *pl) for pl in plates])
    lab = np.repeat(np.arange(3), n_ref).astype(np.int32)
    q = np.concatenate([_plate(rng, n_scan, *pl) for pl in plates]).astype(np.float64)
    scan = (q @ pose[:3, :3].T + pose[:3, 3]).astype(np.float32)
    return ref, lab, scan, np.repeat(np.arange(3), n_scan).astype(np.int32)


def test_oracle_loop_recovers_noise_free_surface_pose():
    T = _pose(IO.rot([1, 2, 3], 0.4), [5.0, 2.0, -3.0])
    ref, lab, scan, slab = _box_scene(300, 2000, T, 3)
    nrm, _, _ = PO.normals(ref, np.array([0, 300, 600, 900]), 3, 10)
    start = _pose(IO.rot([0, 1, 1], np.deg2rad(5)) @ T[:3, :3], T[:3, 3] + [0.2, -0.3, 0.1])
    pose, rmse, pairs, iters, status = PO.icp(scan[None], slab[None], ref, np.array([0, 300, 600, 900]), 3, nrm, start[None],
                                              max_iters=30, tol_rot=1e-9, tol_t=1e-9)
    ang, dt = IO.pose_error(pose[0], T)
    assert status[0] == PO.CONVERGED and iters[0] <= 10 and pairs[0] == 6000, (iters, status)
    assert ang < 1e-6 and dt < 1e-5 and rmse[0] < 1e-5, (ang, dt, rmse)


def test_oracle_single_plane_leaves_unobservable_directions():
    rng = np.random.default_rng(4)
    ref = _plate(rng, 400, [-5.0, -5.0, 0.0], [10.0, 0.0, 0.0], [0.0, 10.0, 0.0])        # z = 0: normal (0, 0, 1)
    seg = np.array([0, 400])
    nrm, _, _ = PO.normals(ref, seg, 1, 10)
    assert np.abs(nrm - [0, 0, 1]).max() < 1e-6
    # the scan: the plane lifted by 0.3 and tilted a little, so every observable direction has something to correct
    q = _plate(rng, 3000, [-4.0, -4.0, 0.0], [8.0, 0.0, 0.0], [0.0, 8.0, 0.0]).astype(np.float64)
    T = _pose(IO.rot([1, 0.5, 0], np.deg2rad(2)), [0.0, 0.0, 0.3])
    scan = (q @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    lab = np.zeros((1, 3000), np.int32)
    idx, _, S = PO.plane_sums(scan[None], lab, ref, seg, 1, nrm, np.eye(4)[None])
    x, dropped = PO.step(S[0])
    assert dropped and abs(x[2]) < 1e-12 and abs(x[3]) < 1e-12 and abs(x[4]) < 1e-12          # rotation about z, shift in x, y
    assert np.abs(x[[0, 1, 5]]).max() > 1e-3
    P, rmse, st = PO.solve(S[0], np.eye(4))
    assert st == PO.DEGENERATE and np.isfinite(rmse)
    # the pose moves only in the observable directions: u' = E u + delta keeps x, y of the origin and the rotation about z
    w = PO.rodrigues(x[:3])
    assert abs(w[0, 1] - w[1, 0]) < 1e-12                                                    # no rotation about z
    pose, _, _, iters, status = PO.icp(scan[None], lab, ref, seg, 1, nrm, np.eye(4)[None], max_iters=20, tol_rot=1e-9, tol_t=1e-9)
    assert status[0] == PO.DEGENERATE | PO.CONVERGED and iters[0] <= 10
    u0 = np.linalg.inv(pose[0]) @ T @ [0.0, 0.0, 0.0, 1.0]          # where the model origin lands, in the estimated model frame
    assert abs(u0[2]) < 1e-6                                         # the height is recovered
    Rm = pose[0, :3, :3].T @ T[:3, :3]
    assert abs(np.arccos(np.clip(Rm[2, 2], -1, 1))) < 1e-6          # so is the tilt


def test_oracle_few_pairs_and_solve_by_hand():
    P0 = _pose(IO.rot([0, 1, 0], 0.3), [1.0, 2.0, 3.0])
    S = np.zeros(29)
    S[0] = 5
    P, rmse, st = PO.solve(S, P0)
    assert st == PO.FEW_PAIRS and np.array_equal(P, P0) and np.isnan(rmse)
    # a pure translation along the three axes: a = [u x n, n] with axis normals, the solve returns delta = -r per axis
    u = np.array([[0.0, 0.0, 0.0]] * 6)
    n = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])
    r = np.array([0.1, -0.1, -0.2, 0.2, 0.05, -0.05])
    a = np.concatenate([np.cross(u, n), n], 1)
    S = np.concatenate([[6], (a[:, :, None] * a[:, None, :]).sum(0)[np.triu_indices(6)], (a * r[:, None]).sum(0), [(r * r).sum()]])
    x, dropped = PO.step(S)
    assert dropped and np.abs(x - [0, 0, 0, -0.1, 0.2, -0.05]).max() < 1e-15
    P, rmse, st = PO.solve(S, np.eye(4))
    assert st == PO.DEGENERATE and np.abs(P - _pose(np.eye(3), [0.1, -0.2, 0.05])).max() < 1e-15
    assert abs(rmse - np.sqrt((r * r).mean())) < 1e-15
