"""Semantic ICP against a triangle mesh without a GPU: the declared surface, the argument checks that run before any HIP call, the
OBJ reader, ops.icp_mesh_reference, and the NumPy oracle (tests/icp_mesh_oracle.py): its fp32 closest point against an independent
fp64 construction, and its loop on a noise-free scan of the procedural aircraft against the sampled-cloud reference."""
import ctypes as C
import os

import numpy as np
import pytest

import icp_mesh_oracle as MO
import icp_oracle as IO
import icp_plane_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pn_icp_mesh_workspace_bytes", "pn_icp_mesh_correspond", "pn_semantic_icp_mesh")
F32 = np.float32
NM = len(MO.MESH_PARTS)


def test_surface_is_declared_and_exported():
    from pointcloudprocessing_amd import _lib, ops, pointcloud
    from pointcloudprocessing_amd.pointnet.PointNet import PointNet
    hdr = open(os.path.join(ROOT, "include", "pointnet_hip.h")).read()
    for name in NEW:
        assert f"{name}(" in hdr and name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert "#define PN_ABI_VERSION 6" in hdr and _lib.lib().pn_abi_version() == 6 and _lib.ABI_VERSION == 6
    assert "#define PN_ICP_METRIC_POINT 1" in hdr and "#define PN_ICP_METRIC_PLANE 2" in hdr
    for f in (ops.icp_mesh_reference, ops.icp_mesh_correspond, pointcloud.read_labelled_mesh):
        assert callable(f)
    assert isinstance(ops.IcpMeshReference, type)
    assert "IcpMeshReference" in PointNet.predict_pose.__doc__ and "IcpMeshReference" in ops.semantic_icp.__doc__
    L = _lib.lib()
    assert L.pn_icp_mesh_workspace_bytes(2, 131072, 80, 4) == L.pn_icp_plane_workspace_bytes(2, 131072, 80, 4)   # one layout, 29 sums
    assert L.pn_icp_mesh_workspace_bytes(0, 10, 4, 1) == 0


def _seg(*v):
    return (C.c_int32 * len(v))(*v)


FAKE = C.c_void_p(0x1000)        # never dereferenced: the checks run before any HIP call
WS = 1 << 30


def _corr_call(ptrs=None, seg=None, T=8, n_parts=2, ws=WS, max_d2=float("inf"), mode=0, B=1):
    from pointcloudprocessing_amd import _lib
    p = ptrs or {}
    g = lambda k: p.get(k, FAKE)                                              # noqa: E731
    return _lib.lib().pn_icp_mesh_correspond(g("scan"), g("labels"), B, 64, g("tri"), seg or _seg(0, 4, T), T, n_parts, g("pose32"),
                                             max_d2, mode, g("normals"), g("pose64"), g("idx"), g("d2"), g("q"), g("sums"), g("ws"), ws,
                                             None)


def _loop_call(ptrs=None, metric=1, max_iters=5, max_d2=float("inf"), tol=(1e-6, 1e-6), ws=WS, seg=None, T=8, n_parts=2):
    from pointcloudprocessing_amd import _lib
    p = ptrs or {}
    g = lambda k: p.get(k, FAKE)                                              # noqa: E731
    return _lib.lib().pn_semantic_icp_mesh(g("scan"), g("labels"), 1, 64, g("tri"), seg or _seg(0, 4, T), T, n_parts, g("normals"),
                                           metric, g("init"), max_iters, max_d2, tol[0], tol[1], g("pose"), g("rmse"), g("pairs"),
                                           g("iters"), g("status"), g("ws"), ws, None)


def test_mesh_argument_checks_without_gpu():
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    short = L.pn_icp_mesh_workspace_bytes(1, 64, 8, 2) - 1
    cases = [
        (lambda: _corr_call({"tri": None}), b"null pointer"), (lambda: _corr_call({"q": None}), b"q_out"),
        (lambda: _corr_call({"pose32": None}), b"pose32"), (lambda: _corr_call(mode=3), b"mode=3"),
        (lambda: _corr_call({"sums": None}, mode=1), b"sums_out"), (lambda: _corr_call({"normals": None}, mode=2), b"normals"),
        (lambda: _corr_call({"pose64": None}, mode=2), b"pose64"), (lambda: _corr_call(ws=short), b"workspace"),
        (lambda: _corr_call(max_d2=float("nan")), b"max_d2 is NaN"), (lambda: _corr_call(seg=_seg(0, 5, 4), T=4), b"not monotone"),
        (lambda: _corr_call(seg=_seg(0, 4, 7)), b"end at M"), (lambda: _corr_call(T=0, seg=_seg(0, 0, 0)), b"T=0"),
        (lambda: _corr_call(n_parts=17), b"n_parts=17"), (lambda: _corr_call(B=0), b"B=0"),
        (lambda: _loop_call(metric=0), b"metric=0"), (lambda: _loop_call(metric=3), b"metric=3"),
        (lambda: _loop_call({"normals": None}, metric=2), b"normals"), (lambda: _loop_call(max_iters=0), b"max_iters=0"),
        (lambda: _loop_call(max_d2=float("nan")), b"max_d2 is NaN"), (lambda: _loop_call(tol=(-1.0, 0.0)), b"tolerances"),
        (lambda: _loop_call(ws=short), b"workspace"), (lambda: _loop_call({"status": None}), b"null pointer"),
        (lambda: _loop_call({"scan": None}), b"null pointer"),
    ]
    for call, msg in cases:
        assert call() == -1
        assert msg in L.pn_last_error(), (msg, L.pn_last_error())


def test_mesh_reference_is_refused_where_a_cloud_is_needed():
    import torch
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd._lib import PointNetHipError
    v, f, p = MO.aircraft_mesh(0)
    m = ops.icp_mesh_reference(v, f, p, NM, device=torch.device("cpu"))
    with pytest.raises(PointNetHipError):
        ops.icp_normals(m)
    with pytest.raises(PointNetHipError, match="icp_mesh_reference"):
        ops.icp_mesh_correspond(torch.zeros(1, 8, 3), torch.zeros(1, 8, dtype=torch.int32), ops.icp_reference(v, np.zeros(len(v)), 1, device=torch.device("cpu")),
                                torch.eye(4)[None])
    with pytest.raises(PointNetHipError, match="sums"):
        ops.icp_mesh_correspond(torch.zeros(1, 8, 3), torch.zeros(1, 8, dtype=torch.int32), m, torch.eye(4)[None], sums="both")
    # the cloud passes refuse a mesh by its family, before they look at a tensor
    with pytest.raises(PointNetHipError, match="ref must come from ops.icp_reference"):
        ops.icp_correspond(torch.zeros(1, 8, 3), torch.zeros(1, 8, dtype=torch.int32), m, torch.eye(4)[None])
    with pytest.raises(PointNetHipError, match="ref must come from ops.icp_reference"):
        ops.icp_plane_sums(torch.zeros(1, 8, 3), torch.zeros(1, 8, dtype=torch.int32), m, torch.eye(4)[None].double())
    with pytest.raises(PointNetHipError, match="3 labels|faces"):
        ops.icp_mesh_reference(v, f, p[:3], NM, device=torch.device("cpu"))


# ---------------------------------------------------------------------------------------------------------------------
# the OBJ reader
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("style,use", [("i", "o"), ("i/t", "g"), ("i//n", "o"), ("i/t/n", "g")])
def test_obj_round_trip(tmp_path, style, use):
    from pointcloudprocessing_amd import pointcloud
    v, f, p = MO.aircraft_mesh(0)
    path = str(tmp_path / "aircraft.obj")
    MO.write_obj(path, v, f, p, MO.MESH_PARTS, style=style, use=use, header=("# a comment", "mtllib a.mtl", "usemtl grey", "s off"))
    rv, rf, rp = pointcloud.read_labelled_mesh(path, MO.MESH_PARTS)
    assert rv.dtype == np.float32 and rf.dtype == np.int32 and rp.dtype == np.int32
    assert np.array_equal(rv, v) and np.array_equal(rf, f) and np.array_equal(rp, p)


def test_obj_negative_indices_quads_names(tmp_path):
    from pointcloudprocessing_amd import pointcloud
    path = str(tmp_path / "m.obj")
    with open(path, "w") as fh:
        fh.write("# two parts\no Body\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvn 0 0 1\n"
                 "f 1/1/1 2/1/1 3/1/1 4/1/1\n"                      # a quad: fan from the first corner
                 "g left_wing\nv 0 0 1\nv 1 0 1\nv 0 1 1\n"
                 "f -3 -2 -1\n"                                     # relative: the last three vertices
                 "f 1 2 3 4 5\n"                                    # a pentagon: three triangles
                 "o Fin\nf 5//1 6//1 7//1\n")                       # a new object: its name, the stale group is dropped
    names = {"Body": "fuselage", "left_wing": "wing", "Fin": "vstab"}
    v, f, p = pointcloud.read_labelled_mesh(path, MO.MESH_PARTS, name_map=names)
    assert v.shape == (7, 3)
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [4, 5, 6], [0, 1, 2], [0, 2, 3], [0, 3, 4], [4, 5, 6]]
    assert p.tolist() == [0, 0, 1, 1, 1, 1, 2]                      # g wins over o while it is set
    # names that are part labels themselves need no map
    with open(path, "w") as fh:
        fh.write("v 0 0 0\nv 1 0 0\nv 0 1 0\no wing\ng hstab\nf 1 2 3\n")
    assert pointcloud.read_labelled_mesh(path, MO.MESH_PARTS)[2].tolist() == [3]
    with open(path, "w") as fh:
        fh.write("v 0 0 0\nv 1 0 0\nv 0 1 0\no wing\nf 1 2 3\ng gear\nf 1 2 3\n")
    with pytest.raises(ValueError, match="line 6"):
        pointcloud.read_labelled_mesh(path, MO.MESH_PARTS)
    with pytest.raises(ValueError, match="line 4"):
        pointcloud.read_labelled_mesh(path, MO.MESH_PARTS, name_map={"wing": "flap"})
    with open(path, "w") as fh:
        fh.write("o wing\nv 0 0 0\nv 1 0 0\nf 1 2 3\n")
    with pytest.raises(ValueError, match="out of range"):
        pointcloud.read_labelled_mesh(path, MO.MESH_PARTS)


# ---------------------------------------------------------------------------------------------------------------------
# ops.icp_mesh_reference
# ---------------------------------------------------------------------------------------------------------------------
def test_icp_mesh_reference_groups_and_drops():
    import torch
    from pointcloudprocessing_amd import ops
    rng = np.random.default_rng(0)
    v = rng.uniform(-5, 5, (30, 3)).astype(F32)
    v[29] = np.nan
    f = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11], [12, 13, 14], [15, 16, 17], [18, 19, 20],
                  [1, 1, 2],            # a repeated corner: zero area
                  [21, 22, 29],         # a NaN vertex
                  [23, 24, 25]])
    v[23], v[24], v[25] = [1, 1, 1], [2, 2, 2], [4, 4, 4]                          # collinear: zero area
    lab = np.array([2, 0, -1, 2, 0, 5, 1, 0, 1, 2])
    r = ops.icp_mesh_reference(v, f, lab, 3, device=torch.device("cpu"))
    assert r.index.tolist() == [1, 4, 6, 0, 3] and r.seg == (0, 2, 3, 5) and r.T == 5 and r.M == 5 and r.n_parts == 3
    assert r.tri.dtype == torch.float32 and tuple(r.tri.shape) == (5, 3, 3) and np.array_equal(r.tri.numpy(), v[f[r.index.numpy()]])
    assert r.normals.dtype == torch.float32 and r.area.dtype == torch.float64
    n, t = r.normals.numpy().astype(np.float64), r.tri.numpy().astype(np.float64)
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-7
    for e in (t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]):
        assert np.abs((n * e).sum(1)).max() < 1e-6 * np.linalg.norm(e, axis=1).max()
    assert np.allclose(r.area.numpy(), 0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1), rtol=1e-14)
    # the oracle groups the same way
    g = MO.group_mesh(v, f, lab, 3)
    assert np.array_equal(g[0], r.tri.numpy()) and g[1].tolist() == list(r.seg) and np.array_equal(g[2], r.index.numpy())
    assert np.array_equal(g[3], r.normals.numpy()) and np.array_equal(g[4], r.area.numpy())
    # the aircraft: nothing dropped, four parts, a closed surface (the area-weighted normals sum to zero)
    av, af, ap = MO.aircraft_mesh(1)
    a = ops.icp_mesh_reference(av, af, ap, NM, device=torch.device("cpu"))
    assert a.T == 320 and all(a.seg[k + 1] > a.seg[k] for k in range(NM))


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's closest point
# ---------------------------------------------------------------------------------------------------------------------
S = 32.0                 # every coordinate lies in [-S, S]
KAPPA = 4.0              # shape guard: (longest edge)^2 <= KAPPA * 2 * area
LE_MIN = S / 2           # shortest edge
U = 2.0 ** -24           # fp32 unit roundoff
# The fp32 closest point against fp64, derived from the coordinates' magnitude.  The point-vertex distances Lp are at most
# 2 sqrt(3) S.  A dot d_k = x.y of an edge vector (length <= Le) and a point-vertex vector has three products and two sums of
# magnitude <= Le Lp on operands that each carry one rounding: |error| <= 6 U Le Lp.  Edge regions: t = d / |edge|^2, so
# |error of t| <= 6 U Lp / Le and the point moves by Le times that: 6 U Lp.  Face: v = vb / (va + vb + vc) with the denominator
# (2 area)^2 >= (Le^2 / KAPPA)^2 and vb a difference of two products of dots, |error| <= 4 * 6 U Le^2 Lp^2 (two products, each of
# two dots with the relative error above, and their own roundings, all counted in the 4); the point moves by Le times the error of
# v and of w: 2 * 24 U KAPPA^2 Lp^2 / Le.  With Lp <= 2 sqrt(3) S and Le >= S / 2 that is 48 * 16 * 24 U S = 18432 U S (0.035 m at S = 32), which also
# covers the edge regions and the final sums (a few U S).  A point that changes region under rounding is covered because the
# closest point is continuous across region boundaries.
Q_BOUND = 2 * 24 * KAPPA ** 2 * (2 * np.sqrt(3) * S) ** 2 / LE_MIN * U


def _good_triangles(rng, n):
    out = []
    while sum(len(t) for t in out) < n:
        t = rng.uniform(-S, S, (4 * n, 3, 3)).astype(F32).astype(np.float64)
        e = np.stack([t[:, 1] - t[:, 0], t[:, 2] - t[:, 1], t[:, 0] - t[:, 2]], 1)
        le = np.linalg.norm(e, axis=2)
        area2 = np.linalg.norm(np.cross(e[:, 0], -e[:, 2]), axis=1)
        out.append(t[(le.max(1) ** 2 <= KAPPA * area2) & (le.min(1) >= LE_MIN)])
    return np.concatenate(out)[:n].astype(F32)


def test_oracle_closest_point_against_independent_fp64():
    assert abs(Q_BOUND - 18432 * U * S) < 1e-12
    rng = np.random.default_rng(11)
    n = 12000
    tri = _good_triangles(rng, n)
    pts = rng.uniform(-S, S, (n, 3)).astype(F32)
    # placed exactly: on vertices, on fp32 edge midpoints and at fp32 face centres
    k = 500
    pts[0:k] = tri[0:k, 0]
    pts[k:2 * k] = tri[k:2 * k, 2]
    pts[2 * k:3 * k] = ((tri[2 * k:3 * k, 0] + tri[2 * k:3 * k, 1]) * F32(0.5)).astype(F32)
    pts[3 * k:4 * k] = ((tri[3 * k:4 * k, 1] + tri[3 * k:4 * k, 2]) * F32(0.5)).astype(F32)
    pts[4 * k:5 * k] = ((tri[4 * k:5 * k, 0] + tri[4 * k:5 * k, 1] + tri[4 * k:5 * k, 2]) / F32(3)).astype(F32)
    pts[5 * k:6 * k] = tri[5 * k:6 * k, 1]
    q, d2 = MO.closest(pts, tri[:, 0], tri[:, 1], tri[:, 2])
    assert q.dtype == np.float32 and d2.dtype == np.float32 and np.isfinite(q).all()
    worst_q = worst_d = 0.0
    for i in range(n):
        eq, ed2 = MO.closest_fp64(pts[i], tri[i, 0], tri[i, 1], tri[i, 2])
        worst_q = max(worst_q, float(np.linalg.norm(q[i].astype(np.float64) - eq)))
        worst_d = max(worst_d, abs(float(np.sqrt(np.float64(d2[i]))) - float(np.sqrt(ed2))))
    print(f"closest point: worst |q32 - q64| = {worst_q:.3e}, worst | |e|32 - |e|64 | = {worst_d:.3e}, bound {Q_BOUND:.3e}")
    assert worst_q <= Q_BOUND and worst_d <= Q_BOUND
    # exact placements: a vertex is returned bit for bit with d2 = 0; a point on the triangle is at most the bound away
    assert np.array_equal(q[0:k], tri[0:k, 0]) and np.array_equal(q[k:2 * k], tri[k:2 * k, 2]) and (d2[0:2 * k] == 0).all()
    assert np.array_equal(q[5 * k:6 * k], tri[5 * k:6 * k, 1]) and (d2[5 * k:6 * k] == 0).all()
    assert np.sqrt(d2[2 * k:5 * k].astype(np.float64)).max() <= Q_BOUND


def test_oracle_regions_and_ties():
    a, b, c = np.array([0, 0, 0], F32), np.array([4, 0, 0], F32), np.array([0, 4, 0], F32)
    cases = [([-1, -1, 2], [0, 0, 0]), ([6, -1, 0], [4, 0, 0]), ([-1, 7, 1], [0, 4, 0]), ([2, -3, 1], [2, 0, 0]), ([-2, 1, 0], [0, 1, 0]),
             ([3, 3, 5], [2, 2, 0]), ([1, 1, -2], [1, 1, 0])]
    for u, exp in cases:
        q, d2 = MO.closest(np.array(u, F32), a, b, c)
        assert np.array_equal(q, np.array(exp, F32)), (u, q)
        assert d2 == F32(((np.array(u, np.float64) - exp) ** 2).sum())
    q, d2 = MO.closest(np.array([np.nan, 0, 0], F32), a, b, c)
    assert np.isnan(d2) and np.isnan(q).any()
    # two triangles sharing the edge (4,0,0)-(0,4,0): a point above the edge's midpoint ties exactly; the lower index wins
    tri = np.array([[a, b, c], [b, np.array([4, 4, 0], F32), c]], F32)
    scan = np.array([[[2, 2, 3], [3, 3, 1], [0.5, 0.5, 1]]], F32)
    idx, d2, q = MO.correspond(scan, np.zeros((1, 3), np.int32), np.concatenate([tri[1:], tri[:1], tri[1:]]), np.array([0, 3]), 1,
                               np.eye(4, dtype=F32)[None])
    assert idx.tolist() == [[0, 0, 1]] and d2.tolist() == [[9.0, 1.0, 1.0]] and q[0, 0].tolist() == [2, 2, 0]


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's loop: what a mesh reference is for
# ---------------------------------------------------------------------------------------------------------------------
PLANE_ANG, PLANE_DT, PLANE_RMSE = 2.1e-8, 3.9e-7, 5.3e-6           # ten times the figures measured below
POINT_ANG, POINT_DT = 5.5e-7, 3.9e-4


def test_oracle_loop_mesh_beats_sampled_reference():
    v, f, p = MO.aircraft_mesh(0)
    tri, seg, _, nrm, _ = MO.group_mesh(v, f, p, NM)
    scan, slab = MO.mesh_scan(v, f, p, 6000, PO.TRUE_POSE, noise=0.0, seed=1)
    start = PO.START_POSE[None]
    # today's path: 3,000 points sampled from the same surface, point to point
    rx, rp, _ = MO.sample_surface(v, f, p, 3000, seed=7)
    g, gseg, _ = IO.group_reference(rx.astype(F32), rp, NM)
    # both point-to-point runs go to convergence at the default tolerances (the mesh one slides along the surfaces and needs about
    # 150 iterations), so the comparison is between what each reference reaches, not between two truncations
    spose, _, _, siters, sstatus = IO.icp(scan[None], slab[None], g, gseg, NM, start, max_iters=200)
    sang, sdt = IO.pose_error(spose[0], PO.TRUE_POSE)
    pl = MO.icp(scan[None], slab[None], tri, seg, NM, nrm, start, metric="plane", max_iters=30)
    ang, dt = IO.pose_error(pl[0][0], PO.TRUE_POSE)
    pt = MO.icp(scan[None], slab[None], tri, seg, NM, nrm, start, metric="point", max_iters=200)
    pang, pdt = IO.pose_error(pt[0][0], PO.TRUE_POSE)
    print(f"sampled reference: {int(siters[0])} iterations, {sang:.3e} rad, {sdt:.3e} m; mesh plane: {int(pl[3][0])} iterations, "
          f"{ang:.3e} rad, {dt:.3e} m, rmse {pl[1][0]:.3e}; mesh point: {int(pt[3][0])} iterations, {pang:.3e} rad, {pdt:.3e} m")
    assert pl[4][0] == MO.CONVERGED and pl[3][0] <= 15 and pl[2][0] == 6000
    assert sstatus[0] == MO.CONVERGED and pt[4][0] == MO.CONVERGED
    assert sdt > 1e-3                                            # the sampled reference leaves a bias of its spacing
    assert dt * 10 <= sdt and pdt * 10 <= sdt
    # ten times the oracle's own measured error (fp32 search, scan about 30 m from the sensor, this scene): measured plane 2.1e-9 rad,
    # 3.9e-8 m, rmse 5.3e-7 m after 6 iterations; point 5.5e-8 rad, 3.9e-5 m after 155; the sampled reference 1.1e-3 rad, 1.0e-2 m
    assert ang <= PLANE_ANG and dt <= PLANE_DT and pl[1][0] <= PLANE_RMSE
    assert pang <= POINT_ANG and pdt <= POINT_DT

