"""pn_scan_normals / ops.estimate_normals / ops.incidence_mask / ops.outlier_mask(method="incidence") without a GPU: the declared
surface, the argument checks (they run before any HIP call), the NumPy oracle's facts on exact inputs (tests/normals_oracle.py), the
incidence rule on CPU tensors, and the veil scene: the mixed pixels that the radius filter keeps and the incidence filter drops."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import neighbors_oracle as NO
import normals_oracle as NN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INVALID = -1          # PN_ERR_INVALID_ARGUMENT


# ---- the library on the CPU -----------------------------------------------------------------------------------------
def test_surface_is_declared_exported_and_bound():
    from pointcloudprocessing_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "pointnet_hip.h")).read()
    for decl in ("size_t pn_scan_normals_workspace_bytes(int N);", "int pn_scan_normals(const float* xyz, int N, float radius, "
                 "const float* origin3_host, int k,"):
        assert decl in hdr
    assert "#define PN_ABI_VERSION 6" in hdr and _lib.lib().pn_abi_version() == 6 == _lib.ABI_VERSION
    for name in ("pn_scan_normals_workspace_bytes", "pn_scan_normals"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert len(_lib.SIGNATURES["pn_scan_normals"][1]) == 13
    assert (_lib.PN_SCAN_NORMALS_MIN_K, _lib.PN_RADIUS_KNN_MAX_K) == (NN.MIN_K, NN.MAX_K) == (2, 16)
    assert callable(ops.estimate_normals) and callable(ops.incidence_mask)
    par = inspect.signature(ops.estimate_normals).parameters
    assert list(par) == ["xyz", "radius", "k", "viewpoint", "origin", "return_neighbors"]
    assert (par["k"].default, par["viewpoint"].default, par["origin"].default, par["return_neighbors"].default) == (8, None, None, False)
    par = inspect.signature(ops.outlier_mask).parameters
    assert list(par)[-2:] == ["viewpoint", "max_angle_deg"] and list(par)[:7] == ["xyz", "method", "radius", "k", "min_neighbors", "std_ratio",
                                                                                   "origin"]
    assert tuple(par["viewpoint"].default) == (0, 0, 0) and par["max_angle_deg"].default == 75.0


def _call(xyz=0x1000, N=8, radius=1.0, origin=(0.0, 0.0, 0.0), k=4, viewpoint=None, nrm=0x1000, curv=0x1000, count=0x1000, idx=0x1000,
          ws=0x1000, ws_bytes=None):
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    p = lambda a: C.c_void_p(a) if a else None      # noqa: E731  (never dereferenced: the checks run before any HIP call)
    f3 = lambda v: (C.c_float * 3)(*v) if v else None      # noqa: E731
    if ws_bytes is None:
        ws_bytes = L.pn_scan_normals_workspace_bytes(N)
    rc = L.pn_scan_normals(p(xyz), N, radius, f3(origin), k, f3(viewpoint), p(nrm), p(curv), p(count), p(idx), p(ws), ws_bytes, None)
    return rc, L.pn_last_error()


@pytest.mark.parametrize("kw,msg", [
    (dict(xyz=0), b"null pointer"), (dict(origin=None), b"null pointer"), (dict(nrm=0), b"null pointer"),
    (dict(N=0, ws_bytes=1 << 20), b"N must be"), (dict(N=-3, ws_bytes=1 << 20), b"N must be"), (dict(N=(1 << 30) + 1, ws_bytes=1 << 20), b"N must be"),
    (dict(radius=0.0), b"radius"), (dict(radius=-1.0), b"radius"), (dict(radius=float("nan")), b"radius"), (dict(radius=float("inf")), b"radius"),
    (dict(radius=1e20), b"radius * radius"), (dict(radius=1e-30), b"radius * radius"), (dict(radius=3.4e38), b"radius * radius"),
    (dict(k=1), b"k=1 "), (dict(k=17), b"k=17"), (dict(k=0), b"k=0"), (dict(k=-1), b"k=-1"),
    (dict(origin=(0.0, float("nan"), 0.0)), b"origin"), (dict(origin=(float("inf"), 0.0, 0.0)), b"origin"),
    (dict(viewpoint=(0.0, float("nan"), 0.0)), b"viewpoint"), (dict(viewpoint=(0.0, 0.0, float("-inf"))), b"viewpoint"),
    (dict(ws=0), b"workspace"), (dict(ws_bytes=1024), b"workspace too small"), (dict(ws=0x1008), b"16-byte aligned"),
])
def test_argument_checks_without_gpu(kw, msg):
    rc, err = _call(**kw)
    assert rc == INVALID and msg in err and err.startswith(b"pn_scan_normals"), err


def test_workspace_size_is_monotone_and_holds_the_search():
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    ns = (1, 2, 255, 256, 257, 4096, 100000, 262144, 262145, 1 << 20)
    sizes = [L.pn_scan_normals_workspace_bytes(n) for n in ns]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
    assert all(s >= L.pn_radius_knn_workspace_bytes(n) for s, n in zip(sizes, ns))
    assert L.pn_scan_normals_workspace_bytes(0) == 0 and L.pn_scan_normals_workspace_bytes(-1) == 0


def test_ops_wrappers_refuse_cpu_tensors_and_bad_keywords():
    import torch
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd._lib import PointNetHipError
    with pytest.raises(PointNetHipError):
        ops.estimate_normals(torch.zeros(4, 3), 1.0)
    with pytest.raises(PointNetHipError):
        ops.outlier_mask(torch.zeros(4, 3), "incidence", 1.0)
    with pytest.raises(PointNetHipError, match="'radius', 'statistical' or 'incidence'"):
        ops.outlier_mask(torch.zeros(4, 3), "median", 1.0)


# ---- oracle facts on exact inputs -----------------------------------------------------------------------------------
def test_cellwise_search_is_the_brute_force_bit_for_bit():
    x = np.concatenate([NO.surface_cloud(1500, seed=3), NO.lattice(6, seed=1)[0] * F32(0.25)])       # ties in distance included
    for radius, k in ((0.3, 5), (0.5, 16)):
        a, b = NN.radius_knn(x, radius, k), NO.radius_knn(x, radius, k)
        assert all(np.array_equal(u.view(np.int32), v.view(np.int32)) for u, v in zip(a, b)) and a[2].max() > k


def test_lattice_plane_normals_are_exact():
    x = NN.lattice_plane()
    for vp, sign in NN.LATTICE_PLANE_VIEWS:
        n, cu, count, idx = NN.normals(x, 1.5, 8, vp)
        assert (count >= 3).all() and np.array_equal(n, np.tile(np.array([0, 0, sign], F32), (len(x), 1)))
        assert (cu == 0).all()
    # k = 2 at radius 1: a corner has exactly two neighbours and the three points span the plane; elsewhere the two lowest rows among
    # the ties at d = 1 may lie on one line with the point, which is the collinear case
    n, cu, count, idx = NN.normals(x, 1.0, 2)
    fin = np.isfinite(n).all(1)
    corner = np.isin(x[:, 0], (0, 8)) & np.isin(x[:, 1], (0, 8))
    assert count.min() == 2 and corner.sum() == 4 and fin[corner].all() and np.array_equal(n[fin], np.tile(np.array([0, 0, 1], F32), (fin.sum(), 1)))
    line = np.array([(x[i] + x[i] == x[idx[i, 0]] + x[idx[i, 1]]).all() for i in range(len(x))])
    assert np.array_equal(~fin, line) and line.any()


def test_degenerate_neighbourhoods_are_nan():
    line = (np.arange(7)[:, None] * [1.0, 2.0, 3.0]).astype(F32)
    n, cu, count, _ = NN.normals(line, 8.0, 4)
    assert np.isnan(n).all() and np.isnan(cu).all() and (count >= 2).all()
    same = np.ones((5, 3), F32)
    n, cu, count, _ = NN.normals(same, 1.0, 4)
    assert np.isnan(n).all() and np.isnan(cu).all() and (count == 4).all()
    pair = np.array([[0, 0, 0], [0.5, 0, 0], [50, 50, 50]], F32)
    n, cu, count, idx = NN.normals(pair, 1.0, 3)
    assert np.isnan(n).all() and count.tolist() == [1, 1, 0] and idx[:, 0].tolist() == [1, 0, -1]
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F32)
    n, cu, count, _ = NN.normals(tri, 2.0, 2)
    assert np.array_equal(n, np.tile(np.array([0, 0, 1], F32), (3, 1))) and (cu == 0).all() and count.tolist() == [2, 2, 2]


# ---- ops.incidence_mask on CPU tensors ------------------------------------------------------------------------------
@pytest.mark.parametrize("angle", [15.0, 60.0, 75.0, 89.5])
def test_incidence_mask_matches_the_oracle_bit_for_bit(angle):
    import torch
    from pointcloudprocessing_amd import ops
    rng = np.random.default_rng(int(angle))
    x = rng.uniform(-5, 5, (4000, 3)).astype(F32)
    n = rng.normal(size=(4000, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F32)
    vp = (0.25, -1.0, 3.0)
    n[5] = np.nan
    n[6, 1] = np.inf
    x[7] = vp                                                             # v = 0: dropped
    x[8] = np.nan
    want = NN.incidence_mask(x, n, vp, angle)
    got = ops.incidence_mask(torch.from_numpy(x), torch.from_numpy(n), vp, angle)
    assert got.dtype == torch.bool and np.array_equal(got.numpy(), want)
    assert not want[5:9].any() and 0.02 * len(x) < want.sum() < len(x) - 20
    # the rule is the angle between the normal's line and the ray
    v = np.asarray(vp) - x.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        cosang = np.abs((n.astype(np.float64) * v).sum(1)) / np.linalg.norm(v, axis=1)
        clear = np.abs(cosang - np.cos(np.radians(angle))) > 1e-9
    clear[5:9] = False
    assert np.array_equal(want[clear], cosang[clear] >= np.cos(np.radians(angle)))
    assert np.array_equal(ops.incidence_mask(torch.from_numpy(x), torch.from_numpy(-n), vp, angle).numpy(), want)      # the sign does not matter


def test_incidence_mask_refuses_bad_angles_and_shapes():
    import torch
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd._lib import PointNetHipError
    x = torch.zeros(4, 3)
    for bad in (0.0, 90.0, -5.0, 120.0, float("nan")):
        with pytest.raises(PointNetHipError, match="max_angle_deg"):
            ops.incidence_mask(x, x, (0, 0, 0), bad)
    with pytest.raises(PointNetHipError):
        ops.incidence_mask(x, torch.zeros(3, 3), (0, 0, 0), 75.0)
    with pytest.raises(PointNetHipError):
        ops.incidence_mask(x, x, (0, 0), 75.0)


# ---- the veil scene -------------------------------------------------------------------------------------------------
def test_veil_scene_incidence_drops_the_veil_that_radius_keeps():
    """measured with the oracle: 312 veil points of 22,500; incidence keeps 3.5 % of the veil and 100 % of plate and wall, the nearest
    decision is 5.9e-3 from the threshold; the radius filter (0.6, 8) keeps 88.1 % of the veil"""
    xyz, kind, keep, margin, count = (NN.veil_case()[name] for name in ("xyz", "kind", "keep", "margin", "count"))
    assert NN.VEIL_SETTINGS == dict(radius=0.6, k=8, max_angle_deg=75.0)
    veil, surf = kind == NN.VEIL, kind != NN.VEIL
    assert xyz.shape == (22500, 3) and veil.sum() == 312 and (kind == NN.PLATE).sum() > 5000 and (kind == NN.WALL).sum() > 15000
    print("veil kept", keep[veil].mean(), "plate kept", keep[kind == NN.PLATE].mean(), "wall kept", keep[kind == NN.WALL].mean(),
          "min margin", margin.min(), "radius keeps veil", (count[veil] >= 8).mean())
    assert keep[veil].mean() <= 0.10
    assert keep[kind == NN.PLATE].mean() >= 0.99 and keep[kind == NN.WALL].mean() >= 0.99
    assert margin.min() > 1e-5
    assert (count[veil] >= 8).mean() > 0.5 and (count[surf] >= 8).all()
