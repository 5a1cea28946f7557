"""pn_radius_knn / ops.radius_knn / ops.neighbor_stat_mask / ops.outlier_mask without a GPU: the containment rule the grid search rests
on (checked with the library's own leaf on adversarial pairs), the NumPy oracle's facts (tests/neighbors_oracle.py), the declared
surface, the argument checks (they run before any HIP call) and the statistical mask on CPU tensors."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import neighbors_oracle as NO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INVALID = -1          # PN_ERR_INVALID_ARGUMENT


def _leaf(radius):
    from pointcloudprocessing_amd import _lib
    return F32(_lib.lib().pn_radius_knn_leaf(float(F32(radius))))


# ---- the containment rule -------------------------------------------------------------------------------------------
RADII = [1e-2, 0.0371, 0.5, 1.0, float(np.sqrt(F32(2))), 1.5, 3.3, 10.0]


def test_leaf_is_the_stated_one_above_the_radius_and_monotone():
    rs = np.sort(np.concatenate([np.asarray(RADII, F32), np.random.default_rng(0).uniform(1e-2, 10.0, 500).astype(F32),
                                 [NO.ulp_steps(1.0, n) for n in range(-4, 5)]]).astype(F32))
    hs = np.array([_leaf(r) for r in rs], F32)
    assert (hs >= rs).all() and (np.diff(hs) >= 0).all()
    for r, h in zip(rs, hs):
        assert h == NO.leaf(r) and np.float64(h) >= np.float64(r) * (1.0 + 2.0 ** -6) > np.float64(np.nextafter(h, F32(0)))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert _leaf(bad) == 0


@pytest.mark.parametrize("origin", [(0.0, 0.0, 0.0), (-1000.0, 1000.0, -999.5), (1000.0, -1000.0, 0.37)])
@pytest.mark.parametrize("radius", RADII)
def test_containment_on_adversarial_pairs(radius, origin):
    """every pair with computed d <= r2 and both keys in [0, MAX_KEY) has keys differing by at most 1 on every axis"""
    r = F32(radius)
    h = _leaf(r)
    r2 = r * r
    a, b = NO.adversarial_pairs(r, origin, NO.MAX_KEY - 1, seed=int(radius * 1000) % 97)
    ka, kb = NO.keys(a, h, origin), NO.keys(b, h, origin)
    valid = ((ka >= 0) & (ka < NO.MAX_KEY) & (kb >= 0) & (kb < NO.MAX_KEY)).all(1)
    dx, dy, dz = (a[:, i] - b[:, i] for i in range(3))
    d = (dx * dx + dy * dy) + dz * dz
    inside = valid & (d <= r2)
    # the fixture is adversarial: pairs inside and outside the radius, in different voxels, at the top keys
    assert inside.sum() > 1000 and (valid & ~(d <= r2)).sum() > 1000
    assert (np.abs(ka - kb).max(1)[inside] == 1).sum() > 500 and (ka[inside].max(1) == NO.MAX_KEY - 1).sum() > 5
    assert np.abs(ka - kb)[inside].max() <= 1


# ---- oracle facts ---------------------------------------------------------------------------------------------------
def test_lattice_facts():
    x, c = NO.lattice(6, seed=3)
    idx, d2, count = NO.radius_knn(x, 1.0, 4)
    on_edge = ((c == 0) | (c == 5)).sum(1)
    interior = np.flatnonzero(on_edge == 0)
    assert (count[interior] == 6).all() and (count == 6 - on_edge).all()          # d = 1 <= r2 = 1: "<=" applies
    assert (d2[interior] == 1).all()
    for i in interior:
        six = np.flatnonzero(np.abs(c - c[i]).sum(1) == 1)
        assert len(six) == 6 and idx[i].tolist() == sorted(six.tolist())[:4]        # ties at d = 1: the four lowest rows
    count15 = NO.radius_knn(x, 1.5, 0)[2]
    assert (count15[interior] == 18).all()                                           # 6 at d = 1 and 12 at d = 2 <= 2.25
    corner = np.flatnonzero(on_edge == 3)
    assert len(corner) == 8 and (count15[corner] == 6).all() and (NO.radius_knn(x, 1.0, 0)[2][corner] == 3).all()
    assert NO.radius_knn(x, 1.5, 0)[0].shape == (216, 0)


def test_oracle_edge_cases():
    one = NO.radius_knn(np.zeros((1, 3), F32), 1.0, 3)
    assert one[0].tolist() == [[-1] * 3] and np.isinf(one[1]).all() and one[2].tolist() == [0]
    two = NO.radius_knn(np.ones((2, 3), F32), 0.5, 2)
    assert two[0].tolist() == [[1, -1], [0, -1]] and two[1][:, 0].tolist() == [0, 0] and two[2].tolist() == [1, 1]
    nan = NO.radius_knn(np.array([[0, 0, 0], [np.nan, 0, 0], [0.1, 0, 0]], F32), 1.0, 2)
    assert nan[2].tolist() == [1, 0, 1] and nan[0].tolist() == [[2, -1], [-1, -1], [0, -1]]


# ---- the library on the CPU -----------------------------------------------------------------------------------------
def test_surface_is_declared_and_exported():
    from pointcloudprocessing_amd import _lib, ops
    from pointcloudprocessing_amd.pointnet.PointNet import PointNet
    hdr = open(os.path.join(ROOT, "include", "pointnet_hip.h")).read()
    for decl in ("float pn_radius_knn_leaf(float radius);", "size_t pn_radius_knn_workspace_bytes(int N);", "int pn_radius_knn(",
                 "#define PN_RADIUS_KNN_MAX_KEY (1 << 14)"):
        assert decl in hdr
    assert "#define PN_ABI_VERSION 6" in hdr and _lib.lib().pn_abi_version() == 6 == _lib.ABI_VERSION
    for name in ("pn_radius_knn_leaf", "pn_radius_knn_workspace_bytes", "pn_radius_knn"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert _lib.PN_RADIUS_KNN_MAX_KEY == NO.MAX_KEY == 1 << 14 and _lib.PN_RADIUS_KNN_MAX_K == NO.MAX_K
    assert callable(ops.radius_knn) and callable(ops.neighbor_stat_mask) and callable(ops.outlier_mask)
    par = inspect.signature(ops.outlier_mask).parameters
    assert (par["k"].default, par["min_neighbors"].default, par["std_ratio"].default, par["origin"].default) == (8, 8, 2.0, None)
    for fn in (PointNet.predict_scan, PointNet.predict_pose):
        assert inspect.signature(fn).parameters["denoise"].default is None


def _call(xyz=0x1000, N=8, radius=1.0, origin=(0.0, 0.0, 0.0), k=4, idx=0x1000, d2=0x1000, count=0x1000, ws=0x1000, ws_bytes=None):
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    p = lambda a: C.c_void_p(a) if a else None      # noqa: E731  (never dereferenced: the checks run before any HIP call)
    if ws_bytes is None:
        ws_bytes = L.pn_radius_knn_workspace_bytes(N)
    rc = L.pn_radius_knn(p(xyz), N, radius, (C.c_float * 3)(*origin) if origin else None, k, p(idx), p(d2), p(count), p(ws), ws_bytes, None)
    return rc, L.pn_last_error()


@pytest.mark.parametrize("kw,msg", [
    (dict(xyz=0), b"null pointer"), (dict(origin=None), b"null pointer"), (dict(count=0), b"null pointer"),
    (dict(idx=0), b"null pointer"), (dict(d2=0), b"null pointer"),
    (dict(N=0, ws_bytes=1 << 20), b"N must be"), (dict(N=-3, ws_bytes=1 << 20), b"N must be"), (dict(N=(1 << 30) + 1, ws_bytes=1 << 20), b"N must be"),
    (dict(radius=0.0), b"radius"), (dict(radius=-1.0), b"radius"), (dict(radius=float("nan")), b"radius"), (dict(radius=float("inf")), b"radius"),
    (dict(radius=1e20), b"radius * radius"), (dict(radius=1e-30), b"radius * radius"), (dict(radius=3.4e38), b"radius * radius"),
    (dict(k=-1), b"k=-1"), (dict(k=17), b"k=17"),
    (dict(k=0), b"k = 0"), (dict(k=0, idx=0), b"k = 0"), (dict(k=0, d2=0), b"k = 0"),
    (dict(origin=(0.0, float("nan"), 0.0)), b"origin"), (dict(origin=(float("inf"), 0.0, 0.0)), b"origin"),
    (dict(ws=0), b"workspace"), (dict(ws_bytes=1024), b"workspace too small"), (dict(ws=0x1008), b"16-byte aligned"),
])
def test_argument_checks_without_gpu(kw, msg):
    rc, err = _call(**kw)
    assert rc == INVALID and msg in err, err


def test_workspace_size_is_monotone_and_holds_the_sort():
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    sizes = [L.pn_radius_knn_workspace_bytes(n) for n in (1, 2, 255, 256, 257, 4096, 100000, 262144, 262145, 1 << 20)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
    assert all(L.pn_radius_knn_workspace_bytes(n) >= L.pn_voxel_workspace_bytes(n) + 24 * n for n in (1, 4096, 262145))
    assert L.pn_radius_knn_workspace_bytes(0) == 0 and L.pn_radius_knn_workspace_bytes(-1) == 0


def test_ops_wrappers_refuse_cpu_tensors_and_bad_keywords():
    import torch
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd._lib import PointNetHipError
    with pytest.raises(PointNetHipError):
        ops.radius_knn(torch.zeros(4, 3), 1.0, 3)
    with pytest.raises(PointNetHipError):
        ops.outlier_mask(torch.zeros(4, 3), "radius", 1.0)
    with pytest.raises(PointNetHipError):
        ops.outlier_mask(torch.zeros(4, 3), "median", 1.0)
    with pytest.raises(PointNetHipError):
        ops.neighbor_stat_mask(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int32), 4, 2.0)


# ---- neighbor_stat_mask on CPU tensors ------------------------------------------------------------------------------
def _stat_case(kind):
    x = NO.surface_cloud(1500, seed=4)
    x = np.concatenate([x, np.random.default_rng(8).uniform(-3, 13, (60, 3)).astype(F32)])
    k = 6
    idx, d2, count = NO.radius_knn(x, {"all": 30.0, "none": 1e-3, "mixed": 0.45}[kind], k)
    return d2, count, k


@pytest.mark.parametrize("std_ratio", [0.5, 2.0])
@pytest.mark.parametrize("kind", ["all", "none", "mixed"])
def test_neighbor_stat_mask_matches_the_oracle(kind, std_ratio):
    import torch
    from pointcloudprocessing_amd import ops
    d2, count, k = _stat_case(kind)
    keep, m, thr, full = NO.stat_mask(d2, count, k, std_ratio, return_stats=True)
    n_full = int((count >= k).sum())
    assert {"all": n_full == len(count), "none": n_full == 0, "mixed": 100 < n_full < len(count) - 100}[kind]
    if n_full:
        # the oracle itself shows no m_i within 1e-9 relative of the threshold: summation order cannot flip a decision
        assert np.abs(m[full] - thr).min() > 1e-9 * thr and 0 < keep.sum() < n_full
    got = ops.neighbor_stat_mask(torch.from_numpy(d2), torch.from_numpy(count), k, std_ratio)
    assert got.dtype == torch.bool and tuple(got.shape) == (len(count),)
    assert np.array_equal(got.numpy(), keep)
    assert not got.numpy()[count < k].any()
