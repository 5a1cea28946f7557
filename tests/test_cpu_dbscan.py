"""pn_dbscan / ops.dbscan / the ``cluster_density`` keyword without a GPU: the declared surface, the workspace size, the argument checks
(they run before any HIP call), and the NumPy oracle's facts (tests/dbscan_oracle.py) on the fixtures the GPU tests run: the bridge
scene that voxel connected components merge and DBSCAN separates, the unit lattice, the border tie."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import cluster_oracle as CO
import dbscan_oracle as DO
import neighbors_oracle as NO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INVALID = -1          # PN_ERR_INVALID_ARGUMENT


# ---- the library on the CPU -----------------------------------------------------------------------------------------
def test_surface_is_declared_exported_and_bound():
    from pointcloudprocessing_amd import _lib, ops
    from pointcloudprocessing_amd.pointnet.PointNet import PointNet
    hdr = open(os.path.join(ROOT, "include", "pointnet_hip.h")).read()
    for decl in ("size_t pn_dbscan_workspace_bytes(int N);",
                 "int pn_dbscan(const float* xyz, int N, float eps, int min_points, const float* origin3_host, int32_t* cluster_out,"):
        assert decl in hdr
    assert "#define PN_ABI_VERSION 6" in hdr and _lib.lib().pn_abi_version() == 6 == _lib.ABI_VERSION      # additive: the version stays
    for name in ("pn_dbscan_workspace_bytes", "pn_dbscan"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert len(_lib.SIGNATURES["pn_dbscan"][1]) == 12
    par = inspect.signature(ops.dbscan).parameters
    assert list(par) == ["xyz", "eps", "min_points", "origin", "return_core"]
    assert (par["origin"].default, par["return_core"].default) == (None, False)
    for fn in (PointNet.predict_scan, PointNet.predict_pose):
        par = inspect.signature(fn).parameters
        assert par["cluster_density"].default is None and par["cluster_leaf"].default == 1.0 and par["isolate"].default is None
    assert all(("pn_dbscan", code) in ops._GRID_ERRORS for code in (1, 3))


def _call(xyz=0x1000, N=8, eps=1.0, min_points=4, origin=(0.0, 0.0, 0.0), cluster=0x1000, core=0x1000, sizes=0x1000, nout=0x1000, ws=0x1000,
          ws_bytes=None):
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    p = lambda a: C.c_void_p(a) if a else None      # noqa: E731  (never dereferenced: the checks run before any HIP call)
    if ws_bytes == "knn":                            # a workspace that would do for pn_radius_knn is too small for pn_dbscan
        ws_bytes = L.pn_radius_knn_workspace_bytes(N)
    elif ws_bytes is None:
        ws_bytes = L.pn_dbscan_workspace_bytes(N)
    rc = L.pn_dbscan(p(xyz), N, eps, min_points, (C.c_float * 3)(*origin) if origin else None, p(cluster), p(core), p(sizes), p(nout), p(ws),
                     ws_bytes, None)
    return rc, L.pn_last_error()


@pytest.mark.parametrize("kw,msg", [
    (dict(xyz=0), b"null pointer"), (dict(origin=None), b"null pointer"), (dict(cluster=0), b"null pointer"), (dict(sizes=0), b"null pointer"),
    (dict(nout=0), b"null pointer"),
    (dict(N=0, ws_bytes=1 << 20), b"N must be"), (dict(N=-3, ws_bytes=1 << 20), b"N must be"), (dict(N=(1 << 30) + 1, ws_bytes=1 << 20), b"N must be"),
    (dict(eps=0.0), b"radius"), (dict(eps=-1.0), b"radius"), (dict(eps=float("nan")), b"radius"), (dict(eps=float("inf")), b"radius"),
    (dict(eps=1e20), b"radius * radius"), (dict(eps=1e-30), b"radius * radius"), (dict(eps=3.4e38), b"radius * radius"),
    (dict(min_points=0), b"min_points=0 "), (dict(min_points=-1), b"min_points=-1 "), (dict(min_points=(1 << 30) + 1), b"min_points=1073741825 "),
    (dict(origin=(0.0, float("nan"), 0.0)), b"origin"), (dict(origin=(float("inf"), 0.0, 0.0)), b"origin"),
    (dict(ws=0), b"workspace"), (dict(ws_bytes=1024), b"workspace too small"), (dict(ws_bytes="knn"), b"workspace too small"),
    (dict(ws=0x1008), b"16-byte aligned"),
])
def test_argument_checks_without_gpu(kw, msg):
    rc, err = _call(**kw)
    assert rc == INVALID and msg in err and err.startswith(b"pn_dbscan"), err


def test_workspace_size_is_monotone_and_holds_the_search():
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    ns = (1, 2, 255, 256, 257, 4096, 100000, (1 << 18) - 1, 1 << 18, (1 << 18) + 1, 1 << 20, 1 << 30)
    sizes = [L.pn_dbscan_workspace_bytes(n) for n in ns]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
    # behind the search's tables: a byte (core) and five int32 (parent, root, lowest row, the row's root, id) per point
    assert all(s >= L.pn_radius_knn_workspace_bytes(n) + 21 * n for s, n in zip(sizes, ns))
    for bad in (0, -1, (1 << 30) + 1):
        assert L.pn_dbscan_workspace_bytes(bad) == 0


def test_ops_and_keyword_refusals_touch_no_device():
    import torch
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd._lib import PointNetHipError
    from pointcloudprocessing_amd.pointnet.PointNet import PointNet
    with pytest.raises(PointNetHipError):
        ops.dbscan(torch.zeros(4, 3), 1.0, 4)                               # a CPU tensor
    x = torch.zeros(4, 3)
    m = object.__new__(PointNet)                                            # (the keyword is checked before the model or the scan is looked at)
    good = dict(eps=1.0, min_points=4)
    for fn, extra in ((m.predict_scan, ()), (m.predict_pose, (None,))):
        for cd in (dict(eps=1.0), dict(min_points=4), dict(eps=1.0, min_points=4, leaf=1.0), dict(), (1.0, 4), "dbscan"):
            with pytest.raises(PointNetHipError, match="cluster_density must be"):
                fn(x, *extra, isolate="largest", cluster_density=cd)
        with pytest.raises(PointNetHipError, match="cluster_density goes with isolate"):
            fn(x, *extra, cluster_density=good)
        with pytest.raises(PointNetHipError, match="cluster_density goes with isolate"):
            fn(x, *extra, isolate=None, denoise=dict(method="radius", radius=1.0, min_neighbors=2), cluster_density=good)
        with pytest.raises(PointNetHipError, match="isolate must be"):
            fn(x, *extra, isolate="biggest", cluster_density=good)


# ---- the oracle's facts on the fixtures -----------------------------------------------------------------------------
def test_bridge_scene_dbscan_separates_what_voxel_components_merge():
    scene, air, blob, bridge, clean = DO.bridge_scene()
    assert scene.shape == (4715, 3) and scene.dtype == F32 and (len(air), len(blob), len(bridge)) == (4096, 600, 19)
    assert np.array_equal(scene[air], clean) and bridge[:5].tolist() == [0, 1, 2, 3, 4] and bridge[-1] == 4714
    cl, _, sz, V, K = CO.voxel_clusters(scene, 1.0, scene.min(0), 26)
    assert K == 1 and sz.tolist() == [4715]                                 # the string of single returns joins the two bodies
    cluster, sizes, core, count = DO.bridge_expected()
    assert sizes.tolist() == [4098, 604] and int((cluster == -1).sum()) == 13
    assert (cluster[air] == 0).all() and (cluster[blob] == 1).all()
    assert cluster[bridge].tolist() == [0] * 2 + [-1] * 13 + [1] * 4        # the bridge points next to a body belong to it, the rest is noise
    assert np.array_equal(count, NO.radius_knn(scene, DO.BRIDGE_EPS, 0)[2])


def test_unit_lattice_facts():
    x = DO.unit_lattice()
    cluster, sizes, core, count = DO.dbscan(x, 1.0, 7)                      # core = an interior point: six neighbours and itself
    border = ~core & (cluster >= 0)
    assert (int(core.sum()), int(border.sum()), int((cluster == -1).sum()), sizes.tolist()) == (64, 96, 56, [160])
    inner = ((x >= 1) & (x <= 4)).all(1)
    assert np.array_equal(core, inner) and np.array_equal(cluster == -1, ((x == 0) | (x == 5)).sum(1) >= 2)
    cluster, sizes, core, _ = DO.dbscan(x, DO.below_one(), 1)               # one ulp below the spacing: nobody has a neighbour
    assert len(sizes) == 216 and np.array_equal(cluster, np.arange(216)) and core.all()


@pytest.mark.parametrize("order", sorted(DO.TIE_ORDERS))
def test_border_tie_follows_the_core_of_lower_row(order):
    x, exp_cluster, exp_sizes = DO.border_tie(order)
    cluster, sizes, core, count = DO.dbscan(x, 1.0, 4)
    assert exp_cluster.tolist() == [0, 0, 0, 0, 1, 1, 1] and exp_sizes.tolist() == [4, 3]
    assert np.array_equal(cluster, exp_cluster) and np.array_equal(sizes, exp_sizes)
    assert core.sum() == 2 and np.array_equal(np.abs(x[core, 0]), [1, 1]) and count[(x == 0).all(1)].tolist() == [2]


def test_min_points_one_has_no_noise_and_no_border():
    cases = [(DO.bridge_scene()[0], DO.BRIDGE_EPS), (DO.unit_lattice(), 1.0), (DO.border_tie("mid_first")[0], 1.0),
             (DO.adversarial_cloud()[0], DO.adversarial_cloud()[1])]
    for x, eps in cases:
        cluster, sizes, core, _ = DO.dbscan(x, eps, 1)
        assert core.all() and (cluster >= 0).all() and sizes.sum() == len(x)


def test_ids_do_not_depend_on_geometry_order_only_on_rows():
    """a permutation of the rows permutes the result and renumbers the clusters by their lowest core row"""
    x = NO.surface_cloud(1500, seed=8)
    a = DO.dbscan(x, 0.4, 6)
    perm = np.random.default_rng(1).permutation(len(x))
    b = DO.dbscan(x[perm], 0.4, 6)
    assert len(a[1]) > 5 and (a[0] == -1).any() and (~a[2] & (a[0] >= 0)).any()
    assert np.array_equal(a[2][perm], b[2]) and np.array_equal(a[0][perm] == -1, b[0] == -1)
    assert CO.same_partition(a[0][perm], b[0]) and sorted(a[1].tolist()) == sorted(b[1].tolist())
    first = [int(np.flatnonzero((b[0] == c) & b[2])[0]) for c in range(len(b[1]))]
    assert first == sorted(first)


def test_scikit_learn_agrees_on_the_bridge_scene():
    sk = pytest.importorskip("sklearn.cluster")
    scene = DO.bridge_scene()[0]
    cluster, sizes, core, _ = DO.bridge_expected()
    ref = sk.DBSCAN(eps=DO.BRIDGE_EPS, min_samples=DO.BRIDGE_MIN_POINTS, algorithm="brute").fit(scene.astype(np.float64))
    ref_core = np.zeros(len(scene), bool)
    ref_core[ref.core_sample_indices_] = True
    assert np.array_equal(ref_core, core) and np.array_equal(ref.labels_ == -1, cluster == -1)
    assert CO.same_partition(ref.labels_[core], cluster[core])             # a border point between two clusters is the library's own rule
