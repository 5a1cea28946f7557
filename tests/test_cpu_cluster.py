"""pn_voxel_cluster / ops.voxel_clusters / ops.cluster_mask without a GPU: the NumPy oracle's invariants (tests/cluster_oracle.py), the
facts recorded for the specification, the declared surface, and the argument checks (they run before any HIP call)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cluster_oracle as CO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _kc46():
    pts = []
    for line in open(os.path.join(ROOT, "tests", "golden", "kc-46.txt")):
        m = re.match(r"\(([^)]*)\)", line.strip())
        pts.append([float(v) for v in m.group(1).split(",")])
    return np.asarray(pts, F32)


# ---- oracle invariants ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", [6, 26])
def test_partition_invariant_under_permutation(conn):
    rng = np.random.default_rng(3)
    x = (rng.random((1500, 3)) * 25).astype(F32)
    a = CO.voxel_clusters(x, 1.0, (0, 0, 0), conn)
    perm = rng.permutation(len(x))
    b = CO.voxel_clusters(x[perm], 1.0, (0, 0, 0), conn)
    assert a[3:] == b[3:] and a[4] > 1
    assert np.array_equal(a[0][perm], b[0]) and np.array_equal(a[1][perm], b[1])       # ids depend on the voxels only
    assert np.array_equal(a[2], b[2])


def test_close_pairs_share_a_cluster():
    rng = np.random.default_rng(4)
    x = (rng.random((2000, 3)) * 20).astype(F32)
    leaf = F32(0.8)
    cl = CO.voxel_clusters(x, leaf, (0, 0, 0), 26)[0]
    assert len(set(cl.tolist())) > 1
    d = np.abs(x[:, None, :] - x[None, :, :]).max(2)
    i, j = np.nonzero(d < leaf)
    assert len(i) > 2000 and (cl[i] == cl[j]).all()
    # and two points of different clusters differ by more than one leaf on some axis
    far = cl[:, None] != cl[None, :]
    assert (d[far] > leaf).all()


def test_six_refines_twenty_six():
    x = CO.random_grid(6000, 16, seed=2)
    c6 = CO.voxel_clusters(x, 1.0, (0, 0, 0), 6)
    c26 = CO.voxel_clusters(x, 1.0, (0, 0, 0), 26)
    assert np.array_equal(c6[1], c26[1]) and c6[3] == c26[3]
    assert c6[4] > c26[4] and CO.refines(c6[0], c26[0]) and not CO.refines(c26[0], c6[0])
    assert int(c6[2].sum()) == len(x) == int(c26[2].sum())


# ---- recorded facts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf,conn,K", [(2.0, 26, 1), (1.0, 26, 12), (1.0, 6, 67)])
def test_kc46_cluster_counts(leaf, conn, K):
    x = _kc46()
    assert len(x) == 490
    assert CO.voxel_clusters(x, leaf, x.min(0), conn)[4] == K


def test_checkerboard():
    x = CO.checkerboard()
    assert len(x) == 108
    assert CO.voxel_clusters(x, 1.0, x.min(0), 6)[3:] == (108, 108)
    assert CO.voxel_clusters(x, 1.0, x.min(0), 26)[3:] == (108, 1)


def test_wrap_pair_is_two_clusters():
    x = np.array([[0.5, 1.5, 0.5], [2097151.5, 0.5, 0.5]], F32)
    k = CO.voxel_indices(x, 1.0, (0, 0, 0))
    key = (k[:, 2] << 42) | (k[:, 1] << 21) | k[:, 0]
    assert abs(int(key[0]) - int(key[1])) == 1                       # neighbours by key, not by coordinates
    for conn in (6, 26):
        cl, vx, sz, V, K = CO.voxel_clusters(x, 1.0, (0, 0, 0), conn)
        assert (V, K) == (2, 2) and sz.tolist() == [1, 1] and vx.tolist() == [1, 0]
    assert np.array_equal(CO.wrap_pair("x"), x)
    for axis in "xyz":
        assert CO.voxel_clusters(CO.wrap_pair(axis), 1.0, (0, 0, 0), 26)[3:] == (2, 2)


def test_shared_cases_are_what_they_claim():
    s = CO.serpentine()
    cl, vx, sz, V, K = CO.voxel_clusters(s, 1.0, (0, 0, 0), 6)
    assert (V, K) == (4096, 1) and np.abs(np.diff(vx)).min() >= 1 and np.median(np.abs(np.diff(vx))) > 30
    st = CO.staircase()
    assert CO.voxel_clusters(st, 1.0, (0, 0, 0), 26)[3:] == (2000, 1) and CO.voxel_clusters(st, 1.0, (0, 0, 0), 6)[3:] == (2000, 2000)
    for lo in (255, 65535):
        assert CO.voxel_clusters(CO.digit_boundary(lo), 1.0, (0, 0, 0), 6)[3:] == (9, 2)
    g = CO.voxel_clusters(CO.random_grid(), 1.0, (0, 0, 0), 6)
    assert g[3] > 6000 and g[4] > 100 and int(np.bincount(g[1]).max()) > 3


def test_cluttered_scene_facts():
    scene, rows, blob, clean = CO.cluttered_scene()
    assert scene.shape == (4360, 3) and rows[0] == 20 and rows[-1] < 4360 - 24 and np.array_equal(scene[rows], clean)
    cl, _, sz, V, K = CO.voxel_clusters(scene, 1.0, scene.min(0), 26)
    order = np.argsort(-sz, kind="stable")
    assert K == 63 and sz[order[0]] == 4096 and sz[order[1]] == 200
    assert np.array_equal(np.flatnonzero(cl == order[0]), rows) and np.array_equal(np.flatnonzero(cl == order[1]), blob)


# ---- the library on the CPU -----------------------------------------------------------------------------------------
def test_surface_is_declared_and_exported():
    from pointcloudprocessing_amd import _lib, ops
    from pointcloudprocessing_amd.pointnet.PointNet import PointNet
    import inspect
    hdr = open(os.path.join(ROOT, "include", "pointnet_hip.h")).read()
    assert "size_t pn_voxel_cluster_workspace_bytes(int N);" in hdr and "int pn_voxel_cluster(" in hdr
    assert "#define PN_ABI_VERSION 6" in hdr and _lib.lib().pn_abi_version() == 6
    for name in ("pn_voxel_cluster_workspace_bytes", "pn_voxel_cluster"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert callable(ops.voxel_clusters) and callable(ops.cluster_mask)
    for fn in (PointNet.predict_scan, PointNet.predict_pose):
        par = inspect.signature(fn).parameters
        assert par["isolate"].default is None and par["cluster_leaf"].default == 1.0 and par["min_cluster_points"].default == 1


def _call(xyz=0x1000, N=8, leaf=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), conn=26, cluster=0x1000, voxel=0x1000, sizes=0x1000, nout=0x1000,
          ws=0x1000, ws_bytes=None):
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    p = lambda a: C.c_void_p(a) if a else None      # noqa: E731  (never dereferenced: the checks run before any HIP call)
    if ws_bytes is None:
        ws_bytes = L.pn_voxel_cluster_workspace_bytes(N)
    rc = L.pn_voxel_cluster(p(xyz), N, (C.c_float * 3)(*leaf) if leaf else None, (C.c_float * 3)(*origin) if origin else None, conn,
                            p(cluster), p(voxel), p(sizes), p(nout), p(ws), ws_bytes, None)
    return rc, L.pn_last_error()


@pytest.mark.parametrize("kw,msg", [
    (dict(xyz=0), b"null pointer"), (dict(leaf=None), b"null pointer"), (dict(origin=None), b"null pointer"),
    (dict(cluster=0), b"null pointer"), (dict(sizes=0), b"null pointer"), (dict(nout=0), b"null pointer"),
    (dict(N=0, ws_bytes=1 << 20), b"N must be"), (dict(N=-3, ws_bytes=1 << 20), b"N must be"), (dict(N=(1 << 30) + 1, ws_bytes=1 << 20), b"N must be"),
    (dict(leaf=(1.0, 0.0, 1.0)), b"leaf"), (dict(leaf=(1.0, 1.0, -2.0)), b"leaf"), (dict(leaf=(float("nan"), 1.0, 1.0)), b"leaf"),
    (dict(leaf=(1.0, float("inf"), 1.0)), b"leaf"), (dict(origin=(0.0, float("nan"), 0.0)), b"origin"),
    (dict(conn=0), b"connectivity"), (dict(conn=18), b"connectivity"), (dict(conn=27), b"connectivity"),
    (dict(ws=0), b"workspace"), (dict(ws_bytes=1024), b"workspace too small"), (dict(ws=0x1008), b"16-byte aligned"),
])
def test_argument_checks_without_gpu(kw, msg):
    rc, err = _call(**kw)
    assert rc == -1 and msg in err, err


def test_workspace_size_is_monotone_and_holds_the_sort():
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    sizes = [L.pn_voxel_cluster_workspace_bytes(n) for n in (1, 2, 255, 256, 257, 4096, 100000, 262144, 262145, 1 << 20)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    assert sizes[0] > 0 and sizes[-1] > sizes[0]
    assert all(L.pn_voxel_cluster_workspace_bytes(n) > L.pn_voxel_workspace_bytes(n) for n in (1, 4096, 262145))
    assert L.pn_voxel_cluster_workspace_bytes(0) == 0


def test_ops_wrappers_refuse_cpu_tensors_and_bad_keywords():
    import torch
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd._lib import PointNetHipError
    with pytest.raises(PointNetHipError):
        ops.voxel_clusters(torch.zeros(4, 3), 1.0)
    with pytest.raises(PointNetHipError):
        ops.cluster_mask(torch.zeros(4, dtype=torch.int32), torch.ones(1, dtype=torch.int32), keep="biggest")


def test_cluster_mask_by_hand():
    import torch
    from pointcloudprocessing_amd import ops
    cluster = torch.tensor([2, 0, -1, 1, 1, 2, 0, 3, -1, 2, 1], dtype=torch.int32)
    sizes = torch.tensor([2, 3, 3, 1], dtype=torch.int32)                  # clusters 1 and 2 tie: the lowest id wins
    assert ops.cluster_mask(cluster, sizes).tolist() == [c == 1 for c in cluster.tolist()]
    assert ops.cluster_mask(cluster, sizes, keep="largest", min_points=3).tolist() == [c == 1 for c in cluster.tolist()]
    assert not ops.cluster_mask(cluster, sizes, keep="largest", min_points=4).any()
    assert ops.cluster_mask(cluster, sizes, keep="all").tolist() == [c >= 0 for c in cluster.tolist()]
    assert ops.cluster_mask(cluster, sizes, keep="all", min_points=2).tolist() == [c in (0, 1, 2) for c in cluster.tolist()]
    assert ops.cluster_mask(cluster, sizes, keep="all", min_points=3).tolist() == [c in (1, 2) for c in cluster.tolist()]
    m = ops.cluster_mask(cluster, sizes, keep="all", min_points=9)
    assert m.dtype == torch.bool and tuple(m.shape) == (11,) and not m.any()
    none = ops.cluster_mask(torch.full((3,), -1, dtype=torch.int32), torch.empty(0, dtype=torch.int32))
    assert none.tolist() == [False] * 3
