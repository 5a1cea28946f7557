"""Every compile-time list length of the radius search and its consumers on the MI355X, one case per (entry, k): pn_radius_knn
(neighbors_search_kernel<K>, K = 0 .. 16), pn_scan_normals (scan_normals_kernel<K>, 2 .. 16), pn_fpfh (fpfh_spfh_kernel<K> and the
K-strided workspace, 2 .. 16) and pn_icp_normals (icp_normals_kernel<K>, 3 .. 16): 61 instantiations, each with its own unrolled
insertion network, list stride and neighbourhood array.  The inputs are tests/knn_k_cases.py's (tests/test_cpu_knn_k_cases.py shows on
the oracles alone that at every k they hold counts of 0, k - 1, k, k + 1 and far above k, ties across the last slot and insertions
into every slot of a full list) next to the clouds the entries' own test files use; the raw callers with their guard bands,
untouched-input and error-word checks, the comparisons and the tolerances are those files', imported.  Each oracle list is computed
once at k = 16: the k nearest are the first k of the 16 nearest."""
import ctypes as C

import numpy as np
import pytest
import torch

import fpfh_oracle as FO
import icp_plane_oracle as PO
import knn_k_cases as KC
import neighbors_oracle as NO
import normals_oracle as NN
from test_gpu_fpfh import _check_fpfh, _cloud, _raw_fpfh
from test_gpu_icp_plane import GUARD, PAT, _guarded, _normals_cases, _normals_close, _raw_normals, _seg_c, _t
from test_gpu_neighbors import _raw as _raw_knn
from test_gpu_neighbors import _same
from test_gpu_normals import SURFACE_RADIUS, VIEWPOINT, _close, _same_lists
from test_gpu_normals import _check as _check_scan
from test_gpu_normals import _raw as _raw_scan

pytestmark = pytest.mark.gpu
F32 = np.float32
ORIGINS = (KC.ORIGIN, KC.SECOND_ORIGIN)      # the second moves every voxel face: another arrival order, the same answer
INF_BITS = 0x7F800000


def _prefix(knn16, k):
    return knn16[0][:, :k].copy(), knn16[1][:, :k].copy(), knn16[2]


@pytest.fixture(scope="module")
def edge():
    xyz = KC.k_edge_cloud()[0]
    knn16 = NO.radius_knn(xyz, KC.RADIUS, 16)
    assert len(xyz) == 1684 and knn16[2].max() == 26 and np.array_equal(np.unique(knn16[2]), np.r_[0:18, 26])
    return xyz, knn16


# ---- pn_radius_knn ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(0, 17))
def test_radius_knn(dev, edge, k):
    xyz, knn16 = edge
    exp = _prefix(knn16, k)
    unfilled = np.arange(k)[None, :] >= exp[2][:, None]
    assert np.array_equal(exp[0] == -1, unfilled) and np.array_equal(np.isposinf(exp[1]), unfilled)
    xt = torch.from_numpy(xyz).to(dev)
    for origin in ORIGINS:
        got = _raw_knn(xt, KC.RADIUS, k, origin)                          # k = 0: NULL lists
        _same(got, exp)
        assert (got[0][unfilled] == -1).all() and (got[1][unfilled] == INF_BITS).all()      # unfilled slots: (-1, +inf)
        assert (got[0][~unfilled] >= 0).all() and (got[1][~unfilled] < INF_BITS).all()


# ---- pn_scan_normals --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(2, 17))
def test_scan_normals_lists(dev, edge, k):
    """idx and count only: the lattice's neighbourhoods are isotropic, their eigenvectors are nobody's to claim"""
    xyz, knn16 = edge
    xt = torch.from_numpy(xyz).to(dev)
    for origin in ORIGINS:
        _same_lists(_raw_scan(xt, KC.RADIUS, k, origin), _prefix(knn16, k))


@pytest.fixture(scope="module")
def surface():
    x = NO.surface_cloud()
    knn16 = NN.radius_knn(x, SURFACE_RADIUS, 16)
    assert 9 < knn16[2].mean() < 11 and knn16[2].max() > 16 and (knn16[2] < 2).any()
    return x, knn16


@pytest.mark.parametrize("k", range(2, 17))
def test_scan_normals_surface_cloud(dev, surface, k):
    """tests/test_gpu_normals.py's test_surface_cloud and test_surface_cloud_with_a_viewpoint, at every k"""
    x, knn16 = surface
    got, exp = _check_scan(x, SURFACE_RADIUS, k, knn=_prefix(knn16, k))
    fin = np.isfinite(exp[0]).all(1)
    assert 0.99 < fin.mean() < 1 and (got["curv"][fin] >= -1e-6).all() and (got["curv"][fin] <= 1 / 3 + 1e-6).all()
    assert np.abs(np.linalg.norm(got["nrm"][fin].astype(np.float64), axis=1) - 1).max() < 1e-6
    seen, facing = _check_scan(x, SURFACE_RADIUS, k, viewpoint=VIEWPOINT, knn=_prefix(knn16, k))
    v = np.asarray(VIEWPOINT) - x[fin].astype(np.float64)
    assert np.array_equal(np.isfinite(facing[0]).all(1), fin)
    assert ((seen["nrm"][fin] * v).sum(1) > -1e-3 * np.linalg.norm(v, axis=1)).all()      # every normal faces the viewpoint
    assert not ((facing[0][fin] * v).sum(1) < 0).any() and ((exp[0][fin] * v).sum(1) < 0).any()


# ---- pn_fpfh ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(2, 17))
def test_fpfh_planes_and_cap(dev, k):
    """radius 0.4 fills the lists, 0.15 leaves them partly filled"""
    x, nrm = _cloud(700)
    _, _, full = _check_fpfh(_raw_fpfh(x, nrm, 0.4, k, dev), x, nrm, 0.4, k)
    _, _, part = _check_fpfh(_raw_fpfh(x, nrm, 0.15, k, dev), x, nrm, 0.15, k)
    assert (full == k).mean() > 0.8 and (part < k).any() and (part > 0).any()


@pytest.mark.parametrize("k", range(2, 17))
def test_fpfh_edge_cloud(dev, edge, k):
    """the lattice's exact coordinates put pair features on bin and |a1| < |a2| boundaries; every pair count 0 .. k occurs"""
    xyz, _ = edge
    nrm = KC.unit_normals(len(xyz))
    for origin in ORIGINS:
        out, counts, pairs = _check_fpfh(_raw_fpfh(xyz, nrm, KC.RADIUS, k, dev, origin=origin), xyz, nrm, KC.RADIUS, k)
    assert np.array_equal(np.unique(pairs), np.arange(k + 1))


def test_fpfh_workspace_grows_with_k(dev):
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    for N in (1, 700, 1684, 8192, 100000):
        need = [L.pn_fpfh_workspace_bytes(N, k) for k in range(2, 17)]
        assert min(need) > 0 and all(a <= b for a, b in zip(need, need[1:])), (N, need)


# ---- pn_icp_normals ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def references():
    """(name, grouped xyz, seg, n_parts, the oracle's 16 nearest) of the part-size reference and tests/test_gpu_icp_plane.py's cases"""
    cases = [("part_sizes",) + KC.part_size_reference()] + list(_normals_cases())
    return [(name, g, seg, n_parts, PO.neighbours(g, seg, n_parts, 16)) for name, g, seg, n_parts in cases]


@pytest.mark.parametrize("k", range(3, 17))
def test_icp_normals(dev, references, k):
    for name, g, seg, n_parts, nbr16 in references:
        out = _raw_normals(g, seg, n_parts, k, dev)
        en, ec, enb = PO.normals(g, seg, n_parts, k)
        assert np.array_equal(enb, nbr16[:, :k]), name                      # the oracle's own prefix property
        assert np.array_equal(out["nbr"], enb), (name, np.argwhere(out["nbr"] != enb)[:5])
        fin = _normals_close(out["nrm"], en)
        assert np.abs(out["curv"][fin].astype(np.float64) - ec[fin]).max() <= 1e-6, name
        assert np.isnan(out["curv"][~fin]).all()
        if name == "degenerate":
            assert (~fin[:14]).all() and fin[14:].all()
        if name == "part_sizes":
            sizes = np.diff(seg)
            filled = (out["nbr"] >= 0).sum(1)
            assert np.array_equal(filled, np.minimum(np.repeat(sizes, sizes), k)) and np.array_equal(fin, np.repeat(sizes, sizes) >= 3)


@pytest.mark.parametrize("k", [2, 17])
def test_icp_normals_refuses_other_k_and_writes_nothing(dev, k):
    from pointcloudprocessing_amd import _lib
    g, seg, n_parts = KC.part_size_reference()
    M = len(g)
    r = _t(g, dev)
    bufs = dict(nrm=_guarded((M, 3), torch.float32, dev), curv=_guarded((M,), torch.float32, dev), nbr=_guarded((M, 17), torch.int32, dev))
    p =lambda n: C.c_void_p(bufs[n][1].data_ptr())                                   # noqa: E731
    rc = _lib.lib().pn_icp_normals(_lib.ptr(r), _seg_c(seg), M, n_parts, k, p("nrm"), p("curv"), p("nbr"), _lib.current_stream())
    torch.cuda.synchronize()
    assert rc != 0 and f"k={k}".encode() in _lib.lib().pn_last_error()
    for name, (buf, _) in bufs.items():
        assert len(buf) > 2 * GUARD and bool((buf == PAT).all()), f"{name}: written by a refused call"
