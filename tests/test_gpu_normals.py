"""pn_scan_normals on the MI355X against the NumPy oracle (tests/normals_oracle.py): the neighbour lists and counts bit for bit with
pn_radius_knn's specification on the cases where the grid lookup or the tie order can go wrong; normals and curvature within the
tolerances tests/test_gpu_icp_plane.py uses for the same Jacobi against the same eigh; both sign rules; guard bands round every
output and each optional output as NULL; purity; the key limit; graph capture; ops.estimate_normals with non-finite rows;
ops.outlier_mask(method="incidence") on the veil scene and PointNet.predict_scan with it.
Every list length k = 2 .. 16 (one kernel each) runs in tests/test_gpu_knn_every_k.py, with ``_raw``, ``_same_lists``, ``_close`` and ``_check`` from here."""
import ctypes as C

import numpy as np
import pytest
import torch

import neighbors_oracle as NO
import normals_oracle as NN

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 4096          # bytes of fill pattern before and after every output buffer and the workspace
PAT = 0xA5
EZ = np.array([0, 0, 1], F32)


def _guarded(nbytes, dev):
    buf = torch.full((GUARD + nbytes + GUARD,), PAT, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + nbytes]


def _raw(x, radius, k, origin=None, viewpoint=None, skip=(), expect_error=0):
    """pn_scan_normals on guard-banded outputs and workspace -> dict(nrm (N, 3) f32, curv (N,) f32, count (N,) i32, idx (N, k) i32);
    an output named in ``skip`` is passed as NULL (and comes back as None).  Asserts that the bands and the input are untouched and
    that the error word is ``expect_error``"""
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(x, F32)).to("cuda:0")
    N = x.shape[0]
    dev = x.device
    if origin is None:
        origin = x.min(0).values.cpu().tolist()
    keep = x.clone()
    nbytes = L.pn_scan_normals_workspace_bytes(N)
    sizes = dict(nrm=12 * N, curv=4 * N, count=4 * N, idx=4 * N * k, ws=nbytes)
    bufs = {name: _guarded(n, dev) for name, n in sizes.items() if name not in skip}
    p = lambda name: C.c_void_p(bufs[name][1].data_ptr()) if name in bufs else None      # noqa: E731
    f3 = lambda v: None if v is None else (C.c_float * 3)(*[float(a) for a in v])         # noqa: E731
    rc = L.pn_scan_normals(_lib.ptr(x), N, float(radius), f3(origin), k, f3(viewpoint), p("nrm"), p("curv"), p("count"), p("idx"), p("ws"),
                           nbytes, _lib.current_stream())
    _lib.check(rc, "pn_scan_normals")
    torch.cuda.synchronize()
    for name, (buf, _) in bufs.items():
        assert bool((buf[:GUARD] == PAT).all()) and bool((buf[-GUARD:] == PAT).all()), f"{name}: guard band overwritten"
    assert torch.equal(keep.view(torch.int32), x.view(torch.int32)), "the input was modified"
    assert int(bufs["ws"][1][:4].view(torch.int32).item()) == expect_error, "error word"
    view = dict(nrm=(torch.float32, (N, 3)), curv=(torch.float32, (N,)), count=(torch.int32, (N,)), idx=(torch.int32, (N, k)))
    return {name: bufs[name][1].view(dt).reshape(shape).cpu().numpy() if name in bufs else None for name, (dt, shape) in view.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same_lists(got, knn):
    """idx and count equal to NO.radius_knn's"""
    assert np.array_equal(got["count"], knn[2]), np.flatnonzero(got["count"] != knn[2])[:5]
    assert np.array_equal(got["idx"], knn[0]), np.flatnonzero((got["idx"] != knn[0]).any(1))[:5]


def _close(got, exp, viewpoint=None, x=None, need_clear=0.9):
    """normals and curvature against the oracle's (nrm, curv, ...): the finite mask equal, | |n . n_oracle| - 1 | <= 1e-6, curvature
    within 1e-6, and the sign equal wherever the oracle's is unambiguous (without a viewpoint: the largest component leads by 1e-3;
    with one: |n . v| / |v| > 1e-3), which must cover more than ``need_clear`` of the finite rows"""
    en, ec = exp[0], exp[1]
    fin = np.isfinite(en).all(1)
    assert np.array_equal(np.isfinite(got["nrm"]).all(1), fin) and np.isnan(got["nrm"][~fin]).all()
    assert np.array_equal(np.isfinite(got["curv"]), fin) and np.isnan(got["curv"][~fin]).all()
    if not fin.any():
        return fin
    g, e = got["nrm"][fin].astype(np.float64), en[fin].astype(np.float64)
    dots = (g * e).sum(1)
    assert np.abs(np.abs(dots) - 1).max() <= 1e-6
    assert np.abs(got["curv"][fin].astype(np.float64) - ec[fin]).max() <= 1e-6
    if viewpoint is None:
        s = np.sort(np.abs(e), axis=1)
        clear = s[:, 2] - s[:, 1] > 1e-3
    else:
        v = np.asarray(viewpoint, F32).astype(np.float64) - np.asarray(x, F32)[fin].astype(np.float64)
        clear = np.abs((e * v).sum(1)) / np.linalg.norm(v, axis=1) > 1e-3
    assert clear.mean() > need_clear and (dots[clear] > 0).all()
    return fin


def _check(x, radius, k, origin=None, viewpoint=None, knn=None, need_clear=0.9, **kw):
    x = np.ascontiguousarray(x, F32)
    knn = NN.radius_knn(x, radius, k) if knn is None else knn
    exp = NN.normals(x, radius, k, viewpoint, knn=knn)
    got = _raw(x, radius, k, origin, viewpoint, **kw)
    _same_lists(got, knn)
    _close(got, exp, viewpoint, x, need_clear)
    return got, exp


# ---- smallest shapes ------------------------------------------------------------------------------------------------
def test_one_and_two_points(dev):
    got = _raw(np.array([[3.25, -1.5, 7.0]], F32), 0.5, 3)
    assert np.isnan(got["nrm"]).all() and np.isnan(got["curv"]).all() and got["count"].tolist() == [0] and got["idx"].tolist() == [[-1, -1, -1]]
    got = _raw(np.array([[3.25, -1.5, 7.0], [3.5, -1.5, 7.0]], F32), 0.5, 2)
    assert np.isnan(got["nrm"]).all() and np.isnan(got["curv"]).all() and got["count"].tolist() == [1, 1] and got["idx"].tolist() == [[1, -1], [0, -1]]


def test_three_points(dev):
    tri = np.array([[0, 0, 5], [1, 0, 5], [0, 1, 5]], F32)
    got, _ = _check(tri, 2.0, 2)
    assert np.array_equal(got["nrm"], np.tile(EZ, (3, 1))) and (got["curv"] == 0).all() and got["count"].tolist() == [2, 2, 2]
    got = _raw(tri, 2.0, 2, viewpoint=(0.0, 0.0, -1.0))
    assert np.array_equal(got["nrm"], np.tile(-EZ, (3, 1)))
    # two identical points and one other: three points on a line
    got, exp = _check(np.array([[1, 2, 3], [1, 2, 3], [1.5, 2, 3.25]], F32), 1.0, 4)
    assert np.isnan(got["nrm"]).all() and got["count"].tolist() == [2, 2, 2] and got["idx"][:, :2].tolist() == [[1, 2], [0, 2], [0, 1]]


def test_all_points_in_one_voxel(dev):
    rng = np.random.default_rng(1)
    x = (rng.random((3000, 3)) * 0.9 + 5.0).astype(F32)                 # several sort tiles, one voxel of leaf ~1.02
    x[:, 2] = (5.0 + 0.02 * rng.random(3000) + 0.1 * x[:, 0]).astype(F32)   # a thin slab: a clear least eigenvector
    got, exp = _check(x, 1.0, 16, origin=(5.0, 5.0, 5.0))
    assert (NO.keys(x, NO.leaf(1.0), (5.0, 5.0, 5.0)) == 0).all() and exp[2].min() > 16 and np.isfinite(got["nrm"]).all()


# ---- neighbour lists and counts, bit for bit ------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1.0, float(np.sqrt(F32(2))), 1.5])
def test_shuffled_lattice(dev, radius):
    x, c = NO.lattice(12, seed=7)
    knn = NO.radius_knn(x, radius, 8)
    got = _raw(x, radius, 8)
    _same_lists(got, knn)
    interior = ((c > 0) & (c < 11)).all(1)
    assert (knn[2][interior] == (6 if F32(radius) * F32(radius) < 2 else 18)).all()
    _same_lists(_raw(x, radius, 8, origin=(-0.5, -0.25, -0.125)), knn)


def test_face_straddling_and_corner_pairs(dev):
    r = F32(0.7)
    for origin in ((0.0, 0.0, 0.0), (-1000.0, 1000.0, -999.5)):
        a, b = NO.adversarial_pairs(r, origin, 40, seed=5, per_kind=4, ulps=3)
        ok = (NO.keys(a, NO.leaf(r), origin) >= 0).all(1) & (NO.keys(b, NO.leaf(r), origin) >= 0).all(1)
        x = np.concatenate([a[ok], b[ok]])
        assert 400 < len(x) < 4000
        _same_lists(_raw(x, r, 4, origin=origin), NO.radius_knn(x, r, 4))


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_cloud_one_voxel_thick(dev, axis):
    rng = np.random.default_rng(axis)
    x = (rng.random((2500, 3)) * 6.0).astype(F32)
    x[:, axis] = (rng.random(2500) * 0.4).astype(F32)                     # key 0 on that axis: no -1 neighbour rows / cells
    got, exp = _check(x, 0.5, 8, origin=(0.0, 0.0, 0.0), need_clear=0.5)
    assert exp[2].mean() > 3 and (NO.keys(x, NO.leaf(0.5), (0.0, 0.0, 0.0))[:, axis] == 0).all()


def test_queries_at_key_zero_on_every_axis(dev):
    rng = np.random.default_rng(9)
    x = (rng.random((3000, 3)) * 3.0).astype(F32)
    got, exp = _check(x, 0.5, 16, need_clear=0.5)                         # origin = the minimum: the corner voxel is (0, 0, 0)
    assert (NO.keys(x, NO.leaf(0.5), x.min(0)) == 0).all(1).sum() > 5 and exp[2].max() > 16


# ---- the surface cloud ----------------------------------------------------------------------------------------------
SURFACE_RADIUS = 0.215
VIEWPOINT = (20.0, 5.0, 4.0)       # oblique; the oracle's |n . v| / |v| exceeds 1e-3 on 99.8 % of the rows (checked on the CPU)


@pytest.fixture(scope="module")
def surface():
    x = NO.surface_cloud()
    knn16 = NN.radius_knn(x, SURFACE_RADIUS, 16)
    assert 9 < knn16[2].mean() < 11 and knn16[2].max() > 16 and (knn16[2] < 2).any()
    return x, knn16


def _prefix(knn16, k):
    return knn16[0][:, :k].copy(), knn16[1][:, :k].copy(), knn16[2]      # the k nearest are a prefix of the 16 nearest


@pytest.mark.parametrize("k", [2, 8, 16])
def test_surface_cloud(dev, surface, k):
    x, knn16 = surface
    got, exp = _check(x, SURFACE_RADIUS, k, knn=_prefix(knn16, k))
    fin = np.isfinite(exp[0]).all(1)
    # (three points always lie in a plane: at k = 2 the least eigenvalue is a rounding residue of either sign, some 1e-17)
    assert 0.99 < fin.mean() < 1 and (got["curv"][fin] >= -1e-6).all() and (got["curv"][fin] <= 1 / 3 + 1e-6).all()
    assert np.abs(np.linalg.norm(got["nrm"][fin].astype(np.float64), axis=1) - 1).max() < 1e-6


@pytest.mark.parametrize("k", [2, 8, 16])
def test_surface_cloud_with_a_viewpoint(dev, surface, k):
    x, knn16 = surface
    got, exp = _check(x, SURFACE_RADIUS, k, viewpoint=VIEWPOINT, knn=_prefix(knn16, k))
    fin = np.isfinite(exp[0]).all(1)
    v = np.asarray(VIEWPOINT) - x[fin].astype(np.float64)
    assert ((got["nrm"][fin] * v).sum(1) > -1e-3 * np.linalg.norm(v, axis=1)).all()       # every normal faces the viewpoint
    plain = NN.normals(x, SURFACE_RADIUS, k, knn=_prefix(knn16, k))[0][fin]
    assert not ((exp[0][fin] * v).sum(1) < 0).any() and ((plain * v).sum(1) < 0).any()      # ... which the other rule's do not


def test_each_optional_output_as_null(dev, surface):
    x, knn16 = surface
    xt = torch.from_numpy(x).to(dev)
    full = _raw(xt, SURFACE_RADIUS, 8, viewpoint=VIEWPOINT)
    for skip in (("curv",), ("count",), ("idx",), ("curv", "count", "idx")):
        got = _raw(xt, SURFACE_RADIUS, 8, viewpoint=VIEWPOINT, skip=skip)
        for name, a in got.items():
            assert (a is None) == (name in skip)
            assert a is None or np.array_equal(_bits(a), _bits(full[name])), name


def test_dense_ball_beside_an_isolated_pair(dev):
    rng = np.random.default_rng(2)
    v = rng.normal(size=(500, 3))
    ball = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.random((500, 1)) ** (1 / 3) * 0.25 + 10.0
    x = np.concatenate([[[14.0, 10.0, 10.0]], ball, [[14.5, 10.0, 10.0]]]).astype(F32)
    got, exp = _check(x, 1.0, 16, need_clear=0.5)
    assert (exp[2][1:-1] == 499).all() and exp[2][[0, -1]].tolist() == [1, 1]              # only the first 16 of 499 enter
    assert np.isfinite(got["nrm"][1:-1]).all() and np.isnan(got["nrm"][[0, -1]]).all() and got["idx"][0].tolist() == [501] + [-1] * 15


# ---- exact inputs ---------------------------------------------------------------------------------------------------
def test_lattice_plane_is_exact_on_the_device(dev):
    x = NN.lattice_plane()
    for vp, sign in NN.LATTICE_PLANE_VIEWS:                                # none, above, below, in the plane (s == 0)
        got = _raw(x, 1.5, 8, viewpoint=vp)
        assert np.array_equal(got["nrm"], np.tile(sign * EZ, (len(x), 1))), vp
        assert (got["curv"] == 0).all() and np.array_equal(got["count"], NO.radius_knn(x, 1.5, 0)[2])


# ---- purity ---------------------------------------------------------------------------------------------------------
def test_two_origins_two_calls_and_far_from_zero(dev):
    shift = (1000.0, -1000.0, 1000.0)
    x = NO.surface_cloud(shift=shift)
    vp = tuple(np.add(VIEWPOINT, shift))
    knn = NN.radius_knn(x, SURFACE_RADIUS, 8)
    assert 4 < knn[2].mean() < 20
    xt = torch.from_numpy(x).to(dev)
    a = _raw(xt, SURFACE_RADIUS, 8, viewpoint=vp)
    b = _raw(xt, SURFACE_RADIUS, 8, origin=(990.03, -1010.7, 995.9), viewpoint=vp)
    c = _raw(xt, SURFACE_RADIUS, 8, viewpoint=vp)
    for name in a:
        assert np.array_equal(_bits(a[name]), _bits(b[name])) and np.array_equal(_bits(a[name]), _bits(c[name])), name
    _same_lists(a, knn)
    _close(a, NN.normals(x, SURFACE_RADIUS, 8, vp, knn=knn), vp, x)


# ---- ops ------------------------------------------------------------------------------------------------------------
def test_non_finite_rows_through_ops(dev):
    from pointcloudprocessing_amd import ops
    x = NO.surface_cloud(3000, seed=6)
    bad = {7: (np.nan, 1.0, 1.0), 100: (1.0, np.inf, 1.0), 101: (1.0, 1.0, -np.inf), 3002: (np.nan, np.nan, np.nan)}
    full = np.insert(x, [7, 99, 99, 2999], 0.0, axis=0)                   # the bad rows land at 7, 100, 101 and 3002
    rows = sorted(bad)
    for r in rows:
        full[r] = bad[r]
    good = np.setdiff1d(np.arange(len(full)), rows)
    assert np.array_equal(full[good], x)
    exp = NN.normals(x, 0.3, 8, VIEWPOINT)
    xt = torch.from_numpy(full.astype(F32)).to(dev)
    nrm, curv, count, idx = (t.cpu().numpy() for t in ops.estimate_normals(xt, 0.3, 8, viewpoint=VIEWPOINT, return_neighbors=True))
    assert np.isnan(nrm[rows]).all() and np.isnan(curv[rows]).all() and (count[rows] == 0).all() and (idx[rows] == -1).all()
    assert np.array_equal(count[good], exp[2])
    assert np.array_equal(idx[good], np.where(exp[3] >= 0, good[np.clip(exp[3], 0, None)], -1))      # rows of xyz AS PASSED IN
    assert not np.isin(idx, rows).any()
    _close(dict(nrm=nrm[good], curv=curv[good]), exp, VIEWPOINT, x)
    three = ops.estimate_normals(xt, 0.3, 8, viewpoint=VIEWPOINT)
    assert len(three) == 3 and np.array_equal(_bits(three[0].cpu().numpy()), _bits(nrm))
    # without the bad rows the call takes the uncompacted path: the same bits
    alone = ops.estimate_normals(torch.from_numpy(x).to(dev), 0.3, 8, viewpoint=VIEWPOINT, return_neighbors=True)
    assert np.array_equal(_bits(alone[0].cpu().numpy()), _bits(nrm[good])) and np.array_equal(alone[3].cpu().numpy(), exp[3])
    none = ops.estimate_normals(torch.full((5, 3), float("nan"), device=dev), 1.0, 2)
    assert bool(torch.isnan(none[0]).all()) and none[2].tolist() == [0] * 5
    keep = ops.outlier_mask(xt, "incidence", 0.3, k=8, viewpoint=VIEWPOINT, max_angle_deg=80.0)
    assert torch.equal(keep, ops.incidence_mask(xt, three[0], VIEWPOINT, 80.0))
    keep = keep.cpu().numpy()
    assert not keep[rows].any() and 0 < keep[good].sum() < len(good)


def test_key_limit_sets_the_error_word_and_raises(dev):
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd._lib import PointNetHipError
    x = NO.surface_cloud(2000, seed=2)
    x[-1] = (10.0 + 0.011 * NO.MAX_KEY, 5.0, 0.0)                          # one point beyond 2^14 leaves of ~0.0102
    xt = torch.from_numpy(x).to(dev)
    _raw(xt, 0.01, 4, (0.0, 0.0, -2.0), expect_error=1)                    # an ordinary guarded call: nothing outside the buffers
    _raw(xt, 0.01, 2, (0.5, 0.0, -2.0), expect_error=1)                    # a key below 0
    with pytest.raises(PointNetHipError, match="16384"):
        ops.estimate_normals(xt, 0.01, 4)
    got = ops.estimate_normals(xt[:-1].contiguous(), 0.05, 4, return_neighbors=True)      # without that point the cloud fits
    knn = NO.radius_knn(x[:-1], 0.05, 4)
    assert np.array_equal(got[3].cpu().numpy(), knn[0]) and np.array_equal(got[2].cpu().numpy(), knn[2])


def test_graph_capture_replays_on_a_second_input(dev):
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    a, b = NO.surface_cloud(6000, seed=21), NO.surface_cloud(6000, seed=22)
    k, radius = 8, 0.25
    ea, eb = NN.normals(a, radius, k, VIEWPOINT), NN.normals(b, radius, k, VIEWPOINT)
    assert not np.array_equal(ea[2], eb[2])
    N = len(a)
    x = torch.from_numpy(a).to(dev)
    nbytes = L.pn_scan_normals_workspace_bytes(N)
    bufs = {name: _guarded(n, dev) for name, n in dict(nrm=12 * N, curv=4 * N, cnt=4 * N, idx=4 * N * k, ws=nbytes).items()}
    nrm, curv = bufs["nrm"][1].view(torch.float32).reshape(N, 3), bufs["curv"][1].view(torch.float32)
    cnt, idx, ws = bufs["cnt"][1].view(torch.int32), bufs["idx"][1].view(torch.int32).reshape(N, k), bufs["ws"][1]
    org = (C.c_float * 3)(-0.5, -0.5, -2.0)

    def call():
        vp = (C.c_float * 3)(*VIEWPOINT)                                   # read during the call: it may go out of scope afterwards
        _lib.check(L.pn_scan_normals(_lib.ptr(x), N, radius, org, k, vp, _lib.ptr(nrm), _lib.ptr(curv), _lib.ptr(cnt), _lib.ptr(idx),
                                     _lib.ptr(ws), nbytes, _lib.current_stream()), "pn_scan_normals")

    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                           # warm-up on the capture stream
        with torch.cuda.graph(g, stream=side):
            call()
    torch.cuda.current_stream().wait_stream(side)
    for data, exp in ((b, eb), (a, ea)):
        x.copy_(torch.from_numpy(data).to(dev))
        for t in (nrm, curv, cnt, idx):
            t.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        assert int(ws[:4].view(torch.int32).item()) == 0
        for name, (buf, _) in bufs.items():
            assert bool((buf[:GUARD] == PAT).all()) and bool((buf[-GUARD:] == PAT).all()), f"{name}: guard band overwritten"
        got = dict(nrm=nrm.cpu().numpy(), curv=curv.cpu().numpy(), count=cnt.cpu().numpy(), idx=idx.cpu().numpy())
        _same_lists(got, (exp[3], None, exp[2]))
        _close(got, exp, VIEWPOINT, data)


# ---- the incidence filter -------------------------------------------------------------------------------------------
def test_outlier_mask_incidence_on_the_veil_scene(dev):
    from pointcloudprocessing_amd import ops
    VEIL = NN.VEIL_SETTINGS
    xyz, kind, en, ec, keep, margin, count = (NN.veil_case()[name] for name in ("xyz", "kind", "nrm", "curv", "keep", "margin", "count"))
    assert margin.min() > 1e-5                                             # no decision near the threshold: the masks must be equal
    xt = torch.from_numpy(xyz).to(dev)
    got = ops.outlier_mask(xt, "incidence", **VEIL)                        # viewpoint: the default, the sensor origin
    nrm, curv, cnt = ops.estimate_normals(xt, VEIL["radius"], VEIL["k"], viewpoint=(0.0, 0.0, 0.0))
    assert got.dtype == torch.bool and torch.equal(got, ops.incidence_mask(xt, nrm, (0.0, 0.0, 0.0), VEIL["max_angle_deg"]))
    assert np.array_equal(cnt.cpu().numpy(), count)
    _close(dict(nrm=nrm.cpu().numpy(), curv=curv.cpu().numpy()), (en, ec), (0.0, 0.0, 0.0), xyz)
    assert np.array_equal(got.cpu().numpy(), keep)
    veil = kind == NN.VEIL
    assert keep[veil].mean() <= 0.10 and keep[~veil].mean() >= 0.99
    radius_keep = ops.outlier_mask(xt, "radius", VEIL["radius"], min_neighbors=8).cpu().numpy()
    assert radius_keep[veil].mean() > 0.5


INCIDENCE = dict(method="incidence", radius=1.0, k=8, max_angle_deg=75.0)


def _tbits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int64) if t.dtype == torch.float64 else t)


def test_predict_scan_with_the_incidence_filter(dev):
    from oracle import pointnet_oracle as O
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd.pointnet.PointNet import PointNet
    scene, rows, noise_rows, clean = NO.noisy_scene()
    # the facts from the oracle (measured: 3,269 of 4,296 kept, none of the 200 noise points, nearest decision 1.1e-4 from the threshold)
    en = NN.normals(scene, INCIDENCE["radius"], INCIDENCE["k"], (0.0, 0.0, 0.0))[0]
    want, margin = NN.incidence_mask(scene, en, (0.0, 0.0, 0.0), INCIDENCE["max_angle_deg"], return_margin=True)
    assert margin.min() > 1e-5 and not want[noise_rows].any() and 3000 < want.sum() < 3500
    model = PointNet(23, 12, 0.3, 42, precision="bf16", device=dev)
    model.set_weights(O.init_params(23, 12, seed=4, randomize_bn=True))
    xt = torch.from_numpy(scene).to(dev)
    keep = ops.outlier_mask(xt, **INCIDENCE)
    assert np.array_equal(keep.cpu().numpy(), want)
    at = keep.nonzero().squeeze(1)
    kw = dict(leaf=0.5, samples=1024, k=3, return_confidence=True)
    ci0, part0, R0, conf0 = model.predict_scan(xt[at].contiguous(), **kw)
    ci, part, R, conf = model.predict_scan(xt, denoise=INCIDENCE, **kw)
    assert tuple(part.shape) == (1, len(scene)) and tuple(conf.shape) == (1, len(scene)) and part.dtype == part0.dtype
    assert torch.equal(ci, ci0) and torch.equal(_tbits(R), _tbits(R0))
    assert torch.equal(part[0, at], part0[0]) and torch.equal(_tbits(conf[0, at]), _tbits(conf0[0])) and bool((part0 >= 0).all())
    assert bool((part[0, ~keep] == -1).all()) and bool((conf[0, ~keep] == 0).all())
    a, b = model.predict_scan(xt, **kw), model.predict_scan(xt, denoise=None, **kw)
    assert all(torch.equal(_tbits(u), _tbits(v)) for u, v in zip(a, b)) and bool((a[1] >= 0).all())
