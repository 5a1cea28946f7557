"""pn_fpfh, pn_feature_match and pn_ransac_poses on the MI355X against the NumPy oracle (tests/fpfh_oracle.py): the SPFH counts, the pair
counts and the descriptors bit for bit; the matches bit for bit; the draws and validity flags exactly, the poses within the
tolerance tests/test_gpu_semantic_icp.py uses for the device Kabsch against NumPy, the counts exactly at the device's own poses
(teacher forcing); guard bands round every output and the workspace; graph capture of the three entries in a row; and
ops.global_register / register_scans(init="global") on the registration fixture against the oracle pipeline driven by the device's
hypotheses.
Every list length k = 2 .. 16 of pn_fpfh (one SPFH kernel each) runs in tests/test_gpu_knn_every_k.py, with ``_raw_fpfh`` and ``_check_fpfh`` from here."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import fpfh_oracle as FO
import icp_oracle as IO

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 4096          # bytes of fill pattern before and after every output buffer and the workspace
PAT = 0xA5
POSE_TOL = 1e-12      # absolute, on metre-scale fixtures: tests/test_gpu_semantic_icp.py's for the device Kabsch against NumPy


def _guarded(nbytes, dev):
    buf = torch.full((GUARD + nbytes + GUARD,), PAT, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + nbytes]


def _bands_ok(bufs):
    for name, (buf, _) in bufs.items():
        assert bool((buf[:GUARD] == PAT).all()) and bool((buf[-GUARD:] == PAT).all()), f"{name}: guard band overwritten"


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _t(a, dev, dtype=F32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


# ---- pn_fpfh ---------------------------------------------------------------------------------------------------------
def _raw_fpfh(x, n, radius, k, dev, origin=None, spfh=True):
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    x, n = _t(x, dev), _t(n, dev)
    N = x.shape[0]
    if origin is None:
        origin = x.min(0).values.cpu().tolist()
    keep = (x.clone(), n.clone())
    nbytes = L.pn_fpfh_workspace_bytes(N, k)
    sizes = dict(out=4 * 33 * N, ws=nbytes, **(dict(counts=4 * 33 * N, pairs=4 * N) if spfh else {}))
    bufs = {name: _guarded(b, dev) for name, b in sizes.items()}
    p = lambda name: C.c_void_p(bufs[name][1].data_ptr()) if name in bufs else None      # noqa: E731
    rc = L.pn_fpfh(_lib.ptr(x), _lib.ptr(n), N, float(radius), (C.c_float * 3)(*[float(a) for a in origin]), k, p("out"), p("counts"), p("pairs"),
                   p("ws"), nbytes, _lib.current_stream())
    _lib.check(rc, "pn_fpfh")
    torch.cuda.synchronize()
    _bands_ok(bufs)
    assert torch.equal(keep[0].view(torch.int32), x.view(torch.int32)) and torch.equal(keep[1].view(torch.int32), n.view(torch.int32))
    assert int(bufs["ws"][1][:4].view(torch.int32).item()) == 0, "error word"
    out = bufs["out"][1].view(torch.float32).reshape(N, 33).cpu().numpy()
    if not spfh:
        return out
    return out, bufs["counts"][1].view(torch.int32).reshape(N, 33).cpu().numpy(), bufs["pairs"][1].view(torch.int32).cpu().numpy()


def _check_fpfh(got, x, n, radius, k):
    out, counts, pairs = FO.fpfh(x, n, radius, k, return_spfh=True)
    assert np.array_equal(got[2], pairs) and np.array_equal(got[1], counts)
    assert np.array_equal(_bits(got[0]), _bits(out))
    return out, counts, pairs


@functools.lru_cache(maxsize=None)
def _cloud(n):
    return FO.planes_and_cap(n, seed=n)


@pytest.mark.parametrize("n,k,radius", [(1, 16, 0.2), (2, 2, 5.0), (257, 16, 0.3), (257, 2, 0.3), (700, 16, 0.4), (700, 16, 0.08), (700, 5, 0.15)])
def test_fpfh_bit_for_bit(dev, n, k, radius):
    """two perpendicular planes and a sphere cap: N = 1 (no neighbour: a zero row), 2, a block plus one, about 700; k = 2 and 16; a
    radius that fills every list and one (0.08) that leaves lists partly filled or empty"""
    x, nrm = _cloud(n)
    got = _raw_fpfh(x, nrm, radius, k, dev)
    out, counts, pairs = _check_fpfh(got, x, nrm, radius, k)
    if n == 1:
        assert not out.any() and pairs[0] == 0
    if n == 700 and radius == 0.08:
        assert ((pairs > 0) & (pairs < k)).any() and (pairs == 0).any()
    if n == 700 and radius == 0.4:
        assert (pairs == k).mean() > 0.8 and np.count_nonzero(out) > 5 * n
        assert np.array_equal(_bits(_raw_fpfh(x, nrm, radius, k, dev, spfh=False)), _bits(out))       # the optional outputs as NULL


def test_fpfh_duplicates_nan_normals_isolated_point_and_origin(dev):
    x, nrm = (a.copy() for a in _cloud(700))
    x[100:110] = x[90:100]                                                  # exact duplicates: d = 0, a neighbour whose pair is skipped
    nrm[100:110] = nrm[90:100]
    nrm[[5, 300, 301]] = np.nan                                             # rows without a normal
    nrm[450, 1] = np.inf
    x[699] = [40.0, 40.0, 40.0]                                             # an isolated point
    for origin in (None, (-3.0, -2.5, -7.0)):
        got = _raw_fpfh(x, nrm, 0.25, 16, dev, origin=origin)
        out, counts, pairs = _check_fpfh(got, x, nrm, 0.25, 16)
    assert pairs[5] == 0 and out[5].any() and not out[699].any() and pairs[100] < 16


def test_ops_fpfh_masks_non_finite_rows(dev):
    from pointcloudprocessing_amd import ops
    x, nrm = (a.copy() for a in _cloud(700))
    bad = [0, 17, 350, 699]
    x[bad] = [[np.nan, 0, 0], [0, np.inf, 0], [np.nan] * 3, [0, 0, -np.inf]]
    nrm[40] = np.nan
    fin = np.setdiff1d(np.arange(700), bad)
    out, counts, pairs = FO.fpfh(x[fin], nrm[fin], 0.25, 16, return_spfh=True)
    got = [t.cpu().numpy() for t in ops.fpfh(_t(x, dev), _t(nrm, dev), 0.25, return_spfh=True)]
    assert np.array_equal(_bits(got[0][fin]), _bits(out)) and np.array_equal(got[1][fin], counts) and np.array_equal(got[2][fin], pairs)
    assert not got[0][bad].any() and not got[1][bad].any() and not got[2][bad].any()
    assert np.array_equal(_bits(ops.fpfh(_t(x, dev), _t(nrm, dev), 0.25, origin=(-9.0, -9.0, -9.0)).cpu().numpy()), _bits(got[0]))
    none = ops.fpfh(torch.full((5, 3), float("nan"), device=dev), torch.zeros(5, 3, device=dev), 1.0)
    assert none.shape == (5, 33) and not bool(none.any())
    # the descriptors of ops.estimate_normals' normals: the composition a user runs
    xt = _t(_cloud(700)[0], dev)
    n_dev = ops.estimate_normals(xt, 0.25, 16, viewpoint=(1.0, 1.0, 5.0))[0]
    assert np.array_equal(_bits(ops.fpfh(xt, n_dev, 0.25).cpu().numpy()), _bits(FO.fpfh(_cloud(700)[0], n_dev.cpu().numpy(), 0.25)))


# ---- pn_feature_match ------------------------------------------------------------------------------------------------
def _raw_match(a, b, dev):
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    a, b = _t(a, dev), _t(b, dev)
    Na, Nb = a.shape[0], b.shape[0]
    nbytes = L.pn_feature_match_workspace_bytes(Na, Nb)
    bufs = {name: _guarded(n, dev) for name, n in dict(idx=4 * Na, d2=4 * Na, ws=nbytes).items()}
    p = lambda name: C.c_void_p(bufs[name][1].data_ptr())      # noqa: E731
    _lib.check(L.pn_feature_match(_lib.ptr(a), Na, _lib.ptr(b), Nb, 33, p("idx"), p("d2"), p("ws"), nbytes, _lib.current_stream()), "pn_feature_match")
    torch.cuda.synchronize()
    _bands_ok(bufs)
    return bufs["idx"][1].view(torch.int32).cpu().numpy(), bufs["d2"][1].view(torch.float32).cpu().numpy()


def _descriptors(n, seed):
    rng = np.random.default_rng(seed)
    f = rng.random((n, 33)) ** 3 * 200.0
    return f.astype(F32)


@pytest.mark.parametrize("na,nb", [(1, 1), (300, 513), (257, 256), (40, 2100)])
def test_feature_match_bit_for_bit(dev, na, nb):
    """one row each; sizes that are no multiple of the block or the tile; more than one slice of b (2,100 rows); duplicated rows of b
    (the tie goes to the lower row); NaN and inf rows on either side"""
    from pointcloudprocessing_amd import ops
    a, b = _descriptors(na, 1), _descriptors(nb, 2)
    if nb > 100:
        b[70] = b[3]
        b[nb - 1] = b[3]
        a[0] = b[3]                                                         # an exact match with three candidates
        a[7] = b[10]
        b[10, 4] = np.nan                                                   # a[7]'s twin is not finite: somebody else wins
        b[11, 32] = np.inf
        a[5, 0] = np.nan
        a[6, 20] = -np.inf
    idx, d2 = FO.feature_match(a, b)
    got = _raw_match(a, b, dev)
    assert np.array_equal(got[0], idx) and np.array_equal(_bits(got[1]), _bits(d2))
    if nb > 100:
        assert idx[0] == 3 and d2[0] == 0 and idx[5] == -1 and idx[6] == -1 and np.isinf(d2[5]) and idx[7] >= 0 and not np.isin(idx, [10, 11]).any()
    for mutual in (False, True):
        oi, od = ops.feature_match(_t(a, dev), _t(b, dev), mutual=mutual)
        ei, ed = FO.feature_match(a, b, mutual)
        assert np.array_equal(oi.cpu().numpy(), ei) and np.array_equal(_bits(od.cpu().numpy()), _bits(ed))
    if (na, nb) == (300, 513):
        assert 0 < (ei >= 0).sum() < (idx >= 0).sum()                        # mutual matching drops pairs
    if nb == 1:
        nan_b = np.full((1, 33), np.nan, F32)
        gi, gd = _raw_match(a, nan_b, dev)
        assert gi.tolist() == [-1] and np.isinf(gd[0])


def test_feature_match_refuses_other_widths(dev):
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd._lib import PointNetHipError
    with pytest.raises(PointNetHipError, match="width=32"):
        ops.feature_match(torch.zeros(4, 32, device=dev), torch.zeros(4, 32, device=dev))


# ---- pn_ransac_poses -------------------------------------------------------------------------------------------------
def _raw_ransac(src, tgt, max_dist, H, edge, seed, dev):
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    s, t = _t(src, dev), _t(tgt, dev)
    Cn = s.shape[0]
    nbytes = L.pn_ransac_poses_workspace_bytes(Cn, H)
    bufs = {name: _guarded(n, dev) for name, n in dict(poses=128 * H, counts=4 * H, rows=12 * H, ws=nbytes).items()}
    p = lambda name: C.c_void_p(bufs[name][1].data_ptr())      # noqa: E731
    _lib.check(L.pn_ransac_poses(_lib.ptr(s), _lib.ptr(t), Cn, float(max_dist), H, float(edge), int(seed), p("poses"), p("counts"), p("rows"), p("ws"),
                                 nbytes, _lib.current_stream()), "pn_ransac_poses")
    torch.cuda.synchronize()
    _bands_ok(bufs)
    return (bufs["poses"][1].view(torch.float64).reshape(H, 4, 4).cpu().numpy(), bufs["counts"][1].view(torch.int32).cpu().numpy(),
            bufs["rows"][1].view(torch.int32).reshape(H, 3).cpu().numpy())


def _check_ransac(src, tgt, max_dist, H, edge, seed, dev):
    """teacher-forced: draws and validity exactly, valid poses within POSE_TOL of the SVD fit, counts exactly at the device's poses"""
    poses, counts, rows = _raw_ransac(src, tgt, max_dist, H, edge, seed, dev)
    exp_rows = FO.draws(len(src), H, seed)
    assert np.array_equal(rows, exp_rows)
    ok = FO.valid(src, tgt, exp_rows, edge)
    assert np.array_equal(counts >= 0, ok) and (counts[~ok] == -1).all() and np.isnan(poses[~ok]).all()
    want = FO.poses(np.asarray(src, F32), np.asarray(tgt, F32), exp_rows, ok)
    if ok.any():
        assert np.abs(poses[ok] - want[ok]).max() <= POSE_TOL, np.abs(poses[ok] - want[ok]).max()
        assert np.array_equal(poses[ok][:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (int(ok.sum()), 1)))
    exp_counts = np.where(ok, FO.count_inliers(src, tgt, np.nan_to_num(poses).astype(F32), max_dist), -1)
    assert np.array_equal(counts, exp_counts)
    return poses, counts, rows, ok


@pytest.mark.parametrize("H", [1, 255, 1024])
def test_ransac_poses_teacher_forced(dev, H):
    src, tgt, true = FO.correspondences(200, 0.6, seed=4)
    poses, counts, rows, ok = _check_ransac(src, tgt, 0.02, H, 0.9, 0, dev)
    if H == 1024:
        assert 3 < ok.sum() < H // 2 and counts.max() >= 60                 # the 80 right pairs: some hypothesis finds most of them
        best = poses[FO.rank(counts)[0]]
        ang, dt = IO.pose_error(best, true)
        assert ang < 0.02 and dt < 0.05
        other = _raw_ransac(src, tgt, 0.02, H, 0.9, 1 << 33, dev)
        assert not np.array_equal(other[2], rows) and np.array_equal(other[2], FO.draws(200, H, 1 << 33))       # two seeds, two sets of draws
        _check_ransac(src, tgt, 0.02, H, 0.0, 7, dev)                       # edge_ratio 0: only the degenerate draws are invalid
        from pointcloudprocessing_amd import ops
        op, oc, order, orows = ops.ransac_poses(_t(src, dev), _t(tgt, dev), 0.02, H, 0.9, 0, return_rows=True)
        assert np.array_equal(oc.cpu().numpy(), counts) and np.array_equal(order.cpu().numpy(), FO.rank(counts))
        assert np.array_equal(op.cpu().numpy().view(np.int64), poses.view(np.int64)) and np.array_equal(orows.cpu().numpy(), rows)


def test_ransac_poses_small_collinear_repeated_and_nan(dev):
    src, tgt, _ = FO.correspondences(3, 0.0, seed=5)
    poses, counts, rows, ok = _check_ransac(src, tgt, 0.05, 255, 0.5, 0, dev)   # C = 3: two draws in nine are a permutation of the rows
    assert 20 < ok.sum() < 120 and (counts[ok] == 3).all()
    line = np.stack([np.arange(50.0), np.zeros(50), np.zeros(50)], 1).astype(F32)
    poses, counts, rows, ok = _check_ransac(line, line + F32(1.0), 0.1, 255, 0.9, 0, dev)      # all collinear: nothing is valid
    assert not ok.any() and (counts == -1).all()
    src, tgt, _ = FO.correspondences(200, 0.5, seed=6)
    src[20:60] = src[20]                                                      # repeated rows: distinct indices, coincident points
    tgt[20:60] = tgt[20]
    src[[3, 150]] = [[np.nan, 0, 0], [0, np.inf, 0]]
    tgt[7, 2] = np.nan
    _check_ransac(src, tgt, 0.02, 1024, 0.9, 3, dev)


# ---- the three entries in one graph ----------------------------------------------------------------------------------
def test_graph_capture_replays_on_a_second_input(dev):
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    N, k, radius, H = 700, 16, 0.25, 255
    clouds = [FO.planes_and_cap(N, seed=s) for s in (31, 32)]
    x, nrm = torch.empty(N, 3, device=dev), torch.empty(N, 3, device=dev)
    nb = (L.pn_fpfh_workspace_bytes(N, k), L.pn_feature_match_workspace_bytes(N, N), L.pn_ransac_poses_workspace_bytes(N, H))
    bufs = {name: _guarded(n, dev) for name, n in dict(f=132 * N, idx=4 * N, d2=4 * N, poses=128 * H, counts=4 * H, ws0=nb[0], ws1=nb[1], ws2=nb[2]).items()}
    v = lambda name: bufs[name][1]      # noqa: E731
    org = (C.c_float * 3)(-1.0, -1.0, -1.0)
    shifted = torch.empty(N, 3, device=dev)

    def call():
        st = _lib.current_stream()
        _lib.check(L.pn_fpfh(_lib.ptr(x), _lib.ptr(nrm), N, radius, org, k, _lib.ptr(v("f")), None, None, _lib.ptr(v("ws0")), nb[0], st), "pn_fpfh")
        _lib.check(L.pn_feature_match(_lib.ptr(v("f")), N, _lib.ptr(v("f")), N, 33, _lib.ptr(v("idx")), _lib.ptr(v("d2")), _lib.ptr(v("ws1")), nb[1], st),
                   "pn_feature_match")
        _lib.check(L.pn_ransac_poses(_lib.ptr(x), _lib.ptr(shifted), N, 0.05, H, 0.9, 5, _lib.ptr(v("poses")), _lib.ptr(v("counts")), None,
                                     _lib.ptr(v("ws2")), nb[2], st), "pn_ransac_poses")

    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    x.copy_(_t(clouds[0][0], dev)); nrm.copy_(_t(clouds[0][1], dev)); shifted.copy_(x + 1.0)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                           # warm-up on the capture stream
        with torch.cuda.graph(g, stream=side):
            call()
    torch.cuda.current_stream().wait_stream(side)
    for cx, cn in (clouds[1], clouds[0]):
        x.copy_(_t(cx, dev)); nrm.copy_(_t(cn, dev)); shifted.copy_(x + 1.0)
        for name in ("f", "idx", "d2", "poses", "counts"):
            v(name).fill_(0x5A)
        g.replay()
        torch.cuda.synchronize()
        _bands_ok(bufs)
        f = v("f").view(torch.float32).reshape(N, 33).cpu().numpy()
        assert np.array_equal(_bits(f), _bits(FO.fpfh(cx, cn, radius, k)))
        ei, ed = FO.feature_match(f, f)
        assert np.array_equal(v("idx").view(torch.int32).cpu().numpy(), ei) and np.array_equal(_bits(v("d2").view(torch.float32).cpu().numpy()), _bits(ed))
        replayed = (v("poses").view(torch.float64).reshape(H, 4, 4).cpu().numpy(), v("counts").view(torch.int32).cpu().numpy())
        eager = _raw_ransac(x.cpu().numpy(), shifted.cpu().numpy(), 0.05, H, 0.9, 5, dev)
        assert np.array_equal(replayed[0].view(np.int64), eager[0].view(np.int64)) and np.array_equal(replayed[1], eager[1])
        assert (replayed[1] >= 0).sum() > 10


# ---- end to end ------------------------------------------------------------------------------------------------------
def test_global_registration_of_the_fixture(dev):
    """register_scans(init="global") registers the pair the local solver cannot: within the bounds tests/test_cpu_fpfh.py establishes
    for the oracle pipeline (fpfh_oracle.BOUND_ROT, BOUND_T).  Against the oracle pipeline driven by the device's own hypotheses: the
    pose within the bound tests/test_gpu_icp_global.py holds global_pose to (1e-5 rad, 1e-4 m); the winner among the oracle's
    candidates of lowest cost.  (On this pair several of the refined candidates converge to the same minimum and their costs, sums of
    fp32 distances, differ in the last digits only: which of them is first is not a property of the pipeline, so candidates within
    1e-6 of the lowest cost, relative, count as that minimum; the cost itself is held to the same 1e-6.)"""
    from pointcloudprocessing_amd import ops
    sc, S = FO.scene(), FO.SCENE
    src, tgt = _t(sc["source"], dev), _t(sc["target"], dev)
    sv, tv = sc["source_viewpoint"].tolist(), sc["target_viewpoint"].tolist()
    # the default init is the local solver from the identity, and it does not register this pair
    before = ops.register_scans(src, tgt, S["max_dist"], max_iters=S["max_iters"])
    eye = ops.register_scans(src, tgt, S["max_dist"], init_pose=torch.eye(4, device=dev, dtype=torch.float64), max_iters=S["max_iters"])
    assert len(before) == 5 and all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(before, eye))
    a0, t0 = IO.pose_error(before[0][0].cpu().numpy(), sc["pose"])
    assert a0 > 10 * FO.BOUND_ROT and t0 > 10 * FO.BOUND_T
    got = ops.register_scans(src, tgt, S["max_dist"], init="global", feature_radius=S["feature_radius"], normals_radius=S["normals_radius"],
                             hypotheses=S["hypotheses"], keep=S["keep"], top=S["top"], mutual=S["mutual"], seed=S["seed"], viewpoint=tv,
                             source_viewpoint=sv, max_iters=S["max_iters"])
    assert len(got) == 7
    pose, rmse, pairs, iters, status, cost, winner = (t.cpu().numpy() for t in got)
    ang, dt = IO.pose_error(pose[0], sc["pose"])
    print(f"register_scans(init='global'): winner {int(winner[0])}, cost {cost[0]:.8f}, {np.rad2deg(ang):.4f} deg, {100 * dt:.3f} cm, "
          f"pairs {int(pairs[0])}, iters {int(iters[0])}")
    assert pose.shape == (1, 4, 4) and winner.dtype == np.int32 and ang <= FO.BOUND_ROT and dt <= FO.BOUND_T
    direct = ops.global_register(src, tgt, S["feature_radius"], S["max_dist"], normals_radius=S["normals_radius"], k=S["k"],
                                 hypotheses=S["hypotheses"], keep=S["keep"], top=S["top"], mutual=S["mutual"], seed=S["seed"],
                                 edge_ratio=S["edge_ratio"], source_viewpoint=sv, target_viewpoint=tv, max_iters=S["max_iters"])
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(got, direct))
    # the steps on the device, then the oracle's tail on the device's hypotheses
    n_s = ops.estimate_normals(src, S["normals_radius"], S["k"], sv)[0]
    n_t = ops.estimate_normals(tgt, S["normals_radius"], S["k"], tv)[0]
    f_s, f_t = ops.fpfh(src, n_s, S["feature_radius"], S["k"]), ops.fpfh(tgt, n_t, S["feature_radius"], S["k"])
    assert np.array_equal(_bits(f_s.cpu().numpy()), _bits(FO.fpfh(sc["source"], n_s.cpu().numpy(), S["feature_radius"], S["k"])))
    idx = ops.feature_match(f_s, f_t)[0].cpu().numpy()
    assert np.array_equal(idx, FO.feature_match(f_s.cpu().numpy(), f_t.cpu().numpy())[0])
    sel = np.flatnonzero(idx >= 0)
    hp, hc, order = ops.ransac_poses(_t(sc["source"][sel], dev), _t(sc["target"][idx[sel]], dev), S["max_dist"], S["hypotheses"], S["edge_ratio"],
                                     S["seed"])
    kept = FO.rank(hc.cpu().numpy())[:S["keep"]]
    assert np.array_equal(order.cpu().numpy()[:S["keep"]], kept)
    want = FO.refine(sc["source"], sc["target"], hp.cpu().numpy()[kept], normals_radius=S["normals_radius"])
    picks = kept[want["order"][:S["top"]]]
    low = picks[want["fine"] <= want["fine"].min() * (1.0 + 1e-6)]
    print(f"oracle tail: candidates {picks.tolist()}, costs {want['fine'].tolist()}, winner {int(kept[want['winner']])}")
    assert int(winner[0]) in low.tolist()
    assert abs(cost[0] - want["cost"]) <= 1e-6 * want["cost"]
    oang, odt = IO.pose_error(pose[0], want["pose"])
    assert oang < 1e-5 and odt < 1e-4, (oang, odt)
