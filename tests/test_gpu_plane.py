"""pn_plane_segment on the MI355X against the NumPy oracle (tests/plane_oracle.py), teacher-forced per round because round r + 1
depends on round r's fp64 plane: on the active set the DEVICE's earlier labels leave, the hypothesis scores are compared bit for bit
(and with them the winner: select() of equal scores), the device's plane with the oracle's within a derived tolerance, and plane_id
exactly with label() applied to the device's own plane.  Guard bands around every output and the workspace; graph capture; the
floor-and-wall scene through ops.plane_segment and PointNet.predict_scan / predict_pose(remove_planes=...), bit for bit against the
aircraft's own scan.

The plane tolerance is 64 x the spread the oracle shows between pairwise and sequential fp64 sums on the same input (the device sums
in a third order: lanes, waves, blocks), with a floor of 1e-12.  Measured on the CPU over every case of this file the spread is at
most 2.1e-14 (test_threshold_edge on quarter-integer coordinates, 75 inliers), 1.8e-15 on the scene's wall, around 5e-16 on the random
clouds and exactly 0 on the lattice and the tiny clouds, so the floor of 1e-12 decides everywhere but on the first of these; the
device's planes differed from the oracle's by at most 1.8e-15 on the MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

import plane_oracle as PO

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 4096          # bytes of fill pattern before and after every output buffer and the workspace
PAT = 0xA5
COS10 = float(F32(np.cos(np.radians(10.0))))


def _guarded(nbytes, dev):
    buf = torch.full((GUARD + nbytes + GUARD,), PAT, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + nbytes]


def _raw(x, threshold, H, P, min_inliers=3, seed=0, axis=None, cos=1.0, want_hyp=True):
    """pn_plane_segment on guard-banded outputs and workspace -> (planes (P, 4), counts (P,), plane_id (N,), hyp_counts (P, H) or None);
    asserts that the bands and the input are untouched"""
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    N = x.shape[0]
    dev = x.device
    keep = x.clone()
    nbytes = L.pn_plane_segment_workspace_bytes(N, H, P)
    assert nbytes > 0
    bufs = {name: _guarded(n, dev) for name, n in (("planes", 32 * P), ("counts", 4 * P), ("id", 4 * N), ("hyp", 4 * P * H), ("ws", nbytes))}
    p = lambda name: C.c_void_p(bufs[name][1].data_ptr())      # noqa: E731
    ax3 = (C.c_float * 3)(*[float(v) for v in axis]) if axis is not None else None
    rc = L.pn_plane_segment(_lib.ptr(x), N, float(threshold), H, P, int(min_inliers), int(seed), ax3, float(cos), p("planes"), p("counts"), p("id"),
                            p("hyp") if want_hyp else None, p("ws"), nbytes, _lib.current_stream())
    _lib.check(rc, "pn_plane_segment")
    torch.cuda.synchronize()
    for name, (buf, _) in bufs.items():
        assert bool((buf[:GUARD] == PAT).all()) and bool((buf[-GUARD:] == PAT).all()), f"{name}: guard band overwritten"
    assert torch.equal(keep.view(torch.int32), x.view(torch.int32)), "the input was modified"
    if not want_hyp:
        assert bool((bufs["hyp"][1] == PAT).all())
    return (bufs["planes"][1].view(torch.float64).reshape(P, 4).cpu().numpy(), bufs["counts"][1].view(torch.int32).cpu().numpy(),
            bufs["id"][1].view(torch.int32).cpu().numpy(), bufs["hyp"][1].view(torch.int32).reshape(P, H).cpu().numpy() if want_hyp else None)


def _check(dev, xyz, threshold, H, P, min_inliers=3, seed=0, axis=None, cos=1.0):
    """the teacher-forced comparison -> (planes, counts, plane_id, hyp_counts, rounds that produced a plane)"""
    xyz = np.ascontiguousarray(xyz, F32)
    planes, counts, pid, hyp = _raw(torch.from_numpy(xyz).to(dev), threshold, H, P, min_inliers, seed, axis, cos)
    assert pid.min() >= -1 and pid.max() < P
    finite = PO.active_rows(xyz)
    stopped, found = False, 0
    for r in range(P):
        if not stopped:
            active = finite & ~((pid >= 0) & (pid < r))                    # what the device's earlier labels leave
            hc, win, plane, mask = PO.round(xyz, active, r, threshold, H, seed, axis, cos)
            if hc is None:
                stopped = True
            else:
                assert np.array_equal(hyp[r], hc), (r, np.flatnonzero(hyp[r] != hc)[:5], hyp[r][hyp[r] != hc][:5], hc[hyp[r] != hc][:5])
                if win < 0 or int(mask.sum()) < min_inliers:
                    stopped = True                                          # no valid hypothesis, or a void round: scored, nothing else
                    assert counts[r] == 0 and not planes[r].any() and not (pid == r).any(), (r, counts[r], planes[r])
                    continue
                spread = PO.order_spread(xyz, active, r, threshold, H, seed, axis, cos)
                tol = max(64.0 * spread, 1e-12)
                print(f"round {r}: M={int(active.sum())} winner={win} count={counts[r]} spread={spread:.3g} plane err={np.abs(planes[r] - plane).max():.3g}")
                assert np.abs(planes[r] - plane).max() <= tol, (r, planes[r], plane, tol)
                own = PO.label(xyz, active, planes[r], threshold)            # the device's own plane
                assert counts[r] == int(own.sum()) >= min_inliers and np.array_equal(pid == r, own), (r, counts[r], int(own.sum()))
                found += 1
                continue
        assert (hyp[r] == -1).all() and counts[r] == 0 and not planes[r].any() and not (pid == r).any(), r
    assert (pid[~finite] == -1).all()
    return planes, counts, pid, hyp, found


# ---- sizes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 63, 64, 100, 256])
@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, PO.TILE - 1, PO.TILE, PO.TILE + 1, 1000])
def test_sizes(dev, N, H):
    """a third of the points near one plane; min_inliers = 6 voids the rounds whose best plane is a skinny triple of leftovers (their
    normal is ill-conditioned: not a summation-order effect)"""
    found = _check(dev, PO.random_cloud(N, seed=N), 0.05, H, 2, min_inliers=6, seed=N + H)[4]
    if N < 3:
        assert found == 0
    if N >= 63 and H >= 63:
        assert found >= 1


def test_tiny_clouds_give_a_plane(dev):
    tri = np.array([[0, 0, 0], [1, 0, 0.25], [0, 1, -0.5], [0.25, 0.25, 3.0]], F32)
    for n in (3, 4):
        planes, counts, pid, hyp, found = _check(dev, tri[:n], 0.01, 64, 2, min_inliers=3)
        assert found == 1 and counts.tolist() == [3, 0] and pid.tolist() == [0, 0, 0, -1][:n]
        assert abs(abs(planes[0][:3] @ np.array([-0.25, 0.5, 1.0]) / np.sqrt(1.3125)) - 1.0) < 1e-12


def test_hyp_counts_is_optional(dev):
    x = PO.random_cloud(777, seed=4)
    full = _raw(torch.from_numpy(x).to(dev), 0.05, 100, 2)
    part = _raw(torch.from_numpy(x).to(dev), 0.05, 100, 2, want_hyp=False)
    assert part[3] is None and all(np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b)
                                   for a, b in zip(full[:3], part[:3]))


# ---- exact arithmetic, ties, the edge of the threshold ---------------------------------------------------------------------
@pytest.mark.parametrize("threshold", [1.0, 0.5])
def test_integer_lattice(dev, threshold):
    x = PO.lattice()
    planes, counts, pid, hyp, found = _check(dev, x, threshold, 256, 3, min_inliers=20)
    exact = PO.lattice_counts_exact(x, PO.hypotheses(x, np.ones(len(x), bool), 0, 256, threshold))(*((1, 1) if threshold == 1.0 else (1, 4)))
    assert np.array_equal(hyp[0], exact) and found >= 1
    assert len(np.unique(hyp[0])) < 100 and (threshold != 1.0 or (hyp[0] == hyp[0].max()).sum() >= 2)      # ties everywhere, the best included


@pytest.mark.parametrize("lattice_base", [True, False])
def test_threshold_edge(dev, lattice_base):
    x, used = PO.threshold_edge(0.25, 64, lattice_base=lattice_base)
    hyp = PO.hypotheses(x, np.ones(len(x), bool), 0, 64, 0.25)
    adv = x[200:]
    verdicts = np.stack([PO.inliers(adv, hyp["p0"][h], hyp["c"][h], hyp["t2"][h]) for h in used])
    own = np.stack([verdicts[i, 34 * i:34 * (i + 1)] for i in range(len(used))])                # each hypothesis's own 2 x 17 points
    assert own.any(1).all() and (~own).any(1).all(), "the adversarial rows must straddle the threshold"
    _check(dev, x, 0.25, 64, 1, min_inliers=6)


# ---- bad rows, duplicates, the stop rules --------------------------------------------------------------------------------
def test_non_finite_rows(dev):
    from pointcloudprocessing_amd import ops
    x = PO.random_cloud(1500, seed=8)
    bad = [0, 1, 750, 1023, 1024, 1499]
    x[bad] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan], [np.inf, 0, np.nan], [0, -np.inf, 0]]
    planes, counts, pid, hyp, found = _check(dev, x, 0.05, 128, 2, min_inliers=6)
    assert found >= 1 and (pid[bad] == -1).all()
    good = np.setdiff1d(np.arange(1500), bad)
    clean = _check(dev, x[good], 0.05, 128, 2, min_inliers=6)                               # never drawn: the same draws as without them
    assert np.array_equal(clean[3], hyp) and np.array_equal(clean[2], pid[good]) and np.array_equal(clean[0].view(np.int64), planes.view(np.int64))
    o = ops.plane_segment(torch.from_numpy(x).to(dev), 0.05, max_planes=2, hypotheses=128, min_inliers=6, return_hypotheses=True)
    assert np.array_equal(o[2].cpu().numpy(), pid) and np.array_equal(o[3].cpu().numpy(), hyp) and np.array_equal(o[1].cpu().numpy(), counts)
    assert np.array_equal(o[0].cpu().numpy().view(np.int64), planes.view(np.int64))
    assert np.array_equal(ops.plane_mask(o[2]).cpu().numpy(), pid < 0)
    none = ops.plane_segment(torch.full((5, 3), float("nan"), device=dev), 0.05, max_planes=2, hypotheses=16, return_hypotheses=True)
    assert none[2].tolist() == [-1] * 5 and not none[0].any() and not none[1].any() and bool((none[3] == -1).all())


def test_duplicated_points(dev):
    x = np.repeat(PO.random_cloud(60, seed=12), 20, axis=0)
    x = x[np.random.default_rng(0).permutation(len(x))]
    planes, counts, pid, hyp, found = _check(dev, x, 0.05, 128, 2, min_inliers=6)
    assert found >= 1 and (hyp[0] == -1).sum() > 0                       # a triple of copies of one point spans nothing
    same = _check(dev, np.repeat(np.array([[1.5, -2.0, 0.25]], F32), 100, axis=0), 0.05, 64, 2)
    assert same[4] == 0 and (same[3][0] == -1).all()


def test_collinear_cloud_stops(dev):
    planes, counts, pid, hyp, found = _check(dev, PO.collinear(), 0.5, 128, 3)
    assert found == 0 and not planes.any() and not counts.any() and (pid == -1).all() and (hyp == -1).all()


def test_min_inliers_above_the_best_count_voids_the_round(dev):
    x, tag = PO.floor_and_wall()
    planes, counts, pid, hyp, found = _check(dev, x, 0.03, 128, 3, min_inliers=5000)
    assert found == 0 and not planes.any() and not counts.any() and (pid == -1).all() and hyp[0].max() > 1000 and (hyp[1:] == -1).all()
    planes, counts, pid, hyp, found = _check(dev, x, 0.03, 128, 3, min_inliers=1000)
    assert found == 2 and counts[2] == 0 and not planes[2].any() and hyp[2].max() > 0 and set(np.unique(pid)) == {-1, 0, 1}


def test_axis_constraint(dev):
    from pointcloudprocessing_amd import ops
    x, tag = PO.floor_and_wall()
    xd = torch.from_numpy(x).to(dev)
    free = PO.hypotheses(x, np.ones(len(x), bool), 0, 128, 0.03)["valid"]
    for axis, want in (((0.0, 0.0, 1.0), 0), ((1.0, 0.0, 0.0), 1), ((0.0, 0.0, -2.5), 0)):
        planes, counts, pid, hyp, found = _check(dev, x, 0.03, 128, 1, axis=axis, cos=COS10)
        valid = PO.hypotheses(x, np.ones(len(x), bool), 0, 128, 0.03, axis=axis, cos_max_angle=COS10)["valid"]
        assert np.array_equal(hyp[0] == -1, ~valid) and 0 < valid.sum() < free.sum()
        unit = np.asarray(axis) / np.linalg.norm(axis)
        assert found == 1 and abs(planes[0][:3] @ unit) > 0.999 and (pid[tag == want] == 0).all() and (pid[tag == 1 - want] == 0).mean() < 0.05
        o = ops.plane_segment(xd, 0.03, hypotheses=128, axis=axis, max_angle_deg=10.0)
        assert np.array_equal(o[2].cpu().numpy(), pid) and np.array_equal(o[0].cpu().numpy().view(np.int64), planes.view(np.int64))


def test_errors_raise_through_ops(dev):
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd._lib import PointNetHipError
    x = torch.from_numpy(PO.random_cloud(100)).to(dev)
    for kw in (dict(threshold=-1.0), dict(threshold=0.1, hypotheses=0), dict(threshold=0.1, hypotheses=5000), dict(threshold=0.1, max_planes=0),
               dict(threshold=0.1, max_planes=9), dict(threshold=0.1, axis=(0, 0, 1)), dict(threshold=0.1, max_angle_deg=10.0),
               dict(threshold=0.1, axis=(0, 0, 0), max_angle_deg=10.0), dict(threshold=0.1, axis=(0, 0, 1), max_angle_deg=120.0),
               dict(threshold=0.1, seed=-1)):
        with pytest.raises(PointNetHipError):
            ops.plane_segment(x, **kw)
    with pytest.raises(PointNetHipError):
        ops.plane_segment(x.reshape(-1), 0.1)


def test_determinism_and_seeds(dev):
    x = torch.from_numpy(PO.random_cloud(3000, seed=3)).to(dev)
    a = _raw(x, 0.05, 256, 2, min_inliers=6, seed=11)
    b = _raw(x, 0.05, 256, 2, min_inliers=6, seed=11)
    assert all(np.array_equal(u.view(np.int64) if u.dtype == np.float64 else u, v.view(np.int64) if v.dtype == np.float64 else v) for u, v in zip(a, b))
    c = _raw(x, 0.05, 256, 2, min_inliers=6, seed=12)
    d = _raw(x, 0.05, 256, 2, min_inliers=6, seed=11 + (1 << 32))                           # the high word is part of the key
    assert not np.array_equal(a[3][0], c[3][0]) and not np.array_equal(a[3][0], d[3][0]) and not np.array_equal(c[3][0], d[3][0])
    assert not np.array_equal(a[3][0], a[3][1])                                             # another round: other draws, another list


def test_graph_capture_replays_on_a_second_input(dev):
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    N, H, P = 3000, 128, 2
    a, b = PO.random_cloud(N, seed=21), PO.random_cloud(N, seed=22)
    b[:, 2] += 0.5
    ea, eb = (_raw(torch.from_numpy(v).to(dev), 0.05, H, P, min_inliers=6) for v in (a, b))      # the eager calls
    assert ea[1][0] > 500 and eb[1][0] > 500 and not np.array_equal(ea[2], eb[2]) and not np.array_equal(ea[3], eb[3])
    x = torch.from_numpy(a).to(dev)
    planes = torch.zeros(P, 4, dtype=torch.float64, device=dev)
    counts = torch.zeros(P, dtype=torch.int32, device=dev)
    pid = torch.zeros(N, dtype=torch.int32, device=dev)
    hyp = torch.zeros(P, H, dtype=torch.int32, device=dev)
    nbytes = L.pn_plane_segment_workspace_bytes(N, H, P)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def call():
        _lib.check(L.pn_plane_segment(_lib.ptr(x), N, 0.05, H, P, 6, 0, None, 1.0, _lib.ptr(planes), _lib.ptr(counts), _lib.ptr(pid), _lib.ptr(hyp),
                                      _lib.ptr(ws), nbytes, _lib.current_stream()), "pn_plane_segment")

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
        for t in (counts, pid, hyp):
            t.fill_(-7)
        planes.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(planes.cpu().numpy().view(np.int64), exp[0].view(np.int64)) and np.array_equal(counts.cpu().numpy(), exp[1])
        assert np.array_equal(pid.cpu().numpy(), exp[2]) and np.array_equal(hyp.cpu().numpy(), exp[3])


# ---- the floor-and-wall scene end to end -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def floor(dev):
    from oracle import pointnet_oracle as O
    from pointcloudprocessing_amd.pointnet.PointNet import PointNet
    scene, air, fl, wall, clean = PO.floor_scene()
    model = PointNet(23, 12, 0.3, 42, precision="bf16", device=dev)
    model.set_weights(O.init_params(23, 12, seed=4, randomize_bn=True))
    t = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
    return dict(model=model, scene=t(scene), clean=t(clean), air=t(air), scene_np=scene, air_np=air, floor_np=fl, wall_np=wall,
                kw=dict(threshold=PO.SCENE["threshold"], hypotheses=PO.SCENE["hypotheses"], max_planes=PO.SCENE["max_planes"],
                        min_inliers=PO.SCENE["min_inliers"]))


def test_scene_planes_match_the_recorded_facts(dev, floor):
    from pointcloudprocessing_amd import ops
    s, S = floor["scene_np"], PO.SCENE
    planes, counts, pid, hyp, found = _check(dev, s, S["threshold"], S["hypotheses"], S["max_planes"], S["min_inliers"])
    assert found == 2 and counts[2] == 0 and not planes[2].any() and hyp[2].max() > 0                # two planes, the third round void
    assert (pid[floor["floor_np"]] >= 0).all() and (pid[floor["wall_np"]] >= 0).all() and (pid[floor["air_np"]] == -1).all()
    assert abs(planes[0][2]) > 0.999 and abs(planes[1][1]) > 0.999 and counts[:2].sum() == 9000
    o = ops.plane_segment(floor["scene"], **floor["kw"])
    assert len(o) == 3 and np.array_equal(o[2].cpu().numpy(), pid) and np.array_equal(o[0].cpu().numpy().view(np.int64), planes.view(np.int64))
    assert np.array_equal(np.flatnonzero(ops.plane_mask(o[2]).cpu().numpy()), floor["air_np"])
    # without the planes removed the largest cluster is aircraft, floor and wall in one
    cl, sz = ops.voxel_clusters(floor["scene"], PO.SCENE_CLUSTER_LEAF)
    kept = ops.cluster_mask(cl, sz).cpu().numpy()
    assert kept[floor["floor_np"]].sum() > 0 and kept.sum() > 4096


def test_predict_scan_removes_floor_and_wall(dev, floor):
    from pointcloudprocessing_amd._lib import PointNetHipError
    m, scene, clean, rows = (floor[k] for k in ("model", "scene", "clean", "air"))
    kw = dict(leaf=0.5, samples=1024, k=3, return_confidence=True)
    ci, part, R, conf = m.predict_scan(scene, remove_planes=floor["kw"], isolate="largest", cluster_leaf=PO.SCENE_CLUSTER_LEAF, **kw)
    ci0, part0, R0, conf0 = m.predict_scan(clean, **kw)
    assert tuple(part.shape) == (1, scene.shape[0]) and tuple(conf.shape) == (1, scene.shape[0]) and part.dtype == part0.dtype
    assert torch.equal(ci, ci0) and torch.equal(R.view(torch.int32), R0.view(torch.int32))
    assert torch.equal(part[0, rows], part0[0]) and torch.equal(conf[0, rows].view(torch.int32), conf0[0].view(torch.int32))
    assert bool((part0 >= 0).all()) and bool((conf0 > 0).all())
    other = torch.ones(scene.shape[0], dtype=torch.bool, device=scene.device)
    other[rows] = False
    assert int(other.sum()) == 9000 and bool((part[0, other] == -1).all()) and bool((conf[0, other] == 0).all())
    # remove_planes alone (the aircraft is all that is left), and without confidence
    out3 = m.predict_scan(scene, leaf=0.5, samples=1024, k=3, remove_planes=floor["kw"])
    assert len(out3) == 3 and torch.equal(out3[1], part)
    # isolate alone keeps the floor: another answer
    iso = m.predict_scan(scene, isolate="largest", cluster_leaf=PO.SCENE_CLUSTER_LEAF, **kw)
    assert int((iso[1][0, other] >= 0).sum()) > 6000
    # the default path is untouched: two calls agree bit for bit, with and without the keyword spelt out
    a = m.predict_scan(scene, remove_planes=None, **kw)
    b = m.predict_scan(scene, **kw)
    assert all(torch.equal(u.view(torch.int32) if u.dtype == torch.float32 else u, v.view(torch.int32) if v.dtype == torch.float32 else v)
               for u, v in zip(a, b))
    assert bool((a[1] >= 0).all())
    with pytest.raises(PointNetHipError):
        m.predict_scan(scene, remove_planes=dict(threshold=100.0, min_inliers=3), **kw)          # everything lies on one plane
    with pytest.raises(PointNetHipError):
        m.predict_scan(scene, remove_planes="floor", **kw)


def test_predict_pose_removes_floor_and_wall(dev, floor):
    import icp_mesh_oracle as MO
    import icp_plane_oracle as IPO
    from pointcloudprocessing_amd import ops
    m, scene, clean, rows = (floor[k] for k in ("model", "scene", "clean", "air"))
    v, f, p = MO.aircraft_mesh(0)
    ref = ops.icp_mesh_reference(v, f, (np.arange(len(f)) % 12).astype(np.int32), 12, device=dev)       # every part label gets triangles
    kw = dict(leaf=0.5, samples=1024, k=3, max_iters=5, max_dist=5.0)
    for extra in (dict(init=IPO.START_POSE), dict(init=IPO.START_POSE, weights="confidence", robust="tukey", metric="plane")):
        ci, part, pose, rmse, pairs = m.predict_pose(scene, ref, remove_planes=floor["kw"], isolate="largest",
                                                     cluster_leaf=PO.SCENE_CLUSTER_LEAF, **kw, **extra)
        ci0, part0, pose0, rmse0, pairs0 = m.predict_pose(clean, ref, **kw, **extra)
        assert bool(torch.isfinite(pose0).all()) and int(pairs0[0]) > 1000
        assert torch.equal(pose.view(torch.int64), pose0.view(torch.int64)) and torch.equal(rmse.view(torch.int64), rmse0.view(torch.int64))
        assert torch.equal(pairs, pairs0) and torch.equal(ci, ci0)
        assert tuple(part.shape) == (1, scene.shape[0]) and torch.equal(part[0, rows], part0[0]) and int((part[0] == -1).sum()) == 9000
