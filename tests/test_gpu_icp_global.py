"""The global start of the semantic ICP on the MI355X: pn_part_moments, pn_icp_seed_poses and pn_icp_score_poses against the
NumPy oracle (tests/icp_global_oracle.py), their reproducibility (eager, graph replay, batch against single scans), and
ops.global_pose / PointNet.predict_pose(init="global") end to end on the cases tests/test_cpu_icp_global.py asserts the oracle
pipeline on."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers
import icp_global_oracle as GO
import icp_mesh_oracle as MO
import icp_oracle as IO

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 4096
PAT = 0xA5
NP = len(helpers.F15_PARTS)
NM = len(MO.MESH_PARTS)


def _guarded(shape, dtype, dev):
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((GUARD + n + GUARD,), PAT, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + n].view(dtype).view(*shape)


def _intact(buf):
    return bool((buf[:GUARD] == PAT).all()) and bool((buf[-GUARD:] == PAT).all())


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint8)


def _pose(R, t):
    P = np.eye(4)
    P[:3, :3] = R
    P[:3, 3] = t
    return P


def _spoil(rng, scan, lab, n_parts):
    """labels of -1 and out of range, NaN and inf coordinates, on rows other than the first"""
    N = scan.shape[1]
    if N < 60:
        return
    for b in range(scan.shape[0]):
        k = 1 + rng.choice(N - 1, 12, replace=False)
        lab[b, k[:3]] = -1
        lab[b, k[3:5]] = n_parts
        lab[b, k[5]] = 99
        scan[b, k[6:8]] = np.nan
        scan[b, k[8], 1] = np.nan
        scan[b, k[9], 2] = np.inf
        scan[b, k[10], 0] = -np.inf


# ---------------------------------------------------------------------------------------------------------------------
# pn_part_moments
# ---------------------------------------------------------------------------------------------------------------------
def _raw_moments(dev, scan, lab, n_parts):
    from pointcloudprocessing_amd import _lib
    B, N, _ = scan.shape
    s, l = _t(scan, dev), _t(lab, dev)
    nbytes = _lib.lib().pn_part_moments_workspace_bytes(B, N)
    out, ws = _guarded((B, n_parts, 4), torch.float64, dev), _guarded((nbytes,), torch.uint8, dev)
    _lib.check(_lib.lib().pn_part_moments(_lib.ptr(s), _lib.ptr(l), B, N, n_parts, C.c_void_p(out[1].data_ptr()),
                                          C.c_void_p(ws[1].data_ptr()), nbytes, _lib.current_stream()), "pn_part_moments")
    torch.cuda.synchronize()
    assert _intact(out[0]) and _intact(ws[0]), "guard band overwritten"
    assert np.array_equal(_bits(s), scan.view(np.uint8)) and np.array_equal(_bits(l), lab.view(np.uint8)), "an input was modified"
    return out[1].cpu().numpy()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [1, 700, 2500])
def test_part_moments(dev, B, N):
    rng = np.random.default_rng(100 * B + N)
    n_parts = 7
    lab = rng.integers(0, n_parts, (B, N)).astype(np.int32)
    # integer-valued coordinates up to 2^20: every fp64 partial sum is an integer below 2^53, exact in any order
    scan = rng.integers(-(1 << 20), (1 << 20) + 1, (B, N, 3)).astype(F32)
    _spoil(rng, scan, lab, n_parts)
    got, exp = _raw_moments(dev, scan, lab, n_parts), GO.part_moments(scan, lab, n_parts)
    assert np.array_equal(got.view(np.uint64), exp.view(np.uint64))
    if N >= 700:
        assert (exp[:, :, 0] > 0).all() and exp[:, :, 0].sum() < B * N           # every part present, some points dropped
    # real-valued coordinates: 1e-13 relative to the sum of the magnitudes
    scan = (rng.normal(size=(B, N, 3)) * 30 + 50).astype(F32)
    _spoil(rng, scan, lab, n_parts)
    got, exp = _raw_moments(dev, scan, lab, n_parts), GO.part_moments(scan, lab, n_parts)
    mag = GO.part_moments(np.abs(scan), lab, n_parts)
    assert np.array_equal(got[..., 0], exp[..., 0])
    assert (np.abs(got - exp) <= 1e-13 * mag).all(), float((np.abs(got - exp) / np.maximum(mag, 1e-300)).max())
    # 16 parts, one of them absent from the scan
    lab16 = rng.integers(0, 15, (B, N)).astype(np.int32)
    got16 = _raw_moments(dev, scan, lab16, 16)
    exp16 = GO.part_moments(scan, lab16, 16)
    assert np.array_equal(got16[..., 0], exp16[..., 0]) and (got16[:, 15] == 0).all()
    assert (np.abs(got16 - exp16) <= 1e-13 * GO.part_moments(np.abs(scan), lab16, 16)).all()


def test_part_moments_of_references(dev):
    from pointcloudprocessing_amd import ops
    xyz, part, ref, seg = GO.kc46(NP)
    r = ops.icp_reference(xyz, part, NP, device=dev)
    got, exp = ops.icp_part_moments(r).cpu().numpy(), GO.ref_moments_cloud(ref, seg, NP)
    assert np.array_equal(got[:, 0], exp[:, 0]) and (np.abs(got - exp) <= 1e-13 * GO.ref_moments_cloud(np.abs(ref), seg, NP)).all()
    v, f, p = MO.aircraft_mesh(1)
    m = ops.icp_mesh_reference(v, f, p, NM, device=dev)
    tri, mseg, _, _, area = MO.group_mesh(v, f, p, NM)
    got, exp = ops.icp_part_moments(m).cpu().numpy(), GO.ref_moments_mesh(tri, mseg, area, NM)
    assert np.abs(got - exp).max() <= 1e-12 * np.abs(exp).max()


# ---------------------------------------------------------------------------------------------------------------------
# pn_icp_seed_poses
# ---------------------------------------------------------------------------------------------------------------------
def _seed_case(rng):
    """six scans against one reference of 8 parts whose part 5 is empty: 5 shared labels, 3, 2, 1, none, and one whose only
    label is the reference's empty part"""
    n_parts = 8
    cen = rng.normal(size=(n_parts, 3)) * 12
    w = rng.integers(5, 200, n_parts).astype(np.float64)
    rmom = np.concatenate([w[:, None], cen * w[:, None]], 1)
    rmom[5] = 0.0
    mom = np.zeros((6, n_parts, 4))
    for b, labs in enumerate(([0, 1, 2, 3, 5, 7], [2, 4, 5, 6], [1, 5, 6], [3], [], [5])):
        T = _pose(IO.rot(rng.normal(size=3), rng.uniform(0.2, 3.0)), rng.normal(size=3) * 25)
        for l in labs:
            n = float(rng.integers(3, 400))
            c = T[:3, :3] @ cen[l] + T[:3, 3] + rng.normal(size=3) * 0.3
            mom[b, l] = [n, *(n * c)]
    return mom, rmom


@pytest.mark.parametrize("K", [0, 1, 70])
def test_seed_poses(dev, K):
    from pointcloudprocessing_amd import ops
    mom, rmom = _seed_case(np.random.default_rng(5))
    rot = GO.rotation_grid(K) if K else None
    got = ops.icp_seed_poses(_t(mom, dev), _t(rmom, dev), _t(rot, dev) if K else None).cpu().numpy()
    exp = GO.seed_poses(mom, rmom, rot)
    assert got.shape == exp.shape == (6, K + 1, 4, 4)
    assert np.array_equal(got[:, :, 3], np.broadcast_to([0, 0, 0, 1.0], (6, K + 1, 4)))
    assert np.abs(got[:, :K] - exp[:, :K]).max(initial=0.0) < 1e-12
    # pose K: the bound tests/test_gpu_semantic_icp.py holds pn_icp_solve to against the same oracle solve
    assert np.abs(got[:, K] - exp[:, K]).max() < 1e-12, np.abs(got[:, K] - exp[:, K]).max((1, 2))
    shared = ((mom[:, :, 0] > 0) & (rmom[None, :, 0] > 0)).sum(1)
    assert shared.tolist() == [5, 3, 2, 1, 0, 0]
    for b in range(6):
        R = got[b, K, :3, :3]
        if shared[b] >= 3:
            assert np.abs(R - np.eye(3)).max() > 1e-2 and abs(np.linalg.det(R) - 1) < 1e-12
        else:
            assert np.array_equal(R, np.eye(3))                      # fewer than 3 shared labels: [I | c_s - c_r]
        if shared[b] == 0:
            assert np.array_equal(got[b, :, :3, 3], np.zeros((K + 1, 3)))    # no shared label: both centroids are 0


# ---------------------------------------------------------------------------------------------------------------------
# pn_icp_score_poses
# ---------------------------------------------------------------------------------------------------------------------
def _raw_score(dev, scan, lab, ref, seg, n_parts, poses, stride, max_d2):
    from pointcloudprocessing_amd import _lib
    B, N, _ = scan.shape
    K, M = poses.shape[1], ref.shape[0]
    ins = [_t(scan, dev), _t(lab, dev), _t(ref, dev), _t(poses, dev)]
    keep = [x.clone() for x in ins]
    nbytes = _lib.lib().pn_icp_score_workspace_bytes(B, N, K)
    bufs = dict(score=_guarded((B, K, 2), torch.float64, dev), order=_guarded((B, K), torch.int32, dev),
                ws=_guarded((nbytes,), torch.uint8, dev))
    p = lambda k: C.c_void_p(bufs[k][1].data_ptr())                                   # noqa: E731
    seg_c = (C.c_int32 * len(seg))(*[int(v) for v in seg])
    _lib.check(_lib.lib().pn_icp_score_poses(_lib.ptr(ins[0]), _lib.ptr(ins[1]), B, N, _lib.ptr(ins[2]), seg_c, M, n_parts,
                                             _lib.ptr(ins[3]), K, stride, float(max_d2), p("score"), p("order"), p("ws"), nbytes,
                                             _lib.current_stream()), "pn_icp_score_poses")
    torch.cuda.synchronize()
    for name, (buf, _) in bufs.items():
        assert _intact(buf), f"{name}: guard band overwritten"
    for a, b in zip(keep, ins):
        assert np.array_equal(_bits(a), _bits(b)), "an input was modified"
    return bufs["score"][1].cpu().numpy(), bufs["order"][1].cpu().numpy()


@pytest.fixture(scope="module")
def score_refs():
    """kc-46 (M = 490), and the same cloud without its engines: a reference with an empty segment the scans still carry"""
    xyz, part, ref, seg = GO.kc46(NP)
    eng = helpers.F15_PARTS.index("engine")
    assert (part == eng).any()
    ref2, seg2, _ = IO.group_reference(xyz[part != eng], part[part != eng], NP)
    assert seg2[eng + 1] == seg2[eng]
    return dict(full=(ref, seg), gap=(ref2, seg2)), xyz, part


def _score_case(xyz, part, B, N, K, seed):
    """scans of kc-46 under a pose each; candidates: the first ones the truth disturbed a little more each (separated costs),
    the rest random rotations about the truth's translation, one of them NaN"""
    rng = np.random.default_rng(seed)
    scans, labs, poses = [], [], []
    for b in range(B):
        T = _pose(IO.rot(rng.normal(size=3), rng.uniform(0, 3)), rng.normal(size=3) * 20)
        s, lab = IO.labelled_scan(xyz, part, max(N, 64), T, noise=0.1, outliers=0.0, seed=seed + b)
        scans.append(s[:N])
        labs.append(lab[:N])
        P = []
        for k in range(K):
            if k < 8:
                P.append(_pose(IO.rot([1, 2 - k, 0.5 * k], 0.02 * (k + 1)) @ T[:3, :3], T[:3, 3] + 0.15 * (k + 1)))
            else:
                P.append(_pose(IO.rot(rng.normal(size=3), rng.uniform(0, np.pi)), T[:3, 3] + rng.normal(size=3)))
        poses.append(np.stack(P))
    scan, lab, poses = np.stack(scans).copy(), np.stack(labs).copy(), np.stack(poses)
    _spoil(rng, scan, lab, NP)
    if K >= 2:
        poses[0, K - 1, 1, 2] = np.nan
    return scan, lab, poses


def _check_score(dev, scan, lab, ref, seg, poses, stride, max_d2):
    B, K = poses.shape[:2]
    score, order = _raw_score(dev, scan, lab, ref, seg, NP, poses, stride, max_d2)
    oscore, oorder = GO.score_poses(scan, lab, ref, seg, NP, poses, stride, max_d2)
    assert np.array_equal(score[..., 0], oscore[..., 0]), np.argwhere(score[..., 0] != oscore[..., 0])[:5]
    assert (np.abs(score[..., 1] - oscore[..., 1]) <= 1e-12 * np.abs(oscore[..., 1])).all()
    assert np.array_equal(order, np.argsort(score[..., 1], axis=1, kind="stable"))
    for b in range(B):
        c = oscore[b, oorder[b], 1]
        sep = np.ones(K + 1, bool)                                           # sep[i]: candidates i - 1 and i are separated
        sep[1:K] = np.diff(c) > 1e-9 * c[1:]
        clear = sep[:-1] & sep[1:]
        assert np.array_equal(order[b][clear], oorder[b][clear])
        assert clear[:min(K, 4)].all(), c[:5]                                # the first four stand apart
    return score, oscore


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("K", [1, 5, 37, 256])
@pytest.mark.parametrize("N", [1, 63, 700])
@pytest.mark.parametrize("B", [1, 3])
def test_score_poses(dev, score_refs, B, N, K, stride):
    refs, xyz, part = score_refs
    ref, seg = refs["full"]
    scan, lab, poses = _score_case(xyz, part, B, N, K, seed=1000 * B + 10 * N + K + stride)
    # a threshold many sampled points sit near: the median distance of the sample under the fourth-best kind of candidate
    d2 = IO.correspond(scan, lab, ref, seg, NP, poses[:, min(3, K - 1)].astype(F32))[1]
    max_d2 = F32(np.median(d2[np.isfinite(d2)])) if N > 1 else F32(4.0) * d2[np.isfinite(d2)].max()
    score, oscore = _check_score(dev, scan, lab, ref, seg, poses, stride, max_d2)
    if N >= 700:
        inl = oscore[0, min(3, K - 1), 0]
        n_s = len(GO.sample(scan[0], lab[0], seg, NP, stride))
        assert 0.2 * n_s < inl < 0.8 * n_s                                   # the threshold cuts through the sample
    if K >= 2:                                                               # the NaN pose: every sampled point at max_d2
        n_s = len(GO.sample(scan[0], lab[0], seg, NP, stride))
        assert score[0, K - 1, 0] == 0 and abs(score[0, K - 1, 1] - float(max_d2) * n_s) <= 1e-12 * float(max_d2) * n_s
    if K == 1 and stride == 1:                                               # consistent with icp_correspond's d2 at that pose
        from pointcloudprocessing_amd import ops
        r = ops.icp_reference(xyz, part, NP, device=dev)
        gd2 = ops.icp_correspond(_t(scan, dev), _t(lab, dev), r, _t(poses[:, 0].astype(F32), dev))[1].cpu().numpy()
        act = IO.active(scan, lab, seg, NP)
        for b in range(B):
            d = gd2[b][act[b]]
            assert score[b, 0, 0] == (d <= max_d2).sum()
            cost = np.where(d <= max_d2, d, max_d2).astype(np.float64).sum()
            assert abs(score[b, 0, 1] - cost) <= 1e-12 * cost


@pytest.mark.parametrize("N,K,stride", [(63, 5, 1), (700, 37, 3), (700, 5, 1)])
def test_score_poses_reference_with_an_empty_segment(dev, score_refs, N, K, stride):
    refs, xyz, part = score_refs
    ref, seg = refs["gap"]
    scan, lab, poses = _score_case(xyz, part, 3, N, K, seed=77 + N + K)
    eng = helpers.F15_PARTS.index("engine")
    assert (lab == eng).any()                                                # the scans carry the label the reference lacks
    d2 = IO.correspond(scan, lab, ref, seg, NP, poses[:, min(3, K - 1)].astype(F32))[1]
    _check_score(dev, scan, lab, ref, seg, poses, stride, F32(np.median(d2[np.isfinite(d2)])))


def test_score_poses_ops_wrapper_and_mesh_vertices(dev):
    from pointcloudprocessing_amd import ops
    v, f, p = MO.aircraft_mesh(1)
    m = ops.icp_mesh_reference(v, f, p, NM, device=dev)
    tri, mseg, _, _, _ = MO.group_mesh(v, f, p, NM)
    T = _pose(IO.rot([0.2, 1, -0.4], 2.0), [5.0, -20.0, 12.0])
    scan, lab = MO.mesh_scan(v, f, p, 900, T, noise=0.05, seed=4)
    poses = np.stack([_pose(IO.rot([1, 0, k], 0.03 * k) @ T[:3, :3], T[:3, 3] + 0.1 * k) for k in range(6)])[None]
    score, order = ops.icp_score_poses(_t(scan[None], dev), _t(lab[None], dev), m, _t(poses, dev), 2.0, stride=2)
    oscore, oorder = GO.score_poses(scan[None], lab[None], tri.reshape(-1, 3), mseg * 3, NM, poses, 2, GO.max_d2_of(2.0))
    assert np.array_equal(score.cpu().numpy()[..., 0], oscore[..., 0]) and np.array_equal(order.cpu().numpy(), oorder)
    assert (np.abs(score.cpu().numpy()[..., 1] - oscore[..., 1]) <= 1e-12 * oscore[..., 1]).all()


# ---------------------------------------------------------------------------------------------------------------------
# reproducibility: eager, graph replay, batch against single scans
# ---------------------------------------------------------------------------------------------------------------------
def test_reproducibility_graph_and_batch(dev, score_refs):
    from pointcloudprocessing_amd import ops
    refs, xyz, part = score_refs
    r = ops.icp_reference(xyz, part, NP, device=dev)
    scan, lab, poses = _score_case(xyz, part, 3, 2500, 37, seed=9)
    S, L, rot = _t(scan, dev), _t(lab, dev), _t(GO.rotation_grid(36), dev)
    rmom = ops.icp_part_moments(r)

    def run(s, l):
        mom = ops.part_moments(s, l, NP)
        seeds = ops.icp_seed_poses(mom, rmom, rot)
        score, order = ops.icp_score_poses(s, l, r, seeds, 2.5, stride=3)
        return mom, seeds, score, order

    a, b = run(S, L), run(S, L)
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x), _bits(y))
    for i in range(3):
        single = run(S[i:i + 1].contiguous(), L[i:i + 1].contiguous())
        for x, y in zip(a, single):
            assert np.array_equal(_bits(x[i:i + 1]), _bits(y))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(S, L)                                                             # warm-up on the capture stream
        with torch.cuda.graph(g, stream=side):
            captured = run(S, L)
    torch.cuda.current_stream().wait_stream(side)
    for t in captured:
        t.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(a, captured):
        assert np.array_equal(_bits(x), _bits(y))


# ---------------------------------------------------------------------------------------------------------------------
# ops.global_pose end to end
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kc46_ref(dev):
    from pointcloudprocessing_amd import ops
    xyz, part, _, _ = GO.kc46(NP)
    return ops.icp_reference(xyz, part, NP, device=dev)


@pytest.mark.parametrize("seed,one_sided", GO.CASES)
def test_global_pose_end_to_end(dev, kc46_ref, seed, one_sided):
    """the oracle pipeline's top-4 set and winner, its pose within the bound tests/test_gpu_semantic_icp.py holds the loop to
    against its oracle (1e-5 rad, 1e-4 m), and the truth within 1e-2 rad and 5e-2 m"""
    from pointcloudprocessing_amd import ops
    scan, lab, T = GO.case(seed, one_sided, NP)
    o = GO.solved(seed, one_sided, NP)
    S, L = _t(scan[None], dev), _t(lab[None], dev)
    pose, rmse, pairs, iters, status, cost, winner = ops.global_pose(S, L, kc46_ref, GO.MAX_DIST, rotations=ops.rotation_grid(256),
                                                                     **GO.PARAMS)
    assert tuple(pose.shape) == (1, 4, 4) and pose.dtype == torch.float64 and winner.dtype == torch.int32 and cost.dtype == torch.float64
    # the coarse stage on its own: the same first four
    seeds = ops.icp_seed_poses(ops.part_moments(S, L, NP), ops.icp_part_moments(kc46_ref), ops.rotation_grid(256).to(dev))
    _, order = ops.icp_score_poses(S, L, kc46_ref, seeds, GO.MAX_DIST, stride=GO.PARAMS["stride"])
    assert sorted(order[0, :4].tolist()) == sorted(o["top"][0].tolist())
    g = pose.cpu().numpy()[0]
    ang, dt = IO.pose_error(g, o["pose"][0])
    tang, tdt = IO.pose_error(g, T)
    print(f"seed {seed} one-sided {one_sided}: winner {int(winner[0])} (oracle {int(o['winner'][0])}), against the oracle {ang:.3e} rad "
          f"{dt:.3e} m, against the truth {tang:.3e} rad {tdt:.3e} m, cost {float(cost[0]):.6f} (oracle {o['cost'][0]:.6f})")
    assert int(winner[0]) == int(o["winner"][0])
    assert ang < 1e-5 and dt < 1e-4, (ang, dt)
    assert tang < GO.CAP_ROT and tdt < GO.CAP_T, (tang, tdt)
    assert (int(status[0]) & ~IO.CONVERGED) == 0
    if (seed, one_sided) == (1, False):
        # the case the feature exists for: a true rotation of 171 degrees; the local solver from [I | c_s - c_r] stays far away
        eye = ops.icp_seed_poses(ops.part_moments(S, L, NP), ops.icp_part_moments(kc46_ref), torch.eye(3, dtype=torch.float64, device=dev)[None])
        assert np.array_equal(eye[0, 0, :3, :3].cpu().numpy(), np.eye(3))
        local = ops.semantic_icp(S, L, kc46_ref, eye[:, 0].contiguous(), max_iters=GO.PARAMS["max_iters"], max_dist=GO.MAX_DIST)[0]
        lang, ldt = IO.pose_error(local.cpu().numpy()[0], T)
        assert not (lang < GO.CAP_ROT and ldt < GO.CAP_T), (lang, ldt)


def test_global_pose_batch_matches_single_scans(dev, kc46_ref):
    from pointcloudprocessing_amd import ops
    cases = [(1, False), (3, True), (5, False)]
    scan = np.stack([GO.case(s, o, NP)[0] for s, o in cases])
    lab = np.stack([GO.case(s, o, NP)[1] for s, o in cases])
    rot = ops.rotation_grid(256)
    out = ops.global_pose(_t(scan, dev), _t(lab, dev), kc46_ref, GO.MAX_DIST, rotations=rot, **GO.PARAMS)
    for i in range(3):
        one = ops.global_pose(_t(scan[i:i + 1], dev), _t(lab[i:i + 1], dev), kc46_ref, GO.MAX_DIST, rotations=rot, **GO.PARAMS)
        for x, y in zip(out, one):
            assert np.array_equal(_bits(x[i:i + 1]), _bits(y))
    with pytest.raises(ops._lib.PointNetHipError, match="max_dist"):
        ops.global_pose(_t(scan, dev), _t(lab, dev), kc46_ref, float("inf"))


def test_global_pose_mesh_plane(dev):
    """the synthetic labelled aircraft mesh turned by 120 degrees: global_pose against the mesh, point to plane"""
    from pointcloudprocessing_amd import ops
    v, f, p = MO.aircraft_mesh(1)
    m = ops.icp_mesh_reference(v, f, p, NM, device=dev)
    tri, mseg, _, nrm, area = MO.group_mesh(v, f, p, NM)
    T = _pose(IO.rot([0.5, -1.0, 0.7], np.deg2rad(120)), [14.0, -6.0, 25.0])
    scan, lab = MO.mesh_scan(v, f, p, 1000, T, noise=0.02, seed=3)
    kw = dict(top=4, stride=1, max_iters=15, metric="plane")
    rot = GO.rotation_grid(64)
    o = GO.global_pose(scan[None], lab[None], None, None, NM, 2.0, rotations=rot, mesh=(tri, mseg, nrm, area), **kw)
    pose, _, _, _, _, cost, winner = ops.global_pose(_t(scan[None], dev), _t(lab[None], dev), m, 2.0, rotations=_t(rot, dev), **kw)
    g = pose.cpu().numpy()[0]
    tang, tdt = IO.pose_error(g, T)
    oang, odt = IO.pose_error(o["pose"][0], T)
    print(f"mesh, plane: winner {int(winner[0])} (oracle {int(o['winner'][0])}), truth {tang:.3e} rad {tdt:.3e} m (oracle {oang:.3e} "
          f"{odt:.3e}), cost {float(cost[0]):.6f} (oracle {o['cost'][0]:.6f})")
    assert int(winner[0]) == int(o["winner"][0])
    assert tang < GO.CAP_ROT and tdt < GO.CAP_T and oang < GO.CAP_ROT and odt < GO.CAP_T


# ---------------------------------------------------------------------------------------------------------------------
# PointNet.predict_pose
# ---------------------------------------------------------------------------------------------------------------------
def test_predict_pose_global_and_default(dev, kc46_ref, monkeypatch):
    from oracle import pointnet_oracle as O            # checker only
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd.pointnet.PointNet import PointNet
    model = PointNet(23, 12, 0.3, 42, precision="bf16", device=dev)
    model.set_weights(O.init_params(23, 12, seed=31, randomize_bn=True))
    scan, lab, T = GO.case(1, False, NP)
    x = _t(scan, dev)
    # init=None: what it returns on the parent commit, predict_scan -> initial_pose -> semantic_icp, bit for bit
    ci, part, pose, rmse, pairs = model.predict_pose(x, kc46_ref, max_iters=10)
    ci2, part2, R = model.predict_scan(x)
    P0 = PointNet.initial_pose(x, part2, R, kc46_ref)
    p2, r2, n2, _, _ = ops.semantic_icp(x.unsqueeze(0), part2, kc46_ref, P0, max_iters=10)
    assert torch.equal(ci, ci2) and torch.equal(part, part2)
    assert np.array_equal(_bits(pose), _bits(p2)) and np.array_equal(_bits(rmse), _bits(r2)) and torch.equal(pairs, n2)
    # init="global" on a labelled scan: the labels of predict_scan replaced by the scan's own
    L = _t(lab[None], dev)
    monkeypatch.setattr(model, "predict_scan", lambda *a, **k: (ci2, L, R))
    kw = dict(max_dist=GO.MAX_DIST, rotations=ops.rotation_grid(256), **GO.PARAMS)
    ci3, part3, pose3, rmse3, pairs3 = model.predict_pose(x, kc46_ref, init="global", **kw)
    gp = ops.global_pose(x.unsqueeze(0), L, kc46_ref, **kw)
    assert torch.equal(part3, L) and torch.equal(ci3, ci2)
    assert np.array_equal(_bits(pose3), _bits(gp[0])) and np.array_equal(_bits(rmse3), _bits(gp[1])) and torch.equal(pairs3, gp[2])
    ang, dt = IO.pose_error(pose3.cpu().numpy()[0], T)
    assert ang < GO.CAP_ROT and dt < GO.CAP_T
    with pytest.raises(ops._lib.PointNetHipError):
        model.predict_pose(x, kc46_ref, init="global")                       # no max_dist
    with pytest.raises(ops._lib.PointNetHipError):
        model.predict_pose(x, kc46_ref, init="nearest", max_dist=3.0)
