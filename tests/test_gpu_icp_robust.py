"""pn_icp_robust_sums / pn_icp_robust_solve / pn_semantic_icp_robust on the MI355X against the NumPy oracle
(tests/icp_robust_oracle.py): the scale bit for bit (the lower median is an exact order statistic), the search bit for bit against
the unweighted entries, the pairs' weights and the 19 / 30 weighted sums, the weighted solve, the loops on scans with a fifth of the
labels wrong, determinism (a batch against the single scans, eager against graph replay), the unchanged default path, and the
confidence PointNet.predict_scan returns."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import helpers
import icp_mesh_oracle as MO
import icp_oracle as IO
import icp_plane_oracle as PO
import icp_robust_oracle as RO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
F32 = np.float32
NP = len(helpers.F15_PARTS)
NM = len(MO.MESH_PARTS)
KERNELS = ("huber", "cauchy", "tukey")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


_CACHE = {}


def _kc46_case():
    """the kc-46 reference (490 points, 7 of 12 parts) with oracle normals, a few of them NaN"""
    if "kc46" not in _CACHE:
        from pointcloudprocessing_amd import pointcloud
        xyz, part = pointcloud.read_labelled_cloud(os.path.join(GOLD, "kc-46.txt"), helpers.F15_PARTS)
        xyz, part = np.asarray(xyz, F32), np.asarray(part, np.int32)
        ref, seg, _ = IO.group_reference(xyz, part, NP)
        nrm, _, _ = PO.normals(ref, seg, NP, 10)
        nrm = nrm.copy()
        nrm[::40] = np.nan
        _CACHE["kc46"] = (xyz, part, ref, seg, nrm)
    return _CACHE["kc46"]


def _mesh_case():
    if "mesh" not in _CACHE:
        v, f, p = MO.aircraft_mesh(0)
        tri, seg, _, nrm, _ = MO.group_mesh(v, f, p, NM)
        _CACHE["mesh"] = (v, f, p, tri, seg, nrm)
    return _CACHE["mesh"]


def _refs(dev, kind):
    """-> (the device reference, the oracle's reference, n_parts, a scan maker (n, seed) -> (scan, labels), the pose of the scans)"""
    from pointcloudprocessing_amd import ops
    if kind == "cloud":
        xyz, part, ref, seg, nrm = _kc46_case()
        r = ops.icp_reference(xyz, part, NP, device=dev)
        r = ops.IcpReference(r.xyz, r.seg, r.index, NP, normals=_t(nrm, dev))
        true = np.eye(4)
        true[:3, :3] = IO.rot([0.2, 1.0, -0.4], 0.9)
        true[:3, 3] = [5.0, -3.0, 12.0]
        make = lambda n, seed: IO.labelled_scan(xyz, part, n, true, noise=0.05, outliers=0.03, seed=seed)    # noqa: E731
        return r, RO.cloud(ref, seg, NP, nrm), NP, make, true
    v, f, p, tri, seg, nrm = _mesh_case()
    r = ops.icp_mesh_reference(v, f, p, NM, device=dev)
    make = lambda n, seed: MO.mesh_scan(v, f, p, n, PO.TRUE_POSE, noise=0.02, seed=seed)                     # noqa: E731
    return r, RO.mesh(tri, seg, NM, nrm), NM, make, PO.TRUE_POSE


def _near(true, seed, rot=0.03, shift=0.2):
    rng = np.random.default_rng(seed)
    P = true.copy()
    P[:3, :3] = IO.rot(rng.normal(size=3), rot) @ true[:3, :3]
    P[:3, 3] += rng.normal(size=3) * shift
    return P


# ---------------------------------------------------------------------------------------------------------------------
# the median and the scale
# ---------------------------------------------------------------------------------------------------------------------
def test_scale_is_the_lower_median_bit_for_bit(dev):
    """B = 3, N = 700 (the last block of 256 is ragged): an even kept count, an odd one with one point repeated 400 times (equal d2
    across the median rank), and a scan whose labels are all -1 (n = 0, c = min_scale)"""
    from pointcloudprocessing_amd import ops
    r, oref, n_parts, make, true = _refs(dev, "cloud")
    N, md = 700, 1.5
    scans, labs = zip(*[make(N, 11 + b) for b in range(3)])
    scan, lab = np.stack(scans).copy(), np.stack(labs).copy()
    row = int(np.flatnonzero(lab[1] >= 0)[0])
    dup = np.flatnonzero(lab[1] >= 0)[:400]
    scan[1, dup], lab[1, dup] = scan[1, row], lab[1, row]
    lab[2] = -1
    pose = np.stack([_near(true, 3 + b) for b in range(3)])
    for b, odd in ((0, 0), (1, 1)):                                            # fix the parity of the kept counts
        idx, _, _ = RO.search(scan[b:b + 1], lab[b:b + 1], oref, pose[b:b + 1].astype(F32), F32(md * md))
        if (idx >= 0).sum() % 2 != odd:
            lab[b, np.flatnonzero((idx[0] >= 0) & (np.arange(N) != row))[-1]] = -1
    free = RO.pass_sums(scan, lab, oref, pose, "point", F32(md * md), None, "tukey", "mad", 0.7, 1e-4)[4]
    floor = 0.5 * (free[0] + free[1])                                          # between the two scans' scales: it holds one of them
    for kernel in KERNELS:
        for tune, ms in ((None, 1e-4), (0.7, floor)):
            o = RO.pass_sums(scan, lab, oref, pose, "point", F32(md * md), None, kernel, "mad", tune, ms)
            g = ops.icp_robust_sums(_t(scan, dev), _t(lab, dev), r, _t(pose, dev), max_dist=md, robust=kernel, robust_tune=tune,
                                    robust_min_scale=ms)
            kept = (o[0] >= 0).sum(1)
            assert kept[0] % 2 == 0 and kept[1] % 2 == 1 and kept[0] > 300 and kept[1] > 500 and kept[2] == 0
            assert np.array_equal(_bits(g[4].cpu().numpy()), _bits(o[4])), (kernel, tune, g[4].cpu().numpy(), o[4])
            assert o[4][2] == ms
    d = np.sort(o[1][1][o[0][1] >= 0])
    k = (d.size - 1) >> 1
    assert d[k - 1] == d[k] == d[k + 1]                                        # the ties straddle the median rank
    assert sorted([o[4][0] == floor, o[4][1] == floor]) == [False, True] and max(o[4][0], o[4][1]) > floor


def test_scale_on_built_d2_patterns(dev):
    """N = 5,000 against a reference of one point at the origin, identity pose, scan points (x, 0, 0): d2 = x * x.  Scan 0: d2
    differs only in the lowest byte (x = 1 + k 2^-23); scan 1: only in the highest (x = 2^j: d2 = 4^j, the exponent moves in steps
    of two); scan 2: exact zeros up to the median rank; scan 3: all three mixed"""
    from pointcloudprocessing_amd import ops
    N = 5000
    rng = np.random.default_rng(9)
    low = (1.0 + rng.integers(0, 100, N) * 2.0 ** -23).astype(F32)
    high = (2.0 ** rng.integers(-20, 20, N)).astype(F32)
    zero = np.where(np.arange(N) < 2600, 0.0, rng.uniform(0.1, 2.0, N)).astype(F32)
    mix = np.concatenate([low[:1700], high[:1700], zero[:1600]])
    xs = np.stack([low, high, rng.permutation(zero), rng.permutation(mix)])
    scan = np.zeros((4, N, 3), F32)
    scan[:, :, 0] = xs
    lab = np.zeros((4, N), np.int32)
    lab[0, :7] = -1                                                            # an odd count
    d2 = (xs * xs).astype(F32)
    b0, b1 = _bits(d2[0][7:]), _bits(d2[1])
    assert len(np.unique(b0)) > 50 and len(np.unique(b0 >> 8)) == 1            # only the lowest byte differs
    assert len(np.unique(b1)) > 30 and len(np.unique(b1 & 0xFFFFFF)) == 1      # only the highest byte differs
    origin = np.zeros((1, 3), F32)
    r = ops.icp_reference(origin, np.zeros(1, np.int32), 1, device=dev)
    oref = RO.cloud(origin, np.array([0, 1]), 1)
    pose = np.tile(np.eye(4), (4, 1, 1))
    o = RO.pass_sums(scan, lab, oref, pose, "point", np.inf, None, "tukey", "mad", None, 1e-4)
    g = ops.icp_robust_sums(_t(scan, dev), _t(lab, dev), r, _t(pose, dev), robust="tukey")
    assert np.array_equal(_bits(g[1].cpu().numpy()), _bits(o[1])) and np.array_equal(_bits(o[1][lab >= 0]), _bits(d2[lab >= 0]))
    assert np.array_equal(_bits(g[4].cpu().numpy()), _bits(o[4])), (g[4].cpu().numpy(), o[4])
    assert o[4][2] == 1e-4 and o[4][0] > 1 and np.isfinite(o[4]).all()        # scan 2: med = 0 exactly, the floor holds


# ---------------------------------------------------------------------------------------------------------------------
# one pass: the search, the weights, the sums
# ---------------------------------------------------------------------------------------------------------------------
def _point_weights(rng, B, N):
    w = rng.uniform(0.05, 1.0, (B, N)).astype(F32)
    k = rng.choice(N, 40, replace=False)
    w[:, k[:10]] = 0.0
    w[:, k[10:20]] = -0.5
    w[:, k[20:30]] = np.nan
    w[:, k[30:35]] = np.inf
    w[:, k[35:]] = -np.inf
    return w


@pytest.mark.parametrize("kind,metric", [("cloud", "point"), ("cloud", "plane"), ("mesh", "point"), ("mesh", "plane")])
def test_single_pass_against_oracle(dev, kind, metric):
    """idx, d2, q bit for bit those of the unweighted search entries; w_out and the sums within 1e-12 of their magnitude (the bound
    tests/test_gpu_icp_mesh.py holds the unweighted sums to), the trailing count exact: every kernel, fixed and automatic scale,
    with and without point weights (a zero, a negative, a NaN and infinities among them)"""
    from pointcloudprocessing_amd import ops
    r, oref, n_parts, make, true = _refs(dev, kind)
    B, N, md = 2, 700, 1.0
    rng = np.random.default_rng(17)
    scans, labs = zip(*[make(N, 21 + b) for b in range(B)])
    scan = np.stack(scans).copy()
    lab = np.stack([RO.wrong_labels(l, 7 if kind == "cloud" else NM, 0.2, 5 + b) for b, l in enumerate(labs)])
    lab[:, :6] = -1
    scan[:, 6:9] = np.nan
    pose = np.stack([_near(true, 40 + b) for b in range(B)])
    S, L, P = _t(scan, dev), _t(lab, dev), _t(pose, dev)
    if kind == "mesh":
        bi, bd, bq = ops.icp_mesh_correspond(S, L, r, P.float(), max_dist=md)
    else:
        bi, bd = ops.icp_correspond(S, L, r, P.float(), max_dist=md)
    pw = _point_weights(rng, B, N)
    for kernel in (None,) + KERNELS:
        for rs in ("mad", 0.35):
            for w in (None, pw):
                if kernel is None and (w is None or rs != "mad"):
                    continue
                o = RO.pass_sums(scan, lab, oref, pose, metric, F32(md * md), w, kernel, rs)
                mag = RO.pass_sums(scan, lab, oref, pose, metric, F32(md * md), w, kernel, rs, magnitude=True)[5]
                g = ops.icp_robust_sums(S, L, r, P, max_dist=md, metric=metric, weights=None if w is None else _t(w, dev), robust=kernel,
                                        robust_scale=rs)
                name = (kind, metric, kernel, rs, w is not None)
                assert torch.equal(g[0], bi) and torch.equal(g[1].view(torch.int32), bd.view(torch.int32)), name
                assert np.array_equal(g[0].cpu().numpy(), o[0]) and np.array_equal(_bits(g[1].cpu().numpy()), _bits(o[1])), name
                gq = g[2].cpu().numpy()
                assert ((_bits(gq) == _bits(o[2])) | (np.isnan(gq) & np.isnan(o[2]))).all(), name
                if kind == "mesh":
                    assert torch.equal(g[2].view(torch.int32), bq.view(torch.int32)), name
                gs = g[4].cpu().numpy()
                assert np.array_equal(_bits(gs), _bits(o[4])) or (kernel is None and np.isnan(gs).all() and np.isnan(o[4]).all()), name
                gw, ew = g[3].cpu().numpy(), o[3]
                assert np.all(np.abs(gw - ew) <= 1e-12 * np.abs(ew)), (name, np.abs(gw - ew).max())
                gS, eS = g[5].cpu().numpy(), o[5]
                assert np.all(np.abs(gS - eS) <= 1e-12 * mag), (name, (np.abs(gS - eS) / np.maximum(mag, 1e-300)).max())
                assert np.array_equal(gS[:, -1], eS[:, -1]) and (eS[:, -1] > 100).all(), (name, gS[:, -1], eS[:, -1])
                if kernel == "tukey" and rs != "mad":
                    assert (eS[:, -1] < (o[0] >= 0).sum(1)).all(), name                        # the kernel cut pairs off


def test_solve_against_oracle(dev):
    from pointcloudprocessing_amd import ops
    r, oref, n_parts, make, true = _refs(dev, "cloud")
    scan, lab = make(700, 3)
    pose = _near(true, 8)
    for metric, ns in (("point", 18), ("plane", 29)):
        S = [RO.pass_sums(scan[None], lab[None], oref, pose[None], metric, F32(1.0), None, k)[5][0] for k in KERNELS]
        few = np.zeros(ns + 1)
        few[ns] = 40                                          # pairs counted, weights that sum to nothing
        low = S[0].copy()
        low[ns] = 2 if metric == "point" else 5               # too few pairs of positive weight
        scaled = 1e-3 * S[2]
        scaled[ns] = S[2][ns]                                 # sum w < 3 with pairs enough: solved
        S = np.stack(S + [few, low, scaled])
        prev = np.stack([pose] * len(S))
        gp, gr, gs = (x.cpu().numpy() for x in ops.icp_robust_solve(_t(S, dev), _t(prev, dev), metric=metric))
        for b in range(len(S)):
            P, rm, st = RO.solve(S[b], prev[b], metric)
            assert gs[b] == st, (metric, b, gs[b], st)
            assert np.abs(gp[b] - P).max() < 1e-12, (metric, b, np.abs(gp[b] - P).max())       # the unweighted solves' bound
            if st & RO.FEW_PAIRS:
                assert np.array_equal(gp[b], prev[b]) and np.isnan(gr[b])
            else:
                assert abs(gr[b] - rm) <= 1e-12 * max(rm, 1.0)
        assert gs.tolist() == [0, 0, 0, 2, 2, 0] and S[5][0] < 3


# ---------------------------------------------------------------------------------------------------------------------
# the loops
# ---------------------------------------------------------------------------------------------------------------------
def _loop_case(dev, kind, B=3, N=1024):
    r, oref, n_parts, make, true = _refs(dev, kind)
    scans, labs = zip(*[make(N, 31 + b) for b in range(B)])
    lab = np.stack([RO.wrong_labels(l, 7 if kind == "cloud" else NM, 0.2, 50 + b) for b, l in enumerate(labs)])
    init = np.stack([_near(true, 60 + b, rot=np.deg2rad(4), shift=0.25) for b in range(B)])
    return r, oref, np.stack(scans), lab, init, true


LOOPS = [("cloud", "point", "huber"), ("cloud", "plane", "tukey"), ("mesh", "plane", "tukey")]


@pytest.mark.parametrize("kind,metric,kernel", LOOPS)
def test_loop_against_oracle(dev, kind, metric, kernel):
    """1,024-point scans with 20 % of the labels replaced: pose within the bounds the unweighted loops' tests hold the device to
    against their oracles (point 1e-5 rad / 1e-4 m, plane 1e-7 rad / 1e-6 m), pairs, iters and status exact.  The scale: the
    distance to the nearest primitive is 1-Lipschitz in the query point and so is its median, so two poses (ang, dt) apart over
    points within radius R of the sensor give medians at most ang R + dt apart, times tune * 1.4826."""
    from pointcloudprocessing_amd import ops
    r, oref, scan, lab, init, true = _loop_case(dev, kind, B=1)
    kw = dict(max_iters=15, tol_rot=1e-6, tol_t=1e-6)
    g = ops.semantic_icp(_t(scan, dev), _t(lab, dev), r, _t(init, dev), max_dist=3.0, metric=metric, robust=kernel, return_scale=True, **kw)
    o = RO.icp(scan, lab, oref, init, metric, max_d2=F32(9.0), kernel=kernel, **kw)
    g = [x.cpu().numpy() for x in g]
    ang, dt = IO.pose_error(g[0][0], o[0][0])
    print(f"{kind} {metric} {kernel}: {g[3][0]} iterations, {g[2][0]} pairs, device against oracle {ang:.3e} rad {dt:.3e} m, scale "
          f"{g[5][0]!r} against {o[5][0]!r}; against the truth {IO.pose_error(g[0][0], true)}")
    assert g[3][0] == o[3][0] and g[4][0] == o[4][0] and g[2][0] == o[2][0], (g[2:5], o[2:5])
    bound = (1e-7, 1e-6) if metric == "plane" else (1e-5, 1e-4)
    assert ang < bound[0] and dt < bound[1], (ang, dt)
    assert abs(g[1][0] - o[1][0]) < 1e-6
    R = np.linalg.norm(scan[0] - init[0][:3, 3], axis=1).max() + 1.0
    assert abs(g[5][0] - o[5][0]) <= RO.TUNE[RO.KERNELS[kernel]] * 1.4826 * (bound[0] * R + bound[1]), (g[5][0], o[5][0])
    assert 500 < g[2][0] < 1024 and g[5][0] > 1e-3


@pytest.mark.parametrize("kind,metric,kernel", LOOPS)
def test_loop_determinism_batch_and_graph(dev, kind, metric, kernel):
    from pointcloudprocessing_amd import ops
    r, _, scan, lab, init, _ = _loop_case(dev, kind)
    S, L, I = _t(scan, dev), _t(lab, dev), _t(init, dev)
    W = _t(np.random.default_rng(1).uniform(0.2, 1.0, lab.shape).astype(F32), dev)
    kw = dict(max_iters=8, max_dist=3.0, tol_rot=1e-7, tol_t=1e-7, metric=metric, robust=kernel, weights=W, return_scale=True)
    same = lambda x, y: np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))     # noqa: E731
    a = ops.semantic_icp(S, L, r, I, **kw)
    for i in range(3):
        kw1 = dict(kw, weights=W[i:i + 1].contiguous())
        single = ops.semantic_icp(S[i:i + 1].contiguous(), L[i:i + 1].contiguous(), r, I[i:i + 1].contiguous(), **kw1)
        for x, y in zip(a, single):
            assert same(x[i:i + 1], y)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.semantic_icp(S, L, r, I, **kw)
        with torch.cuda.graph(graph, stream=side):                             # one chain of launches on one stream
            captured = ops.semantic_icp(S, L, r, I, **kw)
    torch.cuda.current_stream().wait_stream(side)
    for t in captured:
        t.fill_(0)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(a, captured):
        assert same(x, y)
    assert np.isfinite(a[0].cpu().numpy()).all() and (a[2].cpu().numpy() > 400).all()


def test_fixed_scale_and_weights_only_loops(dev):
    """a fixed scale is what scale_out reports; weights alone (no robust kernel) run the weighted loop, which with unit weights ends
    where the unweighted loop ends"""
    from pointcloudprocessing_amd import ops
    r, oref, scan, lab, init, _ = _loop_case(dev, "mesh", B=1)
    S, L, I = _t(scan, dev), _t(lab, dev), _t(init, dev)
    kw = dict(max_iters=6, max_dist=3.0, metric="plane")
    g = ops.semantic_icp(S, L, r, I, robust="cauchy", robust_scale=0.25, return_scale=True, **kw)
    o = RO.icp(scan, lab, oref, init, "plane", max_iters=6, max_d2=F32(9.0), kernel="cauchy", robust_scale=0.25)
    assert float(g[5][0]) == 0.25 == o[5][0] and int(g[2][0]) == int(o[2][0]) and int(g[3][0]) == int(o[3][0])
    ang, dt = IO.pose_error(g[0][0].cpu().numpy(), o[0][0])
    assert ang < 1e-7 and dt < 1e-6, (ang, dt)
    u = ops.semantic_icp(S, L, r, I, **kw)
    w = ops.semantic_icp(S, L, r, I, weights=torch.ones_like(S[:, :, 0]), return_scale=True, **kw)
    ang, dt = IO.pose_error(u[0][0].cpu().numpy(), w[0][0].cpu().numpy())
    assert ang < 1e-7 and dt < 1e-6 and torch.equal(u[2], w[2]) and torch.equal(u[3], w[3]) and torch.equal(u[4], w[4])
    assert bool(torch.isnan(w[5]).all())


def test_defaults_are_the_old_entries(dev):
    """ops.semantic_icp without the new keywords: the same bits as the direct C call of the entry it called before"""
    from pointcloudprocessing_amd import _lib, ops
    for kind, metric in (("cloud", "point"), ("cloud", "plane"), ("mesh", "plane")):
        r, _, scan, lab, init, _ = _loop_case(dev, kind, B=2)
        S, L, I = _t(scan, dev), _t(lab, dev), _t(init, dev)
        got = ops.semantic_icp(S, L, r, I, max_iters=5, max_dist=3.0, metric=metric)
        B, N = lab.shape
        pose = I.clone()
        rmse = torch.empty(B, device=dev, dtype=torch.float64)
        pairs, iters, status = (torch.empty(B, device=dev, dtype=torch.int32) for _ in range(3))
        p, lib = _lib.ptr, _lib.lib()
        if kind == "mesh":
            nb = lib.pn_icp_mesh_workspace_bytes(B, N, r.T, r.n_parts)
            ws = torch.empty(nb, device=dev, dtype=torch.uint8)
            rc = lib.pn_semantic_icp_mesh(p(S), p(L), B, N, p(r.tri), r._seg_c, r.T, r.n_parts, p(r.normals), 2, p(pose), 5, 9.0, 1e-6, 1e-6,
                                          p(pose), p(rmse), p(pairs), p(iters), p(status), p(ws), nb, _lib.current_stream())
        elif metric == "plane":
            nb = lib.pn_icp_plane_workspace_bytes(B, N, r.M, r.n_parts)
            ws = torch.empty(nb, device=dev, dtype=torch.uint8)
            rc = lib.pn_semantic_icp_plane(p(S), p(L), B, N, p(r.xyz), r._seg_c, r.M, r.n_parts, p(pose), 5, 9.0, 1e-6, 1e-6, p(r.normals),
                                           p(pose), p(rmse), p(pairs), p(iters), p(status), p(ws), nb, _lib.current_stream())
        else:
            nb = lib.pn_icp_workspace_bytes(B, N, r.M, r.n_parts)
            ws = torch.empty(nb, device=dev, dtype=torch.uint8)
            rc = lib.pn_semantic_icp(p(S), p(L), B, N, p(r.xyz), r._seg_c, r.M, r.n_parts, p(pose), 5, 9.0, 1e-6, 1e-6, p(pose), p(rmse),
                                     p(pairs), p(iters), p(status), p(ws), nb, _lib.current_stream())
        _lib.check(rc, "the unweighted entry")
        assert len(got) == 5
        for x, y in zip(got, (pose, rmse, pairs, iters, status)):
            assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8)), (kind, metric)


def test_guard_bands_of_the_c_entries(dev):
    """pn_semantic_icp_robust through the C ABI with guard bands around every output and the workspace; N = 700 leaves the last
    blocks ragged"""
    from pointcloudprocessing_amd import _lib
    GUARD, PAT = 4096, 0xA5
    r, _, scan, lab, init, _ = _loop_case(dev, "mesh", B=2, N=700)
    S, L, I = _t(scan, dev), _t(lab, dev), _t(init, dev)
    B, N = lab.shape
    W = torch.ones(B, N, device=dev)
    nb = _lib.lib().pn_icp_robust_workspace_bytes(B, N, r.T, r.n_parts)

    def guarded(shape, dtype):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        buf = torch.full((GUARD + n + GUARD,), PAT, dtype=torch.uint8, device=dev)
        return buf, buf[GUARD:GUARD + n].view(dtype).view(*shape)

    bufs = dict(pose=guarded((B, 4, 4), torch.float64), rmse=guarded((B,), torch.float64), pairs=guarded((B,), torch.int32),
                iters=guarded((B,), torch.int32), status=guarded((B,), torch.int32), scale=guarded((B,), torch.float64),
                ws=guarded((nb,), torch.uint8))
    p = lambda k: C.c_void_p(bufs[k][1].data_ptr())                            # noqa: E731
    keep = [x.clone() for x in (S, L, I, W, r.tri, r.normals)]
    rc = _lib.lib().pn_semantic_icp_robust(_lib.ptr(S), _lib.ptr(L), B, N, _lib.ptr(r.tri), r._seg_c, r.T, r.n_parts, 1, _lib.ptr(r.normals), 2,
                                           _lib.ptr(I), 6, 9.0, 1e-7, 1e-7, 3, 0.0, 4.685, 1e-4, _lib.ptr(W), p("pose"), p("rmse"), p("pairs"),
                                           p("iters"), p("status"), p("scale"), p("ws"), nb, _lib.current_stream())
    _lib.check(rc, "pn_semantic_icp_robust")
    torch.cuda.synchronize()
    for name, (buf, _) in bufs.items():
        assert bool((buf[:GUARD] == PAT).all()) and bool((buf[-GUARD:] == PAT).all()), f"{name}: guard band overwritten"
    for a, b in zip(keep, (S, L, I, W, r.tri, r.normals)):
        assert torch.equal(a, b), "an input was modified"
    assert bool(torch.isfinite(bufs["pose"][1]).all()) and bool((bufs["pairs"][1] > 300).all()) and bool((bufs["scale"][1] > 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# predict_scan / predict_pose
# ---------------------------------------------------------------------------------------------------------------------
def test_predict_scan_confidence_and_predict_pose(dev):
    from oracle import pointnet_oracle as O
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd.pointnet.PointNet import PointNet
    v, f, p, _, _, _ = _mesh_case()
    m = PointNet(23, NP, 0.3, 42, precision="bf16x3", device=dev)
    m.set_weights(O.init_params(23, NP, seed=5, randomize_bn=True))
    xyz, _ = MO.mesh_scan(v, f, p, 3000, PO.TRUE_POSE, noise=0.02, seed=4)
    X = _t(xyz, dev)
    kw = dict(leaf=1.0, samples=256, k=3)
    ci, part, R = m.predict_scan(X, **kw)                                      # the default return is unchanged
    ci2, part2, R2, conf = m.predict_scan(X, return_confidence=True, **kw)
    assert torch.equal(ci, ci2) and torch.equal(part, part2) and torch.equal(R, R2)
    assert tuple(conf.shape) == (1, 3000) and conf.dtype == torch.float32
    # against a direct propagation from the same sampled cloud
    origin = X.min(0).values.cpu().tolist()
    cent, _, _ = ops.voxel_downsample(X, (1.0, 1.0, 1.0), origin)
    if cent.shape[0] > 256:
        idx = ops.farthest_point_sample(cent.unsqueeze(0).contiguous(), 256)
        cloud = cent[idx[0].long()].unsqueeze(0).contiguous()
    else:
        cloud = cent.unsqueeze(0).contiguous()
    _, seg, _ = m(cloud, training=False)
    _, _, mix, arg = ops.knn_propagate(X.unsqueeze(0), cloud, 3, values=seg)
    assert torch.equal(arg, part)
    exp = mix.gather(2, arg.long().clamp(min=0).unsqueeze(2)).squeeze(2)
    exp = torch.where(arg >= 0, exp, torch.zeros_like(exp))
    assert torch.equal(conf, exp) and bool((conf[part >= 0] > 0).all()) and bool((conf <= 1.0001).all())
    assert bool((conf[part < 0] == 0).all())
    ref = ops.icp_mesh_reference(v, f, np.asarray(p) % NP, NP, device=dev)
    out = m.predict_pose(X, ref, init=PO.START_POSE, weights="confidence", robust="tukey", max_iters=5, max_dist=5.0, metric="plane", **kw)
    assert len(out) == 5 and tuple(out[2].shape) == (1, 4, 4) and out[2].dtype == torch.float64
    assert tuple(out[1].shape) == (1, 3000) and tuple(out[3].shape) == (1,) and tuple(out[4].shape) == (1,)
    assert bool(torch.isfinite(out[2]).all())
    out2 = m.predict_pose(X, ref, init=PO.START_POSE, weights=conf, robust="tukey", max_iters=5, max_dist=5.0, metric="plane", **kw)
    assert torch.equal(out[2], out2[2])
