"""pn_semantic_icp / pn_icp_correspond / pn_icp_solve on the MI355X: the correspondence pass bit for bit against the NumPy oracle
(tests/icp_oracle.py), the fp64 sums and the solve against the oracle, the whole loop against the oracle and a known pose,
determinism (eager, graph replay, batch against single scans), guard bands, and PointNet.predict_pose at C5 size."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import helpers
import icp_oracle as IO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
F32 = np.float32
GUARD = 4096
PAT = 0xA5
NP = len(helpers.F15_PARTS)            # 12 part labels; the kc-46 cloud uses 7 of them
# the end-to-end case: the oracle's final pose is 9.8e-6 rad and 2.6e-4 m from the true pose; both implementations must stay
# within these bounds of it
TRUE_ROT_BOUND, TRUE_T_BOUND = 5e-5, 1e-3


def _kc46():
    from pointcloudprocessing_amd import pointcloud
    return pointcloud.read_labelled_cloud(os.path.join(GOLD, "kc-46.txt"), helpers.F15_PARTS)


def _pose(R, t):
    P = np.eye(4)
    P[:3, :3] = R
    P[:3, 3] = t
    return P


TRUE = _pose(IO.rot([0.3, -0.5, 0.8], 0.7), [12.0, -4.0, 30.0])
START = _pose(IO.rot([1, 1, 0], np.deg2rad(10)) @ TRUE[:3, :3], TRUE[:3, 3] + [0.6, -0.5, 0.6])   # ~10 deg and ~1 m off


def _guarded(shape, dtype, dev):
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((GUARD + n + GUARD,), PAT, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + n].view(dtype).view(*shape)


def _intact(buf):
    return bool((buf[:GUARD] == PAT).all()) and bool((buf[-GUARD:] == PAT).all())


def _seg_c(seg):
    return (C.c_int32 * len(seg))(*[int(v) for v in seg])


def _raw_correspond(scan, labels, ref, seg, n_parts, pose32, max_d2):
    """pn_icp_correspond with guard-banded outputs and workspace; asserts the bands and the inputs are untouched"""
    from pointcloudprocessing_amd import _lib
    B, N, _ = scan.shape
    M = ref.shape[0]
    dev = scan.device
    keep = [t.clone() for t in (scan, labels, ref, pose32)]
    nbytes = _lib.lib().pn_icp_workspace_bytes(B, N, M, n_parts)
    bufs = dict(idx=_guarded((B, N), torch.int32, dev), d2=_guarded((B, N), torch.float32, dev),
                sums=_guarded((B, 18), torch.float64, dev), ws=_guarded((nbytes,), torch.uint8, dev))
    p = lambda k: C.c_void_p(bufs[k][1].data_ptr())                                   # noqa: E731
    rc = _lib.lib().pn_icp_correspond(_lib.ptr(scan), _lib.ptr(labels), B, N, _lib.ptr(ref), _seg_c(seg), M, n_parts, _lib.ptr(pose32),
                                      float(max_d2), p("idx"), p("d2"), p("sums"), p("ws"), nbytes, _lib.current_stream())
    _lib.check(rc, "pn_icp_correspond")
    torch.cuda.synchronize()
    for name, (buf, _) in bufs.items():
        assert _intact(buf), f"{name}: guard band overwritten"
    for a, b in zip(keep, (scan, labels, ref, pose32)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "an input was modified"
    return {k: v.cpu().numpy() for k, (_, v) in bufs.items() if k != "ws"}


def _sums_close(got, scan, idx, ref, tol=1e-12):
    """fp64 sums against the oracle's over the same pairs, to ``tol`` relative to the sum of the magnitudes of the terms"""
    exp = IO.sums(scan, idx, ref)
    mag = IO.sums(np.abs(np.nan_to_num(scan)), idx, np.abs(ref))
    err = np.abs(got - exp) / np.maximum(mag, 1e-300)
    return bool(np.all(np.abs(got - exp) <= tol * mag)), float(err.max())


def _correspond_case(rng, B, N):
    """scans of kc-46 under a different pose each, with ties, labels absent from the reference, -1, NaN and inf rows"""
    xyz, part = _kc46()
    xyz = xyz.copy()
    xyz[400:420] = xyz[100:120]                                 # duplicated reference points (mixed labels): ties in distance
    part[400:420] = part[100:120]
    ref, seg, _ = IO.group_reference(xyz, part, NP)
    scans, labs, poses = [], [], []
    for b in range(B):
        T = _pose(IO.rot(rng.normal(size=3), rng.uniform(0, 3)), rng.normal(size=3) * 20)
        s, lab = IO.labelled_scan(xyz, part, N, T, noise=0.3, seed=int(rng.integers(1 << 30)))
        k = rng.choice(N, 40, replace=False)
        lab[k[:10]] = 5                                         # landing_gear: absent from the kc-46 reference
        lab[k[10:15]] = 11                                      # probe: absent
        lab[k[15:20]] = -1
        lab[k[20:22]] = 99                                      # out of range
        s[k[22:26]] = np.nan
        s[k[26], 1] = np.nan
        s[k[27], 2] = np.inf
        q = xyz[rng.integers(0, len(xyz), 6)]
        s[k[30:36]] = (q.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(F32)   # exactly on a point (ties with duplicates)
        scans.append(s)
        labs.append(lab)
        poses.append(T)
    return np.stack(scans), np.stack(labs), ref, seg, np.stack(poses).astype(F32)


@pytest.mark.parametrize("B,N", [(1, 1), (1, 777), (3, 5000), (2, 20000)])
def test_correspond_bit_exact(dev, B, N):
    rng = np.random.default_rng(B * 7 + N)
    scan, lab, ref, seg, pose32 = _correspond_case(rng, B, max(N, 64))
    scan, lab = scan[:, :N].copy(), lab[:, :N].copy()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)        # noqa: E731
    out = _raw_correspond(t(scan), t(lab), t(ref), seg, NP, t(pose32), np.inf)
    ri, rd = IO.correspond(scan, lab, ref, seg, NP, pose32)
    assert np.array_equal(out["idx"], ri), np.argwhere(out["idx"] != ri)[:5]
    assert np.array_equal(out["d2"].view(np.uint32), rd.view(np.uint32))
    ok, err = _sums_close(out["sums"], scan, ri, ref)
    assert ok, err
    if N >= 5000:
        act = IO.active(scan, lab, seg, NP)
        assert (ri[~act] == -1).all() and (ri[act] >= 0).all() and (~act).sum() >= 30 * B
        # a pair exactly at max_d2 is kept, one just above is not
        d_at = np.sort(rd[act])[act.sum() // 2]
        out2 = _raw_correspond(t(scan), t(lab), t(ref), seg, NP, t(pose32), d_at)
        ri2, rd2 = IO.correspond(scan, lab, ref, seg, NP, pose32, max_d2=d_at)
        assert np.array_equal(out2["idx"], ri2) and np.array_equal(out2["d2"].view(np.uint32), rd2.view(np.uint32))
        assert (ri2[rd == d_at] >= 0).all() and (ri2[rd > d_at] == -1).all() and (rd == d_at).any()
        ok, err = _sums_close(out2["sums"], scan, ri2, ref)
        assert ok, err


def test_correspond_ops_wrapper(dev):
    from pointcloudprocessing_amd import ops
    rng = np.random.default_rng(3)
    scan, lab, ref, seg, pose32 = _correspond_case(rng, 2, 3000)
    xyz, part = _kc46()
    r = ops.icp_reference(torch.from_numpy(xyz).to(dev), torch.from_numpy(part), NP)
    assert r.seg == tuple(int(v) for v in IO.group_reference(xyz, part, NP)[1])
    scan2, lab2 = scan.copy(), lab.copy()
    # the same scans against the unduplicated reference
    ref_u, seg_u, _ = IO.group_reference(xyz, part, NP)
    idx, d2, S = ops.icp_correspond(torch.from_numpy(scan2).to(dev), torch.from_numpy(lab2).to(dev), r, torch.from_numpy(pose32).to(dev),
                                    max_dist=2.0, sums=True)
    ri, rd = IO.correspond(scan2, lab2, ref_u, seg_u, NP, pose32, max_d2=F32(4.0))
    assert np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(d2.cpu().numpy().view(np.uint32), rd.view(np.uint32))
    assert (ri == -1).sum() > (rd == np.inf).sum()                                  # max_dist removed pairs
    assert _sums_close(S.cpu().numpy(), scan2, ri, ref_u)[0]
    assert np.array_equal(r.index.cpu().numpy(), IO.group_reference(xyz, part, NP)[2])


def _solve_cases(rng):
    cases, prev = [], []
    for _ in range(4):                                                    # random noisy pairs
        q = rng.normal(size=(100, 3)) * 4
        p = q @ IO.rot(rng.normal(size=3), rng.uniform(0, np.pi)).T + rng.normal(size=3) * 9 + rng.normal(size=q.shape) * 0.2
        cases.append((q, p))
    q = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0], [3, 2, 0], [1, 3, 0]], np.float64)
    cases.append((q, q * [1, -1, 1]))                                     # coplanar mirror
    q = rng.normal(size=(40, 3)) * [3, 2, 1]
    cases.append((q, q * [1, 1, -1] + [1, 2, 3]))                         # 3-D mirror: det(V U^T) < 0
    S = [np.concatenate([[len(q)], p.sum(0), q.sum(0), (q[:, :, None] * p[:, None, :]).sum(0).reshape(9), [(p * p).sum(), (q * q).sum()]])
         for q, p in cases]
    S.append(np.concatenate([[2.0], np.ones(17)]))                        # fewer than 3 pairs
    S.append(np.zeros(18))                                                # none
    for _ in S:
        prev.append(_pose(IO.rot(rng.normal(size=3), 0.5), rng.normal(size=3)))
    return np.stack(S), np.stack(prev)


def test_solve_matches_oracle(dev):
    from pointcloudprocessing_amd import ops
    S, prev = _solve_cases(np.random.default_rng(0))
    pose, rmse, status = ops.icp_solve(torch.from_numpy(S).to(dev), torch.from_numpy(prev).to(dev))
    pose, rmse, status = pose.cpu().numpy(), rmse.cpu().numpy(), status.cpu().numpy()
    for b in range(len(S)):
        P, rm, st = IO.solve(S[b], prev[b])
        assert status[b] == st
        assert np.abs(pose[b] - P).max() < 1e-12, (b, np.abs(pose[b] - P).max())
        if st:
            assert np.array_equal(pose[b], prev[b]) and np.isnan(rmse[b])
        else:
            # rmse^2 comes from Sp + Sq - 2 trace(R H), a difference of large terms: compare it at their scale
            assert abs(rmse[b] ** 2 - rm ** 2) * S[b, 0] < 1e-12 * (S[b, 16] + S[b, 17]), (b, rmse[b], rm)
            assert abs(np.linalg.det(pose[b, :3, :3]) - 1) < 1e-12
    assert (status == IO.FEW_PAIRS).sum() == 2


def _e2e_inputs(n=32768, seed=1):
    xyz, part = _kc46()
    ref, seg, _ = IO.group_reference(xyz, part, NP)
    scan, lab = IO.labelled_scan(xyz, part, n, TRUE, noise=0.05, outliers=0.05, seed=seed)
    return xyz, part, ref, seg, scan, lab


def test_end_to_end_against_oracle_and_truth(dev):
    from pointcloudprocessing_amd import ops
    xyz, part, ref, seg, scan, lab = _e2e_inputs()
    r = ops.icp_reference(xyz, part, NP, device=dev)
    pose, rmse, pairs, iters, status = ops.semantic_icp(torch.from_numpy(scan[None]).to(dev), torch.from_numpy(lab[None]).to(dev), r,
                                                        torch.from_numpy(START[None]).to(dev), max_iters=30)
    opose, ormse, opairs, oiters, ostatus = IO.icp(scan[None], lab[None], ref, seg, NP, START[None], max_iters=30)
    g = pose.cpu().numpy()[0]
    ang, dt = IO.pose_error(g, opose[0])
    assert ang < 1e-5 and dt < 1e-4, (ang, dt)
    for P in (g, opose[0]):
        ang, dt = IO.pose_error(P, TRUE)
        assert ang < TRUE_ROT_BOUND and dt < TRUE_T_BOUND, (ang, dt)
    assert int(status[0]) == IO.CONVERGED == int(ostatus[0])
    assert abs(int(iters[0]) - int(oiters[0])) <= 1 and abs(int(pairs[0]) - int(opairs[0])) <= 2
    assert abs(float(rmse[0]) - float(ormse[0])) < 1e-4 and 0.05 < float(rmse[0]) < 0.12


def test_determinism_graph_and_batch(dev):
    from pointcloudprocessing_amd import ops
    xyz, part, ref, seg, _, _ = _e2e_inputs()
    r = ops.icp_reference(xyz, part, NP, device=dev)
    scans, labs, inits = [], [], []
    for b in range(3):
        s, lab = IO.labelled_scan(xyz, part, 20000, TRUE, noise=0.05, seed=10 + b)
        scans.append(s)
        labs.append(lab)
        inits.append(_pose(IO.rot([1, -1, b], np.deg2rad(4 + 3 * b)) @ TRUE[:3, :3], TRUE[:3, 3] + [0.3 * b, 0.5, -0.4]))
    S = torch.from_numpy(np.stack(scans)).to(dev)
    L = torch.from_numpy(np.stack(labs)).to(dev)
    I = torch.from_numpy(np.stack(inits)).to(dev)
    kw = dict(max_iters=12, max_dist=3.0, tol_rot=1e-7, tol_t=1e-7)
    a = ops.semantic_icp(S, L, r, I, **kw)
    b = ops.semantic_icp(S, L, r, I, **kw)
    for x, y in zip(a, b):
        assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))
    for i in range(3):
        single = ops.semantic_icp(S[i:i + 1].contiguous(), L[i:i + 1].contiguous(), r, I[i:i + 1].contiguous(), **kw)
        for x, y in zip(a, single):
            assert np.array_equal(x[i:i + 1].cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))
    assert (a[3] >= 1).all() and (a[3] <= 12).all()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.semantic_icp(S, L, r, I, **kw)                                # warm-up on the capture stream
        with torch.cuda.graph(g, stream=side):
            captured = ops.semantic_icp(S, L, r, I, **kw)
    torch.cuda.current_stream().wait_stream(side)
    for t in captured:
        t.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(a, captured):
        assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))


def test_guard_bands_and_few_pairs(dev):
    from pointcloudprocessing_amd import _lib
    xyz, part, ref, seg, scan, lab = _e2e_inputs(n=5000)
    B, N = 2, 5000
    scan2 = np.stack([scan, scan])
    lab2 = np.stack([lab, np.where(np.arange(N) < 2, lab, -1).astype(np.int32)])      # scan 1: at most 2 labelled points
    lab2[1, :2] = 3
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                  # noqa: E731
    nbytes = _lib.lib().pn_icp_workspace_bytes(B, N, len(ref), NP)
    init = np.stack([START, START])
    bufs = dict(pose=_guarded((B, 4, 4), torch.float64, dev), rmse=_guarded((B,), torch.float64, dev),
                pairs=_guarded((B,), torch.int32, dev), iters=_guarded((B,), torch.int32, dev), status=_guarded((B,), torch.int32, dev),
                ws=_guarded((nbytes,), torch.uint8, dev))
    p = lambda k: C.c_void_p(bufs[k][1].data_ptr())                                   # noqa: E731
    ins = [t(scan2), t(lab2), t(ref), t(init)]
    keep = [x.clone() for x in ins]
    rc = _lib.lib().pn_semantic_icp(_lib.ptr(ins[0]), _lib.ptr(ins[1]), B, N, _lib.ptr(ins[2]), _seg_c(seg), len(ref), NP,
                                    _lib.ptr(ins[3]), 30, float("inf"), 1e-6, 1e-6, p("pose"), p("rmse"), p("pairs"), p("iters"),
                                    p("status"), p("ws"), nbytes, _lib.current_stream())
    _lib.check(rc, "pn_semantic_icp")
    torch.cuda.synchronize()
    for name, (buf, _) in bufs.items():
        assert _intact(buf), f"{name}: guard band overwritten"
    for a, b in zip(keep, ins):
        assert torch.equal(a, b)
    out = {k: v.cpu().numpy() for k, (_, v) in bufs.items() if k != "ws"}
    opose, ormse, opairs, oiters, ostatus = IO.icp(scan2, lab2, ref, seg, NP, init)
    assert out["status"].tolist() == ostatus.tolist() and out["status"][1] == IO.FEW_PAIRS | IO.CONVERGED
    assert out["iters"].tolist() == oiters.tolist() and out["iters"][1] == 1 and out["pairs"][1] == opairs[1] <= 2
    assert np.array_equal(out["pose"][1], START) and np.isnan(out["rmse"][1])
    ang, dt = IO.pose_error(out["pose"][0], opose[0])
    assert ang < 1e-5 and dt < 1e-4


def test_errors_raise_through_ops(dev):
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd._lib import PointNetHipError
    xyz, part = _kc46()
    r = ops.icp_reference(xyz, part, NP, device=dev)
    S = torch.zeros(1, 100, 3, device=dev)
    L = torch.zeros(1, 100, dtype=torch.int32, device=dev)
    I = torch.eye(4, dtype=torch.float64, device=dev)[None]
    for kw in (dict(max_iters=0), dict(max_dist=float("nan")), dict(tol_rot=-1.0)):
        with pytest.raises(PointNetHipError):
            ops.semantic_icp(S, L, r, I, **kw)
    with pytest.raises(PointNetHipError):
        ops.semantic_icp(S, L[:, :50].contiguous(), r, I)
    with pytest.raises(PointNetHipError):
        ops.semantic_icp(S, L, r, I[:, :3])
    with pytest.raises(PointNetHipError):
        ops.semantic_icp(S, L, ops.icp_reference(xyz, np.arange(len(xyz)) % 17, 17, device=dev), I)


def _bench_scan():
    spec = importlib.util.spec_from_file_location("bench_scan", os.path.join(ROOT, "tools", "bench_scan.py"))
    bs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bs)
    return bs


def test_predict_pose_c5_composition(dev):
    """BASELINE config 5 at full size: predict_pose equals predict_scan -> initial_pose -> semantic_icp, and the initial pose
    equals its definition computed in NumPy"""
    from oracle import pointnet_oracle as O            # checker only
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd.pointnet.PointNet import PointNet
    bs = _bench_scan()
    xyz, origin = bs.make_scan(131072)
    x = torch.from_numpy(xyz).to(dev)
    model = PointNet(23, 12, 0.3, 42, precision="bf16", device=dev)          # with T-Nets: a non-trivial R
    model.set_weights(O.init_params(23, 12, seed=31, randomize_bn=True))
    kx, _ = _kc46()
    kp = (np.arange(len(kx)) % NP).astype(np.int32)          # every part label present: the untrained model's parts all pair
    ref = ops.icp_reference(kx, kp, NP, device=dev)
    ci, part, pose, rmse, pairs = model.predict_pose(x, ref, leaf=0.25, samples=8192, k=3, origin=origin, max_iters=20)
    assert tuple(pose.shape) == (1, 4, 4) and pose.dtype == torch.float64 and tuple(part.shape) == (1, 131072)
    ci2, part2, R = model.predict_scan(x, leaf=0.25, samples=8192, k=3, origin=origin)
    assert torch.equal(ci, ci2) and torch.equal(part, part2)
    P0 = PointNet.initial_pose(x, part2, R, ref)
    # the definition in NumPy
    lab = part2[0].cpu().numpy()
    shared = [l for l in range(NP) if ref.seg[l + 1] > ref.seg[l] and (lab == l).any()]
    U, _, Vt = np.linalg.svd(R[0].double().cpu().numpy())
    R64 = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt                 # the rotation nearest to the T-Net's R
    assert np.abs(R[0].double().cpu().numpy() - np.eye(3)).max() > 1e-2        # (an untrained T-Net: R is no rotation)
    if shared:
        cs = xyz[np.isin(lab, shared)].astype(np.float64).mean(0)
        cr = kx[np.isin(kp, shared)].astype(np.float64).mean(0)
    else:
        cs, cr = xyz.astype(np.float64).mean(0), kx.astype(np.float64).mean(0)
    assert np.abs(P0[0, :3, :3].cpu().numpy() - R64).max() < 1e-12
    assert np.abs(P0[0, :3, 3].cpu().numpy() - (cs - R64 @ cr)).max() < 1e-9
    p2, r2, n2, _, _ = ops.semantic_icp(x.unsqueeze(0), part2, ref, P0, max_iters=20)
    assert torch.equal(pose, p2) and torch.equal(rmse, r2) and torch.equal(pairs, n2) and int(pairs[0]) > 100000
    assert shared and np.isfinite(float(rmse[0]))
    # init= overrides the start
    _, _, p3, _, _ = model.predict_pose(x, ref, origin=origin, init=P0[0].cpu().numpy(), max_iters=20)
    assert torch.equal(p3, p2)
    Rf = pose[0, :3, :3].cpu().numpy()
    assert np.abs(Rf @ Rf.T - np.eye(3)).max() < 1e-12
