"""pn_icp_gicp_sums / pn_semantic_icp_gicp on the MI355X: the search bit for bit against pn_icp_correspond, the 29 sums and the solve
against the NumPy oracle (tests/icp_gicp_oracle.py) on the kc-46 case of tests/test_gpu_icp_plane.py with planted scan normals
(tests/gicp_cases.py; its inputs are examined in tests/test_cpu_icp_gicp.py), the grid against the plain reference byte for byte,
the loop against the oracle loop, determinism (eager, graph replay, batch against single scans), guard bands, too few pairs, and
ops.register_scans(metric="gicp") from a start and without one."""
import ctypes as C

import numpy as np
import pytest
import torch

import fpfh_oracle as FO
import gicp_cases as GC
import icp_gicp_oracle as GO
import icp_mesh_oracle as MO
import icp_oracle as IO
import icp_plane_oracle as PO

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 4096
PAT = 0xA5
NP = GC.NP
NM = len(MO.MESH_PARTS)


def _guarded(shape, dtype, dev):
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((GUARD + n + GUARD,), PAT, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + n].view(dtype).view(*shape)


def _intact(buf):
    return bool((buf[:GUARD] == PAT).all()) and bool((buf[-GUARD:] == PAT).all())


def _seg_c(seg):
    return (C.c_int32 * len(seg))(*[int(v) for v in seg])


def _t(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)            # (a copy: the shared case arrays are read-only)


def _bytes_equal(a, b):
    return all(np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8)) for x, y in zip(a, b))


def _refs(dev, nrm, max_dist=2.0):
    """the grouped kc-46 cloud carrying ``nrm`` as a plain reference and as a grid reference built at ``max_dist``"""
    from pointcloudprocessing_amd import ops
    xyz, part = GC.kc46()
    plain = ops.icp_reference(xyz, part, NP, device=dev)._with_normals(_t(nrm, dev))
    grid = ops.icp_reference(xyz, part, NP, device=dev, accel="grid", max_dist=max_dist)._with_normals(plain.normals)
    assert type(grid) is ops.IcpGridReference and np.array_equal(plain.xyz.cpu().numpy(), GC.reference()[0])
    return plain, grid


def _sums_close(got, c, idx, tol=1e-12):
    """the 29 sums against the oracle's over the same pairs, to ``tol`` relative to the sum of the magnitudes of the terms (|J|, |d| and
    eps I + (eps kappa / 2)(|s||s|^T / D_s + |f||f|^T / D_f): the off-diagonal entries of W cancel)"""
    exp = GO.sums(c["scan"], c["scan_nrm"], idx, c["ref"], c["nrm"], c["pose"])
    mag = GO.sums(c["scan"], c["scan_nrm"], idx, c["ref"], c["nrm"], c["pose"], magnitudes=True)
    err = np.abs(got - exp) / np.maximum(mag, 1e-300)
    return bool(np.all(np.abs(got - exp) <= tol * mag)), float(err.max())


@pytest.mark.parametrize("B,N", [(1, 1), (1, 777), (3, 5000)])
def test_gicp_sums_against_correspond_and_oracle(dev, B, N):
    from pointcloudprocessing_amd import _lib, ops
    c = GC.sums_case(B, N)
    M = len(c["ref"])
    ins = [_t(a, dev) for a in (c["scan"], c["lab"], c["scan_nrm"], c["ref"], c["nrm"], c["pose"].astype(F32), c["pose"])]
    keep = [x.clone() for x in ins]
    nbytes = _lib.lib().pn_icp_gicp_workspace_bytes(B, N, M, NP)
    bufs = dict(idx=_guarded((B, N), torch.int32, dev), d2=_guarded((B, N), torch.float32, dev), sums=_guarded((B, 29), torch.float64, dev),
                ws=_guarded((nbytes,), torch.uint8, dev))
    p = lambda k: C.c_void_p(bufs[k][1].data_ptr())                                   # noqa: E731
    r = ops.IcpReference(ins[3], c["seg"], torch.arange(M, device=dev), NP)
    for max_d2 in GC.MAX_D2:
        rc = _lib.lib().pn_icp_gicp_sums(_lib.ptr(ins[0]), _lib.ptr(ins[1]), _lib.ptr(ins[2]), B, N, _lib.ptr(ins[3]), _seg_c(c["seg"]), M, NP,
                                         _lib.ptr(ins[4]), _lib.ptr(ins[5]), _lib.ptr(ins[6]), max_d2, GO.EPS, p("idx"), p("d2"), p("sums"),
                                         p("ws"), nbytes, None, 0.0, _lib.current_stream())
        _lib.check(rc, "pn_icp_gicp_sums")
        torch.cuda.synchronize()
        for name, (buf, _) in bufs.items():
            assert _intact(buf), f"{name}: guard band overwritten"
        for a, b in zip(keep, ins):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "an input was modified"
        ci, cd = ops.icp_correspond(ins[0], ins[1], r, ins[5], max_dist=float(np.sqrt(max_d2)))
        idx, d2, S = bufs["idx"][1].cpu().numpy(), bufs["d2"][1].cpu().numpy(), bufs["sums"][1].cpu().numpy()
        assert np.array_equal(idx, ci.cpu().numpy()) and np.array_equal(d2.view(np.uint32), cd.cpu().numpy().view(np.uint32))
        ok, err = _sums_close(S, c, idx)
        print(f"B={B} N={N} max_d2={max_d2}: counted {S[:, 0].astype(int).tolist()} of {(idx >= 0).sum(1).tolist()}, worst error {err:.3g} of the magnitudes")
        assert ok, err
        assert np.array_equal(S[:, 0], [GO.counted(idx[b], c["nrm"], c["scan_nrm"][b]).sum() for b in range(B)])
        if N >= 777:
            assert (S[:, 0] < (idx >= 0).sum(1)).all() and (S[:, 0] > 0).all()


def test_gicp_sums_ops_wrapper_grid_and_solve(dev):
    """ops.icp_gicp_sums on the plain and the grid reference (built at max_dist 2) at max_dist <= 2: idx and the sums byte for byte,
    d2 by the grid's contract (include/pointnet_hip.h, pn_icp_grid_build: the same bits within the tables' r2, +inf beyond it, where
    the brute-force search reports the distance of a pair that no max_d2 <= r2 keeps); and ops.icp_plane_solve on the device's sums is
    the oracle's pose"""
    from pointcloudprocessing_amd import ops
    c = GC.sums_case(3, 5000)
    plain, grid = _refs(dev, c["nrm"])
    S, L, SN, P = (_t(c[k], dev) for k in ("scan", "lab", "scan_nrm", "pose"))
    for md in (2.0, 1.0):
        a = ops.icp_gicp_sums(S, L, SN, plain, P, md)
        b = ops.icp_gicp_sums(S, L, SN, grid, P, md)
        assert _bytes_equal((a[0], a[2]), (b[0], b[2])), md
        within = a[1] <= grid.r2
        assert torch.equal(a[1][within], b[1][within]) and bool(torch.isinf(b[1][~within]).all()) and bool((b[0][~within] < 0).all())
        assert int(within.sum()) > 10000 and int((~within).sum()) > 100
        ri, rd = IO.correspond(c["scan"], c["lab"], c["ref"], c["seg"], NP, c["pose"].astype(F32), max_d2=F32(md * md))
        assert np.array_equal(a[0].cpu().numpy(), ri) and np.array_equal(a[1].cpu().numpy().view(np.uint32), rd.view(np.uint32))
        assert _sums_close(a[2].cpu().numpy(), c, ri)[0]
    pose, rmse, status = (x.cpu().numpy() for x in ops.icp_plane_solve(a[2], P))
    sums = a[2].cpu().numpy()
    for b in range(3):
        ep, er, es = PO.solve(sums[b], c["pose"][b])
        assert status[b] == es == 0 and np.abs(pose[b] - ep).max() < 1e-12 and abs(rmse[b] - er) <= 1e-15 * max(er, 1.0)
    # another eps reaches the kernel
    e2 = ops.icp_gicp_sums(S, L, SN, plain, P, 1.0, eps=0.05)[2].cpu().numpy()
    exp = GO.sums(c["scan"], c["scan_nrm"], ri, c["ref"], c["nrm"], c["pose"], eps=0.05)
    mag = GO.sums(c["scan"], c["scan_nrm"], ri, c["ref"], c["nrm"], c["pose"], eps=0.05, magnitudes=True)
    assert np.all(np.abs(e2 - exp) <= 1e-12 * mag) and not np.allclose(e2, sums)


def test_gicp_loop_against_oracle_and_grid(dev):
    """the device loop against the oracle's on the kc-46 case, both from the same normals: 8 iterations at tolerances 1e-9, the
    bounds of the plane loop's test; and the loop through the grid (built at max_dist 2) byte for byte the plain one's"""
    from pointcloudprocessing_amd import ops
    c = GC.sums_case(1, 20000, nan_normals=False, seed=5)             # the plane loop test's scans, poses and normals
    plain, grid = _refs(dev, c["nrm"])
    S, L, SN, P = (_t(c[k], dev) for k in ("scan", "lab", "scan_nrm", "pose"))
    kw = dict(max_iters=8, tol_rot=1e-9, tol_t=1e-9, metric="gicp", scan_normals=SN)
    g = ops.semantic_icp(S, L, plain, P, **kw)
    o = GO.icp(c["scan"], c["lab"], c["scan_nrm"], c["ref"], c["seg"], NP, c["nrm"], c["pose"], max_iters=8, tol_rot=1e-9, tol_t=1e-9)
    ang, dt = IO.pose_error(g[0][0].cpu().numpy(), o[0][0])
    print(f"loop against the oracle: {ang:.3g} rad, {dt:.3g} m, iters {int(g[3][0])}/{int(o[3][0])}, pairs {int(g[2][0])}/{int(o[2][0])}")
    assert ang < 1e-7 and dt < 1e-6, (ang, dt)
    assert int(g[3][0]) == int(o[3][0]) and int(g[4][0]) == int(o[4][0]) and abs(int(g[2][0]) - int(o[2][0])) <= 2
    for md in (2.0, 1.5):
        assert _bytes_equal(ops.semantic_icp(S, L, plain, P, max_dist=md, **kw), ops.semantic_icp(S, L, grid, P, max_dist=md, **kw)), md


def test_gicp_determinism_graph_and_batch(dev):
    from pointcloudprocessing_amd import ops
    c = GC.sums_case(3, 5000)
    plain, _ = _refs(dev, c["nrm"])
    S, L, SN, I = (_t(c[k], dev) for k in ("scan", "lab", "scan_nrm", "pose"))
    kw = dict(max_iters=6, max_dist=3.0, tol_rot=1e-7, tol_t=1e-7, metric="gicp")
    a = ops.semantic_icp(S, L, plain, I, scan_normals=SN, **kw)
    assert _bytes_equal(a, ops.semantic_icp(S, L, plain, I, scan_normals=SN, **kw))
    for i in range(3):
        single = ops.semantic_icp(S[i:i + 1].contiguous(), L[i:i + 1].contiguous(), plain, I[i:i + 1].contiguous(),
                                  scan_normals=SN[i:i + 1].contiguous(), **kw)
        assert _bytes_equal([x[i:i + 1] for x in a], single), i
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.semantic_icp(S, L, plain, I, scan_normals=SN, **kw)
        with torch.cuda.graph(g, stream=side):
            captured = ops.semantic_icp(S, L, plain, I, scan_normals=SN, **kw)
    torch.cuda.current_stream().wait_stream(side)
    for t in captured:
        t.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    assert _bytes_equal(a, captured)
    assert (a[3].cpu().numpy() > 1).all() and np.isfinite(a[1].cpu().numpy()).all()


def test_gicp_guard_bands_and_few_pairs(dev):
    """the loop through the C ABI with guard bands; scan 1 has five labelled points, scan 2 every label but only five valid scan
    normals: fewer than 6 counted pairs keep the pose, with rmse NaN and PN_ICP_FEW_PAIRS"""
    from pointcloudprocessing_amd import _lib
    c = GC.sums_case(1, 5000, seed=9)
    B, N, M = 3, 5000, len(c["ref"])
    scan = np.concatenate([c["scan"]] * 3)
    lab = np.concatenate([c["lab"], np.where(np.arange(N) < 5, 3, -1).astype(np.int32)[None], c["lab"]])
    sn = np.concatenate([c["scan_nrm"]] * 3)
    sn[1, :5] = [0.0, 0.0, 1.0]
    valid = np.flatnonzero(GO.counted(IO.correspond(c["scan"], c["lab"], c["ref"], c["seg"], NP, c["pose"].astype(F32))[0][0], c["nrm"], c["scan_nrm"][0]))
    sn[2] = np.nan
    sn[2, valid[:5]] = c["scan_nrm"][0, valid[:5]]
    init = np.concatenate([c["pose"]] * 3)
    nbytes = _lib.lib().pn_icp_gicp_workspace_bytes(B, N, M, NP)
    bufs = dict(pose=_guarded((B, 4, 4), torch.float64, dev), rmse=_guarded((B,), torch.float64, dev), pairs=_guarded((B,), torch.int32, dev),
                iters=_guarded((B,), torch.int32, dev), status=_guarded((B,), torch.int32, dev), ws=_guarded((nbytes,), torch.uint8, dev))
    p = lambda k: C.c_void_p(bufs[k][1].data_ptr())                                   # noqa: E731
    ins = [_t(a, dev) for a in (scan, lab, sn, c["ref"], c["nrm"], init)]
    keep = [x.clone() for x in ins]
    rc = _lib.lib().pn_semantic_icp_gicp(_lib.ptr(ins[0]), _lib.ptr(ins[1]), _lib.ptr(ins[2]), B, N, _lib.ptr(ins[3]), _seg_c(c["seg"]), M, NP,
                                         _lib.ptr(ins[4]), _lib.ptr(ins[5]), 30, float("inf"), 1e-6, 1e-6, GO.EPS, p("pose"), p("rmse"),
                                         p("pairs"), p("iters"), p("status"), p("ws"), nbytes, None, 0.0, _lib.current_stream())
    _lib.check(rc, "pn_semantic_icp_gicp")
    torch.cuda.synchronize()
    for name, (buf, _) in bufs.items():
        assert _intact(buf), f"{name}: guard band overwritten"
    for a, b in zip(keep, ins):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    out = {k: v.cpu().numpy() for k, (_, v) in bufs.items() if k != "ws"}
    for b in (1, 2):
        assert out["status"][b] == PO.FEW_PAIRS | PO.CONVERGED and out["iters"][b] == 1 and out["pairs"][b] <= 5, (b, out)
        assert np.array_equal(out["pose"][b], init[b]) and np.isnan(out["rmse"][b])
    assert out["pairs"][2] == 5
    assert out["status"][0] & PO.CONVERGED and 1 < out["iters"][0] <= 30 and np.isfinite(out["rmse"][0]) and out["pairs"][0] > 1000


def _registration_pair(dev):
    """the scene of tests/test_gpu_icp_grid.py's test_register_scans"""
    from pointcloudprocessing_amd import ops
    v, f, p = MO.aircraft_mesh(2)
    mesh = ops.icp_mesh_reference(v, f, p, NM, device=dev)
    target = ops.mesh_sample(mesh, 20000, seed=11)[0][0].contiguous()
    src = ops.mesh_sample(mesh, 20000, seed=12)[0][0].double()
    true = np.eye(4)
    true[:3, :3] = IO.rot([1, 2, -1], np.deg2rad(1.0))
    true[:3, 3] = [0.06, -0.05, 0.06]
    gen = torch.Generator(device="cpu").manual_seed(5)
    noise = torch.randn(src.shape, generator=gen, dtype=torch.float64).to(dev) * 0.02
    source = (src @ _t(true[:3, :3].T.copy(), dev) + _t(true[:3, 3].copy(), dev) + noise).float().contiguous()
    source[7] = float("nan")                                                          # a no-return pixel on either side
    target = torch.cat([target, torch.full((1, 3), float("nan"), device=dev)])
    return source, target, true


def test_register_scans_gicp(dev):
    """two independent surface samplings of the aircraft mesh (test_register_scans' scene): the grid and the brute-force search give
    the same bytes, the caller's source normals the same bytes as the call's own, and the pose is within that test's 0.05 degrees /
    5 cm.  Iterations, errors and rmse of the plane metric beside it are printed, not compared."""
    from pointcloudprocessing_amd import ops
    source, target, true = _registration_pair(dev)
    got = ops.register_scans(source, target, 0.5, metric="gicp")
    assert _bytes_equal(got, ops.register_scans(source, target, 0.5, metric="gicp", accel=None))
    sn = ops.estimate_normals(source, 0.5, 8)[0]
    assert _bytes_equal(got, ops.register_scans(source, target, 0.5, metric="gicp", source_normals=sn))
    assert _bytes_equal(got, ops.register_scans(source[None], target, 0.5, metric="gicp", source_normals=sn[None]))
    for metric, res in (("gicp", got), ("plane", ops.register_scans(source, target, 0.5, metric="plane"))):
        pose, rmse, pairs, iters, status = (x.cpu().numpy() for x in res)
        ang, dt = IO.pose_error(pose[0], true)
        print(f"register_scans {metric}: {int(iters[0])} iterations, {np.rad2deg(ang):.4f} deg, {dt * 100:.2f} cm, rmse {rmse[0]:.4f}, pairs {int(pairs[0])}")
        if metric == "gicp":
            assert pose.shape == (1, 4, 4) and pairs[0] > 15000 and status[0] & PO.CONVERGED
            assert np.rad2deg(ang) <= 0.05 and dt <= 0.05, (np.rad2deg(ang), dt)
    # another eps reaches the loop, and a batch is the single scans
    assert not _bytes_equal(got[:1], ops.register_scans(source, target, 0.5, metric="gicp", gicp_eps=0.1)[:1])
    batch = ops.register_scans(torch.stack([source, source]), target, 0.5, metric="gicp")
    assert batch[0].shape == (2, 4, 4) and _bytes_equal([x[:1] for x in batch], got) and _bytes_equal([x[1:] for x in batch], got)


def test_global_registration_gicp(dev):
    """register_scans(init="global", metric="gicp") on the registration fixture: within the bounds tests/test_gpu_fpfh.py asks of the
    plane metric there (fpfh_oracle.BOUND_ROT, BOUND_T); ops.global_register is the same call"""
    from pointcloudprocessing_amd import ops
    sc, S = FO.scene(), FO.SCENE
    src, tgt = _t(sc["source"], dev), _t(sc["target"], dev)
    sv, tv = sc["source_viewpoint"].tolist(), sc["target_viewpoint"].tolist()
    kw = dict(hypotheses=S["hypotheses"], keep=S["keep"], top=S["top"], mutual=S["mutual"], seed=S["seed"], max_iters=S["max_iters"])
    got = ops.register_scans(src, tgt, S["max_dist"], init="global", feature_radius=S["feature_radius"], normals_radius=S["normals_radius"],
                             viewpoint=tv, source_viewpoint=sv, metric="gicp", **kw)
    assert len(got) == 7
    pose, rmse, pairs, iters, status, cost, winner = (t.cpu().numpy() for t in got)
    ang, dt = IO.pose_error(pose[0], sc["pose"])
    print(f"register_scans(init='global', metric='gicp'): winner {int(winner[0])}, cost {cost[0]:.8f}, {np.rad2deg(ang):.4f} deg, {100 * dt:.3f} cm, "
          f"pairs {int(pairs[0])}, iters {int(iters[0])}")
    assert pose.shape == (1, 4, 4) and ang <= FO.BOUND_ROT and dt <= FO.BOUND_T
    direct = ops.global_register(src, tgt, S["feature_radius"], S["max_dist"], normals_radius=S["normals_radius"], k=S["k"],
                                 edge_ratio=S["edge_ratio"], source_viewpoint=sv, target_viewpoint=tv, metric="gicp", **kw)
    assert _bytes_equal(got, direct)
    plane = ops.global_register(src, tgt, S["feature_radius"], S["max_dist"], normals_radius=S["normals_radius"], k=S["k"],
                                edge_ratio=S["edge_ratio"], source_viewpoint=sv, target_viewpoint=tv, **kw)
    assert not _bytes_equal(got[:1], plane[:1])                                       # the metric reached the refinement


def test_gicp_errors_raise_through_ops(dev):
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd._lib import PointNetHipError
    c = GC.sums_case(1, 777)
    plain, grid = _refs(dev, c["nrm"])
    S, L, SN, I = (_t(c[k], dev) for k in ("scan", "lab", "scan_nrm", "pose"))
    v, f, p = MO.aircraft_mesh(0)
    mesh = ops.icp_mesh_reference(v, f, p, NM, device=dev)
    bare = ops.icp_reference(*GC.kc46(), NP, device=dev)
    cases = [(dict(ref=mesh), "cloud reference"), (dict(ref=bare), "needs reference normals"), (dict(scan_normals=None), "needs scan_normals"),
             (dict(scan_normals=SN[:, :100].contiguous()), "scan_normals must be"), (dict(scan_normals=SN.double()), "dtype"),
             (dict(scan_normals=SN.cpu()), "CUDA/HIP tensor"), (dict(robust="huber"), "neither robust= nor weights="),
             (dict(weights=torch.ones(1, 777, device=dev)), "neither robust= nor weights="), (dict(gicp_eps=0.0), "eps=0"),
             (dict(gicp_eps=1.5), "eps=1.5"), (dict(gicp_eps=float("nan")), "eps="), (dict(max_iters=0), "max_iters=0"),
             (dict(ref=grid), "exceeds the grid reference's max_dist=2"), (dict(ref=grid, max_dist=2.5), "exceeds the grid reference's max_dist=2")]
    for kw, msg in cases:
        a = dict(ref=plain, scan_normals=SN)
        a.update(kw)
        ref = a.pop("ref")
        with pytest.raises(PointNetHipError, match=msg):
            ops.semantic_icp(S, L, ref, I, metric="gicp", **a)
    for metric in ("point", "plane"):
        with pytest.raises(PointNetHipError, match="scan_normals goes with metric 'gicp'"):
            ops.semantic_icp(S, L, plain, I, metric=metric, scan_normals=SN)
    with pytest.raises(PointNetHipError, match="eps=-1"):
        ops.icp_gicp_sums(S, L, SN, plain, I, 2.0, eps=-1.0)
    with pytest.raises(PointNetHipError, match="cloud reference"):
        ops.icp_gicp_sums(S, L, SN, mesh, I, 2.0)
    with pytest.raises(PointNetHipError, match="pose must have dtype"):
        ops.icp_gicp_sums(S, L, SN, plain, I.float(), 2.0)
    src, tgt = S[0, :500].contiguous(), plain.xyz
    with pytest.raises(PointNetHipError, match="source_normals goes with metric 'gicp'"):
        ops.register_scans(src, tgt, 1.0, source_normals=SN[0, :500].contiguous())
    with pytest.raises(PointNetHipError, match="source_normals must be"):
        ops.register_scans(src, tgt, 1.0, metric="gicp", source_normals=SN[0, :400].contiguous())
