"""pn_icp_mesh_correspond / pn_semantic_icp_mesh on the MI355X: the point-to-triangle search bit for bit against the NumPy oracle
(tests/icp_mesh_oracle.py) -- triangle index, d2 and closest point, zero excluded cases -- on the procedural aircraft at two
subdivision levels, on random triangles and on an integer grid whose shared edges and vertices give exact ties; both kinds of sums
and both loops against the oracle; determinism (eager, graph replay, batch against single scans), guard bands, the unchanged point
reference path, the seams of the walk that both reference kinds share (segments of 1, U - 1, U, 0 and U + 1 primitives), and
PointNet.predict_pose with a mesh reference at C5 size."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import helpers
import icp_mesh_oracle as MO
import icp_oracle as IO
import icp_plane_oracle as PO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
F32 = np.float32
GUARD = 4096
PAT = 0xA5
NM = len(MO.MESH_PARTS)
NP = len(helpers.F15_PARTS)


def _guarded(shape, dtype, dev):
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((GUARD + n + GUARD,), PAT, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + n].view(dtype).view(*shape)


def _intact(buf):
    return bool((buf[:GUARD] == PAT).all()) and bool((buf[-GUARD:] == PAT).all())


def _seg_c(seg):
    return (C.c_int32 * len(seg))(*[int(v) for v in seg])


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _raw_correspond(dev, scan, lab, tri, seg, n_parts, pose32, max_d2, mode=0, normals=None, pose64=None):
    """pn_icp_mesh_correspond through the C ABI with guard bands around every output and the workspace; the inputs must come back
    untouched"""
    from pointcloudprocessing_amd import _lib
    B, N, _ = scan.shape
    T = len(tri)
    ins = [_t(a, dev) for a in (scan, lab, tri, pose32)] + [None if a is None else _t(a, dev) for a in (normals, pose64)]
    keep = [None if x is None else x.clone() for x in ins]
    nbytes = _lib.lib().pn_icp_mesh_workspace_bytes(B, N, T, n_parts)
    bufs = dict(idx=_guarded((B, N), torch.int32, dev), d2=_guarded((B, N), torch.float32, dev), q=_guarded((B, N, 3), torch.float32, dev),
                sums=_guarded((B, 18 if mode == 1 else 29), torch.float64, dev), ws=_guarded((nbytes,), torch.uint8, dev))
    p = lambda k: C.c_void_p(bufs[k][1].data_ptr())                                   # noqa: E731
    rc = _lib.lib().pn_icp_mesh_correspond(_lib.ptr(ins[0]), _lib.ptr(ins[1]), B, N, _lib.ptr(ins[2]), _seg_c(seg), T, n_parts,
                                           _lib.ptr(ins[3]), float(max_d2), mode, _lib.ptr(ins[4]), _lib.ptr(ins[5]), p("idx"), p("d2"),
                                           p("q"), p("sums") if mode else None, p("ws"), nbytes, _lib.current_stream())
    _lib.check(rc, "pn_icp_mesh_correspond")
    torch.cuda.synchronize()
    for name, (buf, _) in bufs.items():
        assert _intact(buf), f"{name}: guard band overwritten"
    for a, b in zip(keep, ins):
        assert a is None or torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "an input was modified"
    out = {k: v.cpu().numpy() for k, (_, v) in bufs.items() if k != "ws"}
    return out


def _check_search(out, scan, lab, tri, seg, n_parts, pose32, max_d2, name):
    ei, ed, eq = MO.correspond(scan, lab, tri, seg, n_parts, pose32, max_d2)
    assert np.array_equal(out["idx"], ei), (name, np.argwhere(out["idx"] != ei)[:5])
    assert np.array_equal(_bits(out["d2"]), _bits(ed)), (name, np.argwhere(_bits(out["d2"]) != _bits(ed))[:5])
    same = (_bits(out["q"]) == _bits(eq)) | (np.isnan(out["q"]) & np.isnan(eq))
    assert same.all(), (name, np.argwhere(~same)[:5])
    return ei, ed, eq


def _pose_near(rng, true, rot=0.05, shift=0.3):
    P = true.copy()
    P[:3, :3] = IO.rot(rng.normal(size=3), rot) @ true[:3, :3]
    P[:3, 3] += rng.normal(size=3) * shift
    return P


def _spoil(rng, scan, lab, n_parts):
    """labels -1 and out of range, a label whose segment is empty, NaN and inf points"""
    N = scan.shape[0]
    k = rng.choice(N, 40, replace=False)
    lab[k[:8]] = -1
    lab[k[8:14]] = n_parts + 3
    lab[k[14:22]] = n_parts - 1                                   # the empty segment
    scan[k[22:27]] = np.nan
    scan[k[27], 2] = np.inf
    scan[k[28], 0] = -np.inf


def _aircraft_case(level, B, N, seed):
    """scans of the aircraft mesh with 5 cm noise at poses near the true one; one more label than the mesh has (an empty segment)"""
    rng = np.random.default_rng(seed)
    v, f, p = MO.aircraft_mesh(level)
    n_parts = NM + 1
    tri, seg, _, nrm, _ = MO.group_mesh(v, f, p, n_parts)
    scans, labs, poses = [], [], []
    for b in range(B):
        s, lab = MO.mesh_scan(v, f, p, N, PO.TRUE_POSE, noise=0.05, seed=seed + 10 * b)
        s, lab = s.copy(), lab.copy()
        _spoil(rng, s, lab, n_parts)
        scans.append(s)
        labs.append(lab)
        poses.append(_pose_near(rng, PO.TRUE_POSE))
    return np.stack(scans), np.stack(labs), tri, seg, nrm, n_parts, np.stack(poses)


@pytest.mark.parametrize("level,B,N", [(1, 2, 3001), (2, 3, 1500), (1, 1, 1), (0, 1, 255)])
def test_search_bit_exact_on_the_aircraft(dev, level, B, N):
    scan, lab, tri, seg, nrm, n_parts, pose = _aircraft_case(level, B, max(N, 64), 100 * level + N)
    scan, lab = scan[:, :N].copy(), lab[:, :N].copy()
    pose32 = pose.astype(F32)
    for max_d2 in (np.inf, F32(0.01)):
        out = _raw_correspond(dev, scan, lab, tri, seg, n_parts, pose32, max_d2)
        ei, ed, _ = _check_search(out, scan, lab, tri, seg, n_parts, pose32, max_d2, (level, max_d2))
        if N >= 1500:
            assert (ei >= 0).any() and (ei[np.isfinite(ed)] < 0).any() == np.isfinite(max_d2)      # the cut keeps some, drops some
            assert np.isinf(ed[lab == n_parts - 1]).all() and np.isinf(ed[lab < 0]).all()
            assert np.isnan(out["q"][~np.isfinite(ed)]).all()


def test_search_bit_exact_on_random_triangles(dev):
    rng = np.random.default_rng(5)
    T, n_parts, B, N = 700, 6, 2, 2500
    tri = rng.uniform(-10, 10, (T, 1, 3)).astype(F32) + rng.normal(0, 2.0, (T, 3, 3)).astype(F32)
    tri[:40] = tri[:40, :1] + rng.normal(0, 1e-3, (40, 3, 3)).astype(F32)          # tiny triangles
    tri[40:60, 2] = tri[40:60, 0] + F32(0.999) * (tri[40:60, 1] - tri[40:60, 0])   # needles: nearly collinear in fp32
    lab_t = rng.integers(0, n_parts - 1, T)                                        # the last label stays empty
    faces = np.arange(3 * T).reshape(T, 3)
    g, seg, _, nrm, _ = MO.group_mesh(tri.reshape(-1, 3), faces, lab_t, n_parts)
    scan = rng.uniform(-14, 14, (B, N, 3)).astype(F32)
    lab = rng.integers(0, n_parts - 1, (B, N)).astype(np.int32)
    for b in range(B):
        _spoil(rng, scan[b], lab[b], n_parts)
    pose = np.stack([_pose_near(rng, np.eye(4), rot=0.4, shift=2.0) for _ in range(B)]).astype(F32)
    for max_d2 in (np.inf, F32(1.5)):
        out = _raw_correspond(dev, scan, lab, g, seg, n_parts, pose, max_d2)
        _check_search(out, scan, lab, g, seg, n_parts, pose, max_d2, max_d2)


def _grid_mesh(n=6):
    """a planar integer grid in z = 0, every cell cut along its diagonal, two labels (left and right half): every coordinate, every
    difference, dot and product of the closest-point sequence is a small integer or half-integer, so fp32 is exact there"""
    tri, lab = [], []
    for i in range(n):
        for j in range(n):
            a, b, c, d = [i, j, 0], [i + 1, j, 0], [i + 1, j + 1, 0], [i, j + 1, 0]
            tri += [[a, b, c], [a, c, d]]
            lab += [0 if i < n // 2 else 1] * 2
    return np.array(tri, F32), np.array(lab, np.int32)


def test_exact_ties_go_to_the_lowest_triangle(dev):
    """scan points exactly on shared edges (fp32 midpoints of fp32 vertices) and on shared vertices, on the surface and 3 above it,
    at the identity pose (u = p exactly): the triangles that share the edge or vertex tie exactly in d2"""
    tri, lab_t = _grid_mesh()
    T = len(tri)
    g, seg, _, _, _ = MO.group_mesh(tri.reshape(-1, 3), np.arange(3 * T).reshape(T, 3), lab_t, 2)
    pts, labs = [], []
    for t, l in zip(tri, lab_t):
        for k in range(3):
            mid = (t[k] + t[(k + 1) % 3]) * F32(0.5)
            for p in (mid, t[k]):
                for lift in (0, 3):
                    pts.append(p + np.array([0, 0, lift], F32))
                    labs.append(l)
    # the same on the aircraft (generic coordinates): a vertex is returned as it is, d2 = 0 from every triangle that has it
    v, f, p = MO.aircraft_mesh(1)
    atri, aseg, _, _, _ = MO.group_mesh(v, f, p, NM)
    apts = np.concatenate([atri[:, 0], atri[:, 2], ((atri[:, 0] + atri[:, 1]) * F32(0.5)).astype(F32)])
    alab = np.concatenate([np.repeat(np.arange(NM), np.diff(aseg))] * 3).astype(np.int32)
    eye = np.eye(4, dtype=F32)[None]
    for name, mesh, sg, n_parts, P, L in (("grid", g, seg, 2, np.array(pts, F32), np.array(labs, np.int32)),
                                          ("aircraft", atri, aseg, NM, apts, alab)):
        out = _raw_correspond(dev, P[None], L[None], mesh, sg, n_parts, eye, np.inf)
        ei, ed, _ = _check_search(out, P[None], L[None], mesh, sg, n_parts, eye, np.inf, name)
        # the ties are real: count the same-label triangles that reach the winning d2 bit for bit
        check = np.arange(len(P)) if name == "grid" else np.arange(2 * len(atri))                  # aircraft: the vertex points
        mult = np.zeros(len(P), np.int64)
        for l in range(n_parts):
            rows = check[L[check] == l]
            t = mesh[sg[l]:sg[l + 1]]
            _, d = MO.closest(P[rows, None, :], t[None, :, 0], t[None, :, 1], t[None, :, 2])
            assert np.array_equal(_bits(d.min(1)), _bits(ed[0, rows]))
            mult[rows] = (_bits(d) == _bits(ed[0, rows])[:, None]).sum(1)
            first = np.argmax(_bits(d) == _bits(ed[0, rows])[:, None], axis=1) + sg[l]
            assert np.array_equal(first, ei[0, rows])                                             # the lowest index among them
        if name == "grid":
            assert (mult[check] >= 2).mean() > 0.7 and mult.max() >= 6                             # border edges have one triangle
            assert set(np.unique(ed[0]).tolist()) == {0.0, 9.0}
        else:
            assert (mult[check] >= 2).all() and (ed[0, check] == 0).all()


@pytest.mark.parametrize("B,N", [(1, 777), (3, 5000)])
def test_sums_against_oracle(dev, B, N):
    """both kinds of sums over the pairs the search found, at the tolerance the point and plane references' tests use: 1e-12 of the
    sum of the magnitudes of the terms"""
    scan, lab, tri, seg, nrm, n_parts, pose = _aircraft_case(1, B, N, 7 + N)
    pose32 = pose.astype(F32)
    for max_d2 in (np.inf, F32(0.01)):
        o1 = _raw_correspond(dev, scan, lab, tri, seg, n_parts, pose32, max_d2, mode=1)
        o2 = _raw_correspond(dev, scan, lab, tri, seg, n_parts, pose32, max_d2, mode=2, normals=nrm, pose64=pose)
        ei, _, eq = _check_search(o1, scan, lab, tri, seg, n_parts, pose32, max_d2, "point")
        _check_search(o2, scan, lab, tri, seg, n_parts, pose32, max_d2, "plane")             # the search does not depend on the mode
        qq = np.nan_to_num(eq)
        exp = MO.sums_point(scan, ei, qq)
        mag = MO.sums_point(np.abs(np.nan_to_num(scan)), ei, np.abs(qq))
        assert np.all(np.abs(o1["sums"] - exp) <= 1e-12 * mag), float((np.abs(o1["sums"] - exp) / np.maximum(mag, 1e-300)).max())
        assert (exp[:, 0] == (ei >= 0).sum(1)).all() and (exp[:, 0] > 0).all()
        exp = MO.sums_plane(scan, ei, qq, nrm, pose)
        mag = np.zeros_like(exp)
        iu = np.triu_indices(6)
        for b in range(B):
            k = ei[b] >= 0
            r, a = PO.pair_terms(scan[b][k], qq[b][k], nrm[ei[b][k]], pose[b])
            aa, ar = np.abs(a), np.abs(r)
            mag[b] = np.concatenate([[k.sum()], (aa[:, :, None] * aa[:, None, :]).sum(0)[iu], (aa * ar[:, None]).sum(0), [(ar * ar).sum()]])
        assert np.all(np.abs(o2["sums"] - exp) <= 1e-12 * mag), float((np.abs(o2["sums"] - exp) / np.maximum(mag, 1e-300)).max())


def _scene(dev, level=1, n=6000, noise=0.0, B=1):
    from pointcloudprocessing_amd import ops
    v, f, p = MO.aircraft_mesh(level)
    ref = ops.icp_mesh_reference(v, f, p, NM, device=dev)
    tri, seg, _, nrm, _ = MO.group_mesh(v, f, p, NM)
    scans, labs = zip(*[MO.mesh_scan(v, f, p, n, PO.TRUE_POSE, noise=noise, seed=1 + 5 * b) for b in range(B)])
    return ref, (tri, seg, nrm), np.stack(scans), np.stack(labs)


def test_mesh_reference_on_device_matches_oracle_grouping(dev):
    ref, (tri, seg, nrm), _, _ = _scene(dev)
    assert np.array_equal(ref.tri.cpu().numpy(), tri) and list(ref.seg) == seg.tolist() and np.array_equal(ref.normals.cpu().numpy(), nrm)
    assert ref.tri.is_cuda and ref.normals.is_cuda and ref.area.is_cuda and ref.index.is_cuda


@pytest.mark.parametrize("metric", ["plane", "point"])
def test_loop_against_oracle(dev, metric):
    """the device loop against the oracle's from the 10 degree / 1 m start: the same iterations, pairs and status, the pose within
    the bounds of the existing end-to-end tests (plane 1e-7 rad and 1e-6 m, point 1e-5 rad and 1e-4 m)"""
    from pointcloudprocessing_amd import ops
    ref, (tri, seg, nrm), scan, lab = _scene(dev, noise=0.02)
    kw = dict(max_iters=12, tol_rot=1e-7, tol_t=1e-7)
    g = ops.semantic_icp(_t(scan, dev), _t(lab, dev), ref, _t(PO.START_POSE[None], dev), metric=metric, **kw)
    o = MO.icp(scan, lab, tri, seg, NM, nrm, PO.START_POSE[None], metric=metric, **kw)
    ang, dt = IO.pose_error(g[0][0].cpu().numpy(), o[0][0])
    print(f"{metric}: {int(g[3][0])} iterations, device against oracle {ang:.3e} rad, {dt:.3e} m; against the truth "
          f"{IO.pose_error(g[0][0].cpu().numpy(), PO.TRUE_POSE)}")
    assert int(g[3][0]) == int(o[3][0]) and int(g[4][0]) == int(o[4][0]) and int(g[2][0]) == int(o[2][0]) == 6000
    bound = (1e-7, 1e-6) if metric == "plane" else (1e-5, 1e-4)
    assert ang < bound[0] and dt < bound[1], (ang, dt)
    assert abs(float(g[1][0]) - float(o[1][0])) < 1e-6
    if metric == "plane":
        assert int(g[4][0]) == MO.CONVERGED and int(g[3][0]) <= 10
        tang, tdt = IO.pose_error(g[0][0].cpu().numpy(), PO.TRUE_POSE)
        assert tang < 1e-3 and tdt < 5e-3, (tang, tdt)                       # 2 cm noise over 6,000 points


def test_correspond_ops_wrapper(dev):
    from pointcloudprocessing_amd import ops
    ref, (tri, seg, nrm), scan, lab = _scene(dev, n=2000, noise=0.05, B=2)
    rng = np.random.default_rng(2)
    pose = np.stack([_pose_near(rng, PO.TRUE_POSE) for _ in range(2)])
    S, L = _t(scan, dev), _t(lab, dev)
    idx, d2, q = ops.icp_mesh_correspond(S, L, ref, _t(pose.astype(F32), dev), max_dist=0.1)
    ei, ed, eq = MO.correspond(scan, lab, tri, seg, NM, pose.astype(F32), F32(0.1 * 0.1))
    assert np.array_equal(idx.cpu().numpy(), ei) and np.array_equal(_bits(d2.cpu().numpy()), _bits(ed))
    assert np.array_equal(_bits(q.cpu().numpy()), _bits(eq))
    i2, _, _, s18 = ops.icp_mesh_correspond(S, L, ref, _t(pose, dev), max_dist=0.1, sums="point")
    i3, _, _, s29 = ops.icp_mesh_correspond(S, L, ref, _t(pose, dev), max_dist=0.1, sums="plane")
    assert torch.equal(i2, idx) and torch.equal(i3, idx) and tuple(s18.shape) == (2, 18) and tuple(s29.shape) == (2, 29)
    assert torch.equal(s18[:, 0], s29[:, 0]) and (s18[:, 0].cpu().numpy() == (ei >= 0).sum(1)).all()
    from pointcloudprocessing_amd._lib import PointNetHipError
    with pytest.raises(PointNetHipError, match="fp64"):
        ops.icp_mesh_correspond(S, L, ref, _t(pose.astype(F32), dev), sums="plane")


@pytest.mark.parametrize("metric", ["plane", "point"])
def test_determinism_graph_and_batch(dev, metric):
    from pointcloudprocessing_amd import ops
    ref, _, scan, lab = _scene(dev, level=1, n=20000, noise=0.02, B=3)
    inits = []
    for b in range(3):
        P = PO.TRUE_POSE.copy()
        P[:3, :3] = IO.rot([1, -1, b], np.deg2rad(4 + 3 * b)) @ P[:3, :3]
        P[:3, 3] += [0.3 * b, 0.5, -0.4]
        inits.append(P)
    S, L, I = _t(scan, dev), _t(lab, dev), _t(np.stack(inits), dev)
    keep = [x.clone() for x in (S, L, I, ref.tri, ref.normals)]
    kw = dict(max_iters=10, max_dist=3.0, tol_rot=1e-7, tol_t=1e-7, metric=metric)
    a = ops.semantic_icp(S, L, ref, I, **kw)
    b = ops.semantic_icp(S, L, ref, I, **kw)
    for x, y in zip(a, b):
        assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))
    for i in range(3):
        single = ops.semantic_icp(S[i:i + 1].contiguous(), L[i:i + 1].contiguous(), ref, I[i:i + 1].contiguous(), **kw)
        for x, y in zip(a, single):
            assert np.array_equal(x[i:i + 1].cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.semantic_icp(S, L, ref, I, **kw)
        with torch.cuda.graph(g, stream=side):
            captured = ops.semantic_icp(S, L, ref, I, **kw)
    torch.cuda.current_stream().wait_stream(side)
    for t in captured:
        t.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(a, captured):
        assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))
    for x, y in zip(keep, (S, L, I, ref.tri, ref.normals)):
        assert torch.equal(x, y), "an input was modified"
    assert np.isfinite(a[0].cpu().numpy()).all() and (a[2].cpu().numpy() > 15000).all()


def test_loop_guard_bands_and_few_pairs(dev):
    from pointcloudprocessing_amd import _lib
    _, (tri, seg, nrm), scan, lab = _scene(dev, n=5000, noise=0.02, B=2)
    B, N, T = 2, 5000, len(tri)
    init = np.stack([PO.START_POSE, PO.START_POSE])
    nbytes = _lib.lib().pn_icp_mesh_workspace_bytes(B, N, T, NM)
    ins = [_t(a, dev) for a in (scan, lab, tri, nrm, init)]
    keep = [x.clone() for x in ins]
    for metric, few in ((1, 2), (2, 5)):
        bufs = dict(pose=_guarded((B, 4, 4), torch.float64, dev), rmse=_guarded((B,), torch.float64, dev),
                    pairs=_guarded((B,), torch.int32, dev), iters=_guarded((B,), torch.int32, dev), status=_guarded((B,), torch.int32, dev),
                    ws=_guarded((nbytes,), torch.uint8, dev))
        p = lambda k: C.c_void_p(bufs[k][1].data_ptr())                               # noqa: E731
        lab_m = lab.copy()
        lab_m[1, few:] = -1                                             # scan 1: fewer pairs than the solve needs (3 point, 6 plane)
        ins[1].copy_(_t(lab_m, dev))
        keep[1] = ins[1].clone()
        rc = _lib.lib().pn_semantic_icp_mesh(_lib.ptr(ins[0]), _lib.ptr(ins[1]), B, N, _lib.ptr(ins[2]), _seg_c(seg), T, NM, _lib.ptr(ins[3]),
                                             metric, _lib.ptr(ins[4]), 30, float("inf"), 1e-6, 1e-6, p("pose"), p("rmse"), p("pairs"),
                                             p("iters"), p("status"), p("ws"), nbytes, _lib.current_stream())
        _lib.check(rc, "pn_semantic_icp_mesh")
        torch.cuda.synchronize()
        for name, (buf, _) in bufs.items():
            assert _intact(buf), f"{name}: guard band overwritten"
        for a, b in zip(keep, ins):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "an input was modified"
        out = {k: v.cpu().numpy() for k, (_, v) in bufs.items() if k != "ws"}
        assert out["status"][1] == MO.FEW_PAIRS | MO.CONVERGED and out["iters"][1] == 1 and out["pairs"][1] == few
        assert np.array_equal(out["pose"][1], init[1]) and np.isnan(out["rmse"][1])
        assert 1 < out["iters"][0] <= 30 and np.isfinite(out["rmse"][0]) and out["pairs"][0] == N
        # scan 0 against the oracle's loop.  (With 2 cm noise the plane loop need not meet 1e-6 in 30 iterations: points near a
        # shared edge change triangle from one pass to the next and the specified iteration can enter a short cycle, here of
        # about 0.1 mm; the oracle does the same, so what is asserted is agreement, not convergence.)
        o = MO.icp(scan[:1], lab_m[:1], tri, seg, NM, nrm, init[:1], metric="plane" if metric == 2 else "point", max_iters=30)
        assert out["status"][0] == o[4][0] and out["iters"][0] == o[3][0] and out["pairs"][0] == o[2][0]
        ang, dt = IO.pose_error(out["pose"][0], o[0][0])
        assert (ang < 1e-7 and dt < 1e-6) if metric == 2 else (ang < 1e-5 and dt < 1e-4), (metric, ang, dt)


def test_point_reference_path_is_unchanged(dev):
    """ops.semantic_icp with a point reference is bit for bit pn_semantic_icp / pn_semantic_icp_plane called directly"""
    from pointcloudprocessing_amd import _lib, ops, pointcloud
    xyz, part = pointcloud.read_labelled_cloud(os.path.join(GOLD, "kc-46.txt"), helpers.F15_PARTS)
    ref = ops.icp_reference(xyz, part, NP, device=dev)
    _, _, ref = ops.icp_normals(ref, k=10)
    true = PO.TRUE_POSE
    scan, lab = IO.labelled_scan(xyz, part, 20000, true, noise=0.05, seed=3)
    S, L, I = _t(scan[None], dev), _t(lab[None], dev), _t(PO.START_POSE[None], dev)
    for metric in ("point", "plane"):
        a = ops.semantic_icp(S, L, ref, I, max_iters=10, metric=metric)
        B, N = 1, 20000
        plane = metric == "plane"
        nbytes = (_lib.lib().pn_icp_plane_workspace_bytes if plane else _lib.lib().pn_icp_workspace_bytes)(B, N, ref.M, NP)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        pose = I.clone()
        rmse = torch.empty(B, dtype=torch.float64, device=dev)
        pairs, iters, status = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
        pt = _lib.ptr
        if plane:
            rc = _lib.lib().pn_semantic_icp_plane(pt(S), pt(L), B, N, pt(ref.xyz), ref._seg_c, ref.M, NP, pt(pose), 10, float("inf"), 1e-6,
                                                  1e-6, pt(ref.normals), pt(pose), pt(rmse), pt(pairs), pt(iters), pt(status), pt(ws), nbytes,
                                                  _lib.current_stream())
        else:
            rc = _lib.lib().pn_semantic_icp(pt(S), pt(L), B, N, pt(ref.xyz), ref._seg_c, ref.M, NP, pt(pose), 10, float("inf"), 1e-6, 1e-6,
                                            pt(pose), pt(rmse), pt(pairs), pt(iters), pt(status), pt(ws), nbytes, _lib.current_stream())
        _lib.check(rc, "pn_semantic_icp")
        torch.cuda.synchronize()
        for x, y in zip(a, (pose, rmse, pairs, iters, status)):
            assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8)), metric
        assert int(a[2][0]) > 15000 and np.isfinite(float(a[1][0]))


# ---------------------------------------------------------------------------------------------------------------------
# the seams of the shared walk: both reference kinds run one kernel over batches of U primitives (8 points, 4 triangles) and a
# one-at-a-time tail
# ---------------------------------------------------------------------------------------------------------------------
SEAM_PARTS = 5
SEAM_N = 130                  # two full waves and a third of two lanes
# labels per scan in the order the kernel buckets them; 3 is the label whose segment is empty, -1 and 7 lie outside [0, 5).  Scan 0:
# wave 0 holds labels 0, 1 and 2, wave 1 labels 2 and 4 and the points that take no part, wave 2 only such points.  Scan 1: every
# point takes part; wave 0 holds labels 0 and 1, wave 1 labels 1, 2 and 4, and the two lanes of wave 2 label 4.
SEAM_LABELS = (((0, 20), (1, 22), (2, 41), (4, 40), (3, 3), (-1, 2), (7, 2)), ((0, 3), (1, 70), (2, 10), (4, 47)))


def _seam_lengths(U):
    """segment lengths 1, U - 1, U, 0, U + 1: from a range's start the boundary between the batches and the tail falls inside a
    segment, at its end and one primitive past it"""
    return (1, U - 1, U, 0, U + 1)


def _seam_case(kind):
    """(scan (2, 130, 3), labels, reference, seg, normals, pose64) from a seeded generator, checked on the CPU through the oracle
    alone before use"""
    rng = np.random.default_rng(31 if kind == "cloud" else 37)
    lengths = _seam_lengths(8 if kind == "cloud" else 4)
    part = np.repeat(np.arange(SEAM_PARTS), lengths)
    part = part[rng.permutation(len(part))]
    if kind == "cloud":
        ref, seg, _ = IO.group_reference(rng.uniform(-4, 4, (len(part), 3)).astype(F32), part, SEAM_PARTS)
        nrm = rng.normal(size=ref.shape)
        nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F32)
    else:
        v = (rng.uniform(-4, 4, (len(part), 1, 3)) + rng.normal(0, 1.5, (len(part), 3, 3))).astype(F32).reshape(-1, 3)
        ref, seg, _, nrm, _ = MO.group_mesh(v, np.arange(len(v)).reshape(-1, 3), part, SEAM_PARTS)
    assert tuple(np.diff(seg)) == lengths
    scan = rng.uniform(-4, 4, (2, SEAM_N, 3)).astype(F32)
    lab = np.stack([np.concatenate([np.full(c, l) for l, c in row])[rng.permutation(SEAM_N)] for row in SEAM_LABELS]).astype(np.int32)
    k = np.flatnonzero(lab[0] == 1)
    scan[0, k[0]] = np.nan                                        # non-finite points with a good label
    scan[0, k[1], 2] = np.inf
    pose = np.stack([_pose_near(rng, np.eye(4), rot=0.3, shift=1.0) for _ in range(2)])
    # every label that has primitives has a query, and the waves are what SEAM_LABELS says
    act = IO.active(scan, lab, seg, SEAM_PARTS)
    assert act[0].sum() == SEAM_N - 9 and act[1].all()
    for b in range(2):
        assert all((act[b] & (lab[b] == l)).any() for l in range(SEAM_PARTS) if lengths[l])
        order = np.concatenate([np.flatnonzero(act[b] & (lab[b] == l)) for l in range(SEAM_PARTS)])
        waves = [sorted(set(lab[b][order[w:w + 64]])) for w in range(0, len(order), 64)]
        assert waves == ([[0, 1, 2], [2, 4]] if b == 0 else [[0, 1], [1, 2, 4], [4]])
    # no two candidates of a query tie: the d2 of every primitive on its own, from the oracle
    one = np.zeros(SEAM_PARTS + 1, np.int64)
    for l in range(SEAM_PARTS):
        cand = []
        for j in range(seg[l], seg[l + 1]):
            one[l + 1:] = 1
            out = (IO.correspond if kind == "cloud" else MO.correspond)(scan, lab, ref[j:j + 1], one, SEAM_PARTS, pose.astype(F32))
            cand.append(_bits(out[1])[act & (lab == l)])
            one[:] = 0
        if cand:
            cand = np.sort(np.stack(cand), axis=0)
            assert (cand[1:] != cand[:-1]).all()
    return scan, lab, ref, seg, nrm, pose


SEAM_CASES = {}


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("kind", ["cloud", "mesh"])
def test_walk_seams_both_reference_kinds(dev, kind, mode):
    """B = 2, N = 130 against segments of 1, U - 1, U, 0 and U + 1 primitives, with labels outside the range, an empty label and
    non-finite points: idx and d2 (and q against a mesh) bit for bit the oracle's in every mode, the sums at the tolerance of
    test_sums_against_oracle and tests/test_gpu_icp_plane.py (1e-12 of the sum of the magnitudes of the terms)"""
    from pointcloudprocessing_amd import ops
    if kind not in SEAM_CASES:
        SEAM_CASES[kind] = _seam_case(kind)
    scan, lab, ref, seg, nrm, pose = SEAM_CASES[kind]
    pose32 = pose.astype(F32)
    iu = np.triu_indices(6)
    for max_dist in (float("inf"), 2.0):
        max_d2 = F32(max_dist * max_dist)
        if kind == "cloud":
            ei, ed = IO.correspond(scan, lab, ref, seg, SEAM_PARTS, pose32, max_d2)
            r = ops.IcpReference(_t(ref, dev), seg, torch.arange(len(ref), device=dev), SEAM_PARTS, normals=_t(nrm, dev))
            if mode == 2:
                got = ops.icp_plane_sums(_t(scan, dev), _t(lab, dev), r, _t(pose, dev), max_dist=max_dist)
            else:
                got = ops.icp_correspond(_t(scan, dev), _t(lab, dev), r, _t(pose32, dev), max_dist=max_dist, sums=mode == 1)
            out = dict(zip(("idx", "d2", "sums"), (g.cpu().numpy() for g in got)))
            assert np.array_equal(out["idx"], ei), np.argwhere(out["idx"] != ei)[:5]
            assert np.array_equal(_bits(out["d2"]), _bits(ed)), np.argwhere(_bits(out["d2"]) != _bits(ed))[:5]
            eq = ref[np.maximum(ei, 0)]
        else:
            out = _raw_correspond(dev, scan, lab, ref, seg, SEAM_PARTS, pose32, max_d2, mode=mode, normals=nrm if mode == 2 else None,
                                  pose64=pose if mode == 2 else None)
            ei, ed, eq = _check_search(out, scan, lab, ref, seg, SEAM_PARTS, pose32, max_d2, (kind, mode, max_dist))
            eq = np.nan_to_num(eq)
        assert (ei >= 0).any(1).all() and np.isinf(ed[~IO.active(scan, lab, seg, SEAM_PARTS)]).all()
        assert (ei[np.isfinite(ed)] < 0).any() == np.isfinite(max_dist)                           # the cut keeps some, drops some
        if mode == 1:
            exp = MO.sums_point(scan, ei, eq)
            mag = MO.sums_point(np.abs(np.nan_to_num(scan)), ei, np.abs(eq))
        elif mode == 2:
            exp = MO.sums_plane(scan, ei, eq, nrm, pose)
            mag = np.zeros_like(exp)
            for b in range(2):
                k = ei[b] >= 0
                rr, a = PO.pair_terms(scan[b][k], eq[b][k], nrm[ei[b][k]], pose[b])
                aa, ar = np.abs(a), np.abs(rr)
                mag[b] = np.concatenate([[k.sum()], (aa[:, :, None] * aa[:, None, :]).sum(0)[iu], (aa * ar[:, None]).sum(0), [(ar * ar).sum()]])
        if mode:
            err = np.abs(out["sums"] - exp) / np.maximum(mag, 1e-300)
            print(f"{kind} mode {mode} max_dist {max_dist}: worst sums error {err.max():.3e} of the magnitudes")
            assert np.all(np.abs(out["sums"] - exp) <= 1e-12 * mag), float(err.max())
            assert (exp[:, 0] == (ei >= 0).sum(1)).all()


def _bench_scan():
    spec = importlib.util.spec_from_file_location("bench_scan", os.path.join(ROOT, "tools", "bench_scan.py"))
    bs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bs)
    return bs


@pytest.mark.parametrize("metric", ["plane", "point"])
def test_predict_pose_mesh_c5_composition(dev, metric):
    """BASELINE config 5 at full size (131,072 points): predict_pose(mesh reference) returns a finite pose and equals
    predict_scan -> initial_pose -> semantic_icp(mesh)"""
    from oracle import pointnet_oracle as O            # checker only
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd.pointnet.PointNet import PointNet
    bs = _bench_scan()
    xyz, origin = bs.make_scan(131072)
    x = torch.from_numpy(xyz).to(dev)
    model = PointNet(23, 12, 0.3, 42, precision="bf16", device=dev)
    model.set_weights(O.init_params(23, 12, seed=31, randomize_bn=True))
    v, f, p = MO.aircraft_mesh(1)
    mp = (np.arange(len(f)) % NP).astype(np.int32)                     # every part label of the model gets triangles
    ref = ops.icp_mesh_reference(v, f, mp, NP, device=dev)
    ci, part, pose, rmse, pairs = model.predict_pose(x, ref, leaf=0.25, samples=8192, k=3, origin=origin, max_iters=10, metric=metric)
    ci2, part2, R = model.predict_scan(x, leaf=0.25, samples=8192, k=3, origin=origin)
    assert torch.equal(ci, ci2) and torch.equal(part, part2)
    P0 = PointNet.initial_pose(x, part2, R, ref)
    p2, r2, n2, _, _ = ops.semantic_icp(x.unsqueeze(0), part2, ref, P0, max_iters=10, metric=metric)
    assert torch.equal(pose, p2) and torch.equal(rmse, r2) and torch.equal(pairs, n2) and int(pairs[0]) > 100000
    assert np.isfinite(pose.cpu().numpy()).all() and np.isfinite(float(rmse[0]))
    Rf = pose[0, :3, :3].cpu().numpy()
    assert np.abs(Rf @ Rf.T - np.eye(3)).max() < 1e-12
    # the mesh branch of initial_pose: the area-weighted centroid of the triangles of the shared labels
    lab = part2[0].cpu().numpy()
    shared = np.intersect1d(np.unique(lab[(lab >= 0) & (lab < NP)]), np.unique(mp))
    tri, seg, order, _, area = MO.group_mesh(v, f, mp, NP)
    use = np.isin(mp[order], shared)
    c_ref = (tri.astype(np.float64).mean(1) * area[:, None])[use].sum(0) / area[use].sum()
    c_scan = xyz[np.isin(lab, shared)].astype(np.float64).mean(0)
    P0n = P0[0].cpu().numpy()
    assert np.abs(P0n[:3, 3] - (c_scan - P0n[:3, :3] @ c_ref)).max() < 1e-9
