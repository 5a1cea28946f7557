"""pn_lidar_cast / pn_lidar_pack on the MI355X: hit row and range bit for bit against the NumPy oracle (tests/lidar_oracle.py), zero
excluded rays, on the procedural aircraft, on random triangles, on the integer wall whose ties are exact, at the seams of the walk's
batches of four triangles, with NaN inputs and range limits; the packed clouds bit for bit in the three regimes; determinism (eager,
graph replay, batch against single frames); guard bands around every output and the workspace; occlusion; and the closure of a
rendered frame with semantic ICP and with PointCloudSet."""
import ctypes as C

import numpy as np
import pytest
import torch

import icp_mesh_oracle as MO
import icp_oracle as IO
import lidar_oracle as LO
import test_cpu_lidar as CL

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 4096
PAT = 0xA5
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
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _finish(bufs, keep, ins):
    torch.cuda.synchronize()
    for name, (buf, _) in bufs.items():
        assert _intact(buf), f"{name}: guard band overwritten"
    for a, b in zip(keep, ins):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "an input was modified"
    return {k: v.cpu().numpy() for k, (_, v) in bufs.items() if k != "ws"}


def _raw_cast(dev, tri, seg, n_parts, poses, dirs, t_min=0.0, t_max=np.inf):
    """pn_lidar_cast through the C ABI with guard bands around both outputs; the inputs must come back untouched"""
    from pointcloudprocessing_amd import _lib
    tri = np.asarray(tri, F32).reshape(-1, 3, 3)
    B, R, T = len(poses), len(dirs), len(tri)
    ins = [_t(a, dev) for a in (tri if T else np.zeros((1, 3, 3), F32), np.asarray(poses, F32), np.asarray(dirs, F32))]
    keep = [x.clone() for x in ins]
    bufs = dict(hit=_guarded((B, R), torch.int32, dev), t=_guarded((B, R), torch.float32, dev))
    p = lambda k: C.c_void_p(bufs[k][1].data_ptr())                                   # noqa: E731
    rc = _lib.lib().pn_lidar_cast(_lib.ptr(ins[0]) if T else None, _seg_c(seg), T, n_parts, _lib.ptr(ins[1]), B, _lib.ptr(ins[2]), R,
                                  float(t_min), float(t_max), p("hit"), p("t"), _lib.current_stream())
    _lib.check(rc, "pn_lidar_cast")
    return _finish(bufs, keep, ins)


def _raw_pack(dev, hit, t, dirs, seg, n_parts, N):
    """pn_lidar_pack through the C ABI with guard bands around the four outputs and the workspace"""
    from pointcloudprocessing_amd import _lib
    B, R = hit.shape
    ins = [_t(a, dev) for a in (np.asarray(hit, np.int32), np.asarray(t, F32), np.asarray(dirs, F32))]
    keep = [x.clone() for x in ins]
    nbytes = _lib.lib().pn_lidar_workspace_bytes(B, R)
    bufs = dict(xyz=_guarded((B, N, 3), torch.float32, dev), part=_guarded((B, N), torch.int32, dev), ray=_guarded((B, N), torch.int32, dev),
                count=_guarded((B,), torch.int32, dev), ws=_guarded((nbytes,), torch.uint8, dev))
    p = lambda k: C.c_void_p(bufs[k][1].data_ptr())                                   # noqa: E731
    rc = _lib.lib().pn_lidar_pack(_lib.ptr(ins[0]), _lib.ptr(ins[1]), _lib.ptr(ins[2]), B, R, _seg_c(seg), int(seg[n_parts]), n_parts, N,
                                  p("xyz"), p("part"), p("ray"), p("count"), p("ws"), nbytes, _lib.current_stream())
    _lib.check(rc, "pn_lidar_pack")
    return _finish(bufs, keep, ins)


def _check_cast(out, tri, poses, dirs, t_min=0.0, t_max=np.inf, name=""):
    eh, et = LO.cast(tri, poses, dirs, t_min, t_max)
    assert np.array_equal(out["hit"], eh), (name, np.argwhere(out["hit"] != eh)[:5])
    assert np.array_equal(_bits(out["t"]), _bits(et)), (name, np.argwhere(_bits(out["t"]) != _bits(et))[:5])
    return eh, et


def _check_pack(out, hit, t, dirs, seg, n_parts, N, name=""):
    exp = dict(zip(("xyz", "part", "ray", "count"), LO.pack(hit, t, dirs, seg, n_parts, N)))
    for k in ("count", "ray", "part"):
        assert np.array_equal(out[k], exp[k]), (name, k, np.argwhere(out[k] != exp[k])[:5])
    same = (_bits(out["xyz"]) == _bits(exp["xyz"])) | (np.isnan(out["xyz"]) & np.isnan(exp["xyz"]))
    assert same.all(), (name, np.argwhere(~same)[:5])
    return exp


def _views(level, n_views=3, height=37, width=29):
    """the aircraft with one more label than it has (an empty segment), three poses and 37 x 29 = 1,073 rays: a multiple of neither
    64 nor 256"""
    tri, seg, poses, dirs = CL.aircraft_views(level, n_views=n_views, height=height, width=width)
    return tri, np.concatenate([seg, seg[-1:]]), NM + 1, poses.astype(F32), dirs


@pytest.mark.parametrize("level,t_min,t_max", [(0, 0.0, np.inf), (1, 0.0, np.inf), (1, 52.0, 61.5)])
def test_cast_bit_exact_on_the_aircraft(dev, level, t_min, t_max):
    tri, seg, n_parts, poses, dirs = _views(level)
    dirs = dirs.copy()
    dirs[517, 1] = np.nan                                         # a NaN direction: that ray misses in every frame
    out = _raw_cast(dev, tri, seg, n_parts, poses, dirs, t_min, t_max)
    eh, et = _check_cast(out, tri, poses, dirs, t_min, t_max, (level, t_min, t_max))
    full, _ = LO.cast(tri, poses, dirs)
    assert ((eh >= 0).sum(1) > 20).all() and (eh[:, 517] == -1).all() and np.isinf(et[eh < 0]).all()
    if np.isfinite(t_max):
        assert ((full >= 0) & (eh < 0)).any() and (et[eh >= 0] >= t_min).all() and (et[eh >= 0] <= t_max).all()      # the limits cut
    nan_pose = poses.copy()
    nan_pose[1, 2, 0] = np.nan                                    # a NaN pose row: frame 1 sees nothing, the others are unchanged
    out2 = _raw_cast(dev, tri, seg, n_parts, nan_pose, dirs, t_min, t_max)
    _check_cast(out2, tri, nan_pose, dirs, t_min, t_max, "nan pose")
    assert (out2["hit"][1] == -1).all() and np.array_equal(out2["hit"][[0, 2]], eh[[0, 2]])


def _random_triangles(rng, T):
    c = rng.normal(size=(T, 1, 3)) * [20.0, 12.0, 12.0] + [45.0, 0.0, 0.0]
    return (c + rng.normal(0, 3.0, (T, 3, 3))).astype(F32)


def test_cast_bit_exact_on_random_triangles(dev):
    rng = np.random.default_rng(17)
    T, n_parts = 700, 5
    tri = _random_triangles(rng, T)
    tri[:30] = tri[:30, :1] + rng.normal(0, 1e-2, (30, 3, 3)).astype(F32)                     # tiny triangles
    tri[30:50, 2] = tri[30:50, 0] + F32(0.999) * (tri[30:50, 1] - tri[30:50, 0])             # needles: nearly collinear in fp32
    seg = np.array([0, 100, 100, 350, 699, 700])
    poses = np.stack([np.eye(4)] * 2)
    for b in range(2):
        poses[b, :3, :3] = IO.rot(rng.normal(size=3), 0.2)
        poses[b, :3, 3] = rng.normal(size=3) * 2.0
    dirs = CL.aircraft_views(0, n_views=1, height=37, width=29)[3]
    for t_min, t_max in ((0.0, np.inf), (30.0, 47.0)):
        out = _raw_cast(dev, tri, seg, n_parts, poses.astype(F32), dirs, t_min, t_max)
        eh, _ = _check_cast(out, tri, poses.astype(F32), dirs, t_min, t_max, (t_min, t_max))
        assert ((eh >= 0).mean(1) > 0.2).all() and (eh < 0).any()


@pytest.mark.parametrize("T", [0, 1, 3, 4, 5])
def test_cast_seams_of_the_walk(dev, T):
    """batches of U = 4 triangles and a one-at-a-time tail: T = 0 (every ray misses), below, at and above one batch; 130 rays = two
    full waves and one of two lanes"""
    rng = np.random.default_rng(23)
    tri = (_random_triangles(rng, 5) * F32(0.5) + rng.normal(0, 8.0, (5, 3, 3)).astype(F32))[:T]     # large: most rays hit several
    dirs = CL.aircraft_views(0, n_views=1, height=10, width=13)[3]
    poses = np.eye(4, dtype=F32)[None].repeat(2, 0)
    poses[1, :3, 3] = [1.0, -0.5, 0.25]
    seg = np.array([0, min(T, 2), T])
    out = _raw_cast(dev, tri, seg, 2, poses, dirs)
    eh, _ = _check_cast(out, tri, poses, dirs, name=T)
    assert (eh == -1).all() if T == 0 else (T - 1 in eh and 0 in eh and (eh == -1).any())       # the last triangle wins somewhere


def test_exact_ties_go_to_the_lowest_row(dev):
    g, seg, dirs, exp, t, mult = CL.wall_case()
    eye = np.eye(4, dtype=F32)[None]
    out = _raw_cast(dev, g, seg, 2, eye, dirs)
    _check_cast(out, g, eye, dirs, name="wall")
    assert np.array_equal(out["hit"][0], exp) and np.array_equal(_bits(out["t"][0]), _bits(t)) and mult.max() == 6
    tri, cseg, cdirs = CL.coincident_case()
    for order in (slice(None), slice(None, None, -1)):
        out = _raw_cast(dev, tri[order], cseg, 2, eye, cdirs)
        assert out["hit"][0].tolist() == [0, 0, -1] and out["t"][0].tolist() == [5.0, 5.0, np.inf]
    tri, edirs = CL.edge_case_rays()
    up, down = np.nextafter(F32(8), F32(np.inf)), np.nextafter(F32(8), F32(0))
    for t_min, t_max, seen in ((0.0, np.inf, True), (8.0, np.inf, True), (up, np.inf, False), (0.0, 8.0, True), (0.0, down, False),
                               (8.0, 8.0, True)):
        out = _raw_cast(dev, tri, [0, len(tri)], 1, eye, edirs, t_min, t_max)
        _check_cast(out, tri, eye, edirs, t_min, t_max, (t_min, t_max))
        assert (out["hit"][0, 0] >= 0) == seen and out["hit"][0, 1:].tolist() == [-1, -1, -1]


@pytest.mark.parametrize("N", [64, 1711, 2048, 4096])
def test_pack_bit_exact_in_the_three_regimes(dev, N):
    """2,500 rays (three chunks of the compaction, the last one short), four frames in one batch: 1,711 hits (more than, exactly and
    fewer than N), 17 hits, none, and all 2,500"""
    hit, t, dirs, seg, n_parts = CL.pack_case(R=2500, n0=1711)
    out = _raw_pack(dev, hit, t, dirs, seg, n_parts, N)
    exp = _check_pack(out, hit, t, dirs, seg, n_parts, N, N)
    assert exp["count"].tolist() == [1711, 17, 0, 2500]
    assert np.isnan(out["xyz"][2]).all() and (out["part"][2] == -1).all() and (out["ray"][2] == -1).all()


def test_more_frames_than_the_grid_has_rows(dev):
    """B = 65,605 frames of 3 rays: the frames beyond the launch grid's y limit (65,535) follow in a stride.  All frames share one
    pose but three (the first past the limit, one further on, the last), so the oracle runs on four poses"""
    tri, _ = LO.wall_mesh(8, -1, 1, -1, 1)
    seg = [0, 3, len(tri)]
    dirs = np.array([[1.0, 0.03125, 0.0625], [1.0, 0.5, 0.0], [1.0, -0.09375, 0.03125]], F32)
    B = 65535 + 70
    poses = np.eye(4, dtype=F32)[None].repeat(B, 0)
    special = {65535: [0.0, 0.75, 0.0], 65600: [1.0, 0.0, -0.5], B - 1: [-2.0, 0.25, 0.25]}
    for b, t in special.items():
        poses[b, :3, 3] = t
    out = _raw_cast(dev, tri, seg, 2, poses, dirs)
    rows = [0] + list(special)
    eh, et = LO.cast(tri, poses[rows], dirs)
    assert np.array_equal(out["hit"][rows], eh) and np.array_equal(_bits(out["t"][rows]), _bits(et))
    plain = np.setdiff1d(np.arange(B), rows)
    assert (out["hit"][plain] == eh[0]).all() and (_bits(out["t"][plain]) == _bits(et[0])).all()
    assert len({tuple(h) for h in eh}) >= 3 and (eh[0] >= 0).any() and (eh[0] < 0).any()
    pk = _raw_pack(dev, out["hit"], out["t"], dirs, seg, 2, 2)
    e4 = LO.pack(eh, et, dirs, seg, 2, 2)
    for k, e in zip(("xyz", "part", "ray", "count"), e4):
        assert np.array_equal(pk[k][rows], e, equal_nan=True), k
        assert (pk[k][plain] == e[0]).all(), k


def test_frames_pipeline_against_oracle(dev):
    """ops.lidar_frames = cast + pack on real returns: level 1, three poses (one looking away: a frame that sees nothing)"""
    from pointcloudprocessing_amd import ops
    tri, seg, n_parts, poses, dirs = _views(1)
    poses = poses.astype(np.float64)
    poses[2, :3, :3] = np.diag([-1.0, -1.0, 1.0]) @ poses[2, :3, :3]                        # turned about z: the aircraft behind it
    poses[2, :3, 3] = np.diag([-1.0, -1.0, 1.0]) @ poses[2, :3, 3]
    v, f, p = MO.aircraft_mesh(1)
    ref = ops.icp_mesh_reference(v, f, p, NM + 1, device=dev)
    eh, et = LO.cast(tri, poses.astype(F32), dirs)
    assert (eh[2] == -1).all() and (eh[0] >= 0).sum() > 50
    for N in (32, 512):
        xyz, part, ray, count = ops.lidar_frames(ref, poses, dirs, N)
        out = dict(xyz=xyz.cpu().numpy(), part=part.cpu().numpy(), ray=ray.cpu().numpy(), count=count.cpu().numpy())
        _check_pack(out, eh, et, dirs, seg, n_parts, N, N)
    hit, t = ops.lidar_cast(ref, _t(poses.astype(F32), dev), _t(dirs, dev), t_min=1.0)
    assert np.array_equal(hit.cpu().numpy(), eh) and np.array_equal(_bits(t.cpu().numpy()), _bits(et))


def test_determinism_graph_and_batch(dev):
    from pointcloudprocessing_amd import ops
    tri, seg, n_parts, poses, dirs = _views(1)
    v, f, p = MO.aircraft_mesh(1)
    ref = ops.icp_mesh_reference(v, f, p, NM + 1, device=dev)
    P, D = _t(poses, dev), _t(dirs, dev)
    keep = [x.clone() for x in (P, D, ref.tri)]
    N = 256

    def run(pp):
        hit, t = ops.lidar_cast(ref, pp, D)
        return (hit, t) + ops.lidar_pack(ref, hit, t, D, N)

    same = lambda x, y: np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))    # noqa: E731
    a, b = run(P), run(P)
    assert all(same(x, y) for x, y in zip(a, b))
    for i in range(3):
        single = run(P[i:i + 1].contiguous())
        assert all(same(x[i:i + 1], y) for x, y in zip(a, single))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(P)
        with torch.cuda.graph(g, stream=side):
            captured = run(P)
    torch.cuda.current_stream().wait_stream(side)
    for x in captured:
        x.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    assert all(same(x, y) for x, y in zip(a, captured))
    for x, y in zip(keep, (P, D, ref.tri)):
        assert torch.equal(x, y), "an input was modified"
    assert (a[5].cpu().numpy() > 50).all()


def test_occlusion(dev):
    """a 2 m wall at 8 m in front of a 12 m wall at 16 m: every return inside the small wall's silhouette carries its label and its
    range, none reaches the far wall there.  And on the aircraft from the side no return lies behind the nearest fp64 hit of its
    ray by more than the fp32 range error (3 x CL.T_ERR_MEASURED)."""
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd.pointcloud import look_at_pose, pinhole_rays
    near, _ = LO.wall_mesh(8, -1, 1, -1, 1)
    far, _ = LO.wall_mesh(16, -6, 6, -6, 6)
    tri = np.concatenate([far, near])                                                  # the far wall first: order does not decide
    part = np.concatenate([np.ones(len(far), np.int32), np.zeros(len(near), np.int32)])
    ref = ops.icp_mesh_reference(tri.reshape(-1, 3), np.arange(3 * len(tri)).reshape(-1, 3), part, 2, device=dev)
    dirs = pinhole_rays(41, 53, 40.0, 40.0)
    N = 41 * 53
    xyz, lab, ray, count = (x.cpu().numpy()[0] for x in ops.lidar_frames(ref, np.eye(4)[None], dirs, N))
    assert count == N                                                                   # every ray of the 40 degree grid meets the far wall
    d = dirs[ray].astype(np.float64)
    y8, z8 = 8 * d[:, 1] / d[:, 0], 8 * d[:, 2] / d[:, 0]
    inside = (np.abs(y8) < 1 - 1e-5) & (np.abs(z8) < 1 - 1e-5)
    outside = (np.abs(y8) > 1 + 1e-5) | (np.abs(z8) > 1 + 1e-5)
    assert inside.sum() > 100 and outside.sum() > 1000
    assert (lab[inside] == 0).all() and np.abs(xyz[inside, 0] - 8).max() < 1e-5
    assert (lab[outside] == 1).all() and np.abs(xyz[outside, 0] - 16).max() < 1e-5
    # the aircraft from the side (the sensor on the model's y axis): wing, fuselage and fin overlap in the image
    v, f, p = MO.aircraft_mesh(1)
    aref = ops.icp_mesh_reference(v, f, p, NM, device=dev)
    g, _, _, _, _ = MO.group_mesh(v, f, p, NM)
    pose = look_at_pose([0.0, 60.0, 4.0])[None]
    adirs = pinhole_rays(48, 64, 50.0, 40.0)
    hit, t = (x.cpu().numpy() for x in ops.lidar_cast(aref, pose, adirs))
    _, t64, _ = LO.cast_fp64(g, pose.astype(F32), adirs)
    k = hit[0] >= 0
    assert k.sum() > 200 and len(np.unique(p[aref.index.cpu().numpy()][hit[0][k]])) >= 3
    assert (t[0][k] <= t64[0][k] + 3 * CL.T_ERR_MEASURED).all()


def test_closure_with_semantic_icp(dev):
    """a one-sided frame of aircraft_mesh(1) rendered at a known pose, registered by ops.semantic_icp(metric="point") against the
    same mesh reference from about 5 degrees / 0.5 m off with the true labels: the device pose agrees with the oracle's loop on the
    same frame within the bound of tests/test_gpu_icp_mesh.py::test_loop_against_oracle (1e-5 rad, 1e-4 m), and its error to the
    true pose is at most twice the oracle's own (the iteration paths may differ in the last bits).  The oracle's own error after
    these 30 iterations, computed on the CPU: 2.2e-5 rad and 2.5e-2 m (point to point slides slowly along a one-sided frame: after
    60 iterations it is 1.7e-6 rad and 1.7e-3 m)."""
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd.pointcloud import look_at_pose, pinhole_rays
    v, f, p = MO.aircraft_mesh(1)
    ref = ops.icp_mesh_reference(v, f, p, NM, device=dev)
    tri, seg, _, nrm, _ = MO.group_mesh(v, f, p, NM)
    true = look_at_pose([38.0, 41.0, 22.0])
    dirs = pinhole_rays(64, 96, 40.0, 28.0)
    xyz, part, _, count = ops.lidar_frames(ref, true[None], dirs, 1024)
    assert int(count[0]) > 1024                                                         # an even stride over the image
    scan, lab = xyz.cpu().numpy(), part.cpu().numpy()
    start = true.copy()
    start[:3, :3] = IO.rot([1.0, -2.0, 0.5], np.deg2rad(5.0)) @ true[:3, :3]
    start[:3, 3] += [0.3, -0.3, 0.25]
    kw = dict(max_iters=30, tol_rot=1e-7, tol_t=1e-7)
    g = ops.semantic_icp(xyz, part, ref, _t(start[None], dev), metric="point", **kw)
    o = MO.icp(scan, lab, tri, seg, NM, nrm, start[None], metric="point", **kw)
    ang, dt = IO.pose_error(g[0][0].cpu().numpy(), o[0][0])
    g_err, o_err = IO.pose_error(g[0][0].cpu().numpy(), true), IO.pose_error(o[0][0], true)
    print(f"{int(g[3][0])} iterations (oracle {int(o[3][0])}), device against oracle {ang:.3e} rad, {dt:.3e} m; against the truth: "
          f"device {g_err[0]:.3e} rad {g_err[1]:.3e} m, oracle {o_err[0]:.3e} rad {o_err[1]:.3e} m")
    assert ang < 1e-5 and dt < 1e-4, (ang, dt)
    assert g_err[0] <= 2 * o_err[0] and g_err[1] <= 2 * o_err[1], (g_err, o_err)
    assert int(g[2][0]) == int(o[2][0]) == 1024


def test_closure_with_the_dataset(dev, tmp_path):
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd.pointcloud import look_at_pose, pinhole_rays, sample_viewpoints, simulate_dataset
    from pointcloudprocessing_amd.pointcloud.PointCloudSet import PointCloudSet
    v, f, p = MO.aircraft_mesh(1)
    ref = ops.icp_mesh_reference(v, f, p, NM, device=dev)
    vp = sample_viewpoints(12, (45.0, 80.0), (0.0, 360.0), (-5.0, 20.0), seed=2)
    vp = np.concatenate([vp, [[0.0, 0.0, 1.0e4]]])                                     # too far for any ray to meet the aircraft
    dirs = pinhole_rays(32, 48, 50.0, 36.0)
    msgs = []
    W = 128
    obs, cls, parts, se3 = simulate_dataset(ref, 3, vp, dirs, W, roll_deg=10.0, t_max=500.0, print_func=msgs.append)
    assert obs.shape == (12, W, 3) and obs.dtype == np.float32 and cls.shape == (12,) and cls.dtype == np.int32 and (cls == 3).all()
    assert parts.shape == (12, W) and parts.dtype == np.int32 and parts.min() >= 0 and parts.max() < NM
    assert se3.shape == (12, 3, 3) and se3.dtype == np.float32 and np.isfinite(obs).all()
    assert len(msgs) == 1 and "1 of 13" in msgs[0] and "[12]" in msgs[0]
    rots = np.stack([look_at_pose(x, 10.0)[:3, :3] for x in vp[:12]]).astype(F32)
    assert np.array_equal(se3, rots)
    names = ["c%d" % i for i in range(5)]
    pcs = PointCloudSet("sim", names, list(MO.MESH_PARTS), W, batch_size=4, rand_seed=5, data_path=str(tmp_path) + "/",
                        print_func=lambda s: None)
    pcs.add_data("aircraft", obs, cls, parts, se3)
    x, y = next(pcs.get_train_set(device="cuda"))
    assert x.is_cuda and x.shape == (4, W, 3) and x.dtype == torch.float32
    assert y["classification_output"].shape == (4,) and (y["classification_output"] == 3).all()
    seg_y = y["segmentation_output"]
    assert seg_y.shape == (4, W) and seg_y.dtype == torch.int32 and int(seg_y.min()) >= 0 and int(seg_y.max()) < NM
    r = y["se3"].cpu().numpy()
    assert r.shape == (4, 3, 3) and all(any(np.array_equal(q, s) for s in rots) for q in r)
    xs = x.cpu().numpy()
    assert all(any(np.array_equal(q, s) for s in obs) for q in xs)                      # no jitter: the frames as rendered
