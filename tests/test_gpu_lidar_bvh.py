"""pn_lidar_cast_bvh on the MI355X: hit row and range bit for bit against the tree oracle (tests/lidar_bvh_oracle.py) and against
the brute-force device entry pn_lidar_cast, through the raw C ABI with guard bands: on the procedural aircraft with a NaN direction
and a NaN pose, on random, tiny and needle triangles, on exact ties and range limits, at the seams of the tree's shape, at 20,480
triangles, with more frames than the grid has rows; determinism (eager, graph replay, a batch against the single frames); and the
accel= keyword of ops.lidar_cast, ops.lidar_frames and pointcloud.simulate_dataset."""
import ctypes as C

import numpy as np
import pytest
import torch

import icp_bvh_oracle as BO
import icp_mesh_oracle as MO
import lidar_bvh_oracle as TO
import lidar_oracle as LO
import test_cpu_lidar as CL
import test_cpu_lidar_bvh as CB

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 4096
PAT = 0xA5
NM = len(MO.MESH_PARTS)
EYE = CB.EYE


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


def _raw_cast(dev, tri, seg, n_parts, poses, dirs, t_min=0.0, t_max=np.inf, tree=None):
    """pn_lidar_cast_bvh (``tree`` = (nodes, rows, roots)) or pn_lidar_cast (None) through the C ABI with guard bands around both
    outputs; the inputs must come back untouched"""
    from pointcloudprocessing_amd import _lib
    tri = np.asarray(tri, F32).reshape(-1, 3, 3)
    B, R, T = len(poses), len(dirs), len(tri)
    arrays = [tri if T else np.zeros((1, 3, 3), F32), np.asarray(poses, F32), np.asarray(dirs, F32)]
    if tree is not None:
        arrays += [tree[0].view(np.int32).reshape(-1, 8), np.asarray(tree[1], np.int32)]
    ins = [_t(a, dev) for a in arrays]
    keep = [x.clone() for x in ins]
    bufs = dict(hit=_guarded((B, R), torch.int32, dev), t=_guarded((B, R), torch.float32, dev))
    p = lambda k: C.c_void_p(bufs[k][1].data_ptr())                                   # noqa: E731
    args = (_lib.ptr(ins[0]) if T else None, _seg_c(seg), T, n_parts, _lib.ptr(ins[1]), B, _lib.ptr(ins[2]), R, float(t_min), float(t_max),
            p("hit"), p("t"))
    if tree is None:
        _lib.check(_lib.lib().pn_lidar_cast(*args, _lib.current_stream()), "pn_lidar_cast")
    else:
        _lib.check(_lib.lib().pn_lidar_cast_bvh(*args, _lib.ptr(ins[3]), _lib.ptr(ins[4]), _seg_c(tree[2]), len(tree[0]),
                                                _lib.current_stream()), "pn_lidar_cast_bvh")
    torch.cuda.synchronize()
    for name, (buf, _) in bufs.items():
        assert _intact(buf), f"{name}: guard band overwritten"
    for a, b in zip(keep, ins):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "an input was modified"
    return {k: v.cpu().numpy() for k, (_, v) in bufs.items()}


def _same(name, got, hit, t):
    assert np.array_equal(got["hit"], hit), (name, np.argwhere(got["hit"] != hit)[:5])
    assert np.array_equal(_bits(got["t"]), _bits(t)), (name, np.argwhere(_bits(got["t"]) != _bits(t))[:5])


def _both(dev, name, tri, seg, n_parts, poses, dirs, t_min, t_max, tree, oracle=None):
    """the tree entry against the tree oracle (computed here unless given) and against the brute-force device entry"""
    got = _raw_cast(dev, tri, seg, n_parts, poses, dirs, t_min, t_max, tree=tree)
    brute = _raw_cast(dev, tri, seg, n_parts, poses, dirs, t_min, t_max)
    oh, ot = (oracle or TO.cast(tri, poses, dirs, *tree, t_min, t_max))[:2]
    _same((name, "oracle"), got, oh, ot)
    _same((name, "brute"), got, brute["hit"], brute["t"])
    return got


@pytest.mark.parametrize("level", [1, 3])
def test_cast_bit_exact_on_the_aircraft(dev, level):
    tri, seg, n_parts, poses, dirs = CB.aircraft_scene(level)
    tree = CB.aircraft_tree(level)
    for t_min, t_max in CB.AIRCRAFT_RANGES:
        got = _both(dev, (level, t_min, t_max), tri, seg, n_parts, poses, dirs, t_min, t_max, tree, CB.aircraft_oracle(level, t_min, t_max))
        assert ((got["hit"] >= 0).sum(1) > 20).all() and (got["hit"][:, CB.NAN_RAY] == -1).all() and np.isinf(got["t"][got["hit"] < 0]).all()
    if level == 1:
        nan_pose = poses.copy()
        nan_pose[1, 2, 0] = np.nan                                # a NaN pose row: frame 1 sees nothing, the others are unchanged
        first = _raw_cast(dev, tri, seg, n_parts, poses, dirs, tree=tree)
        got = _both(dev, "nan pose", tri, seg, n_parts, nan_pose, dirs, 0.0, np.inf, tree)
        assert (got["hit"][1] == -1).all() and np.array_equal(got["hit"][[0, 2]], first["hit"][[0, 2]])


def test_cast_bit_exact_on_random_triangles(dev):
    tri, seg, n_parts, poses, dirs = CB.random_scene()
    for t_min, t_max in CB.RANDOM_RANGES:
        got = _both(dev, (t_min, t_max), tri, seg, n_parts, poses, dirs, t_min, t_max, CB.random_tree())
        assert ((got["hit"] >= 0).mean(1) > 0.2).all() and (got["hit"] < 0).any()


def test_exact_ties_and_range_limits(dev):
    for name, tri, seg, n_parts, dirs, ranges in CB.exact_scenes():
        tree = BO.build(tri, seg, n_parts)
        for t_min, t_max in ranges:
            got = _both(dev, (name, t_min, t_max), tri, seg, n_parts, EYE, dirs, t_min, t_max, tree)
        if name == "wall":
            assert np.array_equal(got["hit"][0], CL.wall_case()[3])
        if name.startswith("coincident"):
            assert got["hit"][0].tolist() == [0, 0, -1] and got["t"][0].tolist() == [5.0, 5.0, np.inf]


@pytest.mark.parametrize("T", [0, 1, 4, 5, 9])
def test_cast_seams_of_the_tree(dev, T):
    """a root that is a leaf (T = 1), a full leaf (4), the first split (5), two levels (9), all in label 0 with label 1 empty, and no
    triangle at all (no tree: every ray misses); 130 rays = two full waves and one of two lanes"""
    rng = np.random.default_rng(23)
    c = rng.normal(size=(9, 1, 3)) * [10.0, 6.0, 6.0] + [45.0, 0.0, 0.0]
    tri = (c + rng.normal(0, 8.0, (9, 3, 3))).astype(F32)[:T]                        # large: most rays hit several
    dirs = CL.aircraft_views(0, n_views=1, height=10, width=13)[3]
    poses = np.eye(4, dtype=F32)[None].repeat(2, 0)
    poses[1, :3, 3] = [1.0, -0.5, 0.25]
    seg = np.array([0, T, T])
    if T == 0:
        from pointcloudprocessing_amd import _lib
        P, D = _t(poses, dev), _t(dirs, dev)
        hit, t = torch.zeros(2, 130, dtype=torch.int32, device=dev), torch.zeros(2, 130, device=dev)
        _lib.check(_lib.lib().pn_lidar_cast_bvh(None, _seg_c(seg), 0, 2, _lib.ptr(P), 2, _lib.ptr(D), 130, 0.0, float("inf"), _lib.ptr(hit),
                                                _lib.ptr(t), None, None, _seg_c([-1, -1]), 0, _lib.current_stream()), "pn_lidar_cast_bvh")
        assert bool((hit == -1).all()) and bool(torch.isinf(t).all())
        return
    tree = BO.build(tri, seg, 2)
    depth = BO.check_tree(tri, seg, 2, *tree)[0]
    assert depth == {1: 0, 4: 0, 5: 1, 9: 2}[T] and tree[2][1] == -1
    got = _both(dev, T, tri, seg, 2, poses, dirs, 0.0, np.inf, tree)
    assert T - 1 in got["hit"] and 0 in got["hit"] and (got["hit"] == -1).any()


def test_level_4_against_the_brute_force_entry(dev):
    """20,480 triangles: the tree entry against pn_lidar_cast, the same bytes"""
    v, f, p = MO.aircraft_mesh(4)
    tri, seg, _, _, _ = MO.group_mesh(v, f, p, NM)
    _, _, _, poses, dirs = CB.aircraft_scene(1)
    tree = BO.build(tri, seg, NM)
    got = _raw_cast(dev, tri, seg, NM, poses, dirs, tree=tree)
    brute = _raw_cast(dev, tri, seg, NM, poses, dirs)
    assert got["hit"].tobytes() == brute["hit"].tobytes() and got["t"].tobytes() == brute["t"].tobytes()
    assert len(tri) == 20480 and ((got["hit"] >= 0).sum(1) > 20).all()


def test_more_frames_than_the_grid_has_rows(dev):
    """B = 65,537 frames of 3 rays: the frames beyond the launch grid's y limit (65,535) follow in a stride.  All frames share one
    pose but two (the first past the limit and the last), so the oracle runs on three poses"""
    tri, _ = LO.wall_mesh(8, -1, 1, -1, 1)
    seg = [0, 3, len(tri)]
    dirs = np.array([[1.0, 0.03125, 0.0625], [1.0, 0.5, 0.0], [1.0, -0.09375, 0.03125]], F32)
    B = 65537
    poses = np.eye(4, dtype=F32)[None].repeat(B, 0)
    special = {65535: [0.0, 0.75, 0.0], B - 1: [-2.0, 0.25, 0.25]}
    for b, t in special.items():
        poses[b, :3, 3] = t
    tree = BO.build(tri, seg, 2)
    out = _raw_cast(dev, tri, seg, 2, poses, dirs, tree=tree)
    rows = [0] + list(special)
    eh, et = TO.cast(tri, poses[rows], dirs, *tree)[:2]
    bh, bt = LO.cast(tri, poses[rows], dirs)
    assert np.array_equal(eh, bh) and np.array_equal(_bits(et), _bits(bt))
    assert np.array_equal(out["hit"][rows], eh) and np.array_equal(_bits(out["t"][rows]), _bits(et))
    plain = np.setdiff1d(np.arange(B), rows)
    assert (out["hit"][plain] == eh[0]).all() and (_bits(out["t"][plain]) == _bits(et[0])).all()
    assert len({tuple(h) for h in eh}) == 3 and (eh[0] >= 0).any() and (eh[0] < 0).any()


def _refs(dev, level=1):
    from pointcloudprocessing_amd import ops
    v, f, p = MO.aircraft_mesh(level)
    return ops.icp_mesh_reference(v, f, p, NM + 1, device=dev), ops.icp_mesh_reference(v, f, p, NM + 1, device=dev, accel="bvh")


def _bytes_equal(a, b):
    return all(np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8)) for x, y in zip(a, b))


def test_determinism_graph_and_batch(dev):
    from pointcloudprocessing_amd import ops
    _, _, _, poses, dirs = CB.aircraft_scene(1)
    plain, acc = _refs(dev)
    P, D = _t(poses, dev), _t(dirs, dev)
    keep = [x.clone() for x in (P, D, acc.tri, acc.nodes, acc.rows)]
    run = lambda pp: ops.lidar_cast(acc, pp, D, accel="bvh")                           # noqa: E731
    a, b = run(P), run(P)
    assert _bytes_equal(a, b) and _bytes_equal(a, ops.lidar_cast(plain, P, D))
    for i in range(3):
        assert _bytes_equal([x[i:i + 1] for x in a], run(P[i:i + 1].contiguous())), i
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
    assert _bytes_equal(a, captured)
    assert _bytes_equal(keep, (P, D, acc.tri, acc.nodes, acc.rows)), "an input was modified"      # bytes: D holds a NaN
    assert ((a[0] >= 0).sum(1) > 20).all()


class _Spy:
    """the library handle with the names of the entries called through it"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self._lib, name)


def test_the_accel_keyword(dev, monkeypatch):
    from pointcloudprocessing_amd import _lib, ops, pointcloud
    _, _, _, poses, dirs = CB.aircraft_scene(1)
    plain, acc = _refs(dev)
    want = ops.lidar_cast(plain, poses, dirs, t_min=1.0, t_max=70.0)
    assert _bytes_equal(want, ops.lidar_cast(acc, poses, dirs, t_min=1.0, t_max=70.0, accel="bvh")) and int((want[0] >= 0).sum()) > 100
    for N in (32, 512):
        assert _bytes_equal(ops.lidar_frames(plain, poses, dirs, N), ops.lidar_frames(acc, poses, dirs, N, accel="bvh")), N
    vp = pointcloud.sample_viewpoints(5, (45.0, 80.0), (0.0, 360.0), (-5.0, 20.0), seed=2)
    vp = np.concatenate([vp, [[0.0, 0.0, 1.0e4]]])                                     # too far for any ray to meet the aircraft
    kw = dict(roll_deg=10.0, t_max=500.0, print_func=None)
    a = pointcloud.simulate_dataset(plain, 3, vp, dirs, 128, **kw)
    b = pointcloud.simulate_dataset(acc, 3, vp, dirs, 128, accel="bvh", **kw)
    assert len(a[0]) == 5 and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))
    for fn in (lambda: ops.lidar_cast(plain, poses, dirs, accel="bvh"), lambda: ops.lidar_frames(plain, poses, dirs, 32, accel="bvh")):
        with pytest.raises(_lib.PointNetHipError, match=r'icp_mesh_reference\(\.\.\., accel="bvh"\)'):
            fn()
    with pytest.raises(_lib.PointNetHipError, match="accel must be"):
        ops.lidar_cast(acc, poses, dirs, accel="grid")
    spy = _Spy(_lib.lib())
    monkeypatch.setattr(ops, "lib", lambda: spy)
    none = ops.lidar_cast(acc, poses, dirs)                                            # the default: today's call, whatever the reference
    tree = ops.lidar_cast(acc, poses, dirs, accel="bvh")
    monkeypatch.undo()
    assert spy.calls == ["pn_lidar_cast", "pn_lidar_cast_bvh"] and _bytes_equal(none, tree)
