"""pn_mesh_sample on the MI355X: points, rows and parts bit for bit against the NumPy oracle (tests/mesh_sample_oracle.py) with guard
bands around every output and the workspace; purity (set offsets, graph replay); ops.mesh_sample_reference and point-to-plane ICP
against it; ops.global_pose with a sampled score cloud against the oracle composition; pointcloud.sample_dataset."""
import ctypes as C

import numpy as np
import pytest
import torch

import icp_global_oracle as GO
import icp_mesh_oracle as MO
import icp_oracle as IO
import icp_plane_oracle as PO
import mesh_sample_oracle as SO

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 4096
PAT = 0xA5
NM = SO.NM


def _guarded(shape, dtype, dev):
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((GUARD + n + GUARD,), PAT, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + n].view(dtype).view(*shape)


def _intact(buf):
    return bool((buf[:GUARD] == PAT).all()) and bool((buf[-GUARD:] == PAT).all())


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _raw_sample(dev, tri, area, seg, n_parts, n, seed=0, sets=1, set0=0):
    """pn_mesh_sample through the C ABI with guard bands around the three outputs and the workspace; the inputs must come back
    untouched"""
    from pointcloudprocessing_amd import _lib
    tri = np.asarray(tri, F32).reshape(-1, 3, 3)
    T = len(tri)
    ins = [_t(tri if T else np.zeros((1, 3, 3), F32), dev), _t(np.asarray(area, np.float64) if T else np.zeros(1), dev)]
    keep = [x.clone() for x in ins]
    nbytes = _lib.lib().pn_mesh_sample_workspace_bytes(T, sets, n)
    assert nbytes > 0
    bufs = dict(xyz=_guarded((sets, n, 3), torch.float32, dev), row=_guarded((sets, n), torch.int32, dev),
                part=_guarded((sets, n), torch.int32, dev), ws=_guarded((nbytes,), torch.uint8, dev))
    p = lambda k: C.c_void_p(bufs[k][1].data_ptr())                                   # noqa: E731
    seg_c = (C.c_int32 * len(seg))(*[int(v) for v in seg])
    rc = _lib.lib().pn_mesh_sample(_lib.ptr(ins[0]) if T else None, _lib.ptr(ins[1]) if T else None, seg_c, T, n_parts, seed, set0, sets, n,
                                   p("xyz"), p("row"), p("part"), p("ws"), nbytes, _lib.current_stream())
    _lib.check(rc, "pn_mesh_sample")
    torch.cuda.synchronize()
    for name, (buf, _) in bufs.items():
        assert _intact(buf), f"{name}: guard band overwritten"
    for a, b in zip(keep, ins):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "an input was modified"
    return {k: v.cpu().numpy() for k, (_, v) in bufs.items() if k != "ws"}


def _check(out, tri, area, seg, n_parts, n, seed=0, sets=1, set0=0, name=""):
    xyz, part, row = SO.mesh_sample(tri, area, seg, n_parts, n, seed, sets, set0)
    assert np.array_equal(out["row"], row), (name, np.argwhere(out["row"] != row)[:5])
    assert np.array_equal(out["part"], part), (name, np.argwhere(out["part"] != part)[:5])
    same = (_bits(out["xyz"]) == _bits(xyz)) | (np.isnan(out["xyz"]) & np.isnan(xyz))
    assert same.all(), (name, np.argwhere(~same)[:5])
    return xyz, part, row


@pytest.mark.parametrize("sets", [1, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_bit_exact_on_the_aircraft(dev, n, sets):
    tri, seg, _, area = SO.aircraft(0)
    for seed in (0, 7, (1 << 63) + 5):
        out = _raw_sample(dev, tri, area, seg, NM, n, seed, sets)
        _, part, row = _check(out, tri, area, seg, NM, n, seed, sets, name=(n, sets, seed))
        assert row.min() >= 0 and (np.diff(row, axis=1) >= 0).all() and (part >= 0).all()


def test_bit_exact_beyond_one_scan_chunk(dev):
    """5,120 triangles: five chunks of the prefix sum; 4,096 samples: sixteen blocks, windows of about 80 rows; with one more label
    than the mesh has (an empty segment) and a set offset"""
    tri, seg, _, area = SO.aircraft(3)
    assert len(tri) == 5120
    seg5 = np.concatenate([seg, seg[-1:]])
    out = _raw_sample(dev, tri, area, seg5, NM + 1, 4096, 11, 2, 40)
    _, part, row = _check(out, tri, area, seg5, NM + 1, 4096, 11, 2, 40)
    assert len(np.unique(row[0])) > 2000 and part.max() == NM - 1
    # few samples on many triangles: the window of a wave is wider than its slice of LDS
    out = _raw_sample(dev, tri, area, seg, NM, 100, 5)
    _check(out, tri, area, seg, NM, 100, 5, name="wide window")


def test_single_triangle_and_no_triangle(dev):
    tri = np.array([[[1, 2, 3], [4, 2, 3], [1, 7, 5]]], F32)
    area = MO.group_mesh(tri.reshape(-1, 3), np.arange(3).reshape(1, 3), [0], 1)[4]
    out = _raw_sample(dev, tri, area, [0, 1], 1, 300, 9, 2)
    _check(out, tri, area, [0, 1], 1, 300, 9, 2)
    assert (out["row"] == 0).all() and (out["part"] == 0).all()
    out = _raw_sample(dev, np.zeros((0, 3, 3), F32), np.zeros(0), [0, 0, 0], 2, 70, 1, 2)
    assert (out["row"] == -1).all() and (out["part"] == -1).all() and np.isnan(out["xyz"]).all()


def test_negligible_and_invalid_areas(dev):
    tri, seg, _, area = SO.aircraft(0)
    n = 1000
    base = SO.mesh_sample(tri, area, seg, NM, n, 3)
    mid = 46                                                      # the wing's upper skin, in the middle of the rows
    # the middle triangle shrunk about its first corner to 2^-15 of its size, 2^-30 of its area: weight 0, never drawn
    small = tri.copy()
    small[mid, 1:] = small[mid, :1] + (small[mid, 1:] - small[mid, :1]) * F32(2.0 ** -15)
    part_of_row = SO.part_of(np.arange(len(tri)), seg, NM)
    tiny = MO.group_mesh(small.reshape(-1, 3), np.arange(3 * len(tri)).reshape(-1, 3), part_of_row, NM)[4]
    assert len(tiny) == len(tri) and 0 < tiny[mid] < area.max() * 2.0 ** -29 and SO.weights(tiny)[mid] == 0 and np.array_equal(np.delete(tiny, mid), np.delete(area, mid))
    out = _raw_sample(dev, small, tiny, seg, NM, n, 3)
    _check(out, small, tiny, seg, NM, n, 3, name="tiny")
    assert (base[2] == mid).any() and not (out["row"] == mid).any()
    zero = area.copy()
    zero[mid] = 0.0
    assert np.array_equal(out["row"], SO.mesh_sample(tri, zero, seg, NM, n, 3)[2])            # the others: as if it had no area at all
    # a NaN, a zero, a negative and an infinite entry: none of them is drawn and none disturbs the maximum
    bad = area.copy()
    bad[[3, 17, 40, 61]] = [np.nan, 0.0, -5.0, np.inf]
    out = _raw_sample(dev, tri, bad, seg, NM, n, 3)
    _check(out, tri, bad, seg, NM, n, 3, name="bad")
    assert not np.isin(out["row"], [3, 17, 40, 61]).any() and out["row"].min() >= 0
    none = np.full(len(tri), np.nan)
    none[5] = -1.0
    out = _raw_sample(dev, tri, none, seg, NM, 65, 3)
    assert (out["row"] == -1).all() and (out["part"] == -1).all() and np.isnan(out["xyz"]).all()


@pytest.fixture(scope="module")
def aircraft_ref(dev):
    from pointcloudprocessing_amd import ops
    v, f, p = MO.aircraft_mesh(0)
    return ops.icp_mesh_reference(v, f, p, NM, device=dev)


def test_sets_are_pure_and_replay_from_a_graph(dev, aircraft_ref):
    from pointcloudprocessing_amd import ops
    n = 1000
    a = ops.mesh_sample(aircraft_ref, n, seed=7, sets=3)
    b = ops.mesh_sample(aircraft_ref, n, seed=7, sets=2, set0=1)
    for x, y in zip(a, b):
        assert torch.equal(x[1:], y)
    assert a[0].shape == (3, n, 3) and a[1].dtype == torch.int32 and a[2].dtype == torch.int32
    assert not torch.equal(a[2][0], a[2][1])
    tri, seg, _, area = SO.aircraft(0)
    xyz, part, row = SO.mesh_sample(tri, area, seg, NM, n, 7, 3)
    assert np.array_equal(_bits(a[0].cpu().numpy()), _bits(xyz)) and np.array_equal(a[1].cpu().numpy(), part)
    assert np.array_equal(a[2].cpu().numpy(), row)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.mesh_sample(aircraft_ref, n, seed=7, sets=3)                                       # warm up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g = ops.mesh_sample(aircraft_ref, n, seed=7, sets=3)
    for x in g:
        x.fill_(0)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(a, g):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    with pytest.raises(ops._lib.PointNetHipError, match="pn_mesh_sample"):
        ops.mesh_sample(aircraft_ref, 0)
    with pytest.raises(ops._lib.PointNetHipError, match="mesh_ref"):
        ops.mesh_sample(ops.icp_reference(np.zeros((4, 3), F32), np.zeros(4, np.int32), NM, device=dev), 10)


def test_mesh_sample_reference_and_plane_icp(dev, aircraft_ref):
    """the sampled cloud as a reference: seg counted from part, normals the face normals of row; point-to-plane ICP against it from
    5 degrees / 0.5 m off on a full-surface scan agrees with the oracle loop on the same cloud within what
    tests/test_gpu_icp_plane.py holds the device loop to (1e-7 rad, 1e-6 m; iterations and status equal, pairs within 2)"""
    from pointcloudprocessing_amd import ops
    tri, seg, nrm, area = SO.aircraft(0)
    n = 3000
    r = ops.mesh_sample_reference(aircraft_ref, n, seed=5)
    xyz, cseg, row, normals = SO.sample_reference(tri, area, seg, NM, nrm, n, 5)
    assert isinstance(r, ops.IcpReference) and r.n_parts == NM and r.seg == tuple(int(v) for v in cseg) and r.M == n
    assert np.array_equal(_bits(r.xyz.cpu().numpy()), _bits(xyz)) and np.array_equal(r.index.cpu().numpy(), row) and r.index.dtype == torch.int64
    assert np.array_equal(_bits(r.normals.cpu().numpy()), _bits(normals))
    assert torch.equal(r.normals, aircraft_ref.normals[r.index])
    part = np.repeat(np.arange(NM), np.diff(r.seg))
    assert np.array_equal(part, SO.part_of(row, seg, NM))
    v, f, p = MO.aircraft_mesh(0)
    T = np.eye(4)
    T[:3, :3] = IO.rot([0.3, -0.5, 0.8], np.deg2rad(25))
    T[:3, 3] = [4.0, -7.0, 12.0]
    scan, lab = MO.mesh_scan(v, f, p, 2000, pose=T, noise=0.01, seed=2)
    init = np.eye(4)
    init[:3, :3] = IO.rot([1.0, 1.0, -0.5], np.deg2rad(5)) @ T[:3, :3]
    init[:3, 3] = T[:3, 3] + [0.3, -0.3, 0.26]
    kw = dict(max_iters=8, tol_rot=1e-9, tol_t=1e-9)
    g = ops.semantic_icp(_t(scan[None], dev), _t(lab[None], dev), r, _t(init[None], dev), metric="plane", **kw)
    o = PO.icp(scan[None], lab[None], xyz, cseg, NM, normals, init[None], **kw)
    ang, dt = IO.pose_error(g[0][0].cpu().numpy(), o[0][0])
    tang, tdt = IO.pose_error(o[0][0], T)
    print(f"plane ICP against the sampled reference: device against oracle {ang:.3e} rad {dt:.3e} m; oracle against the truth {tang:.3e} rad "
          f"{tdt:.3e} m")
    assert ang < 1e-7 and dt < 1e-6, (ang, dt)
    assert int(g[3][0]) == int(o[3][0]) and int(g[4][0]) == int(o[4][0]) and abs(int(g[2][0]) - int(o[2][0])) <= 2
    assert tang < GO.CAP_ROT and tdt < GO.CAP_T


def test_global_pose_with_a_score_cloud(dev, aircraft_ref):
    """the seed-3 one-sided case, where the vertex score loses the right seed: the device's top-4 set and winner are the oracle
    composition's, its pose lies inside CAP_ROT / CAP_T of the truth and as close to the oracle's as tests/test_gpu_icp_global.py
    requires (1e-5 rad, 1e-4 m)"""
    from pointcloudprocessing_amd import ops
    scan, lab, T = SO.one_sided_case(3)
    o = SO.solved(3, True)
    cloud = ops.mesh_sample_reference(aircraft_ref, SO.SCORE_N, SO.SCORE_SEED)
    assert np.array_equal(_bits(cloud.xyz.cpu().numpy()), _bits(SO.score_cloud(0)[0]))
    S, L = _t(scan[None], dev), _t(lab[None], dev)
    rot = ops.rotation_grid(256)
    pose, rmse, pairs, iters, status, cost, winner = ops.global_pose(S, L, aircraft_ref, GO.MAX_DIST, rotations=rot, score_cloud=cloud,
                                                                     **GO.PARAMS)
    seeds = ops.icp_seed_poses(ops.part_moments(S, L, NM), ops.icp_part_moments(aircraft_ref), rot.to(dev))
    _, order = ops.icp_score_poses(S, L, cloud, seeds, GO.MAX_DIST, stride=GO.PARAMS["stride"])
    assert sorted(order[0, :4].tolist()) == sorted(o["top"][0].tolist())
    g = pose.cpu().numpy()[0]
    ang, dt = IO.pose_error(g, o["pose"][0])
    tang, tdt = IO.pose_error(g, T)
    print(f"winner {int(winner[0])} (oracle {int(o['winner'][0])}), against the oracle {ang:.3e} rad {dt:.3e} m, against the truth "
          f"{tang:.3e} rad {tdt:.3e} m, cost {float(cost[0]):.6f} (oracle {o['cost'][0]:.6f})")
    assert int(winner[0]) == int(o["winner"][0])
    assert ang < 1e-5 and dt < 1e-4, (ang, dt)
    assert tang < GO.CAP_ROT and tdt < GO.CAP_T, (tang, tdt)
    # the default is unchanged: the vertex score, which on this case ends far from the truth, as the oracle's does
    vpose, _, _, _, _, _, vwinner = ops.global_pose(S, L, aircraft_ref, GO.MAX_DIST, rotations=rot, **GO.PARAMS)
    assert int(vwinner[0]) == int(SO.solved(3, False)["winner"][0]) and IO.pose_error(vpose.cpu().numpy()[0], T)[0] > 1.0
    # what a score cloud must be
    kc = ops.icp_reference(np.zeros((4, 3), F32), np.zeros(4, np.int32), NM, device=dev)
    with pytest.raises(ops._lib.PointNetHipError, match="score_cloud"):
        ops.global_pose(S, L, kc, GO.MAX_DIST, score_cloud=cloud)                              # goes with a mesh reference only
    with pytest.raises(ops._lib.PointNetHipError, match="score_cloud"):
        ops.global_pose(S, L, aircraft_ref, GO.MAX_DIST, score_cloud=ops.icp_reference(np.zeros((4, 3), F32), np.zeros(4, np.int32), NM + 1, device=dev))
    with pytest.raises(ops._lib.PointNetHipError, match="score_cloud"):
        ops.global_pose(S, L, aircraft_ref, GO.MAX_DIST, score_cloud=aircraft_ref)


def test_sample_dataset(dev, aircraft_ref):
    """3 viewpoints x 64 points: shapes, dtypes and class ids; se3 the look-at rotations; the points taken back to the model frame
    lie on their triangles within the sampler's bound (16 * 2^-24 * M per coordinate, tests/test_cpu_mesh_sample.py: sqrt(3) times
    that as a distance) plus the transform's rounding: p = R q + t rounds once, every coordinate by at most 2^-24 of itself, so the
    error vector is at most 2^-24 |p| <= 2^-24 (sqrt(3) M + |t|) long, |t| <= 80 m; the way back runs in fp64"""
    from pointcloudprocessing_amd import pointcloud
    tri, seg, nrm, area = SO.aircraft(0)
    vp = pointcloud.sample_viewpoints(3, (45.0, 80.0), seed=4)
    roll = np.array([0.0, 20.0, -35.0])
    obs, cls, part, se3 = pointcloud.sample_dataset(aircraft_ref, 6, vp, 64, roll_deg=roll, seed=12)
    assert obs.shape == (3, 64, 3) and obs.dtype == F32 and cls.dtype == np.int32 and cls.tolist() == [6, 6, 6]
    assert part.shape == (3, 64) and part.dtype == np.int32 and se3.shape == (3, 3, 3) and se3.dtype == F32
    poses = np.stack([pointcloud.look_at_pose(v, r) for v, r in zip(vp, roll)])
    assert np.array_equal(se3, poses[:, :3, :3].astype(F32))
    xyz, epart, row = SO.mesh_sample(tri, area, seg, NM, 64, 12, 3)
    assert np.array_equal(part, epart)
    M = float(np.abs(tri).max())
    rounding = 2.0 ** -24 * (np.sqrt(3.0) * M + 80.0)
    bound = np.sqrt(3.0) * 16 * 2.0 ** -24 * M + rounding
    for i in range(3):
        q = (obs[i].astype(np.float64) - poses[i, :3, 3]) @ poses[i, :3, :3]                    # R^T (p - t)
        t = tri[row[i]].astype(np.float64)
        d = np.array([np.sqrt(MO.closest_fp64(q[k], t[k, 0], t[k, 1], t[k, 2])[1]) for k in range(64)])
        assert d.max() <= bound, (i, d.max(), bound)
        assert np.abs(q - xyz[i]).max() <= rounding
    raw = pointcloud.sample_dataset(aircraft_ref, 6, vp, 64, roll_deg=roll, seed=12, reproject=False)
    assert np.array_equal(_bits(raw[0]), _bits(xyz)) and np.array_equal(raw[2], part) and np.array_equal(raw[3], se3)
    again = pointcloud.sample_dataset(aircraft_ref, 6, vp, 64, roll_deg=roll, seed=12)
    for x, y in zip((obs, cls, part, se3), again):
        assert np.array_equal(x, y)
    other = pointcloud.sample_dataset(aircraft_ref, 6, vp, 64, roll_deg=roll, seed=13)
    assert not np.array_equal(other[0], obs) and not np.array_equal(other[2], part)
    assert not np.array_equal(obs[0], obs[1])                                                   # one independent set per frame
    empty = pointcloud.sample_dataset(aircraft_ref, 6, np.zeros((0, 3)), 64)
    assert empty[0].shape == (0, 64, 3) and empty[3].shape == (0, 3, 3)
