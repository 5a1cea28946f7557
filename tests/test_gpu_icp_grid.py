"""pn_icp_grid_build / pn_icp_grid_correspond / pn_semantic_icp_grid on the MI355X: the search through the voxel grid against the
brute-force device entries on the same grouped cloud (pn_icp_correspond / pn_icp_plane_sums / pn_semantic_icp /
pn_semantic_icp_plane) and against the NumPy oracle (tests/icp_grid_oracle.py), by the contract of include/pointnet_hip.h: idx
everywhere, d2 and q bit for bit within the tables' r2 and (-1, +inf, NaN) beyond it, zero excluded queries; through the C ABI with
guard bands round every output, the tables and both workspaces, inputs and tables untouched by a search; the sums byte for byte;
the loops, their graph replay and the batch against single scans; and the higher-level calls that take a grid reference.  The
inputs of the single-pass cases are checked on the oracle alone in tests/test_cpu_icp_grid.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import helpers
import icp_grid_oracle as GO
import icp_mesh_oracle as MO
import icp_oracle as IO
import icp_plane_oracle as PO

pytestmark = pytest.mark.gpu
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


def _vp(t):
    return C.c_void_p(t.data_ptr())


def _build(dev, ref, r2, origin):
    """pn_icp_grid_build through the C ABI on a device cloud, guard bands round the tables and the workspace -> (guarded buffer,
    tables); the error word must be 0 and the reference untouched"""
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    M = ref.shape[0]
    keep = ref.clone()
    gbuf, grid = _guarded((L.pn_icp_grid_bytes(M),), torch.uint8, dev)
    nws = L.pn_icp_grid_build_workspace_bytes(M)
    wbuf, ws = _guarded((nws,), torch.uint8, dev)
    assert grid.data_ptr() % 16 == 0 and ws.data_ptr() % 16 == 0
    _lib.check(L.pn_icp_grid_build(_lib.ptr(ref), M, float(r2), (C.c_float * 3)(*[float(v) for v in origin]), _vp(grid), grid.numel(), _vp(ws),
                                   nws, _lib.current_stream()), "pn_icp_grid_build")
    torch.cuda.synchronize()
    assert _intact(gbuf) and _intact(wbuf), "pn_icp_grid_build: guard band overwritten"
    assert int(ws[:4].view(torch.int32).item()) == 0 and torch.equal(keep, ref)
    head = grid[:32].cpu().numpy()
    assert head[:8].view(np.int32)[1] == M and head[8:16].view(F32).tolist() == [F32(r2), GO.leaf(r2)]
    assert head[16:28].view(F32).tolist() == [F32(v) for v in origin]
    return gbuf, grid


def _raw(dev, c, max_d2, mode=0, normals=None, pose64=None, grid=None, q_out=True):
    """pn_icp_grid_correspond (``grid``: the tables) or the brute-force pn_icp_correspond / pn_icp_plane_sums through the C ABI, with
    guard bands round every output and the workspace; the inputs and the tables must come back untouched"""
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    scan, lab, ref, seg, n_parts = c["scan"], c["lab"], c["ref"], c["seg"], c["n_parts"]
    B, N, _ = scan.shape
    M = len(ref)
    ins = [None if a is None else _t(a, dev) for a in (scan, lab, ref, c["pose"].astype(F32), normals, pose64)]
    keep = [None if x is None else x.clone() for x in ins] + ([grid.clone()] if grid is not None else [])
    nbytes = (L.pn_icp_plane_workspace_bytes if grid is not None or mode == 2 else L.pn_icp_workspace_bytes)(B, N, M, n_parts)
    bufs = dict(idx=_guarded((B, N), torch.int32, dev), d2=_guarded((B, N), torch.float32, dev), q=_guarded((B, N, 3), torch.float32, dev),
                sums=_guarded((B, 29 if mode == 2 else 18), torch.float64, dev), ws=_guarded((nbytes,), torch.uint8, dev))
    p = lambda k: _vp(bufs[k][1])                                                     # noqa: E731
    head = (_lib.ptr(ins[0]), _lib.ptr(ins[1]), B, N, _lib.ptr(ins[2]), _seg_c(seg), M, n_parts, _lib.ptr(ins[3]), float(max_d2))
    if grid is not None:
        rc = L.pn_icp_grid_correspond(*head, mode, _lib.ptr(ins[4]), _lib.ptr(ins[5]), p("idx"), p("d2"), p("q") if q_out else None,
                                      p("sums") if mode else None, p("ws"), nbytes, _vp(grid), float(c["r2"]), _lib.current_stream())
    elif mode == 2:
        rc = L.pn_icp_plane_sums(*head, _lib.ptr(ins[4]), _lib.ptr(ins[5]), p("idx"), p("d2"), p("sums"), p("ws"), nbytes, _lib.current_stream())
    else:
        rc = L.pn_icp_correspond(*head, p("idx"), p("d2"), p("sums") if mode else None, p("ws"), nbytes, _lib.current_stream())
    _lib.check(rc, "correspond")
    torch.cuda.synchronize()
    for name, (buf, _) in bufs.items():
        assert _intact(buf), f"{name}: guard band overwritten"
    for a, b in zip(keep, ins + [grid]):
        assert a is None or torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "an input or the tables were modified"
    return {k: v.cpu().numpy() for k, (_, v) in bufs.items() if k != "ws"}


def _check_contract(name, c, got, brute, max_d2):
    """the grid entry against the brute-force device entry and against the oracle, every query compared"""
    r2 = c["r2"]
    near = brute["d2"] <= r2                                                          # (false for +inf > r2: not found either way)
    assert np.array_equal(got["idx"], np.where(near, brute["idx"], -1)), (name, max_d2, np.argwhere(got["idx"] != np.where(near, brute["idx"], -1))[:5])
    want_d2 = np.where(near, brute["d2"], F32(np.inf)).astype(F32)
    assert np.array_equal(_bits(got["d2"]), _bits(want_d2)), (name, max_d2, np.argwhere(_bits(got["d2"]) != _bits(want_d2))[:5])
    ei, ed, eq = c["expect"]
    assert np.array_equal(got["idx"], np.where(ed <= max_d2, ei, -1)), (name, max_d2, "oracle idx")
    assert np.array_equal(_bits(got["d2"]), _bits(ed)), (name, max_d2, "oracle d2")
    same = (_bits(got["q"]) == _bits(eq)) | (np.isnan(got["q"]) & np.isnan(eq))
    assert same.all(), (name, max_d2, np.argwhere(~same)[:5])
    assert (np.isnan(got["q"]).all(-1) == np.isinf(got["d2"])).all()


@pytest.mark.parametrize("name", list(GO.CASES))
def test_single_pass_against_both_yardsticks(dev, name):
    c = GO.case(name)
    gbuf, grid = _build(dev, _t(c["ref"], dev), c["r2"], c["origin"])
    for max_d2 in c["max_d2"]:
        got = _raw(dev, c, max_d2, grid=grid)
        brute = _raw(dev, c, max_d2)
        _check_contract(name, c, got, brute, max_d2)
        bare = _raw(dev, c, max_d2, grid=grid, q_out=False)                            # q_out is optional
        assert np.array_equal(bare["idx"], got["idx"]) and np.array_equal(_bits(bare["d2"]), _bits(got["d2"]))
    assert _intact(gbuf)
    ei = c["expect"][0]
    if name == "ties":
        assert got["idx"][0, :6].tolist() == [0, 11, 8, 12, 8, 12]
    if name == "box":
        assert got["idx"][0].tolist() == list(range(8)) + [-1] * 8
    if name == "radius":
        assert (got["idx"][0, 0:12:2] < 0).all() and (_raw(dev, c, 2.25, grid=grid)["idx"][0, 0:12:2] >= 0).all()     # last cut: 1.0
    if name == "radius_below":
        assert (got["idx"][0, 1:12:2] < 0).all() and (got["d2"][0, 1:12:2] == np.nextafter(F32(2.25), F32(3))).all()
    assert (ei >= 0).any() and (ei < 0).any()


def _with_normals(c, seed):
    """random unit normals for a case's reference, a few of them NaN"""
    rng = np.random.default_rng(seed)
    n = rng.normal(size=c["ref"].shape)
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F32)
    n[rng.choice(len(n), max(1, len(n) // 50), replace=False)] = np.nan
    return n


@pytest.mark.parametrize("name", ["random", "radius_below", "one_voxel"])
def test_sums_byte_identical(dev, name):
    """the pairs, their order and the reduction are the brute-force entries': the same bytes, no tolerance"""
    c = GO.case(name)
    nrm = _with_normals(c, 3)
    _, grid = _build(dev, _t(c["ref"], dev), c["r2"], c["origin"])
    for max_d2 in c["max_d2"]:
        for mode in (1, 2):
            kw = dict(mode=mode, normals=nrm if mode == 2 else None, pose64=c["pose"] if mode == 2 else None)
            got = _raw(dev, c, max_d2, grid=grid, **kw)
            brute = _raw(dev, c, max_d2, **kw)
            _check_contract((name, mode), c, got, brute, max_d2)
            assert got["sums"].tobytes() == brute["sums"].tobytes(), (name, mode, max_d2)
            assert got["sums"][:, 0].sum() > 0
            if mode == 1:
                assert got["sums"][:, 0].tolist() == (brute["idx"] >= 0).sum(1).tolist()


def _kc46():
    from pointcloudprocessing_amd import pointcloud
    return pointcloud.read_labelled_cloud(os.path.join(helpers.GOLD, "kc-46.txt"), helpers.F15_PARTS)


def _off(true, b, deg=5.0, shift=0.3):
    P = np.array(true, np.float64)
    P[:3, :3] = IO.rot([1, -1, b], np.deg2rad(deg)) @ P[:3, :3]
    P[:3, 3] += np.array([1.0, -2.0, 2.0]) / 3.0 * shift
    return P


_SCENES = {}


def _scene(dev, name):
    """the two loop scenes -> (plain reference with normals, grid reference, scans (3, n, 3), labels, inits 5 degrees / 0.3 m off,
    max_dist): the kc-46 golden cloud (490 points, 7 of 12 parts, device normals), and 20,000 samples of the aircraft mesh"""
    from pointcloudprocessing_amd import ops
    if name not in _SCENES:
        if name == "kc46":
            xyz, part = _kc46()
            max_dist, n_parts = 2.0, NP
            _, _, plain = ops.icp_normals(ops.icp_reference(xyz, part, NP, device=dev), k=10)
            acc = ops._with_grid("test", plain, max_dist)
            true = PO.TRUE_POSE
            scans, labs = zip(*[IO.labelled_scan(xyz, part, 2000, true, noise=0.05, outliers=0.05, seed=3 + b) for b in range(3)])
        else:
            v, f, p = MO.aircraft_mesh(2)
            mesh = ops.icp_mesh_reference(v, f, p, NM, device=dev)
            max_dist, n_parts, true = 0.5, NM, PO.TRUE_POSE
            plain = ops.mesh_sample_reference(mesh, 20000, seed=1)
            acc = ops.mesh_sample_reference(mesh, 20000, seed=1, accel="grid", max_dist=max_dist)
            assert torch.equal(plain.xyz, acc.xyz) and torch.equal(plain.normals, acc.normals) and plain.seg == acc.seg
            scans, labs = zip(*[MO.mesh_scan(v, f, p, 4000, true, noise=0.02, seed=1 + 5 * b) for b in range(3)])
        assert type(acc) is ops.IcpGridReference and type(plain) is ops.IcpReference and acc.max_dist == max_dist
        inits = np.stack([_off(true, b) for b in range(3)])
        _SCENES[name] = (plain, acc, _t(np.stack(scans), dev), _t(np.stack(labs).astype(np.int32), dev), _t(inits, dev), max_dist)
    return _SCENES[name]


def _raw_loop(dev, ref, S, L, I, metric, max_dist, grid, max_iters=12):
    """pn_semantic_icp_grid (``grid``) or pn_semantic_icp / pn_semantic_icp_plane through the C ABI with guard bands"""
    from pointcloudprocessing_amd import _lib, ops
    lib = _lib.lib()
    B, N, _ = S.shape
    nbytes = (lib.pn_icp_plane_workspace_bytes if grid or metric == 2 else lib.pn_icp_workspace_bytes)(B, N, ref.M, ref.n_parts)
    bufs = dict(pose=_guarded((B, 4, 4), torch.float64, dev), rmse=_guarded((B,), torch.float64, dev), pairs=_guarded((B,), torch.int32, dev),
                iters=_guarded((B,), torch.int32, dev), status=_guarded((B,), torch.int32, dev), ws=_guarded((nbytes,), torch.uint8, dev))
    q = lambda k: _vp(bufs[k][1])                                                     # noqa: E731
    head = (_lib.ptr(S), _lib.ptr(L), B, N, _lib.ptr(ref.xyz), ref._seg_c, ref.M, ref.n_parts)
    loop = (_lib.ptr(I), max_iters, ops._max_d2(max_dist), 1e-7, 1e-7)
    outs = (q("pose"), q("rmse"), q("pairs"), q("iters"), q("status"), q("ws"), nbytes)
    if grid:
        rc = lib.pn_semantic_icp_grid(*head, _lib.ptr(ref.normals) if metric == 2 else None, metric, *loop, *outs, _lib.ptr(ref.grid), ref.r2,
                                      _lib.current_stream())
    elif metric == 2:
        rc = lib.pn_semantic_icp_plane(*head, *loop, _lib.ptr(ref.normals), *outs, _lib.current_stream())
    else:
        rc = lib.pn_semantic_icp(*head, *loop, *outs, _lib.current_stream())
    _lib.check(rc, "loop")
    return bufs


def _loop_out(bufs):
    torch.cuda.synchronize()
    for name, (buf, _) in bufs.items():
        assert _intact(buf), f"{name}: guard band overwritten"
    return {k: v.cpu().numpy() for k, (_, v) in bufs.items() if k != "ws"}


@pytest.mark.parametrize("metric", [1, 2])
@pytest.mark.parametrize("name", ["kc46", "sampled"])
def test_loops_bit_equal_to_the_brute_force_loops(dev, name, metric):
    plain, acc, S, L, I, max_dist = _scene(dev, name)
    keep = [x.clone() for x in (S, L, I, acc.xyz, acc.normals, acc.grid)]
    want = _loop_out(_raw_loop(dev, plain, S, L, I, metric, max_dist, False))
    got = _loop_out(_raw_loop(dev, acc, S, L, I, metric, max_dist, True))
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), (name, metric, k, got[k], want[k])
    assert np.isfinite(got["pose"]).all() and (got["iters"] > 1).all() and (got["pairs"] > S.shape[1] // 10).all(), (got["iters"], got["pairs"])
    print(f"{name} metric {metric}: iters {got['iters'].tolist()} pairs {got['pairs'].tolist()} status {got['status'].tolist()}")
    for i in range(3):                                                                # the batch equals its scans run singly
        single = _loop_out(_raw_loop(dev, acc, S[i:i + 1].contiguous(), L[i:i + 1].contiguous(), I[i:i + 1].contiguous(), metric, max_dist, True))
        for k in want:
            assert single[k].tobytes() == got[k][i:i + 1].tobytes(), (name, metric, i, k)
    g = torch.cuda.CUDAGraph()                                                        # a graph replay equals the eager call
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _raw_loop(dev, acc, S, L, I, metric, max_dist, True)
        with torch.cuda.graph(g, stream=side):
            captured = _raw_loop(dev, acc, S, L, I, metric, max_dist, True)
    torch.cuda.current_stream().wait_stream(side)
    for k in ("pose", "rmse", "pairs", "iters", "status"):
        captured[k][1].fill_(0)
    g.replay()
    replay = _loop_out(captured)
    for k in want:
        assert replay[k].tobytes() == want[k].tobytes(), (name, metric, k, "replay")
    for x, y in zip(keep, (S, L, I, acc.xyz, acc.normals, acc.grid)):
        assert torch.equal(x, y), "an input or the tables were modified"


def test_build_is_capturable_and_reports_its_errors(dev):
    from pointcloudprocessing_amd import _lib, ops
    from pointcloudprocessing_amd._lib import PointNetHipError
    L = _lib.lib()
    c = GO.case("random")
    ref = _t(c["ref"], dev)
    _, eager = _build(dev, ref, c["r2"], c["origin"])
    M = len(c["ref"])
    grid = torch.zeros(L.pn_icp_grid_bytes(M), dtype=torch.uint8, device=dev)
    ws = torch.zeros(L.pn_icp_grid_build_workspace_bytes(M), dtype=torch.uint8, device=dev)
    o = (C.c_float * 3)(*[float(v) for v in c["origin"]])
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            _lib.check(L.pn_icp_grid_build(_lib.ptr(ref), M, float(c["r2"]), o, _vp(grid), grid.numel(), _vp(ws), ws.numel(), _lib.current_stream()), "build")
    torch.cuda.current_stream().wait_stream(side)
    g.replay()
    torch.cuda.synchronize()
    al = lambda v: (v + 255) & ~255                                                    # noqa: E731  (the tables; the gaps between them are not written)
    o_key = 256 + al(16 * M)
    for lo, n in ((0, 32), (256, 16 * M), (o_key, 8 * M), (o_key + al(8 * M), 4 * (M + 1))):
        assert torch.equal(grid[lo:lo + n], eager[lo:lo + n]), lo
    assert o_key + al(8 * M) + al(4 * (M + 1)) == grid.numel()
    # error word 1: a key outside the box (an origin above the cloud, a cloud wider than 2^14 leaves), a non-finite coordinate
    for o_bad, pts in (((6.0, -5.0, -5.0), c["ref"]), (c["origin"], np.concatenate([c["ref"], [[2e4, 0, 0]]]).astype(F32)),
                       (c["origin"], np.concatenate([c["ref"], [[np.nan, 0, 0]]]).astype(F32))):
        x = _t(pts, dev)
        gr = torch.zeros(L.pn_icp_grid_bytes(len(pts)), dtype=torch.uint8, device=dev)
        w = torch.zeros(L.pn_icp_grid_build_workspace_bytes(len(pts)), dtype=torch.uint8, device=dev)
        _lib.check(L.pn_icp_grid_build(_lib.ptr(x), len(pts), float(c["r2"]), (C.c_float * 3)(*[float(v) for v in o_bad]), _vp(gr), gr.numel(),
                                       _vp(w), w.numel(), _lib.current_stream()), "build")
        torch.cuda.synchronize()
        assert int(w[:4].view(torch.int32).item()) == 1
    plain = ops.IcpReference(_t(np.concatenate([c["ref"], [[2e4, 0, 0]]]).astype(F32), dev), (0, M + 1), None, 1)
    with pytest.raises(PointNetHipError, match="grid key fell outside"):
        ops._with_grid("test", plain, 0.7)
    with pytest.raises(PointNetHipError, match="not finite"):
        ops._with_grid("test", ops.IcpReference(_t(np.array([[0, np.inf, 0]], F32), dev), (0, 1), None, 1), 0.7)


def _bytes_equal(a, b):
    return all(np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8)) for x, y in zip(a, b))


def test_higher_level_calls_take_the_grid_reference(dev):
    from oracle import pointnet_oracle as O            # checker only
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd._lib import PointNetHipError
    from pointcloudprocessing_amd.pointnet.PointNet import PointNet
    plain, acc, S, L, I, max_dist = _scene(dev, "kc46")
    for metric in ("point", "plane"):
        kw = dict(max_iters=10, max_dist=max_dist, metric=metric)
        assert _bytes_equal(ops.semantic_icp(S, L, plain, I, **kw), ops.semantic_icp(S, L, acc, I, **kw)), metric
        kw["max_dist"] = 1.0                                                          # below the reference's
        assert _bytes_equal(ops.semantic_icp(S, L, plain, I, **kw), ops.semantic_icp(S, L, acc, I, **kw)), metric
    # the single passes: idx and sums are the plain reference's; d2 differs only beyond the reference's max_dist, where it is +inf
    for fn, pose in ((lambda r: ops.icp_correspond(S, L, r, I.float(), max_dist=max_dist, sums=True), None),
                     (lambda r: ops.icp_plane_sums(S, L, r, I, max_dist=max_dist), None)):
        (i0, d0, s0), (i1, d1, s1) = fn(plain), fn(acc)
        assert torch.equal(i0, i1) and torch.equal(s0, s1) and torch.equal(torch.where(d0 <= acc.r2, d0, torch.full_like(d0, float("inf"))), d1)
        assert bool((i1 >= 0).any()) and bool(torch.isinf(d1).any())
    kw = dict(top=2, stride=1, max_iters=6, metric="plane", rotations=ops.rotation_grid(16))
    want, got = ops.global_pose(S, L, plain, max_dist, **kw), ops.global_pose(S, L, acc, max_dist, **kw)
    assert _bytes_equal(want, got) and np.isfinite(got[0].cpu().numpy()).all()
    model = PointNet(23, 12, 0.3, 42, precision="bf16", device=dev)
    model.set_weights(O.init_params(23, 12, seed=31, randomize_bn=True))
    x = S[0].contiguous()
    for metric in ("point", "plane"):
        a = model.predict_pose(x, plain, leaf=0.25, samples=1024, k=3, max_iters=5, metric=metric, max_dist=max_dist)
        b = model.predict_pose(x, acc, leaf=0.25, samples=1024, k=3, max_iters=5, metric=metric, max_dist=max_dist)
        assert _bytes_equal(a, b), metric
    with pytest.raises(PointNetHipError, match="exceeds the grid reference's"):
        ops.semantic_icp(S, L, acc, I)
    with pytest.raises(PointNetHipError, match="exceeds the grid reference's"):
        model.predict_pose(x, acc, leaf=0.25, samples=1024, k=3, max_iters=5)
    for opt in (dict(robust="huber"), dict(weights=torch.ones_like(S[..., 0]))):
        with pytest.raises(PointNetHipError, match="accel=None"):
            ops.semantic_icp(S, L, acc, I, max_dist=max_dist, **opt)
    with pytest.raises(PointNetHipError, match="accel=None"):
        ops.global_pose(S, L, acc, max_dist, top=1, rotations=ops.rotation_grid(16), robust="tukey")
    # icp_reference(accel="grid") groups as the plain call does and carries the library's tables
    xyz, part = _kc46()
    r = ops.icp_reference(xyz, part, NP, device=dev, accel="grid", max_dist=max_dist)
    assert type(r) is ops.IcpGridReference and torch.equal(r.xyz, plain.xyz) and r.seg == plain.seg and torch.equal(r.grid, acc.grid)
    assert r.r2 == ops._max_d2(max_dist) and r.normals is None
    _, _, rn = ops.icp_normals(r, k=10)
    assert type(rn) is ops.IcpGridReference and torch.equal(rn.normals, plain.normals) and rn.grid is r.grid


def test_register_scans(dev):
    """two independent surface samplings of the aircraft mesh, the source moved by a known pose with 2 cm noise: the grid and the
    brute-force search give the same bits, and both land within the 0.05 degrees / 5 cm that tests/test_gpu_icp_plane.py asks of
    its surface-sampled scene"""
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
    for metric in ("plane", "point"):
        got = ops.register_scans(source, target, 0.5, metric=metric)
        want = ops.register_scans(source, target, 0.5, metric=metric, accel=None)
        assert _bytes_equal(got, want), metric
        pose, rmse, pairs, iters, status = (x.cpu().numpy() for x in got)
        ang, dt = IO.pose_error(pose[0], true)
        print(f"register_scans {metric}: {int(iters[0])} iterations, {np.rad2deg(ang):.4f} deg, {dt * 100:.2f} cm, rmse {rmse[0]:.4f}, pairs {int(pairs[0])}")
        assert pose.shape == (1, 4, 4) and pairs[0] > 15000
        if metric == "plane":
            assert np.rad2deg(ang) <= 0.05 and dt <= 0.05, (np.rad2deg(ang), dt)
    batch = ops.register_scans(torch.stack([source, source]), target, 0.5, init_pose=torch.eye(4, device=dev, dtype=torch.float64))
    assert _bytes_equal([x[:1] for x in batch], ops.register_scans(source, target, 0.5)) and batch[0].shape == (2, 4, 4)
