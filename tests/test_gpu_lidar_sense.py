"""pn_lidar_sense on the MI355X: hit_out, the bits of t_out and kind_out equal to the NumPy oracle (tests/lidar_sense_oracle.py) through
the raw entry on guard-banded outputs, on rasters shorter and longer than a wave, several frames and blocks, every stage alone, bad
rows and ranges among the inputs, and the jump threshold at its last bit; graph capture; ops.lidar_sense, ops.lidar_frames and
pointcloud.simulate_dataset with ``sensor``; and a simulated frame through the incidence filter of the cleaning stage."""
import ctypes as C

import numpy as np
import pytest
import torch

import icp_mesh_oracle as MO
import lidar_oracle as LO
import lidar_sense_oracle as SE

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 4096          # bytes of fill pattern before and after every output buffer
PAT = 0xA5


def _guarded(nbytes, dev):
    buf = torch.full((GUARD + nbytes + GUARD,), PAT, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + nbytes]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _raw(dev, tri, poses, dirs, hit, t, H, W, seed=0, frame0=0, want_kind=True, **m):
    """pn_lidar_sense on guard-banded outputs -> (hit_out, t_out, kind_out or None); asserts that the bands and the inputs are untouched"""
    from pointcloudprocessing_amd import _lib
    m = dict(SE.OFF, **m)
    tri = np.asarray(tri, F32).reshape(-1, 3, 3)
    B, R = hit.shape
    ins = [_t(a, dev) for a in (tri, np.asarray(poses, F32), np.asarray(dirs, F32), np.asarray(hit, np.int32), np.asarray(t, F32))]
    keep = [x.clone() for x in ins]
    bufs = {name: _guarded(n, dev) for name, n in (("hit", 4 * B * R), ("t", 4 * B * R), ("kind", B * R))}
    p = lambda name: C.c_void_p(bufs[name][1].data_ptr())      # noqa: E731
    rc = _lib.lib().pn_lidar_sense(_lib.ptr(ins[0]), len(tri), _lib.ptr(ins[1]), B, _lib.ptr(ins[2]), H, W, _lib.ptr(ins[3]), _lib.ptr(ins[4]),
                                   int(seed), int(frame0), m["sigma0"], m["sigma1"], m["strength"], m["range_ref"], m["min_cos2"], m["jump"],
                                   m["p_mix"], p("hit"), p("t"), p("kind") if want_kind else None, _lib.current_stream())
    _lib.check(rc, "pn_lidar_sense")
    torch.cuda.synchronize()
    for name, (buf, _) in bufs.items():
        assert bool((buf[:GUARD] == PAT).all()) and bool((buf[-GUARD:] == PAT).all()), f"{name}: guard band overwritten"
    for a, b in zip(keep, ins):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "an input was modified"
    if not want_kind:
        assert bool((bufs["kind"][1] == PAT).all())
    return (bufs["hit"][1].view(torch.int32).view(B, R).cpu().numpy(), bufs["t"][1].view(torch.float32).view(B, R).cpu().numpy(),
            bufs["kind"][1].view(B, R).cpu().numpy() if want_kind else None)


def _same(got, exp, name=""):
    assert np.array_equal(got[0], exp[0]), (name, "hit", np.argwhere(got[0] != exp[0])[:5])
    assert np.array_equal(_bits(got[1]), _bits(exp[1])), (name, "t", np.argwhere(_bits(got[1]) != _bits(exp[1]))[:5])
    if got[2] is not None:
        assert np.array_equal(got[2], exp[2]), (name, "kind", np.argwhere(got[2] != exp[2])[:5])


def _check(dev, tri, poses, dirs, hit, t, H, W, seed=0, frame0=0, want_kind=True, name="", **m):
    exp = SE.sense(tri, poses, dirs, hit, t, H, W, seed=seed, frame0=frame0, **dict(SE.OFF, **m))
    _same(_raw(dev, tri, poses, dirs, hit, t, H, W, seed, frame0, want_kind, **m), exp, name)
    return exp


ON = SE.model_args(**SE.ALL_ON)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 70), (70, 1), (5, 67)])
def test_rasters_shorter_and_longer_than_a_wave(dev, H, W):
    """a row and a column of one pixel, of more than 64, and a row pitch that is no multiple of 64, two frames each: head on (the plate's
    edge runs through the image) and from the side"""
    tri = SE.plate_wall()[0]
    dirs = SE.pinhole(H, W, 100.0, 80.0)
    poses = np.stack([SE.yaw_pose(0.0, (0.0, -0.25, 0.125)), SE.yaw_pose(-40.0, (1.0, 3.0, -0.5))]).astype(F32)
    hit, t = LO.cast(tri, poses, dirs)
    assert (hit >= 0).any()
    exp = _check(dev, tri, poses, dirs, hit, t, H, W, seed=21, frame0=2, name=(H, W), **ON)
    if H * W > 1:
        assert (exp[2] == SE.MIXED).any() and (exp[2] == SE.RETURN).any()


@pytest.mark.parametrize("stage", sorted(SE.STAGES))
def test_four_kinds_every_stage(dev, stage):
    """17 x 33 rays in three frames at frame0 = 5: 561 rays a frame, more than two blocks; all stages on, each alone, all off"""
    tri, seg, poses, dirs, hit, t = SE.four_kinds()
    m = SE.model_args(**SE.STAGES[stage])
    exp = _check(dev, tri, poses, dirs, hit, t, *SE.FOUR_KINDS_SHAPE, seed=SE.FOUR_KINDS_SEED, frame0=SE.FOUR_KINDS_FRAME0, name=stage, **m)
    counts = SE.kind_counts(exp[2])
    if stage == "all":
        assert min(counts) >= 20, counts
        _check(dev, tri, poses, dirs, hit, t, *SE.FOUR_KINDS_SHAPE, seed=SE.FOUR_KINDS_SEED, frame0=SE.FOUR_KINDS_FRAME0, want_kind=False, **m)
        other = _check(dev, tri, poses, dirs, hit, t, *SE.FOUR_KINDS_SHAPE, seed=SE.FOUR_KINDS_SEED + (1 << 40), frame0=0, **m)
        assert not np.array_equal(other[2], exp[2])
    if stage == "off":
        assert np.array_equal(exp[0], hit) and np.array_equal(_bits(exp[1]), _bits(t)) and counts[2:] == [0, 0]


def test_bad_rows_and_ranges_among_the_inputs(dev):
    tri, seg, poses, dirs, hit, t = SE.four_kinds()
    hit, t = hit.copy(), t.copy()
    R = hit.shape[1]
    live = np.flatnonzero(hit.reshape(-1) >= 0)
    rows = live[np.linspace(0, len(live) - 1, 24).astype(int)]
    hit.reshape(-1)[rows[:8]] = [len(tri), len(tri) + 1, 1 << 20, 1 << 24, (1 << 31) - 1, -2, -(1 << 31), len(tri)]
    t.reshape(-1)[rows[8:]] = [np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, 1e-30, 3e38] * 2
    for name, m in (("off", SE.OFF), ("on", ON)):
        exp = _check(dev, tri, poses, dirs, hit, t, *SE.FOUR_KINDS_SHAPE, seed=4, name=name, **m)
        k = exp[2].reshape(-1)
        gone = 14 if name == "off" else 11             # NaN and +-inf are lost whatever the model; 0, -0 and -1 fail the validity rule
        assert (k[rows[:8]] == SE.MISS).all() and (k[rows[8:gone]] == SE.DROPPED).all() and (k[rows[16:gone + 8]] == SE.DROPPED).all()
        assert (exp[0].reshape(-1)[rows[:gone]] == -1).all() and np.isposinf(exp[1].reshape(-1)[rows[:gone]]).all()
    assert R == 561


def test_jump_threshold_at_its_last_bit(dev):
    tri, poses, dirs, hit, t = SE.exact_walls()
    assert set(np.unique(t[hit >= 0]).tolist()) == {8.0, 11.0}
    mixed = {}
    for name, jump in (("below", np.nextafter(3.0, 0.0)), ("at", 3.0), ("above", np.nextafter(3.0, 4.0))):
        exp = _check(dev, tri, poses, dirs, hit, t, 21, 21, seed=5, name=name, **dict(SE.OFF, jump=float(jump), p_mix=1.0))
        mixed[name] = SE.kind_counts(exp[2])[SE.MIXED]
    assert mixed["below"] >= 40 and mixed["at"] == 0 == mixed["above"], mixed
    _check(dev, tri, poses, dirs, hit, t, 21, 21, seed=5, name="noise on exact ranges", **dict(ON, jump=0.0, p_mix=0.5))


def test_graph_capture_replays_on_a_second_input(dev):
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    tri, seg, poses, dirs, hit, t = SE.four_kinds()
    H, W = SE.FOUR_KINDS_SHAPE
    R = H * W
    cases = [(poses[b:b + 1], hit[b:b + 1], t[b:b + 1]) for b in (0, 1)]
    exps = [SE.sense(tri, p, dirs, h, tt, H, W, seed=9, frame0=1, **ON) for p, h, tt in cases]
    assert not np.array_equal(exps[0][2], exps[1][2])
    tri_d, dirs_d = _t(tri, dev), _t(dirs, dev)
    pose_d, hit_d, t_d = (_t(a, dev) for a in cases[0])
    ho = torch.zeros(1, R, dtype=torch.int32, device=dev)
    to = torch.zeros(1, R, dtype=torch.float32, device=dev)
    ko = torch.zeros(1, R, dtype=torch.uint8, device=dev)

    def call():
        _lib.check(L.pn_lidar_sense(_lib.ptr(tri_d), len(tri), _lib.ptr(pose_d), 1, _lib.ptr(dirs_d), H, W, _lib.ptr(hit_d), _lib.ptr(t_d), 9, 1,
                                    ON["sigma0"], ON["sigma1"], ON["strength"], ON["range_ref"], ON["min_cos2"], ON["jump"], ON["p_mix"],
                                    _lib.ptr(ho), _lib.ptr(to), _lib.ptr(ko), _lib.current_stream()), "pn_lidar_sense")

    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                           # warm-up on the capture stream
        with torch.cuda.graph(g, stream=side):
            call()
    torch.cuda.current_stream().wait_stream(side)
    for (p, h, tt), exp in ((cases[1], exps[1]), (cases[0], exps[0])):
        pose_d.copy_(_t(p, dev)); hit_d.copy_(_t(h, dev)); t_d.copy_(_t(tt, dev))
        ho.fill_(-7); to.fill_(-7.0); ko.fill_(9)
        g.replay()
        torch.cuda.synchronize()
        _same((ho.cpu().numpy(), to.cpu().numpy(), ko.cpu().numpy()), exp)


# ---- the Python surface ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plate_ref(dev):
    from pointcloudprocessing_amd import ops
    tri, seg, v, f, lab = SE.plate_wall()
    return ops.icp_mesh_reference(v, f, lab, 2, device=dev)


def _np(ts):
    return [x.cpu().numpy() for x in ts]


def _same_frames(got, exp, name=""):
    for k, (a, b) in enumerate(zip(got, exp)):
        if a.dtype == np.float32:
            assert ((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all(), (name, k)
        else:
            assert a.dtype == b.dtype and np.array_equal(a, b), (name, k)


def test_ops_sense_and_frames_equal_the_oracle(dev, plate_ref):
    from pointcloudprocessing_amd import ops
    tri, seg, poses, dirs, hit, t = SE.four_kinds()
    assert np.array_equal(plate_ref.tri.cpu().numpy().reshape(-1, 3, 3), tri)
    H, W = SE.FOUR_KINDS_SHAPE
    h_d, t_d = ops.lidar_cast(plate_ref, poses, dirs)
    assert np.array_equal(h_d.cpu().numpy(), hit) and np.array_equal(_bits(t_d.cpu().numpy()), _bits(t))
    got = _np(ops.lidar_sense(plate_ref, poses, dirs, h_d, t_d, (H, W), seed=13, frame0=2, **SE.ALL_ON))
    assert got[2].dtype == np.uint8
    _same(got, SE.sense(tri, poses, dirs, hit, t, H, W, seed=13, frame0=2, **ON), "ops.lidar_sense")
    off = _np(ops.lidar_sense(plate_ref, poses.astype(np.float64), torch.from_numpy(dirs).to(dev), h_d, t_d, (H, W)))
    assert np.array_equal(off[0], hit) and np.array_equal(_bits(off[1]), _bits(t)) and np.array_equal(off[2], (hit >= 0).astype(np.uint8))
    for n in (64, 300):                                     # fewer and more points than a frame has returns
        sensor = dict(SE.ALL_ON, shape=(H, W))
        got = _np(ops.lidar_frames(plate_ref, poses, dirs, n, sensor=sensor, seed=13, frame0=2))
        exp = SE.frames(tri, seg, 2, poses, dirs, n, (H, W), seed=13, frame0=2, **SE.ALL_ON)
        assert len(got) == 5 and got[4].dtype == np.uint8 and set(np.unique(exp[4])) == {SE.RETURN, SE.MIXED}
        _same_frames(got, exp, ("frames", n))
        plain = _np(ops.lidar_frames(plate_ref, poses, dirs, n))
        assert len(plain) == 4
        _same_frames(plain, LO.pack(hit, t, dirs, seg, 2, n), ("sensor=None", n))
        _same_frames(plain, _np(ops.lidar_pack(plate_ref, h_d, t_d, dirs, n)), ("cast + pack", n))
    nothing = poses.copy()
    nothing[0] = SE.yaw_pose(180.0)                         # a frame that sees nothing: kind 0 where ray is -1
    got = _np(ops.lidar_frames(plate_ref, nothing, dirs, 64, sensor=dict(shape=(H, W), mixed=dict(jump=0.3, prob=0.6))))
    assert got[3][0] == 0 and (got[2][0] == -1).all() and (got[4][0] == 0).all()
    _same_frames(got, SE.frames(tri, seg, 2, nothing, dirs, 64, (H, W), mixed=dict(jump=0.3, prob=0.6)), "empty frame")


def test_simulate_dataset_is_a_function_of_the_frame_index(dev):
    from pointcloudprocessing_amd import ops, pointcloud
    NM = len(MO.MESH_PARTS)
    v, f, p = MO.aircraft_mesh(0)
    tri, seg, _, _, _ = MO.group_mesh(v, f, p, NM)
    ref = ops.icp_mesh_reference(v, f, p, NM, device=dev)
    H, W, n = 23, 29, 256
    dirs = pointcloud.pinhole_rays(H, W, 50.0, 40.0)
    vp = pointcloud.sample_viewpoints(6, (45.0, 80.0), (0.0, 360.0), (-30.0, 60.0), seed=11)
    sensor = dict(shape=(H, W), range_sigma=(0.02, 0.001), detection=dict(strength=1.2, range_ref=60.0), max_incidence_deg=80.0,
                  mixed=dict(jump=1.0, prob=0.5))
    whole = pointcloud.simulate_dataset(ref, 3, vp, dirs, n, sensor=sensor, seed=17, print_func=None)
    a = pointcloud.simulate_dataset(ref, 3, vp[:2], dirs, n, sensor=sensor, seed=17, print_func=None)
    b = pointcloud.simulate_dataset(ref, 3, vp[2:], dirs, n, sensor=sensor, seed=17, frame0=2, print_func=None)
    assert whole[0].shape == (6, n, 3) and whole[2].shape == (6, n) and whole[3].shape == (6, 3, 3) and whole[1].tolist() == [3] * 6
    for w, x, y in zip(whole, a, b):
        assert w.dtype == x.dtype and np.array_equal(w.view(np.uint8), np.concatenate([x, y]).view(np.uint8))
    poses = np.stack([pointcloud.look_at_pose(x) for x in vp])
    model = {k: val for k, val in sensor.items() if k != "shape"}
    exp = SE.frames(tri, seg, NM, poses, dirs, n, (H, W), seed=17, **model)
    assert (exp[3] > 0).all() and len(set(np.unique(exp[4]).tolist())) == 2
    _same_frames([whole[0], whole[2]], [exp[0], exp[1]], "simulate_dataset")
    wrong = pointcloud.simulate_dataset(ref, 3, vp[2:], dirs, n, sensor=sensor, seed=17, print_func=None)      # frame0 left at 0
    assert not np.array_equal(wrong[0].view(np.uint8), whole[0][2:].view(np.uint8))
    plain = pointcloud.simulate_dataset(ref, 3, vp, dirs, n, print_func=None)
    ideal = LO.pack(*LO.cast(tri, poses, dirs), dirs, seg, NM, n)
    _same_frames([plain[0], plain[2]], [ideal[0], ideal[1]], "sensor=None")


def test_simulated_frame_through_the_incidence_filter(dev, plate_ref):
    """what the sensor model is for: the frame carries mixed pixels on the plate's edge, and the cleaning stage's incidence filter drops
    them rather than clean returns -- the rows normals_oracle.incidence_mask drops on the oracle's frame"""
    import normals_oracle as NN
    from pointcloudprocessing_amd import ops
    e = SE.E2E
    dirs, xyz, part, ray, count, kind = SE.e2e_frame()
    H, W = e["shape"]
    n = int(count[0])
    assert n == H * W
    nrm = NN.normals(xyz[0], e["radius"], e["k"], (0.0, 0.0, 0.0))[0]
    want, margin = NN.incidence_mask(xyz[0], nrm, (0.0, 0.0, 0.0), e["max_angle_deg"], return_margin=True)
    assert margin.min() > 1e-5                                             # no decision near the threshold: the masks must be equal
    k = kind[0]
    kept_mixed, kept_clean = want[k == SE.MIXED].mean(), want[k == SE.RETURN].mean()
    assert 1.0 - kept_mixed > 1.0 - kept_clean                             # the oracle alone drops more mixed than clean returns
    got = ops.lidar_frames(plate_ref, np.eye(4)[None], dirs, n, sensor=dict(e["sensor"], shape=(H, W)), seed=e["seed"])
    _same_frames(_np(got), (xyz, part, ray, count, kind), "frame")
    keep = ops.outlier_mask(got[0][0].contiguous(), "incidence", e["radius"], k=e["k"], max_angle_deg=e["max_angle_deg"]).cpu().numpy()
    assert np.array_equal(keep, want)
    gk = got[4][0].cpu().numpy()
    assert keep[gk == SE.MIXED].mean() == kept_mixed and keep[gk == SE.RETURN].mean() == kept_clean
