"""pn_recon_field / pn_recon_count / pn_recon_emit on the MI355X against the NumPy oracle (tests/recon_oracle.py, whose own facts
tests/test_cpu_recon.py checks): validity, the NaN pattern, the neighbour counts, n_vertices, n_faces and the faces exactly; f bit for
bit (the header fixes the order of the fp64 sums and the oracle follows it; the licensed bound was one fp32 ulp, 2^-22 max(|f|,
1e-30), which is asserted first); the vertices within 1e-6 voxel (f_a and f_b have opposite signs, so a relative 2^-23 change of
either moves t by less than 2.4e-7 and the vertex by less than sqrt(3) voxel 2.4e-7), and bit for bit where f is.  Guard bands
round every output and the workspaces, the inputs unmodified; capacities one short; purity with dirty workspaces; graph capture
of the field and of the emit phase; the ops level with non-finite rows, the default lattice and hemisphere labels; and scans ->
mesh -> mesh ICP end to end.

Which level of the two scans (256 lattice points per workgroup, 256 workgroup totals per level-1 workgroup, one level-2 workgroup
that walks the level-1 sums 256 at a time with a carry) a case reaches:
  sphere, plate, plate_on_plane, layer, sparse   2 .. 12 workgroups: level 0, one level-1 workgroup, a single level-2 entry
  sphere_large   45^3 = 91,125 points and 44^3 = 85,184 cubes, 356 workgroups: two level-1 workgroups, two level-2 entries
  the long lattice   14 x 14 x 85,700 = 16,797,200 points, 65,615 workgroups, 257 level-1 sums: the level-2 carry"""
import ctypes as C

import numpy as np
import pytest
import torch

import recon_oracle as RO

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 4096
PAT = 0xA5
ERR_CAPACITY = 4


def _t(a, dev="cuda:0"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _guarded(nbytes, dev, fill=PAT):
    buf = torch.full((GUARD + nbytes + GUARD,), PAT, dtype=torch.uint8, device=dev)
    buf[GUARD:GUARD + nbytes] = fill
    return buf, buf[GUARD:GUARD + nbytes]


def _finish(bufs, keep, ins, expect_error):
    torch.cuda.synchronize()
    for name, (buf, _) in bufs.items():
        assert bool((buf[:GUARD] == PAT).all()) and bool((buf[-GUARD:] == PAT).all()), f"{name}: guard band overwritten"
    for a, b in zip(keep, ins):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "an input was modified"
    assert int(bufs["ws"][1][:4].view(torch.int32).item()) == expect_error, "error word"


def _d3(v):
    return (C.c_double * 3)(*[float(a) for a in v])


def _raw_field(c, want_count=True, grid_origin=None, ws_fill=PAT, expect_error=0, stream=None):
    """pn_recon_field through the C ABI on guard-banded outputs and workspace -> (f (P,) f32, count (P,) i32 or None)"""
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    x, n = _t(c["xyz"]), _t(c["normals"])
    keep = [x.clone(), n.clone()]
    N, P = x.shape[0], int(np.prod(c["dims"]))
    go = x.min(0).values.cpu().tolist() if grid_origin is None else grid_origin
    nbytes = L.pn_recon_field_workspace_bytes(N)
    bufs = dict(f=_guarded(4 * P, x.device), ws=_guarded(nbytes, x.device, ws_fill))
    if want_count:
        bufs["count"] = _guarded(4 * P, x.device)
    p = lambda k: C.c_void_p(bufs[k][1].data_ptr()) if k in bufs else None            # noqa: E731
    rc = L.pn_recon_field(_lib.ptr(x), _lib.ptr(n), N, c["radius"], (C.c_float * 3)(*go), _d3(c["origin"]), c["voxel"], *c["dims"],
                          c["min_points"], p("f"), p("count"), p("ws"), nbytes, stream or _lib.current_stream())
    _lib.check(rc, "pn_recon_field")
    _finish(bufs, keep, [x, n], expect_error)
    return bufs["f"][1].view(torch.float32).cpu().numpy(), bufs["count"][1].view(torch.int32).cpu().numpy() if want_count else None


def _raw_count(f, dims, ws_fill=PAT):
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    ft = f if torch.is_tensor(f) else _t(np.asarray(f, F32))
    keep = [ft.clone()]
    nbytes = L.pn_recon_workspace_bytes(*dims)
    bufs = dict(n=_guarded(8, ft.device), ws=_guarded(nbytes, ft.device, ws_fill))
    rc = L.pn_recon_count(_lib.ptr(ft), *dims, C.c_void_p(bufs["n"][1].data_ptr()), C.c_void_p(bufs["ws"][1].data_ptr()), nbytes,
                          _lib.current_stream())
    _lib.check(rc, "pn_recon_count")
    _finish(bufs, keep, [ft], 0)
    return tuple(int(v) for v in bufs["n"][1].view(torch.int32).cpu().tolist())


def _raw_emit(f, origin, voxel, dims, V, Fc, vcap=None, fcap=None, ws_fill=PAT, expect_error=0):
    """pn_recon_emit into buffers of V and Fc rows, told the capacities ``vcap`` / ``fcap`` (default: all of them) -> (vertices (V, 3)
    f32, faces (Fc, 3) i32, (n_vertices, n_faces)); rows at and past a capacity come back as the fill pattern"""
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    ft = f if torch.is_tensor(f) else _t(np.asarray(f, F32))
    keep = [ft.clone()]
    nbytes = L.pn_recon_workspace_bytes(*dims)
    dev = ft.device
    bufs = dict(v=_guarded(12 * V, dev), f=_guarded(12 * Fc, dev), n=_guarded(8, dev), ws=_guarded(nbytes, dev, ws_fill))
    p = lambda k: C.c_void_p(bufs[k][1].data_ptr())                                   # noqa: E731
    rc = L.pn_recon_emit(_lib.ptr(ft), _d3(origin), float(voxel), *dims, p("v"), V if vcap is None else vcap, p("f"), Fc if fcap is None else fcap,
                         p("n"), p("ws"), nbytes, _lib.current_stream())
    _lib.check(rc, "pn_recon_emit")
    _finish(bufs, keep, [ft], expect_error)
    return (bufs["v"][1].view(torch.float32).view(V, 3).cpu().numpy(), bufs["f"][1].view(torch.int32).view(Fc, 3).cpu().numpy(),
            tuple(int(v) for v in bufs["n"][1].view(torch.int32).cpu().tolist()))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_field(name, f, count, c):
    ef, ec = c["f"], c["count"]
    assert np.array_equal(count, ec), (name, np.flatnonzero(count != ec)[:5])
    assert np.array_equal(np.isnan(f), np.isnan(ef)), (name, np.flatnonzero(np.isnan(f) != np.isnan(ef))[:5])
    ok = ~np.isnan(ef)
    err = np.abs(f[ok].astype(np.float64) - ef[ok].astype(np.float64))
    bound = 2.0 ** -22 * np.maximum(np.abs(ef[ok].astype(np.float64)), 1e-30)
    exact = np.array_equal(_bits(f[ok]), _bits(ef[ok]))
    print(f"{name}: lattice {c['dims']}, {int(ok.sum())} valid, f bit for bit: {exact}, max |f - oracle| / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all(), (name, float((err / bound).max()))
    assert exact, name             # the header fixes the order of the sums: reached bit for bit on the MI355X, so that is what holds
    return exact


def _check_surface(name, f, c):
    """count and emit on ``f`` against the oracle's mesh of the case"""
    ev, efc = c["vertices"], c["faces"]
    V, Fc = _raw_count(f, c["dims"])
    assert (V, Fc) == (len(ev), len(efc)), name
    v, faces, n = _raw_emit(f, c["origin"], c["voxel"], c["dims"], V, Fc)
    assert n == (V, Fc) and np.array_equal(faces, efc), (name, np.flatnonzero((faces != efc).any(1))[:5])
    err = np.abs(v.astype(np.float64) - ev.astype(np.float64)).max() if V else 0.0
    print(f"{name}: V = {V}, F = {Fc}, vertices bit for bit: {np.array_equal(_bits(v), _bits(ev))}, max |v - oracle| = {err:.3e} "
          f"(bound {1e-6 * c['voxel']:.3e})")
    assert err <= 1e-6 * c["voxel"], (name, err)
    if np.array_equal(_bits(np.asarray(f.cpu() if torch.is_tensor(f) else f)), _bits(c["f"])):
        assert np.array_equal(_bits(v), _bits(ev)), name      # the same f: the same fp64 operations, the same bits
    return v, faces


@pytest.mark.parametrize("name", RO.CASES)
def test_field_and_surface_against_oracle(dev, name):
    c = RO.solved(name)
    f, count = _raw_field(c)
    _check_field(name, f, count, c)
    v, faces = _check_surface(name, f, c)
    _check_surface(name + " (the oracle's f)", c["f"], c)
    if name in ("sphere", "sphere_large"):                   # the device's own output
        assert RO.closed(faces) and RO.oriented(faces) and RO.euler(len(v), faces) == 2 and RO.unused_vertices(len(v), faces) == 0
    if name == "plate":
        assert (RO.face_normals(v, faces)[:, 2] > 0).all() and RO.edge_face_counts(faces).max() == 2
    # without the optional count, and with the cloud's grid placed elsewhere: the same neighbours, summed in that grid's order
    go = (c["xyz"].min(0) - F32(0.37)).tolist()
    f2, _ = _raw_field(c, want_count=False, grid_origin=go)
    e2, n2 = RO.field(c["xyz"], c["normals"], c["radius"], c["origin"], c["voxel"], c["dims"], c["min_points"], grid_origin=go)
    assert np.array_equal(n2, c["count"]) and np.array_equal(_bits(f2), _bits(e2))
    ok = ~np.isnan(f)
    assert (np.abs(f2[ok].astype(np.float64) - f[ok]) <= 2.0 ** -22 * np.abs(f[ok])).all()


def test_zero_is_outside_and_the_mesh_goes_into_the_mesh_reference(dev):
    from pointcloudprocessing_amd import ops
    c = RO.solved("plate_on_plane")
    f, _ = _raw_field(c)
    on_plane = (c["f"] == 0)
    assert on_plane.sum() > 50 and np.array_equal(_bits(f[on_plane]), _bits(c["f"][on_plane]))      # +0, bit for bit
    v, faces = _check_surface("plate_on_plane", f, c)
    assert (v[:, 2] == 0).all()                                                                     # t = 1: the outside end itself
    area = np.linalg.norm(RO.face_normals(v, faces), axis=1)
    ref = ops.icp_mesh_reference(v, faces, np.zeros(len(faces), np.int32), 1, device=dev)
    assert 0 < int((area > 0).sum()) == ref.tri.shape[0] < len(faces)                               # the zero-area faces are dropped


def test_capacities_one_short(dev):
    c = RO.solved("sphere")
    V, Fc = len(c["vertices"]), len(c["faces"])
    v, faces, n = _raw_emit(c["f"], c["origin"], c["voxel"], c["dims"], V, Fc, vcap=V - 1, expect_error=ERR_CAPACITY)
    assert n == (V, Fc) and (v.view(np.uint8)[V - 1] == PAT).all()                                  # nothing at or past the capacity
    assert np.array_equal(_bits(v[:V - 1]), _bits(c["vertices"][:V - 1])) and np.array_equal(faces, c["faces"])
    v, faces, n = _raw_emit(c["f"], c["origin"], c["voxel"], c["dims"], V, Fc, fcap=Fc - 1, expect_error=ERR_CAPACITY)
    assert n == (V, Fc) and (faces.view(np.uint8)[Fc - 1] == PAT).all()
    assert np.array_equal(faces[:Fc - 1], c["faces"][:Fc - 1]) and np.array_equal(_bits(v), _bits(c["vertices"]))
    v, faces, n = _raw_emit(c["f"], c["origin"], c["voxel"], c["dims"], V, Fc, vcap=0, fcap=0, expect_error=ERR_CAPACITY)
    assert n == (V, Fc) and (v.view(np.uint8) == PAT).all() and (faces.view(np.uint8) == PAT).all()


def test_purity_and_dirty_workspaces(dev):
    c = RO.solved("sparse_min1")
    a, ca = _raw_field(c)
    b, cb = _raw_field(c, ws_fill=0x3C)
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(ca, cb)
    V, Fc = _raw_count(a, c["dims"])
    assert (V, Fc) == _raw_count(a, c["dims"], ws_fill=0xFF) == _raw_count(a, c["dims"], ws_fill=0)
    first = _raw_emit(a, c["origin"], c["voxel"], c["dims"], V, Fc)
    for fill in (0xFF, 0x3C, 0):
        again = _raw_emit(a, c["origin"], c["voxel"], c["dims"], V, Fc, ws_fill=fill)
        assert np.array_equal(_bits(first[0]), _bits(again[0])) and np.array_equal(first[1], again[1]) and first[2] == again[2]


def test_scan_carry_on_a_long_lattice(dev):
    """The sphere's f as a pattern at both ends of a 14 x 14 x 85,700 lattice that is invalid in between: 257 level-1 sums, so the
    level-2 workgroup takes a second step and its carry holds the first block's counts.  origin 0 and voxel 0.25 make every
    lattice coordinate exact, so the second block's vertices are the oracle's for a lattice shifted by 85,686 voxels, bit for bit."""
    pat = RO.solved("sphere")["f"]
    nz = 85700
    dims = (14, 14, nz)
    assert (14 * 14 * nz + 255) // 256 > 256 * 256
    f = torch.full((14 * 14 * nz,), float("nan"), device=dev)
    f[:pat.shape[0]] = _t(pat, dev)
    f[-pat.shape[0]:] = _t(pat, dev)
    va, fa = RO.extract(pat, (0.0, 0.0, 0.0), 0.25, (14, 14, 14))
    vb, fb = RO.extract(pat, (0.0, 0.0, 0.25 * (nz - 14)), 0.25, (14, 14, 14))
    V, Fc = _raw_count(f, dims)
    assert (V, Fc) == (2 * len(va), 2 * len(fa))
    v, faces, n = _raw_emit(f, (0.0, 0.0, 0.0), 0.25, dims, V, Fc)
    assert n == (V, Fc) and np.array_equal(faces, np.concatenate([fa, fb + len(va)]))
    assert np.array_equal(_bits(v), _bits(np.concatenate([va, vb])))


def _captured(run):
    """``run`` eagerly and from a captured graph -> (the eager outputs, the replayed ones, cleared before the replay)"""
    eager = run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
        with torch.cuda.graph(g, stream=side):
            captured = run()
    torch.cuda.current_stream().wait_stream(side)
    for x in captured:
        x.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    return eager, captured


def test_graph_capture_of_the_field_and_of_the_emit_phase(dev):
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    c = RO.solved("plate")
    x, nrm = _t(c["xyz"], dev), _t(c["normals"], dev)
    N, P = x.shape[0], int(np.prod(c["dims"]))
    go = (C.c_float * 3)(*x.min(0).values.cpu().tolist())
    fbytes, sbytes = L.pn_recon_field_workspace_bytes(N), L.pn_recon_workspace_bytes(*c["dims"])
    ws_f = torch.empty(fbytes, dtype=torch.uint8, device=dev)
    ws_s = torch.empty(sbytes, dtype=torch.uint8, device=dev)

    def field():
        f = torch.empty(P, device=dev)
        cnt = torch.empty(P, device=dev, dtype=torch.int32)
        _lib.check(L.pn_recon_field(_lib.ptr(x), _lib.ptr(nrm), N, c["radius"], go, _d3(c["origin"]), c["voxel"], *c["dims"], c["min_points"],
                                    _lib.ptr(f), _lib.ptr(cnt), _lib.ptr(ws_f), fbytes, _lib.current_stream()), "pn_recon_field")
        return f, cnt

    eager, replayed = _captured(field)
    assert all(np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8)) for a, b in zip(eager, replayed))
    _check_field("plate (replayed)", replayed[0].cpu().numpy(), replayed[1].cpu().numpy(), c)
    f = eager[0]
    V, Fc = len(c["vertices"]), len(c["faces"])

    def emit():
        v = torch.empty(V, 3, device=dev)
        faces = torch.empty(Fc, 3, device=dev, dtype=torch.int32)
        n = torch.empty(2, device=dev, dtype=torch.int32)
        _lib.check(L.pn_recon_emit(_lib.ptr(f), _d3(c["origin"]), c["voxel"], *c["dims"], _lib.ptr(v), V, _lib.ptr(faces), Fc, _lib.ptr(n),
                                   _lib.ptr(ws_s), sbytes, _lib.current_stream()), "pn_recon_emit")
        return v, faces, n

    eager, replayed = _captured(emit)
    assert all(np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8)) for a, b in zip(eager, replayed))
    assert replayed[2].tolist() == [V, Fc] and np.array_equal(replayed[1].cpu().numpy(), c["faces"])
    assert np.abs(replayed[0].cpu().numpy().astype(np.float64) - c["vertices"]).max() <= 1e-6 * c["voxel"]
    assert int(ws_s[:4].view(torch.int32).item()) == 0 and int(ws_f[:4].view(torch.int32).item()) == 0


# ---- the ops level ------------------------------------------------------------------------------------------------------
def test_ops_drop_unusable_rows_and_build_the_default_lattice(dev):
    from pointcloudprocessing_amd import ops
    c = RO.solved("sphere")
    x, n = c["xyz"].copy(), c["normals"].copy()
    bad_x = np.array([[np.nan, 0, 0], [0, np.inf, 0], [5, 5, 5], [6, 6, 6], [7, 7, 7]], F32)
    bad_n = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0], [np.nan, 0, 1], [0, -np.inf, 0]], F32)
    at = [0, 100, 100, 250, 400]                                            # in front, inside, behind
    xs, ns = np.insert(x, at, bad_x, 0), np.insert(n, at, bad_n, 0)
    for pts, nrm in ((x, n), (xs, ns)):
        f, origin, dims, count = ops.implicit_field(_t(pts, dev), _t(nrm, dev), c["voxel"], c["radius"], return_count=True)
        assert dims == c["dims"] == (14, 14, 14) and np.array_equal(np.asarray(origin), c["origin"]) and tuple(f.shape) == (14, 14, 14)
        _check_field("ops.implicit_field", f.cpu().numpy().reshape(-1), count.cpu().numpy().reshape(-1), c)
        v, faces, lab = ops.reconstruct_mesh(_t(pts, dev), _t(nrm, dev), c["voxel"], c["radius"])
        assert lab is None and np.array_equal(faces.cpu().numpy(), c["faces"])
        assert np.abs(v.cpu().numpy().astype(np.float64) - c["vertices"]).max() <= 1e-6 * c["voxel"]
    # a lattice given by hand; radius = None is 3 voxels
    f, origin, dims = ops.implicit_field(_t(x, dev), _t(n, dev), 0.25, 0.6, origin=(-1.5, -1.25, -1.0), dims=(13, 11, 9))
    ef, _ = RO.field(x, n, 0.6, (-1.5, -1.25, -1.0), 0.25, (13, 11, 9))
    assert tuple(f.shape) == (9, 11, 13) and origin == (-1.5, -1.25, -1.0) and dims == (13, 11, 9)
    got = f.cpu().numpy().reshape(-1)
    ok = ~np.isnan(ef)
    assert np.array_equal(np.isnan(got), ~ok) and (np.abs(got[ok].astype(np.float64) - ef[ok]) <= 2.0 ** -22 * np.abs(ef[ok])).all()
    v3, f3, _ = ops.reconstruct_mesh(_t(x, dev), _t(n, dev), 0.2)
    o3, d3 = RO.default_lattice(x, 0.2, 3 * 0.2)
    e3 = RO.extract(RO.field(x, n, 3 * 0.2, o3, 0.2, d3)[0], o3, 0.2, d3)
    assert np.array_equal(f3.cpu().numpy(), e3[1]) and np.abs(v3.cpu().numpy().astype(np.float64) - e3[0]).max() <= 1e-6 * 0.2


def test_reconstruct_mesh_labels_the_hemispheres(dev):
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd._lib import PointNetHipError
    c = RO.solved("sphere")
    lab = (c["xyz"][:, 2] > 0).astype(np.int32)
    v, faces, fl = ops.reconstruct_mesh(_t(c["xyz"], dev), _t(c["normals"], dev), c["voxel"], c["radius"], labels=_t(lab, dev), n_labels=2)
    assert np.array_equal(faces.cpu().numpy(), c["faces"])
    fl, cz = fl.cpu().numpy(), v.cpu().numpy()[c["faces"]].mean(1)[:, 2]
    assert fl.dtype == np.int32 and fl.shape == (len(c["faces"]),) and ((fl == 0) | (fl == 1)).all()
    far = np.abs(cz) > c["radius"]
    assert far.sum() > 400 and np.array_equal(fl[far], (cz[far] > 0).astype(np.int32))
    with pytest.raises(PointNetHipError, match="outside"):
        ops.reconstruct_mesh(_t(c["xyz"], dev), _t(c["normals"], dev), c["voxel"], c["radius"], labels=_t(lab + 1, dev), n_labels=2)


def test_scans_to_mesh_to_mesh_icp(dev):
    """Six frames of the LiDAR tests' aircraft (level 1) from one side and above, so that every thin part is seen from one side only;
    five of them, moved by their true poses, become a labelled mesh (voxel 0.12 m, radius 0.36 m: the field's zero lies outside
    the points of a convex surface by about radius^2 / (8 R), and the surface runs on past the edge of the data by up to a radius,
    so the radius is what the residual depends on), and the sixth is registered against that mesh from 5 degrees and 0.3 m off.
    Measured on the MI355X: 0.0076 degrees and 0.015 m at this voxel (0.048 m at voxel 0.17, 0.095 m at 0.25, all along the
    fuselage axis; against the true mesh the same frame ends at 0.0000 degrees, 0.0000 m).  The end state must be closer to the truth than a tenth of the start offset in rotation
    and in translation: a sanity bound, not the expected accuracy (DESIGN.md section 7 has the residuals measured)."""
    import icp_mesh_oracle as MO
    import icp_oracle as IO
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd.pointcloud import look_at_pose, pinhole_rays
    NM, VOXEL = len(MO.MESH_PARTS), 0.12
    ref = ops.icp_mesh_reference(*MO.aircraft_mesh(1), NM, device=dev)
    az, el, dist = np.deg2rad([25, 55, 85, 115, 145, 70]), np.deg2rad([25, 45, 30, 50, 25, 38]), [46, 50, 44, 52, 47, 48]
    poses = np.stack([look_at_pose(d * np.array([np.cos(a) * np.cos(e), np.sin(a) * np.cos(e), np.sin(e)])) for a, e, d in zip(az, el, dist)])
    N = 8192
    xyz, part, _, count = ops.lidar_frames(ref, poses, pinhole_rays(192, 256, 50.0, 40.0), N)      # returns about 0.17 m apart
    assert int(count.min()) > 7000 and int(count[5]) >= N               # (a frame with fewer hits repeats some: coincident points)
    to_model = torch.from_numpy(np.linalg.inv(poses[:5])).to(dev)
    v, faces, fl = ops.scans_to_mesh([xyz[i] for i in range(5)], to_model, VOXEL, labels=[part[i] for i in range(5)], n_labels=NM)
    assert len(faces) > 50000 and int(fl.min()) >= 0 and int(fl.max()) < NM and len(torch.unique(fl)) == NM
    mesh = ops.icp_mesh_reference(v, faces, fl, NM)
    true = poses[5]
    start = true.copy()
    start[:3, :3] = IO.rot([1.0, -2.0, 0.5], np.deg2rad(5.0)) @ true[:3, :3]
    start[:3, 3] += np.array([0.2, -0.2, 0.1])
    a0, t0 = IO.pose_error(start, true)
    assert abs(np.rad2deg(a0) - 5.0) < 1e-6 and abs(t0 - 0.3) < 1e-9
    g = ops.semantic_icp(xyz[5:6].contiguous(), part[5:6].contiguous(), mesh, _t(start[None], dev), metric="plane", max_iters=30)
    a1, t1 = IO.pose_error(g[0][0].cpu().numpy(), true)
    print(f"mesh of {len(v)} vertices, {len(faces)} faces; start {np.rad2deg(a0):.3f} deg {t0:.3f} m -> end {np.rad2deg(a1):.4f} deg {t1:.4f} m")
    assert a1 < a0 / 10 and t1 < t0 / 10, (a1, t1)
