"""Surface reconstruction without a GPU: the surface is declared, exported and bound; every argument refusal of pn_recon_field /
pn_recon_count / pn_recon_emit runs before a HIP call; the workspace sizers; the NumPy oracle's own facts (tests/recon_oracle.py) on
the cases the GPU test compares against -- the sphere is closed, oriented, of Euler characteristic 2 and without an unused vertex,
the plate has at most two faces per edge and every normal has +z, every comparison case keeps min |f| > 1e-9 over its valid lattice
points except the one that puts f = 0 on lattice points on purpose -- and the OBJ round trip of write_labelled_mesh."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import recon_oracle as RO
from helpers import ROOT

F32 = np.float32
INVALID = -1


def test_surface_is_declared_and_exported():
    from pointcloudprocessing_amd import _lib, ops, pointcloud
    hdr = open(os.path.join(ROOT, "include", "pointnet_hip.h")).read()
    for decl in ("#define PN_RECON_MAX_LATTICE (1 << 28)", "size_t pn_recon_field_workspace_bytes(int N);",
                 "int pn_recon_field(const float* xyz, const float* normals, int N, float radius, const float* grid_origin3_host,",
                 "size_t pn_recon_workspace_bytes(int nx, int ny, int nz);", "int pn_recon_count(const float* f, int nx, int ny, int nz,",
                 "int pn_recon_emit(const float* f, const double* lattice_origin3_host, double voxel, int nx, int ny, int nz,",
                 "m=3: 02 03 13, 02 13 12", "t = fa / (fa - fb)", "u = 1 - d_j / r2; w = u*u", "a sparse (narrow-band) lattice is out of scope"):
        assert decl in hdr, decl
    assert "#define PN_ABI_VERSION 6" in hdr and _lib.lib().pn_abi_version() == 6 == _lib.ABI_VERSION      # additive: the version stays
    for name in ("pn_recon_field_workspace_bytes", "pn_recon_field", "pn_recon_workspace_bytes", "pn_recon_count", "pn_recon_emit"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert len(_lib.SIGNATURES["pn_recon_field"][1]) == 16 and _lib.SIGNATURES["pn_recon_field"][1][6] is C.c_double
    assert len(_lib.SIGNATURES["pn_recon_count"][1]) == 8 and len(_lib.SIGNATURES["pn_recon_emit"][1]) == 14
    assert _lib.PN_RECON_MAX_LATTICE == RO.MAX_LATTICE == 1 << 28
    par = inspect.signature(ops.implicit_field).parameters
    assert list(par)[:7] == ["xyz", "normals", "voxel", "radius", "min_points", "origin", "dims"]
    assert [par[k].default for k in list(par)[4:7]] == [3, None, None]
    par = inspect.signature(ops.reconstruct_mesh).parameters
    assert list(par) == ["xyz", "normals", "voxel", "radius", "min_points", "labels", "n_labels", "label_k"]
    assert [par[k].default for k in list(par)[3:]] == [None, 3, None, 0, 3]
    par = inspect.signature(ops.scans_to_mesh).parameters
    assert list(par) == ["clouds", "poses", "voxel", "radius", "normals_radius", "normals_k", "labels", "n_labels", "min_points"]
    assert [par[k].default for k in list(par)[3:]] == [None, None, 8, None, 0, 3]
    assert list(inspect.signature(pointcloud.write_labelled_mesh).parameters) == ["path", "vertices", "faces", "face_labels", "part_names"]


def _p(a):
    return C.c_void_p(a) if a else None      # (never dereferenced: the checks run before any HIP call)


def _d3(v):
    return (C.c_double * 3)(*v) if v else None


def _field(xyz=0x1000, nrm=0x1000, N=8, radius=1.0, go=(0.0, 0.0, 0.0), lo=(0.0, 0.0, 0.0), voxel=0.5, dims=(4, 5, 6), min_points=3, f=0x1000,
           count=0, ws=0x1000, ws_bytes=None):
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    if ws_bytes is None:
        ws_bytes = L.pn_recon_field_workspace_bytes(N)
    rc = L.pn_recon_field(_p(xyz), _p(nrm), N, radius, (C.c_float * 3)(*go) if go else None, _d3(lo), voxel, *dims, min_points, _p(f), _p(count),
                          _p(ws), ws_bytes, None)
    return rc, L.pn_last_error()


def _count(f=0x1000, dims=(4, 5, 6), n_out=0x1000, ws=0x1000, ws_bytes=None):
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    if ws_bytes is None:
        ws_bytes = L.pn_recon_workspace_bytes(*dims)
    rc = L.pn_recon_count(_p(f), *dims, _p(n_out), _p(ws), ws_bytes, None)
    return rc, L.pn_last_error()


def _emit(f=0x1000, lo=(0.0, 0.0, 0.0), voxel=0.5, dims=(4, 5, 6), v=0x1000, vcap=10, faces=0x1000, fcap=10, n_out=0x1000, ws=0x1000,
          ws_bytes=None):
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    if ws_bytes is None:
        ws_bytes = L.pn_recon_workspace_bytes(*dims)
    rc = L.pn_recon_emit(_p(f), _d3(lo), voxel, *dims, _p(v), vcap, _p(faces), fcap, _p(n_out), _p(ws), ws_bytes, None)
    return rc, L.pn_last_error()


BIG = dict(ws_bytes=1 << 40)      # (for shapes whose sizer gives 0: the shape is what is refused)


@pytest.mark.parametrize("call,kw,msg", [
    (_field, dict(xyz=0), b"null pointer"), (_field, dict(nrm=0), b"null pointer"), (_field, dict(f=0), b"null pointer"),
    (_field, dict(go=None), b"null pointer"), (_field, dict(lo=None), b"null pointer"),
    (_field, dict(voxel=0.0), b"voxel"), (_field, dict(voxel=-1.0), b"voxel"), (_field, dict(voxel=float("nan")), b"voxel"),
    (_field, dict(voxel=float("inf")), b"voxel"), (_field, dict(radius=0.0), b"radius"), (_field, dict(radius=-1.0), b"radius"),
    (_field, dict(radius=float("nan")), b"radius"), (_field, dict(radius=1e-30), b"radius * radius"),
    (_field, dict(dims=(1, 5, 6)), b"at least 2"), (_field, dict(dims=(4, 1, 6)), b"at least 2"), (_field, dict(dims=(4, 5, 0)), b"at least 2"),
    (_field, dict(dims=(1 << 14, 1 << 14, 2)), b"more than 2^28"), (_field, dict(dims=(1 << 16, 1 << 16, 1 << 16)), b"more than 2^28"),
    (_field, dict(dims=(2, 2, (1 << 26) + 1)), b"more than 2^28"),
    (_field, dict(dims=(1 << 20, 2, 2), voxel=0.5, radius=1.0), b"key limit"), (_field, dict(dims=(2, 2, 40000), voxel=1.0, radius=2.0), b"key limit"),
    (_field, dict(lo=(0.0, float("inf"), 0.0)), b"finite fp32 range"), (_field, dict(lo=(3e38, 0.0, 0.0), voxel=1e37, dims=(16, 2, 2)), b"finite fp32 range"),
    (_field, dict(go=(0.0, float("nan"), 0.0)), b"origin"), (_field, dict(min_points=0), b"min_points"),
    (_field, dict(N=0, **BIG), b"N must be"), (_field, dict(ws=0), b"workspace"), (_field, dict(ws_bytes=64), b"workspace too small"),
    (_field, dict(ws=0x1008), b"16-byte aligned"),
    (_count, dict(f=0), b"null pointer"), (_count, dict(n_out=0), b"null pointer"), (_count, dict(dims=(1, 5, 6), **BIG), b"at least 2"),
    (_count, dict(dims=(1 << 14, 1 << 14, 2), **BIG), b"more than 2^28"), (_count, dict(ws=0), b"workspace"),
    (_count, dict(ws_bytes=64), b"workspace too small"), (_count, dict(ws=0x1008), b"16-byte aligned"),
    (_emit, dict(f=0), b"null pointer"), (_emit, dict(n_out=0), b"null pointer"), (_emit, dict(lo=None), b"null pointer"),
    (_emit, dict(v=0), b"null pointer"), (_emit, dict(faces=0), b"null pointer"), (_emit, dict(vcap=-1), b"negative capacity"),
    (_emit, dict(fcap=-1), b"negative capacity"), (_emit, dict(voxel=0.0), b"voxel"), (_emit, dict(dims=(4, 5, 1), **BIG), b"at least 2"),
    (_emit, dict(dims=(2, 1 << 14, 1 << 14), **BIG), b"more than 2^28"), (_emit, dict(ws=0), b"workspace"),
    (_emit, dict(ws_bytes=64), b"workspace too small"), (_emit, dict(ws=0x1008), b"16-byte aligned"),
])
def test_argument_checks_without_gpu(call, kw, msg):
    rc, err = call(**kw)
    assert rc == INVALID and msg in err, err


def test_workspace_sizes():
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    for n in (1, 255, 4096, 100000):
        assert L.pn_recon_field_workspace_bytes(n) == L.pn_radius_knn_workspace_bytes(n) > 0
    assert L.pn_recon_field_workspace_bytes(0) == 0
    shapes = ((2, 2, 2), (16, 14, 6), (14, 14, 14), (45, 45, 45), (300, 300, 300), (1 << 14, 1 << 14, 1))
    sizes = [L.pn_recon_workspace_bytes(*s) for s in shapes[:-1]]
    assert all(b > a for a, b in zip(sizes, sizes[1:]))
    assert all(s >= 8 * int(np.prod(d)) + 256 for s, d in zip(sizes, shapes))          # the edge words and the first vertex of every point
    for bad in ((1, 5, 5), (5, 0, 5), (5, 5, -3), (1 << 14, 1 << 14, 2), (1 << 16, 1 << 16, 1 << 16), (1 << 14, 1 << 14, 1)):
        assert L.pn_recon_workspace_bytes(*bad) == 0
    assert L.pn_recon_workspace_bytes(1 << 14, 1 << 13, 2) > 0                          # exactly 2^28 points


def test_ops_wrappers_refuse_cpu_tensors_and_bad_shapes():
    import torch
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd._lib import PointNetHipError
    x = torch.zeros(8, 3)
    for call in (lambda: ops.implicit_field(x, x, 0.1, 0.3), lambda: ops.reconstruct_mesh(x, x, 0.1), lambda: ops.reconstruct_mesh(np.zeros((8, 3), F32), x, 0.1),
                 lambda: ops.scans_to_mesh([x], torch.eye(4)[None], 0.1), lambda: ops.scans_to_mesh(x, torch.eye(4)[None], 0.1),
                 lambda: ops.scans_to_mesh([x], torch.eye(4), 0.1), lambda: ops.scans_to_mesh([x], torch.eye(4)[None], 0.1, labels=[x, x])):
        with pytest.raises(PointNetHipError):                               # no CPU fallback
            call()


# ---- the oracle's own facts ---------------------------------------------------------------------------------------------
def test_the_table_is_complementary_and_uses_each_crossed_edge():
    """a mask and its complement give the same triangles reversed, over exactly the edges whose ends differ"""
    for m in range(1, 15):
        n = int(RO.NTRI[m])
        assert n == int(RO.NTRI[15 - m]) == (2 if bin(m).count("1") == 2 else 1)
        tri = [tuple(map(tuple, t)) for t in RO.TRI[m][:n]]
        crossed = {(p, q) for p in range(4) for q in range(p + 1, 4) if ((m >> p) & 1) != ((m >> q) & 1)}
        assert {e for t in tri for e in t} == crossed
        directed = lambda ts: {(t[k], t[(k + 1) % 3]) for t in ts for k in range(3)}                # noqa: E731
        other = [tuple(map(tuple, t)) for t in RO.TRI[15 - m][:n]]
        inner = {e for e in directed(tri) if (e[1], e[0]) in directed(tri)}                         # the quad's diagonal
        assert {(b, a) for a, b in directed(tri) - inner} == directed(other) - {e for e in directed(other) if (e[1], e[0]) in directed(other)}
    assert RO.NTRI[0] == RO.NTRI[15] == 0


def test_a_linear_field_gives_a_plane_with_its_gradient_as_normal():
    """f = g . x - c on every lattice point, for gradients in all octants: every face normal is along +g, every vertex on the plane,
    the patch is oriented and has no crack (every inner edge in two faces)"""
    dims, origin, voxel = (7, 6, 5), np.array([-0.3, 0.2, -1.0]), 0.25
    ax = RO.lattice_axes(origin, voxel, dims)
    Z, Y, X = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    for g in ((1, 2, 3), (-1, 2, 3), (1, -2, 3), (1, 2, -3), (-3, -1, -2), (0, 0, 1), (1, 0, 0), (0, -1, 0), (1, 1, 0)):
        g = np.array(g, np.float64) / np.linalg.norm(g)
        c = g @ (origin + 0.5 * voxel * (np.array(dims) - 1)) + 0.013
        f = (g[0] * X + g[1] * Y + g[2] * Z - c).astype(F32).reshape(-1)
        v, faces = RO.extract(f, origin, voxel, dims)
        assert len(faces) > 20 and RO.oriented(faces) and RO.unused_vertices(len(v), faces) == 0 and RO.edge_face_counts(faces).max() == 2
        n = RO.face_normals(v, faces)
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        assert (n @ g > 1 - 1e-5).all() and np.abs(v.astype(np.float64) @ g - c).max() < 1e-6
        assert RO.euler(len(v), faces) == 1                                                          # a disc


def test_sphere_facts():
    c = RO.solved("sphere")
    v, f = c["vertices"], c["faces"]
    assert c["dims"] == (14, 14, 14) and (len(v), len(f)) == (946, 1888)
    assert RO.closed(f) and RO.oriented(f) and RO.euler(len(v), f) == 2 and RO.unused_vertices(len(v), f) == 0
    n, cen = RO.face_normals(v, f), v[f].astype(np.float64).mean(1)
    assert ((n * cen).sum(1) > 0).all()                                   # outwards: the way the input normals face
    r = np.linalg.norm(v.astype(np.float64), axis=1)
    assert 1.0 < r.min() and r.max() < 1.08                               # IMLS's outward bias on a convex surface
    big = RO.solved("sphere_large")
    assert big["dims"] == (45, 45, 45) and RO.closed(big["faces"]) and RO.oriented(big["faces"]) and RO.euler(len(big["vertices"]), big["faces"]) == 2
    assert 45 ** 3 > 256 * 256 and 44 ** 3 > 256 * 256                    # the third level of both scans


def test_plate_facts():
    for name, dims in (("plate", (16, 14, 6)), ("layer", (37, 5, 2))):
        c = RO.solved(name)
        v, f = c["vertices"], c["faces"]
        counts = RO.edge_face_counts(f)
        assert c["dims"] == dims and len(f) > 500 and counts.max() == 2 and (counts == 1).sum() > 50 and RO.oriented(f)
        assert (RO.face_normals(v, f)[:, 2] > 0).all() and np.abs(v[:, 2] - 0.03).max() < 1e-6
        assert RO.unused_vertices(len(v), f) == 0 and np.isnan(c["f"]).any()          # the rim's tetrahedra have invalid corners


def test_margins_of_the_comparison_cases():
    for name in RO.CASES:
        c = RO.solved(name)
        least, lo, hi = RO.margins(c["f"], c["count"])
        print(f"{name}: lattice {c['dims']}, min |f| = {least:.3e}, neighbour counts {lo} .. {hi}, V = {len(c['vertices'])}, F = {len(c['faces'])}")
        if name == "plate_on_plane":
            assert least == 0.0 and ((c["f"] == 0) & (c["count"] >= 3)).sum() > 50
        else:
            assert least > 1e-9
        assert lo >= c["min_points"]


def test_zero_is_outside_and_gives_t_equal_one():
    c = RO.solved("plate_on_plane")
    v, f = c["vertices"], c["faces"]
    assert (v[:, 2] == 0).all()                                           # every vertex sits on the outside end: t = 1
    area = np.linalg.norm(RO.face_normals(v, f), axis=1)
    assert (area == 0).sum() > 100 and (area > 0).sum() > 100             # the zero-area faces icp_mesh_reference drops
    assert (RO.face_normals(v, f)[area > 0][:, 2] > 0).all() and RO.oriented(f)


def test_min_points_and_coincident_points():
    a, b = RO.solved("sparse"), RO.solved("sparse_min1")
    assert np.isnan(a["f"]).sum() > np.isnan(b["f"]).sum() and len(b["faces"]) > len(a["faces"])
    assert RO.closed(a["faces"]) and RO.euler(len(a["vertices"]), a["faces"]) == 2      # the strays are below min_points = 3
    same = ~np.isnan(a["f"])
    assert np.array_equal(a["f"][same], b["f"][same]) and np.array_equal(a["count"], b["count"])
    x = a["xyz"]
    assert (x[300:325] == x[:25]).all()                                   # the coincident rows


def test_default_lattice_covers_the_padded_box():
    c = RO.solved("sphere")
    ax = RO.lattice_axes(c["origin"], c["voxel"], c["dims"])
    for a in range(3):
        assert ax[a][0] == float(c["xyz"][:, a].min()) - c["radius"] and ax[a][-1] >= float(c["xyz"][:, a].max()) + c["radius"] > ax[a][-2]


def test_the_field_order_is_the_sorted_grid():
    """the accumulation order: ascending (kz, ky, kx, row) of the points' grid keys"""
    c = RO.solved("sphere")
    order = RO.grid_order(c["xyz"], c["radius"])
    h = RO.leaf(c["radius"])
    k = np.floor((c["xyz"] - c["xyz"].min(0)) / h).astype(np.int64)[order]
    rows = np.stack([k[:, 2], k[:, 1], k[:, 0], order], 1)
    assert (np.lexsort(rows.T[::-1]) == np.arange(len(order))).all() and float(h) >= 0.6 * (1 + 2.0 ** -6)


# ---- the OBJ round trip -------------------------------------------------------------------------------------------------
def test_write_and_read_labelled_mesh(tmp_path):
    from pointcloudprocessing_amd.pointcloud import read_labelled_mesh, write_labelled_mesh
    c = RO.solved("sphere")
    v, f = c["vertices"], c["faces"]
    lab = (v[f].mean(1)[:, 2] > 0).astype(np.int32) + 2 * (v[f].mean(1)[:, 0] > 0.5).astype(np.int32)      # interleaved along the face list
    names = ["south", "north", "south east", "cap"]
    path = str(tmp_path / "mesh.obj")
    write_labelled_mesh(path, v, f, lab, names)
    v2, f2, l2 = read_labelled_mesh(path, names)
    assert v2.dtype == F32 and np.array_equal(v2.view(np.uint32), v.view(np.uint32)) and np.array_equal(f2, f) and np.array_equal(l2, lab)
    text = open(path).read()
    assert all(f"g {n}\n" in text for n in names) and text.count("\nf ") == len(f)
    for bad in (dict(face_labels=lab[:-1]), dict(face_labels=lab + 3), dict(faces=f + len(v)), dict(part_names=["a", "a", "b", "c"]),
                dict(part_names=["a", "", "b", "c"])):
        kw = dict(dict(vertices=v, faces=f, face_labels=lab, part_names=names), **bad)
        with pytest.raises(ValueError):
            write_labelled_mesh(path, **kw)
    write_labelled_mesh(path, v[:0], f[:0], lab[:0], names)
    v0, f0, l0 = read_labelled_mesh(path, names)
    assert v0.shape == (0, 3) and f0.shape == (0, 3) and l0.shape == (0,)
