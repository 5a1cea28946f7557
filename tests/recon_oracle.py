"""NumPy restatement of pn_recon_field / pn_recon_count / pn_recon_emit (include/pointnet_hip.h): the IMLS field of an oriented
cloud on a dense lattice and marching tetrahedra over it; the facts a reconstructed mesh is tested for (closed, oriented, Euler
characteristic, unused vertices, margins); and the clouds the CPU and GPU tests share.  NumPy only.

The search is brute force: every point visits the block of lattice points its radius can reach, the points taken in ascending
(grid key, row) -- the accumulation order the header fixes -- so every lattice point's fp64 sums run in that order."""
import numpy as np

F32 = np.float32
MAX_KEY = 1 << 14
MAX_LATTICE = 1 << 28

# corner codes (dx | dy << 1 | dz << 2) of the six tetrahedra, permutations in lexicographic order; numbers 1, 2, 5 are odd
CODE = np.array([[0, 1, 3, 7], [0, 1, 5, 7], [0, 2, 3, 7], [0, 2, 6, 7], [0, 4, 5, 7], [0, 4, 6, 7]])
ODD = np.array([0, 1, 1, 0, 0, 1], bool)
TYPE_OF_DIR = np.array([-1, 0, 1, 3, 2, 4, 5, 6])      # direction code -> edge type
DIR_OF_TYPE = np.array([1, 2, 4, 3, 5, 6, 7])
# the header's table: inside mask -> triangles of an even permutation, corners as edges (p, q) of the tetrahedron
_T = {1: "01 02 03", 2: "01 13 12", 4: "02 12 23", 8: "03 23 13", 14: "01 03 02", 13: "01 12 13", 11: "02 23 12", 7: "03 13 23",
      3: "02 03 13 02 13 12", 12: "02 12 13 02 13 03", 5: "03 01 12 03 12 23", 10: "12 01 03 12 03 23", 9: "01 02 23 01 23 13",
      6: "01 13 23 01 23 02"}
NTRI = np.zeros(16, np.int64)
TRI = np.zeros((16, 2, 3, 2), np.int64)                # mask, triangle, corner, (p, q)
for _m, _s in _T.items():
    _e = [(int(t[0]), int(t[1])) for t in _s.split()]
    NTRI[_m] = len(_e) // 3
    TRI[_m].reshape(-1, 2)[:len(_e)] = _e


def leaf(radius):
    """pn_radius_knn_leaf: radius (1 + 2^-6) rounded UP to fp32"""
    exact = float(F32(radius)) * (1.0 + 1.0 / 64.0)
    h = F32(exact)
    return h if float(h) >= exact else np.nextafter(h, F32(np.inf))


def default_lattice(xyz, voxel, radius):
    """ops.implicit_field's default: the bounding box of the points padded by the radius -> (origin (3,) float64, dims (nx, ny, nz))"""
    lo, hi = xyz.min(0).astype(np.float64), xyz.max(0).astype(np.float64)
    origin = lo - float(radius)
    dims = np.maximum(np.ceil(((hi + float(radius)) - origin) / float(voxel)).astype(np.int64) + 1, 2)
    return origin, tuple(int(d) for d in dims)


def lattice_axes(origin, voxel, dims):
    """per axis the fp64 coordinates origin + i * voxel (one multiply, one add)"""
    return [np.float64(origin[a]) + np.arange(dims[a], dtype=np.float64) * np.float64(voxel) for a in range(3)]


def grid_order(xyz, radius, grid_origin=None):
    """the rows of xyz in ascending (grid key, row): the order of the sorted grid"""
    h = leaf(radius)
    go = (xyz.min(0) if grid_origin is None else np.asarray(grid_origin)).astype(F32)
    k = np.floor((xyz.astype(F32) - go) / h).astype(np.int64)
    assert (k >= 0).all() and (k < MAX_KEY).all(), "a grid key outside the limit"
    return np.argsort((k[:, 2] << 42) | (k[:, 1] << 21) | k[:, 0], kind="stable")


def field(xyz, normals, radius, origin, voxel, dims, min_points=3, grid_origin=None):
    """-> (f (nx*ny*nz,) float32 with NaN where invalid, count (nx*ny*nz,) int32)"""
    xyz, normals = np.asarray(xyz, F32), np.asarray(normals, F32)
    nx, ny, nz = dims
    r2 = F32(radius) * F32(radius)
    r2d = np.float64(r2)
    ax64 = lattice_axes(origin, voxel, dims)
    ax32 = [a.astype(F32) for a in ax64]
    axw = [a.astype(np.float64) for a in ax32]                     # the fp32 coordinates, widened
    num, den = np.zeros((nz, ny, nx)), np.zeros((nz, ny, nx))
    count = np.zeros((nz, ny, nx), np.int32)
    reach = float(radius) * (1.0 + 1e-5) + 1e-30
    for j in grid_order(xyz, radius, grid_origin):
        p, n = xyz[j], normals[j].astype(np.float64)
        sl = []
        for a in range(3):
            lo = int(np.searchsorted(ax64[a], float(p[a]) - reach, "left")) - 1
            hi = int(np.searchsorted(ax64[a], float(p[a]) + reach, "right")) + 1
            sl.append(slice(max(lo, 0), min(hi, dims[a])))
        dx, dy, dz = ax32[0][sl[0]] - p[0], ax32[1][sl[1]] - p[1], ax32[2][sl[2]] - p[2]
        d = ((dx * dx)[None, None, :] + (dy * dy)[None, :, None]) + (dz * dz)[:, None, None]
        assert d.dtype == F32
        keep = d <= r2
        if not keep.any():
            continue
        u = 1.0 - d.astype(np.float64) / r2d
        w = u * u
        ex, ey, ez = axw[0][sl[0]] - np.float64(p[0]), axw[1][sl[1]] - np.float64(p[1]), axw[2][sl[2]] - np.float64(p[2])
        e = ((ex * n[0])[None, None, :] + (ey * n[1])[None, :, None]) + (ez * n[2])[:, None, None]
        blk = (sl[2], sl[1], sl[0])
        num[blk] += np.where(keep, w * e, 0.0)        # (+ 0.0 leaves a sum as it is: a sum that is -0.0 does not occur, it starts at +0.0)
        den[blk] += np.where(keep, w, 0.0)
        count[blk] += keep
    valid = (count >= int(min_points)) & (den > 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(valid, (num / den).astype(F32), F32(np.nan)).astype(F32)
    return f.reshape(-1), count.reshape(-1)


def _offset(code, nx, nxy):
    return (code & 1) + ((code >> 1) & 1) * nx + ((code >> 2) & 1) * nxy


def extract(f, origin, voxel, dims):
    """marching tetrahedra over f (nx*ny*nz,) -> (vertices (V, 3) float32, faces (F, 3) int32), in the header's orders"""
    nx, ny, nz = dims
    nxy, P = nx * ny, nx * ny * nz
    f = np.asarray(f, F32).reshape(-1)
    assert f.shape[0] == P
    valid, inside = ~np.isnan(f), f < 0
    iz, iy, ix = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    L0 = ((iz * ny + iy) * nx + ix).reshape(-1)                    # ascending
    order_key, slots = [], []
    for perm in range(6):
        Lc = np.stack([L0 + _offset(int(c), nx, nxy) for c in CODE[perm]], 1)          # (C, 4)
        ok = valid[Lc].all(1)
        m = (inside[Lc] * (1 << np.arange(4))).sum(1)
        nt = np.where(ok, NTRI[m], 0)
        for t in range(2):
            sel = np.nonzero(nt > t)[0]
            if not sel.size:
                continue
            pq = TRI[m[sel], t]                                    # (S, 3, 2)
            cp, cq = CODE[perm][pq[..., 0]], CODE[perm][pq[..., 1]]
            slot = (L0[sel, None] + _offset(cp, nx, nxy)) * 7 + TYPE_OF_DIR[cq ^ cp]
            if ODD[perm]:
                slot = slot[:, [0, 2, 1]]
            order_key.append(L0[sel] * 12 + perm * 2 + t)
            slots.append(slot)
    if not slots:
        return np.zeros((0, 3), F32), np.zeros((0, 3), np.int32)
    order_key, slots = np.concatenate(order_key), np.concatenate(slots)
    slots = slots[np.argsort(order_key, kind="stable")]
    used = np.unique(slots)                                        # ascending (owner, type)
    faces = np.searchsorted(used, slots).astype(np.int32)
    L, typ = used // 7, used % 7
    dirc = DIR_OF_TYPE[typ]
    Lb = L + _offset(dirc, nx, nxy)
    fl, fu = f[L].astype(np.float64), f[Lb].astype(np.float64)
    low_in = f[L] < 0
    assert (low_in != (f[Lb] < 0)).all()
    fa, fb = np.where(low_in, fl, fu), np.where(low_in, fu, fl)
    t = fa / (fa - fb)
    idx = [L % nx, (L // nx) % ny, L // nxy]
    v = np.empty((used.shape[0], 3), F32)
    for a in range(3):
        step = (dirc >> a) & 1
        plo = np.float64(origin[a]) + idx[a].astype(np.float64) * np.float64(voxel)
        phi = np.float64(origin[a]) + (idx[a] + step).astype(np.float64) * np.float64(voxel)
        pa, pb = np.where(low_in, plo, phi), np.where(low_in, phi, plo)
        v[:, a] = (pa + t * (pb - pa)).astype(F32)
    return v, faces


# ---- facts about a mesh ----
def _edges(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def edge_face_counts(faces):
    """how many faces every undirected edge is in"""
    e = np.sort(_edges(faces), 1)
    return np.unique(e, axis=0, return_counts=True)[1]


def closed(faces):
    return bool(len(faces)) and bool((edge_face_counts(faces) == 2).all())


def oriented(faces):
    """every directed edge appears at most once"""
    return bool((np.unique(_edges(faces), axis=0, return_counts=True)[1] == 1).all())


def euler(n_vertices, faces):
    return int(n_vertices) - int(edge_face_counts(faces).shape[0]) + int(len(faces))


def unused_vertices(n_vertices, faces):
    return int(n_vertices) - int(np.unique(np.asarray(faces)).shape[0])


def face_normals(vertices, faces):
    v = np.asarray(vertices, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return np.cross(b - a, c - a)


def margins(f, count):
    """(min |f| over the valid lattice points, the least and the largest neighbour count among them)"""
    ok = ~np.isnan(f)
    return float(np.abs(f[ok]).min()), int(count[ok].min()), int(count[ok].max())


# ---- the shared cases: name -> dict(xyz, normals, voxel, radius, origin, dims, min_points) ----
def sphere_cloud(n, seed, R=1.0):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (R * d).astype(F32), d.astype(F32)


def plate_cloud(n, seed, z, half=(1.2, 1.0)):
    rng = np.random.default_rng(seed)
    xyz = np.stack([rng.uniform(-half[0], half[0], n), rng.uniform(-half[1], half[1], n), np.full(n, z)], 1).astype(F32)
    return xyz, np.tile(np.array([0, 0, 1], F32), (n, 1))


def _case(xyz, normals, voxel, radius, origin=None, dims=None, min_points=3):
    if origin is None:
        origin, dims = default_lattice(xyz, voxel, radius)
    return dict(xyz=xyz, normals=normals, voxel=float(voxel), radius=float(radius), origin=np.asarray(origin, np.float64),
                dims=tuple(dims), min_points=int(min_points))


def make_case(name):
    if name == "sphere":                  # 400 points, lattice 14^3
        return _case(*sphere_cloud(400, 0), 0.25, 0.6)
    if name == "plate":                   # three different dimensions; the rim's tetrahedra have invalid corners
        return _case(*plate_cloud(600, 1, 0.03), 0.25, 0.6, (-1.9, -1.65, -0.6), (16, 14, 6))
    if name == "plate_on_plane":          # f == 0 at the lattice points of the plane z = 0
        return _case(*plate_cloud(600, 2, 0.0), 0.25, 0.6, (-1.75, -1.5, -0.5), (15, 13, 5))
    if name == "sphere_large":            # 45^3 = 91,125 lattice points, 44^3 = 85,184 cubes: both above 256^2
        return _case(*sphere_cloud(2000, 3), 0.0625, 0.35)
    if name == "layer":                   # one layer of cubes (nz = 2), nx = 37: no multiple of a wave
        return _case(*plate_cloud(600, 4, 0.03), 0.1, 0.3, (-1.8, -0.2, -0.02), (37, 5, 2))
    if name in ("sparse", "sparse_min1"):  # coincident points, and two stray points whose neighbourhoods hold 1 and 2 points
        xyz, nrm = sphere_cloud(300, 5)
        stray = np.array([[2.0, 0.1, 0.05], [2.9, -0.2, 0.1], [2.95, -0.15, 0.12]], F32)
        sn = np.array([[1, 0, 0], [0, 0.6, 0.8], [0, 0.6, 0.8]], F32)
        xyz, nrm = np.concatenate([xyz, xyz[:25], stray]), np.concatenate([nrm, nrm[:25], sn])
        return _case(xyz, nrm, 0.25, 0.6, min_points=1 if name == "sparse_min1" else 3)
    raise KeyError(name)


CASES = ("sphere", "plate", "plate_on_plane", "sphere_large", "layer", "sparse", "sparse_min1")
_DONE = {}


def solved(name):
    """the case with the oracle's f, count, vertices and faces; computed once, shared, not to be modified"""
    if name not in _DONE:
        c = make_case(name)
        c["f"], c["count"] = field(c["xyz"], c["normals"], c["radius"], c["origin"], c["voxel"], c["dims"], c["min_points"])
        c["vertices"], c["faces"] = extract(c["f"], c["origin"], c["voxel"], c["dims"])
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _DONE[name] = c
    return _DONE[name]
