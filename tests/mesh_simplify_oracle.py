"""NumPy restatement of pn_mesh_components and pn_mesh_simplify (spec: include/pointnet_hip.h) and the small meshes their tests use.

Every fp32 and fp64 operation of the spec is one NumPy (or Python float) operation here, in the order the header states, so the
device result can be compared bit for bit.  The sums of a cluster run in list order; ``simplify`` walks all clusters in step
(operation k of every cluster at once, element-wise, which changes no rounding) and ``place_scalar`` is the same text one cluster
at a time in Python floats: tests/test_cpu_mesh_simplify.py holds the two against each other.  The Jacobi is the fixed-order
cyclic routine of the library (pn_icp_normals' sym_jacobi) restated without contraction, again in both forms."""
import math

import numpy as np

F32 = np.float32
AXIS_BITS = 21
MAX_CLUSTERS = 1 << AXIS_BITS
ERR_KEY, ERR_INDEX, ERR_NONFINITE, ERR_CLUSTERS, ERR_CAPACITY = 1, 5, 6, 7, 8


# ---- components ---------------------------------------------------------------------------------------------------------
def components(n_vertices, faces):
    """-> (face_component (F,) int32, sizes (K,) int32): a union-find over vertex indices, every face joins its corners 0-1 and
    0-2; ids ascend with the component's lowest referenced vertex; a face takes its first corner's component"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    parent = list(range(n_vertices))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    ref = np.zeros(n_vertices, bool)
    for a, b, c in faces.tolist():
        ref[[a, b, c]] = True
        for u, v in ((a, b), (a, c)):
            ru, rv = find(u), find(v)
            if ru != rv:
                parent[max(ru, rv)] = min(ru, rv)          # the root is the set's lowest member
    roots = [v for v in range(n_vertices) if ref[v] and find(v) == v]      # ascending
    cid = {r: k for k, r in enumerate(roots)}
    comp = np.array([cid[find(f[0])] for f in faces.tolist()], np.int32).reshape(-1)
    return comp, np.bincount(comp, minlength=len(roots)).astype(np.int32)


# ---- the Jacobi ---------------------------------------------------------------------------------------------------------
def sym_jacobi_scalar(A):
    """A: 3 x 3 nested lists of Python floats (symmetric) -> (eigenvalues [A00, A11, A22], V as nested lists, column i the vector
    of eigenvalue i).  Cyclic, pairs (0,1) (0,2) (1,2), at most 30 sweeps, every operation in the library's order"""
    N = 3
    A = [list(map(float, r)) for r in A]
    V = [[1.0 if r == c else 0.0 for c in range(N)] for r in range(N)]
    for _ in range(30):
        rotated = False
        for p in range(N - 1):
            for q in range(p + 1, N):
                apq, app, aqq = A[p][q], A[p][p], A[q][q]
                if apq == 0.0 or abs(apq) <= 1e-16 * math.sqrt(abs(app) * abs(aqq)):
                    continue
                rotated = True
                th = (aqq - app) / (2.0 * apq)
                t = (1.0 if th >= 0.0 else -1.0) / (abs(th) + math.sqrt(1.0 + th * th))
                c = 1.0 / math.sqrt(1.0 + t * t)
                s = t * c
                for k in range(N):
                    akp, akq = A[k][p], A[k][q]
                    A[k][p] = c * akp - s * akq
                    A[k][q] = s * akp + c * akq
                for k in range(N):
                    apk, aqk = A[p][k], A[q][k]
                    A[p][k] = c * apk - s * aqk
                    A[q][k] = s * apk + c * aqk
                A[p][q] = 0.0
                A[q][p] = 0.0
                for k in range(N):
                    vp, vq = V[k][p], V[k][q]
                    V[k][p] = c * vp - s * vq
                    V[k][q] = s * vp + c * vq
        if not rotated:
            break
    return [A[0][0], A[1][1], A[2][2]], V


def sym_jacobi_batch(A):
    """the same routine on n matrices in step: A (n, 3, 3) fp64 -> (eigenvalues (n, 3), V (n, 3, 3)).  A matrix whose pair is
    skipped keeps its entries (np.where), and a sweep in which it rotates nothing changes nothing, so running every matrix until
    none rotates gives each the result of its own early exit"""
    A = np.array(A, np.float64)
    n, N = A.shape[0], 3
    V = np.zeros((n, N, N))
    V[:, range(N), range(N)] = 1.0
    with np.errstate(all="ignore"):
        for _ in range(30):
            any_rot = False
            for p in range(N - 1):
                for q in range(p + 1, N):
                    apq, app, aqq = A[:, p, q].copy(), A[:, p, p].copy(), A[:, q, q].copy()
                    rot = ~((apq == 0.0) | (np.abs(apq) <= 1e-16 * np.sqrt(np.abs(app) * np.abs(aqq))))
                    if not rot.any():
                        continue
                    any_rot = True
                    th = (aqq - app) / (2.0 * apq)
                    t = np.where(th >= 0.0, 1.0, -1.0) / (np.abs(th) + np.sqrt(1.0 + th * th))
                    c = 1.0 / np.sqrt(1.0 + t * t)
                    s = t * c
                    for k in range(N):
                        akp, akq = A[:, k, p].copy(), A[:, k, q].copy()
                        A[:, k, p] = np.where(rot, c * akp - s * akq, akp)
                        A[:, k, q] = np.where(rot, s * akp + c * akq, akq)
                    for k in range(N):
                        apk, aqk = A[:, p, k].copy(), A[:, q, k].copy()
                        A[:, p, k] = np.where(rot, c * apk - s * aqk, apk)
                        A[:, q, k] = np.where(rot, s * apk + c * aqk, aqk)
                    A[:, p, q] = np.where(rot, 0.0, A[:, p, q])
                    A[:, q, p] = np.where(rot, 0.0, A[:, q, p])
                    for k in range(N):
                        vp, vq = V[:, k, p].copy(), V[:, k, q].copy()
                        V[:, k, p] = np.where(rot, c * vp - s * vq, vp)
                        V[:, k, q] = np.where(rot, s * vp + c * vq, vq)
            if not any_rot:
                break
    return A[:, range(N), range(N)].copy(), V


# ---- simplification -----------------------------------------------------------------------------------------------------
def voxel_keys(p, leaf, origin):
    """pn_voxel_downsample's key of fp32 points (n, 3): floor((p - origin) / leaf) per axis in fp32 -> (key int64, k (n, 3))"""
    k = np.floor((np.asarray(p, F32) - np.asarray(origin, F32)) / np.asarray(leaf, F32))
    assert k.dtype == F32 and ((k >= 0) & (k < MAX_CLUSTERS)).all(), "a key outside [0, 2^21)"
    k = k.astype(np.int64)
    return (k[:, 2] << (2 * AXIS_BITS)) | (k[:, 1] << AXIS_BITS) | k[:, 0], k


def place_scalar(P, corner_list, placement, rank_tol, leaf):
    """the position of ONE cluster in Python floats: P (3F, 3) fp64, the widened corner positions; corner_list ascending ->
    (x as three fp32, m as three fp64, info: dict(rank=, fallback=))"""
    s = [0.0, 0.0, 0.0]
    for c in corner_list:
        for k in range(3):
            s[k] = s[k] + float(P[c, k])
    cnt = float(len(corner_list))
    m = [s[0] / cnt, s[1] / cnt, s[2] / cnt]
    info = dict(rank=0, fallback=False)
    if placement != "quadric":
        return np.array(m).astype(F32), m, info
    A = [[0.0] * 3 for _ in range(3)]
    r = [0.0, 0.0, 0.0]
    for c in corner_list:
        f3 = 3 * (c // 3)
        a = [float(P[f3, k]) - m[k] for k in range(3)]
        b = [float(P[f3 + 1, k]) - m[k] for k in range(3)]
        cc = [float(P[f3 + 2, k]) - m[k] for k in range(3)]
        e1 = [b[k] - a[k] for k in range(3)]
        e2 = [cc[k] - a[k] for k in range(3)]
        n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
        d = (n[0] * a[0] + n[1] * a[1]) + n[2] * a[2]
        for p in range(3):
            for q in range(p, 3):
                A[p][q] = A[p][q] + n[p] * n[q]
            r[p] = r[p] + n[p] * d
    A[1][0], A[2][0], A[2][1] = A[0][1], A[0][2], A[1][2]
    lam, Vv = sym_jacobi_scalar(A)
    lmax = lam[0]
    if lam[1] > lmax:
        lmax = lam[1]
    if lam[2] > lmax:
        lmax = lam[2]
    info["fallback"] = True
    if not (lmax > 0.0 and math.isfinite(lmax)):
        return np.array(m).astype(F32), m, info
    cut = rank_tol * lmax
    acc = [0.0, 0.0, 0.0]
    for i in range(3):
        if lam[i] > cut:
            info["rank"] += 1
            dot = (Vv[0][i] * r[0] + Vv[1][i] * r[1]) + Vv[2][i] * r[2]
            coef = dot / lam[i]
            for k in range(3):
                acc[k] = acc[k] + Vv[k][i] * coef
    x = [m[k] + acc[k] for k in range(3)]
    if not all(math.isfinite(v) for v in x) or any(abs(x[k] - m[k]) > float(F32(leaf[k])) for k in range(3)):
        return np.array(m).astype(F32), m, info
    info["fallback"] = False
    with np.errstate(over="ignore"):
        return np.array(x).astype(F32), m, info


def place_batch(P, order, start, length, sel, placement, rank_tol, leaf):
    """the positions of the clusters ``sel`` in step -> (x (n, 3) fp32, m (n, 3) fp64, rank (n,), fallback (n,) bool)"""
    st, ln = start[sel], length[sel]
    n = len(sel)
    s = np.zeros((n, 3))
    for j in range(int(ln.max()) if n else 0):
        on = np.flatnonzero(ln > j)
        s[on] = s[on] + P[order[st[on] + j]]
    m = s / ln.astype(np.float64)[:, None]
    rank, fb = np.zeros(n, np.int64), np.zeros(n, bool)
    if placement != "quadric" or n == 0:
        return m.astype(F32), m, rank, fb
    A, r = np.zeros((n, 3, 3)), np.zeros((n, 3))
    with np.errstate(all="ignore"):
        for j in range(int(ln.max())):
            on = np.flatnonzero(ln > j)
            f3 = 3 * (order[st[on] + j] // 3)
            a, b, c = P[f3] - m[on], P[f3 + 1] - m[on], P[f3 + 2] - m[on]
            e1, e2 = b - a, c - a
            nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
            ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
            nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
            nn = (nx, ny, nz)
            d = (nx * a[:, 0] + ny * a[:, 1]) + nz * a[:, 2]
            for p in range(3):
                for q in range(p, 3):
                    A[on, p, q] = A[on, p, q] + nn[p] * nn[q]
                r[on, p] = r[on, p] + nn[p] * d
        A[:, 1, 0], A[:, 2, 0], A[:, 2, 1] = A[:, 0, 1], A[:, 0, 2], A[:, 1, 2]
        lam, Vv = sym_jacobi_batch(A)
        lmax = lam[:, 0].copy()
        lmax = np.where(lam[:, 1] > lmax, lam[:, 1], lmax)
        lmax = np.where(lam[:, 2] > lmax, lam[:, 2], lmax)
        good = (lmax > 0.0) & np.isfinite(lmax)
        cut = rank_tol * lmax
        acc = np.zeros((n, 3))
        for i in range(3):
            take = good & (lam[:, i] > cut)
            rank += take
            dot = (Vv[:, 0, i] * r[:, 0] + Vv[:, 1, i] * r[:, 1]) + Vv[:, 2, i] * r[:, 2]
            coef = dot / lam[:, i]
            for k in range(3):
                acc[:, k] = np.where(take, acc[:, k] + Vv[:, k, i] * coef, acc[:, k])
        x = m + acc
        lf = np.asarray(leaf, F32).astype(np.float64)
        ok = good & np.isfinite(x).all(1) & ~(np.abs(x - m) > lf).any(1)
        rank = np.where(good, rank, 0)
        return np.where(ok[:, None], x, m).astype(F32), m, rank, ~ok


def simplify(vertices, faces, leaf, origin, labels=None, placement="quadric", rank_tol=1e-3):
    """-> dict(vertices (V', 3) fp32, faces (F', 3) int32, labels (F',) int32 or None, kept (F',) the input faces that stay,
    clusters (V',) the ranks of the returned clusters among all, m (V', 3) fp64, rank, fallback (V',), n_clusters,
    max_corners: the longest corner list)"""
    vertices = np.asarray(vertices, F32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    Fc = faces.shape[0]
    assert Fc > 0 and faces.min() >= 0 and faces.max() < len(vertices) and np.isfinite(vertices[faces]).all()
    corner = faces.reshape(-1)
    ck, _ = voxel_keys(vertices[corner], leaf, origin)
    order = np.argsort(ck, kind="stable")                          # by (key, c)
    sk = ck[order]
    head = np.r_[True, sk[1:] != sk[:-1]]
    start = np.flatnonzero(head)
    length = np.diff(np.r_[start, 3 * Fc])
    assert len(start) <= MAX_CLUSTERS
    crank = np.empty(3 * Fc, np.int64)
    crank[order] = np.cumsum(head) - 1
    fr = crank.reshape(Fc, 3)
    live = (fr[:, 0] != fr[:, 1]) & (fr[:, 1] != fr[:, 2]) & (fr[:, 0] != fr[:, 2])
    first = np.argmin(fr, 1)                                       # the rotation that puts the lowest rank first keeps the cyclic order
    rows = np.arange(Fc)
    a, b, c = fr[rows, first], fr[rows, (first + 1) % 3], fr[rows, (first + 2) % 3]
    key = (a << (2 * AXIS_BITS)) | (b << AXIS_BITS) | c
    cand = np.flatnonzero(live)
    _, idx = np.unique(key[cand], return_index=True)               # the first occurrence: the earliest face
    kept = np.sort(cand[idx])
    used = np.zeros(len(start), bool)
    used[fr[kept].reshape(-1)] = True
    sel = np.flatnonzero(used)
    vrank = np.cumsum(used) - 1
    P = vertices[corner].astype(np.float64)
    x, m, rank, fb = place_batch(P, order, start, length, sel, placement, rank_tol, leaf)
    return dict(vertices=x.reshape(-1, 3), faces=vrank[fr[kept]].astype(np.int32).reshape(-1, 3),
                labels=None if labels is None else np.asarray(labels, np.int32)[kept], kept=kept, clusters=sel, m=m.reshape(-1, 3), rank=rank,
                fallback=fb, n_clusters=len(start), max_corners=int(length.max()), corner_lists=(order, start, length), P=P)


# ---- meshes -------------------------------------------------------------------------------------------------------------
def grid_mesh(nx, ny=None, spacing=1.0, z=0.0):
    """a flat nx x ny vertex grid in the plane z, two triangles per square, normals +z -> (vertices fp32, faces int32)"""
    ny = nx if ny is None else ny
    gx, gy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    v = np.stack((gx.ravel() * spacing, gy.ravel() * spacing, np.full(nx * ny, z)), 1).astype(F32)
    i = (gy[:-1, :-1] * nx + gx[:-1, :-1]).ravel()
    f = np.concatenate((np.stack((i, i + 1, i + nx + 1), 1), np.stack((i, i + nx + 1, i + nx), 1)))
    return v, f.astype(np.int32)


def cube_mesh(n, side=1.0, offset=(0.0, 0.0, 0.0)):
    """the surface of a cube, n squares per edge, shared vertices, outward normals"""
    verts, index, faces = [], {}, []

    def vid(p):
        if p not in index:
            index[p] = len(verts)
            verts.append(p)
        return index[p]

    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for side_k in (0, n):
            for i in range(n):
                for j in range(n):
                    def pt(di, dj):
                        p = [0, 0, 0]
                        p[axis], p[u], p[w] = side_k, i + di, j + dj
                        return tuple(p)
                    q = [vid(pt(0, 0)), vid(pt(1, 0)), vid(pt(1, 1)), vid(pt(0, 1))]       # counter-clockwise seen along +axis
                    if side_k == 0:
                        q = q[::-1]
                    faces += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    v = (np.array(verts, np.float64) * (side / n) + np.asarray(offset, np.float64)).astype(F32)
    return v, np.array(faces, np.int32)


def sphere_mesh(n_lat, n_lon, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """a latitude / longitude sphere with pole fans, outward normals"""
    v = [(0.0, 0.0, 1.0)]
    for i in range(1, n_lat):
        th = math.pi * i / n_lat
        v += [(math.sin(th) * math.cos(2 * math.pi * j / n_lon), math.sin(th) * math.sin(2 * math.pi * j / n_lon), math.cos(th)) for j in range(n_lon)]
    v.append((0.0, 0.0, -1.0))
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon                # noqa: E731
    f = [(0, ring(1, j), ring(1, j + 1)) for j in range(n_lon)]
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            f += [(ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)), (ring(i, j), ring(i + 1, j + 1), ring(i, j + 1))]
    last = len(v) - 1
    f += [(last, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)) for j in range(n_lon)]
    return (np.array(v) * radius + np.asarray(centre)).astype(F32), np.array(f, np.int32)


def strip_mesh(n_faces, spacing=0.25):
    """one long triangle strip: n_faces + 2 vertices, face i = (i, i+1, i+2) with alternating order: one component whose
    union-find chain is as long as the mesh"""
    i = np.arange(n_faces + 2)
    v = np.stack((0.5 * spacing * i, spacing * (i % 2), np.zeros(len(i))), 1).astype(F32)
    k = np.arange(n_faces)
    f = np.stack((k, np.where(k % 2 == 0, k + 1, k + 2), np.where(k % 2 == 0, k + 2, k + 1)), 1)
    return v, f.astype(np.int32)


def interleave(meshes):
    """several meshes as ONE indexed mesh whose vertex rows and face rows alternate between them (mesh a's vertex i becomes row
    a + i * len(meshes) while rows last, the leftovers follow): components that are not contiguous in either table ->
    (vertices, faces, the source mesh of every face)"""
    k = len(meshes)
    nv = [len(m[0]) for m in meshes]
    slots = sorted((i, a) for a in range(k) for i in range(nv[a]))           # (row within the mesh, the mesh): round robin
    new = {(a, i): row for row, (i, a) in enumerate(slots)}
    v = np.zeros((len(slots), 3), F32)
    for (a, i), row in new.items():
        v[row] = meshes[a][0][i]
    fslots = sorted((i, a) for a in range(k) for i in range(len(meshes[a][1])))
    f = np.array([[new[(a, int(j))] for j in meshes[a][1][i]] for i, a in fslots], np.int32)
    return v, f, np.array([a for _, a in fslots], np.int32)


def spike_mesh(n, seed=0):
    """n faces whose first corners all lie in the voxel [0, 1)^3 (one cluster of exactly n corners, at leaf 1 and origin
    (0, -2, 0)) and whose other corners lie one per voxel along two rows: every face stays"""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    a = rng.uniform(0.2, 0.8, (n, 3))
    b = np.stack((2.0 + k + rng.uniform(0.1, 0.9, n), rng.uniform(0.1, 0.9, n), rng.uniform(0.1, 0.9, n)), 1)
    c = np.stack((2.0 + k + rng.uniform(0.1, 0.9, n), 2.0 + rng.uniform(0.1, 0.9, n), rng.uniform(0.1, 0.9, n)), 1)
    v = np.concatenate((a, b, c)).astype(F32)
    return v, np.stack((k, n + k, 2 * n + k), 1).astype(np.int32)


def soup_mesh(n_vertices, n_faces, seed=0, extent=8.0):
    """random positions and random index triples: faces with repeated indices, repeated faces, long and short corner lists"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.0, extent, (n_vertices, 3)).astype(F32)
    f = rng.integers(0, n_vertices, (n_faces, 3)).astype(np.int32)
    return v, f
