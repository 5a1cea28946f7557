"""NumPy specification of semantic ICP against a labelled triangle mesh (include/pointnet_hip.h, pn_icp_mesh_correspond and
pn_semantic_icp_mesh): the fp32 closest point on a triangle by region classification, operation for operation in np.float32; the
grouping of a mesh; the label-constrained search with its tie rule; both kinds of sums, the solves and the loop on top of
tests/icp_oracle.py and tests/icp_plane_oracle.py.  Also a procedural labelled aircraft mesh with a 1-to-4 subdivision, an
area-weighted surface sampler and an OBJ writer.  Test infrastructure only; nothing in the package imports it."""
import numpy as np

import icp_oracle as IO
import icp_plane_oracle as PO

F32 = np.float32
CONVERGED, FEW_PAIRS, DEGENERATE = 1, 2, 4


# ---------------------------------------------------------------------------------------------------------------------
# the closest point
# ---------------------------------------------------------------------------------------------------------------------
def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def closest(u, a, b, c):
    """closest point of u on triangle (a, b, c): all (..., 3) float32, broadcast against each other -> (q (..., 3) f32,
    d2 (...) f32).  Every line is one rounded fp32 operation per element, in the header's operand order."""
    u, a, b, c = (np.asarray(x, F32) for x in (u, a, b, c))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ab, ac = b - a, c - a
        ap, bp, cp = u - a, u - b, u - c
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        rA = (d1 <= 0) & (d2 <= 0)
        rB = (d3 >= 0) & (d4 <= d3)
        rC = (d6 >= 0) & (d5 <= d6)
        rAB = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        rAC = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        rBC = (va <= 0) & (e43 >= 0) & (e56 >= 0)
        one = np.ones_like(d1)
        num = np.where(rAB, d1, np.where(rAC, d2, np.where(rBC, e43, one)))
        den = np.where(rAB, d1 - d3, np.where(rAC, d2 - d6, np.where(rBC, e43 + e56, (va + vb) + vc)))
        t = (num / den).astype(F32)
        t3 = t[..., None]
        qAB = a + t3 * ab
        qAC = a + t3 * ac
        qBC = b + t3 * (c - b)
        v, w = (vb * t)[..., None], (vc * t)[..., None]
        qF = (a + ab * v) + ac * w
        sel = lambda m, x, y: np.where(m[..., None], x, y)                     # noqa: E731
        q = sel(rA, a, sel(rB, b, sel(rC, c, sel(rAB, qAB, sel(rAC, qAC, sel(rBC, qBC, qF))))))
        q = np.broadcast_to(q, np.broadcast(q, u).shape).astype(F32)
        e = u - q
        dist = _dot(e, e)
    return q, dist.astype(F32)


def closest_fp64(u, a, b, c):
    """an independent check in fp64 (one point, one triangle): the nearest of the three clamped edge projections and, when it falls
    inside the triangle, the projection onto its plane -> (q, d2)"""
    u, a, b, c = (np.asarray(x, np.float64) for x in (u, a, b, c))
    cands = []
    for p0, p1 in ((a, b), (b, c), (c, a)):
        e = p1 - p0
        t = np.clip(np.dot(u - p0, e) / np.dot(e, e), 0.0, 1.0)
        cands.append(p0 + t * e)
    n = np.cross(b - a, c - a)
    proj = u - n * (np.dot(u - a, n) / np.dot(n, n))
    inside = all(np.dot(np.cross(p1 - p0, proj - p0), n) >= 0 for p0, p1 in ((a, b), (b, c), (c, a)))
    if inside:
        cands.append(proj)
    d = [np.dot(u - q, u - q) for q in cands]
    k = int(np.argmin(d))
    return cands[k], d[k]


# ---------------------------------------------------------------------------------------------------------------------
# grouping, search, sums, loop
# ---------------------------------------------------------------------------------------------------------------------
def group_mesh(vertices, faces, labels, n_parts):
    """-> (tri (T, 3, 3) f32 grouped by label in a stable order, seg (n_parts + 1,), index (T,) into ``faces``, normals (T, 3) f32,
    area (T,) f64); triangles with a label outside [0, n_parts), a non-finite vertex or zero fp64 area are dropped"""
    v = np.asarray(vertices, F32).reshape(-1, 3)
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    tri = v[f]
    t64 = tri.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        cr = np.cross(t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 0])
        nn = np.linalg.norm(cr, axis=1)
    ok = np.isfinite(tri).all((1, 2)) & np.isfinite(nn) & (nn > 0) & (lab >= 0) & (lab < n_parts)
    keep = np.flatnonzero(ok)
    order = keep[np.argsort(lab[keep], kind="stable")]
    seg = np.searchsorted(lab[order], np.arange(n_parts + 1)).astype(np.int64)
    return tri[order], seg, order, (cr[order] / nn[order, None]).astype(F32), 0.5 * nn[order]


def correspond(scan, labels, tri, seg, n_parts, pose32, max_d2=np.inf, chunk=512):
    """-> idx (B, N) int32 (the winner's grouped triangle or -1), d2 (B, N) f32 (+inf when none), q (B, N, 3) f32 (NaN when none)"""
    scan = np.asarray(scan, F32)
    tri = np.asarray(tri, F32)
    B, N, _ = scan.shape
    idx = np.full((B, N), -1, np.int32)
    d2 = np.full((B, N), np.inf, F32)
    q = np.full((B, N, 3), np.nan, F32)
    act = IO.active(scan, labels, seg, n_parts)
    md = F32(max_d2)
    for b in range(B):
        u = IO.to_model_frame(scan[b], np.asarray(pose32[b], F32))
        for lab in range(n_parts):
            rows = np.flatnonzero(act[b] & (labels[b] == lab))
            if rows.size == 0:
                continue
            t = tri[seg[lab]:seg[lab + 1]]
            for c0 in range(0, rows.size, chunk):
                rr = rows[c0:c0 + chunk]
                qq, dist = closest(u[rr, None, :], t[None, :, 0], t[None, :, 1], t[None, :, 2])
                key = dist.view(np.uint32)
                j = np.argmin(key, axis=1)                       # first minimum: ties -> lowest index
                ar = np.arange(rr.size)
                kmin = key[ar, j]
                found = kmin < IO.EMPTY
                dd = np.where(found, kmin.view(F32), F32(np.inf)).astype(F32)
                d2[b, rr] = dd
                idx[b, rr] = np.where(found & (dd <= md), j + seg[lab], -1)
                q[b, rr] = np.where(found[:, None], qq[ar, j], F32(np.nan))
    return idx, d2, q


def _self_idx(idx_b):
    return np.where(idx_b >= 0, np.arange(idx_b.shape[0]), -1).astype(np.int32)[None]


def sums_point(scan, idx, q):
    """(B, 18): icp_oracle.sums with each kept point's partner its own closest point"""
    return np.stack([IO.sums(scan[b:b + 1], _self_idx(idx[b]), q[b])[0] for b in range(scan.shape[0])])


def sums_plane(scan, idx, q, normals, pose64):
    """(B, 29): icp_plane_oracle.sums with each kept point's partner its own closest point and its winner's face normal"""
    out = []
    for b in range(scan.shape[0]):
        nrm = np.asarray(normals, F32)[np.maximum(idx[b], 0)]
        out.append(PO.sums(scan[b:b + 1], _self_idx(idx[b]), q[b], nrm, np.asarray(pose64[b:b + 1], np.float64))[0])
    return np.stack(out)


def pass_sums(scan, labels, tri, seg, n_parts, normals, pose64, metric, max_d2=np.inf):
    """one pass at the fp32 rounding of pose64 -> (idx, d2, q, sums)"""
    pose64 = np.asarray(pose64, np.float64)
    idx, d2, q = correspond(scan, labels, tri, seg, n_parts, pose64.astype(F32), max_d2)
    S = sums_plane(scan, idx, q, normals, pose64) if metric == "plane" else sums_point(scan, idx, q)
    return idx, d2, q, S


def icp(scan, labels, tri, seg, n_parts, normals, init_pose, metric="point", max_iters=30, max_d2=np.inf, tol_rot=1e-6,
        tol_t=1e-6):
    """the whole loop -> (pose (B,4,4), rmse (B,), pairs (B,), iters (B,), status (B,))"""
    scan = np.asarray(scan, F32)
    B = scan.shape[0]
    pose = np.array(init_pose, np.float64).reshape(B, 4, 4).copy()
    pose[:, 3] = [0, 0, 0, 1]
    rmse = np.full(B, np.nan)
    pairs = np.zeros(B, np.int32)
    iters = np.zeros(B, np.int32)
    status = np.zeros(B, np.int32)
    solve = PO.solve if metric == "plane" else IO.solve
    for b in range(B):
        for _ in range(max_iters):
            _, _, _, S = pass_sums(scan[b:b + 1], labels[b:b + 1], tri, seg, n_parts, normals, pose[b:b + 1], metric, max_d2)
            new, rm, st = solve(S[0], pose[b])
            iters[b] += 1
            rmse[b], pairs[b] = rm, int(S[0, 0])
            few = st & FEW_PAIRS
            conv = bool(few) or (IO.rotation_angle(new[:3, :3], pose[b, :3, :3]) < tol_rot
                                 and np.linalg.norm(new[:3, 3] - pose[b, :3, 3]) < tol_t)
            pose[b] = new
            status[b] = st | (CONVERGED if conv else 0)
            if conv:
                break
    return pose, rmse, pairs, iters, status


# ---------------------------------------------------------------------------------------------------------------------
# the procedural labelled aircraft mesh
# ---------------------------------------------------------------------------------------------------------------------
MESH_PARTS = ("fuselage", "wing", "vstab", "hstab")


def _box(origin, e1, e2, e3):
    """the 12 triangles of the parallelepiped origin + [0,1] e1 + [0,1] e2 + [0,1] e3"""
    o, e1, e2, e3 = (np.asarray(x, np.float64) for x in (origin, e1, e2, e3))
    out = []
    for base, p, r in ((o, e1, e2), (o + e3, e1, e2), (o, e2, e3), (o + e1, e2, e3), (o, e3, e1), (o + e2, e3, e1)):
        out += [[base, base + p, base + p + r], [base, base + p + r, base + r]]
    return np.array(out)


def _prism(x0, x1, radius, sides):
    """a capped prism along x: 2 * sides wall triangles and 2 * (sides - 2) cap triangles"""
    ang = 2 * np.pi * (np.arange(sides) + 0.5) / sides
    ring = np.stack([np.zeros(sides), radius * np.cos(ang), radius * np.sin(ang)], 1)
    lo, hi = ring + [x0, 0, 0], ring + [x1, 0, 0]
    out = []
    for k in range(sides):
        n = (k + 1) % sides
        out += [[lo[k], hi[k], hi[n]], [lo[k], hi[n], lo[n]]]
    for cap in (lo, hi):
        out += [[cap[0], cap[k], cap[k + 1]] for k in range(1, sides - 1)]
    return np.array(out)


def aircraft_mesh(levels=0):
    """-> (vertices (3T, 3) f32, faces (T, 3) int32, part (T,) int32): a 12-sided capped prism fuselage and three slanted boxes
    (wing, fin, tailplane), 80 triangles at level 0, four times as many per level.  A triangle soup: a shared corner is repeated
    with the same coordinates, so shared edges and vertices coincide bit for bit."""
    pieces = [(0, _prism(-18.0, 20.0, 2.0, 12)),
              (1, _box([-3.0, -17.0, -0.9], [6.0, 0.0, 0.2], [1.0, 34.0, 0.0], [0.0, 0.3, 0.5])),
              (2, _box([-18.0, -0.2, 1.8], [5.0, 0.0, 0.0], [-2.5, 0.1, 7.0], [0.0, 0.4, 0.0])),
              (3, _box([-18.5, -6.5, 0.6], [4.0, 0.2, 0.0], [0.5, 13.0, 0.3], [0.0, 0.0, 0.3]))]
    tri = np.concatenate([t for _, t in pieces])
    part = np.concatenate([np.full(len(t), p, np.int32) for p, t in pieces])
    tri, part = subdivide(tri.astype(F32), part, levels)
    T = len(tri)
    return tri.reshape(-1, 3), np.arange(3 * T, dtype=np.int32).reshape(T, 3), part


def subdivide(tri, part, levels=1):
    """every triangle into four through its fp32 edge midpoints, ``levels`` times -> (tri (4^levels T, 3, 3) f32, part)"""
    tri = np.asarray(tri, F32)
    part = np.asarray(part, np.int32)
    half = F32(0.5)
    for _ in range(levels):
        a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
        ab, bc, ca = (a + b) * half, (b + c) * half, (c + a) * half          # a + b == b + a: a shared edge gets one midpoint
        tri = np.stack([np.stack([a, ab, ca], 1), np.stack([ab, b, bc], 1), np.stack([ca, bc, c], 1), np.stack([ab, bc, ca], 1)],
                       1).reshape(-1, 3, 3)
        part = np.repeat(part, 4)
    return tri, part


def sample_surface(vertices, faces, part, n, seed=0):
    """n area-weighted uniform surface samples -> (xyz (n, 3) f64, part (n,) int32, face (n,))"""
    rng = np.random.default_rng(seed)
    t = np.asarray(vertices, np.float64)[np.asarray(faces)]
    area = 0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)
    f = rng.choice(len(t), n, p=area / area.sum())
    r1, r2 = np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 1, n)
    xyz = (1 - r1)[:, None] * t[f, 0] + (r1 * (1 - r2))[:, None] * t[f, 1] + (r1 * r2)[:, None] * t[f, 2]
    return xyz, np.asarray(part, np.int32)[f], f


def mesh_scan(vertices, faces, part, n, pose=PO.TRUE_POSE, noise=0.0, seed=1):
    """a labelled scan of the mesh under ``pose``: n surface samples with N(0, noise) noise -> (xyz (n, 3) f32, part (n,) int32)"""
    q, lab, _ = sample_surface(vertices, faces, part, n, seed)
    rng = np.random.default_rng(seed + 1000)
    p = q @ np.asarray(pose)[:3, :3].T + np.asarray(pose)[:3, 3] + rng.normal(0, noise, size=q.shape)
    return p.astype(F32), lab


def write_obj(path, vertices, faces, part, names, style="i", use="o", header=()):
    """a Wavefront OBJ with one named sub-mesh per run of equal part ids; ``style`` picks the corner form (i, i/t, i//n, i/t/n),
    ``use`` the naming statement (o or g)"""
    form = {"i": "{0}", "i/t": "{0}/1", "i//n": "{0}//1", "i/t/n": "{0}/1/1"}[style]
    with open(path, "w") as f:
        for h in header:
            f.write(h + "\n")
        f.write("vt 0.0 0.0\nvn 0.0 0.0 1.0\n")
        for v in np.asarray(vertices):
            f.write(f"v {float(v[0])!r} {float(v[1])!r} {float(v[2])!r}\n")
        last = None
        for tri, p in zip(np.asarray(faces), np.asarray(part)):
            if p != last:
                f.write(f"{use} {names[int(p)]}\n")
                last = p
            f.write("f " + " ".join(form.format(int(i) + 1) for i in tri) + "\n")
