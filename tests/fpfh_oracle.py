"""NumPy statements of pn_fpfh's, pn_feature_match's and pn_ransac_poses' specifications (include/pointnet_hip.h) -- TEST
INFRASTRUCTURE.  Nothing in the package imports it.

fpfh            the lists are neighbors_oracle.radius_knn's; the pair feature, the sector rule, the bins, S, A, T and the final sum in
                float64, every operation in the header's order (NumPy does not contract)
feature_match   d2 summed over the 33 bins in order in float32; the winner is the lowest (bit pattern of d2, row)
ransac          draws = Philox4x32-10 with the domain word "RANS"; the validity tests in float32; the fit through icp_oracle.solve
                (np.linalg.svd) on the 18 sums; counts at a given float32 pose in the header's operation order
"""
from __future__ import annotations

import math

import numpy as np

import icp_oracle as IO
import neighbors_oracle as NO
from mesh_sample_oracle import philox4x32

F32 = np.float32
F64 = np.float64
BINS, DIV = 33, 11
DOMAIN = 0x52414E53
MAX_H = 65536
BETA = [-math.pi + 2.0 * math.pi * m / 11.0 for m in range(1, 11)]
COS = np.array([math.cos(b) for b in BETA])
SIN = np.array([math.sin(b) for b in BETA])


# ---- pn_fpfh ---------------------------------------------------------------------------------------------------------
def sector(x, y):
    """the angle bin of (x, y) (arrays, float64): the number of m that pass the header's test"""
    x, y = np.asarray(x, F64), np.asarray(y, F64)
    b = np.zeros(x.shape, np.int64)
    for m in range(10):
        side = COS[m] * y - SIN[m] * x >= 0.0
        b += ((y >= 0.0) | side) if m < 5 else ((y >= 0.0) & side)
    return b


def bin11(t):
    f = np.nan_to_num(np.floor((11.0 * (np.asarray(t, F64) + 1.0)) * 0.5))      # (a NaN belongs to a skipped pair)
    return np.clip(f, 0, 10).astype(np.int64)


def pair_features(pi, ni, pj, nj):
    """(..., 3) float32 inputs -> (x, y, alpha, phi, ok) float64 arrays: the header's pair feature; ok is False where the pair is
    skipped for a non-finite normal or l = 0 (d = 0 is the caller's test, on the float32 distance)"""
    pi, ni, pj, nj = (np.asarray(a, F32).astype(F64) for a in (pi, ni, pj, nj))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        e = pj - pi
        dist = np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])
        dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]      # noqa: E731
        a1, a2 = dot(ni, e) / dist, dot(nj, e) / dist
        sw = np.abs(a1) < np.abs(a2)
        n1 = np.where(sw[..., None], nj, ni)
        n2 = np.where(sw[..., None], ni, nj)
        e = np.where(sw[..., None], -e, e)
        phi = np.where(sw, -a2, a1)
        cross = lambda a, b: np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],      # noqa: E731
                                       a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)
        v = cross(e, n1)
        l = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
        v = v / l[..., None]
        w = cross(n1, v)
        alpha = dot(v, n2)
        x, y = dot(n1, n2), dot(w, n2)
        ok = np.isfinite(ni).all(-1) & np.isfinite(nj).all(-1) & (l > 0.0)
    return x, y, alpha, phi, ok


def spfh(xyz, normals, idx, d2):
    """-> (counts (N, 33) int32, pairs (N,) int32) from the lists (idx, d2) of radius_knn"""
    xyz, normals = np.asarray(xyz, F32), np.asarray(normals, F32)
    N, k = idx.shape
    counts = np.zeros((N, BINS), np.int32)
    pairs = np.zeros(N, np.int32)
    if k == 0 or N == 0:
        return counts, pairs
    j = np.clip(idx, 0, None)
    x, y, alpha, phi, ok = pair_features(xyz[:, None, :], normals[:, None, :], xyz[j], normals[j])
    ok &= (idx >= 0) & (d2 != 0)
    rows = np.broadcast_to(np.arange(N)[:, None], idx.shape)[ok]
    for off, b in ((0, sector(x, y)), (DIV, bin11(alpha)), (2 * DIV, bin11(phi))):
        np.add.at(counts, (rows, off + b[ok]), 1)
    pairs[:] = ok.sum(1)
    return counts, pairs


def fpfh(xyz, normals, radius, k=16, return_spfh=False):
    """pn_fpfh / ops.fpfh -> fpfh (N, 33) float32 (and counts, pairs)"""
    xyz = np.ascontiguousarray(xyz, F32)
    idx, d2, _ = NO.radius_knn(xyz, radius, k)
    counts, pairs = spfh(xyz, normals, idx, d2)
    N = len(xyz)
    with np.errstate(invalid="ignore", divide="ignore"):
        S = np.where(pairs[:, None] > 0, (100.0 * counts.astype(F64)) / pairs[:, None].astype(F64), 0.0)
        A = np.zeros((N, BINS))
        for s in range(idx.shape[1]):
            use = (idx[:, s] >= 0) & (d2[:, s] > 0)
            j = np.clip(idx[:, s], 0, None)
            A = np.where(use[:, None], A + S[j] / d2[:, s].astype(F64)[:, None], A)
        out = np.zeros((N, BINS))
        for g in range(3):
            T = np.zeros(N)
            for b in range(DIV):
                T = T + A[:, g * DIV + b]
            sc = np.where(T != 0.0, 100.0 / np.where(T != 0.0, T, 1.0), 0.0)
            for b in range(DIV):
                c = g * DIV + b
                out[:, c] = S[:, c] + np.where(T != 0.0, A[:, c] * sc, 0.0)
    out = out.astype(F32)
    return (out, counts, pairs) if return_spfh else out


# ---- pn_feature_match ------------------------------------------------------------------------------------------------
def feature_match(a, b, mutual=False, chunk=256):
    """-> (idx (Na,) int32, d2 (Na,) float32)"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    Na, Nb = len(a), len(b)
    idx = np.full(Na, -1, np.int32)
    d2 = np.full(Na, np.inf, F32)
    okb = np.isfinite(b).all(1)
    oka = np.isfinite(a).all(1)
    cols = np.arange(Nb, dtype=np.uint64)
    empty = np.uint64(0xFFFFFFFFFFFFFFFF)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, Na, chunk):
            e = min(s + chunk, Na)
            d = np.zeros((e - s, Nb), F32)
            for c in range(a.shape[1]):
                t = a[s:e, None, c] - b[None, :, c]
                d = d + t * t
            key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | cols[None, :]
            key[:, ~okb] = empty
            key[~oka[s:e]] = empty
            best = key.min(1)
            found = best != empty
            idx[s:e] = np.where(found, (best & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
            d2[s:e] = np.where(found, (best >> np.uint64(32)).astype(np.uint32).view(F32), F32(np.inf))
    if mutual:
        back, _ = feature_match(b, a)
        keep = (idx >= 0) & (back[np.clip(idx, 0, None)] == np.arange(Na))
        idx = np.where(keep, idx, -1).astype(np.int32)
    return idx, d2


# ---- pn_ransac_poses -------------------------------------------------------------------------------------------------
def draws(C, H, seed=0):
    """(H, 3) int64: the rows of every hypothesis, a pure function of (seed, h, C)"""
    counter = np.zeros((H, 4), np.uint64)
    counter[:, 0] = np.arange(H)
    counter[:, 3] = DOMAIN
    x = philox4x32(counter, (int(seed) & 0xFFFFFFFF, int(seed) >> 32)).astype(np.uint64)
    return ((x[:, :3] * np.uint64(C)) >> np.uint64(32)).astype(np.int64)


def _len2(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _area2(p):
    a, b = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], -1)
    return (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]


def edges_ok(la2, lb2, e2):
    """the inclusive edge-length test on float32 squared lengths"""
    la2, lb2, e2 = F32(la2), F32(lb2), F32(e2)
    return (la2 >= e2 * lb2) & (lb2 >= e2 * la2)


def valid(src, tgt, rows, edge_ratio):
    """(H,) bool: every test of the header but the fit's own"""
    src, tgt = np.asarray(src, F32), np.asarray(tgt, F32)
    p, q = src[rows], tgt[rows]                                           # (H, 3, 3)
    e2 = F32(edge_ratio) * F32(edge_ratio)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = (rows[:, 0] != rows[:, 1]) & (rows[:, 0] != rows[:, 2]) & (rows[:, 1] != rows[:, 2])
        ok &= np.isfinite(p).all((1, 2)) & np.isfinite(q).all((1, 2))
        for u, v in ((0, 1), (0, 2), (1, 2)):
            la2, lb2 = _len2(p[:, u], p[:, v]), _len2(q[:, u], q[:, v])
            ok &= (la2 >= e2 * lb2) & (lb2 >= e2 * la2)
        ap, aq = _area2(p), _area2(q)
        ok &= np.isfinite(ap) & (ap > 0) & np.isfinite(aq) & (aq > 0)
    return ok


def fit(p, q):
    """the rigid fit p ~ R q + t of three pairs (3, 3) float32 through pn_icp_solve's rule on the 18 sums -> (4, 4) float64"""
    p, q = np.asarray(p, F32).astype(F64), np.asarray(q, F32).astype(F64)
    S = np.zeros(18)
    S[0] = 3.0
    S[1:4] = (p[0] + p[1]) + p[2]
    S[4:7] = (q[0] + q[1]) + q[2]
    for r in range(3):
        for c in range(3):
            S[7 + 3 * r + c] = (q[0, r] * p[0, c] + q[1, r] * p[1, c]) + q[2, r] * p[2, c]
    n2 = lambda a: (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]      # noqa: E731
    S[16] = (n2(p)[0] + n2(p)[1]) + n2(p)[2]
    S[17] = (n2(q)[0] + n2(q)[1]) + n2(q)[2]
    return IO.solve(S, np.eye(4))[0]


def poses(src, tgt, rows, ok):
    """(H, 4, 4) float64, NaN for an invalid hypothesis"""
    out = np.full((len(rows), 4, 4), np.nan)
    for h in np.flatnonzero(ok):
        out[h] = fit(src[rows[h]], tgt[rows[h]])
    return out


def count_inliers(src, tgt, pose32, max_dist, chunk=512):
    """(H,) int32: the pairs within max_dist under the float32 poses (H, 4, 4), in the header's operation order; a NaN pose counts 0"""
    src, tgt, P = np.asarray(src, F32), np.asarray(tgt, F32), np.asarray(pose32, F32)
    md2 = F32(max_dist) * F32(max_dist)
    out = np.zeros(len(P), np.int32)
    qx, qy, qz = tgt[None, :, 0], tgt[None, :, 1], tgt[None, :, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, len(P), chunk):
            M = P[s:s + chunk]
            e = [(((M[:, a, 0, None] * qx + M[:, a, 1, None] * qy) + M[:, a, 2, None] * qz) + M[:, a, 3, None]) - src[None, :, a] for a in range(3)]
            out[s:s + chunk] = (((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) <= md2).sum(1)
    return out


def ransac_poses(src, tgt, max_dist, hypotheses=4096, edge_ratio=0.9, seed=0):
    """the whole entry with the oracle's own fits -> dict(rows, valid, poses, counts, order)"""
    src, tgt = np.ascontiguousarray(src, F32), np.ascontiguousarray(tgt, F32)
    rows = draws(len(src), hypotheses, seed)
    ok = valid(src, tgt, rows, edge_ratio)
    P = poses(src, tgt, rows, ok)
    ok &= np.isfinite(P[:, :3]).all((1, 2))
    P[~ok] = np.nan
    counts = np.where(ok, count_inliers(src, tgt, P.astype(F32), max_dist), -1).astype(np.int32)
    return dict(rows=rows, valid=ok, poses=P, counts=counts, order=rank(counts))


def rank(counts):
    """the hypotheses by (count descending, h ascending)"""
    return np.argsort(-np.asarray(counts, np.int64), kind="stable")


# ---- clouds the CPU and the GPU tests share --------------------------------------------------------------------------
def planes_and_cap(n=700, seed=0):
    """two perpendicular planes and a sphere cap with outward normals -> (xyz (n, 3) f32, normals (n, 3) f32)"""
    rng = np.random.default_rng(seed)
    a = n // 3
    u, v = rng.random((2, a)) * 2.0
    p1, n1 = np.stack([u, v, np.zeros(a)], 1), np.tile([0.0, 0.0, 1.0], (a, 1))
    u, v = rng.random((2, a)) * 2.0
    p2, n2 = np.stack([np.zeros(a), u, v], 1), np.tile([1.0, 0.0, 0.0], (a, 1))
    m = n - 2 * a
    th, ph = rng.random(m) * 0.9, rng.random(m) * 2 * np.pi
    d = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], 1)
    p3 = np.array([1.0, 1.0, 0.0]) + 0.8 * d
    xyz = np.concatenate([p1, p2, p3]) + rng.normal(0, 0.003, (n, 3))
    nrm = np.concatenate([n1, n2, d])
    perm = rng.permutation(n)
    return xyz[perm].astype(F32), nrm[perm].astype(F32)


def flat_lattice(side=6):
    """side^2 lattice points of the plane z = 0 with normals +z"""
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)
    xyz = np.concatenate([g, np.zeros((len(g), 1))], 1).astype(F32)
    return xyz, np.tile(np.array([0, 0, 1], F32), (len(xyz), 1))


def correspondences(C=200, wrong=0.6, seed=0, angle=2.0):
    """C metre-scale pairs p = R q + t (+ a little noise), a share ``wrong`` of them re-paired at random -> (src, tgt, true pose)"""
    rng = np.random.default_rng(seed)
    q = rng.uniform(-2.0, 2.0, (C, 3))
    R = IO.rot(rng.normal(size=3), angle)
    t = rng.uniform(-1.0, 1.0, 3)
    p = q @ R.T + t + rng.normal(0, 0.002, (C, 3))
    bad = rng.permutation(C)[:int(round(wrong * C))]
    p[bad] = rng.uniform(-3.0, 3.0, (len(bad), 3))
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = R, t
    return p.astype(F32), q.astype(F32), P


# ---- the registration fixture and the whole pipeline -------------------------------------------------------------------
def _body_surfaces():
    """(area, sampler(rng, n)) of an asymmetric body about 4 m long, x forward: a box hull, a tilted fin on top, a cylinder along one
    side and a half sphere at the nose"""
    def plate(o, e1, e2):
        o, e1, e2 = (np.asarray(v, F64) for v in (o, e1, e2))
        return float(np.linalg.norm(np.cross(e1, e2))), lambda g, n: o + g.random(n)[:, None] * e1 + g.random(n)[:, None] * e2

    def cylinder(g, n):
        a = g.random(n) * 2 * np.pi
        return np.stack([-1.2 + 2.0 * g.random(n), 0.75 + 0.25 * np.cos(a), -0.1 + 0.25 * np.sin(a)], 1)

    def nose(g, n):
        v = g.normal(size=(n, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        v[:, 0] = np.abs(v[:, 0])
        return v * 0.4 + [1.6, 0.0, 0.0]

    L, W, Hh = 3.2, 1.0, 0.8                                           # the hull: x in [-1.6, 1.6], y in [-0.5, 0.5], z in [-0.4, 0.4]
    out = [plate([-1.6, -0.5, s * 0.4], [L, 0, 0], [0, W, 0]) for s in (-1, 1)]
    out += [plate([-1.6, s * 0.5, -0.4], [L, 0, 0], [0, 0, Hh]) for s in (-1, 1)]
    out += [plate([-1.6, -0.5, -0.4], [0, W, 0], [0, 0, Hh])]
    out += [plate([-1.5, -0.1, 0.4], [0.9, 0.0, 0.0], [-0.5, 0.35, 0.9])]          # the fin, leaning back and to one side
    out += [(2 * np.pi * 0.25 * 2.0, cylinder), (2 * np.pi * 0.4 * 0.4, nose)]
    return out


def body(n, seed):
    """n area-weighted surface samples of the body, thinned from 4 n candidates by greedy farthest-point picking so that the spacing is
    even (what a voxel-downsampled scan looks like) -> (n, 3) float64"""
    rng = np.random.default_rng(seed)
    surf = _body_surfaces()
    area = np.array([a for a, _ in surf])
    cnt = rng.multinomial(4 * n, area / area.sum())
    x = np.concatenate([f(rng, int(c)) for (_, f), c in zip(surf, cnt)])
    pick = np.zeros(n, np.int64)
    d = ((x - x[0]) ** 2).sum(1)
    for i in range(1, n):
        pick[i] = int(np.argmax(d))
        d = np.minimum(d, ((x - x[pick[i]]) ** 2).sum(1))
    return x[pick]


SCENE = dict(n=800, feature_radius=0.6, normals_radius=0.5, max_dist=0.3, k=16, hypotheses=4096, keep=32, top=4, seed=0, mutual=False,
             edge_ratio=0.9, max_iters=30)
SCENE_POSE = np.eye(4)
SCENE_POSE[:3, :3] = IO.rot([0.2, -0.4, 0.9], np.deg2rad(150.0))
SCENE_POSE[:3, 3] = [1.5, -2.0, 0.8]
# How close to the truth the registration must end (rad, m).  The clouds are noise-free samplings about 0.15 m apart and the refinement
# is point to plane, so a converged pose sits well inside a third of the spacing and the angle that spacing subtends over the body's
# 4 m; a wrong basin is tens of degrees away.
BOUND_ROT, BOUND_T = np.deg2rad(1.0), 0.05


def scene():
    """-> dict(target (n, 3) f32, source (m, 3) f32, pose (4, 4): p_source = R q_target + t, target_viewpoint, source_viewpoint): two
    different samplings of the body, the source cut to the front 80 % of its length, turned 150 degrees and shifted; the viewpoints
    are the clouds' own means, so the normals point inwards on both"""
    tgt = body(SCENE["n"], 1)
    src = body(SCENE["n"], 2)
    src = src[src[:, 0] >= -1.6 + 0.2 * 3.6]
    src = src @ SCENE_POSE[:3, :3].T + SCENE_POSE[:3, 3]
    tgt, src = tgt.astype(F32), src.astype(F32)
    return dict(target=tgt, source=src, pose=SCENE_POSE, target_viewpoint=tgt.astype(F64).mean(0).astype(F32),
                source_viewpoint=src.astype(F64).mean(0).astype(F32))


def descriptors(xyz, viewpoint, S=SCENE):
    import normals_oracle as NN
    nrm = NN.normals(xyz, S["normals_radius"], S["k"], viewpoint)[0]
    return fpfh(xyz, nrm, S["feature_radius"], S["k"])


def refine(source, target, seeds, S=SCENE, metric="plane", normals_radius=None):
    """global_pose's tail on given seed poses (K, 4, 4), one part: the coarse score (stride 1 at these sizes), the best ``top``
    refined against the target with ops.register_scans' normals (``normals_radius`` or max_dist, k = 8), scored again -> dict(order, refined, fine, pose, cost, winner: the index among the seeds)"""
    import icp_global_oracle as GO
    import icp_plane_oracle as PO
    import normals_oracle as NN
    src, tgt = np.asarray(source, F32)[None], np.asarray(target, F32)
    lab = np.zeros((1, src.shape[1]), np.int32)
    seg = np.array([0, len(tgt)])
    md = GO.max_d2_of(S["max_dist"])
    _, order = GO.score_poses(src, lab, tgt, seg, 1, np.asarray(seeds)[None], max(1, src.shape[1] // 8192), md)
    top = min(S["top"], len(seeds))
    pick = order[0, :top]
    s, l = np.repeat(src, top, 0), np.repeat(lab, top, 0)
    if metric == "plane":
        nrm = NN.normals(tgt, S["max_dist"] if normals_radius is None else normals_radius, 8, None)[0]
        r = PO.icp(s, l, tgt, seg, 1, nrm, seeds[pick], max_iters=S["max_iters"], max_d2=md)
    else:
        r = IO.icp(s, l, tgt, seg, 1, seeds[pick], max_iters=S["max_iters"], max_d2=md)
    fine = GO.score_poses(src, lab, tgt, seg, 1, r[0][None], 1, md)[0][0, :, 1]
    w = int(np.argmin(fine))
    return dict(order=order[0], refined=r[0], fine=fine, pose=r[0][w], cost=fine[w], winner=int(pick[w]), result=tuple(a[w] for a in r))


def global_register(source, target, source_viewpoint, target_viewpoint, S=SCENE, hypotheses=None):
    """the ops.global_register composition; ``hypotheses`` = (poses (H, 4, 4), counts (H,)) replaces the oracle's own (teacher
    forcing) -> dict(idx, true-free statistics, ransac, kept, and refine()'s entries with winner mapped to the hypothesis h)"""
    source, target = np.asarray(source, F32), np.asarray(target, F32)
    fs, ft = descriptors(source, source_viewpoint, S), descriptors(target, target_viewpoint, S)
    idx, _ = feature_match(fs, ft, S["mutual"])
    sel = np.flatnonzero(idx >= 0)
    if hypotheses is None:
        ra = ransac_poses(source[sel], target[idx[sel]], S["max_dist"], S["hypotheses"], S["edge_ratio"], S["seed"])
        P, counts = ra["poses"], ra["counts"]
    else:
        P, counts = hypotheses
    kept = rank(counts)[:S["keep"]]
    out = refine(source, target, np.asarray(P)[kept], S, normals_radius=S["normals_radius"])
    out.update(idx=idx, sel=sel, poses=P, counts=counts, kept=kept, winner=int(kept[out["winner"]]))
    return out
