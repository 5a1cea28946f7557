"""NumPy specification of point-to-plane semantic ICP (include/pointnet_hip.h, pn_icp_normals, pn_icp_plane_sums,
pn_icp_plane_solve, pn_semantic_icp_plane): per-part PCA normals of the grouped reference, the 29 fp64 sums of the pairs found by
the point-to-point correspondence rule (tests/icp_oracle.py), the minimum-norm solve (np.linalg.eigh with the same cut) and the
loop.  Also the labelled analytic "aircraft" scene the tests and tools/bench_scan.py register against: surfaces sampled, not
reference points copied.  Test infrastructure only; nothing in the package imports it."""
import numpy as np

import icp_oracle as IO

F32 = np.float32
NS = 29
CONVERGED, FEW_PAIRS, DEGENERATE = 1, 2, 4
EIG_CUT = 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# normals
# ---------------------------------------------------------------------------------------------------------------------
def neighbours(ref, seg, n_parts, k):
    """(M, k) int32: the k nearest points of the same label (fp32 distance without contraction, the point included), ordered by
    (distance, grouped index), -1 padded; a NaN distance never enters"""
    ref = np.asarray(ref, F32)
    M = ref.shape[0]
    nbr = np.full((M, k), -1, np.int32)
    for lab in range(n_parts):
        a, b = int(seg[lab]), int(seg[lab + 1])
        if b <= a:
            continue
        x = ref[a:b]
        with np.errstate(invalid="ignore", over="ignore"):
            e = x[:, None, :] - x[None, :, :]
            d = ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]).astype(F32)
        key = d.view(np.uint32)
        order = np.argsort(key, axis=1, kind="stable")[:, :k]               # stable: ties -> lowest index
        kk = np.take_along_axis(key, order, axis=1)
        nbr[a:b, :order.shape[1]] = np.where(kk < IO.EMPTY, order + a, -1)
    return nbr


def normals(ref, seg, n_parts, k=10):
    """-> (normals (M, 3) f32, curvature (M,) f32, neighbours (M, k) int32); NaN rows for degenerate points"""
    ref = np.asarray(ref, F32)
    nbr = neighbours(ref, seg, n_parts, k)
    M = ref.shape[0]
    nrm = np.full((M, 3), np.nan, F32)
    curv = np.full(M, np.nan, F32)
    for i in range(M):
        ids = nbr[i][nbr[i] >= 0]
        if ids.size < 3:
            continue
        x = ref[ids].astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            mean = x.sum(0) / ids.size
            e = x - mean
            C = (e[:, :, None] * e[:, None, :]).sum(0) / ids.size
        if not np.isfinite(C).all():
            continue
        lam, V = np.linalg.eigh(C)                                          # ascending
        v = V[:, 0]
        ax = int(np.argmax(np.abs(v)))                                      # first maximum: lowest axis on ties
        v = -v if v[ax] < 0 else v
        with np.errstate(invalid="ignore", divide="ignore"):
            cu = lam[0] / ((lam[0] + lam[1]) + lam[2])
        if not (lam[1] > 1e-12 * lam[2]) or not np.isfinite(cu):
            continue
        nrm[i] = v.astype(F32)
        curv[i] = F32(cu)
    return nrm, curv, nbr


# ---------------------------------------------------------------------------------------------------------------------
# sums, solve, loop
# ---------------------------------------------------------------------------------------------------------------------
def pair_terms(p, q, n, pose):
    """per pair (fp64): r (P,), a (P, 6) = [u x n, n] with u = R^T (p - t)"""
    R, t = pose[:3, :3], pose[:3, 3]
    u = (np.asarray(p, np.float64) - t) @ R
    n = np.asarray(n, np.float64)
    r = ((u - np.asarray(q, np.float64)) * n).sum(1)
    return r, np.concatenate([np.cross(u, n), n], axis=1)


def sums(scan, idx, ref, nrm, pose64):
    """(B, 29) fp64 sums over the kept pairs whose partner has a finite normal (layout: pn_icp_plane_sums)"""
    scan = np.asarray(scan, F32)
    B = scan.shape[0]
    out = np.zeros((B, NS))
    iu = np.triu_indices(6)
    for b in range(B):
        k = idx[b] >= 0
        k[k] = np.isfinite(nrm[idx[b][k]]).all(1)
        j = idx[b][k]
        r, a = pair_terms(scan[b][k], ref[j], nrm[j], np.asarray(pose64[b], np.float64))
        out[b, 0] = k.sum()
        out[b, 1:22] = (a[:, :, None] * a[:, None, :]).sum(0)[iu]
        out[b, 22:28] = (a * r[:, None]).sum(0)
        out[b, 28] = (r * r).sum()
    return out


def plane_sums(scan, labels, ref, seg, n_parts, nrm, pose64, max_d2=np.inf):
    """one pass: the point-to-point correspondence at the fp32 rounding of pose64, the terms at pose64 -> (idx, d2, sums)"""
    pose64 = np.asarray(pose64, np.float64)
    idx, d2 = IO.correspond(scan, labels, ref, seg, n_parts, pose64.astype(F32), max_d2)
    return idx, d2, sums(scan, idx, ref, nrm, pose64)


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th2 = float(w @ w)
    th = np.sqrt(th2)
    if th == 0.0:
        return np.eye(3)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    h = np.sin(0.5 * th) / th
    return np.eye(3) + np.sin(th) / th * K + 2.0 * h * h * (np.outer(w, w) - th2 * np.eye(3))


def step(S):
    """-> (x (6,), dropped): the minimum-norm solution of (sum a a^T) x = -(sum a r), eigenvalues <= 1e-12 lambda_max dropped"""
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = S[1:22]
    A = A + np.triu(A, 1).T
    if not np.isfinite(A).all() or not np.isfinite(S[22:28]).all():
        return np.zeros(6), True
    lam, V = np.linalg.eigh(A)
    keep = lam > EIG_CUT * lam.max()
    x = -(V[:, keep] @ ((V[:, keep].T @ S[22:28]) / lam[keep]))
    return x, not keep.all()


def apply(pose, x):
    """the pose after the model-frame step x = [omega, delta] (u -> E u + delta): R E^T, t - R E^T delta"""
    P = np.array(pose, np.float64).copy()
    R = P[:3, :3] @ rodrigues(x[:3]).T
    P[:3, :3] = R
    P[:3, 3] = P[:3, 3] - R @ np.asarray(x[3:], np.float64)
    P[3] = [0, 0, 0, 1]
    return P


def solve(S, pose_prev):
    """point-to-plane solve of one scan's sums -> (pose (4, 4), rmse, status)"""
    n = S[0]
    if not n >= 6:
        return np.array(pose_prev, np.float64).copy(), np.nan, FEW_PAIRS
    x, dropped = step(S)
    return apply(pose_prev, x), float(np.sqrt(S[28] / n)), DEGENERATE if dropped else 0


def icp(scan, labels, ref, seg, n_parts, nrm, init_pose, max_iters=30, max_d2=np.inf, tol_rot=1e-6, tol_t=1e-6):
    """the whole loop -> (pose (B,4,4), rmse (B,), pairs (B,), iters (B,), status (B,))"""
    scan = np.asarray(scan, F32)
    B = scan.shape[0]
    pose = np.array(init_pose, np.float64).reshape(B, 4, 4).copy()
    pose[:, 3] = [0, 0, 0, 1]
    rmse = np.full(B, np.nan)
    pairs = np.zeros(B, np.int32)
    iters = np.zeros(B, np.int32)
    status = np.zeros(B, np.int32)
    for b in range(B):
        for _ in range(max_iters):
            _, _, S = plane_sums(scan[b:b + 1], labels[b:b + 1], ref, seg, n_parts, nrm, pose[b:b + 1], max_d2)
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
# the labelled analytic scene
# ---------------------------------------------------------------------------------------------------------------------
AIRCRAFT_PARTS = ("fuselage", "wing", "hstab", "vstab", "engine")
TRUE_POSE = np.eye(4)
TRUE_POSE[:3, :3] = IO.rot([0.3, -0.5, 0.8], 0.7)                 # the pose of tools/bench_scan.py
TRUE_POSE[:3, 3] = [12.0, -4.0, 30.0]
START_POSE = np.eye(4)                                            # about 10 degrees and 1 m off
START_POSE[:3, :3] = IO.rot([1, 1, 0], np.deg2rad(10)) @ TRUE_POSE[:3, :3]
START_POSE[:3, 3] = TRUE_POSE[:3, 3] + [0.6, -0.5, 0.6]


def _cylinder(rng, n, x0, x1, radius, cy, cz):
    x = rng.uniform(x0, x1, n)
    a = rng.uniform(0, 2 * np.pi, n)
    return np.stack([x, cy + radius * np.cos(a), cz + radius * np.sin(a)], 1)


def _hemisphere(rng, n, cx, radius):
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v[:, 0] = np.abs(v[:, 0])                                      # the half facing +x
    return v * radius + [cx, 0, 0]


def _plate(rng, n, origin, e1, e2):
    s, t = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    return np.asarray(origin) + s[:, None] * np.asarray(e1, np.float64) + t[:, None] * np.asarray(e2, np.float64)


def _disc(rng, n, cx, cy, cz, radius):
    r = radius * np.sqrt(rng.uniform(0, 1, n))
    a = rng.uniform(0, 2 * np.pi, n)
    return np.stack([np.full(n, cx), cy + r * np.cos(a), cz + r * np.sin(a)], 1)


def _surfaces():
    """(part, area, sampler(rng, n)) of every analytic surface, model frame in metres, x forward"""
    R_F, R_E = 2.0, 1.0
    out = [(0, 2 * np.pi * R_F * 38.0, lambda g, n: _cylinder(g, n, -18.0, 20.0, R_F, 0.0, 0.0)),
           (0, 2 * np.pi * R_F * R_F, lambda g, n: _hemisphere(g, n, 20.0, R_F))]
    for sgn in (1.0, -1.0):
        out += [(1, 6.0 * 17.0, lambda g, n, s=sgn: _plate(g, n, [-2.0, s * 2.0, -0.8], [6.0, 0.0, 0.0], [-3.0, s * 17.0, 1.0])),
                (2, 4.0 * 6.0, lambda g, n, s=sgn: _plate(g, n, [-18.0, s * 1.5, 0.6], [4.0, 0.0, 0.0], [-1.5, s * 6.0, 0.3])),
                (4, 2 * np.pi * R_E * 5.0, lambda g, n, s=sgn: _cylinder(g, n, -2.0, 3.0, R_E, s * 8.0, -2.2)),
                (4, np.pi * R_E * R_E, lambda g, n, s=sgn: _disc(g, n, 3.0, s * 8.0, -2.2, R_E))]
    out.append((3, 5.0 * 7.0, lambda g, n: _plate(g, n, [-18.0, 0.0, 1.8], [5.0, 0.0, 0.0], [-2.5, 0.0, 7.0])))
    return out


def aircraft_surface(n, seed=0):
    """n area-weighted surface samples of the aircraft -> (xyz (n, 3) f64, part (n,) int32)"""
    rng = np.random.default_rng(seed)
    surf = _surfaces()
    area = np.array([a for _, a, _ in surf])
    counts = rng.multinomial(n, area / area.sum())
    xyz = np.concatenate([f(rng, int(c)) for (_, _, f), c in zip(surf, counts)])
    part = np.concatenate([np.full(int(c), p, np.int32) for (p, _, _), c in zip(surf, counts)])
    perm = rng.permutation(n)
    return xyz[perm], part[perm]


def aircraft_scene(n_ref=3000, n_scan=60000, noise=0.02, pose=TRUE_POSE, seed=0):
    """the labelled reference (xyz (n_ref, 3) f32, part (n_ref,) int32, model frame) and a labelled scan (xyz (n_scan, 3) f32 =
    independent surface samples under ``pose`` with N(0, noise) noise, part (n_scan,) int32)"""
    ref, ref_part = aircraft_surface(n_ref, seed)
    q, scan_part = aircraft_surface(n_scan, seed + 1)
    rng = np.random.default_rng(seed + 2)
    p = q @ np.asarray(pose)[:3, :3].T + np.asarray(pose)[:3, 3] + rng.normal(0, noise, size=q.shape)
    return ref.astype(F32), ref_part, p.astype(F32), scan_part
