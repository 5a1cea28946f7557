"""NumPy specification of the robust, confidence-weighted semantic ICP (include/pointnet_hip.h, pn_icp_robust_sums,
pn_icp_robust_solve, pn_semantic_icp_robust): the scale of the robust kernel from the lower median of the kept pairs' d2, the pairs'
weights, the 19 / 30 weighted sums, the weighted solves and the loop, on top of the searches, per-pair terms and solves of
tests/icp_oracle.py, tests/icp_plane_oracle.py and tests/icp_mesh_oracle.py.  A reference is a dict: a cloud
``dict(xyz=(M, 3) f32 grouped, seg=..., n_parts=..., normals=(M, 3) f32 or None)`` or a mesh ``dict(tri=(T, 3, 3) f32 grouped,
seg=..., n_parts=..., normals=(T, 3) f32)``.  Test infrastructure only; nothing in the package imports it."""
import numpy as np

import icp_mesh_oracle as MO
import icp_oracle as IO
import icp_plane_oracle as PO

F32 = np.float32
CONVERGED, FEW_PAIRS, DEGENERATE = 1, 2, 4
KERNELS = {None: 0, "none": 0, "huber": 1, "cauchy": 2, "tukey": 3}
TUNE = {0: 1.0, 1: 1.345, 2: 2.385, 3: 4.685}


def cloud(xyz, seg, n_parts, normals=None):
    return dict(xyz=np.asarray(xyz, F32), seg=seg, n_parts=n_parts, normals=normals)


def mesh(tri, seg, n_parts, normals):
    return dict(tri=np.asarray(tri, F32), seg=seg, n_parts=n_parts, normals=np.asarray(normals, F32))


def search(scan, labels, ref, pose32, max_d2=np.inf):
    """the unchanged correspondence search -> (idx (B, N), d2 (B, N), q (B, N, 3): the partner, NaN when there is none)"""
    if "tri" in ref:
        return MO.correspond(scan, labels, ref["tri"], ref["seg"], ref["n_parts"], pose32, max_d2)
    # the nearest candidate first, kept or not: the search reports its point as q, and keeps the pair iff d2 <= max_d2
    near, d2 = IO.correspond(scan, labels, ref["xyz"], ref["seg"], ref["n_parts"], pose32, np.inf)
    q = np.where((near >= 0)[..., None], ref["xyz"][np.maximum(near, 0)], F32(np.nan)).astype(F32)
    return np.where(d2 <= F32(max_d2), near, -1).astype(np.int32), d2, q


def lower_median(d2_kept):
    """the element of rank (n - 1) >> 1 in ascending order of the fp32 bit patterns, as a uint32 pattern (n >= 1)"""
    bits = np.sort(np.ascontiguousarray(d2_kept, F32).view(np.uint32))
    return bits[(bits.size - 1) >> 1]


def scale(d2, kept, kernel, robust_scale="mad", tune=None, min_scale=1e-4):
    """c of one scan: d2 (N,) f32, kept (N,) bool"""
    k = KERNELS[kernel] if not isinstance(kernel, int) else kernel
    if k == 0:
        return np.nan
    if robust_scale != "mad":
        return float(robust_scale)
    tune = TUNE[k] if tune is None else float(tune)
    if not kept.any():
        return float(min_scale)
    med = np.array([lower_median(d2[kept])], np.uint32).view(F32)[0]
    sigma = 1.4826 * np.sqrt(np.float64(med))
    t = tune * sigma
    return float(t if t > min_scale else min_scale)


def kernel_weight(kernel, d2, c):
    """the robust weight of pairs at squared distance d2 (fp32 array) and scale c, fp64"""
    k = KERNELS[kernel] if not isinstance(kernel, int) else kernel
    d = np.asarray(d2, F32).astype(np.float64)
    if k == 0:
        return np.ones_like(d)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        x = d / (c * c)
        if k == 1:
            return np.where(x <= 1.0, 1.0, 1.0 / np.sqrt(x))
        if k == 2:
            return 1.0 / (1.0 + x)
        return np.where(x < 1.0, (1.0 - x) * (1.0 - x), 0.0)


def point_weight(weights):
    """the per-point factor: fp32 widened to fp64; negative, NaN or infinite counts as 0"""
    u = np.asarray(weights, F32)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(u) & (u >= 0)
    return np.where(ok, u, F32(0)).astype(np.float64)


def pass_sums(scan, labels, ref, pose64, metric="point", max_d2=np.inf, weights=None, kernel=None, robust_scale="mad", tune=None,
              min_scale=1e-4, magnitude=False):
    """one pass at the fp32 rounding of pose64 -> (idx, d2, q, w (B, N) f64, scale (B,), sums (B, 19 | 30)); with ``magnitude``
    the sums are those of the terms' absolute values (what a tolerance on the sums scales with)"""
    scan = np.asarray(scan, F32)
    pose64 = np.asarray(pose64, np.float64)
    B, N, _ = scan.shape
    plane = metric == "plane"
    idx, d2, q = search(scan, labels, ref, pose64.astype(F32), max_d2)
    ns = 29 if plane else 18
    w = np.zeros((B, N))
    sc = np.zeros(B)
    S = np.zeros((B, ns + 1))
    iu = np.triu_indices(6)
    for b in range(B):
        kept = idx[b] >= 0
        sc[b] = scale(d2[b], kept, kernel, robust_scale, tune, min_scale)
        counted = kept.copy()
        if plane:
            counted[kept] = np.isfinite(ref["normals"][idx[b][kept]]).all(1)
        wb = kernel_weight(kernel, d2[b][counted], sc[b])
        if weights is not None:
            wb = wb * point_weight(weights[b][counted])
        w[b, counted] = wb
        p = scan[b][counted].astype(np.float64)
        qq = q[b][counted].astype(np.float64)
        if magnitude:
            p, qq = np.abs(p), np.abs(qq)
        if plane:
            r, a = PO.pair_terms(scan[b][counted], q[b][counted], ref["normals"][idx[b][counted]], pose64[b])
            if magnitude:
                r, a = np.abs(r), np.abs(a)
            S[b, 0] = wb.sum()
            S[b, 1:22] = ((a[:, :, None] * a[:, None, :]) * wb[:, None, None]).sum(0)[iu]
            S[b, 22:28] = ((a * r[:, None]) * wb[:, None]).sum(0)
            S[b, 28] = ((r * r) * wb).sum()
        else:
            S[b, 0] = wb.sum()
            S[b, 1:4] = (p * wb[:, None]).sum(0)
            S[b, 4:7] = (qq * wb[:, None]).sum(0)
            S[b, 7:16] = ((qq[:, :, None] * p[:, None, :]) * wb[:, None, None]).sum(0).reshape(9)
            S[b, 16] = ((p * p) * wb[:, None]).sum()
            S[b, 17] = ((qq * qq) * wb[:, None]).sum()
        S[b, ns] = (wb > 0).sum()
    return idx, d2, q, w, sc, S


def solve(S, pose_prev, metric="point"):
    """the weighted solve of one scan's 19 / 30 sums -> (pose (4, 4), rmse, status)"""
    plane = metric == "plane"
    ns, need = (29, 6) if plane else (18, 3)
    n = S[0]
    if not S[ns] >= need or not n > 0:
        return np.array(pose_prev, np.float64).copy(), np.nan, FEW_PAIRS
    if plane:
        x, dropped = PO.step(S[:29])
        return PO.apply(pose_prev, x), float(np.sqrt(S[28] / n)), DEGENERATE if dropped else 0
    sp, sq = S[1:4], S[4:7]                                     # icp_oracle.solve's Kabsch with n = sum w
    H = S[7:16].reshape(3, 3) - np.outer(sq, sp) / n
    U, _, Vt = np.linalg.svd(H)
    R = Vt.T @ U.T
    if np.linalg.det(R) < 0:
        Vt = Vt.copy()
        Vt[2, :] *= -1
        R = Vt.T @ U.T
    Sp = S[16] - sp @ sp / n
    Sq = S[17] - sq @ sq / n
    P = np.eye(4)
    P[:3, :3] = R
    P[:3, 3] = sp / n - R @ (sq / n)
    return P, float(np.sqrt(max(0.0, Sp + Sq - 2.0 * np.trace(R @ H)) / n)), 0


def icp(scan, labels, ref, init_pose, metric="point", max_iters=30, max_d2=np.inf, tol_rot=1e-6, tol_t=1e-6, weights=None, kernel=None,
        robust_scale="mad", tune=None, min_scale=1e-4):
    """the whole loop -> (pose (B,4,4), rmse (B,), pairs (B,), iters (B,), status (B,), scale (B,))"""
    scan = np.asarray(scan, F32)
    B = scan.shape[0]
    pose = np.array(init_pose, np.float64).reshape(B, 4, 4).copy()
    pose[:, 3] = [0, 0, 0, 1]
    rmse = np.full(B, np.nan)
    pairs = np.zeros(B, np.int32)
    iters = np.zeros(B, np.int32)
    status = np.zeros(B, np.int32)
    sc = np.full(B, np.nan)
    ns = 29 if metric == "plane" else 18
    for b in range(B):
        wb = None if weights is None else weights[b:b + 1]
        for _ in range(max_iters):
            _, _, _, _, c, S = pass_sums(scan[b:b + 1], labels[b:b + 1], ref, pose[b:b + 1], metric, max_d2, wb, kernel, robust_scale,
                                         tune, min_scale)
            new, rm, st = solve(S[0], pose[b], metric)
            iters[b] += 1
            rmse[b], pairs[b], sc[b] = rm, int(S[0, ns]), c[0]
            few = st & FEW_PAIRS
            conv = bool(few) or (IO.rotation_angle(new[:3, :3], pose[b, :3, :3]) < tol_rot
                                 and np.linalg.norm(new[:3, 3] - pose[b, :3, 3]) < tol_t)
            pose[b] = new
            status[b] = st | (CONVERGED if conv else 0)
            if conv:
                break
    return pose, rmse, pairs, iters, status, sc


def wrong_labels(labels, n_parts, share, seed):
    """a copy of labels (N,) with a share of them (chosen without replacement) replaced by a random OTHER part"""
    rng = np.random.default_rng(seed)
    lab = np.array(labels, np.int32).copy()
    pick = rng.choice(lab.size, int(round(share * lab.size)), replace=False)
    lab[pick] = (lab[pick] + rng.integers(1, n_parts, pick.size)) % n_parts
    return lab
