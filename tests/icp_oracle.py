"""NumPy specification of the label-constrained ICP (include/pointnet_hip.h, pn_semantic_icp): fp32 correspondence without
contraction, fp64 sums and Kabsch solve (np.linalg.svd with the literal reflection rule), the convergence rule of the loop.
Test infrastructure only; nothing in the package imports it."""
import numpy as np

F32 = np.float32
EMPTY = np.uint32(0x7F800001)          # above +inf's pattern, at or below every NaN pattern
CONVERGED, FEW_PAIRS = 1, 2


def group_reference(xyz, labels, n_parts):
    """stable grouping by label -> (grouped xyz (M, 3) f32, seg (n_parts + 1,), original index (M,))"""
    lab = np.asarray(labels).astype(np.int64)
    keep = np.flatnonzero((lab >= 0) & (lab < n_parts))
    order = keep[np.argsort(lab[keep], kind="stable")]
    seg = np.searchsorted(lab[order], np.arange(n_parts + 1))
    return np.asarray(xyz, F32)[order], seg.astype(np.int64), order


def active(scan, labels, seg, n_parts):
    """(B, N) bool: the points that take part"""
    lab = labels.astype(np.int64)
    ok = (lab >= 0) & (lab < n_parts) & np.isfinite(scan).all(-1)
    sizes = np.diff(seg)
    ok &= sizes[np.clip(lab, 0, n_parts - 1)] > 0
    return ok


def to_model_frame(p, pose32):
    """u = R^T (p - t) in fp32, each product and sum rounded, left to right: (R_0i dx + R_1i dy) + R_2i dz"""
    R = pose32[:3, :3].astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):          # NaN / inf rows: they never take part
        d = (p - pose32[:3, 3].astype(F32)).astype(F32)
        return np.stack([(R[0, i] * d[:, 0] + R[1, i] * d[:, 1]) + R[2, i] * d[:, 2] for i in range(3)], axis=1).astype(F32)


def correspond(scan, labels, ref, seg, n_parts, pose32, max_d2=np.inf, chunk=4096):
    """-> idx (B, N) int32 (grouped partner index or -1), d2 (B, N) f32 (nearest same-label distance, +inf when none)"""
    scan = np.asarray(scan, F32)
    B, N, _ = scan.shape
    idx = np.full((B, N), -1, np.int32)
    d2 = np.full((B, N), np.inf, F32)
    act = active(scan, labels, seg, n_parts)
    md = F32(max_d2)
    for b in range(B):
        u = to_model_frame(scan[b], np.asarray(pose32[b], F32))
        for lab in range(n_parts):
            rows = np.flatnonzero(act[b] & (labels[b] == lab))
            if rows.size == 0:
                continue
            r = ref[seg[lab]:seg[lab + 1]]
            for c0 in range(0, rows.size, chunk):
                rr = rows[c0:c0 + chunk]
                e = u[rr, None, :] - r[None, :, :]
                dist = ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]).astype(F32)
                key = dist.view(np.uint32)
                j = np.argmin(key, axis=1)                       # first minimum: ties -> lowest index
                kmin = key[np.arange(rr.size), j]
                found = kmin < EMPTY
                dd = np.where(found, kmin.view(F32), F32(np.inf)).astype(F32)
                d2[b, rr] = dd
                idx[b, rr] = np.where(found & (dd <= md), j + seg[lab], -1)
    return idx, d2


def sums(scan, idx, ref):
    """(B, 18) fp64 sums over the kept pairs: n, sum p, sum q, sum q_i p_j (7 + 3i + j), sum |p|^2, sum |q|^2"""
    B = scan.shape[0]
    out = np.zeros((B, 18))
    for b in range(B):
        k = idx[b] >= 0
        p = scan[b][k].astype(np.float64)
        q = ref[idx[b][k]].astype(np.float64)
        out[b, 0] = k.sum()
        out[b, 1:4] = p.sum(0)
        out[b, 4:7] = q.sum(0)
        out[b, 7:16] = (q[:, :, None] * p[:, None, :]).sum(0).reshape(9)
        out[b, 16] = (p * p).sum()
        out[b, 17] = (q * q).sum()
    return out


def solve(S, pose_prev):
    """Kabsch on one scan's sums -> (pose (4, 4), rmse, status)"""
    n = S[0]
    if not n >= 3:
        return np.array(pose_prev, np.float64).copy(), np.nan, FEW_PAIRS
    sp, sq = S[1:4], S[4:7]
    H = S[7:16].reshape(3, 3) - np.outer(sq, sp) / n
    U, s, Vt = np.linalg.svd(H)
    R = Vt.T @ U.T
    if np.linalg.det(R) < 0:
        Vt = Vt.copy()
        Vt[2, :] *= -1                                           # the smallest singular value's vector (s is descending)
        R = Vt.T @ U.T
    t = sp / n - R @ (sq / n)
    Sp = S[16] - sp @ sp / n
    Sq = S[17] - sq @ sq / n
    rmse = np.sqrt(max(0.0, Sp + Sq - 2.0 * np.trace(R @ H)) / n)
    P = np.eye(4)
    P[:3, :3] = R
    P[:3, 3] = t
    return P, rmse, 0


def rotation_angle(R_new, R_old):
    M = R_new.T @ R_old
    w = np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    return float(np.arctan2(0.5 * np.linalg.norm(w), 0.5 * (np.trace(M) - 1.0)))


def icp(scan, labels, ref, seg, n_parts, init_pose, max_iters=30, max_d2=np.inf, tol_rot=1e-6, tol_t=1e-6):
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
            idx, _ = correspond(scan[b:b + 1], labels[b:b + 1], ref, seg, n_parts, pose[b:b + 1].astype(F32), max_d2)
            S = sums(scan[b:b + 1], idx, ref)[0]
            new, rm, few = solve(S, pose[b])
            iters[b] += 1
            rmse[b], pairs[b] = rm, int(S[0])
            conv = bool(few) or (rotation_angle(new[:3, :3], pose[b, :3, :3]) < tol_rot
                                 and np.linalg.norm(new[:3, 3] - pose[b, :3, 3]) < tol_t)
            pose[b] = new
            status[b] = few | (CONVERGED if conv else 0)
            if conv:
                break
    return pose, rmse, pairs, iters, status


def horn(q, p):
    """independent rigid fit p ~= R q + t by Horn's unit-quaternion method (fp64)"""
    q = np.asarray(q, np.float64)
    p = np.asarray(p, np.float64)
    qc, pc = q - q.mean(0), p - p.mean(0)
    Sm = qc.T @ pc
    (xx, xy, xz), (yx, yy, yz), (zx, zy, zz) = Sm
    Nm = np.array([[xx + yy + zz, yz - zy, zx - xz, xy - yx],
                   [yz - zy, xx - yy - zz, xy + yx, zx + xz],
                   [zx - xz, xy + yx, -xx + yy - zz, yz + zy],
                   [xy - yx, zx + xz, yz + zy, -xx - yy + zz]])
    w, v = np.linalg.eigh(Nm)
    a, b, c, d = v[:, -1]
    R = np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                  [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                  [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])
    return R, p.mean(0) - R @ q.mean(0)


def rot(axis, angle):
    """rotation matrix about ``axis`` by ``angle`` (Rodrigues)"""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def pose_error(P, Q):
    """(rotation angle between P and Q, |t_P - t_Q|)"""
    return rotation_angle(P[:3, :3], Q[:3, :3]), float(np.linalg.norm(P[:3, 3] - Q[:3, 3]))


def labelled_scan(ref_xyz, ref_part, n, true_pose, noise=0.05, outliers=0.05, seed=0):
    """scan (n, 3) f32 and labels (n,) int32: reference points under ``true_pose`` with N(0, noise) noise, plus a share of
    uniform outliers labelled -1, shuffled"""
    rng = np.random.default_rng(seed)
    n_out = int(round(outliers * n))
    pick = rng.integers(0, len(ref_xyz), n - n_out)
    q = ref_xyz[pick].astype(np.float64)
    p = q @ true_pose[:3, :3].T + true_pose[:3, 3] + rng.normal(0, noise, size=q.shape)
    lo, hi = p.min(0) - 1, p.max(0) + 1
    o = rng.uniform(lo, hi, size=(n_out, 3))
    xyz = np.concatenate([p, o]).astype(F32)
    lab = np.concatenate([ref_part[pick], np.full(n_out, -1)]).astype(np.int32)
    perm = rng.permutation(n)
    return xyz[perm], lab[perm]
