"""NumPy specification of plane-to-plane (generalized) semantic ICP (include/pointnet_hip.h, pn_icp_gicp_sums,
pn_semantic_icp_gicp): the per-pair weight matrix W by its closed form, the 29 fp64 sums over the pairs found by the point-to-point
correspondence rule (tests/icp_oracle.py), one pass and the loop.  The solve is the plane metric's (tests/icp_plane_oracle.py).
Test infrastructure only; nothing in the package imports it."""
import numpy as np

import icp_oracle as IO
import icp_plane_oracle as PO

F32 = np.float32
NS = 29
EPS = 1e-3


def unit(n):
    """rows of n (fp32 or fp64) widened and divided by sqrt((x*x + y*y) + z*z)"""
    n = np.asarray(n, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return n / np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])[:, None]


def to_model(v, R):
    """R^T v per row in the operand order of the header: (R_0i x + R_1i y) + R_2i z"""
    return np.stack([(R[0, i] * v[:, 0] + R[1, i] * v[:, 1]) + R[2, i] * v[:, 2] for i in range(3)], axis=1)


def valid_normal(n):
    """(P,) bool: finite in all components, squared length finite and > 0"""
    n = np.asarray(n)
    with np.errstate(invalid="ignore", over="ignore"):
        w = n.astype(np.float64)
        l2 = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]
    return np.isfinite(n).all(1) & np.isfinite(l2) & (l2 > 0)


def weight_parts(a, m, eps=EPS):
    """unit a, m (P, 3) -> (s, f, D_s, D_f)"""
    kap = 1.0 - eps
    s, f = a + m, a - m
    Ds = 2.0 * eps + 0.5 * kap * ((f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]) + f[:, 2] * f[:, 2])
    Df = 2.0 * eps + 0.5 * kap * ((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    return s, f, Ds, Df


def weight(a, m, eps=EPS, absolute=False):
    """W (P, 3, 3) = eps I + (eps kappa / 2)(s s^T / D_s + f f^T / D_f) for unit a and m; ``absolute``: with |s| and |f|, the
    termwise magnitude of W (its off-diagonal entries cancel, W's own magnitudes do not bound the rounding)"""
    s, f, Ds, Df = weight_parts(a, m, eps)
    if absolute:
        s, f = np.abs(s), np.abs(f)
    c = 0.5 * eps * (1.0 - eps)
    return eps * np.eye(3)[None] + ((c / Ds)[:, None, None] * (s[:, :, None] * s[:, None, :])
                                    + (c / Df)[:, None, None] * (f[:, :, None] * f[:, None, :]))


def jacobian(u):
    """J (P, 3, 6) = [-[u]_x, I]: d(E u + delta) / d[omega, delta] at 0"""
    J = np.zeros((len(u), 3, 6))
    J[:, 0, 1], J[:, 0, 2] = u[:, 2], -u[:, 1]
    J[:, 1, 0], J[:, 1, 2] = -u[:, 2], u[:, 0]
    J[:, 2, 0], J[:, 2, 1] = u[:, 1], -u[:, 0]
    J[:, :, 3:] = np.eye(3)
    return J


def pair_terms(p, q, nq, npn, pose, eps=EPS):
    """per counted pair (fp64): u (P, 3), d (P, 3), W (P, 3, 3), a, m (P, 3)"""
    pose = np.asarray(pose, np.float64)
    R, t = pose[:3, :3], pose[:3, 3]
    u = to_model(np.asarray(p, np.float64) - t, R)
    d = u - np.asarray(q, np.float64)
    a = unit(nq)
    m = unit(to_model(np.asarray(npn, np.float64), R))
    return u, d, weight(a, m, eps), a, m


def counted(idx_b, nrm, scan_nrm_b):
    """(N,) bool: the kept pairs of one scan that count"""
    k = idx_b >= 0
    k[k] = valid_normal(nrm[idx_b[k]])
    return k & valid_normal(scan_nrm_b)


def assemble(u, d, W, absolute=False):
    """the 29 sums of the given pairs from their J, W and d; ``absolute``: every factor already a magnitude"""
    J = jacobian(u)
    if absolute:
        J = np.abs(J)
    e = np.einsum("nab,nb->na", W, d)
    out = np.zeros(NS)
    out[0] = len(u)
    out[1:22] = np.einsum("nai,nab,nbj->ij", J, W, J)[np.triu_indices(6)]
    out[22:28] = np.einsum("nai,na->i", J, e)
    out[28] = (d * e).sum()
    return out


def sums(scan, scan_nrm, idx, ref, nrm, pose64, eps=EPS, magnitudes=False):
    """(B, 29) fp64 sums over the counted pairs (layout: pn_icp_gicp_sums); ``magnitudes``: the sums of the termwise magnitudes
    instead, from |J|, |d| and weight(absolute=True)"""
    scan = np.asarray(scan, F32)
    B = scan.shape[0]
    out = np.zeros((B, NS))
    for b in range(B):
        k = counted(idx[b], nrm, scan_nrm[b])
        j = idx[b][k]
        u, d, W, a, m = pair_terms(scan[b][k], ref[j], nrm[j], scan_nrm[b][k], pose64[b], eps)
        if magnitudes:
            d, W = np.abs(d), weight(a, m, eps, absolute=True)
        out[b] = assemble(u, d, W, absolute=magnitudes)
    return out


def gicp_sums(scan, labels, scan_nrm, ref, seg, n_parts, nrm, pose64, max_d2=np.inf, eps=EPS):
    """one pass: the point-to-point correspondence at the fp32 rounding of pose64, the terms at pose64 -> (idx, d2, sums)"""
    pose64 = np.asarray(pose64, np.float64)
    idx, d2 = IO.correspond(scan, labels, ref, seg, n_parts, pose64.astype(F32), max_d2)
    return idx, d2, sums(scan, scan_nrm, idx, ref, nrm, pose64, eps)


def icp(scan, labels, scan_nrm, ref, seg, n_parts, nrm, init_pose, max_iters=30, max_d2=np.inf, tol_rot=1e-6, tol_t=1e-6, eps=EPS):
    """the whole loop -> (pose (B,4,4), rmse (B,), pairs (B,), iters (B,), status (B,)); the plane oracle's loop with these sums"""
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
            _, _, S = gicp_sums(scan[b:b + 1], labels[b:b + 1], scan_nrm[b:b + 1], ref, seg, n_parts, nrm, pose[b:b + 1], max_d2, eps)
            new, rm, st = PO.solve(S[0], pose[b])
            iters[b] += 1
            rmse[b], pairs[b] = rm, int(S[0, 0])
            few = st & PO.FEW_PAIRS
            conv = bool(few) or (IO.rotation_angle(new[:3, :3], pose[b, :3, :3]) < tol_rot
                                 and np.linalg.norm(new[:3, 3] - pose[b, :3, 3]) < tol_t)
            pose[b] = new
            status[b] = st | (PO.CONVERGED if conv else 0)
            if conv:
                break
    return pose, rmse, pairs, iters, status


def covariance(n, eps=EPS):
    """C = I - (1 - eps) n n^T for unit rows n: the surface covariance with eigenvalues (eps, 1, 1)"""
    return np.eye(3)[None] - (1.0 - eps) * (n[:, :, None] * n[:, None, :])


# ---------------------------------------------------------------------------------------------------------------------
# the shared GPU case: tests/test_gpu_icp_plane.py's kc-46 case with scan normals
# ---------------------------------------------------------------------------------------------------------------------
PLANTED = ("half", "triple", "parallel", "antiparallel", "nan", "zero")   # (the counting kinds first: a scan of one point has one)
N_PLANTED = 24                               # rows per planted kind


def scan_normals(rng, scan, labels, ref, seg, n_parts, nrm, pose, max_d2=np.inf):
    """random unit directions (B, N, 3) fp32 with N_PLANTED rows of every kind in PLANTED among the pairs that are kept and whose
    partner has a valid normal (as many as there are, when fewer) -> (normals, {kind: (b, rows)})"""
    B, N, _ = scan.shape
    v = rng.normal(size=(B, N, 3))
    sn = (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F32)
    idx, _ = IO.correspond(scan, labels, ref, seg, n_parts, np.asarray(pose, np.float64).astype(F32), max_d2)
    where = {}
    for b in range(B):
        ok = np.flatnonzero(idx[b] >= 0)
        ok = ok[valid_normal(nrm[idx[b][ok]])]
        pick = rng.permutation(ok)
        for t, kind in enumerate(PLANTED):
            rows = pick[t * N_PLANTED:(t + 1) * N_PLANTED]
            where.setdefault(kind, []).append((b, rows))
            if kind == "nan":
                sn[b, rows, rng.integers(0, 3, len(rows))] = np.nan
            elif kind == "zero":
                sn[b, rows] = 0
            elif kind == "half":
                sn[b, rows] *= F32(0.5)
            elif kind == "triple":
                sn[b, rows] *= F32(3)
            else:
                R = np.asarray(pose[b], np.float64)[:3, :3]
                a = unit(nrm[idx[b][rows]]) @ R.T                        # R n_q: the partner's normal in the scan's frame
                sn[b, rows] = (a if kind == "parallel" else -a).astype(F32)
    return sn, where
