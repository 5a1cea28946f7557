"""NumPy specification of the global start of the semantic ICP (include/pointnet_hip.h: pn_part_moments, pn_icp_seed_poses,
pn_icp_score_poses) and of the ops.global_pose composition: moments -> seeds -> score -> refine the top few -> select.  Built on
tests/icp_oracle.py (correspondence, Kabsch solve, the loop); the plane and mesh loops come from their own oracles.  Test
infrastructure only; nothing in the package imports it."""
import functools
import os

import numpy as np

import icp_oracle as IO

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rotation_grid(n):
    """(n, 3, 3) fp64: the super-Fibonacci spiral on the unit quaternions"""
    s = np.arange(n) + 0.5
    r, R = np.sqrt(s / n), np.sqrt(1.0 - s / n)
    al, be = 2.0 * np.pi * s / np.sqrt(2.0), 2.0 * np.pi * s / 1.533751168755204288118041
    x, y, z, w = r * np.sin(al), r * np.cos(al), R * np.sin(be), R * np.cos(be)
    out = np.empty((n, 3, 3))
    out[:, 0] = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1)
    out[:, 1] = np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1)
    out[:, 2] = np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)
    return out


def part_moments(scan, labels, n_parts):
    """(B, n_parts, 4) fp64: [n, sum x, sum y, sum z] over the points with label l and three finite coordinates"""
    scan = np.asarray(scan, F32)
    B = scan.shape[0]
    out = np.zeros((B, n_parts, 4))
    fin = np.isfinite(scan).all(-1)
    for b in range(B):
        for l in range(n_parts):
            p = scan[b][fin[b] & (labels[b] == l)].astype(np.float64)
            out[b, l, 0] = len(p)
            out[b, l, 1:] = p.sum(0)
    return out


def ref_moments_cloud(ref, seg, n_parts):
    """(n_parts, 4): point count and coordinate sum of every part of a grouped reference cloud"""
    lab = np.repeat(np.arange(n_parts), np.diff(seg)).astype(np.int32)
    return part_moments(np.asarray(ref, F32)[None], lab[None], n_parts)[0]


def ref_moments_mesh(tri, seg, area, n_parts):
    """(n_parts, 4): area and area-weighted sum of the triangle centroids of every part of a grouped mesh"""
    out = np.zeros((n_parts, 4))
    cen = np.asarray(tri, np.float64).mean(1)
    for l in range(n_parts):
        a = np.asarray(area, np.float64)[seg[l]:seg[l + 1]]
        out[l, 0] = a.sum()
        out[l, 1:] = (cen[seg[l]:seg[l + 1]] * a[:, None]).sum(0)
    return out


def seed_poses(mom, rmom, rotations):
    """(B, K + 1, 4, 4) fp64: K rotations about the shared-label centroids, then the rigid fit of the part centroids"""
    mom, rmom = np.asarray(mom, np.float64), np.asarray(rmom, np.float64)
    rot = np.zeros((0, 3, 3)) if rotations is None else np.asarray(rotations, np.float64).reshape(-1, 3, 3)
    B, n_parts, K = mom.shape[0], mom.shape[1], len(rot)
    out = np.zeros((B, K + 1, 4, 4))
    out[:, :, 3, 3] = 1.0
    for b in range(B):
        S = np.zeros(18)
        shared = 0
        for l in range(n_parts):
            n, w = mom[b, l, 0], rmom[l, 0]
            if not (n > 0 and w > 0):
                continue
            shared += 1
            p, cr = mom[b, l, 1:], rmom[l, 1:] / w
            cs = p / n
            S[0] += n
            S[1:4] += p
            S[4:7] += n * cr
            S[7:16] += np.outer(cr, p).reshape(9)
            S[16] += n * (cs @ cs)
            S[17] += n * (cr @ cr)
        cs, cr = (S[1:4] / S[0], S[4:7] / S[0]) if shared else (np.zeros(3), np.zeros(3))
        for k in range(K):
            out[b, k, :3, :3] = rot[k]
            out[b, k, :3, 3] = cs - rot[k] @ cr
        P = np.eye(4)
        P[:3, 3] = cs - cr
        if shared >= 3:
            P = IO.solve(S, P)[0]
        out[b, K] = P
    return out


def sample(scan_b, labels_b, seg, n_parts, stride):
    """indices of the sampled points of one scan: the points that take part, sorted by (label, index), every stride-th"""
    act = IO.active(scan_b[None], labels_b[None], seg, n_parts)[0]
    rows = np.flatnonzero(act)
    rows = rows[np.argsort(labels_b[rows], kind="stable")]
    return rows[::stride]


def _nearest_d2(p, lab, ref, seg, n_parts, pose32, chunk=32):
    """(K, m) f32: for K fp32 poses, every point's distance to the nearest reference point of its label (+inf when none),
    bit for bit icp_oracle.correspond's d2"""
    K, m = len(pose32), len(p)
    d2 = np.full((K, m), np.inf, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(n_parts):
            cols = np.flatnonzero(lab == l)
            r = ref[seg[l]:seg[l + 1]]
            if cols.size == 0 or len(r) == 0:
                continue
            for k0 in range(0, K, chunk):
                P = pose32[k0:k0 + chunk]
                d = (p[cols][None] - P[:, None, :3, 3]).astype(F32)                            # (k, m, 3)
                u = np.stack([(P[:, 0, i, None] * d[..., 0] + P[:, 1, i, None] * d[..., 1]) + P[:, 2, i, None] * d[..., 2]
                              for i in range(3)], -1).astype(F32)
                e = u[:, :, None, :] - r[None, None]
                dist = ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]).astype(F32)
                kmin = dist.view(np.uint32).min(-1)
                d2[k0:k0 + chunk, cols] = np.where(kmin < IO.EMPTY, kmin.view(F32), F32(np.inf))
    return d2


def score_poses(scan, labels, ref, seg, n_parts, poses, stride, max_d2):
    """-> (score (B, K, 2) fp64: inliers and truncated cost on the strided sample, order (B, K) int32: ascending (cost, k))"""
    scan = np.asarray(scan, F32)
    poses = np.asarray(poses, np.float64)
    B, K = poses.shape[:2]
    md = F32(max_d2)
    score = np.zeros((B, K, 2))
    for b in range(B):
        rows = sample(scan[b], labels[b], seg, n_parts, stride)
        with np.errstate(invalid="ignore", over="ignore"):
            p32 = poses[b].astype(F32)
        d2 = _nearest_d2(scan[b][rows], labels[b][rows], np.asarray(ref, F32), seg, n_parts, p32)
        with np.errstate(invalid="ignore"):
            inl = d2 <= md
        score[b, :, 0] = inl.sum(1)
        score[b, :, 1] = np.where(inl, d2, md).astype(F32).astype(np.float64).sum(1)
    return score, np.argsort(score[..., 1], axis=1, kind="stable").astype(np.int32)


def max_d2_of(max_dist):
    return F32(float(max_dist) * float(max_dist))


def global_pose(scan, labels, ref, seg, n_parts, max_dist, rotations=None, top=4, stride=None, metric="point", normals=None,
                mesh=None, **icp):
    """The ops.global_pose composition.  ``ref``/``seg``: a grouped cloud, or with ``mesh`` = (tri, seg, normals, area) the mesh
    (the coarse score then runs against its labelled vertex cloud).  -> dict(pose, rmse, pairs, iters, status, cost, winner, top,
    seeds, coarse (B, K + 1, 2), order, refined (B, top, 4, 4), fine (B, top))"""
    scan = np.asarray(scan, F32)
    B, N, _ = scan.shape
    md = max_d2_of(max_dist)
    rot = rotation_grid(256) if rotations is None else rotations
    stride = max(1, N // 8192) if stride is None else stride
    if mesh is not None:
        tri, mseg, mnrm, area = mesh
        rmom = ref_moments_mesh(tri, mseg, area, n_parts)
        cloud, cseg = np.asarray(tri, F32).reshape(-1, 3), np.asarray(mseg) * 3
    else:
        rmom = ref_moments_cloud(ref, seg, n_parts)
        cloud, cseg = np.asarray(ref, F32), np.asarray(seg)
    seeds = seed_poses(part_moments(scan, labels, n_parts), rmom, rot)
    coarse, order = score_poses(scan, labels, cloud, cseg, n_parts, seeds, stride, md)
    top = min(top, seeds.shape[1])
    pick = order[:, :top]
    out = dict(seeds=seeds, coarse=coarse, order=order, top=pick, refined=np.zeros((B, top, 4, 4)), fine=np.zeros((B, top)))
    res = [np.zeros((B, 4, 4)), np.zeros(B), np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)]
    out["winner"], out["cost"] = np.zeros(B, np.int32), np.zeros(B)
    for b in range(B):
        s, l = np.repeat(scan[b:b + 1], top, 0), np.repeat(labels[b:b + 1], top, 0)
        start = seeds[b, pick[b]]
        if mesh is not None:
            import icp_mesh_oracle as MO
            r = MO.icp(s, l, tri, mseg, n_parts, mnrm, start, metric=metric, max_d2=md, **icp)
            d2 = MO.correspond(s, l, tri, mseg, n_parts, r[0].astype(F32))[1]
            act = IO.active(s, l, mseg, n_parts)
            with np.errstate(invalid="ignore"):
                c = np.where(d2 <= md, d2, md).astype(np.float64)
            fine = np.where(act, c, 0.0).sum(1)
        else:
            if metric == "plane":
                import icp_plane_oracle as PO
                r = PO.icp(s, l, ref, seg, n_parts, normals, start, max_d2=md, **icp)
            else:
                r = IO.icp(s, l, ref, seg, n_parts, start, max_d2=md, **icp)
            fine = score_poses(scan[b:b + 1], labels[b:b + 1], cloud, cseg, n_parts, r[0][None], 1, md)[0][0, :, 1]
        w = int(np.argmin(fine))                                     # first minimum: ties go to the earlier candidate
        out["refined"][b], out["fine"][b] = r[0], fine
        for dst, src in zip(res, r):
            dst[b] = src[w]
        out["winner"][b], out["cost"][b] = pick[b, w], fine[w]
    out.update(pose=res[0], rmse=res[1], pairs=res[2], iters=res[3], status=res[4])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the shared cases: kc-46, 1024-point scans, 5 cm noise, 5 % outliers, a true pose per seed
# ---------------------------------------------------------------------------------------------------------------------
FULL_SEEDS, ONE_SIDED_SEEDS = (1, 2, 5, 6), (0, 1, 3, 7)
CASES = tuple((s, False) for s in FULL_SEEDS) + tuple((s, True) for s in ONE_SIDED_SEEDS)
CAP_ROT, CAP_T = 1e-2, 5e-2                        # rad, m: how close to the truth a recovered pose must be
PARAMS = dict(top=4, stride=4, max_iters=40)
MAX_DIST = 3.0


def true_pose(seed):
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=3)
    angle = rng.uniform(0, np.pi)
    P = np.eye(4)
    P[:3, :3] = IO.rot(axis, angle)
    P[:3, 3] = rng.uniform(-30, 30, 3)
    return P


@functools.lru_cache(maxsize=None)
def kc46(n_parts):
    """the kc-46 fixture grouped: (xyz, part, ref, seg)"""
    import helpers
    from pointcloudprocessing_amd import pointcloud
    xyz, part = pointcloud.read_labelled_cloud(os.path.join(ROOT, "tests", "golden", "kc-46.txt"), helpers.F15_PARTS)
    ref, seg, _ = IO.group_reference(xyz, part, n_parts)
    return xyz, part, ref, seg


@functools.lru_cache(maxsize=None)
def case(seed, one_sided, n_parts):
    """-> (scan (1024, 3) f32, labels (1024,) int32, true pose): a kc-46 scan under true_pose(seed); one-sided: the points
    whose model-frame y is at most -1 m carry label -1, as a LiDAR sees an aircraft from one side"""
    xyz, part, _, _ = kc46(n_parts)
    T = true_pose(seed)
    scan, lab = IO.labelled_scan(xyz, part, 1024, T, noise=0.05, outliers=0.05, seed=seed)
    if one_sided:
        model = (scan.astype(np.float64) - T[:3, 3]) @ T[:3, :3]
        lab = np.where(model[:, 1] <= -1.0, -1, lab).astype(np.int32)
    return scan, lab, T


@functools.lru_cache(maxsize=None)
def solved(seed, one_sided, n_parts):
    """the oracle pipeline on one shared case, computed once"""
    _, _, ref, seg = kc46(n_parts)
    scan, lab, _ = case(seed, one_sided, n_parts)
    return global_pose(scan[None], lab[None], ref, seg, n_parts, MAX_DIST, rotations=rotation_grid(256), **PARAMS)
