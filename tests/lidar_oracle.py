"""NumPy specification of the LiDAR ray caster and packer (include/pointnet_hip.h, pn_lidar_cast and pn_lidar_pack): two-sided
Moller-Trumbore operation for operation in np.float32 with the header's operand order and tie rule, the same formula in fp64 (with
the second-smallest t, for judging near ties), and the packing rule.  Also the integer-grid wall whose hits are exact in fp32.  Test
infrastructure only; nothing in the package imports it."""
import numpy as np

F32 = np.float32


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _cross(x, y):
    return np.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1],
                     x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
                     x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], axis=-1)


def _frame(P, dirs, dt):
    """the origin o = R^T (0 - t) and the directions R^T d in the model frame, in icp_to_model's operand order"""
    R = P[:3, :3].astype(dt)
    g = (dt(0) - P[:3, 3].astype(dt)).astype(dt)
    o = np.array([(R[0, i] * g[0] + R[1, i] * g[1]) + R[2, i] * g[2] for i in range(3)], dt)
    d = np.stack([(R[0, i] * dirs[:, 0] + R[1, i] * dirs[:, 1]) + R[2, i] * dirs[:, 2] for i in range(3)], axis=1).astype(dt)
    return o, d


def _ray_triangle(o, d, tri, t_min, t_max, dt):
    """every ray of d (n, 3) against every triangle of tri (T, 3, 3) from the origin o -> (hit (n, T) bool, t (n, T)); every line is
    one rounded operation per element in ``dt``"""
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    e1, e2 = b - a, c - a
    s = o[None, :] - a                                         # (T, 3): per (frame, triangle)
    q = _cross(s, e1)
    w = _dot(e2, q)[None, :]
    p = _cross(d[:, None, :], e2[None, :, :])                  # (n, T, 3): per ray
    det = _dot(e1[None], p)
    u = _dot(s[None], p)
    v = _dot(d[:, None, :], q[None])
    neg = det < 0
    det = np.where(neg, -det, det)
    u = np.where(neg, -u, u)
    v = np.where(neg, -v, v)
    w = np.where(neg, -w, w)
    t = (w / det).astype(dt)
    hit = (det > 0) & (u >= 0) & (v >= 0) & (u + v <= det) & (t >= dt(t_min)) & (t <= dt(t_max))
    return hit, t


def cast(tri, poses, dirs, t_min=0.0, t_max=np.inf, chunk=2048):
    """the specification in fp32 -> (hit (B, R) int32: the first triangle's grouped row or -1, t (B, R) f32: its ray parameter or
    +inf).  Among equal t the lowest row wins (np.argmin takes the first minimum, and -0 == +0)."""
    tri = np.asarray(tri, F32).reshape(-1, 3, 3)
    poses = np.asarray(poses, F32).reshape(-1, 4, 4)
    dirs = np.asarray(dirs, F32).reshape(-1, 3)
    B, R = len(poses), len(dirs)
    hit = np.full((B, R), -1, np.int32)
    tt = np.full((B, R), np.inf, F32)
    if len(tri) == 0:
        return hit, tt
    with np.errstate(all="ignore"):
        for b in range(B):
            o, d = _frame(poses[b], dirs, F32)
            for r0 in range(0, R, chunk):
                h, t = _ray_triangle(o, d[r0:r0 + chunk], tri, t_min, t_max, F32)
                tm = np.where(h, t, F32(np.inf))
                j = np.argmin(tm, axis=1)
                best = tm[np.arange(len(j)), j]
                found = best < F32(np.inf)
                hit[b, r0:r0 + chunk] = np.where(found, j, -1)
                tt[b, r0:r0 + chunk] = np.where(found, best, F32(np.inf))
    return hit, tt


def cast_fp64(tri, poses, dirs, t_min=0.0, t_max=np.inf, chunk=2048):
    """the same formula in fp64 on the same fp32 inputs -> (hit (B, R) int32, t (B, R) f64, t2 (B, R) f64: the second-smallest t
    among the triangles hit, +inf when fewer than two are)"""
    tri = np.asarray(tri, F32).reshape(-1, 3, 3).astype(np.float64)
    poses = np.asarray(poses, F32).reshape(-1, 4, 4).astype(np.float64)
    dirs = np.asarray(dirs, F32).reshape(-1, 3).astype(np.float64)
    B, R = len(poses), len(dirs)
    hit = np.full((B, R), -1, np.int32)
    tt = np.full((B, R), np.inf)
    t2 = np.full((B, R), np.inf)
    if len(tri) == 0:
        return hit, tt, t2
    with np.errstate(all="ignore"):
        for b in range(B):
            o, d = _frame(poses[b], dirs, np.float64)
            for r0 in range(0, R, chunk):
                h, t = _ray_triangle(o, d[r0:r0 + chunk], tri, t_min, t_max, np.float64)
                tm = np.where(h, t, np.inf)
                j = np.argmin(tm, axis=1)
                ar = np.arange(len(j))
                best = tm[ar, j]
                found = best < np.inf
                hit[b, r0:r0 + chunk] = np.where(found, j, -1)
                tt[b, r0:r0 + chunk] = np.where(found, best, np.inf)
                if tm.shape[1] > 1:
                    tm[ar, j] = np.inf
                    t2[b, r0:r0 + chunk] = tm.min(axis=1)
    return hit, tt, t2


def part_of_row(rows, seg, n_parts):
    """the label whose range [seg[l], seg[l + 1]) holds each grouped triangle row: the last l < n_parts with seg[l] <= row"""
    return np.searchsorted(np.asarray(seg)[1:n_parts], rows, side="right").astype(np.int32)


def pack(hit, t, dirs, seg, n_parts, N):
    """-> (xyz (B, N, 3) f32, part (B, N) int32, ray (B, N) int32, count (B,) int32)"""
    hit = np.asarray(hit)
    t = np.asarray(t, F32)
    dirs = np.asarray(dirs, F32).reshape(-1, 3)
    B = hit.shape[0]
    xyz = np.full((B, N, 3), np.nan, F32)
    part = np.full((B, N), -1, np.int32)
    ray = np.full((B, N), -1, np.int32)
    count = np.zeros(B, np.int32)
    k = np.arange(N, dtype=np.int64)
    with np.errstate(all="ignore"):
        for b in range(B):
            rays = np.flatnonzero(hit[b] >= 0)
            n = count[b] = len(rays)
            if n == 0:
                continue
            src = rays[(k * n) // N if n >= N else k % n]
            ray[b] = src
            part[b] = part_of_row(hit[b, src], seg, n_parts)
            xyz[b] = t[b, src, None] * dirs[src]
    return xyz, part, ray, count


def wall_mesh(x, y0, y1, z0, z1, label=0):
    """the plane x = const over [y0, y1] x [z0, z1] as unit quads with integer vertices, each cut along its diagonal ->
    (tri (T, 3, 3) f32, part (T,) int32).  A grid vertex inside the wall belongs to six triangles, an edge to two."""
    tri = []
    for j in range(y0, y1):
        for k in range(z0, z1):
            a, b, c, d = [x, j, k], [x, j + 1, k], [x, j + 1, k + 1], [x, j, k + 1]
            tri += [[a, b, c], [a, c, d]]
    return np.array(tri, F32), np.full(len(tri), label, np.int32)
