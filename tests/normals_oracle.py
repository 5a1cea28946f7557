"""NumPy statement of pn_scan_normals' specification (include/pointnet_hip.h), of ops.incidence_mask, and the veil scene -- TEST
INFRASTRUCTURE.

neighbourhood   row i itself, then the filled slots of neighbors_oracle.radius_knn(xyz, radius, k) in their order; c = min(count, k) + 1
covariance      the c points in float64: mean = (sum in that order) / c, C = (sum in that order of (x - mean)(x - mean)^T) / c
eigenvectors    np.linalg.eigh (ascending), as icp_plane_oracle.normals: the library runs a fixed-order Jacobi, the tests compare
                |n . n_oracle| and the curvature l0 / ((l0 + l1) + l2) within 1e-6
degenerate      c < 3, l1 <= 1e-12 l2, or a non-finite value: NaN normal and curvature; the count is written all the same
sign            no viewpoint: the component of largest magnitude positive, lowest axis on ties.  With a viewpoint vp:
                s = (n.x (vp.x - p.x) + n.y (vp.y - p.y)) + n.z (vp.z - p.z) in float64 on the float32 values; s < 0 flips, s > 0
                keeps, s == 0 or NaN leaves the rule above
incidence       v = vp - p in float64; keep iff the normal is finite, v.v > 0 and (n.v)^2 >= cos^2(max_angle) (v.v)
"""
from __future__ import annotations

import functools
import math

import numpy as np

import neighbors_oracle as NO

F32 = np.float32
MIN_K, MAX_K = 2, NO.MAX_K
PLATE, WALL, VEIL = 0, 1, 2


def dot3(a, b):
    """(a.x b.x + a.y b.y) + a.z b.z, rows of (P, 3) float64"""
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def radius_knn(xyz, radius, k):
    """NO.radius_knn(xyz, radius, k), bit for bit, in less time on a large finite cloud: its brute force (NO.dist2, the same 64-bit
    keys) runs per cell of a coarse grid (side 2 radius, far above any rounding of the distance), the cell's rows against the rows of
    the 27 cells around it.  (tests/test_cpu_normals.py compares the two.)"""
    xyz = np.ascontiguousarray(xyz, F32)
    N = len(xyz)
    cell = np.floor((xyz.astype(np.float64) - xyz.min(0)) / (2.0 * float(radius))).astype(np.int64)
    idx = np.full((N, k), -1, np.int32)
    d2 = np.full((N, k), np.inf, F32)
    count = np.zeros(N, np.int32)
    r2 = F32(radius) * F32(radius)
    empty = np.uint64(0xFFFFFFFFFFFFFFFF)
    for c in np.unique(cell, axis=0):
        cand = np.flatnonzero((np.abs(cell - c) <= 1).all(1))               # ascending rows
        rows = cand[(cell[cand] == c).all(1)]
        d = NO.dist2(xyz[rows], xyz[cand])
        ok = (d <= r2) & (rows[:, None] != cand[None, :])                   # False for a NaN; j != i by row
        count[rows] = ok.sum(1)
        key = np.where(ok, (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | cand.astype(np.uint64)[None, :], empty)
        best = np.sort(key, axis=1)[:, :k]
        filled = best != empty
        kk = best.shape[1]
        idx[rows, :kk] = np.where(filled, (best & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
        d2[rows, :kk] = np.where(filled, (best >> np.uint64(32)).astype(np.uint32).view(F32), F32(np.inf))
    return idx, d2, count


def normals(xyz, radius, k=8, viewpoint=None, knn=None):
    """-> (normals (N, 3) f32, curvature (N,) f32, count (N,) i32, idx (N, k) i32); ``knn``: a precomputed radius_knn(xyz, radius, k)"""
    xyz = np.ascontiguousarray(xyz, F32)
    assert MIN_K <= k <= MAX_K
    idx, _, count = radius_knn(xyz, radius, k) if knn is None else knn
    N = len(xyz)
    x64 = xyz.astype(np.float64)
    ids = np.concatenate([np.arange(N)[:, None], idx], 1)                   # (N, k + 1): the filled slots are a prefix
    valid = ids >= 0
    c = valid.sum(1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        pts = np.where(valid[:, :, None], x64[np.clip(ids, 0, None)], 0.0)
        mean = np.zeros((N, 3))
        for s in range(k + 1):                                              # in neighbourhood order (an unfilled slot adds 0)
            mean = mean + pts[:, s]
        mean = mean / c[:, None]
        C = np.zeros((N, 3, 3))
        for s in range(k + 1):
            e = np.where(valid[:, s, None], pts[:, s] - mean, 0.0)
            C = C + e[:, :, None] * e[:, None, :]
        C = C / c[:, None, None]
        ok = (c >= 3) & np.isfinite(C).all((1, 2))
        lam, V = np.linalg.eigh(np.where(ok[:, None, None], C, np.eye(3)))  # ascending
        v = V[:, :, 0]
        ax = np.argmax(np.abs(v), 1)                                        # first maximum: lowest axis on ties
        v = np.where((v[np.arange(N), ax] < 0)[:, None], -v, v)
        cu = lam[:, 0] / ((lam[:, 0] + lam[:, 1]) + lam[:, 2])
        ok &= (lam[:, 1] > 1e-12 * lam[:, 2]) & np.isfinite(cu) & np.isfinite(v).all(1)
        if viewpoint is not None:
            d = np.asarray(viewpoint, F32).astype(np.float64) - x64
            v = np.where((dot3(v, d) < 0)[:, None], -v, v)
    nrm = np.where(ok[:, None], v, np.nan).astype(F32)
    curv = np.where(ok, cu, np.nan).astype(F32)
    return nrm, curv, count, idx


def incidence_mask(xyz, nrm, viewpoint, max_angle_deg, return_margin=False):
    """bool (N,); with ``return_margin`` also | |n.v| / |v| - cos(max_angle) | per row (inf where the normal is not finite or v = 0): how
    far a decision is from the threshold"""
    ang = float(max_angle_deg)
    assert 0.0 < ang < 90.0
    v = np.asarray([float(a) for a in viewpoint], np.float64) - np.asarray(xyz).astype(np.float64)
    n = np.asarray(nrm).astype(np.float64)
    c = math.cos(math.radians(ang))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        nv, vv = dot3(n, v), dot3(v, v)
        ok = np.isfinite(n).all(1) & (vv > 0)
        keep = ok & (nv * nv >= (c * c) * vv)
        margin = np.where(ok, np.abs(np.abs(nv) / np.sqrt(vv) - c), np.inf)
    return (keep, margin) if return_margin else keep


def veil_scene(seed=0):
    """A mixed-pixel scene.  Sensor at the origin looking along +x, a 150 x 150 raster over +-10 degrees in azimuth and elevation; a
    plate through (20, 0, 0) with normal (cos 30, sin 30, 0) and half-extents 2.5 (in-plane horizontal) x 1.5 (z); a wall at
    x = 22.5.  Every wall ray that is 4-adjacent in the raster to a plate ray is a mixed pixel: re-ranged uniformly in
    [t_plate + 0.3 + 0.15 g, t_plate + 0.3 + 0.85 g] with g = t_wall - t_plate - 0.6 and t_plate the ray's own intersection with the
    plate's (unbounded) plane -- a veil along the view rays between the plate's edge and the wall close behind it.  N(0, 0.01) range
    noise on every ray.  -> (xyz (22500, 3) f32, kind (22500,) int: PLATE / WALL / VEIL)"""
    rng = np.random.default_rng(seed)
    R = 150
    a = np.radians(np.linspace(-10.0, 10.0, R))
    az, el = np.meshgrid(a, a, indexing="ij")
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1)          # (R, R, 3) unit rays
    n = np.array([math.cos(math.radians(30.0)), math.sin(math.radians(30.0)), 0.0])
    u = np.array([-n[1], n[0], 0.0])                                                           # in-plane horizontal axis
    c0 = np.array([20.0, 0.0, 0.0])
    t_plate = (c0 @ n) / (d @ n)
    hit = d * t_plate[..., None] - c0
    on_plate = (np.abs(hit @ u) <= 2.5) & (np.abs(hit[..., 2]) <= 1.5)
    t_wall = 22.5 / d[..., 0]
    near = np.zeros_like(on_plate)
    near[1:] |= on_plate[:-1]
    near[:-1] |= on_plate[1:]
    near[:, 1:] |= on_plate[:, :-1]
    near[:, :-1] |= on_plate[:, 1:]
    veil = near & ~on_plate
    g = t_wall - t_plate - 0.6
    t_veil = t_plate + 0.3 + g * rng.uniform(0.15, 0.85, size=g.shape)
    t = np.where(on_plate, t_plate, np.where(veil, t_veil, t_wall)) + rng.normal(0.0, 0.01, size=g.shape)
    kind = np.where(on_plate, PLATE, np.where(veil, VEIL, WALL))
    return (d * t[..., None]).reshape(-1, 3).astype(F32), kind.reshape(-1)


# ---- fixtures the CPU and the GPU tests share -----------------------------------------------------------------------
def lattice_plane(side=9, z=3.0, seed=5):
    """the side^2 points of the integer lattice in the plane z = const, shuffled"""
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)
    g = g[np.random.default_rng(seed).permutation(len(g))]
    return np.concatenate([g, np.full((len(g), 1), z)], 1).astype(F32)


# (viewpoint, sign of the normal's z) on lattice_plane(): none, above, below, and in the plane (s == 0: the rule without a viewpoint)
LATTICE_PLANE_VIEWS = ((None, 1.0), ((4.0, 4.0, 10.0), 1.0), ((4.0, 4.0, -2.5), -1.0), ((100.0, -7.0, 3.0), 1.0))

VEIL_SETTINGS = dict(radius=0.6, k=8, max_angle_deg=75.0)


@functools.lru_cache(maxsize=None)
def veil_case():
    """the veil scene at VEIL_SETTINGS seen from the sensor origin, computed once: dict(xyz, kind, nrm, curv, count, keep, margin)"""
    xyz, kind = veil_scene(0)
    nrm, curv, count, _ = normals(xyz, VEIL_SETTINGS["radius"], VEIL_SETTINGS["k"], (0.0, 0.0, 0.0))
    keep, margin = incidence_mask(xyz, nrm, (0.0, 0.0, 0.0), VEIL_SETTINGS["max_angle_deg"], return_margin=True)
    return dict(xyz=xyz, kind=kind, nrm=nrm, curv=curv, count=count, keep=keep, margin=margin)
