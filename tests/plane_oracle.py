"""NumPy statement of pn_plane_segment's specification (include/pointnet_hip.h) -- TEST INFRASTRUCTURE.

One function per step of a round (hypotheses, score, select, refine, label), ``round`` for a whole round on a given active set and
``segment`` for the loop, plus the fixtures tests/test_cpu_plane.py and tests/test_gpu_plane.py share.  Hypotheses and scores are
integers and np.float32 operations in the order the header writes them, so they are compared bit for bit; the refined plane is
fp64 sums whose order the device fixes differently (blocks, waves), so ``refine`` takes the order as an argument and the tests derive
their tolerance from the spread between two orders.  Nothing in the package imports this module."""
import numpy as np

import mesh_sample_oracle as SO

F32 = np.float32
F64 = np.float64
DOMAIN = 0x504C414E
TILE = 1024            # PN_PLANE_TILE
MAX_H, MAX_P = 4096, 8


def active_rows(xyz, plane_id=None):
    """bool (N,): three finite coordinates and on no plane yet"""
    a = np.isfinite(np.asarray(xyz, F32)).all(1)
    return a if plane_id is None else a & (np.asarray(plane_id) < 0)


def draws(M, r, H, seed):
    """(H, 3) int64: the list positions i_0, i_1, i_2 of every hypothesis of round r on a list of M rows"""
    ctr = np.zeros((H, 4), np.uint64)
    ctr[:, 0] = np.arange(H)
    ctr[:, 1] = r
    ctr[:, 3] = DOMAIN
    x = SO.philox4x32(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).astype(np.uint64)
    return ((x[:, :3] * np.uint64(M)) >> np.uint64(32)).astype(np.int64)


def hypotheses(xyz, active, r, H, threshold, seed=0, axis=None, cos_max_angle=1.0):
    """-> dict(idx (H, 3) list positions, p0 (H, 3) f32, c (H, 3) f32, t2 (H,) f32, valid (H,) bool) on the ascending active list"""
    x = np.asarray(xyz, F32)[np.flatnonzero(active)]
    idx = draws(len(x), r, H, seed)
    p0, p1, p2 = x[idx[:, 0]], x[idx[:, 1]], x[idx[:, 2]]
    with np.errstate(all="ignore"):
        e1, e2 = p1 - p0, p2 - p0
        c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1).astype(F32)
        l2 = ((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]).astype(F32)
        valid = (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2]) & np.isfinite(l2) & (l2 > 0)
        if axis is not None:
            a = np.asarray(axis, F32)
            g = ((c[:, 0] * a[0] + c[:, 1] * a[1]) + c[:, 2] * a[2]).astype(F32)
            a2 = F32(F32(a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
            cos = F32(cos_max_angle)
            valid &= (g * g).astype(F32) >= ((F32(cos * cos) * l2).astype(F32) * a2).astype(F32)
        t2 = (F32(F32(threshold) * F32(threshold)) * l2).astype(F32)
    assert c.dtype == F32 and l2.dtype == F32 and t2.dtype == F32
    return dict(idx=idx, p0=p0, c=c, t2=t2, valid=valid)


def inliers(x, p0, c, t2):
    """bool (M,): s*s <= t2 for the points x (M, 3) f32 against one hypothesis"""
    with np.errstate(all="ignore"):
        d = x - p0
        s = ((c[0] * d[:, 0] + c[1] * d[:, 1]) + c[2] * d[:, 2]).astype(F32)
        return (s * s).astype(F32) <= t2


def score(xyz, active, hyp):
    """(H,) int32: the inliers of every hypothesis among the active rows, -1 for an invalid one"""
    x = np.asarray(xyz, F32)[np.flatnonzero(active)]
    out = np.full(len(hyp["valid"]), -1, np.int32)
    for h in np.flatnonzero(hyp["valid"]):
        out[h] = int(inliers(x, hyp["p0"][h], hyp["c"][h], hyp["t2"][h]).sum())
    return out


def select(counts):
    """the largest count, the lowest h among ties (np.argmax: the first maximum); -1 when no hypothesis is valid"""
    return int(np.argmax(counts)) if (np.asarray(counts) >= 0).any() else -1


def _sum(v, order):
    if order == "pairwise":                                              # NumPy sums a contiguous axis pairwise (a strided one in sequence)
        return np.ascontiguousarray(v.reshape(len(v), -1).T).sum(-1).reshape(v.shape[1:])
    if order == "sequential":
        return np.cumsum(v, 0)[-1]
    raise ValueError(order)


def refine(xyz, active, hyp, h, order="pairwise"):
    """the refined plane (4,) f64 of hypothesis h: least-eigenvalue direction of the inliers' covariance about their mean, in
    coordinates relative to p0, oriented along c; ``order``: how the ten sums are taken ("pairwise" or "sequential")"""
    x = np.asarray(xyz, F32)[np.flatnonzero(active)]
    p0, c = hyp["p0"][h].astype(F64), hyp["c"][h].astype(F64)
    q = x[inliers(x, hyp["p0"][h], hyp["c"][h], hyp["t2"][h])].astype(F64) - p0
    n = float(len(q))
    mean = _sum(q, order) / n
    Q = _sum(q[:, :, None] * q[:, None, :], order)
    C = Q / n - mean[:, None] * mean[None, :]
    lam, V = np.linalg.eigh(C)                                           # ascending
    nrm = V[:, 0]
    if (nrm[0] * c[0] + nrm[1] * c[1]) + nrm[2] * c[2] < 0:
        nrm = -nrm
    pm = p0 + mean
    d = -((nrm[0] * pm[0] + nrm[1] * pm[1]) + nrm[2] * pm[2])
    return np.array([nrm[0], nrm[1], nrm[2], d], F64)


def label(xyz, active, plane, threshold):
    """bool (N,): the active rows within ``threshold`` (fp32 value, compared in fp64) of ``plane`` (4,) f64"""
    x = np.asarray(xyz, F32).astype(F64)
    pl = np.asarray(plane, F64)
    with np.errstate(all="ignore"):
        e = ((pl[0] * x[:, 0] + pl[1] * x[:, 1]) + pl[2] * x[:, 2]) + pl[3]
        return np.asarray(active, bool) & (np.abs(e) <= F64(F32(threshold)))


def round(xyz, active, r, threshold, hypotheses_n, seed=0, axis=None, cos_max_angle=1.0, order="pairwise"):   # noqa: A001
    """one round on the active set -> (hyp_counts (H,) int32, winner, plane (4,) f64, mask (N,) bool of the rows within the threshold of
    the refined plane).  M < 3: (None, -1, None, None); no valid hypothesis: (counts, -1, None, None).  min_inliers is the loop's."""
    active = np.asarray(active, bool)
    if int(active.sum()) < 3:
        return None, -1, None, None
    hyp = hypotheses(xyz, active, r, hypotheses_n, threshold, seed, axis, cos_max_angle)
    counts = score(xyz, active, hyp)
    win = select(counts)
    if win < 0:
        return counts, -1, None, None
    plane = refine(xyz, active, hyp, win, order)
    return counts, win, plane, label(xyz, active, plane, threshold)


def segment(xyz, threshold, max_planes=1, hypotheses_n=1024, min_inliers=3, seed=0, axis=None, cos_max_angle=1.0, order="pairwise"):
    """the whole loop -> (planes (P, 4) f64, counts (P,) int32, plane_id (N,) int32, hyp_counts (P, H) int32)"""
    xyz = np.asarray(xyz, F32)
    P, H = max_planes, hypotheses_n
    planes, counts = np.zeros((P, 4), F64), np.zeros(P, np.int32)
    plane_id, hyp_counts = np.full(len(xyz), -1, np.int32), np.full((P, H), -1, np.int32)
    for r in range(P):
        hc, win, plane, mask = round(xyz, active_rows(xyz, plane_id), r, threshold, H, seed, axis, cos_max_angle, order)
        if hc is None:
            break
        hyp_counts[r] = hc
        if win < 0 or int(mask.sum()) < min_inliers:
            break
        planes[r], counts[r] = plane, int(mask.sum())
        plane_id[mask] = r
    return planes, counts, plane_id, hyp_counts


def order_spread(xyz, active, r, threshold, hypotheses_n, seed=0, axis=None, cos_max_angle=1.0):
    """max |difference| between the planes refined with pairwise and with sequential sums: the size of the fp64 summation-order
    effect on this input (0.0 when the round refines nothing)"""
    a = round(xyz, active, r, threshold, hypotheses_n, seed, axis, cos_max_angle, "pairwise")[2]
    b = round(xyz, active, r, threshold, hypotheses_n, seed, axis, cos_max_angle, "sequential")[2]
    return 0.0 if a is None else float(np.abs(a - b).max())


# ---------------------------------------------------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------------------------------------------------
def random_cloud(n, seed=0):
    """n points in [-1, 1]^3, a third of them within 0.02 of the plane z = 0.3 x - 0.2 y"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, size=(n, 3))
    on = rng.random(n) < 1.0 / 3.0
    x[on, 2] = 0.3 * x[on, 0] - 0.2 * x[on, 1] + rng.uniform(-0.02, 0.02, size=int(on.sum()))
    return x.astype(F32)


def lattice(seed=0):
    """the 512 points with integer coordinates in [0, 8), shuffled: every product and sum of the hypothesis and the score is exact in
    fp32 (|c| <= 98, |s| <= 2058, s*s and t2 < 2^24 at threshold 1; quarters at threshold 0.5), so the inlier test s*s <= t2 is an
    exact integer comparison, distances of exactly the threshold occur, and the scores tie massively (the best one too)"""
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3)
    return g[np.random.default_rng(seed).permutation(512)].astype(F32)


def lattice_counts_exact(xyz, hyp):
    """the scores of ``lattice`` in Python integers (threshold^2 as the exact fraction num / den) -> function(num, den) -> (H,) counts"""
    x = np.asarray(xyz).astype(np.int64)
    p0, c = hyp["p0"].astype(np.int64), hyp["c"].astype(np.int64)

    def counts(num, den):
        out = np.full(len(c), -1, np.int64)
        for h in np.flatnonzero(hyp["valid"]):
            s = (x - p0[h]) @ c[h]
            out[h] = int((den * s * s <= num * int(c[h] @ c[h])).sum())
        return out
    return counts


def collinear(n=500, seed=0):
    """n distinct points on the line t (1, 2, 4), t = 0 .. n-1: exact in fp32, every cross product is exactly zero"""
    t = np.random.default_rng(seed).permutation(n).astype(F32)
    return np.stack([t, 2 * t, 4 * t], 1).astype(F32)


def ulp_steps(v, k):
    """the fp32 value k representable steps from v"""
    v = F32(v)
    for _ in range(abs(int(k))):
        v = np.nextafter(v, F32(np.inf) if k > 0 else F32(-np.inf), dtype=F32)
    return v


def threshold_edge(threshold, H, r=0, seed=0, lattice_base=False, n_base=200, per_side=17, n_hyp=6, rng_seed=3):
    """a cloud whose last rows sit within +-8 ulp of the threshold distance from the planes of ``n_hyp`` valid hypotheses of round r:
    base rows (quarter-integer coordinates when ``lattice_base``, else random) come first and the hypotheses used draw only from
    them, so appending the adversarial rows (M is fixed in advance) does not move the planes.  For every such hypothesis and both
    sides of its plane a point p0 + u e1 + v e2 +- threshold c/|c| is rounded to fp32 and its coordinate along the largest |c|
    component is stepped -8 .. +8 ulp -> (xyz (M, 3) f32, the hypotheses used)"""
    rng = np.random.default_rng(rng_seed)
    n_adv = n_hyp * 2 * per_side
    M = n_base + n_adv
    base = (rng.integers(-40, 40, size=(n_base, 3)) / 4.0 if lattice_base else rng.uniform(-3.0, 3.0, size=(n_base, 3))).astype(F32)
    xyz = np.concatenate([base, np.zeros((n_adv, 3), F32)])
    idx = draws(M, r, H, seed)
    hyp = hypotheses(np.concatenate([base, np.zeros((n_adv, 3), F32)]), np.ones(M, bool), r, H, threshold, seed)
    usable = [h for h in range(H) if hyp["valid"][h] and (idx[h] < n_base).all()][:n_hyp]
    assert len(usable) == n_hyp, "too few hypotheses draw from the base rows alone"
    row = n_base
    for h in usable:
        p0, c = hyp["p0"][h].astype(F64), hyp["c"][h].astype(F64)
        e1, e2 = base[idx[h, 1]].astype(F64) - p0, base[idx[h, 2]].astype(F64) - p0
        ax = int(np.argmax(np.abs(c)))
        for side in (1.0, -1.0):
            u, v = rng.uniform(-0.5, 1.5, size=2)
            p = (p0 + u * e1 + v * e2 + side * float(F32(threshold)) * c / np.sqrt(c @ c)).astype(F32)
            for k in range(-(per_side // 2), per_side // 2 + 1):
                q = p.copy()
                q[ax] = ulp_steps(p[ax], k)
                xyz[row] = q
                row += 1
    assert row == M
    return xyz, usable


def floor_and_wall(n=1500, seed=0):
    """a floor (z ~ 0) and a wall (x ~ 0) of n points each, +-0.01 of noise, and 300 scattered points; rows shuffled"""
    rng = np.random.default_rng(seed)
    floor = np.stack([rng.uniform(0, 4, n), rng.uniform(0, 4, n), rng.uniform(-0.01, 0.01, n)], 1)
    wall = np.stack([rng.uniform(-0.01, 0.01, n), rng.uniform(0, 4, n), rng.uniform(0, 4, n)], 1)
    other = rng.uniform(0.5, 3.5, size=(300, 3))
    tag = np.r_[np.zeros(n, int), np.ones(n, int), np.full(300, 2)]
    perm = rng.permutation(len(tag))
    return np.concatenate([floor, wall, other])[perm].astype(F32), tag[perm]


SCENE = dict(threshold=0.1, hypotheses=256, max_planes=3, min_inliers=1500)
SCENE_CLUSTER_LEAF = 1.0


def floor_scene(seed=7):
    """the clean 4,096-point aircraft scan of cluster_oracle.cluttered_scene() on a floor (6,000 points, +-0.03 in height, half a
    cluster leaf below the aircraft's lowest point) in front of a wall (3,000 points, +-0.03, half a leaf behind its rearmost point in y);
    the row groups interleaved -> (scene (13096, 3) f32, aircraft rows, floor rows, wall rows, clean scan (4096, 3) f32)"""
    import cluster_oracle as CO
    clean = CO.cluttered_scene()[3]
    rng = np.random.default_rng(seed)
    lo, hi = clean.min(0).astype(F64), clean.max(0).astype(F64)
    z0 = lo[2] - 0.5 * SCENE_CLUSTER_LEAF
    y0 = hi[1] + 0.5 * SCENE_CLUSTER_LEAF
    floor = np.stack([rng.uniform(lo[0] - 3, hi[0] + 3, 6000), rng.uniform(lo[1] - 3, y0, 6000), z0 + rng.uniform(-0.03, 0.03, 6000)], 1).astype(F32)
    wall = np.stack([rng.uniform(lo[0] - 3, hi[0] + 3, 3000), y0 + rng.uniform(-0.03, 0.03, 3000), rng.uniform(z0, z0 + 12, 3000)], 1).astype(F32)
    parts = [("f", floor[:1000]), ("a", clean[:2000]), ("w", wall[:1500]), ("f", floor[1000:4000]), ("a", clean[2000:]), ("w", wall[1500:]),
             ("f", floor[4000:])]
    scene = np.concatenate([x for _, x in parts]).astype(F32)
    tag = np.concatenate([np.full(len(x), t) for t, x in parts])
    return scene, np.flatnonzero(tag == "a"), np.flatnonzero(tag == "f"), np.flatnonzero(tag == "w"), clean
