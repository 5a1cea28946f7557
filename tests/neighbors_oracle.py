"""NumPy statement of pn_radius_knn's specification (include/pointnet_hip.h) and of ops.neighbor_stat_mask -- TEST INFRASTRUCTURE.

distance    dx = p_i.x - p_j.x etc., d = (dx*dx + dy*dy) + dz*dz in float32, that operand order (NumPy does not contract)
neighbours  { j != i : d(i, j) <= r2 }, r2 = radius * radius in float32; a NaN never qualifies; j != i is by row
outputs     count = the size of that set (not capped); idx / d2 (N, k) = the k smallest by ascending (bit pattern of d, j), unfilled
            slots (-1, +inf).  Brute force over all pairs, in row chunks: the grid is the library's business, not the specification's
keys        floor((p - origin) / h) per axis in float32 with h = leaf(radius): only what the containment test looks at
"""
from __future__ import annotations

import itertools

import numpy as np

F32 = np.float32
MAX_KEY = 1 << 14
MAX_K = 16


def leaf(radius):
    """radius * (1 + 2^-6) rounded UP to float32 (the product is exact in float64): pn_radius_knn_leaf"""
    exact = np.float64(F32(radius)) * (1.0 + 2.0 ** -6)
    h = F32(exact)
    if np.float64(h) < exact:
        h = np.nextafter(h, F32(np.inf))
    return F32(h)


def keys(xyz, h, origin):
    """(N, 3) float64 of the per-axis floor((p - origin) / h) computed in float32 (not range-checked: the caller decides)"""
    xyz = np.asarray(xyz, F32)
    return np.floor((xyz - np.asarray(origin, F32)) / F32(h)).astype(np.float64)


def dist2(a, b):
    """d(a_i, b_j) (len(a), len(b)) float32 in the specified operand order"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def radius_knn(xyz, radius, k, chunk=512):
    """-> (idx (N, k) i32, d2 (N, k) f32, count (N,) i32)"""
    xyz = np.ascontiguousarray(xyz, F32)
    N = len(xyz)
    assert 0 <= k <= MAX_K
    r2 = F32(radius) * F32(radius)
    idx = np.full((N, k), -1, np.int32)
    d2 = np.full((N, k), np.inf, F32)
    count = np.zeros(N, np.int32)
    cols = np.arange(N, dtype=np.uint64)
    empty = np.uint64(0xFFFFFFFFFFFFFFFF)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, N, chunk):
            e = min(s + chunk, N)
            d = dist2(xyz[s:e], xyz)
            ok = d <= r2                                           # False for a NaN
            ok[np.arange(e - s), np.arange(s, e)] = False          # j != i by row
            count[s:e] = ok.sum(1)
            if k == 0:
                continue
            key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | cols[None, :]
            key[~ok] = empty
            kk = min(k, N)
            best = np.sort(np.partition(key, kk - 1, axis=1)[:, :kk], axis=1) if kk < N else np.sort(key, axis=1)
            filled = best != empty
            idx[s:e, :kk] = np.where(filled, (best & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
            d2[s:e, :kk] = np.where(filled, (best >> np.uint64(32)).astype(np.uint32).view(F32), F32(np.inf))
    return idx, d2, count


def stat_mask(d2, count, k, std_ratio, return_stats=False):
    """ops.neighbor_stat_mask: full = count >= k; m_i = mean over the k slots of sqrt(d2) in float64; mu, population sigma of m over
    the full points; keep = full and m_i <= mu + std_ratio * sigma (nothing when no point is full)"""
    d2 = np.asarray(d2)
    full = np.asarray(count) >= k
    keep = np.zeros(len(full), bool)
    if not full.any() or k < 1:
        return (keep, None, None, None) if return_stats else keep
    with np.errstate(invalid="ignore"):
        m = np.sqrt(d2[:, :k].astype(np.float64)).mean(1)
    mu = m[full].mean()
    sigma = np.sqrt(((m[full] - mu) ** 2).mean())
    thr = mu + float(std_ratio) * sigma
    keep[full] = m[full] <= thr
    return (keep, m, thr, full) if return_stats else keep


# ---- fixtures the CPU and the GPU tests share -----------------------------------------------------------------------
def lattice(side, seed=0):
    """the side^3 points of the unit integer lattice in shuffled row order -> (xyz f32, integer coordinates)"""
    c = np.array(list(itertools.product(range(side), repeat=3)), np.int64)
    c = c[np.random.default_rng(seed).permutation(len(c))]
    return c.astype(F32), c


def ulp_steps(x, n):
    """x moved by n float32 ulps (n may be negative)"""
    x = F32(x)
    for _ in range(abs(int(n))):
        x = np.nextafter(x, F32(np.inf) if n > 0 else F32(-np.inf))
    return F32(x)


def adversarial_pairs(radius, origin, kmax, seed=0, per_kind=64, ulps=8):
    """pairs (a, b) (P, 3) f32 at distances within +-``ulps`` ulp of ``radius``: on-axis and corner-diagonal pairs, placed so that they
    straddle a voxel face (a just below a multiple of h, b beyond it) or sit anywhere in a voxel, at keys from 0 up to kmax.  The keys
    of some rows may fall outside [0, kmax]: the caller filters."""
    rng = np.random.default_rng(seed)
    r = F32(radius)
    h = leaf(r)
    o = np.asarray(origin, F32)
    A, B = [], []
    cells = np.concatenate([[0, 1, kmax - 1, kmax], rng.integers(0, kmax + 1, per_kind)]).astype(np.int64)
    dirs = [np.array(s, np.float64) for s in itertools.product((-1, 0, 1), repeat=3) if sum(abs(v) for v in s) in (1, 3)]
    for cell in cells:
        for n in range(-ulps, ulps + 1):
            d = dirs[int(rng.integers(len(dirs)))]
            length = np.float64(ulp_steps(r, n)) / np.sqrt((d * d).sum())
            base_cell = np.where(rng.random(3) < 0.5, cell, rng.integers(0, kmax + 1, 3)).astype(np.float64)
            for straddle in (True, False):
                frac = np.where(d != 0, (1.0 - 2.0 ** -rng.integers(1, 22, 3)) if straddle else rng.random(3), rng.random(3))
                frac = np.where(d < 0, 1.0 - frac, frac) if straddle else frac
                a = (o.astype(np.float64) + (base_cell + frac) * np.float64(h)).astype(F32)
                b = (a.astype(np.float64) + d * length).astype(F32)
                for t in range(-2, 3):                              # and the last bits of the far end itself
                    bb = b.copy()
                    ax = int(np.flatnonzero(d)[0])
                    bb[ax] = ulp_steps(bb[ax], t)
                    A.append(a)
                    B.append(bb)
    return np.asarray(A, F32), np.asarray(B, F32)


def surface_cloud(n=8192, seed=0, shift=(0.0, 0.0, 0.0)):
    """n points on a bumpy sheet over [0, 10]^2 with a little noise: the local geometry of a scanned surface"""
    rng = np.random.default_rng(seed)
    u, v = rng.random(n) * 10.0, rng.random(n) * 10.0
    z = np.sin(u) * np.cos(0.7 * v) + rng.normal(0.0, 0.02, n)
    return (np.stack([u, v, z], 1) + np.asarray(shift, np.float64)).astype(F32)


def noisy_scene(seed=11, n_noise=200, reach=1.5):
    """the denoising scene: cluster_oracle.cluttered_scene()'s clean 4,096-point aircraft scan plus ``n_noise`` points drawn (fixed seed,
    rejection sampling) inside the scan's bounding box inflated by 1 m, each with 1 to 3 clean points within ``reach`` and no other
    noise point within ``reach``; half of the noise before the clean rows, half behind them
    -> (scene (4096 + n_noise, 3) f32, clean rows, noise rows, clean (4096, 3) f32)"""
    import cluster_oracle as CO
    clean = CO.cluttered_scene()[3]
    rng = np.random.default_rng(seed)
    lo, hi = clean.min(0).astype(np.float64) - 1.0, clean.max(0).astype(np.float64) + 1.0
    r2 = F32(reach) * F32(reach)
    noise = np.zeros((0, 3), F32)
    for _ in range(64):                                             # (bounded: about six rounds are needed)
        cand = rng.uniform(lo, hi, size=(4096, 3)).astype(F32)
        near = (dist2(cand, clean) <= r2).sum(1)
        for c in cand[(near >= 1) & (near <= 3)]:
            if len(noise) < n_noise and not (dist2(c[None], noise) <= r2).any():
                noise = np.concatenate([noise, c[None]])
        if len(noise) == n_noise:
            break
    assert len(noise) == n_noise, "the rejection sampling did not find enough isolated points"
    half = n_noise // 2
    scene = np.concatenate([noise[:half], clean, noise[half:]]).astype(F32)
    rows = np.arange(half, half + len(clean))
    noise_rows = np.r_[np.arange(half), np.arange(half + len(clean), len(scene))]
    return scene, rows, noise_rows, clean
