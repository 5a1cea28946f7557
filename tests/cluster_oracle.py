"""NumPy / pure-Python statement of pn_voxel_cluster's specification (include/pointnet_hip.h) -- TEST INFRASTRUCTURE.

keys   k = floor((p - origin) / leaf) per axis in float32 (that operand order), each in [0, 2^21)
ranks  the occupied voxels in ascending (kz, ky, kx): np.unique of the 63-bit key
graph  26-connectivity: max |dk| <= 1; 6-connectivity: sum |dk| = 1.  A neighbour is three integer coordinates, each checked against
       BOTH ends of [0, 2^21) before it is looked up: a key +- offset would make (kx = 2^21 - 1, ky = 0) and (kx = 0, ky = 1), whose
       keys differ by one, neighbours, which they are not
ids    a cluster's representative is its lowest voxel rank; ids 0 .. K-1 in ascending representative; sizes count points
"""
from __future__ import annotations

import itertools

import numpy as np

F32 = np.float32
KLIM = 1 << 21


def voxel_indices(xyz, leaf, origin):
    xyz = np.asarray(xyz, F32)
    leaf = np.broadcast_to(np.asarray(leaf, F32), (3,))
    origin = np.asarray(origin, F32)
    q = np.floor((xyz - origin) / leaf)
    assert np.isfinite(q).all(), "non-finite voxel index"
    k = q.astype(np.int64)
    assert (k >= 0).all() and (k < KLIM).all(), "voxel key out of range"
    return k


def offsets(connectivity):
    if connectivity == 26:
        return [d for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0)]
    if connectivity == 6:
        return [d for d in itertools.product((-1, 0, 1), repeat=3) if abs(d[0]) + abs(d[1]) + abs(d[2]) == 1]
    raise ValueError(f"connectivity must be 6 or 26, got {connectivity}")


def voxel_clusters(xyz, leaf, origin, connectivity=26):
    """-> (cluster (N,) i32, voxel (N,) i32, sizes (K,) i32, V, K)"""
    k = voxel_indices(xyz, leaf, origin)
    key = (k[:, 2] << 42) | (k[:, 1] << 21) | k[:, 0]
    ukey, voxel = np.unique(key, return_inverse=True)
    voxel = voxel.reshape(-1)
    V = len(ukey)
    coords = [(int(u & (KLIM - 1)), int((u >> 21) & (KLIM - 1)), int(u >> 42)) for u in ukey]          # (kx, ky, kz) by rank
    rank = {c: v for v, c in enumerate(coords)}
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    offs = offsets(connectivity)
    for v, (x, y, z) in enumerate(coords):
        for dx, dy, dz in offs:
            nx, ny, nz = x + dx, y + dy, z + dz
            if nx < 0 or ny < 0 or nz < 0 or nx >= KLIM or ny >= KLIM or nz >= KLIM:       # both ends, every axis
                continue
            w = rank.get((nx, ny, nz))
            if w is not None:
                a, b = find(v), find(w)
                if a != b:
                    parent[max(a, b)] = min(a, b)                                         # the root is the lowest rank
    root = np.array([find(v) for v in range(V)], np.int64)
    reps = np.flatnonzero(root == np.arange(V))                                            # ascending representatives
    cid = np.full(V, -1, np.int64)
    cid[reps] = np.arange(len(reps))
    vcl = cid[root]
    cluster = vcl[voxel].astype(np.int32)
    sizes = np.bincount(cluster, minlength=len(reps)).astype(np.int32)
    return cluster, voxel.astype(np.int32), sizes, V, len(reps)


def same_partition(a, b):
    """do two labelings of the same points describe one partition?"""
    a, b = np.asarray(a), np.asarray(b)
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def refines(fine, coarse):
    """is every cluster of ``fine`` inside one cluster of ``coarse``?"""
    pairs = set(zip(np.asarray(fine).tolist(), np.asarray(coarse).tolist()))
    return len(pairs) == len(set(np.asarray(fine).tolist()))


# ---- the cases the CPU and the GPU tests share: (xyz f32, leaf, origin) with coordinates k + 0.5, exact in fp32 for k < 2^21 ----
def centres(k):
    return (np.asarray(k, np.int64).astype(F32) + F32(0.5)).astype(F32)


def checkerboard():
    """the 108 voxel centres of a 6^3 grid with kx + ky + kz even: no two share a face, all touch by edges"""
    k = np.array([c for c in itertools.product(range(6), repeat=3) if sum(c) % 2 == 0], np.int64)
    return centres(k)


KMAX = KLIM - 1
WRAP_PAIRS = {                 # two voxels whose keys differ by one step of an axis although they sit at opposite ends of it
    "x": [(0, 1, 0), (KMAX, 0, 0)],
    "y": [(0, 0, 1), (0, KMAX, 0)],
    "z": [(0, 0, 0), (0, 0, KMAX)],          # key + 2^42 leaves the 63 bits: modulo 2^63 it is voxel 0
}


def wrap_pair(axis):
    return centres(np.array(WRAP_PAIRS[axis], np.int64))


def digit_boundary(lo):
    """the eight voxels kx, ky, kz in {lo, lo + 1} (lo = 255, 65535: across the radix sort's digit boundaries), two points each, and a
    ninth voxel two steps away"""
    k = np.array(list(itertools.product((lo, lo + 1), repeat=3)) * 2 + [(lo + 3, lo, lo)], np.int64)
    return centres(k)


def serpentine(n=4096, height=63):
    """n face-adjacent voxels in the plane ky = 3: columns along z at kx = 0, 2, 4, .. joined alternately at the top and the bottom.
    Ranks ascend with (kz, kx), so consecutive links of a column lie a whole z layer apart in rank: the long-path case for find"""
    path, c = [], 0
    while len(path) < n:
        zs = range(height) if c % 2 == 0 else range(height - 1, -1, -1)
        path += [(2 * c, 3, z) for z in zs]
        path.append((2 * c + 1, 3, height - 1 if c % 2 == 0 else 0))
        c += 1
    return centres(np.array(path[:n], np.int64))


def staircase(n=2000):
    """n voxels (i, i, i): adjacent only by corners"""
    i = np.arange(n, dtype=np.int64)
    return centres(np.stack([i, i, i], 1))


def random_grid(n=20000, side=24, seed=0):
    """n points over about half of the cells of a side^3 grid: multi-point voxels, many simultaneous hooks on shared roots"""
    rng = np.random.default_rng(seed)
    cells = np.flatnonzero(rng.random(side ** 3) < 0.5)
    pick = cells[rng.integers(0, len(cells), n)]
    k = np.stack([pick % side, (pick // side) % side, pick // (side * side)], 1)
    return (k.astype(F32) + rng.uniform(0.05, 0.95, size=(n, 3)).astype(F32)).astype(F32)


def cluttered_scene(seed=5):
    """the isolation scene: a 4,096-point scan of the test aircraft, 64 strays in [60,90] x [-20,20] x [30,50] and a 200-point blob
    (sigma 0.3) at (0, 0, -40); strays before, inside and after the aircraft rows -> (scene (4360, 3) f32, aircraft rows (4096,),
    blob rows (200,), clean scan (4096, 3) f32)"""
    import icp_mesh_oracle as MO
    v, f, p = MO.aircraft_mesh(0)
    clean, _ = MO.mesh_scan(v, f, p, 4096, noise=0.02)
    rng = np.random.default_rng(seed)
    strays = rng.uniform([60.0, -20.0, 30.0], [90.0, 20.0, 50.0], size=(64, 3)).astype(F32)
    blob = (rng.normal(0.0, 0.3, size=(200, 3)) + np.array([0.0, 0.0, -40.0])).astype(F32)
    parts = [("s", strays[:20]), ("a", clean[:2000]), ("s", strays[20:40]), ("b", blob), ("a", clean[2000:]), ("s", strays[40:])]
    scene = np.concatenate([x for _, x in parts]).astype(F32)
    tag = np.concatenate([np.full(len(x), t) for t, x in parts])
    return scene, np.flatnonzero(tag == "a"), np.flatnonzero(tag == "b"), clean
