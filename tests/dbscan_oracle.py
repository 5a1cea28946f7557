"""NumPy statement of pn_dbscan's specification (include/pointnet_hip.h) and the fixtures its tests share -- TEST INFRASTRUCTURE.

neighbours  pn_radius_knn's: { j != i : d(i, j) <= r2 }, r2 = eps * eps in float32, d = neighbors_oracle.dist2 (float32, the specified
            operand order), j != i by row.  Brute force over all pairs, in row chunks: the grid is the library's business
core        |N(i)| + 1 >= min_points
clusters    connected components of the core rows with an edge where d <= r2 (union-find, the larger root under the smaller, so a
            root is its component's lowest core ROW); ids 0 .. K-1 in ascending representative
border      a row that is not core joins the cluster of its core neighbour with the lowest (bit pattern of d, row); otherwise -1
"""
from __future__ import annotations

import numpy as np

import cluster_oracle as CO
import neighbors_oracle as NO

F32 = np.float32
MAX_MIN_POINTS = 1 << 30


def dbscan(xyz, eps, min_points, chunk=512):
    """-> (cluster (N,) i32, sizes (K,) i32, core (N,) bool, count (N,) i32: |N(i)|)"""
    xyz = np.ascontiguousarray(xyz, F32)
    N = len(xyz)
    assert 1 <= min_points <= MAX_MIN_POINTS
    r2 = F32(eps) * F32(eps)
    count = np.zeros(N, np.int64)

    def chunks():
        with np.errstate(invalid="ignore", over="ignore"):
            for s in range(0, N, chunk):
                e = min(s + chunk, N)
                d = NO.dist2(xyz[s:e], xyz)
                ok = d <= r2                                       # False for a NaN
                ok[np.arange(e - s), np.arange(s, e)] = False      # j != i by row
                yield s, ok, d

    for s, ok, _ in chunks():
        count[s:s + len(ok)] = ok.sum(1)
    core = count + 1 >= min_points
    parent = np.arange(N)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    cluster = np.full(N, -1, np.int64)
    border = []                                                    # (row, its best core neighbour)
    for s, ok, d in chunks():                                      # (formed again: all pairs at once would not fit)
        for i in range(ok.shape[0]):
            js = np.flatnonzero(ok[i] & core)
            if core[s + i]:
                for j in js[js < s + i]:                           # every pair once, from its higher end
                    a, b = find(s + i), find(j)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
            elif len(js):
                key = (d[i, js].view(np.uint32).astype(np.uint64) << np.uint64(32)) | js.astype(np.uint64)
                border.append((s + i, int(js[np.argmin(key)])))
    root = np.array([find(i) if core[i] else -1 for i in range(N)], np.int64)
    reps = np.flatnonzero(root == np.arange(N))                    # ascending lowest core rows
    cid = np.full(N, -1, np.int64)
    cid[reps] = np.arange(len(reps))
    cluster[core] = cid[root[core]]
    for i, j in border:
        cluster[i] = cid[root[j]]
    sizes = np.bincount(cluster[cluster >= 0], minlength=len(reps)).astype(np.int32)
    return cluster.astype(np.int32), sizes, core, count.astype(np.int32)


# ---- fixtures the CPU and the GPU tests share -----------------------------------------------------------------------
BRIDGE_EPS, BRIDGE_MIN_POINTS = 1.0, 4
_cache = {}


def bridge_scene():
    """the acceptance scene: the clean 4,096-point aircraft scan of cluster_oracle.cluttered_scene(), a 600-point blob (sigma 0.5) 12 m
    off its nose (the row of largest x) and 19 single points every 0.6 m between them; bridge rows before and after, the blob
    inside the aircraft rows -> (scene (4715, 3) f32, aircraft rows (4096,), blob rows (600,), bridge rows (19,), clean (4096, 3) f32)"""
    if "bridge" not in _cache:
        clean = CO.cluttered_scene()[3]
        c = clean[np.argmax(clean[:, 0])].astype(np.float64)
        rng = np.random.default_rng(3)
        blob = (rng.normal(0, 0.5, (600, 3)) + c + np.array([12.0, 0.0, 0.0])).astype(F32)
        t = 0.6 * np.arange(1, 20)
        bridge = (c[None, :] + t[:, None] * np.array([1.0, 0.0, 0.0])).astype(F32)
        parts = [("s", bridge[:5]), ("a", clean[:2000]), ("b", blob), ("a", clean[2000:]), ("s", bridge[5:])]
        scene = np.concatenate([x for _, x in parts]).astype(F32)
        tag = np.concatenate([np.full(len(x), k) for k, x in parts])
        _cache["bridge"] = (scene, np.flatnonzero(tag == "a"), np.flatnonzero(tag == "b"), np.flatnonzero(tag == "s"), clean)
    return _cache["bridge"]


def bridge_expected():
    """the oracle's result on the bridge scene at (BRIDGE_EPS, BRIDGE_MIN_POINTS), computed once"""
    if "bridge_exp" not in _cache:
        _cache["bridge_exp"] = dbscan(bridge_scene()[0], BRIDGE_EPS, BRIDGE_MIN_POINTS)
    return _cache["bridge_exp"]


TIE_ORDERS = {                 # [a, a's two helpers, b, b's two helpers, mid] in three row orders; each gives clusters [0,0,0,0,1,1,1]
    "a_first": [0, 1, 2, 6, 3, 4, 5],
    "b_first": [3, 4, 5, 6, 0, 1, 2],
    "mid_first": [6, 1, 0, 2, 4, 3, 5],
}


def border_tie(order):
    """seven points: a = (-1,0,0) with two helpers at (-2,0,0), b = (1,0,0) with two helpers at (2,0,0), mid = (0,0,0).  With eps = 1,
    min_points = 4 only a and b are core (3 neighbours each), the helpers are border, and mid is at exactly d = 1 from both cores: it
    follows the core of lower row -> (xyz (7, 3) f32, expected cluster (7,), expected sizes)"""
    base = np.array([[-1, 0, 0], [-2, 0, 0], [-2, 0, 0], [1, 0, 0], [2, 0, 0], [2, 0, 0], [0, 0, 0]], F32)
    perm = np.array(TIE_ORDERS[order])
    x = base[perm]
    side = np.array([0, 0, 0, 1, 1, 1, -1])[perm]                    # 0: a's, 1: b's, -1: mid
    row_a, row_b = int(np.flatnonzero(perm == 0)[0]), int(np.flatnonzero(perm == 3)[0])
    first = 0 if row_a < row_b else 1                                # the side whose core has the lower row: cluster 0, and mid's
    cluster = np.where(side == -1, 0, np.where(side == first, 0, 1)).astype(np.int32)
    sizes = np.array([4, 3], np.int32)
    return x, cluster, sizes


def unit_lattice(side=6, seed=2):
    """the side^3 points of the unit integer lattice in shuffled row order (neighbors_oracle.lattice)"""
    return NO.lattice(side, seed)[0]


def below_one():
    """the float32 one ulp below 1"""
    return float(np.nextafter(F32(1.0), F32(0.0)))


def adversarial_cloud(eps=0.37, origin=(-3.0, 2.0, 0.5), kmax=400, seed=4, per_kind=40):
    """neighbors_oracle.adversarial_pairs at +-8 ulp of eps, both ends of every pair, filtered to the key range [0, 2^14) of the grid
    at ``origin`` -> (xyz (2P, 3) f32, eps, origin)"""
    a, b = NO.adversarial_pairs(eps, origin, kmax, seed=seed, per_kind=per_kind)
    a, b = a[2::5], b[2::5]                                          # one far end per near end (the five differ by an ulp: they would join each other)
    h = NO.leaf(eps)
    ok = np.ones(len(a), bool)
    for p in (a, b):
        k = NO.keys(p, h, origin)
        ok &= ((k >= 0) & (k < NO.MAX_KEY)).all(1)
    x = np.concatenate([a[ok], b[ok]]).astype(F32)
    return x, eps, origin


def shuffled(x, seed):
    return np.ascontiguousarray(x[np.random.default_rng(seed).permutation(len(x))])
