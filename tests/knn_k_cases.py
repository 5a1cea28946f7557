"""Input builders for the tests of every compile-time list length k of the radius search and its consumers (pn_radius_knn,
pn_scan_normals, pn_fpfh) and of pn_icp_normals -- TEST INFRASTRUCTURE, pure NumPy, nothing of the package is imported.

One cloud makes every unrolled insertion network do all of its work at every k = 0 .. 16: queries whose candidate count sits on
either side of k, ties across the list's last slot, and candidates that arrive when the list is already full and belong into each
of its slots.  tests/test_cpu_knn_k_cases.py checks on the oracles alone (tests/neighbors_oracle.py, tests/icp_plane_oracle.py)
that the inputs do what is said here; tests/test_gpu_knn_every_k.py runs them through the kernels.  Every builder is a pure
function of its seed.
"""
from __future__ import annotations

import functools

import numpy as np

import neighbors_oracle as NO

F32 = np.float32
RADIUS = 1.75
ORIGIN = (0.0, 0.0, 0.0)
SECOND_ORIGIN = (-0.37, -1.9, -0.6)      # below every point: the voxel faces move, the neighbours do not
MAX_K = NO.MAX_K
LATTICE_SIDE = 10
BLOB_SIZES = tuple(range(1, 19))         # counts 0 .. 17: k - 1, k and k + 1 for every k up to 16
BLOB_REACH = 0.8                         # every pair of a blob is closer than 1.6 < RADIUS
BLOB_PITCH = 8                           # leaves between the centres of two blobs: more than 7 leaves between their points
REPLICAS = 4


def k_edge_cloud(seed=0):
    """-> (xyz (N, 3) f32, RADIUS, ORIGIN), N = 1684 in shuffled row order:

    lattice   neighbors_oracle.lattice(10, seed): exact integer distances, 26 neighbours within 1.75 of an interior point in tie groups
              of 6 / 12 / 8 at d = 1 / 2 / 3; faces, edges and corners have 17 / 11 / 7
    blobs     m = 1 .. 18 points with real coordinates inside a ball of radius 0.8 round a voxel CORNER of the grid of leaf(RADIUS) at
              ORIGIN (the candidates of a query come from up to eight voxels), so every point of a blob has count m - 1; the blobs are
              more than 6 leaves from each other and from the lattice; four replicas (other points) at four heights"""
    rng = np.random.default_rng([seed, 0x6B4E4E])
    h = np.float64(NO.leaf(RADIUS))
    parts = [NO.lattice(LATTICE_SIDE, seed)[0].astype(np.float64)]
    first = int(np.ceil((LATTICE_SIDE - 1) / h)) + BLOB_PITCH                   # the lattice's last key + 1, then a pitch
    for rep in range(REPLICAS):
        for b, m in enumerate(BLOB_SIZES):
            corner = np.array([first + BLOB_PITCH * (b % 6), 2 + BLOB_PITCH * (b // 6), 2 + BLOB_PITCH * rep], np.float64) * h
            v = rng.normal(size=(m, 3))
            v *= (BLOB_REACH * rng.random((m, 1)) ** (1.0 / 3.0)) / np.linalg.norm(v, axis=1, keepdims=True)
            parts.append(corner + v)
    xyz = np.concatenate(parts).astype(F32)
    return xyz[rng.permutation(len(xyz))], RADIUS, ORIGIN


@functools.lru_cache(maxsize=4)
def _walk(xyz_bytes, origin):
    """what does not depend on k: per query the count and the sorted (d bits << 32 | row) keys of ALL its candidates (padded with the
    all-ones key), and per (query, candidate) pair `before` = the candidates of that query in voxels of strictly smaller key and `rank`
    = how many of those precede the candidate by (d bits, row)"""
    xyz = np.frombuffer(xyz_bytes, F32).reshape(-1, 3)
    N = len(xyz)
    r2 = F32(RADIUS) * F32(RADIUS)
    d = NO.dist2(xyz, xyz)
    ok = d <= r2
    ok[np.arange(N), np.arange(N)] = False
    count = ok.sum(1).astype(np.int32)
    key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(N, dtype=np.uint64)[None, :]
    empty = np.uint64(0xFFFFFFFFFFFFFFFF)
    width = int(count.max()) + 1
    ordered = np.sort(np.where(ok, key, empty), axis=1)[:, :width]
    kk = NO.keys(xyz, NO.leaf(RADIUS), origin).astype(np.int64)
    vox = (kk[:, 2] * NO.MAX_KEY + kk[:, 1]) * NO.MAX_KEY + kk[:, 0]             # the order candidates reach a lane in: z-major, x last
    query, before, rank = [], [], []
    for i in range(N):
        cand = np.flatnonzero(ok[i])
        earlier = vox[cand][None, :] < vox[cand][:, None]                        # [c, j]: j's voxel comes before c's
        nearer = key[i, cand][None, :] < key[i, cand][:, None]
        query.append(np.full(len(cand), i))
        before.append(earlier.sum(1))
        rank.append((earlier & nearer).sum(1))
    return dict(count=count, ordered=ordered, kk=kk, query=np.concatenate(query), before=np.concatenate(before), rank=np.concatenate(rank))


def k_edge_facts(xyz, k, origin=ORIGIN):
    """From neighbors_oracle alone, at list length k and RADIUS on the grid at ``origin``:

    count   (N,) the number of candidates of every query
    tie     (N,) bool, a boundary tie: the query has more than k candidates and its k-th and (k+1)-th smallest distances have equal
            bits, so only the row decides which of them holds the last slot
    late    (k,) per slot s the number of late insertions: candidates c with at least k candidates of the same query in voxels of
            strictly smaller key (the list is full when c arrives whatever the order inside a voxel is) that rank s among those and
            themselves by (d bits, row): the insertion network must carry c from the last slot down to slot s, or stop sooner only for
            members of c's own voxel
    keys    (N, 3) the per-axis voxel indices (float64 -> int64)"""
    w = _walk(np.ascontiguousarray(xyz, F32).tobytes(), tuple(float(v) for v in origin))
    N = len(w["count"])
    tie = np.zeros(N, bool)
    if k >= 1:
        more = w["count"] > k
        kth, nxt = w["ordered"][:, k - 1] >> np.uint64(32), w["ordered"][:, min(k, w["ordered"].shape[1] - 1)] >> np.uint64(32)
        tie = more & (kth == nxt)
    full = w["before"] >= k
    late = np.array([int((full & (w["rank"] == s)).sum()) for s in range(k)], np.int64)
    return dict(count=w["count"], tie=tie, late=late, keys=w["kk"])


def unit_normals(n, seed=0):
    """(n, 3) f32 seeded random unit vectors: the normals pn_fpfh is given on the case cloud"""
    v = np.random.default_rng([seed, 0xF9F4]).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


PART_SIZES = tuple(range(2, 18))         # for every K in 3 .. 16 a part of K - 1, of K and of K + 1 members
PLATE_GAP = 1e-3                         # (l1 - l0) / l2 of every neighbourhood's covariance: an eigenvector error of some 1e-13 in fp64


def plate_gap(x):
    """the least (l1 - l0) / l2 over the covariances of the K nearest members (the point included) of every point of the part ``x``,
    K = 3 .. min(len(x), 16): how far every neighbourhood is from a line, on which its normal would be anybody's"""
    x = np.asarray(x, F32).astype(np.float64)
    order = np.argsort(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1), axis=1, kind="stable")
    gap = np.inf
    for K in range(3, min(len(x), MAX_K) + 1):
        e = x[order[:, :K]]
        e = e - e.mean(1, keepdims=True)
        lam = np.linalg.eigvalsh(np.einsum("nki,nkj->nij", e, e) / K)
        gap = min(gap, float(((lam[:, 1] - lam[:, 0]) / lam[:, 2]).min()))
    return gap


def part_size_reference(seed=0):
    """-> (grouped xyz (152, 3) f32, seg (17,) int64, n_parts = 16): sixteen parts of 2, 3, .., 17 points laid out one behind the other
    (three waves of one lane per point, several labels in each).  Every part is a thin plate -- thickness 1e-3 of its extent -- tilted
    a little out of the x-y plane, a different tilt per part, and drawn again until no K nearest members of any point (K = 3 .. 16) are
    close to a line (PLATE_GAP): the least eigenvector is unambiguous and its z component leads"""
    rng = np.random.default_rng([seed, 0x9A127])
    pts = []
    for p, m in enumerate(PART_SIZES):
        while True:
            u, v = rng.uniform(0.0, 2.0, m), rng.uniform(0.0, 1.5, m)
            tx, ty = rng.uniform(-0.2, 0.2, 2)
            z = tx * u + ty * v + rng.uniform(-1e-3, 1e-3, m)
            plate = (np.stack([u, v, z], 1) + [5.0 * (p % 4), 4.0 * (p // 4), 0.5 * p]).astype(F32)
            if m < 3 or plate_gap(plate) > PLATE_GAP:
                break
        pts.append(plate)
    seg = np.concatenate([[0], np.cumsum(PART_SIZES)]).astype(np.int64)
    return np.concatenate(pts), seg, len(PART_SIZES)
