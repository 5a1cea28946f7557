"""NumPy specification of the area-uniform surface sampler of the labelled part mesh (include/pointnet_hip.h, pn_mesh_sample):
integer weights from the fp64 areas, Philox4x32-10 bits, a stratified position in the cumulative weights with Python integers for
the 128-bit product, the folded barycentric point in np.float32.  Also the ops.global_pose composition with a score cloud, built
from the functions of tests/icp_global_oracle.py and tests/icp_mesh_oracle.py.  Test infrastructure only; nothing in the package
imports it."""
import functools

import numpy as np

import icp_global_oracle as GO
import icp_mesh_oracle as MO
import icp_oracle as IO

F32 = np.float32
U32 = np.uint32
U64 = np.uint64
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
ONE24 = 1 << 24


def philox4x32(counter, key):
    """Philox4x32-10: counter (..., 4) and key (2,) as unsigned 32-bit integers -> (..., 4) uint32, the outputs x0..x3"""
    c = np.asarray(counter).astype(U64) & U64(0xFFFFFFFF)
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    mask, s32 = U64(0xFFFFFFFF), U64(32)
    for _ in range(10):
        p0, p1 = U64(PHILOX_M0) * c0, U64(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ U64(k0), p1 & mask, (p0 >> s32) ^ c3 ^ U64(k1), p0 & mask
        k0, k1 = (k0 + PHILOX_W0) & 0xFFFFFFFF, (k1 + PHILOX_W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], -1).astype(U32)


def weights(area):
    """the integer weights of fp64 areas -> (T,) uint64: rint(area * 2^(24 - e)) with the largest finite positive area m * 2^e,
    m in [0.5, 1); 0 for an area that is not finite or not positive (and for every area when none is)"""
    a = np.asarray(area, np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(a) & (a > 0)
    if not ok.any():
        return np.zeros(len(a), U64)
    _, e = np.frexp(a[ok].max())
    w = np.rint(np.ldexp(np.where(ok, a, 0.0), 24 - int(e)))       # the scaling is exact, rint rounds ties to even
    return w.astype(U64)


def draw(area, n, seed=0, sets=1, set0=0):
    """the integer half of the specification -> (row (sets, n) int32, a (sets, n) int64, b (sets, n) int64): the grouped triangle
    row of every sample and its folded barycentric numerators (u = a / 2^24, v = b / 2^24); W = 0 -> (-1, 0, 0)"""
    w = weights(area)
    C = np.cumsum(w.astype(object)) if len(w) else np.zeros(0, object)
    W = int(C[-1]) if len(w) else 0
    row = np.full((sets, n), -1, np.int32)
    a = np.zeros((sets, n), np.int64)
    b = np.zeros((sets, n), np.int64)
    if W == 0:
        return row, a, b
    Cu = np.array([int(v) for v in C], U64)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    k = np.arange(n)
    for s in range(sets):
        ctr = np.stack([k, np.full(n, set0 + s), np.zeros(n, np.int64), np.zeros(n, np.int64)], -1)
        x = philox4x32(ctr, key)
        pos = np.empty(n, U64)
        for i in range(n):
            h = (int(x[i, 0]) << 32) | int(x[i, 1])
            f = (h * W) >> 64
            pos[i] = (i * W + f) // n
        row[s] = np.searchsorted(Cu, pos, side="right")             # the first i with C_i > pos
        aa, bb = (x[:, 2] >> U32(8)).astype(np.int64), (x[:, 3] >> U32(8)).astype(np.int64)
        fold = aa + bb > ONE24
        a[s], b[s] = np.where(fold, ONE24 - aa, aa), np.where(fold, ONE24 - bb, bb)
    return row, a, b


def points(tri, row, a, b):
    """the fp32 half: p = (A + u * (B - A)) + v * (C - A) per component, every operation rounded once; row < 0 -> NaN"""
    tri = np.asarray(tri, F32).reshape(-1, 3, 3)
    out = np.full(row.shape + (3,), np.nan, F32)
    ok = row >= 0
    if ok.any():
        t = tri[row[ok]]
        u = (a[ok].astype(F32) * F32(2.0 ** -24))[:, None]           # exact: a <= 2^24
        v = (b[ok].astype(F32) * F32(2.0 ** -24))[:, None]
        A, B, C = t[:, 0], t[:, 1], t[:, 2]
        out[ok] = (A + u * (B - A)) + v * (C - A)
    return out


def part_of(row, seg, n_parts):
    """the label whose [seg[l], seg[l + 1]) holds the row: the last l < n_parts with seg[l] <= row; -1 for row < 0"""
    seg = np.asarray(seg)
    lab = np.zeros(row.shape, np.int32)
    for l in range(1, n_parts):
        lab = np.where(seg[l] <= row, l, lab)
    return np.where(row >= 0, lab, -1).astype(np.int32)


def mesh_sample(tri, area, seg, n_parts, n, seed=0, sets=1, set0=0):
    """pn_mesh_sample -> (xyz (sets, n, 3) f32, part (sets, n) int32, row (sets, n) int32)"""
    row, a, b = draw(area, n, seed, sets, set0)
    return points(tri, row, a, b), part_of(row, seg, n_parts), row


def sample_reference(tri, area, seg, n_parts, normals, n, seed=0):
    """ops.mesh_sample_reference: set 0 as a grouped cloud -> (xyz (n, 3), seg (n_parts + 1,), row (n,), normals (n, 3))"""
    xyz, part, row = mesh_sample(tri, area, seg, n_parts, n, seed)
    cseg = np.searchsorted(part[0], np.arange(n_parts + 1), side="left")      # rows ascend, so the parts do
    return xyz[0], cseg, row[0], np.asarray(normals, F32)[row[0]]


# ---------------------------------------------------------------------------------------------------------------------
# global_pose with a score cloud
# ---------------------------------------------------------------------------------------------------------------------
def global_pose(scan, labels, mesh, n_parts, max_dist, score_cloud=None, rotations=None, top=4, stride=None, metric="point", **icp):
    """The ops.global_pose composition against a mesh = (tri, seg, normals, area).  ``score_cloud`` = (xyz, seg) of a grouped
    cloud: the coarse ranking runs against it; None: against the labelled vertices.  Seeds, refinement and the fine
    point-to-triangle selection are icp_global_oracle.global_pose's.  -> the same dict"""
    scan = np.asarray(scan, F32)
    B, N, _ = scan.shape
    tri, mseg, mnrm, area = mesh
    md = GO.max_d2_of(max_dist)
    rot = GO.rotation_grid(256) if rotations is None else rotations
    stride = max(1, N // 8192) if stride is None else stride
    if score_cloud is None:
        cloud, cseg = np.asarray(tri, F32).reshape(-1, 3), np.asarray(mseg) * 3
    else:
        cloud, cseg = np.asarray(score_cloud[0], F32), np.asarray(score_cloud[1])
    seeds = GO.seed_poses(GO.part_moments(scan, labels, n_parts), GO.ref_moments_mesh(tri, mseg, area, n_parts), rot)
    coarse, order = GO.score_poses(scan, labels, cloud, cseg, n_parts, seeds, stride, md)
    top = min(top, seeds.shape[1])
    pick = order[:, :top]
    out = dict(seeds=seeds, coarse=coarse, order=order, top=pick, refined=np.zeros((B, top, 4, 4)), fine=np.zeros((B, top)))
    res = [np.zeros((B, 4, 4)), np.zeros(B), np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)]
    out["winner"], out["cost"] = np.zeros(B, np.int32), np.zeros(B)
    for b in range(B):
        s, l = np.repeat(scan[b:b + 1], top, 0), np.repeat(labels[b:b + 1], top, 0)
        r = MO.icp(s, l, tri, mseg, n_parts, mnrm, seeds[b, pick[b]], metric=metric, max_d2=md, **icp)
        d2 = MO.correspond(s, l, tri, mseg, n_parts, r[0].astype(F32))[1]
        act = IO.active(s, l, mseg, n_parts)
        with np.errstate(invalid="ignore"):
            c = np.where(d2 <= md, d2, md).astype(np.float64)
        fine = np.where(act, c, 0.0).sum(1)
        w = int(np.argmin(fine))
        out["refined"][b], out["fine"][b] = r[0], fine
        for dst, src in zip(res, r):
            dst[b] = src[w]
        out["winner"][b], out["cost"][b] = pick[b, w], fine[w]
    out.update(pose=res[0], rmse=res[1], pairs=res[2], iters=res[3], status=res[4])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the shared case: the 80-triangle aircraft, 1,024-point one-sided scans, the score cloud of 2,048 samples (seed 7, set 0)
# ---------------------------------------------------------------------------------------------------------------------
NM = len(MO.MESH_PARTS)
SCORE_N, SCORE_SEED = 2048, 7
ONE_SIDED_SEEDS = (0, 1, 3, 4, 5, 6, 7)            # seed 2 ranks the closest seed fifth (rank 4) and is left out


@functools.lru_cache(maxsize=None)
def aircraft(level=0):
    """(tri, seg, normals, area) of the grouped procedural aircraft"""
    v, f, p = MO.aircraft_mesh(level)
    tri, seg, _, nrm, area = MO.group_mesh(v, f, p, NM)
    return tri, seg, nrm, area


@functools.lru_cache(maxsize=None)
def score_cloud(level=0):
    tri, seg, nrm, area = aircraft(level)
    xyz, cseg, _, _ = sample_reference(tri, area, seg, NM, nrm, SCORE_N, SCORE_SEED)
    return xyz, cseg


@functools.lru_cache(maxsize=None)
def one_sided_case(seed):
    """-> (scan (1024, 3) f32, labels (1024,) int32, true pose): a scan of the level-0 aircraft under icp_global_oracle.true_pose,
    5 cm noise; the points whose model-frame y is at most -1 m carry label -1"""
    v, f, p = MO.aircraft_mesh(0)
    T = GO.true_pose(seed)
    scan, lab = MO.mesh_scan(v, f, p, 1024, pose=T, noise=0.05, seed=seed)
    model = (scan.astype(np.float64) - T[:3, 3]) @ T[:3, :3]
    return scan, np.where(model[:, 1] <= -1.0, -1, lab).astype(np.int32), T


def closest_seed_rank(seed, cloud):
    """the rank, in the coarse order of rotation_grid(256) + the centroid fit at stride 4 and 3 m, of the seed whose rotation is
    closest to the truth; ``cloud`` = (xyz, seg)"""
    tri, seg, _, area = aircraft(0)
    scan, lab, T = one_sided_case(seed)
    seeds = GO.seed_poses(GO.part_moments(scan[None], lab[None], NM), GO.ref_moments_mesh(tri, seg, area, NM), GO.rotation_grid(256))
    _, order = GO.score_poses(scan[None], lab[None], cloud[0], cloud[1], NM, seeds, GO.PARAMS["stride"], GO.max_d2_of(GO.MAX_DIST))
    ang = [IO.rotation_angle(P[:3, :3], T[:3, :3]) for P in seeds[0]]
    return int(np.flatnonzero(order[0] == int(np.argmin(ang)))[0])


@functools.lru_cache(maxsize=None)
def solved(seed, with_cloud):
    """the oracle pipeline on a one-sided case, computed once"""
    scan, lab, _ = one_sided_case(seed)
    return global_pose(scan[None], lab[None], aircraft(0), NM, GO.MAX_DIST, score_cloud=score_cloud(0) if with_cloud else None,
                       rotations=GO.rotation_grid(256), **GO.PARAMS)
