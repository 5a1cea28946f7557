"""NumPy specification of the grid search of a cloud reference (include/pointnet_hip.h, pn_icp_grid_build and the rules below it):
tests/icp_oracle.correspond plus the (-1, +inf, NaN) rule beyond the tables' r2, and a restatement of the key and clamp rules (the
leaf, a query's key, which queries are searched, which rows and x range a query walks) with a walk that follows them literally.
Test infrastructure only; nothing in the package imports it."""
import numpy as np

import icp_oracle as IO

F32 = np.float32
MAX_KEY = 1 << 14


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def leaf(r2):
    """h = sqrt(r2) (1 + 2^-6), root and product in fp64, rounded UP to fp32"""
    exact = np.sqrt(np.float64(F32(r2))) * (1.0 + 1.0 / 64.0)
    h = F32(exact)
    return np.nextafter(h, F32(np.inf)) if np.float64(h) < exact else h


def keys(u, origin, h):
    """F = floor(fl(fl(u - o) / h)) per axis, fp32 (a float array: it may be -1, MAX_KEY, far outside or not a number)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.floor(((np.asarray(u, F32) - np.asarray(origin, F32)).astype(F32) / F32(h)).astype(F32))


def searched(F):
    """the out-of-box rule: a query is searched iff -1 <= F <= MAX_KEY on every axis (false for a NaN)"""
    with np.errstate(invalid="ignore"):
        return ((F >= -1) & (F <= MAX_KEY)).all(-1)


def rows_of(k):
    """the clamp rule for the voxel k = (kx, ky, kz), each in [-1, MAX_KEY]: the (nz, ny, x0, x1) rows it walks, in walking order"""
    kx, ky, kz = (int(v) for v in k)
    x0, x1 = max(kx - 1, 0), min(kx + 1, MAX_KEY - 1)
    out = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            nz, ny = kz + dz, ky + dy
            if 0 <= nz < MAX_KEY and 0 <= ny < MAX_KEY:
                out.append((nz, ny, x0, x1))
    return out


def correspond(scan, labels, ref, seg, n_parts, pose32, r2, max_d2=None):
    """the contract: the brute-force pairs with d2 <= r2, nothing beyond -> idx (cut at max_d2, default r2), d2, q (B, N, 3)"""
    max_d2 = F32(r2) if max_d2 is None else F32(max_d2)
    assert max_d2 <= F32(r2)
    bi, bd = IO.correspond(scan, labels, ref, seg, n_parts, pose32)
    near = (bi >= 0) & (bd <= F32(r2))
    idx = np.where(near & (bd <= max_d2), bi, -1).astype(np.int32)
    d2 = np.where(near, bd, F32(np.inf)).astype(F32)
    q = np.where(near[..., None], ref[np.clip(bi, 0, None)], F32(np.nan)).astype(F32)
    return idx, d2, q


def walk(scan, labels, ref, seg, n_parts, pose32, r2, origin, trace=None):
    """the search as the header states it, one query at a time over a dictionary of voxels: the key rule, the out-of-box rule, the
    clamp rule, the label mask, d2 <= r2 and (bits of d2, row) as the order -> idx (not cut by a max_d2), d2.  ``trace`` (a list)
    receives (b, i, key, [(voxel, rows visited)]) per searched query."""
    scan = np.asarray(scan, F32)
    h = leaf(r2)
    rk = keys(ref, origin, h)
    assert ((rk >= 0) & (rk < MAX_KEY)).all(), "a reference key is outside the box"
    vox = {}
    for j, k in enumerate(rk.astype(np.int64)):
        vox.setdefault((int(k[2]), int(k[1]), int(k[0])), []).append(j)
    B, N, _ = scan.shape
    idx = np.full((B, N), -1, np.int32)
    d2 = np.full((B, N), np.inf, F32)
    act = IO.active(scan, labels, seg, n_parts)
    r2b = int(_bits(F32(r2))[0])
    for b in range(B):
        u = IO.to_model_frame(scan[b], np.asarray(pose32[b], F32))
        F = keys(u, origin, h)
        go = searched(F) & act[b]
        for i in np.flatnonzero(go):
            s0, s1 = seg[labels[b, i]], seg[labels[b, i] + 1]
            best, bj, seen = int(IO.EMPTY), -1, []
            for nz, ny, x0, x1 in rows_of(F[i]):
                for nx in range(x0, x1 + 1):
                    cand = vox.get((nz, ny, nx), ())
                    if cand:
                        seen.append(((nx, ny, nz), list(cand)))
                    for j in cand:
                        e = u[i] - ref[j]
                        d = int(_bits(F32(F32(e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]))[0])
                        if s0 <= j < s1 and d <= r2b and (d < best or (d == best and j < bj)):
                            best, bj = d, j
            if bj >= 0:
                idx[b, i], d2[b, i] = bj, np.array([best], np.uint32).view(F32)[0]
            if trace is not None:
                trace.append((b, int(i), tuple(int(v) for v in F[i]), seen))
    return idx, d2


# ---- the single-pass cases tests/test_cpu_icp_grid.py (on the oracle alone) and tests/test_gpu_icp_grid.py (on the device) share.
# A case: scan (B, N, 3), lab (B, N), ref (M, 3) grouped, seg, n_parts, pose (B, 4, 4) fp64, r2 (the tables'), max_d2 (the cuts to
# run, each <= r2), origin (None: the reference's per-axis minimum, as ops builds it).
def _case(scan, lab, ref, seg, n_parts, pose, r2, max_d2, origin=None):
    scan, lab = np.asarray(scan, F32), np.asarray(lab, np.int32)
    if scan.ndim == 2:
        scan, lab = scan[None], lab[None]
    pose = np.broadcast_to(np.eye(4), (scan.shape[0], 4, 4)).copy() if pose is None else np.asarray(pose, np.float64)
    ref = np.ascontiguousarray(ref, F32)
    origin = ref.min(0) if origin is None else np.asarray(origin, F32)
    return dict(scan=scan, lab=lab, ref=ref, seg=np.asarray(seg, np.int64), n_parts=n_parts, pose=pose, r2=F32(r2),
                max_d2=[F32(m) for m in max_d2], origin=origin.astype(F32))


def spoil(rng, scan, lab, n_parts):
    """tests/test_gpu_icp_bvh.py's: labels -1 and out of range, a label whose segment is empty, NaN and inf points"""
    k = rng.choice(scan.shape[0], 40, replace=False)
    lab[k[:8]] = -1
    lab[k[8:14]] = n_parts + 3
    lab[k[14:22]] = n_parts - 1
    scan[k[22:27]] = np.nan
    scan[k[27], 2] = np.inf
    scan[k[28], 0] = -np.inf


def pose_near(rng, true, rot=0.05, shift=0.3):
    P = np.array(true, np.float64)
    P[:3, :3] = IO.rot(rng.normal(size=3), rot) @ P[:3, :3]
    P[:3, 3] += rng.normal(size=3) * shift
    return P


def case_random():
    """B = 2, N = 300 (a full block and a 44-lane tail), M = 2,000 over 5 labels, the last one empty; the scan spoiled"""
    rng = np.random.default_rng(7)
    n_parts, B, N = 5, 2, 300
    ref, seg, _ = IO.group_reference(rng.uniform(-5, 5, (2000, 3)), rng.integers(0, n_parts - 1, 2000), n_parts)
    scan = rng.uniform(-5.5, 5.5, (B, N, 3)).astype(F32)
    lab = rng.integers(0, n_parts - 1, (B, N)).astype(np.int32)
    for b in range(B):
        spoil(rng, scan[b], lab[b], n_parts)
    pose = np.stack([pose_near(rng, np.eye(4), rot=0.2, shift=0.5) for _ in range(B)])
    return _case(scan, lab, ref, seg, n_parts, pose, F32(0.7) * F32(0.7), [F32(0.7) * F32(0.7), 0.25])


TIES_C = F32(2.03125)                  # two leaves of r2 = 1 (h = 1.015625): a corner shared by eight voxels
TIES_DUP = np.array([6.125, 6.25, 6.375], F32)


def case_ties():
    """r2 = 1, origin 0, identity pose.  Label 0: the eight points c +- 1/2 around the voxel corner c, all at d2 = 0.75 from it in
    eight different voxels, the one in the voxel visited LAST first (row 0); then three copies of one point.  Label 1: a point 0.05
    from c, and two more copies of the duplicated point.  Queries: c with label 0 (row 0 must win, not the nearer label-1 point), c
    with label 1, the duplicated point and one 0.125 off it with either label (the lowest row of the label wins), and as many
    queries with nothing within r2."""
    c = TIES_C
    lattice = [(+1, +1, +1)] + [(sx, sy, sz) for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1) if (sx, sy, sz) != (1, 1, 1)]
    l0 = [c + F32(0.5) * np.array(s, F32) for s in lattice] + [TIES_DUP] * 3
    l1 = [np.array([c + F32(0.05), c, c], F32)] + [TIES_DUP] * 2
    ref = np.array(l0 + l1, F32)
    cc = np.array([c, c, c], F32)
    off = TIES_DUP + np.array([0.125, 0, 0], F32)
    q = [cc, cc, TIES_DUP, TIES_DUP, off, off]
    ql = [0, 1, 0, 1, 0, 1]
    for k in range(6):                                                   # nothing within 1 of these (inside the box)
        q.append(np.array([10.5 + k, 2.0, 9.0], F32))
        ql.append(k % 2)
    return _case(np.array(q, F32), ql, ref, [0, len(l0), len(ref)], 2, None, 1.0, [1.0], origin=(0, 0, 0))


RADIUS_STEP = F32(2.0 ** -11)          # 1.5^2 + (2^-11)^2 = 2.25 + 2^-22: one ulp above 2.25


def case_radius(r2):
    """pairs at d2 = 2.25 exactly and one ulp above it, across voxel faces and inside a voxel; queries one ulp either side of a
    voxel face on every axis with reference points a metre away on both sides; queries with nothing near.  Run with the tables'
    r2 = 2.25 (cuts 2.25 and 1) and r2 = 4 (cut 2.25: max_d2 below the tables')."""
    h = leaf(r2)
    ref, q = [], []
    for i in range(6):
        base = np.array([5.0 * i + 0.25 + i / 64.0, 3.0 + 0.7 * i + 1 / 64.0, 2.0 + i / 32.0], F32)
        if i == 0:                                                        # this pair stays inside one voxel: x in [3 h + 1/128, 4 h)
            base = np.array([F32(3) * h + F32(1 / 128), 20.0 + 1 / 64.0, 2.0], F32)
        ref.append(base)
        q.append(base + np.array([1.5, 0, 0], F32))
        q.append(base + np.array([1.5, RADIUS_STEP, 0], F32))
    for axis in range(3):
        for k, side in ((3, -np.inf), (4, np.inf)):
            f = F32(k) * h
            p = np.array([40.0, 40.0, 40.0], F32) + F32(10.0) * np.arange(3, dtype=F32) * F32(axis + 1)
            p[axis] = np.nextafter(f, F32(side))
            q.append(p.copy())
            for d in (-1.0, 1.0):
                r = p.copy()
                r[axis] = f + F32(d)
                ref.append(r)
    for k in range(8):
        q.append(np.array([100.0 + 3 * k, 50.0, 20.0 + k], F32))
    ref.append(np.array([0, 0, 0], F32))                                  # the origin's corner
    ref = np.array(ref, F32)
    cuts = [2.25, 1.0] if F32(r2) == F32(2.25) else [2.25]
    return _case(np.array(q, F32), np.zeros(len(q), np.int32), ref, [0, len(ref)], 1, None, r2, cuts, origin=(0, 0, 0))


BOX_ORIGIN = np.array([-3.0, 7.0, 100.0], F32)


def case_box():
    """r2 = 1, an explicit origin, reference keys 0 and MAX_KEY - 1 on every axis (and both corners of the box).  Queries at keys -1
    and MAX_KEY within the radius of those points (they must find them), two voxels out and 10^6 m out (they must not)."""
    h = np.float64(leaf(1.0))
    mid = 8000
    kk, moves = [], []
    for a in range(3):
        for edge, sgn in ((0, -1.0), (MAX_KEY - 1, 1.0)):
            k = [mid, mid + 3, mid - 5]
            k[a] = edge
            kk.append(k)
            m = np.zeros(3)
            m[a] = sgn * (0.5 * h + 0.3)
            moves.append(m)
    kk += [[0, 0, 0], [MAX_KEY - 1] * 3]
    moves += [np.full(3, -(0.5 * h + 0.05)), np.full(3, 0.5 * h + 0.05)]
    ref = (BOX_ORIGIN.astype(np.float64) + (np.array(kk) + 0.5) * h).astype(F32)
    q = [(ref[j].astype(np.float64) + moves[j]).astype(F32) for j in range(len(ref))]
    for a in range(3):
        two = np.zeros(3)
        two[a] = -(0.5 * h + 1.3)
        q.append((ref[2 * a].astype(np.float64) + two).astype(F32))
        far = np.zeros(3)
        far[a] = 1e6 if a != 1 else -1e6
        q.append((ref[2 * a + 1].astype(np.float64) + far).astype(F32))
    q.append((ref[6].astype(np.float64) - 2.5 * h).astype(F32))
    q.append((ref[7].astype(np.float64) + 2.5 * h).astype(F32))
    return _case(np.array(q, F32), np.zeros(len(q), np.int32), ref, [0, len(ref)], 1, None, 1.0, [1.0], origin=BOX_ORIGIN)


def case_m1():
    rng = np.random.default_rng(21)
    scan = (np.array([1.0, 2.0, 3.0]) + rng.normal(0, 0.75, (70, 3))).astype(F32)
    return _case(scan, np.zeros(70, np.int32), np.array([[1.0, 2.0, 3.0]], F32), [0, 1], 1, None, 1.0, [1.0, 0.3])


def case_m40():
    rng = np.random.default_rng(22)
    ref, seg, _ = IO.group_reference(rng.uniform(0, 3, (40, 3)), rng.integers(0, 2, 40), 2)
    scan = rng.uniform(-0.5, 3.5, (100, 3)).astype(F32)
    return _case(scan, rng.integers(0, 2, 100), ref, seg, 2, [pose_near(rng, np.eye(4), 0.1, 0.1)], F32(0.36), [F32(0.36)])


def case_one_voxel():
    rng = np.random.default_rng(23)
    ref = rng.uniform(0.05, 0.95, (500, 3)).astype(F32)
    scan = rng.uniform(-1.5, 2.5, (100, 3)).astype(F32)
    return _case(scan, np.zeros(100, np.int32), ref, [0, 500], 1, None, 1.0, [1.0], origin=(0, 0, 0))


def case_n1():
    """B = 2, N = 1: one query with a partner, one without"""
    c = case_m40()
    scan = np.stack([c["ref"][:1] + F32(0.01), c["ref"][:1] + F32(30.0)])
    return _case(scan, np.zeros((2, 1), np.int32), c["ref"], c["seg"], 2, None, c["r2"], c["max_d2"])


CASES = {"random": case_random, "ties": case_ties, "radius": lambda: case_radius(2.25), "radius_below": lambda: case_radius(4.0),
         "box": case_box, "m1": case_m1, "m40": case_m40, "one_voxel": case_one_voxel, "n1": case_n1}
_CACHE = {}


def case(name):
    """a case and its expected search (the contract's, cut at r2), computed once and shared"""
    if name not in _CACHE:
        c = CASES[name]()
        c["expect"] = correspond(c["scan"], c["lab"], c["ref"], c["seg"], c["n_parts"], c["pose"].astype(F32), c["r2"])
        _CACHE[name] = c
    return _CACHE[name]
