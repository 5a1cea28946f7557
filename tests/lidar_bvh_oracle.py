"""NumPy specification of the LiDAR cast through the per-part trees (include/pointnet_hip.h, pn_lidar_cast_bvh): the admit rule of
a node operation for operation in np.float32, and the specified walk (labels ascending, depth first, the admitted child of
smaller entry first, a popped node tested again) over the nodes the C host builder returns (icp_bvh_oracle.build), with
tests/lidar_oracle._ray_triangle for the leaf tests and the (t, row) take rule.  It counts the triangles every ray tests and the
nodes whose box it tests.  The rays of a frame walk in lockstep, one step each per round; every ray's walk is its own, so the
result and the counts are those of walking the rays one by one.  Test infrastructure only; nothing in the package imports it."""
import numpy as np

import lidar_oracle as LO
from icp_bvh_oracle import LEAF, MAX_DEPTH

F32 = np.float32
K = F32(1.0) + F32(2.0 ** -18)


def reciprocals(d):
    """i = 1 / d per axis, one correctly rounded fp32 division (+-0 -> +-inf)"""
    with np.errstate(all="ignore"):
        return (F32(1) / np.asarray(d, F32)).astype(F32)


def admit(lo, hi, o, inv, t_min, bound):
    """the admit rule for boxes lo, hi (..., 3), the origin o (3,), reciprocals inv (..., 3) and bound = fmin(best, t_max) (...,),
    all f32, one rounded operation per line -> (admitted (...,) bool, tn (...,) f32)"""
    lo, hi, o, inv, bound = (np.asarray(x, F32) for x in (lo, hi, o, inv, bound))
    with np.errstate(all="ignore"):
        a = (lo - o) * inv
        b = (hi - o) * inv
        n, f = np.fmin(a, b), np.fmax(a, b)
        tn = np.fmax(np.fmax(n[..., 0], n[..., 1]), n[..., 2])
        tf = np.fmin(np.fmin(f[..., 0], f[..., 1]), f[..., 2]) * K
        return (tn <= tf) & (tn <= bound * K) & (tf >= F32(t_min)), tn


def _walk(o, d, tri, nodes, rows, roots, t_min, t_max):
    """one frame: rays d (n, 3) from o -> (hit (n,), t (n,), tests (n,), visits (n,))"""
    n = len(d)
    inv = reciprocals(d)
    lo, hi, first, count = nodes["lo"], nodes["hi"], nodes["first"].astype(np.int64), nodes["count"].astype(np.int64)
    with np.errstate(all="ignore"):
        H, Tm = LO._ray_triangle(o, d, tri, t_min, t_max, F32)           # the leaf tests look their (ray, row) up in here
    best, bj = np.full(n, np.inf, F32), np.full(n, -1, np.int64)
    tests, visits = np.zeros(n, np.int64), np.zeros(n, np.int64)
    tmax = F32(t_max)
    ok_of = lambda rays, nd: admit(lo[nd], hi[nd], o, inv[rays], t_min, np.fmin(best[rays], tmax))     # noqa: E731
    POP, DONE = -2, -1
    for root in roots:                                                  # the labels in ascending order, best carried across
        if root < 0:
            continue
        stack, sp = np.zeros((n, MAX_DEPTH), np.int64), np.zeros(n, np.int64)
        cur = np.full(n, int(root), np.int64)
        visits += 1
        cur[~ok_of(np.arange(n), cur)[0]] = DONE
        while True:
            live = np.flatnonzero(cur >= 0)
            if len(live) == 0:
                break
            leaf = count[cur[live]] > 0
            ii = live[~leaf]                                            # internal: both children against the best of this moment
            if len(ii):
                c0 = first[cur[ii]]
                assert (c0 > cur[ii]).all() and (c0 + 1 < len(nodes)).all()
                visits[ii] += 2
                (oa, ta), (ob, tb) = ok_of(ii, c0), ok_of(ii, c0 + 1)
                swap = ob & (~oa | (tb < ta))                           # enter the second child
                both = oa & ob
                assert (sp[ii[both]] < MAX_DEPTH).all()
                stack[ii[both], sp[ii[both]]] = np.where(swap, c0, c0 + 1)[both]
                sp[ii[both]] += 1
                cur[ii] = np.where(oa | ob, np.where(swap, c0 + 1, c0), POP)
            il = live[leaf]                                             # a leaf: its rows in order, the (t, row) take rule
            if len(il):
                f, c = first[cur[il]], count[cur[il]]
                assert (c <= LEAF).all()
                for k in range(LEAF):
                    m = k < c
                    rr, r = il[m], rows[f[m] + k].astype(np.int64)
                    t = Tm[rr, r]
                    take = H[rr, r] & ((t < best[rr]) | ((t == best[rr]) & (r < bj[rr])))
                    best[rr[take]], bj[rr[take]] = t[take], r[take]
                    tests[rr] += 1
                cur[il] = POP
            while True:                                                 # the next admitted node from the stack
                ip = np.flatnonzero(cur == POP)
                if len(ip) == 0:
                    break
                empty = sp[ip] == 0
                cur[ip[empty]] = DONE
                ip = ip[~empty]
                sp[ip] -= 1
                nd = stack[ip, sp[ip]]
                visits[ip] += 1
                cur[ip] = np.where(ok_of(ip, nd)[0], nd, POP)
    return np.where(bj >= 0, bj, -1).astype(np.int32), best, tests, visits


def cast(tri, poses, dirs, nodes, rows, roots, t_min=0.0, t_max=np.inf, chunk=1024):
    """lidar_oracle.cast through the trees -> (hit (B, R) int32, t (B, R) f32, tests (B, R): the triangles every ray was tested
    against, visits (B, R): the nodes whose box it tested)"""
    tri = np.asarray(tri, F32).reshape(-1, 3, 3)
    poses = np.asarray(poses, F32).reshape(-1, 4, 4)
    dirs = np.asarray(dirs, F32).reshape(-1, 3)
    B, R = len(poses), len(dirs)
    hit, tt = np.full((B, R), -1, np.int32), np.full((B, R), np.inf, F32)
    tests, visits = np.zeros((B, R), np.int64), np.zeros((B, R), np.int64)
    if len(tri) == 0:
        return hit, tt, tests, visits
    with np.errstate(all="ignore"):
        for b in range(B):
            o, d = LO._frame(poses[b], dirs, F32)
            for r0 in range(0, R, chunk):
                s = slice(r0, r0 + chunk)
                hit[b, s], tt[b, s], tests[b, s], visits[b, s] = _walk(o, d[s], tri, nodes, rows, roots, t_min, t_max)
    return hit, tt, tests, visits


def leaf_of_rows(nodes, rows):
    """the leaf node that holds every grouped row -> (T,) int"""
    out = np.full(len(rows), -1, np.int64)
    for n in np.flatnonzero(nodes["count"] > 0):
        out[rows[nodes["first"][n]:nodes["first"][n] + nodes["count"][n]]] = n
    assert (out >= 0).all()
    return out


def hits_not_admitted(tri, poses, dirs, nodes, rows, t_min=0.0, t_max=np.inf):
    """the condition the derivation rests on: every (ray, triangle) pair that hits in the brute-force oracle, with best set to
    that pair's t, against the box of the triangle's leaf -> (pairs checked, the (frame, ray, row) of those not admitted)"""
    tri = np.asarray(tri, F32).reshape(-1, 3, 3)
    poses = np.asarray(poses, F32).reshape(-1, 4, 4)
    dirs = np.asarray(dirs, F32).reshape(-1, 3)
    leaf = leaf_of_rows(nodes, rows)
    n_pairs, bad = 0, []
    with np.errstate(all="ignore"):
        for b in range(len(poses)):
            o, d = LO._frame(poses[b], dirs, F32)
            H, Tm = LO._ray_triangle(o, d, tri, t_min, t_max, F32)
            r, j = np.nonzero(H)
            nd = leaf[j]
            ok, _ = admit(nodes["lo"][nd], nodes["hi"][nd], o, reciprocals(d)[r], t_min, np.fmin(Tm[r, j], F32(t_max)))
            n_pairs += len(r)
            bad += [(b, int(x), int(y)) for x, y in zip(r[~ok], j[~ok])]
    return n_pairs, bad
