"""pn_icp_information, pn_pose_graph_optimize and ops.multiway_register on the MI355X: the information pass between guard bands
against pn_icp_correspond (bit for bit) and the NumPy oracle (tests/pose_graph_oracle.py) on the cases of tests/gicp_cases.py, the
grid against the plain reference, determinism (eager, graph replay, a batch against the single scans); the graph solve against the
oracle at the smallest graphs at which it can go wrong, to a tolerance measured on the oracle itself; its guarded paths (a node
without a live edge, an edge index out of range); and four surface samplings of the aircraft mesh registered end to end."""
import ctypes as C

import numpy as np
import pytest
import torch

import gicp_cases as GC
import icp_mesh_oracle as MO
import icp_oracle as IO
import pose_graph_oracle as PG

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 4096
PAT = 0xA5
NP = GC.NP
NM = len(MO.MESH_PARTS)


def _guarded(shape, dtype, dev):
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((GUARD + n + GUARD,), PAT, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + n].view(dtype).view(*shape)


def _intact(buf):
    return bool((buf[:GUARD] == PAT).all()) and bool((buf[-GUARD:] == PAT).all())


def _seg_c(seg):
    return (C.c_int32 * len(seg))(*[int(v) for v in seg])


def _t(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)            # (a copy: the shared case arrays are read-only)


def _bytes_equal(a, b):
    return all(np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8)) for x, y in zip(a, b))


# ---- pn_icp_information ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", [(1, 1), (1, 777), (3, 5000)])
def test_information_against_correspond_and_oracle(dev, B, N):
    """(1, 1) is one lane, (1, 777) has a partial last block, (3, 5000) a batch and a ragged tail"""
    from pointcloudprocessing_amd import _lib, ops
    c = GC.sums_case(B, N)
    M = len(c["ref"])
    ins = [_t(a, dev) for a in (c["scan"], c["lab"], c["ref"], c["pose"].astype(F32))]
    keep = [x.clone() for x in ins]
    nbytes = _lib.lib().pn_icp_information_workspace_bytes(B, N, M, NP)
    bufs = dict(idx=_guarded((B, N), torch.int32, dev), d2=_guarded((B, N), torch.float32, dev), sums=_guarded((B, 29), torch.float64, dev),
                ws=_guarded((nbytes,), torch.uint8, dev))
    p = lambda k: C.c_void_p(bufs[k][1].data_ptr())                                   # noqa: E731
    r = ops.IcpReference(ins[2], c["seg"], torch.arange(M, device=dev), NP)
    for max_d2 in GC.MAX_D2:
        rc = _lib.lib().pn_icp_information(_lib.ptr(ins[0]), _lib.ptr(ins[1]), B, N, _lib.ptr(ins[2]), _seg_c(c["seg"]), M, NP, _lib.ptr(ins[3]),
                                           max_d2, p("idx"), p("d2"), p("sums"), p("ws"), nbytes, None, 0.0, _lib.current_stream())
        _lib.check(rc, "pn_icp_information")
        torch.cuda.synchronize()
        for name, (buf, _) in bufs.items():
            assert _intact(buf), f"{name}: guard band overwritten"
        for a, b in zip(keep, ins):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "an input was modified"
        ci, cd = ops.icp_correspond(ins[0], ins[1], r, ins[3], max_dist=float(np.sqrt(max_d2)))
        idx, d2, S = bufs["idx"][1].cpu().numpy(), bufs["d2"][1].cpu().numpy(), bufs["sums"][1].cpu().numpy()
        assert np.array_equal(idx, ci.cpu().numpy()) and np.array_equal(d2.view(np.uint32), cd.cpu().numpy().view(np.uint32))
        worst = 0.0
        for b in range(B):
            kept = idx[b] >= 0
            exp, mag = PG.information(c["ref"][idx[b][kept]], d2[b][kept])
            assert S[b, 0] == kept.sum() == exp[0]
            assert np.all(S[b, 22:28] == 0.0) and not np.signbit(S[b, 22:28]).any()
            err = np.abs(S[b] - exp)
            assert np.all(err[1:22] <= 1e-12 * mag[1:22]) and err[28] <= 1e-12 * mag[28], (b, err, mag)
            worst = max(worst, float((err / np.maximum(mag, 1e-300)).max()))
        print(f"B={B} N={N} max_d2={max_d2}: kept {S[:, 0].astype(int).tolist()}, worst error {worst:.3g} of the magnitudes")
        if N >= 777:
            assert (S[:, 0] > 0).all()


def _refs(dev, max_dist=2.0):
    from pointcloudprocessing_amd import ops
    xyz, part = GC.kc46()
    plain = ops.icp_reference(xyz, part, NP, device=dev)
    grid = ops.icp_reference(xyz, part, NP, device=dev, accel="grid", max_dist=max_dist)
    assert type(grid) is ops.IcpGridReference and np.array_equal(plain.xyz.cpu().numpy(), GC.reference()[0])
    return plain, grid


def test_information_ops_wrapper_and_grid(dev):
    """ops.icp_information on the plain and the grid reference (built at max_dist 2): info, pairs, rmse and idx byte for byte, d2 by
    the grid's contract; info is the symmetric matrix of the oracle's sums and rmse their root mean square"""
    from pointcloudprocessing_amd import ops
    c = GC.sums_case(3, 5000)
    plain, grid = _refs(dev)
    S, L, P = (_t(c[k], dev) for k in ("scan", "lab", "pose"))
    for md in (2.0, 1.0):
        a = ops.icp_information(S, L, plain, P, md)
        b = ops.icp_information(S, L, grid, P, md)
        assert _bytes_equal(a[:4], b[:4]), md
        within = a[4] <= grid.r2
        assert torch.equal(a[4][within], b[4][within]) and bool(torch.isinf(b[4][~within]).all()) and int((~within).sum()) > 100
        assert _bytes_equal(a, ops.icp_information(S, L, plain, P.float(), md))        # the search runs at the fp32 rounding
        info, pairs, rmse, idx, d2 = (x.cpu().numpy() for x in a)
        ri, rd = IO.correspond(c["scan"], c["lab"], c["ref"], c["seg"], NP, c["pose"].astype(F32), max_d2=F32(md * md))
        assert np.array_equal(idx, ri) and np.array_equal(d2.view(np.uint32), rd.view(np.uint32))
        assert info.shape == (3, 6, 6) and pairs.dtype == np.int32 and np.array_equal(info, np.swapaxes(info, 1, 2))
        for s in range(3):
            kept = ri[s] >= 0
            exp, mag = PG.information(c["ref"][ri[s][kept]], rd[s][kept])
            assert pairs[s] == kept.sum() and np.all(np.abs(info[s] - PG.info_matrix(exp)) <= 1e-12 * PG.info_matrix(mag))
            assert abs(rmse[s] - np.sqrt(exp[28] / exp[0])) <= 1e-12 * rmse[s] and np.all(np.linalg.eigvalsh(info[s]) > 0)
    # a scan without a pair: no information, rmse NaN
    far = ops.icp_information(S[:1].contiguous() + 1e6, L[:1].contiguous(), plain, P[:1].contiguous(), 1.0)
    assert int(far[1][0]) == 0 and bool(torch.isnan(far[2][0])) and bool((far[0] == 0).all())


def test_information_determinism_graph_and_batch(dev):
    from pointcloudprocessing_amd import ops
    c = GC.sums_case(3, 5000)
    plain, _ = _refs(dev)
    S, L, P = (_t(c[k], dev) for k in ("scan", "lab", "pose"))
    a = ops.icp_information(S, L, plain, P, 2.0)
    assert _bytes_equal(a, ops.icp_information(S, L, plain, P, 2.0))
    for i in range(3):
        single = ops.icp_information(S[i:i + 1].contiguous(), L[i:i + 1].contiguous(), plain, P[i:i + 1].contiguous(), 2.0)
        assert _bytes_equal([x[i:i + 1] for x in a], single), i
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.icp_information(S, L, plain, P, 2.0)
        with torch.cuda.graph(g, stream=side):
            captured = ops.icp_information(S, L, plain, P, 2.0)
    torch.cuda.current_stream().wait_stream(side)
    for t in captured:
        t.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    assert _bytes_equal(a, captured) and int(a[1].min()) > 1000


# ---- pn_pose_graph_optimize ------------------------------------------------------------------------------------
def _solve_raw(dev, K, edges, Z, info, poses, weight=None, max_iters=50, tol=1e-10, lambda0=1e-3, capture=False):
    """the raw entry between guard bands -> (poses, cost, iters, status) as arrays; with ``capture`` also the same from a replay of
    the captured call"""
    from pointcloudprocessing_amd import _lib
    E = len(edges)
    ins = [_t(np.asarray(edges, np.int32), dev), _t(Z, dev), _t(info, dev)] + ([] if weight is None else [_t(np.asarray(weight, np.float64), dev)])
    keep = [x.clone() for x in ins]
    nbytes = _lib.lib().pn_pose_graph_workspace_bytes(K, E)
    bufs = dict(poses=_guarded((K, 4, 4), torch.float64, dev), cost=_guarded((2,), torch.float64, dev), iters=_guarded((1,), torch.int32, dev),
                status=_guarded((1,), torch.int32, dev), ws=_guarded((max(nbytes, 8),), torch.uint8, dev))
    p = lambda k: C.c_void_p(bufs[k][1].data_ptr())                                   # noqa: E731
    start = _t(poses, dev)

    def call():
        bufs["poses"][1].copy_(start)
        rc = _lib.lib().pn_pose_graph_optimize(K, E, _lib.ptr(ins[0]), _lib.ptr(ins[1]), _lib.ptr(ins[2]), _lib.ptr(ins[3]) if weight is not None else None,
                                               p("poses"), max_iters, tol, lambda0, p("cost"), p("iters"), p("status"), p("ws"), nbytes,
                                               _lib.current_stream())
        _lib.check(rc, "pn_pose_graph_optimize")

    def read():
        torch.cuda.synchronize()
        for name, (buf, _) in bufs.items():
            assert _intact(buf), f"{name}: guard band overwritten"
        for a, b in zip(keep, ins):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "an input was modified"
        return tuple(bufs[k][1].cpu().numpy().copy() for k in ("poses", "cost", "iters", "status"))

    call()
    eager = read()
    if not capture:
        return eager
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
        with torch.cuda.graph(g, stream=side):
            call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for k in ("poses", "cost", "iters", "status"):
        bufs[k][1].fill_(0)
    g.replay()
    return eager, read()


@pytest.mark.parametrize("K,E,kind,trials", [(2, 1, "consistent", 8), (6, 9, "noisy", 8), (44, 300, "noisy", 2), (64, 300, "noisy", 2)])
def test_pose_graph_against_oracle(dev, K, E, kind, trials):
    """(2, 1): the smallest legal graph (n = 6); (6, 9): fewer edges than a wave; (44, 300): more edges and more unknowns (258)
    than threads; (64, 300): the maximum (378).  The device may differ from the oracle by 100 max(s, 1e-14), s the oracle's own
    largest pose change under relative 2^-50 perturbations of every Z entry (fixed seeds): two decimal orders for device libm and
    reduction-order differences of a few ulp each.  Eager equals graph replay byte for byte, and X_0 comes back bit for bit.
    Measured on the MI355X, s / device - oracle: (2, 1) 1.78e-15 / 2.2e-16; (6, 9) 2.18e-11 / 4.4e-15; (44, 300) 5.08e-9 / 5.08e-9
    (both end by "no try accepted", the device two iterations later: DESIGN.md section 7); (64, 300) 4.22e-15 / 1.78e-15."""
    g = PG.graph(K, E, kind)
    s, base = PG.sensitivity(g, trials)
    (X, cost, iters, status), replay = _solve_raw(dev, K, g["edges"], g["Z"], g["info"], g["start"], capture=True)
    diff = float(np.abs(X - base[0]).max())
    print(f"K={K} E={E} n={6 * (K - 1)}: s = {s:.3g}, device - oracle = {diff:.3g}, iters {int(iters[0])}/{base[2]}, status {int(status[0])}/{base[3]}, "
          f"cost {cost[0]:.6g} -> {cost[1]:.6g} (oracle {base[1][0]:.6g} -> {base[1][1]:.6g})")
    assert np.array_equal(X[0].view(np.uint64), np.asarray(g["start"][0]).view(np.uint64))
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip((X, cost, iters, status), replay))
    assert status[0] == base[3] == 0 and 1 <= iters[0] <= 50
    assert abs(cost[0] - base[1][0]) <= 1e-12 * base[1][0] and cost[1] <= cost[0]
    assert diff <= 100 * max(s, 1e-14), (diff, s)


def test_pose_graph_weights_singular_and_bad_edges(dev):
    """guarded numeric paths, not faults: a node whose every edge has weight 0 gives PN_POSE_GRAPH_SINGULAR with the input poses back
    bit for bit; an index K in ``edges`` gives PN_POSE_GRAPH_BAD_EDGE, NaN costs and untouched poses; an edge of weight 0 (or a
    negative or non-finite weight) is bit for bit the graph without it; max_iters running out sets PN_POSE_GRAPH_MAX_ITERS"""
    g = PG.graph(6, 9, "noisy")
    K, e, Z, L, S = 6, np.asarray(g["edges"]), g["Z"], g["info"], np.asarray(g["start"])
    w = np.where((e == 5).any(1), 0.0, 1.0)
    X, cost, iters, status = _solve_raw(dev, K, e, Z, L, S, weight=w)
    assert status[0] == PG.SINGULAR and iters[0] == 1 and np.array_equal(X.view(np.uint64), S.view(np.uint64)) and cost[0] == cost[1] > 0
    bad = e.copy()
    bad[3, 1] = K
    X, cost, iters, status = _solve_raw(dev, K, bad, Z, L, S)
    assert status[0] == PG.BAD_EDGE and iters[0] == 0 and np.isnan(cost).all() and np.array_equal(X.view(np.uint64), S.view(np.uint64))
    for i, j in ((-1, 2), (2, 2)):
        bad = e.copy()
        bad[8] = (i, j)
        assert _solve_raw(dev, K, bad, Z, L, S)[3][0] == PG.BAD_EDGE
    keep = np.arange(9) != 7
    without = _solve_raw(dev, K, e[keep], Z[keep], L[keep], S)
    full = _solve_raw(dev, K, e, Z, L, S)
    assert without[3][0] == 0 and not np.array_equal(without[0], full[0])
    for v in (0.0, -2.0, np.nan, np.inf):
        w = np.ones(9)
        w[7] = v
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(_solve_raw(dev, K, e, Z, L, S, weight=w), without)), v
    # a weight scales its edge: 2 on every edge doubles the costs and leaves the minimiser where it is (to rounding)
    twice = _solve_raw(dev, K, e, Z, L, S, weight=np.full(9, 2.0))
    assert abs(twice[1][0] - 2 * full[1][0]) <= 1e-12 * full[1][0] and np.abs(twice[0] - full[0]).max() < 1e-7
    short = _solve_raw(dev, K, e, Z, L, S, max_iters=2)
    assert short[3][0] == PG.MAX_ITERS and short[2][0] == 2 and short[1][1] < short[1][0]


def test_pose_graph_ops_wrapper(dev):
    from pointcloudprocessing_amd import ops
    g = PG.graph(6, 9, "noisy")
    Z, L, S = (_t(g[k], dev) for k in ("Z", "info", "start"))
    raw = _solve_raw(dev, 6, g["edges"], g["Z"], g["info"], g["start"])
    for edges in ([tuple(int(v) for v in p) for p in g["edges"]], torch.from_numpy(np.array(g["edges"])), torch.from_numpy(np.array(g["edges"], np.int64))):
        got = ops.pose_graph_optimize(edges, Z, L, S)
        assert all(np.array_equal(a.cpu().numpy().view(np.uint8), b.view(np.uint8)) for a, b in zip(got, raw))
    assert got[0].data_ptr() != S.data_ptr() and torch.equal(S, _t(g["start"], dev))
    w = torch.ones(9, device=dev, dtype=torch.float64)
    w[7] = 0.0
    assert not _bytes_equal(ops.pose_graph_optimize(edges, Z, L, S, edge_weight=w)[:1], got[:1])


# ---- end to end --------------------------------------------------------------------------------------------------
MAX_DIST = 3.0


def _scene(dev):
    """K = 4 independent surface samplings of the aircraft mesh, 2,000 points each; cloud i is the model seen from a frame that is
    2.5 to 3.5 degrees and 0.3 to 0.45 m from its neighbour's -> (clouds, truth (4, 4, 4) with X_0 = I)"""
    from pointcloudprocessing_amd import ops
    v, f, p = MO.aircraft_mesh(2)
    mesh = ops.icp_mesh_reference(v, f, p, NM, device=dev)
    xyz = ops.mesh_sample(mesh, 2000, seed=21, sets=4)[0].double()
    steps = [([1, 2, -1], 3.0, [0.25, -0.15, 0.2]), ([-2, 1, 1], 2.5, [-0.2, 0.2, 0.1]), ([1, -1, 3], 3.5, [0.3, 0.3, -0.15])]
    truth = [np.eye(4)]
    for axis, deg, t in steps:
        D = np.eye(4)
        D[:3, :3] = IO.rot(axis, np.deg2rad(deg))
        D[:3, 3] = t
        truth.append(truth[-1] @ D)
    truth = np.stack(truth)
    clouds = []
    for i in range(4):
        Xi = _t(PG.inv(truth[i]), dev)
        clouds.append((xyz[i] @ Xi[:3, :3].T + Xi[:3, 3]).float().contiguous())
    return clouds, truth


def _displacement(X, truth, pts):
    """how far a pose is off: the largest distance between a model point moved by it and by the truth, in metres"""
    a = pts @ X[:3, :3].T + X[:3, 3]
    b = pts @ truth[:3, :3].T + truth[:3, 3]
    return float(np.linalg.norm(a - b, axis=1).max())


def test_multiway_register_end_to_end(dev):
    """multiway_register(edges="all") on the four samplings equals, byte for byte, the same steps composed by hand (register_scans
    per target, icp_information, pose_graph_optimize).  Against the truth the yardstick is register_scans of cloud 0 directly
    against each cloud i from the same start (the composed chain): the multiway poses may be at most twice as far off as the worst
    of those, since the graph spreads the edges' errors over the nodes and does not remove them.  Measured on the MI355X (largest
    displacement of a cloud point, nodes 1..3): direct 0.048 / 0.032 / 0.034 m, multiway 0.069 / 0.024 / 0.036 m (bound 0.096 m).  merge_scans of the result is voxel_downsample of the hand-transformed concatenation
    and serves icp_reference; with min_fitness above one edge's fitness that edge's weight is 0 and the result is the call without
    it."""
    from pointcloudprocessing_amd import ops
    clouds, truth = _scene(dev)
    K = 4
    got = ops.multiway_register(clouds, MAX_DIST, edges="all")
    poses, cost, iters, status, edges, Z, info, pairs = got
    e = edges.numpy()
    assert e.tolist() == [[i, j] for i in range(K) for j in range(i + 1, K)] and int(status[0]) == 0 and float(cost[1]) <= float(cost[0])
    assert torch.equal(poses[0], torch.eye(4, device=dev, dtype=torch.float64))
    # the same by hand: the chain edges from the identity, the nodes' start composed from them, the other edges from that start
    eye = torch.eye(4, device=dev, dtype=torch.float64)
    hz, hi, hp = torch.zeros_like(Z), torch.zeros_like(info), torch.zeros_like(pairs)

    def by_hand(ks, start_of):
        for j in sorted({int(e[k, 1]) for k in ks}):
            group = [k for k in ks if e[k, 1] == j]
            src = torch.stack([clouds[int(e[k, 0])] for k in group])
            res = ops.register_scans(src, clouds[j], MAX_DIST, init_pose=torch.stack([start_of(k) for k in group]))
            ref = ops.icp_reference(clouds[j], torch.zeros(len(clouds[j]), dtype=torch.int32), 1, accel="grid", max_dist=MAX_DIST)
            inf = ops.icp_information(src, torch.zeros(src.shape[:2], device=dev, dtype=torch.int32), ref, res[0], MAX_DIST)
            rows = torch.tensor(group, device=dev)
            hz[rows], hi[rows], hp[rows] = res[0], inf[0], inf[1]

    chain = [k for k in range(len(e)) if e[k, 1] == e[k, 0] + 1]
    by_hand(chain, lambda k: eye)
    nodes = [eye]
    for a in range(K - 1):
        nodes.append(nodes[a] @ hz[[k for k in chain if e[k, 0] == a][0]])
    start = torch.stack(nodes)
    inv = lambda T: torch.from_numpy(PG.inv(T.cpu().numpy())).to(dev)                 # noqa: E731
    by_hand([k for k in range(len(e)) if k not in chain], lambda k: ops._rigid_inverse(start[e[k, 0]]) @ start[e[k, 1]])
    assert _bytes_equal((Z, info, pairs), (hz, hi, hp))
    hand = ops.pose_graph_optimize(e, hz, hi, start, torch.ones(len(e), device=dev, dtype=torch.float64))
    assert _bytes_equal(got[:4], hand)
    assert float((ops._rigid_inverse(start) - inv(start)).abs().max()) < 1e-12
    # against the truth
    pts = [c.double().cpu().numpy() for c in clouds]
    yard, multi, chained = [], [], []
    P = poses.cpu().numpy()
    for i in range(1, K):
        d = ops.register_scans(clouds[0], clouds[i], MAX_DIST, init_pose=start[i])[0][0].cpu().numpy()   # p_0 ~= X_i p_i
        yard.append(_displacement(d, truth[i], pts[i]))
        multi.append(_displacement(P[i], truth[i], pts[i]))
        chained.append(_displacement(start[i].cpu().numpy(), truth[i], pts[i]))
    print(f"displacement against the truth (m): direct {np.round(yard, 4).tolist()}, multiway {np.round(multi, 4).tolist()}, composed chain "
          f"{np.round(chained, 4).tolist()}; cost {float(cost[0]):.6g} -> {float(cost[1]):.6g} in {int(iters[0])} iterations")
    assert max(yard) < 0.5, "the yardstick itself did not converge"
    assert max(multi) <= 2.0 * max(yard), (multi, yard)
    # the merged model
    xyz, counts, maj = ops.merge_scans(clouds, poses, 0.5)
    moved = torch.cat([c @ poses[i].float()[:3, :3].T + poses[i].float()[:3, 3] for i, c in enumerate(clouds)])
    exp = ops.voxel_downsample(moved, [0.5] * 3, moved.min(0).values.cpu().tolist())
    assert maj is None and _bytes_equal((xyz, counts), exp[:2]) and int(counts.sum()) == 8000 and 1000 < len(xyz) < 8000
    labels = [torch.full((2000,), i % 2, device=dev, dtype=torch.int32) for i in range(K)]
    xyz2, counts2, maj2 = ops.merge_scans(clouds, poses, 0.5, labels=labels, n_labels=2)
    assert _bytes_equal((xyz2, counts2), (xyz, counts)) and set(maj2.cpu().tolist()) == {0, 1}
    ref = ops.icp_reference(xyz2, maj2, 2)
    assert ref.M == len(xyz) and ref.n_parts == 2
    back = ops.semantic_icp(clouds[0][None], torch.zeros(1, 2000, device=dev, dtype=torch.int32), ops.icp_reference(xyz, torch.zeros(len(xyz)), 1),
                            eye[None], max_dist=MAX_DIST)
    assert _displacement(back[0][0].cpu().numpy(), np.eye(4), pts[0]) < 0.5
    # min_fitness between the lowest and the second lowest fitness switches that edge off: the call without it (from given node
    # poses, so that no edge is needed to compose a start)
    init = _t(truth, dev)
    tight = 0.6                                                                       # (at MAX_DIST every point has a partner)
    a = ops.multiway_register(clouds, tight, edges="all", init=init, min_fitness=0.0)
    fa = a[7].cpu().numpy() / 2000.0
    oa = np.argsort(fa, kind="stable")
    thr = 0.5 * (fa[oa[0]] + fa[oa[1]])
    print(f"fitness at max_dist {tight}: {np.round(fa, 3).tolist()}")
    assert fa[oa[0]] < thr < fa[oa[1]]
    cut = ops.multiway_register(clouds, tight, edges="all", init=init, min_fitness=float(thr))
    less = ops.multiway_register(clouds, tight, edges=[tuple(p) for k, p in enumerate(e.tolist()) if k != oa[0]], init=init)
    live = np.arange(len(e)) != oa[0]
    assert _bytes_equal(cut[:4], less[:4]) and _bytes_equal((cut[5][live], cut[6][live], cut[7][live]), less[5:8])
    assert _bytes_equal(cut[5:8], a[5:8]) and not _bytes_equal(cut[:1], a[:1])
