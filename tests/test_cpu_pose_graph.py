"""Multiway registration without a GPU: the surface (header, binding, exports, ABI), every argument refusal of pn_icp_information
and pn_pose_graph_optimize (made before any HIP call), the Python-side refusals of the four ops functions, and -- on the oracle
alone (tests/pose_graph_oracle.py) -- that the information sums are G^T G, that the Jacobians are the derivatives of the residual,
that the loop brings a consistent graph back to the truth, converges on the noisy graphs the GPU tests use, and beats the composed
chain on a graph whose chain drifts."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import pose_graph_oracle as PG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
FAKE = C.c_void_p(0x1000)        # never dereferenced: the checks run before any HIP call
WS = 1 << 30
ENTRIES = ("pn_icp_information_workspace_bytes", "pn_icp_information", "pn_pose_graph_workspace_bytes", "pn_pose_graph_optimize")
# the graphs of tests/test_gpu_pose_graph.py: (K, E, kind)
GPU_GRAPHS = ((2, 1, "consistent"), (6, 9, "noisy"), (44, 300, "noisy"), (64, 300, "noisy"))


def _seg(*v):
    return (C.c_int32 * len(v))(*v)


def test_symbols_declared_bound_and_exported():
    from pointcloudprocessing_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "pointnet_hip.h")).read()
    for name in ENTRIES:
        assert f"{name}(" in hdr and name in _lib.SIGNATURES and hasattr(_lib.lib(), name), name
    assert "#define PN_ABI_VERSION 6" in hdr and _lib.lib().pn_abi_version() == 6 and _lib.ABI_VERSION == 6
    for name, value in (("MAX_NODES", 64), ("MAX_EDGES", 4096), ("MAX_ITERS", 1), ("SINGULAR", 2), ("BAD_EDGE", 4)):
        assert f"#define PN_POSE_GRAPH_{name} {value}\n" in hdr and getattr(_lib, "PN_POSE_GRAPH_" + name) == value
    assert (PG.MAX_ITERS, PG.SINGULAR, PG.BAD_EDGE) == (1, 2, 4)
    L = _lib.lib()
    assert L.pn_icp_information_workspace_bytes(0, 5, 5, 1) == 0 and L.pn_icp_information_workspace_bytes(1, 0, 5, 1) == 0
    for B, N in ((1, 1), (3, 5000)):                                          # the plane layout, no idx / d2 tail
        assert L.pn_icp_information_workspace_bytes(B, N, 100, 2) == L.pn_icp_plane_workspace_bytes(B, N, 100, 2)
    for K, E in ((1, 1), (65, 64), (4, 2), (4, 4097), (0, 0)):
        assert L.pn_pose_graph_workspace_bytes(K, E) == 0, (K, E)
    n = 6 * 63
    assert L.pn_pose_graph_workspace_bytes(64, 4096) >= 8 * (2 * n * n + 4096 * (72 + 6)) and L.pn_pose_graph_workspace_bytes(2, 1) > 0
    for name in ("icp_information", "pose_graph_optimize", "multiway_register", "merge_scans"):
        assert hasattr(ops, name), name
    assert ops.IcpGridReference._INFO == ops.IcpReference._INFO == ENTRIES[1::-1]
    assert ops.IcpMeshReference._INFO is None and ops.IcpBvhMeshReference._INFO is None


def _info(ptrs=None, seg=None, M=8, n_parts=2, ws=WS, max_d2=1.0, B=1, grid=None, grid_r2=0.0):
    from pointcloudprocessing_amd import _lib
    p = ptrs or {}
    g = lambda k: p.get(k, FAKE)                                              # noqa: E731
    return _lib.lib().pn_icp_information(g("scan"), g("labels"), B, 64, g("ref"), seg or _seg(0, 4, M), M, n_parts, g("pose32"), max_d2,
                                         g("idx"), g("d2"), g("sums"), g("ws"), ws, grid, grid_r2, None)


def _solve(ptrs=None, K=4, E=5, max_iters=50, tol=1e-10, lambda0=1e-3, ws=WS):
    from pointcloudprocessing_amd import _lib
    p = ptrs or {}
    g = lambda k: p.get(k, FAKE)                                              # noqa: E731
    return _lib.lib().pn_pose_graph_optimize(K, E, g("edges"), g("Z"), g("info"), p.get("weight"), g("poses"), max_iters, tol, lambda0,
                                             g("cost"), g("iters"), g("status"), g("ws"), ws, None)


def test_argument_refusals_without_gpu():
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    short = L.pn_icp_information_workspace_bytes(1, 64, 8, 2) - 1
    pg_short = L.pn_pose_graph_workspace_bytes(4, 5) - 1
    inf, nan = float("inf"), float("nan")
    odd = C.c_void_p(0x1004)
    cases = [
        (lambda: _info({"pose32": None}), b"pose32"), (lambda: _info({"scan": None}), b"null pointer"),
        (lambda: _info({"labels": None}), b"null pointer"), (lambda: _info({"ref": None}), b"null pointer"),
        (lambda: _info({"ws": None}), b"null pointer"), (lambda: _info({"idx": None}), b"idx_out"), (lambda: _info({"d2": None}), b"d2_out"),
        (lambda: _info({"sums": None}), b"sums_out"), (lambda: _info(max_d2=nan), b"max_d2 is NaN"), (lambda: _info(ws=short), b"workspace"),
        (lambda: _info(seg=_seg(0, 5, 4), M=4), b"not monotone"), (lambda: _info(seg=_seg(0, 4, 7)), b"end at M"),
        (lambda: _info(M=0, seg=_seg(0, 0, 0)), b"M=0"), (lambda: _info(n_parts=17), b"n_parts=17"), (lambda: _info(n_parts=0), b"n_parts=0"),
        (lambda: _info(B=0), b"B=0"),
        # with a grid: the grid entries' own checks first
        (lambda: _info(grid=odd, grid_r2=1.0), b"16-byte aligned"), (lambda: _info(grid=FAKE, grid_r2=0.0), b"grid_max_d2"),
        (lambda: _info(grid=FAKE, grid_r2=nan), b"grid_max_d2"), (lambda: _info(grid=FAKE, grid_r2=1.0, max_d2=inf), b"at most the tables'"),
        (lambda: _info(grid=FAKE, grid_r2=1.0, max_d2=float(np.nextafter(F32(1), F32(2)))), b"at most the tables'"),
        (lambda: _info({"sums": None}, grid=FAKE, grid_r2=1.0), b"sums_out"),
        # the graph solve
        (lambda: _solve({"edges": None}), b"null pointer"), (lambda: _solve({"Z": None}), b"null pointer"),
        (lambda: _solve({"info": None}), b"null pointer"), (lambda: _solve({"poses": None}), b"null pointer"),
        (lambda: _solve({"cost": None}), b"null pointer"), (lambda: _solve({"iters": None}), b"null pointer"),
        (lambda: _solve({"status": None}), b"null pointer"), (lambda: _solve({"ws": None}), b"null pointer"),
        (lambda: _solve(K=1, E=1), b"K=1"), (lambda: _solve(K=65, E=64), b"K=65"), (lambda: _solve(K=4, E=2), b"E=2"),
        (lambda: _solve(K=4, E=4097), b"E=4097"), (lambda: _solve(max_iters=0), b"max_iters=0"), (lambda: _solve(max_iters=10001), b"max_iters="),
        (lambda: _solve(tol=-1.0), b"tol="), (lambda: _solve(tol=nan), b"tol="), (lambda: _solve(lambda0=0.0), b"lambda0=0"),
        (lambda: _solve(lambda0=-1.0), b"lambda0="), (lambda: _solve(lambda0=nan), b"lambda0="), (lambda: _solve(lambda0=inf), b"lambda0="),
        (lambda: _solve(ws=pg_short), b"workspace"), (lambda: _solve({"ws": odd}), b"8-byte aligned"),
    ]
    for k, (call, msg) in enumerate(cases):
        assert call() == -1, k
        assert msg in L.pn_last_error(), (k, msg, L.pn_last_error())
    # a max_d2 of +inf without a grid, and one at the tables' with one, pass the checks (the next refusal is the workspace's)
    for kw in (dict(max_d2=inf, ws=short), dict(grid=FAKE, grid_r2=1.0, max_d2=1.0, ws=short)):
        assert _info(**kw) == -1 and b"workspace" in L.pn_last_error(), kw


def test_python_side_refusals():
    """every refusal below is made on the host, before a tensor is asked to be on the device"""
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd._lib import PointNetHipError
    z, i64 = torch.zeros, torch.int64
    mesh = ops.IcpMeshReference(z(4, 3, 3), (0, 2, 4), z(4, dtype=i64), 2, z(4, 3), z(4, dtype=torch.float64))
    grid = ops.IcpGridReference(z(6, 3), (0, 3, 6), z(6, dtype=i64), 2, None, z(64, dtype=torch.uint8), 0.5, ops._max_d2(0.5), (0, 0, 0))
    S, L, P = z(1, 8, 3), z(1, 8, dtype=torch.int32), z(1, 4, 4)
    with pytest.raises(PointNetHipError, match="cloud reference"):
        ops.icp_information(S, L, mesh, P, 1.0)
    with pytest.raises(PointNetHipError, match="must come from"):
        ops.icp_information(S, L, object(), P, 1.0)
    for md in (0.6, float("inf")):
        with pytest.raises(PointNetHipError, match="exceeds the grid reference's max_dist=0.5"):
            ops.icp_information(S, L, grid, P, md)
    X = z(4, 4, 4, dtype=torch.float64)
    cases = [([(0, 1), (1, 0), (2, 3)], r"not connected: no path of edges joins node 2 to node 0 \(2 such nodes\)"),
             ([(0, 1), (1, 2), (2, 4)], r"edge 2 = \(2, 4\) has an index outside \[0, 4\)"),
             ([(0, 1), (1, 2), (-1, 3)], r"edge 2 = \(-1, 3\) has an index"), ([(0, 1), (1, 2), (3, 3)], r"edge 2 = \(3, 3\) joins a node to itself"),
             ([(0, 1), (1, 2)], "2 edges outside"), ([(0, 1, 2)] * 3, "pairs"), (torch.zeros(3, 2), "CPU integer tensor"), (7, "pairs")]
    for edges, msg in cases:
        with pytest.raises(PointNetHipError, match=msg):
            ops.pose_graph_optimize(edges, None, None, X)
        if not isinstance(edges, int):
            with pytest.raises(PointNetHipError, match=msg):
                ops.multiway_register([z(5, 3)] * 4, 1.0, edges=edges)
    with pytest.raises(PointNetHipError, match="CPU integer tensor"):
        ops.pose_graph_optimize(torch.zeros(3, 2), None, None, X)
    with pytest.raises(PointNetHipError, match=r"poses must be a \(K,4,4\)"):
        ops.pose_graph_optimize([(0, 1)], None, None, z(4, 4))
    with pytest.raises(PointNetHipError, match="65 nodes outside"):
        ops.pose_graph_optimize([(0, 1)], None, None, z(65, 4, 4))
    with pytest.raises(PointNetHipError, match="CUDA/HIP tensor"):                    # a good edge list reaches the tensors
        ops.pose_graph_optimize(torch.tensor([[0, 1], [1, 2], [3, 2]]), z(3, 4, 4), z(3, 6, 6), X)
    clouds = [z(5, 3)] * 4
    for kw, msg in ((dict(viewpoint=(0, 0, 0)), "viewpoint= is not an argument"), (dict(init_pose=P), "init_pose= is not an argument"),
                    (dict(source_normals=S), "source_normals= is not an argument"), (dict(gicp_eps=0.1), "gicp_eps= is not an argument"),
                    (dict(feature_radius=1.0), "feature_radius= is not an argument"), (dict(robust="huber"), "robust= is not an argument"),
                    (dict(pose_graph=dict(iters=3)), "pose_graph has no iters"), (dict(metric="mesh"), "metric must be"),
                    (dict(init="local"), "init must be None, 'global' or"), (dict(edges="chain"), "edges must be None"),
                    (dict(edges=[(0, 1), (0, 2), (0, 3)]), r"edges must contain \(1, 2\)")):
        with pytest.raises(PointNetHipError, match=msg):
            ops.multiway_register(clouds, 1.0, **kw)
    with pytest.raises(PointNetHipError, match="at least two"):
        ops.multiway_register(clouds[:1], 1.0)
    with pytest.raises(PointNetHipError, match="CUDA/HIP tensor"):                    # good keywords reach the tensors
        ops.multiway_register(clouds, 1.0, edges="all", max_iters=5, normals_k=6, accel=None, pose_graph=dict(tol=1e-9))
    with pytest.raises(PointNetHipError, match=r"poses must be a \(4,4,4\)"):
        ops.merge_scans(clouds, z(3, 4, 4), 0.1)
    with pytest.raises(PointNetHipError, match="labels must be a list of 4"):
        ops.merge_scans(clouds, X, 0.1, labels=[L[0]] * 3)


# ---- the oracle on itself ------------------------------------------------------------------------------------
def test_information_is_the_sum_of_GtG():
    rng = np.random.default_rng(4)
    q = rng.uniform(-30, 30, (500, 3)).astype(F32)
    d2 = rng.uniform(0, 4, 500).astype(F32)
    sums, mag = PG.information(q, d2)
    G = np.concatenate([-PG.hat(q.astype(np.float64)), np.broadcast_to(np.eye(3), (500, 3, 3))], 2)       # (n, 3, 6)
    M = PG.info_matrix(sums)
    assert np.allclose(M, (np.swapaxes(G, 1, 2) @ G).sum(0), rtol=1e-13, atol=0) and np.array_equal(M, M.T)
    assert sums[0] == 500 and np.all(sums[22:28] == 0) and sums[28] == d2.astype(np.float64).sum() and np.all(mag >= np.abs(sums))
    assert np.all(np.linalg.eigvalsh(M) > 0)
    # G^T G is the Hessian of sum |E q - q|^2 / 2 in a right perturbation E = D(delta) of the pose in the reference's frame
    f = lambda d: 0.5 * np.sum((q.astype(np.float64) @ PG.D(d)[:3, :3].T + PG.D(d)[:3, 3] - q) ** 2)        # noqa: E731
    h = 1e-4
    for a in range(6):
        for b in range(6):
            ea, eb = np.eye(6)[a] * h, np.eye(6)[b] * h
            num = (f(ea + eb) - f(ea - eb) - f(eb - ea) + f(-ea - eb)) / (4 * h * h)
            assert abs(num - M[a, b]) <= 1e-5 * np.sqrt(M[a, a] * M[b, b]), (a, b, num, M[a, b])


def test_jacobians_are_the_derivatives_of_the_residual():
    g = PG.graph(6, 9, "noisy")
    X, e, Z = np.array(g["start"]), g["edges"].astype(np.int64), g["Z"]
    for a in range(1, 6):                                              # off the solution, so that omega is not small
        X[a] = X[a] @ PG.random_pose(np.random.default_rng(a), 20, 0.5)
    r, Ji, Jj = PG.jacobians(X, e, Z)
    h = 1e-6
    for k, (i, j) in enumerate(e):
        for node, J in ((i, Ji[k]), (j, Jj[k])):
            for m in range(6):
                d = np.zeros(6)
                d[m] = h
                Xp, Xm = X.copy(), X.copy()
                Xp[node], Xm[node] = X[node] @ PG.D(d), X[node] @ PG.D(-d)
                num = (PG.residuals(Xp, e[k:k + 1], Z[k:k + 1])[0][0] - PG.residuals(Xm, e[k:k + 1], Z[k:k + 1])[0][0]) / (2 * h)
                assert np.abs(num - J[:, m]).max() <= 1e-8 * max(1.0, np.abs(J).max()), (k, node, m)


def test_consistent_graph_comes_back_to_the_truth():
    for K, E in ((2, 1), (6, 9), (12, 20)):
        g = PG.graph(K, E, "consistent")
        assert PG.node_error(g["start"], g["truth"]) > 1e-2
        X, cost, iters, status = PG.optimize(K, g["edges"], g["Z"], g["info"], g["start"])
        assert status == 0 and 1 < iters < 50 and cost[0] > 1.0 and cost[1] < 1e-20 * cost[0], (K, cost, iters)
        assert PG.node_error(X, g["truth"]) < 1e-12 and np.array_equal(X[0], g["start"][0])


@pytest.mark.parametrize("K,E,kind", [g for g in GPU_GRAPHS if g[2] == "noisy"] + [(8, 12, "drift")])
def test_noisy_graphs_converge(K, E, kind):
    """the central-difference gradient of the true cost at the result is at most 1e-6 of its value at the start (measured: 2.8e-11
    at (6, 9), 1.2e-9 at (44, 300), 2.0e-12 at (64, 300), 3.0e-11 on the drift graph): the Jacobians are exact to first order, so the iteration does not stall"""
    g = PG.graph(K, E, kind)
    w = np.ones(E)
    X, cost, iters, status = PG.optimize(K, g["edges"], g["Z"], g["info"], g["start"])
    assert status == 0 and iters < 50 and cost[1] < cost[0]
    sub = slice(None) if K <= 8 else np.r_[1:3, K - 2:K]              # (every node at the small sizes, four nodes at the large)
    e64 = g["edges"].astype(np.int64)

    def grad(P):
        if K <= 8:
            return PG.numeric_gradient(P, e64, g["Z"], g["info"], w)
        out = []
        for a in sub:
            for m in range(6):
                d = np.zeros(6)
                d[m] = 1e-6
                Pp, Pm = np.array(P), np.array(P)
                Pp[a], Pm[a] = P[a] @ PG.D(d), P[a] @ PG.D(-d)
                out.append((PG.cost(Pp, e64, g["Z"], g["info"], w) - PG.cost(Pm, e64, g["Z"], g["info"], w)) / 2e-6)
        return np.array(out)

    g0, g1 = np.abs(grad(g["start"])).max(), np.abs(grad(X)).max()
    print(f"K={K} E={E} {kind}: cost {cost[0]:.4g} -> {cost[1]:.4g} in {iters} iterations, gradient {g0:.3g} -> {g1:.3g}")
    assert g0 > 1.0 and g1 <= 1e-6 * g0, (g0, g1)


def test_drift_graph_beats_the_composed_chain():
    """a chain whose every link carries the same bias drifts; loop closures pull it back: the worst node error against the truth
    is at most a quarter of the composed chain's (measured 0.325 -> 0.037 at (8, 12), 0.672 -> 0.054 at (12, 20))"""
    for K, E in ((8, 12), (12, 20)):
        g = PG.graph(K, E, "drift")
        X, cost, iters, status = PG.optimize(K, g["edges"], g["Z"], g["info"], g["start"])
        e0, e1 = PG.node_error(g["start"], g["truth"]), PG.node_error(X, g["truth"])
        print(f"drift K={K} E={E}: chain {e0:.4g}, graph {e1:.4g}")
        assert status == 0 and e0 > 0.2 and e1 <= 0.25 * e0, (e0, e1)


def test_weights_bad_edges_and_singular_graphs():
    g = PG.graph(6, 9, "noisy")
    K, e, Z, L, S = 6, g["edges"], g["Z"], g["info"], g["start"]
    base = PG.optimize(K, e, Z, L, S)
    # an edge of weight 0, negative, NaN or inf is the graph without it
    for bad in (0.0, -1.0, np.nan, np.inf):
        w = np.ones(9)
        w[7] = bad
        keep = np.arange(9) != 7
        a, b = PG.optimize(K, e, Z, L, S, edge_weight=w), PG.optimize(K, e[keep], Z[keep], L[keep], S)
        assert np.array_equal(a[0], b[0]) and a[3] == b[3] == 0 and not np.array_equal(a[0], base[0])
    # node 5 without a live edge: singular, the input back
    w = np.where((e == 5).any(1), 0.0, 1.0)
    X, cost, iters, status = PG.optimize(K, e, Z, L, S, edge_weight=w)
    assert status == PG.SINGULAR and iters == 1 and np.array_equal(X, S) and cost[0] == cost[1]
    eb = e.copy()
    eb[3, 1] = 6
    X, cost, iters, status = PG.optimize(K, eb, Z, L, S)
    assert status == PG.BAD_EDGE and iters == 0 and np.isnan(cost).all() and np.array_equal(X, S)
    assert PG.optimize(K, e, Z, L, S, max_iters=2)[3] == PG.MAX_ITERS


def test_sensitivity_is_small_and_the_oracle_is_quick():
    import time
    t = time.perf_counter()
    s, base = PG.sensitivity(PG.graph(64, 300), 2)
    dt = (time.perf_counter() - t) / 3
    print(f"K=64 E=300: sensitivity {s:.3g}, {dt:.2f} s per solve")
    assert base[3] == 0 and s < 1e-6 and dt < 2.0
