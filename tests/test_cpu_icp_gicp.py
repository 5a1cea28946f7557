"""Plane-to-plane (generalized) ICP without a GPU: the surface (header, binding, exports, ABI), every argument refusal of the two C
entries (made before any HIP call), the Python-side refusals, the routing of the wrappers for a plain and a grid reference (the
library replaced by a recorder, as in tests/test_cpu_icp_bindings.py), and -- on the oracle alone (tests/icp_gicp_oracle.py) -- that W
is what the header says it is, that J and the gradient are the derivatives of the residual, that the oracle loop registers the
analytic scene, and that the inputs of the GPU cases (shared with tests/test_gpu_icp_gicp.py) are what they claim to be."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import icp_gicp_oracle as GO
import icp_oracle as IO
import icp_plane_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
FAKE = C.c_void_p(0x1000)        # never dereferenced: the checks run before any HIP call
WS = 1 << 30
ENTRIES = ("pn_icp_gicp_workspace_bytes", "pn_icp_gicp_sums", "pn_semantic_icp_gicp")


def _seg(*v):
    return (C.c_int32 * len(v))(*v)


def test_symbols_declared_bound_and_exported():
    from pointcloudprocessing_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "pointnet_hip.h")).read()
    for name in ENTRIES:
        assert f"{name}(" in hdr and name in _lib.SIGNATURES and hasattr(_lib.lib(), name), name
    assert "#define PN_ABI_VERSION 6" in hdr and _lib.lib().pn_abi_version() == 6 and _lib.ABI_VERSION == 6
    L = _lib.lib()
    assert L.pn_icp_gicp_workspace_bytes(0, 5, 5, 1) == 0 and L.pn_icp_gicp_workspace_bytes(1, 0, 5, 1) == 0
    for B, N in ((1, 1), (3, 5000)):
        plane, robust, got = (getattr(L, f"pn_icp_{k}_workspace_bytes")(B, N, 100, 2) for k in ("plane", "robust", "gicp"))
        assert plane + 8 * B * N <= got < robust and got % 256 == 0           # the plane layout and the idx / d2 tail, not q
    assert hasattr(ops, "icp_gicp_sums")
    assert ops.IcpReference._GICP == ENTRIES[1:] + ENTRIES[:1] and ops.IcpGridReference._GICP == ops.IcpReference._GICP
    assert ops.IcpMeshReference._GICP is None and ops.IcpBvhMeshReference._GICP is None


def _sums(ptrs=None, seg=None, M=8, n_parts=2, ws=WS, max_d2=1.0, eps=1e-3, B=1, grid=None, grid_r2=0.0):
    from pointcloudprocessing_amd import _lib
    p = ptrs or {}
    g = lambda k: p.get(k, FAKE)                                              # noqa: E731
    return _lib.lib().pn_icp_gicp_sums(g("scan"), g("labels"), g("scan_normals"), B, 64, g("ref"), seg or _seg(0, 4, M), M, n_parts,
                                       g("ref_normals"), g("pose32"), g("pose64"), max_d2, eps, g("idx"), g("d2"), g("sums"), g("ws"), ws,
                                       grid, grid_r2, None)


def _loop(ptrs=None, max_iters=5, max_d2=1.0, tol=(1e-6, 1e-6), eps=1e-3, ws=WS, seg=None, M=8, n_parts=2, grid=None, grid_r2=0.0):
    from pointcloudprocessing_amd import _lib
    p = ptrs or {}
    g = lambda k: p.get(k, FAKE)                                              # noqa: E731
    return _lib.lib().pn_semantic_icp_gicp(g("scan"), g("labels"), g("scan_normals"), 1, 64, g("ref"), seg or _seg(0, 4, M), M, n_parts,
                                           g("ref_normals"), g("init"), max_iters, max_d2, tol[0], tol[1], eps, g("pose"), g("rmse"),
                                           g("pairs"), g("iters"), g("status"), g("ws"), ws, grid, grid_r2, None)


def test_argument_refusals_without_gpu():
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    short = L.pn_icp_gicp_workspace_bytes(1, 64, 8, 2) - 1
    inf, nan = float("inf"), float("nan")
    odd = C.c_void_p(0x1004)
    cases = [
        (lambda: _sums({"scan_normals": None}), b"scan_normals"), (lambda: _sums({"ref_normals": None}), b"ref_normals"),
        (lambda: _sums({"pose64": None}), b"pose64"), (lambda: _sums({"pose32": None}), b"pose32"),
        (lambda: _sums({"scan": None}), b"null pointer"), (lambda: _sums({"labels": None}), b"null pointer"),
        (lambda: _sums({"ref": None}), b"null pointer"), (lambda: _sums({"ws": None}), b"null pointer"),
        (lambda: _sums({"idx": None}), b"idx_out"), (lambda: _sums({"d2": None}), b"d2_out"), (lambda: _sums({"sums": None}), b"sums_out"),
        (lambda: _sums(eps=0.0), b"eps=0"), (lambda: _sums(eps=-1e-3), b"eps="), (lambda: _sums(eps=nan), b"eps="),
        (lambda: _sums(eps=float(np.nextafter(1.0, 2.0))), b"eps="), (lambda: _sums(eps=inf), b"eps="),
        (lambda: _sums(max_d2=nan), b"max_d2 is NaN"), (lambda: _sums(ws=short), b"workspace"),
        (lambda: _sums(seg=_seg(0, 5, 4), M=4), b"not monotone"), (lambda: _sums(seg=_seg(0, 4, 7)), b"end at M"),
        (lambda: _sums(M=0, seg=_seg(0, 0, 0)), b"M=0"), (lambda: _sums(n_parts=17), b"n_parts=17"), (lambda: _sums(B=0), b"B=0"),
        # with a grid: the grid entries' own checks first
        (lambda: _sums(grid=odd, grid_r2=1.0), b"16-byte aligned"), (lambda: _sums(grid=FAKE, grid_r2=0.0), b"grid_max_d2"),
        (lambda: _sums(grid=FAKE, grid_r2=nan), b"grid_max_d2"), (lambda: _sums(grid=FAKE, grid_r2=1.0, max_d2=inf), b"at most the tables'"),
        (lambda: _sums(grid=FAKE, grid_r2=1.0, max_d2=float(np.nextafter(F32(1), F32(2)))), b"at most the tables'"),
        (lambda: _sums({"scan_normals": None}, grid=FAKE, grid_r2=1.0), b"scan_normals"),
        (lambda: _sums(grid=FAKE, grid_r2=1.0, eps=2.0), b"eps=2"),
        (lambda: _loop({"scan_normals": None}), b"scan_normals"), (lambda: _loop({"ref_normals": None}), b"ref_normals"),
        (lambda: _loop({"init": None}), b"null pointer"), (lambda: _loop({"status": None}), b"null pointer"),
        (lambda: _loop({"pose": None}), b"null pointer"), (lambda: _loop({"scan": None}), b"null pointer"),
        (lambda: _loop(eps=0.0), b"eps=0"), (lambda: _loop(eps=1.5), b"eps=1.5"), (lambda: _loop(eps=nan), b"eps="),
        (lambda: _loop(max_iters=0), b"max_iters=0"), (lambda: _loop(max_iters=10001), b"max_iters="),
        (lambda: _loop(max_d2=nan), b"max_d2 is NaN"), (lambda: _loop(tol=(-1.0, 0.0)), b"tolerances"), (lambda: _loop(ws=short), b"workspace"),
        (lambda: _loop(grid=odd, grid_r2=1.0), b"16-byte aligned"), (lambda: _loop(grid=FAKE, grid_r2=2.25, max_d2=4.0), b"at most the tables'"),
        (lambda: _loop(grid=FAKE, grid_r2=1.0, max_d2=inf), b"at most the tables'"), (lambda: _loop(n_parts=0), b"n_parts=0"),
    ]
    for k, (call, msg) in enumerate(cases):
        assert call() == -1, k
        assert msg in L.pn_last_error(), (k, msg, L.pn_last_error())
    # eps = 1 and a max_d2 of +inf without a grid pass the checks (the next refusal is the workspace's)
    for kw in (dict(eps=1.0, ws=short), dict(max_d2=inf, ws=short), dict(grid=FAKE, grid_r2=1.0, max_d2=1.0, ws=short)):
        assert _sums(**kw) == -1 and b"workspace" in L.pn_last_error(), kw


# ---- the wrappers, with the library replaced by a recorder -----------------------------------------------------------
STREAM = 0x5
B, N, MD = 2, 8, 0.4


def _tensor_or_not(t, name, dtype=None):
    """_lib.require_gpu_tensor without its is_cuda test"""
    from pointcloudprocessing_amd._lib import PointNetHipError
    if not isinstance(t, torch.Tensor):
        raise PointNetHipError(f"{name} must be a CUDA/HIP tensor: the PointNet hot path has no CPU fallback")
    if not t.is_contiguous():
        raise PointNetHipError(f"{name} must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise PointNetHipError(f"{name} must have dtype {dtype}, got {t.dtype}")
    return t


@pytest.fixture
def calls(monkeypatch):
    from pointcloudprocessing_amd import ops
    rec = []

    class Recorder:
        def __getattr__(self, name):
            def entry(*args):
                rec.append((name, args))
                return 64 if name.endswith("_bytes") else 0
            return entry

    recorder = Recorder()
    monkeypatch.setattr(ops, "lib", lambda: recorder)
    monkeypatch.setattr(ops, "check", lambda rc, what="": None)
    monkeypatch.setattr(ops, "current_stream", lambda: C.c_void_p(STREAM))
    monkeypatch.setattr(ops, "require_gpu_tensor", _tensor_or_not)
    return rec


def _refs():
    from pointcloudprocessing_amd import ops
    z, i64 = torch.zeros, torch.int64
    return {"cloud": ops.IcpReference(z(6, 3), (0, 3, 6), z(6, dtype=i64), 2),
            "normals": ops.IcpReference(z(6, 3), (0, 3, 6), z(6, dtype=i64), 2, normals=z(6, 3)),
            "grid": ops.IcpGridReference(z(6, 3), (0, 3, 6), z(6, dtype=i64), 2, z(6, 3), z(64, dtype=torch.uint8), 0.5, ops._max_d2(0.5), (0, 0, 0)),
            "mesh": ops.IcpMeshReference(z(4, 3, 3), (0, 2, 4), z(4, dtype=i64), 2, z(4, 3), z(4, dtype=torch.float64))}


def _addr(a):
    return None if a is None else a.value


def _conforms(name, args):
    from pointcloudprocessing_amd import _lib
    slots = _lib.SIGNATURES[name][1]
    assert len(args) == len(slots), (name, len(args), len(slots))
    for k, (arg, slot) in enumerate(zip(args, slots)):
        if slot is C.c_void_p:
            ok = arg is None or isinstance(arg, C.c_void_p)
        elif slot is C.POINTER(C.c_int32):
            ok = isinstance(arg, C.Array) and arg._type_ is C.c_int32
        elif slot in (C.c_int, C.c_size_t):
            ok = type(arg) is int
        else:
            ok = slot in (C.c_float, C.c_double) and type(arg) is float
        assert ok, (name, k, arg, slot)


@pytest.mark.parametrize("kind", ["normals", "grid"])
def test_wrappers_call_the_gicp_entries(calls, kind):
    from pointcloudprocessing_amd import ops
    ref = _refs()[kind]
    S, L, SN = torch.zeros(B, N, 3), torch.zeros(B, N, dtype=torch.int32), torch.ones(B, N, 3)
    P64 = torch.zeros(B, 4, 4, dtype=torch.float64)
    tail = (ref.grid.data_ptr(), ref.r2) if kind == "grid" else (None, 0.0)
    ops.icp_gicp_sums(S, L, SN, ref, P64, MD, eps=0.01)
    ops.semantic_icp(S, L, ref, P64, 7, MD, 1e-5, 1e-4, metric="gicp", scan_normals=SN, gicp_eps=0.02)
    for name, args in calls:
        _conforms(name, args)
    (n0, a0), (n1, a1) = [c for c in calls if not c[0].endswith("_bytes")]
    assert [c[0] for c in calls if c[0].endswith("workspace_bytes")] == 2 * ["pn_icp_gicp_workspace_bytes"]
    for name, args in ((n0, a0), (n1, a1)):
        assert [_addr(a) for a in args[:3]] == [S.data_ptr(), L.data_ptr(), SN.data_ptr()] and args[3:5] == (B, N)
        assert _addr(args[5]) == ref.xyz.data_ptr() and list(args[6]) == [0, 3, 6] and args[7:9] == (6, 2) and _addr(args[9]) == ref.normals.data_ptr()
        assert (_addr(args[-3]), args[-2], _addr(args[-1])) == tail + (STREAM,)
    assert n0 == "pn_icp_gicp_sums" and _addr(a0[11]) == P64.data_ptr() and a0[12:14] == (ops._max_d2(MD), 0.01)
    assert n1 == "pn_semantic_icp_gicp" and a1[11:16] == (7, ops._max_d2(MD), 1e-5, 1e-4, 0.02) and _addr(a1[10]) == _addr(a1[16])
    # "point" and "plane" run exactly the calls they ran before
    del calls[:]
    ops.semantic_icp(S, L, ref, P64, 7, MD, metric="plane")
    ops.semantic_icp(S, L, ref, P64, 7, MD)
    want = {"normals": ["pn_semantic_icp_plane", "pn_semantic_icp"], "grid": 2 * ["pn_semantic_icp_grid"]}[kind]
    assert [c[0] for c in calls if not c[0].endswith("_bytes")] == want


def test_python_side_refusals(calls):
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd._lib import PointNetHipError
    R = _refs()
    S, L, SN = torch.zeros(B, N, 3), torch.zeros(B, N, dtype=torch.int32), torch.ones(B, N, 3)
    I = torch.zeros(B, 4, 4, dtype=torch.float64)
    bad = [(dict(ref=R["mesh"]), "cloud reference"), (dict(ref=R["cloud"]), "needs reference normals"),
           (dict(scan_normals=None), "needs scan_normals"), (dict(scan_normals=SN[:, :5].contiguous()), "scan_normals must be"),
           (dict(scan_normals=SN.double()), "dtype"), (dict(scan_normals=SN.numpy()), "CUDA/HIP tensor"),
           (dict(scan_normals=SN.to("meta")), "scan_normals must be")]
    for kw, msg in bad:
        a = dict(ref=R["normals"], scan_normals=SN)
        a.update(kw)
        with pytest.raises(PointNetHipError, match=msg):
            ops.semantic_icp(S, L, a["ref"], I, max_dist=MD, metric="gicp", scan_normals=a["scan_normals"])
        with pytest.raises(PointNetHipError, match=msg):
            ops.icp_gicp_sums(S, L, a["scan_normals"], a["ref"], I, MD)
    for kw in (dict(robust="huber"), dict(weights=torch.ones(B, N)), dict(robust="tukey", weights=torch.ones(B, N))):
        with pytest.raises(PointNetHipError, match="neither robust= nor weights="):
            ops.semantic_icp(S, L, R["normals"], I, max_dist=MD, metric="gicp", scan_normals=SN, **kw)
    for metric in ("point", "plane"):
        with pytest.raises(PointNetHipError, match="scan_normals goes with metric 'gicp'"):
            ops.semantic_icp(S, L, R["normals"], I, max_dist=MD, metric=metric, scan_normals=SN)
    with pytest.raises(PointNetHipError, match="'point', 'plane' or 'gicp'"):
        ops.semantic_icp(S, L, R["normals"], I, metric="line")
    with pytest.raises(PointNetHipError, match="exceeds the grid reference's max_dist=0.5"):
        ops.semantic_icp(S, L, R["grid"], I, metric="gicp", scan_normals=SN)
    with pytest.raises(PointNetHipError, match="exceeds the grid reference's max_dist=0.5"):
        ops.icp_gicp_sums(S, L, SN, R["grid"], I, 0.6)
    with pytest.raises(PointNetHipError, match="return_scale"):
        ops.semantic_icp(S, L, R["normals"], I, max_dist=MD, metric="gicp", scan_normals=SN, return_scale=True)
    assert not [c for c in calls if not c[0].endswith("_bytes")]
    src, tgt = torch.zeros(8, 3), torch.zeros(9, 3)
    for fn, lead in ((ops.register_scans, (src, tgt, 1.0)), (ops.global_register, (src, tgt, 1.0, 1.0))):
        with pytest.raises(PointNetHipError, match="'point', 'plane' or 'gicp'"):
            fn(*lead, metric="line")
        with pytest.raises(PointNetHipError, match="source_normals goes with metric 'gicp'"):
            fn(*lead, source_normals=torch.zeros(8, 3))
        with pytest.raises(PointNetHipError, match="gicp_eps= is not an argument"):
            fn(*lead, gicp_eps=0.1)
        with pytest.raises(PointNetHipError, match="robust= is not an argument"):
            fn(*lead, metric="gicp", robust="huber")


# ---- the oracle alone ------------------------------------------------------------------------------------------------
def _normal_pairs(rng, n=4000):
    """unit a and m (n, 3): random, near-parallel, parallel and antiparallel quarters"""
    a = GO.unit(rng.normal(size=(n, 3)))
    m = GO.unit(rng.normal(size=(n, 3)))
    q = n // 4
    m[q:2 * q] = GO.unit(a[q:2 * q] + 1e-5 * rng.normal(size=(q, 3)))
    m[2 * q:3 * q] = a[2 * q:3 * q]
    m[3 * q:] = -a[3 * q:]
    return a, m


@pytest.mark.parametrize("eps", [1e-3, 1e-2, 0.5])
def test_w_is_the_scaled_inverse_of_the_summed_covariances(eps):
    a, m = _normal_pairs(np.random.default_rng(0))
    W = GO.weight(a, m, eps)
    S = GO.covariance(a, eps) + GO.covariance(m, eps)
    assert np.abs(np.einsum("nab,nbc->nac", W, S) / (2 * eps) - np.eye(3)).max() <= 1e-9
    assert np.abs(W - np.swapaxes(W, 1, 2)).max() == 0 and (np.linalg.eigvalsh(W) > 0).all()


def test_w_does_not_depend_on_sign_or_length_of_a_normal():
    rng = np.random.default_rng(1)
    n = 500
    R = IO.rot(rng.normal(size=3), 0.9)
    pose = np.eye(4)
    pose[:3, :3], pose[:3, 3] = R, [3.0, -2.0, 5.0]
    p, q = rng.normal(size=(n, 3)).astype(F32), rng.normal(size=(n, 3)).astype(F32)
    nq, npn = rng.normal(size=(n, 3)).astype(F32), rng.normal(size=(n, 3)).astype(F32)
    W0 = GO.pair_terms(p, q, nq, npn, pose)[2]
    # the scalings are applied to the widened normals (3 x is not exact in fp32).  A sign or a power of two changes no bit; 3 changes
    # the unit vector by a rounding, 2.2e-16, which W amplifies by at most 1 / (2 eps) = 500: 1.1e-13, held to 1e-12
    for fq, fp in ((-1, 1), (1, -1), (-1, -1), (0.5, 1), (1, 0.5), (3, 1), (1, 3), (-3, 0.5)):
        W = GO.pair_terms(p, q, nq.astype(np.float64) * fq, npn.astype(np.float64) * fp, pose)[2]
        exact = abs(fq) != 3 and abs(fp) != 3
        assert np.abs(W - W0).max() <= (0.0 if exact else 1e-12), (fq, fp, np.abs(W - W0).max())


def test_w_at_eps_one_and_for_parallel_normals():
    rng = np.random.default_rng(2)
    a, m = _normal_pairs(rng, 400)
    assert np.abs(GO.weight(a, m, 1.0) - np.eye(3)).max() <= 1e-15
    for eps in (1e-3, 0.1):
        for sgn in (1.0, -1.0):
            W = GO.weight(a, sgn * a, eps)
            aa = a[:, :, None] * a[:, None, :]
            assert np.abs(W - (aa + eps * (np.eye(3) - aa))).max() <= 1e-14


def test_jacobian_and_gradient_by_finite_differences():
    """with W held fixed, c(x) = 1/2 sum d(x)^T W d(x) at the pose PO.apply(pose, x): J is dd/dx and sums[22:28] the gradient"""
    rng = np.random.default_rng(3)
    n = 40
    pose = np.eye(4)
    pose[:3, :3], pose[:3, 3] = IO.rot(rng.normal(size=3), 0.7), rng.normal(size=3) * 5
    q = rng.normal(size=(n, 3)) * 4
    p = (q + rng.normal(size=(n, 3)) * 0.1) @ pose[:3, :3].T + pose[:3, 3]
    nq, npn = rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
    u, d, W, _, _ = GO.pair_terms(p, q, nq, npn, pose)
    J = GO.jacobian(u)
    S = GO.assemble(u, d, W)

    def resid(x):
        P = PO.apply(pose, x)
        return GO.to_model(p - P[:3, 3], P[:3, :3]) - q

    h = 1e-6
    for i in range(6):
        e = np.zeros(6)
        e[i] = h
        dd = (resid(e) - resid(-e)) / (2 * h)
        assert np.abs(dd - J[:, :, i]).max() <= 1e-8, (i, np.abs(dd - J[:, :, i]).max())
        cost = lambda x: 0.5 * np.einsum("na,nab,nb->", resid(x), W, resid(x))          # noqa: E731
        g = (cost(e) - cost(-e)) / (2 * h)
        assert abs(g - S[22 + i]) <= 1e-6 * max(1.0, abs(S[22 + i])), (i, g, S[22 + i])
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = S[1:22]
    H = H + np.triu(H, 1).T
    assert np.abs(H - np.einsum("nai,nab,nbj->ij", J, W, J)).max() <= 1e-12 * np.abs(H).max()
    assert abs(S[28] - np.einsum("na,nab,nb->", d, W, d)) <= 1e-12 * S[28] and S[0] == n


def _analytic_normals(n_ref=3000, n_scan=6000, noise=0.02):
    """PO.aircraft_scene with PCA normals of both clouds: the reference's by PO.normals, the scan's per part the same way"""
    ref, part, scan, slab = PO.aircraft_scene(n_ref, n_scan, noise)
    na = len(PO.AIRCRAFT_PARTS)
    g, seg, _ = IO.group_reference(ref, part, na)
    nrm, _, _ = PO.normals(g, seg, na, 10)
    sg, sseg, order = IO.group_reference(scan, slab, na)
    sn = np.full(scan.shape, np.nan, F32)
    sn[order] = PO.normals(sg, sseg, na, 10)[0]
    return g, seg, nrm, scan, slab, sn


def test_oracle_loop_registers_the_analytic_scene():
    g, seg, nrm, scan, slab, sn = _analytic_normals()
    pose, rmse, pairs, iters, status = GO.icp(scan[None], slab[None], sn[None], g, seg, len(PO.AIRCRAFT_PARTS), nrm, PO.START_POSE[None],
                                              max_iters=30)
    ang, dt = IO.pose_error(pose[0], PO.TRUE_POSE)
    print(f"oracle gicp: {int(iters[0])} iterations, {np.rad2deg(ang):.4f} deg, {dt * 100:.2f} cm, rmse {rmse[0]:.4f}, pairs {int(pairs[0])}")
    assert np.rad2deg(ang) <= 0.05 and dt <= 0.05, (np.rad2deg(ang), dt)
    assert status[0] & PO.CONVERGED and not status[0] & (PO.FEW_PAIRS | PO.DEGENERATE)


@pytest.mark.parametrize("B,N", [(1, 1), (1, 777), (3, 5000)])
def test_gpu_case_inputs_are_what_they_claim(B, N):
    """tests/test_gpu_icp_gicp.py's sums case: at least a quarter of the live pairs count; where the scan is large enough to hold
    them (N >= 777: the planted scan normals; B * N = 15000: pairs onto the 25 NaN reference normals too), at least 20 pairs do not
    count for each reason, and the planted parallel / antiparallel rows reach the smallest D the case holds"""
    import gicp_cases as GC
    c = GC.sums_case(B, N)
    for max_d2 in GC.MAX_D2:
        idx, _ = IO.correspond(c["scan"], c["lab"], c["ref"], c["seg"], GC.NP, c["pose"].astype(F32), max_d2)
        live = idx >= 0
        ref_ok = np.zeros_like(live)
        ref_ok[live] = GO.valid_normal(c["nrm"][idx[live]])
        sn = c["scan_nrm"].reshape(-1, 3)
        nan_sn = ~np.isfinite(sn).all(1).reshape(B, N)
        zero_sn = (sn == 0).all(1).reshape(B, N)
        count = np.stack([GO.counted(idx[b], c["nrm"], c["scan_nrm"][b]) for b in range(B)])
        assert np.array_equal(count, live & ref_ok & ~nan_sn & ~zero_sn)
        print(f"B={B} N={N} max_d2={max_d2}: live {int(live.sum())}, counted {int(count.sum())}, NaN ref normal {int((live & ~ref_ok).sum())}, "
              f"NaN scan normal {int((live & nan_sn).sum())}, zero scan normal {int((live & zero_sn).sum())}")
        assert live.sum() >= 1 and count.sum() >= 0.25 * live.sum()
        if N >= 777:
            assert (live & nan_sn).sum() >= 20 and (live & zero_sn).sum() >= 20
        if B * N >= 15000:
            assert (live & ~ref_ok).sum() >= 20
    if N >= 777:                                   # (planted at max_d2 = 4, the tighter of the two: kept at both)
        D = []
        for b in range(B):
            k = GO.counted(idx[b], c["nrm"], c["scan_nrm"][b])
            j = idx[b][k]
            _, _, _, a, m = GO.pair_terms(c["scan"][b][k], c["ref"][j], c["nrm"][j], c["scan_nrm"][b][k], c["pose"][b])
            _, _, Ds, Df = GO.weight_parts(a, m)
            rows = np.flatnonzero(k)
            for kind, D_of in (("parallel", Ds), ("antiparallel", Df)):
                hit = np.isin(rows, dict(c["where"][kind])[b])
                assert hit.sum() >= 20 and np.abs(D_of[hit] - 2 * GO.EPS).max() <= 1e-9
            D.append(np.minimum(Ds, Df).min())
        assert min(D) <= 2 * GO.EPS * (1 + 1e-6)
