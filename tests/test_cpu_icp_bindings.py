"""Which library entry every ICP / LiDAR wrapper of ops.py calls for every kind of reference, and with which arguments, without a
GPU: the library is replaced by a recorder (sizers answer 64, everything else 0), so the wrappers run on CPU tensors up to and
including their one call.  (a) every recorded call fits its row of _lib.SIGNATURES: a bound symbol, its arity, every argument of
its slot's type; (b) the entry and the kind's trailing arguments are those of the table below.  The accelerated entries return
the brute-force bits by design, so no test that compares outputs can tell a wrapper that routes a tree or grid reference to the
brute-force entry from one that does not: this file is what pins the routing."""
import ctypes as C

import pytest
import torch

from pointcloudprocessing_amd import _lib, ops
from pointcloudprocessing_amd._lib import PointNetHipError

B, N, MD = 2, 8, 0.4
STREAM = 0x5


def _gpu_tensor_or_not(t, name, dtype=None):
    """_lib.require_gpu_tensor without its is_cuda test"""
    if not isinstance(t, torch.Tensor):
        raise PointNetHipError(f"{name} must be a CUDA/HIP tensor: the PointNet hot path has no CPU fallback")
    if not t.is_contiguous():
        raise PointNetHipError(f"{name} must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise PointNetHipError(f"{name} must have dtype {dtype}, got {t.dtype}")
    return t


@pytest.fixture
def calls(monkeypatch):
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
    monkeypatch.setattr(ops, "require_gpu_tensor", _gpu_tensor_or_not)
    return rec


def _refs():
    """the five references, built through their constructors: a 6-point cloud in two parts, without and with normals and with a
    64-byte grid table built for max_dist 0.5; a 4-triangle mesh in two parts, plain and with a 3-node tree table"""
    z, i64, i32 = torch.zeros, torch.int64, torch.int32
    return {
        "cloud": ops.IcpReference(z(6, 3), (0, 3, 6), z(6, dtype=i64), 2),
        "normals": ops.IcpReference(z(6, 3), (0, 3, 6), z(6, dtype=i64), 2, normals=z(6, 3)),
        "grid": ops.IcpGridReference(z(6, 3), (0, 3, 6), z(6, dtype=i64), 2, z(6, 3), z(64, dtype=torch.uint8), 0.5, ops._max_d2(0.5), (0, 0, 0)),
        "mesh": ops.IcpMeshReference(z(4, 3, 3), (0, 2, 4), z(4, dtype=i64), 2, z(4, 3), z(4, dtype=torch.float64)),
        "trees": ops.IcpBvhMeshReference(z(4, 3, 3), (0, 2, 4), z(4, dtype=i64), 2, z(4, 3), z(4, dtype=torch.float64), z(3, 8, dtype=i32),
                                         z(4, dtype=i32), (0, 1)),
    }


REFS = _refs()
SCAN, LABELS = torch.zeros(B, N, 3), torch.zeros(B, N, dtype=torch.int32)
P32, P64 = torch.zeros(B, 4, 4), torch.zeros(B, 4, 4, dtype=torch.float64)
WEIGHTS = torch.ones(B, N)
ROBUST = dict(robust="tukey", weights=WEIGHTS, return_scale=True)
LPOSES, DIRS = torch.zeros(B, 4, 4), torch.zeros(5, 3)


def _fits(arg, slot):
    if slot is C.c_void_p:
        return arg is None or isinstance(arg, C.c_void_p)
    if slot is C.POINTER(C.c_int32):
        return isinstance(arg, C.Array) and arg._type_ is C.c_int32
    if slot in (C.c_int, C.c_size_t, C.c_uint64):
        return type(arg) is int
    if slot in (C.c_float, C.c_double):
        return type(arg) is float
    return False


def _conforms(name, args):
    assert name in _lib.SIGNATURES, name
    slots = _lib.SIGNATURES[name][1]
    assert len(args) == len(slots), (name, len(args), len(slots))
    for k, (arg, slot) in enumerate(zip(args, slots)):
        assert _fits(arg, slot), (name, k, arg, slot)


def _one_call(calls, wrapper):
    """run the wrapper -> the one call it makes that is not a sizer's; every call it makes conforms to SIGNATURES"""
    del calls[:]
    wrapper()
    for name, args in calls:
        _conforms(name, args)
    entries = [(name, args) for name, args in calls if not name.endswith("_bytes")]
    assert len(entries) == 1, [name for name, _ in calls]
    return entries[0]


def _addr(arg):
    return None if arg is None else arg.value


def _tail(ref):
    """the trailing arguments of a kind's accelerated entries, as plain values"""
    return {"grid": lambda: (REFS["grid"].grid.data_ptr(), REFS["grid"].r2),
            "trees": lambda: (REFS["trees"].nodes.data_ptr(), REFS["trees"].rows.data_ptr(), [0, 1], 3)}.get(ref, tuple)()


def _plain(args):
    return tuple(_addr(a) if isinstance(a, C.c_void_p) else list(a) if isinstance(a, C.Array) else a for a in args)


def _check_icp_call(kind, name, args, entry, trailing=()):
    """an ICP entry's call: its name, the reference's head (primitives, seg, count, n_parts), the trailing arguments, the stream"""
    ref = REFS[kind]
    assert name == entry, (kind, name, entry)
    prim = ref.tri if kind in ("mesh", "trees") else ref.xyz
    assert _plain(args[:8]) == (SCAN.data_ptr(), LABELS.data_ptr(), B, N, prim.data_ptr(), list(ref.seg), ref.seg[-1], 2), (kind, name)
    n = len(trailing)
    assert _plain(args[len(args) - 1 - n:]) == tuple(trailing) + (STREAM,), (kind, name, _plain(args[-1 - n:]))


# wrapper, kind -> entry; the kinds a wrapper refuses are listed with None
PASSES = [
    ("icp_correspond", "cloud", "pn_icp_correspond"), ("icp_correspond", "normals", "pn_icp_correspond"),
    ("icp_correspond", "grid", "pn_icp_grid_correspond"), ("icp_correspond", "mesh", None), ("icp_correspond", "trees", None),
    ("icp_plane_sums", "normals", "pn_icp_plane_sums"), ("icp_plane_sums", "grid", "pn_icp_grid_correspond"),
    ("icp_plane_sums", "cloud", None), ("icp_plane_sums", "mesh", None), ("icp_plane_sums", "trees", None),
    ("icp_mesh_correspond", "mesh", "pn_icp_mesh_correspond"), ("icp_mesh_correspond", "trees", "pn_icp_bvh_correspond"),
    ("icp_mesh_correspond", "cloud", None), ("icp_mesh_correspond", "grid", None),
]


@pytest.mark.parametrize("wrapper,kind,entry", PASSES)
def test_single_pass_entries(calls, wrapper, kind, entry):
    ref = REFS[kind]
    variants = {"icp_correspond": [(dict(sums=False), 0, P32), (dict(sums=True), 1, P32)], "icp_plane_sums": [(dict(), 2, P64)],
                "icp_mesh_correspond": [(dict(sums=None), 0, P64), (dict(sums="point"), 1, P32), (dict(sums="plane"), 2, P64)]}[wrapper]
    for kw, mode, pose in variants:
        run = lambda: getattr(ops, wrapper)(SCAN, LABELS, ref, pose, MD, **kw)        # noqa: E731
        if entry is None:
            del calls[:]
            with pytest.raises(PointNetHipError, match="ref must come from|needs reference normals"):
                run()
            assert not calls or kind == "cloud"                   # a family refusal comes before any call, a sizer's included
            continue
        name, args = _one_call(calls, run)
        _check_icp_call(kind, name, args, entry, _tail(kind))
        assert args[9] == ops._max_d2(MD)
        if name not in ("pn_icp_correspond", "pn_icp_plane_sums"):                    # the general argument list carries the mode
            assert args[10] == mode, (wrapper, kind, kw)
            normals = ref.normals.data_ptr() if mode == 2 or kind in ("mesh", "trees") else None
            assert _addr(args[11]) == normals and (args[12] is None) == (mode != 2)
            assert (args[15] is None) == (kind == "grid") and (args[16] is None) == (mode == 0)
        elif name == "pn_icp_plane_sums":
            assert _addr(args[10]) == ref.normals.data_ptr() and _addr(args[11]) == P64.data_ptr()


LOOPS = [("cloud", "point", "pn_semantic_icp"), ("normals", "point", "pn_semantic_icp"), ("normals", "plane", "pn_semantic_icp_plane"),
         ("grid", "point", "pn_semantic_icp_grid"), ("grid", "plane", "pn_semantic_icp_grid"),
         ("mesh", "point", "pn_semantic_icp_mesh"), ("mesh", "plane", "pn_semantic_icp_mesh"),
         ("trees", "point", "pn_semantic_icp_bvh"), ("trees", "plane", "pn_semantic_icp_bvh")]


@pytest.mark.parametrize("kind,metric,entry", LOOPS)
def test_loop_entries(calls, kind, metric, entry):
    ref = REFS[kind]
    name, args = _one_call(calls, lambda: ops.semantic_icp(SCAN, LABELS, ref, P32, 7, MD, 1e-5, 1e-4, metric=metric))
    _check_icp_call(kind, name, args, entry, _tail(kind))
    plane = metric == "plane"
    if name in ("pn_semantic_icp", "pn_semantic_icp_plane"):
        assert args[9:13] == (7, ops._max_d2(MD), 1e-5, 1e-4) and _addr(args[8]) == _addr(args[13 + plane])
        assert not plane or _addr(args[13]) == ref.normals.data_ptr()
    else:
        normals = ref.normals.data_ptr() if plane or kind in ("mesh", "trees") else None
        assert _addr(args[8]) == normals and args[9] == (2 if plane else 1) and args[11:15] == (7, ops._max_d2(MD), 1e-5, 1e-4)
        assert _addr(args[10]) == _addr(args[15])                                      # the pose is refined in place


@pytest.mark.parametrize("kind", ["cloud", "normals", "grid", "mesh", "trees"])
@pytest.mark.parametrize("metric", ["point", "plane"])
def test_robust_entries(calls, kind, metric):
    ref = REFS[kind]
    mesh = kind in ("mesh", "trees")
    loop = lambda **kw: ops.semantic_icp(SCAN, LABELS, ref, P64, 7, MD, metric=metric, **kw)                         # noqa: E731
    sums = lambda: ops.icp_robust_sums(SCAN, LABELS, ref, P64, MD, metric=metric, weights=WEIGHTS, robust="huber")   # noqa: E731
    if kind in ("grid", "trees") or (kind == "cloud" and metric == "plane"):
        msg = "needs reference normals" if kind == "cloud" else "accel=None"
        for run in (lambda: loop(**ROBUST), lambda: loop(weights=WEIGHTS), lambda: loop(robust="huber"), sums):
            with pytest.raises(PointNetHipError, match=msg):
                run()
        return
    normals = ref.normals.data_ptr() if metric == "plane" else None
    for kw in (ROBUST, dict(weights=WEIGHTS), dict(robust="huber")):
        name, args = _one_call(calls, lambda: loop(**kw))
        _check_icp_call(kind, name, args, "pn_semantic_icp_robust")
        assert args[8] == int(mesh) and _addr(args[9]) == normals and args[10] == (2 if metric == "plane" else 1)
        assert args[16] == ops.ROBUST_KERNELS[kw.get("robust")] and _addr(args[20]) == (WEIGHTS.data_ptr() if "weights" in kw else None)
    name, args = _one_call(calls, sums)
    _check_icp_call(kind, name, args, "pn_icp_robust_sums")
    assert args[8] == int(mesh) and _addr(args[9]) == normals and args[10] == (2 if metric == "plane" else 1)
    assert _addr(args[12]) == P64.data_ptr() and args[13] == ops._max_d2(MD) and args[14] == ops.ROBUST_KERNELS["huber"]


@pytest.mark.parametrize("kind", ["mesh", "trees"])
def test_lidar_entries(calls, kind):
    ref = REFS[kind]
    head = (ref.tri.data_ptr(), [0, 2, 4], 4, 2, LPOSES.data_ptr(), B, DIRS.data_ptr(), 5, 0.25, 9.0)
    name, args = _one_call(calls, lambda: ops.lidar_cast(ref, LPOSES, DIRS, 0.25, 9.0))
    assert name == "pn_lidar_cast" and _plain(args[:10]) == head and _plain(args[12:]) == (STREAM,)    # whatever the reference's kind
    if kind == "mesh":
        del calls[:]
        with pytest.raises(PointNetHipError, match=r'icp_mesh_reference\(\.\.\., accel="bvh"\)'):
            ops.lidar_cast(ref, LPOSES, DIRS, accel="bvh")
        assert not calls
        return
    name, args = _one_call(calls, lambda: ops.lidar_cast(ref, LPOSES, DIRS, 0.25, 9.0, accel="bvh"))
    assert name == "pn_lidar_cast_bvh" and _plain(args[:10]) == head and _plain(args[12:]) == _tail("trees") + (STREAM,)


@pytest.mark.parametrize("kind", ["cloud", "grid", "mesh", "trees"])
def test_score_poses_entry(calls, kind):
    ref = REFS[kind]
    poses = torch.zeros(B, 3, 4, 4, dtype=torch.float64)
    name, args = _one_call(calls, lambda: ops.icp_score_poses(SCAN, LABELS, ref, poses, MD, 2))
    assert name == "pn_icp_score_poses"
    if kind in ("mesh", "trees"):                       # the (3T, 3) vertex view of the triangles: no copy, offsets 3 * seg
        assert _plain(args[4:8]) == (ref.tri.data_ptr(), [0, 6, 12], 12, 2)
    else:
        assert _plain(args[4:8]) == (ref.xyz.data_ptr(), [0, 3, 6], 6, 2)
    assert _plain(args[8:12]) == (poses.data_ptr(), 3, 2, ops._max_d2(MD)) and _addr(args[-1]) == STREAM
