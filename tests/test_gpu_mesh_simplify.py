"""pn_mesh_components and pn_mesh_simplify on the MI355X against the NumPy oracle (tests/mesh_simplify_oracle.py, whose own facts
tests/test_cpu_mesh_simplify.py checks), through the raw C ABI on guard-banded, pattern-filled outputs and workspaces.  Everything is
compared bit for bit: the two counts, the faces, the labels, the bits of every vertex coordinate, the component ids and sizes -- the
header fixes the order of every fp64 operation and forbids contraction, and the oracle follows it.

Which path a case reaches:
  F = 1, 255, 256, 257     one workgroup of faces and the first face of a second; 3F = 3 .. 771 corners, one to four workgroups
  soup 2,000 / sphere      several workgroups of both kinds, repeated indices, repeated faces, rank-3 clusters
  spikes 1, 64, 65, 256, 257   one cluster whose corner list has exactly that many entries (a wave, a wave and one, a workgroup, ...)
  cube, grid               rank-3 corners, rank-2 edges, rank-1 faces; a flat grid (rank 1, r = 0)
  rank_tol = 0 on spikes   the fallback to the mean (a position more than a leaf from it)
  sphere 210 x 210         3F = 263,340 > 2^18: the sort changes its tile shape; corner lists of thousands
  strip 5,000, interleaved shells   the union-find's long chain and components that are contiguous in neither table"""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_simplify_oracle as MO

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 4096
PAT = 0xA5


def _t(a, dev="cuda:0"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _guarded(nbytes, dev, fill=PAT):
    buf = torch.full((GUARD + nbytes + GUARD,), PAT, dtype=torch.uint8, device=dev)
    buf[GUARD:GUARD + nbytes] = fill
    return buf, buf[GUARD:GUARD + nbytes]


def _finish(bufs, keep, ins, expect_error):
    torch.cuda.synchronize()
    for name, (buf, _) in bufs.items():
        assert bool((buf[:GUARD] == PAT).all()) and bool((buf[-GUARD:] == PAT).all()), f"{name}: guard band overwritten"
    for a, b in zip(keep, ins):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "an input was modified"
    assert int(bufs["ws"][1][:4].view(torch.int32).item()) == expect_error, "error word"


def _f3(v):
    return (C.c_float * 3)(*[float(a) for a in v])


def _raw_simplify(v, f, leaf, origin, labels=None, placement="quadric", rank_tol=1e-3, ws_fill=PAT, expect_error=0, dev="cuda:0"):
    """pn_mesh_simplify through the C ABI -> (vertices (V', 3) f32, faces (F', 3) i32, labels (F',) or None, the whole output
    buffers as bytes); with ``expect_error`` only the error word and the guards are checked"""
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    vt, ft = _t(np.asarray(v, F32), dev), _t(np.asarray(f, np.int32), dev)
    lt = None if labels is None else _t(np.asarray(labels, np.int32), dev)
    ins = [vt, ft] + ([] if lt is None else [lt])
    keep = [x.clone() for x in ins]
    V, Fc = vt.shape[0], ft.shape[0]
    nbytes = L.pn_mesh_simplify_workspace_bytes(Fc)
    assert nbytes > 0
    bufs = dict(v=_guarded(12 * min(V, 3 * Fc), dev), f=_guarded(12 * Fc, dev), n=_guarded(8, dev), ws=_guarded(nbytes, dev, ws_fill))
    if lt is not None:
        bufs["l"] = _guarded(4 * Fc, dev)
    p = lambda k: C.c_void_p(bufs[k][1].data_ptr()) if k in bufs else None            # noqa: E731
    rc = L.pn_mesh_simplify(_lib.ptr(vt), V, _lib.ptr(ft), _lib.ptr(lt), Fc, _f3(leaf), _f3(origin), {"mean": 0, "quadric": 1}[placement],
                            float(rank_tol), p("v"), p("f"), p("l"), p("n"), p("ws"), nbytes, _lib.current_stream())
    _lib.check(rc, "pn_mesh_simplify")
    _finish(bufs, keep, ins, expect_error)
    if expect_error:
        return None
    nv, nf = (int(x) for x in bufs["n"][1].view(torch.int32).cpu().tolist())
    assert 0 <= nv <= min(V, 3 * Fc) and 0 <= nf <= Fc
    raw = {k: bufs[k][1].cpu().numpy().copy() for k in bufs if k != "ws"}
    for k, n in (("v", 12 * nv), ("f", 12 * nf), ("l", 4 * nf)):
        assert k not in raw or (raw[k][n:] == PAT).all(), f"{k}: written past the count"
    return (raw["v"][:12 * nv].view(F32).reshape(nv, 3), raw["f"][:12 * nf].view(np.int32).reshape(nf, 3),
            raw["l"][:4 * nf].view(np.int32) if "l" in raw else None, raw)


def _raw_components(v, f, capacity=None, ws_fill=PAT, expect_error=0, dev="cuda:0"):
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    vt, ft = _t(np.asarray(v, F32), dev), _t(np.asarray(f, np.int32), dev)
    keep = [vt.clone(), ft.clone()]
    V, Fc = vt.shape[0], ft.shape[0]
    cap = min(V, Fc) if capacity is None else capacity
    nbytes = L.pn_mesh_components_workspace_bytes(V)
    bufs = dict(c=_guarded(4 * Fc, dev), s=_guarded(4 * cap, dev), n=_guarded(4, dev), ws=_guarded(nbytes, dev, ws_fill))
    p = lambda k: C.c_void_p(bufs[k][1].data_ptr())                                   # noqa: E731
    rc = L.pn_mesh_components(_lib.ptr(vt), V, _lib.ptr(ft), Fc, p("c"), p("s"), cap, p("n"), p("ws"), nbytes, _lib.current_stream())
    _lib.check(rc, "pn_mesh_components")
    _finish(bufs, keep, [vt, ft], expect_error)
    K = int(bufs["n"][1].view(torch.int32).item())
    sizes = bufs["s"][1].view(torch.int32).cpu().numpy()
    assert (sizes[min(K, cap):].view(np.uint8) == PAT).all()
    return bufs["c"][1].view(torch.int32).cpu().numpy(), sizes[:min(K, cap)], K


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _compare(name, got, o):
    v, f, lab, _ = got
    print(f"{name}: {o['n_clusters']} clusters (longest list {o['max_corners']}), V' = {len(v)} / {len(o['vertices'])}, F' = {len(f)} / "
          f"{len(o['faces'])}, ranks {np.bincount(o['rank'], minlength=4).tolist()}, fallbacks {int(o['fallback'].sum())}")
    assert (len(v), len(f)) == (len(o["vertices"]), len(o["faces"])), name
    assert np.array_equal(f, o["faces"]), (name, np.flatnonzero((f != o["faces"]).any(1))[:5])
    assert (lab is None) == (o["labels"] is None) and (lab is None or np.array_equal(lab, o["labels"])), name
    diff = np.flatnonzero((_bits(v) != _bits(o["vertices"])).any(1))
    if len(diff):
        print(f"{name}: {len(diff)} vertices differ, max |dv| = {np.abs(v.astype(np.float64) - o['vertices']).max():.3e}, first {diff[:5]}")
    assert len(diff) == 0, name


def _with_specials(v, f, seed):
    """+ a face whose three corners are one vertex, and copies of face 0 in both orientations (a rotation, a flip, a plain copy)"""
    f = np.asarray(f, np.int32)
    a, b, c = f[0]
    extra = np.array([(a, a, a), (b, c, a), (a, c, b), (c, b, a), (a, b, c)], np.int32)
    at = np.random.default_rng(seed).integers(1, len(f) + 1, len(extra))
    return v, np.insert(f, np.sort(at), extra, 0)


def _cases():
    one = (1.0, 1.0, 1.0)
    out = {}
    for n in (1, 255, 256, 257):
        out[f"soup{n}"] = (*MO.soup_mesh(40, n, seed=n, extent=3.0), one, (0.0, 0.0, 0.0))
    out["soup2000"] = (*_with_specials(*MO.soup_mesh(300, 2000, seed=1), 3), one, (0.0, 0.0, 0.0))
    out["sphere"] = (*_with_specials(*MO.sphere_mesh(24, 48, 3.0, (4.0, 4.0, 4.0)), 4), (0.7, 0.7, 0.7), (0.0, 0.0, 0.0))
    out["sphere_aniso"] = (*MO.sphere_mesh(24, 48, 3.0, (4.0, 4.0, 4.0)), (0.5, 0.9, 1.3), (0.25, -0.5, 0.125))
    out["cube"] = (*_with_specials(*MO.cube_mesh(8, 1.0, (0.13, 0.21, 0.17)), 5), (0.3, 0.3, 0.3), (0.0, 0.0, 0.0))
    out["grid"] = (*MO.grid_mesh(20, 23, 1.0, 0.37), (3.0, 3.0, 3.0), (-0.5, -0.5, -0.5))
    for n in (1, 64, 65, 256, 257):
        out[f"spike{n}"] = (*MO.spike_mesh(n, seed=n), one, (0.0, -2.0, 0.0))
    return out


CASES = _cases()
_ORACLE = {}


def _oracle(name, placement, rank_tol, labelled):
    key = (name, placement, rank_tol, labelled)
    if key not in _ORACLE:
        v, f, leaf, origin = CASES[name]
        lab = (np.arange(len(f)) * 7 % 11).astype(np.int32) if labelled else None
        _ORACLE[key] = (lab, MO.simplify(v, f, leaf, origin, lab, placement, rank_tol))
    return _ORACLE[key]


@pytest.mark.parametrize("placement", ["mean", "quadric"])
@pytest.mark.parametrize("name", list(CASES))
def test_simplify_against_oracle(dev, name, placement):
    v, f, leaf, origin = CASES[name]
    labelled = name not in ("sphere_aniso", "soup255")                   # labels present and absent
    for rank_tol in ((1e-3, 0.0) if placement == "quadric" and name.startswith(("spike", "soup2000")) else (1e-3,)):
        lab, o = _oracle(name, placement, rank_tol, labelled)
        _compare(f"{name} {placement} {rank_tol}", _raw_simplify(v, f, leaf, origin, lab, placement, rank_tol, dev=dev), o)
    if name == "spike257" and placement == "quadric":
        assert _oracle(name, placement, 0.0, labelled)[1]["fallback"].any()      # the fallback to the mean is among what was compared
    if name == "cube" and placement == "quadric":
        assert set(np.unique(o["rank"])) == {1, 2, 3}
    if name.startswith("spike"):
        assert o["max_corners"] == int(name[5:])
    if name == "soup2000":
        assert len(o["kept"]) < len(f) - 5                                # the specials and the soup's own repeats are dropped


def test_sort_tile_change_above_2_to_the_18_corners(dev):
    v, f = MO.sphere_mesh(210, 210, 10.0, (11.0, 11.0, 11.0))
    assert 3 * len(f) > (1 << 18) >= 3 * len(f) - 3000
    leaf, origin = (0.9, 0.9, 0.9), (0.0, 0.0, 0.0)
    lab = (np.arange(len(f)) % 5).astype(np.int32)
    for placement in ("mean", "quadric"):
        _compare(f"sphere 210 x 210 {placement}", _raw_simplify(v, f, leaf, origin, lab, placement, dev=dev),
                 MO.simplify(v, f, leaf, origin, lab, placement))


def test_every_face_collapses(dev):
    v, f = MO.cube_mesh(4)
    for placement in ("mean", "quadric"):
        gv, gf, gl, _ = _raw_simplify(v, f, (100.0, 100.0, 100.0), (-1.0, -1.0, -1.0), np.zeros(len(f), np.int32), placement, dev=dev)
        assert len(gv) == 0 and len(gf) == 0 and len(gl) == 0
    gv, gf, _, _ = _raw_simplify(v[:1], np.zeros((1, 3), np.int32), (1.0, 1.0, 1.0), (-1.0, -1.0, -1.0), dev=dev)   # F = 1, one vertex three times
    assert len(gv) == 0 and len(gf) == 0


def test_duplicates_in_both_orientations(dev):
    v = np.array([(0.5, 0.5, 0.5), (2.5, 0.5, 0.5), (0.5, 2.5, 0.5), (0.6, 0.4, 0.5)], F32)       # vertex 3 shares vertex 0's cell
    f = np.array([(0, 1, 2), (1, 2, 0), (0, 2, 1), (2, 1, 3), (3, 1, 2), (0, 0, 1), (2, 0, 1)], np.int32)
    lab = np.arange(10, 17, dtype=np.int32)
    gv, gf, gl, _ = _raw_simplify(v, f, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), lab, "mean", dev=dev)
    # cells ascend (0,0,0) < (2,0,0) < (0,2,0) in (kz, ky, kx): ranks 0, 1, 2.  Face 0 stays; 1 and 4 and 6 are its rotations; 2 is
    # the opposite orientation and stays; 3 = (2, 1, 0) is a rotation of 2; 5 has two corners in one cell
    assert gf.tolist() == [[0, 1, 2], [0, 2, 1]] and gl.tolist() == [10, 12] and len(gv) == 3


def test_purity_dirty_workspace_and_repeat(dev):
    v, f, leaf, origin = CASES["sphere"]
    lab = (np.arange(len(f)) % 3).astype(np.int32)
    runs = [_raw_simplify(v, f, leaf, origin, lab, "quadric", ws_fill=fill, dev=dev)[3] for fill in (PAT, 0x00, 0xFF, PAT)]
    for r in runs[1:]:
        assert all(np.array_equal(r[k], runs[0][k]) for k in runs[0])
    sv, sf = MO.strip_mesh(5000)
    outs = [_raw_components(sv, sf, ws_fill=fill, dev=dev) for fill in (PAT, 0x00, 0xFF)]
    assert all(np.array_equal(o[0], outs[0][0]) and np.array_equal(o[1], outs[0][1]) and o[2] == outs[0][2] for o in outs)


def test_error_words_and_memory_safety(dev):
    v, f, leaf, origin = CASES["sphere"]
    for bad in (-1, len(v), 2 ** 31 - 1, -2 ** 31):
        g = f.copy()
        g[len(g) // 2, 1] = bad
        _raw_simplify(v, g, leaf, origin, expect_error=MO.ERR_INDEX, dev=dev)
        comp, _, _ = _raw_components(v, g, expect_error=MO.ERR_INDEX, dev=dev)
        assert comp[len(g) // 2] == -1
    for bad in (np.nan, np.inf, -np.inf):
        w = v.copy()
        w[int(f[7, 2]), 1] = bad
        _raw_simplify(w, f, leaf, origin, expect_error=MO.ERR_NONFINITE, dev=dev)
    w = np.concatenate((v, [[np.nan, 0.0, 0.0]])).astype(F32)                    # a non-finite vertex that no face refers to is not an error
    _compare("unreferenced NaN", _raw_simplify(w, f, leaf, origin, dev=dev), MO.simplify(v, f, leaf, origin))
    _raw_simplify(v, f, leaf, (5.0, 0.0, 0.0), expect_error=MO.ERR_KEY, dev=dev)          # a vertex below the origin
    comp, sizes, K = _raw_components(*MO.interleave([MO.cube_mesh(2), MO.cube_mesh(2), MO.cube_mesh(2)])[:2], capacity=2,
                                     expect_error=MO.ERR_CAPACITY, dev=dev)
    assert K == 3 and sizes.tolist() == [48, 48]                      # 6 sides x 2 x 2 squares x 2 triangles each


def test_the_cluster_limit_sets_its_error_word(dev):
    """2^21 + 1 corners, each in a voxel of its own (699,051 faces over 2,097,153 vertices on a 2048-wide sheet): one cluster more
    than a rank triple can hold.  The limit is on the number of occupied cells, which only the device counts: no argument reaches
    it, so the mesh is built (NumPy arange and stack; about 0.07 s for both calls on the MI355X, the buffers some 200 MB).  Only the
    error word and the guards are checked; three corners fewer, and the call is a plain renumbering"""
    n = (1 << 21) + 1
    i = np.arange(n)
    v = np.stack((i % 2048 + 0.5, i // 2048 + 0.5, np.full(n, 0.5)), 1).astype(F32)
    f = i.astype(np.int32).reshape(-1, 3)
    _raw_simplify(v, f, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), placement="mean", expect_error=MO.ERR_CLUSTERS, dev=dev)
    gv, gf, _, _ = _raw_simplify(v[:-3], f[:-1], (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), placement="mean", dev=dev)      # 2^21 - 2 clusters: fine
    assert len(gv) == n - 3 and np.array_equal(gf, f[:-1])


def test_components_against_oracle(dev):
    cases = {"strip": MO.strip_mesh(5000), "interleaved": MO.interleave([MO.cube_mesh(3), MO.sphere_mesh(5, 6), MO.strip_mesh(40)])[:2],
             "soup": MO.soup_mesh(3000, 1500, seed=9), "one face": (np.zeros((3, 3), F32), np.array([[2, 2, 2]], np.int32))}
    for n in (255, 256, 257):
        cases[f"soup{n}"] = MO.soup_mesh(700, n, seed=n)
    for name, (v, f) in cases.items():
        comp, sizes, K = _raw_components(v, f, dev=dev)
        ec, es = MO.components(len(v), f)
        print(f"{name}: {K} components, sizes {es[:6].tolist()}")
        assert K == len(es) and np.array_equal(comp, ec) and np.array_equal(sizes, es), name
    assert _raw_components(*cases["strip"], dev=dev)[2] == 1
    assert _raw_components(*cases["interleaved"], dev=dev)[1].tolist() == [108, 48, 40]


def _captured(run):
    """``run`` eagerly and from a captured graph on one stream -> (the eager outputs, the replayed ones, cleared before the replay)"""
    eager = run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
        with torch.cuda.graph(g, stream=side):
            captured = run()
    torch.cuda.current_stream().wait_stream(side)
    for x in captured:
        x.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    return eager, captured


def test_graph_capture_of_both_entries(dev):
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    v, f, leaf, origin = CASES["sphere"]
    lab = (np.arange(len(f)) % 3).astype(np.int32)
    vt, ft, lt = _t(v, dev), _t(f, dev), _t(lab, dev)
    V, Fc = len(v), len(f)
    sbytes, cbytes = L.pn_mesh_simplify_workspace_bytes(Fc), L.pn_mesh_components_workspace_bytes(V)
    ws_s = torch.empty(sbytes, dtype=torch.uint8, device=dev)
    ws_c = torch.empty(cbytes, dtype=torch.uint8, device=dev)

    def simplify():
        vo = torch.zeros(min(V, 3 * Fc), 3, device=dev)
        fo = torch.zeros(Fc, 3, device=dev, dtype=torch.int32)
        lo = torch.zeros(Fc, device=dev, dtype=torch.int32)
        n = torch.zeros(2, device=dev, dtype=torch.int32)
        _lib.check(L.pn_mesh_simplify(_lib.ptr(vt), V, _lib.ptr(ft), _lib.ptr(lt), Fc, _f3(leaf), _f3(origin), 1, 1e-3, _lib.ptr(vo), _lib.ptr(fo),
                                      _lib.ptr(lo), _lib.ptr(n), _lib.ptr(ws_s), sbytes, _lib.current_stream()), "pn_mesh_simplify")
        return vo, fo, lo, n

    eager, replayed = _captured(simplify)
    assert all(np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8)) for a, b in zip(eager, replayed))
    o = MO.simplify(v, f, leaf, origin, lab)
    nv, nf = replayed[3].tolist()
    assert (nv, nf) == (len(o["vertices"]), len(o["faces"])) and np.array_equal(replayed[1][:nf].cpu().numpy(), o["faces"])
    assert np.array_equal(_bits(replayed[0][:nv].cpu().numpy()), _bits(o["vertices"]))

    def components():
        c = torch.zeros(Fc, device=dev, dtype=torch.int32)
        s = torch.zeros(min(V, Fc), device=dev, dtype=torch.int32)
        n = torch.zeros(1, device=dev, dtype=torch.int32)
        _lib.check(L.pn_mesh_components(_lib.ptr(vt), V, _lib.ptr(ft), Fc, _lib.ptr(c), _lib.ptr(s), min(V, Fc), _lib.ptr(n), _lib.ptr(ws_c), cbytes,
                                        _lib.current_stream()), "pn_mesh_components")
        return c, s, n

    eager, replayed = _captured(components)
    assert all(np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8)) for a, b in zip(eager, replayed))
    ec, es = MO.components(V, f)
    assert replayed[2].item() == len(es) and np.array_equal(replayed[0].cpu().numpy(), ec)
    assert int(ws_s[:4].view(torch.int32).item()) == 0 and int(ws_c[:4].view(torch.int32).item()) == 0


# ---- the ops level ------------------------------------------------------------------------------------------------------
def test_ops_simplify_and_components(dev):
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd._lib import PointNetHipError
    v, f, leaf, origin = CASES["sphere"]
    lab = (np.arange(len(f)) % 3).astype(np.int32)
    for placement in ("mean", "quadric"):
        o = MO.simplify(v, f, leaf, origin, lab, placement)
        gv, gf, gl = ops.simplify_mesh(_t(v, dev), _t(f, dev), leaf[0], _t(lab, dev), placement, origin)
        assert np.array_equal(gf.cpu().numpy(), o["faces"]) and np.array_equal(gl.cpu().numpy(), o["labels"])
        assert np.array_equal(_bits(gv.cpu().numpy()), _bits(o["vertices"]))
    # the default origin is the minimum of the finite vertices; a face with a non-finite vertex is dropped before the call
    w, g = np.concatenate((v, [[np.nan, 1.0, 1.0]])).astype(F32), np.concatenate((f[:100], [[0, 1, len(v)]], f[100:])).astype(np.int32)
    gv, gf, gl = ops.simplify_mesh(_t(w, dev), _t(g, dev), leaf)
    o = MO.simplify(v, f, leaf, v.min(0))
    assert gl is None and np.array_equal(gf.cpu().numpy(), o["faces"]) and np.array_equal(_bits(gv.cpu().numpy()), _bits(o["vertices"]))
    bad = f.copy()
    bad[5, 0] = len(v)
    with pytest.raises(PointNetHipError, match=r"face index is outside \[0, "):
        ops.simplify_mesh(_t(v, dev), _t(bad, dev), leaf)
    with pytest.raises(PointNetHipError, match=r"face index is outside \[0, "):
        ops.mesh_components(_t(v, dev), _t(bad, dev))
    with pytest.raises(PointNetHipError, match="placement"):
        ops.simplify_mesh(_t(v, dev), _t(f, dev), leaf, placement="median")
    # components -> cluster_mask, unchanged
    mv, mf, src = MO.interleave([MO.cube_mesh(3), MO.sphere_mesh(5, 6), MO.strip_mesh(40)])
    comp, sizes = ops.mesh_components(_t(mv, dev), _t(mf, dev))
    assert sizes.tolist() == [108, 48, 40] and np.array_equal(comp.cpu().numpy(), src)
    assert np.array_equal(ops.cluster_mask(comp, sizes).cpu().numpy(), src == 0)
    assert np.array_equal(ops.cluster_mask(comp, sizes, keep="all", min_points=45).cpu().numpy(), src != 2)
    cv, cf, cl = ops.clean_mesh(_t(mv, dev), _t(mf, dev), _t(src, dev), clean=dict(keep="all", min_faces=45))
    assert len(cf) == 156 and len(cv) == len(mv) - 42 and int(cf.max()) == len(cv) - 1 and set(cl.tolist()) == {0, 1}
    assert np.array_equal(cv.cpu().numpy()[cf.cpu().numpy()], mv[mf[src != 2]])          # the same triangles, renumbered
    same = ops.clean_mesh(_t(mv, dev), _t(mf, dev))
    assert same[2] is None and np.array_equal(same[0].cpu().numpy(), mv) and np.array_equal(same[1].cpu().numpy(), mf)


def test_simplified_aircraft_in_the_robust_mesh_loop(dev):
    """The aircraft of the mesh ICP tests at level 5 (81,920 triangles, a triangle soup) simplified at a 0.25 m leaf -- below the
    thickness of its thinnest slab (the tailplane, 0.3 m), so the two sides of a slab mostly keep cells of their own -- and used as the
    mesh reference of the robust loop, which searches a mesh by brute force only: a 1,024-point scan of the FULL mesh (2 cm noise,
    a fifth of its labels replaced) from 4 degrees and about 0.5 m off, the start of the robust loop's own tests.  The loop must
    end where tests/test_gpu_icp_mesh.py::test_loop_against_oracle holds the plane loop on the full mesh: within 1e-3 rad and
    5e-3 m of the truth, with either placement."""
    import icp_mesh_oracle as IM
    import icp_oracle as IO
    import icp_plane_oracle as PO
    import icp_robust_oracle as RO
    from pointcloudprocessing_amd import ops
    NM, LEVEL, LEAF = len(IM.MESH_PARTS), 5, 0.25
    v, f, p = IM.aircraft_mesh(LEVEL)
    scan, lab = IM.mesh_scan(v, f, p, 1024, PO.TRUE_POSE, noise=0.02, seed=31)
    lab = RO.wrong_labels(lab, NM, 0.2, 50)
    rng = np.random.default_rng(60)
    init = PO.TRUE_POSE.copy()
    init[:3, :3] = IO.rot(rng.normal(size=3), np.deg2rad(4)) @ init[:3, :3]
    init[:3, 3] += rng.normal(size=3) * 0.25
    a0, t0 = IO.pose_error(init, PO.TRUE_POSE)
    for placement in ("quadric", "mean"):
        sv, sf, sl = ops.simplify_mesh(_t(v, dev), _t(f, dev), LEAF, _t(p, dev), placement)
        assert 0 < len(sf) < len(f) // 2 and len(torch.unique(sl)) == NM
        ref = ops.icp_mesh_reference(sv, sf, sl, NM)
        g = ops.semantic_icp(_t(scan[None], dev), _t(lab[None], dev), ref, _t(init[None], dev), max_dist=3.0, metric="plane", robust="tukey",
                             max_iters=30, tol_rot=1e-6, tol_t=1e-6)
        a1, t1 = IO.pose_error(g[0][0].cpu().numpy(), PO.TRUE_POSE)
        print(f"leaf {LEAF} {placement}: {len(f)} -> {len(sf)} faces ({ref.T} in the reference), {len(v)} -> {len(sv)} vertices; start "
              f"{np.rad2deg(a0):.3f} deg {t0:.3f} m -> end {a1:.3e} rad {t1:.4f} m after {int(g[3][0])} iterations")
        assert a1 < 1e-3 and t1 < 5e-3, (placement, a1, t1)


def test_clean_and_simplify_a_reconstruction_with_a_planted_blob(dev):
    """The sphere of the reconstruction tests plus a small ball of points well away from it: the plain reconstruction has two
    shells, clean= keeps the large one, simplify= returns fewer faces than the plain call"""
    import recon_oracle as RO
    from pointcloudprocessing_amd import ops
    c = RO.solved("sphere")
    rng = np.random.default_rng(5)
    d = rng.normal(size=(60, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    centre = c["xyz"].max(0) + 4 * c["radius"]
    xyz = np.concatenate((c["xyz"], centre + 0.3 * d)).astype(F32)
    nrm = np.concatenate((c["normals"], d)).astype(F32)
    lab = np.concatenate((np.zeros(len(c["xyz"]), np.int32), np.ones(len(d), np.int32)))
    v, f, fl = ops.reconstruct_mesh(_t(xyz, dev), _t(nrm, dev), c["voxel"], c["radius"], labels=_t(lab, dev), n_labels=2)
    comp, sizes = ops.mesh_components(v, f)
    assert len(sizes) == 2 and int(sizes.min()) > 0 and set(fl.tolist()) == {0, 1}
    cv, cf, cl = ops.clean_mesh(v, f, fl, clean=dict(keep="largest"))
    assert len(cf) == int(sizes.max()) and set(cl.tolist()) == {0} and len(ops.mesh_components(cv, cf)[1]) == 1
    assert np.linalg.norm(cv.cpu().numpy() - centre, axis=1).min() > 2 * c["radius"]              # the blob is gone
    sv, sf, sl = ops.clean_mesh(v, f, fl, clean=dict(keep="largest"), simplify=dict(leaf=2 * c["voxel"], placement="quadric"))
    print(f"{len(f)} faces, {len(sizes)} shells {sizes.tolist()} -> cleaned {len(cf)} -> simplified {len(sf)}")
    assert 0 < len(sf) < len(cf) < len(f) and set(sl.tolist()) == {0} and int(sf.max()) == len(sv) - 1
    assert len(ops.mesh_components(sv, sf)[1]) == 1


def test_scans_to_mesh_then_clean_and_simplify_drops_a_planted_blob(dev):
    """The scene of tests/test_gpu_recon.py's scans -> mesh test (five LiDAR frames of the aircraft, voxel 0.12 m) with 80 points on
    a ball of 0.25 m radius planted 15 m above the fuselage in the first scan: the plain mesh has a detached shell there.  The
    field's zero may lie up to a radius (0.36 m) outside the points, so the shell is a ball of at most 0.61 m: 4.7 m^2, some 330
    voxel squares of about four triangles each, 1,300 faces; the aircraft's own shells have tens of thousands.
    clean=dict(keep="all", min_faces=5000) drops the blob and keeps every part, and simplify= at a 0.5 m leaf returns fewer faces"""
    import icp_mesh_oracle as IM
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd.pointcloud import look_at_pose, pinhole_rays
    NM, VOXEL = len(IM.MESH_PARTS), 0.12
    ref = ops.icp_mesh_reference(*IM.aircraft_mesh(1), NM, device=dev)
    az, el, dist = np.deg2rad([25, 55, 85, 115, 145]), np.deg2rad([25, 45, 30, 50, 25]), [46, 50, 44, 52, 47]
    poses = np.stack([look_at_pose(d * np.array([np.cos(a) * np.cos(e), np.sin(a) * np.cos(e), np.sin(e)])) for a, e, d in zip(az, el, dist)])
    xyz, part, _, count = ops.lidar_frames(ref, poses, pinhole_rays(192, 256, 50.0, 40.0), 8192)
    rng = np.random.default_rng(8)
    d = rng.normal(size=(80, 3))
    centre = np.array([-5.0, 0.0, 15.0])
    blob = centre + 0.25 * d / np.linalg.norm(d, axis=1, keepdims=True)
    blob0 = (blob @ poses[0][:3, :3].T + poses[0][:3, 3]).astype(F32)                     # in the first scan's frame
    clouds = [torch.cat((xyz[0], _t(blob0, dev)))] + [xyz[i] for i in range(1, 5)]
    labels = [torch.cat((part[0], torch.zeros(80, device=dev, dtype=torch.int32)))] + [part[i] for i in range(1, 5)]
    to_model = torch.from_numpy(np.linalg.inv(poses)).to(dev)
    v, f, fl = ops.scans_to_mesh(clouds, to_model, VOXEL, labels=labels, n_labels=NM)
    near = lambda vv: int((np.linalg.norm(vv.cpu().numpy() - centre, axis=1) < 1.0).sum())      # noqa: E731
    comp, sizes = ops.mesh_components(v, f)
    cv, cf, cl = ops.clean_mesh(v, f, fl, clean=dict(keep="all", min_faces=5000))
    sv, sf, sl = ops.clean_mesh(v, f, fl, clean=dict(keep="all", min_faces=5000), simplify=dict(leaf=0.5))
    print(f"plain {len(v)} vertices {len(f)} faces in {len(sizes)} shells (largest {sorted(sizes.tolist())[-4:]}), {near(v)} vertices at the blob; "
          f"cleaned {len(cf)} faces; simplified {len(sv)} vertices {len(sf)} faces")
    assert near(v) > 0 and near(cv) == 0 and near(sv) == 0
    assert 0 < len(sf) < len(cf) < len(f) and len(torch.unique(sl)) == NM == len(torch.unique(cl))
    mesh = ops.icp_mesh_reference(sv, sf, sl, NM)                       # and it is a mesh reference like any other
    assert mesh.tri.shape[0] > 0
