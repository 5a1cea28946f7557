"""The mesh sampler's specification and host side without a GPU: the Philox known answers, the invariants of the NumPy oracle
(tests/mesh_sample_oracle.py) on the procedural aircraft, the C ABI surface with its host-only argument checks, and what the
sampler is for: the coarse ranking of ops.global_pose against a sampled score cloud instead of the mesh's vertices."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import icp_global_oracle as GO
import icp_oracle as IO
import mesh_sample_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_philox_known_answers():
    x = SO.philox4x32(np.zeros(4, np.int64), (0, 0))
    assert [int(v) for v in x] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    x = SO.philox4x32(np.full(4, 0xFFFFFFFF, np.int64), (0xFFFFFFFF, 0xFFFFFFFF))
    assert [int(v) for v in x] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    many = SO.philox4x32(np.stack([np.arange(5), np.full(5, 3), np.zeros(5, np.int64), np.zeros(5, np.int64)], -1), (7, 0))
    assert many.shape == (5, 4) and many.dtype == np.uint32 and len({tuple(r) for r in many.tolist()}) == 5
    assert np.array_equal(many[2], SO.philox4x32(np.array([2, 3, 0, 0]), (7, 0)))


def test_weights():
    area = np.array([3.0, 1.5, 0.0, -2.0, np.nan, np.inf, 3.0 * 2.0 ** -30, 3.0 * 2.0 ** -24, 2.5 * 2.0 ** -23])
    w = SO.weights(area)
    # amax = 3 = 0.75 * 2^2: the scale is 2^22; 3 * 2^-24 * 2^22 = 0.75 -> 1; 2.5 * 2^-23 * 2^22 = 1.25 -> 1
    assert w.dtype == np.uint64 and w.tolist() == [3 << 22, 3 << 21, 0, 0, 0, 0, 0, 1, 1]
    assert SO.weights(np.array([0.5, 1.5]) * 2.0 ** -22).tolist() == [1 << 22, 3 << 22]            # the scale follows amax: 2^45
    assert SO.weights(np.array([2.0 ** 24, 0.5, 1.5, 2.5])).tolist() == [1 << 23, 0, 1, 1]        # rint: 0.25 -> 0, 0.75 -> 1, 1.25 -> 1
    assert SO.weights(np.array([2.0 ** 25, 1.0, 3.0, 5.0])).tolist() == [1 << 23, 0, 1, 1]        # 0.25 -> 0, 0.75 -> 1, 1.25 -> 1
    assert SO.weights(np.array([2.0 ** 24, 1.0, 3.0, 5.0])).tolist() == [1 << 23, 0, 2, 2]        # ties to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    assert SO.weights(np.array([np.nan, -1.0, 0.0])).tolist() == [0, 0, 0] and SO.weights(np.zeros(0)).tolist() == []
    for amax in (1.0, 1.0 - 2.0 ** -53, 1e-310, 1e300):                                             # the largest weight in [2^23, 2^24]
        assert (1 << 23) <= int(SO.weights(np.array([amax]))[0]) <= (1 << 24)


def test_oracle_invariants_on_the_aircraft():
    tri, seg, nrm, area = SO.aircraft(0)
    n = 2048
    row, a, b = SO.draw(area, n, seed=7)
    xyz, part, row2 = SO.mesh_sample(tri, area, seg, SO.NM, n, seed=7)
    assert np.array_equal(row, row2) and xyz.dtype == F32 and xyz.shape == (1, n, 3) and part.dtype == np.int32 and row.dtype == np.int32
    assert (np.diff(row[0]) >= 0).all() and row.min() >= 0 and row.max() < len(tri)                 # rows never decrease
    w = SO.weights(area).astype(np.float64)
    dev = np.abs(np.bincount(row[0], minlength=len(tri)) - n * w / w.sum()).max()
    print(f"largest |count - n w / W| = {dev:.3f}")
    assert dev < 2                                                                                  # the stratification's bound
    assert (a >= 0).all() and (b >= 0).all() and (a + b <= SO.ONE24).all() and (a + b).max() > 0.99 * SO.ONE24
    # the fp32 point against fp64 from the same (row, a, b): six roundings, each below 2^-23 M -> 12 * 2^-24 M; 16 allowed
    M = np.abs(tri).max()
    t = tri[row[0]].astype(np.float64)
    u, v = a[0, :, None] / SO.ONE24, b[0, :, None] / SO.ONE24
    p64 = t[:, 0] + u * (t[:, 1] - t[:, 0]) + v * (t[:, 2] - t[:, 0])
    err = np.abs(xyz[0].astype(np.float64) - p64).max()
    plane = np.abs(((p64 - t[:, 0]) * nrm[row[0]].astype(np.float64)).sum(1)).max()
    print(f"M = {M}, max |p32 - p64| = {err:.3e} (bound {16 * 2.0 ** -24 * M:.3e}), plane residual of p64 {plane:.3e}")
    assert err <= 16 * 2.0 ** -24 * M
    assert np.array_equal(part[0], np.searchsorted(seg, row[0], side="right") - 1)                  # no empty segment here
    # a set is a function of (seed, set index) alone
    r3, a3, b3 = SO.draw(area, n, seed=7, sets=3)
    r2, a2, b2 = SO.draw(area, n, seed=7, sets=2, set0=1)
    assert np.array_equal(r3[0], row[0]) and np.array_equal(r3[1:], r2) and np.array_equal(a3[1:], a2) and np.array_equal(b3[1:], b2)
    assert not np.array_equal(r3[0], r3[1]) and not np.array_equal(SO.draw(area, n, seed=8)[0], row)
    # nothing to draw from
    xyz0, part0, row0 = SO.mesh_sample(np.zeros((0, 3, 3), F32), np.zeros(0), np.zeros(SO.NM + 1, np.int64), SO.NM, 5)
    assert np.isnan(xyz0).all() and (part0 == -1).all() and (row0 == -1).all()
    # a label with an empty segment is never returned
    seg5 = np.array([0, seg[1], seg[1], seg[2], seg[3], seg[4]])
    assert set(np.unique(SO.part_of(row[0], seg5, 5)).tolist()) == {0, 2, 3, 4}


def test_sample_reference_is_grouped():
    tri, seg, nrm, area = SO.aircraft(0)
    xyz, cseg, row, normals = SO.sample_reference(tri, area, seg, SO.NM, nrm, 500, seed=3)
    assert cseg[0] == 0 and cseg[-1] == 500 and (np.diff(cseg) > 0).all()
    for l in range(SO.NM):
        assert ((row[cseg[l]:cseg[l + 1]] >= seg[l]) & (row[cseg[l]:cseg[l + 1]] < seg[l + 1])).all()
    assert np.array_equal(normals, nrm[row])


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI surface
# ---------------------------------------------------------------------------------------------------------------------
SAMPLE_SYMBOLS = ("pn_mesh_sample_workspace_bytes", "pn_mesh_sample")


def test_symbols_declared_bound_and_exported():
    from pointcloudprocessing_amd import _lib, ops, pointcloud
    hdr = open(os.path.join(ROOT, "include", "pointnet_hip.h")).read()
    l = C.CDLL(_lib.LIB_PATH)
    for name in SAMPLE_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(l, name), name
    assert "#define PN_ABI_VERSION 6" in hdr and _lib.ABI_VERSION == 6                # additive: the version stays
    for name in ("mesh_sample", "mesh_sample_reference"):
        assert callable(getattr(ops, name))
    assert "sample_dataset" in pointcloud.__all__ and callable(pointcloud.sample_dataset)
    import inspect
    assert inspect.signature(ops.global_pose).parameters["score_cloud"].default is None


def test_bad_arguments_are_refused_before_any_device_call():
    """every limit of pn_mesh_sample from the host-only checks: the pointers are never dereferenced"""
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    P = C.c_void_p(4096)                                                          # stands for a device pointer; never used
    seg = (C.c_int32 * 3)(0, 4, 10)
    bad_seg = (C.c_int32 * 3)(0, 11, 10)
    need = L.pn_mesh_sample_workspace_bytes(10, 2, 100)
    assert need >= 10 * 8
    for T, B, n in ((-1, 2, 100), ((1 << 20) + 1, 2, 100), (10, 0, 100), (10, 2, 0), (10, 2, (1 << 19) + 1), (10, 1025, 1 << 18)):
        assert L.pn_mesh_sample_workspace_bytes(T, B, n) == 0, (T, B, n)
    assert L.pn_mesh_sample_workspace_bytes(0, 1, 1) > 0 and L.pn_mesh_sample_workspace_bytes(1 << 20, 512, 1 << 19) >= 8 << 20
    ok = dict(tri=P, area=P, seg=seg, T=10, n_parts=2, seed=7, set0=0, B=2, n=100, xyz=P, row=P, part=P, ws=P, ws_bytes=need)
    order = ("tri", "area", "seg", "T", "n_parts", "seed", "set0", "B", "n", "xyz", "row", "part", "ws", "ws_bytes")

    def call(**kw):
        a = dict(ok, **kw)
        return L.pn_mesh_sample(*[a[k] for k in order], None)

    for kw in (dict(T=-1), dict(T=(1 << 20) + 1), dict(T=9), dict(n=0), dict(n=-3), dict(n=(1 << 19) + 1), dict(B=0), dict(B=-1),
               dict(B=1025, n=1 << 18, ws_bytes=1 << 30), dict(set0=-1), dict(set0=(1 << 31) - 2, B=3), dict(set0=(1 << 31) - 1),
               dict(n_parts=0), dict(n_parts=17), dict(seg=bad_seg), dict(seg=None), dict(tri=None), dict(area=None), dict(xyz=None),
               dict(row=None), dict(part=None), dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
        assert call(**kw) == -1, kw
        assert b"pn_mesh_sample" in L.pn_last_error(), kw


# ---------------------------------------------------------------------------------------------------------------------
# what it is for: the coarse score of global_pose against the sampled surface
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SO.ONE_SIDED_SEEDS)
def test_closest_seed_survives_the_coarse_ranking_on_samples(seed):
    """80 triangles, 1,024-point one-sided scans, rotation_grid(256), stride 4, 3 m: scored on 2,048 surface samples the seed
    closest to the truth ranks below top = 4 (measured: 0, 3, 0, 3, 0, 0, 2 on seeds 0, 1, 3, 4, 5, 6, 7; seed 2 ranks 4 and is left
    out; scored on the 240 vertices the ranks are 9, 4, 4, 33, 16, 0, 40)"""
    rank = SO.closest_seed_rank(seed, SO.score_cloud(0))
    print(f"seed {seed}: rank {rank} of the closest seed, scored on samples")
    assert rank < GO.PARAMS["top"]


def test_seed_3_needs_the_score_cloud():
    """the whole composition on seed 3: with the score cloud inside CAP_ROT / CAP_T of the truth (measured 5.6e-4 rad, 1.3e-2 m,
    cost 1.64), with the vertex cloud more than 1 rad away (measured 3.14 rad, 1.09 m, cost 1189)"""
    T = SO.one_sided_case(3)[2]
    ang, dt = IO.pose_error(SO.solved(3, True)["pose"][0], T)
    vang, vdt = IO.pose_error(SO.solved(3, False)["pose"][0], T)
    print(f"samples: {ang:.3e} rad {dt:.3e} m cost {SO.solved(3, True)['cost'][0]:.3f}; vertices: {vang:.3e} rad {vdt:.3e} m cost "
          f"{SO.solved(3, False)['cost'][0]:.1f}")
    assert ang < GO.CAP_ROT and dt < GO.CAP_T
    assert vang > 1.0
