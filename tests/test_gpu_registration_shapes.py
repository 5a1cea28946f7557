"""pn_feature_match, pn_ransac_poses, pn_fpfh and ops.global_register on the MI355X at the launch shapes tests/test_gpu_fpfh.py does
not reach, on the cases of tests/registration_cases.py (tests/test_cpu_fpfh.py checks the cases' own conditions on the oracle):
several LDS tiles per slice of b with planted rows, a short last slice, a partial last tile and two query blocks; a score grid of
more than one block in either dimension; bins that hold k = 16; the batched, mutual, few-valid and no-valid calls of
ops.global_register.  Every comparison with the NumPy oracle (tests/fpfh_oracle.py) is an equality of bits, integers or indices, the
RANSAC poses excepted, which keep test_gpu_fpfh's POSE_TOL."""
import numpy as np
import pytest
import torch

import fpfh_oracle as FO
import icp_oracle as IO
import registration_cases as RC
from test_gpu_fpfh import _bits, _check_fpfh, _check_ransac, _raw_fpfh, _raw_match, _t

pytestmark = pytest.mark.gpu
F32 = np.float32
PN_ICP_CONVERGED, PN_ICP_FEW_PAIRS = 1, 2


# ---- pn_feature_match: several tiles per slice -----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RC.MATCH_SHAPES))
def test_feature_match_several_tiles_per_slice(dev, name):
    """idx and the bits of d2 against the oracle with guard bands round the outputs and the workspace; the planted rows are named
    in registration_cases.match_case.  At Na = 257 the oracle runs on the planted rows, both ends of either query block and some
    rows between (rows are independent in the specification); the other rows' idx must name a row of b"""
    case = RC.match_case(name)
    b = case["b"]
    for a, plants in case["rounds"]:
        rows = RC.match_rows(name, plants)
        idx, d2 = FO.feature_match(a[rows], b, chunk=4)
        got = _raw_match(a, b, dev)
        print(f"{name}: planted {[(r, e) for r, (e, _) in plants.items()]}, device {[int(got[0][r]) for r in plants]}")
        assert np.array_equal(got[0][rows], idx) and np.array_equal(_bits(got[1][rows]), _bits(d2))
        for r, (e, what) in plants.items():
            assert got[0][r] == e and got[1][r] == 0, what
        rest = np.setdiff1d(np.arange(len(a)), rows)
        assert ((got[0][rest] >= -1) & (got[0][rest] < len(b))).all() and not np.isnan(got[1][rest]).any()
        if len(a) == 257:
            assert got[0][31] == -1 and np.isinf(got[1][31]) and (got[0][rest] >= 0).all()


def test_feature_match_mutual_with_a_long_back_direction(dev):
    """ops.feature_match(mutual=True) on (3, 128 * 4096 + 5): the back direction has 524,293 queries in 2,049 blocks against 3 rows"""
    from pointcloudprocessing_amd import ops
    case = RC.match_case("two_tiles")
    a, plants = case["rounds"][RC.MUTUAL_ROUND]
    ei, ed = FO.feature_match(a, case["b"], mutual=True, chunk=4)
    oi, od = ops.feature_match(_t(a, dev), _t(case["b"], dev), mutual=True)
    assert np.array_equal(oi.cpu().numpy(), ei) and np.array_equal(_bits(od.cpu().numpy()), _bits(ed))
    assert all(ei[r] == e for r, (e, _) in plants.items())
    # the back direction by itself, every one of its rows
    back = FO.feature_match(case["b"], a)
    got = _raw_match(case["b"], a, dev)
    assert np.array_equal(got[0], back[0]) and np.array_equal(_bits(got[1]), _bits(back[1]))
    assert (back[0] == -1).sum() == 2 and len(np.unique(back[0])) == 4            # the two rows that are not finite; every query is somebody's


def test_feature_match_beyond_65535_tiles(dev):
    """Na = 2 against 8,388,781 rows built from nine copies of one block: a unique best near the end, and a best that every copy
    holds, of which the first must win.  1.1 GB of descriptors; 3.5 s on the MI355X, most of it the oracle's pass over b"""
    a, b, partners = RC.tiled_match()
    idx, d2 = FO.feature_match(a, b, chunk=2)
    assert tuple(idx) == partners and not d2.any() and len(b) > 65535 * RC.TILE
    got = _raw_match(a, b, dev)
    assert np.array_equal(got[0], idx) and np.array_equal(_bits(got[1]), _bits(d2))


# ---- pn_ransac_poses: more than one block in each grid dimension -----------------------------------------------------
@pytest.mark.parametrize("C,H,seed", RC.RANSAC_SHAPES)
def test_ransac_poses_beyond_one_block(dev, C, H, seed):
    """teacher-forced as in test_gpu_fpfh: draws, validity and counts exactly, poses within POSE_TOL.  (257, 1025): a second pair
    block of one row and a second hypothesis block of one hypothesis; (700, 2500): three by three blocks; (700, 65536): the largest
    H the entry takes"""
    src, tgt, _ = RC.ransac_case(C, seed)
    R = RC.RANSAC
    poses, counts, rows, ok = _check_ransac(src, tgt, R["max_dist"], H, R["edge_ratio"], seed, dev)
    print(f"C {C} H {H}: {int(ok.sum())} valid, {int(ok[1024:].sum())} of them at h >= 1024, {int((counts[1024:] > 3).sum())} with a count "
          f"above 3, best {int(counts.max())}")
    assert len(counts) == H and rows.shape == (H, 3)                               # hypothesis H - 1 is checked like the others
    if (C, H) == (700, 2500):
        assert (ok[1024:] & (counts[1024:] > 3)).sum() >= 50
    if H == FO.MAX_H:
        assert (ok[H - 256:]).any() and counts[H - 256:].max() > 3                 # the last hypothesis block counts


def test_ransac_poses_refuses_more_hypotheses(dev):
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd._lib import PointNetHipError
    src, tgt, _ = RC.ransac_case(257, 8)
    with pytest.raises(PointNetHipError, match=r"hypotheses=65537 outside \[1, 65536\]"):
        ops.ransac_poses(_t(src, dev), _t(tgt, dev), 0.02, FO.MAX_H + 1)


def test_ransac_counts_from_the_last_pair_block_only(dev):
    """the right pairs sit in rows >= 512 of 700, a NaN row among them: a valid hypothesis counts in the third, partial pair block and
    nowhere else"""
    src, tgt, true = RC.late_inliers()
    R = RC.RANSAC
    poses, counts, rows, ok = _check_ransac(src, tgt, R["max_dist"], RC.LATE_H, R["edge_ratio"], RC.LATE_SEED, dev)
    early = FO.count_inliers(src[:RC.LATE_FIRST], tgt[:RC.LATE_FIRST], np.nan_to_num(poses).astype(F32), R["max_dist"])
    assert ok.sum() >= 20 and not early[ok].any() and counts.max() >= 150
    ang, dt = IO.pose_error(poses[FO.rank(counts)[0]], true)
    assert ang < 0.02 and dt < 0.05


# ---- pn_fpfh: a bin that holds k -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RC.FPFH_FLAT))
def test_fpfh_full_bins(dev, name):
    """counts, pairs and descriptor bits on flat clouds whose rows put all 16 pairs into one bin per feature (the lattice's distances
    tie as well); with the tilted strip a full bin has a neighbour that counts in the descriptor"""
    x, n, radius, (out, counts, pairs) = RC.fpfh_flat(name)
    got = _raw_fpfh(x, n, radius, RC.FLAT_K, dev)
    _check_fpfh(got, x, n, radius, RC.FLAT_K)
    full = RC.full_rows(counts)
    assert counts.max() == 16 and got[1].max() == 16 and np.array_equal(RC.full_rows(got[1]), full)
    assert full.sum() >= {"lattice": 16, "patch": 270, "tilted_strip": 150}[name]
    if name == "tilted_strip":
        assert RC.full_bin_beside_a_counted_one(got[0], got[1]).sum() >= 30


# ---- ops.global_register: the calls nobody has run -------------------------------------------------------------------
def _register(src, tgt, sc, S, **kw):
    from pointcloudprocessing_amd import ops
    args = dict(normals_radius=S["normals_radius"], k=S["k"], hypotheses=S["hypotheses"], keep=S["keep"], top=S["top"], mutual=S["mutual"],
                seed=S["seed"], edge_ratio=S["edge_ratio"], source_viewpoint=sc["source_viewpoint"].tolist(),
                target_viewpoint=sc["target_viewpoint"].tolist(), max_iters=S["max_iters"])
    args.update(kw)
    return ops.global_register(src, tgt, S["feature_radius"], S["max_dist"], **args)


def test_global_register_batch_equals_its_rows(dev):
    sc, S = FO.scene(), FO.SCENE
    two = np.stack([sc["source"], RC.second_source(sc["source"], sc["source_viewpoint"])])
    src, tgt = _t(two, dev), _t(sc["target"], dev)
    both = _register(src, tgt, sc, S)
    assert [tuple(t.shape) for t in both] == [(2, 4, 4)] + [(2,)] * 6
    for b in range(2):
        one = _register(src[b].contiguous(), tgt, sc, S)
        for name, x, y in zip(("pose", "rmse", "pairs", "iters", "status", "cost", "winner"), both, one):
            assert x.dtype == y.dtype and torch.equal(x[b:b + 1].contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), (b, name)
    pose = both[0].cpu().numpy()
    assert np.isfinite(pose).all() and IO.pose_error(pose[0], sc["pose"])[0] <= FO.BOUND_ROT
    assert IO.pose_error(pose[1], pose[0])[0] > 10 * FO.BOUND_ROT                 # the second row is another registration


def _oracle_tail(dev, sc, S, got):
    """the steps on the device, then the oracle's tail on the device's hypotheses, held to the bounds of
    test_gpu_fpfh.test_global_registration_of_the_fixture -> the device's counts (H,)"""
    from pointcloudprocessing_amd import ops
    pose, rmse, pairs, iters, status, cost, winner = got
    src, tgt = _t(sc["source"], dev), _t(sc["target"], dev)
    sv, tv = sc["source_viewpoint"].tolist(), sc["target_viewpoint"].tolist()
    f_s = ops.fpfh(src, ops.estimate_normals(src, S["normals_radius"], S["k"], sv)[0], S["feature_radius"], S["k"])
    f_t = ops.fpfh(tgt, ops.estimate_normals(tgt, S["normals_radius"], S["k"], tv)[0], S["feature_radius"], S["k"])
    idx = ops.feature_match(f_s, f_t, mutual=S["mutual"])[0].cpu().numpy()
    assert np.array_equal(idx, FO.feature_match(f_s.cpu().numpy(), f_t.cpu().numpy(), S["mutual"])[0])
    sel = np.flatnonzero(idx >= 0)
    hp, hc, order = ops.ransac_poses(_t(sc["source"][sel], dev), _t(sc["target"][idx[sel]], dev), S["max_dist"], S["hypotheses"], S["edge_ratio"],
                                     S["seed"])
    hc = hc.cpu().numpy()
    kept = FO.rank(hc)[:S["keep"]]
    want = FO.refine(sc["source"], sc["target"], hp.cpu().numpy()[kept], S, normals_radius=S["normals_radius"])
    picks = kept[want["order"][:S["top"]]]
    low = picks[want["fine"] <= want["fine"].min() * (1.0 + 1e-6)]
    print(f"{len(sel)} pairs, {int((hc >= 0).sum())} valid hypotheses; oracle tail: candidates {picks.tolist()}, costs {want['fine'].tolist()}; "
          f"device: winner {int(winner[0])}, cost {cost[0]:.8f}, status {int(status[0])}")
    assert int(winner[0]) in low.tolist()
    assert abs(cost[0] - want["cost"]) <= 1e-6 * want["cost"]
    oang, odt = IO.pose_error(pose[0], want["pose"])
    assert oang < 1e-5 and odt < 1e-4, (oang, odt)
    ang, dt = IO.pose_error(pose[0], sc["pose"])
    assert ang <= FO.BOUND_ROT and dt <= FO.BOUND_T, (ang, dt)
    return hc, sel


def test_global_register_mutual(dev):
    """mutual=True on the fixture ends within the bounds, and at the oracle tail's result on the device's hypotheses: those drawn
    from the mutual pairs, fewer than half of the one-way ones"""
    sc, S = FO.scene(), RC.MUTUAL
    got = [t.cpu().numpy() for t in _register(_t(sc["source"], dev), _t(sc["target"], dev), sc, S)]
    hc, sel = _oracle_tail(dev, sc, S, got)
    assert 50 < len(sel) < len(sc["source"]) // 2 and (hc >= 0).sum() >= 16


def test_global_register_with_fewer_valid_hypotheses_than_keep(dev):
    """16 hypotheses, two of them valid, keep = 32 and top = 4: order[:keep] and the refined candidates hold NaN poses.  The winner is
    a valid hypothesis, the pose is finite, and the result is the oracle tail's on the device's hypotheses"""
    sc, S = FO.scene(), RC.FEW
    got = [t.cpu().numpy() for t in _register(_t(sc["source"], dev), _t(sc["target"], dev), sc, S)]
    pose, rmse, pairs, iters, status, cost, winner = got
    hc, _ = _oracle_tail(dev, sc, S, got)
    assert tuple(np.flatnonzero(hc >= 0)) == RC.FEW_VALID and len(hc) < S["keep"] and len(RC.FEW_VALID) < S["top"]
    assert hc[int(winner[0])] >= 0 and np.isfinite(pose).all() and np.isfinite(cost).all() and np.isfinite(rmse).all()


def test_global_register_without_a_valid_hypothesis(dev):
    """source and target on one line: every hypothesis is invalid, every start is NaN.  As pn_semantic_icp promises for a start that
    finds no pairs, the pose is kept (not finite) and status carries PN_ICP_FEW_PAIRS"""
    sc = dict(source_viewpoint=np.zeros(3, F32), target_viewpoint=np.zeros(3, F32))
    src, tgt = RC.line_scans()
    for metric in ("plane", "point"):
        pose, rmse, pairs, iters, status, cost, winner = (t.cpu().numpy() for t in _register(_t(src, dev), _t(tgt, dev), sc, FO.SCENE,
                                                                                             hypotheses=RC.LINE_H, metric=metric))
        print(f"no valid hypothesis ({metric}): status {int(status[0])}, pairs {int(pairs[0])}, cost {cost[0]}, winner {int(winner[0])}")
        assert pose.shape == (1, 4, 4) and not np.isfinite(pose[0, :3]).any()
        assert int(status[0]) & PN_ICP_FEW_PAIRS and int(status[0]) != PN_ICP_CONVERGED and int(pairs[0]) == 0 and np.isnan(rmse[0])
        assert int(status[0]) == PN_ICP_CONVERGED | PN_ICP_FEW_PAIRS                  # a kept pose also converges: it did not move
        assert 0 <= int(winner[0]) < RC.LINE_H
