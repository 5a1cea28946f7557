"""The inputs of tests/test_gpu_voxel.py, tests/test_gpu_fps.py and the k-NN instantiation test, checked without a GPU: every case
must make the path it is named after the path that runs.  Checked on the NumPy oracles alone (oracle/sampling_oracle.py,
tests/knn_oracle.py), so a later edit of a builder cannot leave a GPU case vacuous."""
import numpy as np
import pytest

import knn_oracle as KO
import sampler_cases as SC
from oracle import sampling_oracle as SO


def _indices(case):
    return SO.voxel_indices(case["xyz"], case["leaf"], case["origin"])


def _check_keys(case):
    """the oracle's keys are the keys built, in range, live exactly where the case says, with a non-zero digit everywhere else"""
    k = _indices(case)
    assert np.array_equal(k, case["k"])
    assert (k >= 0).all() and (k < SC.KEY_LIMIT).all()
    assert SC.live_positions(k) == case["live"]
    dig = SC.key_digits(k)
    for p in SC.ALL_POS:
        if p not in case["live"]:
            assert (dig[:, p] == dig[0, p]).all() and dig[0, p] != 0, p
    return k


def test_digit_positions_are_the_kernels():
    """shift and width of the nine digit positions as pn_voxel.hip states them: they tile the 63 key bits"""
    at = 0
    for axis in range(3):
        for part, bits in enumerate((8, 8, 5)):
            p = 3 * axis + part
            assert SC.digit_shift(p) == at and SC.digit_bits(p) == bits
            assert 1 <= SC.dead_digit(p) < (1 << bits)
            at += bits
    assert at == 63


@pytest.mark.parametrize("live", SC.VOXEL_LIVE_SETS, ids=lambda v: "live" + "".join(map(str, v)))
def test_voxel_live_sets(live):
    case = SC.voxel_live_case(live)
    _check_keys(case)
    assert len(case["xyz"]) == 3000 and set(case["labels"]) == set(range(SC.N_LABELS))


def test_voxel_live_sets_cover_both_buffer_parities_and_tied_majorities():
    assert sorted({len(v) for v in SC.VOXEL_LIVE_SETS}) == [0, 1, 2, 3, 4, 9]
    tied = 0
    for live in SC.VOXEL_LIVE_SETS:
        case = SC.voxel_live_case(live)
        k = case["k"]
        _, inv = np.unique((k[:, 2] << 42) | (k[:, 1] << 21) | k[:, 0], return_inverse=True)
        h = np.zeros((inv.max() + 1, SC.N_LABELS), np.int64)
        np.add.at(h, (inv, case["labels"]), 1)
        tied += int(((h == h.max(1, keepdims=True)).sum(1) > 1).sum())
    assert tied >= 50, tied


@pytest.mark.parametrize("N", SC.VOXEL_SIZES)
def test_voxel_sizes(N):
    case = SC.voxel_size_case(N)
    k = _check_keys(case)
    assert len(k) == N
    assert len(np.unique(k, axis=0)) > (N // 4) * 0.9 or N < 64              # the pool is in use: about four points per voxel


@pytest.mark.parametrize("kind", SC.VOXEL_ORDERS)
def test_voxel_order_and_skew(kind):
    case = SC.voxel_order_case(kind)
    k = _check_keys(case)
    key = (k[:, 2] << 42) | (k[:, 1] << 21) | k[:, 0]
    if kind == "sorted":
        assert (np.diff(key) >= 0).all() and (np.diff(key) > 0).sum() > 4000
    if kind == "reversed":
        assert (np.diff(key) <= 0).all() and (np.diff(key) < 0).sum() > 4000
    if kind == "skewed":
        _, n = np.unique(key, return_counts=True)
        assert n.max() >= 0.985 * len(key) and len(n) > 100


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_voxel_faces_tell_fp32_from_fp64(axis):
    case = SC.voxel_face_case(axis)
    k = _indices(case)
    assert len(k) == 1197 and k[:, axis].min() == 0 and k[:, axis].max() == SC.FACE_K
    other = [a for a in range(3) if a != axis]
    assert (k[:, other] == k[0, other]).all() and (k >= 0).all()
    differ = int((k[:, axis] != SC.face_keys_fp64(case)).sum())
    assert differ >= 300, differ                                              # measured: 343


def test_voxel_bad_labels():
    case = SC.voxel_bad_label_case()
    _check_keys(case)
    lab, allbad = case["labels"], case["all_bad_points"]
    valid = (lab >= 0) & (lab < SC.N_LABELS)
    for bad in SC.BAD_LABELS:
        assert (lab == bad).sum() > 100
    assert not valid[allbad].any() and allbad.sum() > 300
    cent, cnt, maj = SO.voxel_downsample(case["xyz"], case["leaf"], case["origin"], lab, SC.N_LABELS)
    k = case["k"]
    keys, inv = np.unique((k[:, 2] << 42) | (k[:, 1] << 21) | k[:, 0], return_inverse=True)
    no_valid = np.bincount(inv, weights=valid, minlength=len(keys)) == 0
    assert no_valid.sum() >= 50 and (maj[no_valid] == 0).all()
    # the labels that are ignored change nothing: the same majority as over the valid points alone
    _, _, maj_valid = SO.voxel_downsample(case["xyz"][valid], case["leaf"], case["origin"], lab[valid], SC.N_LABELS)
    assert np.array_equal(maj[~no_valid], maj_valid) and (maj[~no_valid] > 0).any()


@pytest.mark.parametrize("kind", SC.VOXEL_REFUSALS)
def test_voxel_refusals_have_one_refused_point(kind):
    case = SC.voxel_refusal_case(kind)
    k = _indices(case)
    out = ((k < 0) | (k >= SC.KEY_LIMIT)).any(1)
    assert np.flatnonzero(out).tolist() == [case["bad"]]
    if kind == "key_2_21":
        assert k[case["bad"]].max() == SC.KEY_LIMIT
    if kind == "below_origin":
        assert k[case["bad"]].min() == -1
    with pytest.raises(AssertionError):
        SO.voxel_downsample(case["xyz"], case["leaf"], case["origin"])


# --------------------------------------------------------------------------------------------------------------------- FPS
def _bpc(N):
    return 1 if N <= SC.FPS_SINGLE_BLOCK_MAX else -(-N // SC.FPS_BLOCK)


def test_fps_cases_reach_their_paths():
    c = SC.FPS_CASES
    B, N, M, s = c["clouds_x_blocks"]
    assert B > 1 and _bpc(N) == 3 and SC.fps_block_of(s) == 2
    B, N, M, s = c["two_launches"]
    assert _bpc(N) == 2 and B * _bpc(N) > 128 and s != 0
    x = SC.fps_cloud("two_launches")
    assert len({x[b].tobytes() for b in range(B)}) == B                        # every cloud different
    B, N, M, s = c["tag_wrap"]
    assert M - 1 > SC.FPS_TAG_PERIOD and N > SC.FPS_SINGLE_BLOCK_MAX
    B, N, M, s = c["largest_cloud"]
    assert _bpc(N) == 64 and N == 64 * SC.FPS_BLOCK and s == N - 1 == (1 << 20) - 1
    B, N, M, s = c["one_point_block"]
    assert N % SC.FPS_BLOCK == 1 and s == N - 1
    B, N, M, s = c["block_boundary"]
    assert N == 2 * SC.FPS_BLOCK
    sizes = [c[n][1] for n in ("plain_1000", "plain_4000", "plain_16000", "plain_21000")]
    for n, lo, hi in zip(sizes, (0, 1024, 4096, 16384), (1024, 4096, 16384, SC.FPS_SINGLE_BLOCK_MAX)):
        assert lo < n <= hi                                                    # one size per single-block instantiation
    for name in ("plain_1000", "plain_4000", "plain_16000", "plain_21000"):
        assert c[name][3] == c[name][1] - 1
    assert c["m1_small"][2] == 1 and c["m1_multi_block"][2] == 1 and _bpc(c["m1_multi_block"][1]) > 1
    assert c["m_above_n"][2] > c["m_above_n"][1]
    B, N, M, s = SC.FPS_PRUNED_CASE
    g = SC.fps_ordered_grid()
    assert g.shape == (B, N, 3) and B == 2 and 4096 < N <= 20480 and not np.array_equal(g[0], g[1])


def test_fps_cross_block_ties():
    B, N, M, s = SC.FPS_CASES["cross_block_ties"]
    xyz = SC.fps_cloud("cross_block_ties")[0]
    idx, _ = SO.fps(xyz, M, s)
    twins = dict(SC.FPS_TIE_PAIRS)
    hit = [i for i in idx if i in twins]
    assert len(hit) >= 4, hit
    for i in hit:
        j = twins[i]
        assert i < SC.FPS_BLOCK and j > 2 * SC.FPS_BLOCK and SC.fps_block_of(i) != SC.fps_block_of(j)
        assert np.array_equal(xyz[i], xyz[j])
        assert j not in idx[:list(idx).index(i)]                               # the lower index won the tie


def test_fps_oracle_on_degenerate_draws():
    """M = 1: no round runs, every distance stays +inf.  M > N: once every point is drawn all distances are 0 and the tie rule
    gives index 0 from then on."""
    B, N, M, s = SC.FPS_CASES["m_above_n"]
    xyz = SC.fps_cloud("m_above_n")
    for b in range(B):
        idx, md = SO.fps(xyz[b], M, s)
        assert sorted(idx[:N]) == list(range(N)) and (idx[N:] == 0).all() and (md == 0).all()
    idx, md = SO.fps(SC.fps_cloud("m1_small")[0], 1, 0)
    assert idx.tolist() == [0] and np.isposinf(md).all()


# -------------------------------------------------------------------------------------------------------------------- k-NN
@pytest.mark.parametrize("k", range(1, 9))
def test_knn_instantiation_cases_have_ties_and_zero_distances(k):
    import test_gpu_scan_propagation as G
    for M in G.knn_case_sizes(k):
        q, ref, vals = G.knn_case(k, M)
        assert q.shape == (2, 130, 3) and ref.shape == (2, M, 3) and vals.shape == (2, M, 5)
        ri, rd = KO.knn(q, ref, k)
        rv, _ = KO.interpolate(ri, rd, vals)
        assert (ri >= 0).all() and (rd[:, :, 0] == 0).any()
        top = np.sort(rv, axis=2)
        assert (top[..., -1] == top[..., -2]).any(), (k, M)
