"""The inputs of tests/test_gpu_knn_every_k.py, checked without a GPU on the NumPy oracles alone (tests/neighbors_oracle.py,
tests/icp_plane_oracle.py, tests/fpfh_oracle.py): at every list length k the case cloud has queries on either side of k, ties across
the last slot and late insertions into every slot, and the part-size reference has a part of K - 1, K and K + 1 members for every K.
These are conditions on the inputs, not measurements: if an edit of a builder misses one, the input changes, not the bound."""
import numpy as np
import pytest

import fpfh_oracle as FO
import icp_plane_oracle as PO
import knn_k_cases as KC
import neighbors_oracle as NO

F32 = np.float32
MANY = 32             # queries with a boundary tie, and late insertions per slot, at the least
ORIGINS = [KC.ORIGIN, KC.SECOND_ORIGIN]


@pytest.fixture(scope="module")
def cloud():
    xyz, radius, origin = KC.k_edge_cloud()
    assert radius == KC.RADIUS == 1.75 and tuple(origin) == KC.ORIGIN == (0.0, 0.0, 0.0)
    return xyz


def test_cloud_is_what_the_builder_says(cloud):
    assert cloud.dtype == F32 and cloud.shape == (1684, 3) and np.isfinite(cloud).all()
    assert len(cloud) > 1024                                               # more than one 1024-row tile of the shared sort
    again = KC.k_edge_cloud()[0]
    assert np.array_equal(cloud.view(np.int32), again.view(np.int32))      # a pure function of the seed
    assert not np.array_equal(cloud, KC.k_edge_cloud(seed=1)[0])
    # the lattice rows hold integers (shuffled among the others); an interior point has 6 + 12 + 8 neighbours at d = 1, 2, 3
    whole = (cloud == np.round(cloud)).all(1) & (cloud.max(1) <= KC.LATTICE_SIDE - 1)
    assert whole.sum() == KC.LATTICE_SIDE ** 3 and 0 < np.flatnonzero(whole)[0] < 20 and not whole[-20:].all()
    idx, d2, count = NO.radius_knn(cloud, KC.RADIUS, 16)
    inner = whole & (cloud > 0).all(1) & (cloud < KC.LATTICE_SIDE - 1).all(1)
    assert inner.sum() == 512 and (count[inner] == 26).all()
    assert (d2[inner][:, :6] == 1).all() and (d2[inner][:, 6:16] == 2).all()
    assert sorted(np.unique(count[whole]).tolist()) == [7, 11, 17, 26]
    # a blob of m points: every one has count m - 1, and its neighbours lie in more than one voxel
    assert sorted(np.unique(count[~whole]).tolist()) == list(range(18))
    assert np.array_equal(np.bincount(count[~whole]), KC.REPLICAS * np.arange(1, 19))
    keys = KC.k_edge_facts(cloud, 1)["keys"]
    spread = [len(np.unique(keys[np.r_[i, idx[i][idx[i] >= 0]]], axis=0)) for i in np.flatnonzero(~whole & (count >= 8))]
    assert min(spread) >= 3 and max(spread) == 8
    # the facts agree with the oracle's own count
    assert np.array_equal(KC.k_edge_facts(cloud, 5)["count"], count)


@pytest.mark.parametrize("origin", ORIGINS, ids=["origin0", "origin1"])
@pytest.mark.parametrize("k", range(KC.MAX_K + 1))
def test_every_k_has_its_edge_cases(cloud, k, origin):
    f = KC.k_edge_facts(cloud, k, origin)
    count = f["count"]
    for c in (0, k - 1, k, k + 1):
        assert c < 0 or (count == c).any(), c
    assert (count >= k + 8).any()
    assert (f["keys"] >= 0).all() and (f["keys"] < NO.MAX_KEY).all()
    if k >= 1:
        assert f["tie"].sum() >= MANY
        assert f["late"].shape == (k,) and f["late"].min() >= MANY, f["late"]
    else:
        assert not f["tie"].any() and f["late"].shape == (0,)


def test_facts_are_the_oracles(cloud):
    """the tie flag and the late insertions recomputed the slow way for a few queries at k = 6 (the k at which an interior lattice
    point has NO tie: 6 neighbours at d = 1, then 12 at d = 2)"""
    k = 6
    f = KC.k_edge_facts(cloud, k)
    idx, d2, count = NO.radius_knn(cloud, KC.RADIUS, 16)
    want = (count > k) & (d2[:, k - 1].view(np.int32) == d2[:, k].view(np.int32))
    assert np.array_equal(f["tie"], want)
    whole = (cloud == np.round(cloud)).all(1)
    inner = whole & (cloud > 0).all(1) & (cloud < KC.LATTICE_SIDE - 1).all(1)
    assert not f["tie"][inner].any() and f["tie"].sum() == 480           # the lattice's faces and edges
    # late insertions by replaying the arrival order of the candidates of every query with a Python list
    vox = (f["keys"][:, 2] * NO.MAX_KEY + f["keys"][:, 1]) * NO.MAX_KEY + f["keys"][:, 0]
    d = NO.dist2(cloud, cloud)
    r2 = F32(KC.RADIUS) * F32(KC.RADIUS)
    late = np.zeros(k, np.int64)
    for i in range(0, len(cloud), 7):
        cand = [j for j in np.flatnonzero(d[i] <= r2) if j != i]
        for c in cand:
            before = [(int(d[i, j].view(np.uint32)), j) for j in cand if vox[j] < vox[c]]
            rank = sum(b < (int(d[i, c].view(np.uint32)), c) for b in before)
            if len(before) >= k and rank < k:
                late[rank] += 1
    w = KC._walk(np.ascontiguousarray(cloud).tobytes(), KC.ORIGIN)
    pick = (w["query"] % 7 == 0) & (w["before"] >= k)
    assert np.array_equal(late, [int((pick & (w["rank"] == s)).sum()) for s in range(k)]) and late.min() > 0


def test_fpfh_on_the_cloud_takes_every_pair_count():
    xyz = KC.k_edge_cloud()[0]
    nrm = KC.unit_normals(len(xyz))
    assert nrm.dtype == F32 and np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1).max() < 1e-6
    out, counts, pairs = FO.fpfh(xyz, nrm, KC.RADIUS, 16, return_spfh=True)
    assert np.array_equal(np.unique(pairs), np.arange(17)) and np.isfinite(out).all()


# ---- pn_icp_normals ---------------------------------------------------------------------------------------------------
def test_part_size_reference():
    g, seg, n_parts = KC.part_size_reference()
    assert g.dtype == F32 and g.shape == (152, 3) and n_parts == 16 and len(seg) == 17 and seg[0] == 0 and seg[-1] == 152
    sizes = np.diff(seg)
    assert sizes.tolist() == list(range(2, 18))
    lab = np.repeat(np.arange(n_parts), sizes)
    assert [len(np.unique(lab[w:w + 64])) for w in (0, 64, 128)] == [10, 6, 2]      # three waves, more than one label in each
    for K in range(3, 17):
        nbr = PO.neighbours(g, seg, n_parts, K)
        filled = (nbr >= 0).sum(1)
        assert (filled[lab == K - 3] == K - 1).all() and (filled[lab == K - 2] == K).all() and (filled[sizes[lab] > K] == K).all()
        assert (nbr[:, 0] == np.arange(152)).all()                          # the point itself leads its list
        assert all(np.isin(nbr[i][nbr[i] >= 0], np.arange(seg[lab[i]], seg[lab[i] + 1])).all() for i in range(152))
        en, ec, _ = PO.normals(g, seg, n_parts, K)
        fin = np.isfinite(en).all(1)
        assert np.array_equal(fin, sizes[lab] >= 3) and np.isfinite(ec[fin]).all()
        s = np.sort(np.abs(en[fin].astype(np.float64)), axis=1)
        assert (s[:, 2] - s[:, 1] > 1e-3).mean() > 0.9                       # tests/test_gpu_icp_plane.py::_normals_close's rule
        assert (np.abs(en[fin, 2]) > 0.9).all()                              # thin plates near the x-y plane
    assert min(KC.plate_gap(g[seg[p]:seg[p + 1]]) for p in range(1, n_parts)) > KC.PLATE_GAP      # no neighbourhood near a line
