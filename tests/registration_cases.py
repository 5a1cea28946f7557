"""Case builders the CPU and the GPU tests of the registration front end share (tests/test_cpu_fpfh.py,
tests/test_gpu_registration_shapes.py) -- TEST INFRASTRUCTURE.  Nothing in the package imports it.

match_case      descriptor sets at which pn_feature_match streams several LDS tiles per slice of b, with planted rows whose place
                within a slice is stated next to each of them
tiled_match     a b of more than 65,535 tiles, nine copies of one block
ransac cases    correspondence sets for more than one block in either dimension of the score grid
fpfh clouds     flat clouds on which the oracle puts all k pairs of a row into one bin per feature
register cases  the keyword sets and scans of ops.global_register's batched, mutual, few-valid and no-valid calls
"""
from __future__ import annotations

import functools

import numpy as np

import fpfh_oracle as FO
import icp_oracle as IO

F32 = np.float32
TILE = 128            # rows of b per LDS tile of pn_feature_match (FM_TILE)

# (Na, Nb) -> the tiles a slice of b holds at that shape, as pn_feature_match's host code sizes it.  A fact about the launch that
# the cases are laid out by; the tests do not recompute it.
MATCH_SHAPES = {
    "two_tiles": (3, TILE * 4096 + 5, 2),          # 2,049 slices; the last holds one partial tile of 5 rows
    "three_tiles": (3, TILE * 6144 + 77, 3),       # the last slice is short: one tile, partial (77 rows)
    "two_blocks": (257, TILE * 2048 + 130, 2),     # two query blocks; the last slice holds a full tile and a partial one of 2 rows
}
# the query rows of the (257, ...) shape that are compared with the oracle next to the planted ones: both ends of either query block
# and rows without a plant
MATCH_ROWS_257 = (0, 1, 255, 256, 2, 31, 64, 127, 128, 191, 254)
MUTUAL_ROUND = 1      # the round of "two_tiles" that ops.feature_match(mutual=True) runs: the two ties and a query without a plant


def descriptors(n, seed):
    """(n, 33) float32 rows with the skew of a histogram: most bins small, a few large"""
    rng = np.random.default_rng(seed)
    return (rng.random((n, 33), dtype=F32) ** 3 * F32(200.0)).astype(F32)


@functools.lru_cache(maxsize=None)
def match_case(name):
    """-> dict(b (Nb, 33) f32, rounds: a list of (a (Na, 33) f32, plants {query row: (expected idx, what)})).  Every plant is a query
    that equals a row of b exactly (d2 = 0), so its expected partner is known without the oracle; the CPU test checks that the oracle
    agrees.  With Na = 3 the seven plants take three rounds against one b; with Na = 257 they share one a.  L = tiles * TILE is the
    length of a slice; the slices named below are all full ones.  Cached: callers do not write to it."""
    na, nb, tiles = MATCH_SHAPES[name]
    L = tiles * TILE
    n_full = nb // L
    assert n_full > 900
    b = descriptors(nb, 11)
    s = [5, 300, 77, 640, n_full - 1, 411]         # the slices that hold a plant (distinct, in no order)
    plants = []                                    # (query vector, expected idx, what)

    # a unique exact match on the first and on the last row of the second tile of slice s[0]
    for r, what in ((TILE, "first row of the second tile of a slice"), (2 * TILE - 1, "last row of the second tile of a slice")):
        plants.append((b[s[0] * L + r].copy(), s[0] * L + r, what))
    # one exact match in the final, partial tile of b (the middle of its 5, 77 or 2 rows)
    tail = nb % TILE
    assert 0 < tail < TILE
    plants.append((b[nb - tail + tail // 2].copy(), nb - tail + tail // 2, "the final partial tile"))
    # equal rows at position 17 of the first tile and position 3 of the last tile of slice s[1]: the lower row wins
    b[s[1] * L + (tiles - 1) * TILE + 3] = b[s[1] * L + 17]
    plants.append((b[s[1] * L + 17].copy(), s[1] * L + 17, "a tie between two tiles of one slice"))
    # equal rows at position 40 of the second tile of slice s[2] and position 9 of the first tile of the later slice s[3]
    assert s[2] < s[3]
    b[s[3] * L + 9] = b[s[2] * L + TILE + 40]
    plants.append((b[s[2] * L + TILE + 40].copy(), s[2] * L + TILE + 40, "a tie between two slices"))
    # position 77 of the first tile of slice s[4] is not finite and would otherwise match exactly; the match is position 77 of the
    # second tile
    q = b[s[4] * L + TILE + 77].copy()
    b[s[4] * L + 77] = q
    b[s[4] * L + 77, 4] = np.nan
    plants.append((q, s[4] * L + TILE + 77, "a non-finite row in the first tile, the match at its position in the second"))
    # the reverse in slice s[5]: position 21 of the second tile is not finite, the match is position 21 of the first
    q = b[s[5] * L + 21].copy()
    b[s[5] * L + TILE + 21] = q
    b[s[5] * L + TILE + 21, 32] = -np.inf
    plants.append((q, s[5] * L + 21, "a non-finite row in the second tile, the match at its position in the first"))

    rounds = []
    if na == 3:
        for i, group in enumerate((plants[0:3], plants[3:5], plants[5:7])):
            a = descriptors(3, 20 + i)
            for row, (q, _, _) in enumerate(group):
                a[row] = q
            rounds.append((a, {row: (idx, what) for row, (_, idx, what) in enumerate(group)}))
    else:
        a = descriptors(na, 20)
        rows = (0, 255, 256, 100, 129, 200, 1)      # both query blocks hold plants; row 1 is the reverse non-finite arrangement
        for row, (q, _, _) in zip(rows, plants):
            a[row] = q
        a[31, 7] = np.nan                            # a query that is not finite: (-1, +inf)
        rounds.append((a, {row: (idx, what) for row, (_, idx, what) in zip(rows, plants)}))
    return dict(b=b, rounds=rounds)


def match_rows(name, plants):
    """the query rows of a round that go to the oracle: all of them when Na = 3; the planted rows and MATCH_ROWS_257 otherwise"""
    na = MATCH_SHAPES[name][0]
    return np.arange(na) if na == 3 else np.array(sorted(set(plants) | set(MATCH_ROWS_257)))


TILED_NB = 65535 * TILE + 1 + 300      # b just above 65,535 tiles


def tiled_match(nb=TILED_NB):
    """-> (a (2, 33), b (nb, 33), the two partners' rows): b repeats one block of ceil(nb / 9) rows (1.1 GB at TILED_NB; not cached;
    the CPU test runs a small nb).  Query 0 equals a row planted 200 rows before the end of b and nowhere else; query 1 equals row
    1234 of the block, which all nine copies hold, in as many slices at TILED_NB: the first copy wins"""
    block = -(-nb // 9)
    blk = descriptors(block, 12)
    b = np.tile(blk, (9, 1))[:nb]
    a = descriptors(2, 13)
    b[nb - 200] = a[0]
    a[1] = blk[1234]
    assert 1234 + 8 * block < nb - 200
    return a, b, (nb - 200, 1234)


# ---- pn_ransac_poses -------------------------------------------------------------------------------------------------
RANSAC = dict(max_dist=0.02, edge_ratio=0.9, wrong=0.6)
RANSAC_SHAPES = ((257, 1025, 8), (700, 2500, 9), (700, 65536, 9))      # (C, H, the seed of the pairs and of the draws)


@functools.lru_cache(maxsize=None)
def ransac_case(C, seed):
    src, tgt, true = FO.correspondences(C, RANSAC["wrong"], seed=seed)
    return src, tgt, true


LATE_FIRST, LATE_NAN, LATE_H, LATE_SEED = 512, 690, 2500, 10


@functools.lru_cache(maxsize=None)
def late_inliers(C=700, seed=10):
    """C pairs of which only rows >= LATE_FIRST (the third block of 256 pairs, a partial one) are right; the rows before are re-paired
    at random some 40 m away, so no hypothesis fitted to right pairs counts one of them; row LATE_NAN of the last block is NaN
    -> (src, tgt, true pose)"""
    rng = np.random.default_rng(seed)
    q = rng.uniform(-2.0, 2.0, (C, 3))
    R = IO.rot(rng.normal(size=3), 2.0)
    t = rng.uniform(-1.0, 1.0, 3)
    p = q @ R.T + t + rng.normal(0, 0.002, (C, 3))
    p[:LATE_FIRST] = rng.uniform(-3.0, 3.0, (LATE_FIRST, 3)) + 40.0
    p[LATE_NAN] = np.nan
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = R, t
    src, tgt = p.astype(F32), q.astype(F32)
    return src, tgt, P


# ---- pn_fpfh ---------------------------------------------------------------------------------------------------------
FLAT_K = 16
STRIP = (0.9, 1.1)       # the x range of flat_patch's tilted strip


def flat_patch(n=300, seed=0, tilt=0.0):
    """n points uniform on the 2 x 2 square at z = 0 with normals +z; ``tilt`` (rad) turns the normals of the strip STRIP about y
    -> (xyz, normals) float32"""
    rng = np.random.default_rng(seed)
    xyz = np.concatenate([rng.random((n, 2)) * 2.0, np.zeros((n, 1))], 1).astype(F32)
    nrm = np.tile(np.array([0.0, 0.0, 1.0]), (n, 1))
    strip = (xyz[:, 0] >= STRIP[0]) & (xyz[:, 0] <= STRIP[1])
    nrm[strip] = [np.sin(tilt), 0.0, np.cos(tilt)]
    return xyz, nrm.astype(F32)


# name -> (cloud, radius); k = FLAT_K.  On the lattice the 16 rows at least two steps from every edge have 20 others within 2.5, so
# their lists are full, and distances tie.
FPFH_FLAT = {
    "lattice": (lambda: FO.flat_lattice(8), 2.5),
    "patch": (lambda: flat_patch(300, 0), 0.5),
    "tilted_strip": (lambda: flat_patch(300, 0, tilt=0.6), 0.5),
}


@functools.lru_cache(maxsize=None)
def fpfh_flat(name):
    """-> (xyz, normals, radius, (out, counts, pairs) of the oracle)"""
    make, radius = FPFH_FLAT[name]
    x, n = make()
    return x, n, radius, FO.fpfh(x, n, radius, FLAT_K, return_spfh=True)


def full_rows(counts):
    """the rows with a bin that holds k"""
    return (counts == FLAT_K).any(1)


def full_bin_beside_a_counted_one(out, counts):
    """rows in which a bin holds k while the next bin of the same feature is non-zero in the descriptor (through the neighbours' rows):
    a carry out of a field too narrow for k would land in a bin that counts"""
    hit = np.zeros(len(counts), bool)
    for g in range(3):
        for c in range(g * FO.DIV, (g + 1) * FO.DIV - 1):
            hit |= (counts[:, c] == FLAT_K) & (out[:, c + 1] != 0)
    return hit


# ---- ops.global_register ---------------------------------------------------------------------------------------------
MUTUAL = dict(FO.SCENE, mutual=True)
# 16 hypotheses, fewer than keep = 32: seed 16 is the first for which the oracle has more than one valid draw among them (h = 6 and
# 13; about one draw in a hundred is valid on the fixture), so order[:keep] and the top 4 hold NaN poses next to the valid ones
FEW = dict(FO.SCENE, hypotheses=16, seed=16)
FEW_VALID = (6, 13)


def second_source(source, viewpoint):
    """the fixture's source turned 25 degrees about its viewpoint (which stays where it is), with four NaN rows"""
    c = np.asarray(viewpoint, np.float64)
    R = IO.rot([0.3, 0.5, -0.2], np.deg2rad(25.0))
    out = ((source.astype(np.float64) - c) @ R.T + c).astype(F32)
    out[[0, 7, 300, len(out) - 1]] = np.nan
    return out


LINE_H = 64


def line_scans(n=60):
    """source and target on one line: no normals, zero descriptors, every match is row 0, no valid hypothesis"""
    tgt = np.stack([np.arange(n) * 0.1, np.zeros(n), np.zeros(n)], 1).astype(F32)
    src = tgt[:n - 10] + F32(0.03)
    return src, tgt
