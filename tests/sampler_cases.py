"""Input builders for the voxel-grid, FPS and k-NN tests -- TEST INFRASTRUCTURE, pure NumPy.

Every builder makes ONE path of a kernel the path that runs (one digit position of the voxel grid's radix sort, one launch shape
of the FPS kernel, ...).  tests/test_cpu_sampler_cases.py checks on the oracles alone that each input does what its case says;
tests/test_gpu_voxel.py and tests/test_gpu_fps.py run the same inputs through the kernels.  Every case is a pure function of its
parameters (its own seeded generator), so both sides see the same bits.
"""
from __future__ import annotations

import zlib

import numpy as np

F32 = np.float32
VX_POS = 9                       # digit positions of the voxel grid's LSD radix sort (pn_voxel.hip)
KEY_LIMIT = 1 << 21              # per-axis voxel indices lie in [0, 2^21)
ALL_POS = list(range(VX_POS))


def _rng(*tag):
    return np.random.default_rng(zlib.crc32(repr(tag).encode()))


# ------------------------------------------------------------------------------------------------------------ voxel grid
def digit_shift(p: int) -> int:
    """bit offset of digit position p in the 63-bit key (kz << 42) | (ky << 21) | kx"""
    return (p // 3) * 21 + (p % 3) * 8


def digit_bits(p: int) -> int:
    return 5 if p % 3 == 2 else 8


def dead_digit(p: int) -> int:
    """the one digit a dead position holds: fixed and non-zero, so a dead position is "one occupied bin", not "bin 0" """
    return (37 * (p + 1)) % ((1 << digit_bits(p)) - 1) + 1


def key_digits(k: np.ndarray) -> np.ndarray:
    """per-axis indices (N,3) -> the nine digits (N,9) of every key"""
    k = np.asarray(k, np.int64)
    key = (k[:, 2] << 42) | (k[:, 1] << 21) | k[:, 0]
    return np.stack([(key >> digit_shift(p)) & ((1 << digit_bits(p)) - 1) for p in ALL_POS], axis=1)


def live_positions(k: np.ndarray):
    """the digit positions with more than one occupied digit: the passes of the sort that do work"""
    d = key_digits(k)
    return [p for p in ALL_POS if len(np.unique(d[:, p])) > 1]


def _pool_voxels(rng, live, pool):
    """`pool` distinct voxels as digits (pool', 9): random digits at the live positions, dead_digit elsewhere.  pool' = pool unless
    the live positions have fewer combinations."""
    bits = sum(digit_bits(p) for p in live)
    if bits <= 20:
        space = 1 << bits
        pool = min(pool, space)
        codes = rng.permutation(space)[:pool].astype(np.int64)
    else:
        codes = np.zeros(0, np.int64)
        while len(codes) < pool:
            more = (rng.integers(0, 1 << 64, size=2 * pool, dtype=np.uint64) & np.uint64((1 << bits) - 1)).astype(np.int64)
            codes = np.unique(np.concatenate([codes, more]))
        codes = rng.permutation(codes)[:pool]
    dig = np.empty((pool, VX_POS), np.int64)
    at = 0
    for p in ALL_POS:
        if p in live:
            dig[:, p] = (codes >> at) & ((1 << digit_bits(p)) - 1)
            at += digit_bits(p)
        else:
            dig[:, p] = dead_digit(p)
    return dig


def _digits_to_indices(dig):
    key = np.zeros(dig.shape[0], np.int64)
    for p in ALL_POS:
        key |= dig[:, p] << digit_shift(p)
    m = KEY_LIMIT - 1
    return np.stack([key & m, (key >> 21) & m, (key >> 42) & m], axis=1)


def voxel_keys(rng, N: int, live, pool: int, member=None) -> np.ndarray:
    """Per-axis 21-bit voxel indices (N,3) int64 of N points over `pool` distinct voxels: the digit positions in `live` take random
    digits, every other position holds dead_digit(p).  member (N,), optional: which pool voxel each point falls into (default:
    uniformly random)."""
    vox = _digits_to_indices(_pool_voxels(rng, list(live), pool))
    if member is None:
        member = rng.integers(0, len(vox), size=N)
    return vox[np.asarray(member) % len(vox)]


def key_coordinates(rng, k: np.ndarray) -> np.ndarray:
    """fp32 coordinates k + f, f in {0.25, 0.5, 0.75}: exact for every k < 2^21, so with leaf 1 and origin 0 the keys are k"""
    f = rng.integers(1, 4, size=k.shape).astype(F32) * F32(0.25)
    return (k.astype(F32) + f).astype(F32)


UNIT_LEAF = (1.0, 1.0, 1.0)
ZERO_ORIGIN = (0.0, 0.0, 0.0)
N_LABELS = 32

VOXEL_LIVE_SETS = [[]] + [[p] for p in ALL_POS] + [[0, 1], [2, 5, 8], [0, 3, 6, 7], ALL_POS]
VOXEL_SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 8192, 8193, 9217, 16385, 262144, 262145, 300000]
VOXEL_ORDERS = ["sorted", "reversed", "skewed"]
VOXEL_REFUSALS = ["below_origin", "key_2_21", "nan", "inf"]


def _voxel_case(rng, k, live, labels=True):
    xyz = key_coordinates(rng, k)
    lab = rng.integers(0, N_LABELS, size=len(k)).astype(np.int32) if labels else None
    return dict(xyz=xyz, k=k, live=list(live), labels=lab, n_labels=N_LABELS if labels else 0, leaf=UNIT_LEAF, origin=ZERO_ORIGIN)


def voxel_live_case(live):
    """(a) N = 3000 points over 600 voxels (fewer where the live digits have fewer combinations); labels over all 32 values"""
    rng = _rng("live", tuple(live))
    return _voxel_case(rng, voxel_keys(rng, 3000, live, 600), live)


def voxel_size_case(N: int):
    """(b) all nine positions live over max(1, N // 4) voxels (a single point leaves no position live)"""
    rng = _rng("size", N)
    k = voxel_keys(rng, N, ALL_POS, max(1, N // 4))
    return _voxel_case(rng, k, ALL_POS if N > 1 else [])


def voxel_order_case(kind: str):
    """(c) N = 20000, live [0, 1, 3, 6]: the points already in (kz, ky, kx) order, in reverse order, or 99 % of them in one voxel"""
    rng = _rng("order", kind)
    N, live = 20000, [0, 1, 3, 6]
    member = None
    if kind == "skewed":
        member = np.where(rng.random(N) < 0.99, 0, rng.integers(0, 5000, size=N))
    k = voxel_keys(rng, N, live, 5000, member)
    if kind in ("sorted", "reversed"):
        order = np.argsort((k[:, 2] << 42) | (k[:, 1] << 21) | k[:, 0], kind="stable")
        k = k[order[::-1] if kind == "reversed" else order]
    return _voxel_case(rng, k, live)


FACE_LEAF = F32(0.1)
FACE_ORIGIN = F32(-3.7)
FACE_K = 399


def voxel_face_case(axis: int):
    """(d) points on and next to the voxel faces of a non-dyadic grid along one axis: fl(o + fl(k * leaf)) for k = 1 .. 399 and the
    fp32 neighbour on each side of every one (1197 points); the other two axes are constant.  Many of these keys differ from the
    same formula in higher precision, so a kernel that contracts, reorders or approximates subtract-divide-floor changes counts."""
    kk = np.arange(1, FACE_K + 1).astype(F32)
    face = (FACE_ORIGIN + (kk * FACE_LEAF).astype(F32)).astype(F32)
    line = np.concatenate([np.nextafter(face, F32(-np.inf)), face, np.nextafter(face, F32(np.inf))]).astype(F32)
    line = _rng("face", axis).permutation(line)
    xyz = np.full((len(line), 3), F32(1.25), F32)
    xyz[:, axis] = line
    return dict(xyz=xyz, axis=axis, labels=None, n_labels=0, leaf=(FACE_LEAF,) * 3, origin=(FACE_ORIGIN,) * 3)


def face_keys_fp64(case) -> np.ndarray:
    """the keys of a face case along its axis with the oracle's formula evaluated in float64 on the same fp32 inputs"""
    x = case["xyz"][:, case["axis"]].astype(np.float64)
    return np.floor((x - np.float64(FACE_ORIGIN)) / np.float64(FACE_LEAF)).astype(np.int64)


BAD_LABELS = (-1, N_LABELS, 1000)


def voxel_bad_label_case():
    """(e) labels -1, n_labels and 1000 mixed into valid ones (they are ignored); the points of every fifth voxel carry only such
    labels (the voxel reports 0)"""
    rng = _rng("bad labels")
    live = [0, 3, 6]
    N, pool = 3000, 400
    member = rng.integers(0, pool, size=N)
    case = _voxel_case(rng, voxel_keys(rng, N, live, pool, member), live)
    lab = case["labels"]
    bad = rng.random(N) < 0.3
    bad |= member % 5 == 0
    lab[bad] = rng.choice(BAD_LABELS, size=int(bad.sum()))
    case["all_bad_points"] = member % 5 == 0
    return case


def voxel_refusal_case(kind: str):
    """(g) a valid cloud in which exactly point `bad` is refused: below the origin, a key of exactly 2^21, a NaN, a +Inf"""
    rng = _rng("refusal", kind)
    case = _voxel_case(rng, voxel_keys(rng, 3000, [0, 3, 6], 600), [0, 3, 6])
    bad, axis = 1234, VOXEL_REFUSALS.index(kind) % 3
    case["xyz"][bad, axis] = {"below_origin": F32(-0.25), "key_2_21": F32(KEY_LIMIT) + F32(0.25), "nan": F32(np.nan),
                              "inf": F32(np.inf)}[kind]
    case["bad"] = bad
    return case


# ------------------------------------------------------------------------------------------------------------------- FPS
FPS_SINGLE_BLOCK_MAX = 21504     # clouds above this are split over blocks of FPS_BLOCK points (pn_sample.hip)
FPS_BLOCK = 16384
FPS_TAG_PERIOD = 4096            # the round tag of the cross-block granule has 12 bits

# name -> (B, N, M, start_idx)
FPS_CASES = {
    "clouds_x_blocks": (3, 40000, 64, 39999),
    "two_launches": (65, 21505, 8, 7),
    "tag_wrap": (1, 21505, 4200, 0),
    "largest_cloud": (1, 1048576, 6, 1048575),
    "one_point_block": (1, 32769, 50, 32768),
    "block_boundary": (1, 32768, 50, 0),
    "cross_block_ties": (1, 40000, 40, 0),
    "plain_1000": (2, 1000, 50, 999),
    "plain_4000": (1, 4000, 50, 3999),
    "plain_16000": (1, 16000, 50, 15999),
    "plain_21000": (1, 21000, 50, 20999),
    "m1_small": (2, 300, 1, 0),
    "m1_multi_block": (1, 40000, 1, 0),
    "m_above_n": (2, 17, 25, 3),
}
FPS_TIE_PAIRS = [(1000 + 1900 * c, 33000 + 800 * c) for c in range(8)]       # (corner, its copy in another block)


def fps_block_of(i):
    return np.asarray(i) // FPS_BLOCK


def fps_cloud(name: str) -> np.ndarray:
    """(B, N, 3) fp32, uniform in [-10, 10]^3, every cloud different; "cross_block_ties" adds the eight corners of [-30, 30]^3 below
    index 16384 and an exact copy of each above 32768: the corners are drawn in the first rounds, each tied with its copy"""
    B, N, _, _ = FPS_CASES[name]
    xyz = _rng("fps", name).uniform(-10, 10, size=(B, N, 3)).astype(F32)
    if name == "cross_block_ties":
        for c, (lo, hi) in enumerate(FPS_TIE_PAIRS):
            xyz[0, lo] = [30.0 if (c >> a) & 1 else -30.0 for a in range(3)]
            xyz[0, hi] = xyz[0, lo]
    return xyz


FPS_PRUNED_CASE = (2, 8000, 600, 4000)       # B, N, M, start_idx


def fps_ordered_grid() -> np.ndarray:
    """(2, 8000, 3): jittered grid points in (z, y, x) order, as the voxel grid leaves them -- the input the pruned kernel is built
    for -- with a different jitter per cloud and duplicated points inside a group, between groups of a wave and between waves"""
    B, N, _, _ = FPS_PRUNED_CASE
    side = int(np.ceil(N ** (1.0 / 3.0))) + 1
    gi = np.stack(np.meshgrid(np.arange(side), np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 3)[:N]
    rng = _rng("fps pruned")
    xyz = (gi[None, :, ::-1] * 0.25 + rng.uniform(-0.1, 0.1, size=(B, N, 3))).astype(F32)
    xyz[:, 70:75] = xyz[:, 10:15]
    xyz[:, 3000:3004] = xyz[:, 200:204]
    xyz[:, N - 3:] = xyz[:, N - 6:N - 3]
    return xyz
