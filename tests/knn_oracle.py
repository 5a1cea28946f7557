"""NumPy oracle of pn_knn_propagate (include/pointnet_hip.h) -- TEST INFRASTRUCTURE.

Exact k-nearest-neighbour search and inverse-distance interpolation, stated the plain way: fp32 distances
d = (dx*dx + dy*dy) + dz*dz (NumPy float32 arithmetic never contracts to FMA), k rounds of first-argmin with
masking (ties -> lowest ref index, NaN distances never chosen), then w_t = 1 / (sqrt(d_t) + 1e-8) and the two
sums over the filled slots, t ascending, in float32.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
EMPTY_KEY = np.int64(0x7F800001)       # above every non-NaN distance key


def distances(q: np.ndarray, r: np.ndarray) -> np.ndarray:
    """q (Nq,3), r (M,3) float32 -> (Nq, M) float32 squared distances, evaluated as specified"""
    with np.errstate(over="ignore", invalid="ignore"):
        dx = q[:, None, 0] - r[None, :, 0]
        dy = q[:, None, 1] - r[None, :, 1]
        dz = q[:, None, 2] - r[None, :, 2]
        return (dx * dx + dy * dy) + dz * dz


def _keys(d: np.ndarray) -> np.ndarray:
    """int64 sort keys: the fp32 bit pattern (order-preserving for d >= +0, +inf included); NaN -> beyond EMPTY_KEY"""
    key = d.view(np.uint32).astype(np.int64)
    key[np.isnan(d)] = EMPTY_KEY + 1
    return key


def knn(query: np.ndarray, ref: np.ndarray, k: int, chunk: int = 1024):
    """query (B,Nq,3), ref (B,M,3) float32 -> idx (B,Nq,k) int32, d2 (B,Nq,k) float32; empty slot = (-1, +inf)"""
    query = np.asarray(query, F32)
    ref = np.asarray(ref, F32)
    B, Nq, _ = query.shape
    idx = np.full((B, Nq, k), -1, np.int32)
    d2 = np.full((B, Nq, k), np.inf, F32)
    for b in range(B):
        for s in range(0, Nq, chunk):
            d = distances(query[b, s:s + chunk], ref[b])
            key = _keys(d)
            rows = np.arange(d.shape[0])
            for t in range(k):
                j = np.argmin(key, axis=1)                      # first minimum: lowest index among equal keys
                ok = key[rows, j] < EMPTY_KEY
                idx[b, s:s + chunk, t] = np.where(ok, j, -1)
                d2[b, s:s + chunk, t] = np.where(ok, d[rows, j], F32(np.inf))
                key[rows, j] = EMPTY_KEY + 2                    # masked: never chosen again
    return idx, d2


def knn_lexsort(query: np.ndarray, ref: np.ndarray, k: int):
    """independent formulation for the oracle's own check: per query, np.lexsort on (j, d) over the non-NaN distances"""
    query = np.asarray(query, F32)
    ref = np.asarray(ref, F32)
    B, Nq, _ = query.shape
    idx = np.full((B, Nq, k), -1, np.int32)
    d2 = np.full((B, Nq, k), np.inf, F32)
    for b in range(B):
        d = distances(query[b], ref[b])
        for i in range(Nq):
            j = np.flatnonzero(~np.isnan(d[i]))
            o = j[np.lexsort((j, d[i, j]))][:k]
            idx[b, i, :len(o)] = o
            d2[b, i, :len(o)] = d[i, o]
    return idx, d2


def interpolate(idx: np.ndarray, d2: np.ndarray, values: np.ndarray):
    """idx / d2 (B,Nq,k) from knn(), values (B,M,C) float32 -> (values_out (B,Nq,C) float32, arg (B,Nq) int32)"""
    values = np.asarray(values, F32)
    B, Nq, k = idx.shape
    C = values.shape[2]
    sw = np.zeros((B, Nq), F32)
    acc = np.zeros((B, Nq, C), F32)
    for t in range(k):
        filled = idx[:, :, t] >= 0
        with np.errstate(divide="ignore"):
            w = F32(1) / (np.sqrt(d2[:, :, t]) + F32(1e-8))
        w = np.where(filled, w, F32(0)).astype(F32)
        v = np.take_along_axis(values, np.maximum(idx[:, :, t], 0)[:, :, None].astype(np.int64), axis=1)
        sw = np.where(filled, sw + w, sw).astype(F32)
        acc = np.where(filled[:, :, None], acc + w[:, :, None] * v, acc).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = (acc / sw[:, :, None]).astype(F32)
    arg = np.argmax(out, axis=2).astype(np.int32)              # first maximum; a NaN counts as the maximum
    arg[idx[:, :, 0] < 0] = -1
    return out, arg


def labelled_scan(n: int, seed: int = 20261016):
    """A labelled dense scan of the reference's kc-46 cloud (tests/golden/kc-46.txt): each point a random reference point plus
    N(0, 0.15 m) noise, labelled with that point's part id (helpers.F15_PARTS order).  Returns (xyz (n,3) f32, labels (n,) i32)."""
    import os
    import re
    from helpers import F15_PARTS, GOLD
    pts, lab = [], []
    for line in open(os.path.join(GOLD, "kc-46.txt")):
        m = re.match(r"\(([^)]*)\)\s*(\S+)\s+(\S+)", line.strip())
        pts.append([float(v) for v in m.group(1).split(",")])
        lab.append(F15_PARTS.index(m.group(3)))
    pts = np.asarray(pts, F32)
    lab = np.asarray(lab, np.int32)
    rng = np.random.default_rng(seed)
    src = rng.integers(0, len(pts), n)
    xyz = (pts[src] + rng.normal(0, 0.15, size=(n, 3)).astype(F32)).astype(F32)
    return xyz, lab[src]
