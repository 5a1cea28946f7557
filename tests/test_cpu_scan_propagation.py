"""pn_knn_propagate / ops.knn_propagate / PointNet.predict_scan without a GPU: the declared surface, the argument checks (they run
before any HIP call), and the NumPy oracle (tests/knn_oracle.py) against an independent formulation and a hand-worked case."""
import ctypes as C
import os

import numpy as np
import pytest

import knn_oracle as KO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
# agreement of k = 1 propagation with the ground-truth part labels on the labelled scan below, as the oracle computes it
# (voxel grid 0.25 m -> FPS 1024 -> majority label of the nearest sample); the GPU test asserts just under it
LABELLED_SCAN = dict(n=16384, leaf=0.25, samples=1024)
LABELLED_AGREEMENT = 16295 / 16384     # 0.99457


def test_surface_is_declared_and_exported():
    from pointcloudprocessing_amd import _lib, ops
    from pointcloudprocessing_amd.pointnet.PointNet import PointNet
    hdr = open(os.path.join(ROOT, "include", "pointnet_hip.h")).read()
    assert "int pn_knn_propagate(" in hdr
    assert "pn_knn_propagate" in _lib.SIGNATURES
    assert hasattr(_lib.lib(), "pn_knn_propagate")
    assert callable(ops.knn_propagate) and callable(PointNet.predict_scan)


@pytest.mark.parametrize("k,M,C_,msg", [(0, 16, 4, b"k=0"), (9, 16, 4, b"k=9"), (4, 3, 4, b"fewer than k"), (3, 16, 17, b"C=17")])
def test_argument_checks_without_gpu(k, M, C_, msg):
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    fake = C.c_void_p(0x1000)                # never dereferenced: the checks run before any HIP call
    rc = L.pn_knn_propagate(fake, fake, 1, 8, M, k, fake, C_, fake, fake, fake, fake, None)
    assert rc == -1
    assert msg in L.pn_last_error()


def test_argument_checks_pointers_and_search_only():
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    fake = C.c_void_p(0x1000)
    assert L.pn_knn_propagate(None, fake, 1, 8, 8, 3, None, 0, fake, fake, None, None, None) == -1
    assert b"null pointer" in L.pn_last_error()
    assert L.pn_knn_propagate(fake, fake, 1, 8, 8, 3, None, 4, fake, fake, None, None, None) == -1      # C without values
    assert L.pn_knn_propagate(fake, fake, 1, 8, 8, 3, fake, 4, fake, fake, None, fake, None) == -1      # values_out missing
    assert L.pn_knn_propagate(fake, fake, 0, 8, 8, 3, None, 0, fake, fake, None, None, None) == -1
    assert L.pn_knn_propagate(fake, fake, 1, 0, 8, 3, None, 0, fake, fake, None, None, None) == -1


def test_ops_wrapper_refuses_cpu_tensors():
    import torch
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd._lib import PointNetHipError
    with pytest.raises(PointNetHipError):
        ops.knn_propagate(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3), 3)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_matches_lexsort_formulation(seed):
    rng = np.random.default_rng(seed)
    B, Nq, M, k = 2, 150, 40, 5
    ref = rng.normal(size=(B, M, 3)).astype(F32)
    ref[:, 10:20] = ref[:, 0:10]                          # duplicated refs: ties
    ref[:, 25] = ref[:, 3]
    q = rng.normal(size=(B, Nq, 3)).astype(F32)
    q[:, :8] = ref[:, :8]                                 # d = 0, tied with the duplicates
    q[0, 9] = np.nan                                      # every distance NaN
    ref[1, 30, 1] = np.nan                                # one ref never chosen
    q[1, 11] = [1e30, 0, 0]                               # overflows to +inf: filled slots with d = +inf
    a = KO.knn(q, ref, k, chunk=37)
    b = KO.knn_lexsort(q, ref, k)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert (a[0][0, 9] == -1).all() and np.isinf(a[1][0, 9]).all()
    assert (a[0][1, 11] >= 0).all() and np.isinf(a[1][1, 11]).all()
    assert 30 not in a[0][1]
    # ties go to the lowest index: query i < 8 sits on ref i and on its copy i + 10
    assert (a[0][:, :8, 0] == np.arange(8)).all() and (a[0][:, :8, 1] == np.arange(8) + 10).all()


def test_oracle_interpolation_by_hand():
    ref = np.array([[[0, 0, 0], [3, 0, 0], [0, 0, 10]]], F32)
    q = np.array([[[1, 0, 0]]], F32)
    vals = np.array([[[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [9.0, 9.0, 9.0]]], F32)
    idx, d2 = KO.knn(q, ref, 2)
    assert idx.tolist() == [[[0, 1]]] and d2.tolist() == [[[1.0, 4.0]]]
    out, arg = KO.interpolate(idx, d2, vals)
    w0 = F32(1) / (F32(1) + F32(1e-8))
    w1 = F32(1) / (F32(2) + F32(1e-8))
    sw = F32(F32(0) + w0) + w1
    exp = np.array([F32(F32(0) + w0 * F32(1)) / sw, F32(F32(F32(0) + w0 * F32(0)) + w1 * F32(1)) / sw,
                    F32(F32(F32(0) + w0 * F32(0.5)) + w1 * F32(0.5)) / sw], F32)
    assert np.array_equal(out[0, 0], exp)
    assert abs(float(out[0, 0, 0]) - 2 / 3) < 1e-6 and abs(float(out[0, 0, 1]) - 1 / 3) < 1e-6
    assert arg.tolist() == [[0]]
    # a tie of the maxima -> the first; no neighbour -> arg -1
    out, arg = KO.interpolate(np.array([[[0, -1]]], np.int32), np.array([[[0.0, np.inf]]], F32), np.array([[[2.0, 2.0, 1.0]]], F32))
    assert arg.tolist() == [[0]]
    out, arg = KO.interpolate(np.array([[[-1]]], np.int32), np.array([[[np.inf]]], F32), np.array([[[2.0, 2.0, 1.0]]], F32))
    assert arg.tolist() == [[-1]] and np.isnan(out).all()


def labelled_scan_agreement():
    """voxel grid with labels -> FPS -> k = 1 propagation of the samples' majority labels, all in the NumPy oracles"""
    from oracle import sampling_oracle as SO
    xyz, gt = KO.labelled_scan(LABELLED_SCAN["n"])
    origin = xyz.min(0)
    leaf = (LABELLED_SCAN["leaf"],) * 3
    cent, _, maj = SO.voxel_downsample(xyz, leaf, origin, labels=gt, n_labels=12)
    fi, _ = SO.fps(cent, LABELLED_SCAN["samples"], 0)
    idx, _ = KO.knn(xyz[None], cent[fi][None], 1)
    return float(np.mean(maj[fi][idx[0, :, 0]] == gt))


def test_labelled_scan_agreement_oracle():
    a = labelled_scan_agreement()
    assert abs(a - LABELLED_AGREEMENT) < 1e-9, a
