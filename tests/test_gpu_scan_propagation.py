"""pn_knn_propagate on the MI355X: exact k-NN search and inverse-distance interpolation bit for bit against the NumPy oracle
(tests/knn_oracle.py), memory safety by guard bands, graph capture, and PointNet.predict_scan on BASELINE config 5 at full size."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import knn_oracle as KO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
GUARD = 4096          # bytes of fill pattern before and after every output buffer
PAT = 0xA5


def _cloud(rng, B, Nq, M, offset=0.0):
    ref = (rng.normal(size=(B, M, 3)) * 4 + offset).astype(F32)
    if M >= 8:
        ref[:, M // 2:M // 2 + M // 8] = ref[:, :M // 8]                     # duplicated refs: ties in distance
    q = (rng.normal(size=(B, Nq, 3)) * 4 + offset).astype(F32)
    n_eq = min(Nq, M, 16)
    q[:, :n_eq] = ref[:, :n_eq]                                              # queries on refs: d = 0 (tied with the duplicates)
    return q, ref


def _guarded(shape, dtype, dev):
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((GUARD + n + GUARD,), PAT, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + n].view(dtype).view(*shape)


def _intact(buf):
    return bool((buf[:GUARD] == PAT).all()) and bool((buf[-GUARD:] == PAT).all())


def _raw(q, r, k, values=None):
    """pn_knn_propagate on guard-banded outputs; returns the outputs and asserts the bands and the inputs are untouched"""
    from pointcloudprocessing_amd import _lib
    B, Nq, _ = q.shape
    M = r.shape[1]
    C_ = values.shape[2] if values is not None else 0
    dev = q.device
    keep = [t.clone() for t in (q, r) + ((values,) if values is not None else ())]
    bufs = dict(idx=_guarded((B, Nq, k), torch.int32, dev), d2=_guarded((B, Nq, k), torch.float32, dev))
    if values is not None:
        bufs["vout"] = _guarded((B, Nq, C_), torch.float32, dev)
        bufs["arg"] = _guarded((B, Nq), torch.int32, dev)
    p = lambda name: C.c_void_p(bufs[name][1].data_ptr()) if name in bufs else None      # noqa: E731
    rc = _lib.lib().pn_knn_propagate(_lib.ptr(q), _lib.ptr(r), B, Nq, M, k, _lib.ptr(values), C_, p("idx"), p("d2"), p("vout"),
                                     p("arg"), _lib.current_stream())
    _lib.check(rc, "pn_knn_propagate")
    torch.cuda.synchronize()
    for name, (buf, _) in bufs.items():
        assert _intact(buf), f"{name}: guard band overwritten"
    for a, b in zip(keep, (q, r) + ((values,) if values is not None else ())):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "an input was modified"      # bitwise: NaN inputs included
    return {name: v.cpu().numpy() for name, (_, v) in bufs.items()}


@pytest.mark.parametrize("B,Nq,M,k,offset", [(1, 1, 1, 1, 0.0), (2, 1000, 37, 3, 0.0), (3, 64, 5, 5, 1e3), (1, 4097, 8192, 8, 0.0),
                                             (2, 5000, 300, 4, 1e3)])
def test_search_bit_exact(dev, B, Nq, M, k, offset):
    rng = np.random.default_rng(B * 1000 + Nq + M + k)
    q, ref = _cloud(rng, B, Nq, M, offset)
    out = _raw(torch.from_numpy(q).to(dev), torch.from_numpy(ref).to(dev), k)
    ri, rd = KO.knn(q, ref, k)
    assert np.array_equal(out["idx"], ri), np.argwhere(out["idx"] != ri)[:5]
    assert np.array_equal(out["d2"].view(np.uint32), rd.view(np.uint32))
    assert (ri >= 0).all()


@pytest.mark.parametrize("C_", [1, 12, 16])
@pytest.mark.parametrize("split", ["1", "2", "4"])
def test_interpolation_bit_exact(dev, monkeypatch, C_, split):
    monkeypatch.setenv("PN_KNN_SPLIT", split)
    rng = np.random.default_rng(C_)
    B, Nq, M, k = 2, 3000, 500, 3
    q, ref = _cloud(rng, B, Nq, M, 50.0)
    vals = (rng.integers(0, 3, size=(B, M, C_)) * 0.5).astype(F32)          # few levels: tied maxima are common
    vals[0, :, 0] = vals[0, :, C_ - 1]
    out = _raw(torch.from_numpy(q).to(dev), torch.from_numpy(ref).to(dev), k, torch.from_numpy(vals).to(dev))
    ri, rd = KO.knn(q, ref, k)
    rv, ra = KO.interpolate(ri, rd, vals)
    assert np.array_equal(out["idx"], ri) and np.array_equal(out["d2"], rd)
    assert np.array_equal(out["vout"].view(np.uint32), rv.view(np.uint32))
    assert np.array_equal(out["arg"], ra)
    if C_ > 1:
        top = np.sort(rv, axis=2)
        assert (top[..., -1] == top[..., -2]).sum() > 50                    # the tie rule was exercised


def knn_case_sizes(k):
    return (k, 37)


def knn_case(k, M):
    """two clouds of 130 queries (a last tile of two lanes) on M refs with 5 value channels of few levels; the first queries lie on
    refs.  tests/test_cpu_sampler_cases.py checks on the oracle that every case has a query at d = 0 and a tied maximum."""
    rng = np.random.default_rng(1000 * k + M)
    q, ref = _cloud(rng, 2, 130, M)
    vals = (rng.integers(0, 3, size=(2, M, 5)) * 0.5).astype(F32)
    vals[0, :, 0] = vals[0, :, 4]
    return q, ref, vals


@pytest.mark.parametrize("split", ["1", "2", "4"])
@pytest.mark.parametrize("k,M", [(k, M) for k in range(1, 9) for M in knn_case_sizes(k)])
def test_every_k_instantiation_bit_exact(dev, monkeypatch, k, M, split):
    """knn_propagate_kernel<K> for every K = 1 .. 8, search and interpolation, under every split of the refs over waves; at M = k
    every wave's slice is shorter than k, so every list reaches the merge with empty slots"""
    monkeypatch.setenv("PN_KNN_SPLIT", split)
    q, ref, vals = knn_case(k, M)
    out = _raw(torch.from_numpy(q).to(dev), torch.from_numpy(ref).to(dev), k, torch.from_numpy(vals).to(dev))
    ri, rd = KO.knn(q, ref, k)
    rv, ra = KO.interpolate(ri, rd, vals)
    assert (rd[:, :, 0] == 0).any()
    top = np.sort(rv, axis=2)
    assert (top[..., -1] == top[..., -2]).any()
    assert np.array_equal(out["idx"], ri), np.argwhere(out["idx"] != ri)[:5]
    assert np.array_equal(out["d2"].view(np.uint32), rd.view(np.uint32))
    assert np.array_equal(out["vout"].view(np.uint32), rv.view(np.uint32))
    assert np.array_equal(out["arg"], ra)


def test_search_only_and_nan_rows(dev):
    from pointcloudprocessing_amd import ops
    rng = np.random.default_rng(7)
    q, ref = _cloud(rng, 1, 300, 120)
    q[0, 5] = np.nan
    q[0, 6, 1] = np.nan
    ref[0, 40] = np.nan                                                    # a NaN ref is never a neighbour
    vals = rng.random(size=(1, 120, 12)).astype(F32)
    outs = ops.knn_propagate(torch.from_numpy(q).to(dev), torch.from_numpy(ref).to(dev), 4)
    assert len(outs) == 2
    raw = _raw(torch.from_numpy(q).to(dev), torch.from_numpy(ref).to(dev), 4, torch.from_numpy(vals).to(dev))
    ri, rd = KO.knn(q, ref, 4)
    rv, ra = KO.interpolate(ri, rd, vals)
    assert np.array_equal(outs[0].cpu().numpy(), ri) and np.array_equal(outs[1].cpu().numpy(), rd)
    assert np.array_equal(raw["idx"], ri) and np.array_equal(raw["d2"], rd)
    for row in (5, 6):
        assert (raw["idx"][0, row] == -1).all() and np.isposinf(raw["d2"][0, row]).all()
        assert raw["arg"][0, row] == -1 and np.isnan(raw["vout"][0, row]).all()
    assert 40 not in raw["idx"]
    assert np.array_equal(raw["vout"], rv, equal_nan=True) and np.array_equal(raw["arg"], ra)


def test_graph_capture_replay_matches_eager(dev):
    from pointcloudprocessing_amd import ops
    rng = np.random.default_rng(11)
    q, ref = _cloud(rng, 2, 2000, 700)
    vals = rng.random(size=(2, 700, 12)).astype(F32)
    qd, rd_, vd = (torch.from_numpy(a).to(dev) for a in (q, ref, vals))
    eager = ops.knn_propagate(qd, rd_, 3, values=vd)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.knn_propagate(qd, rd_, 3, values=vd)                           # warm-up on the capture stream
        with torch.cuda.graph(g, stream=side):
            captured = ops.knn_propagate(qd, rd_, 3, values=vd)
    torch.cuda.current_stream().wait_stream(side)
    for t in captured:
        t.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)


def test_errors_raise_through_ops(dev):
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd._lib import PointNetHipError
    q = torch.zeros(1, 10, 3, device=dev)
    r = torch.zeros(1, 6, 3, device=dev)
    for kw in (dict(k=0), dict(k=9), dict(k=7), dict(k=3, values=torch.zeros(1, 6, 17, device=dev)),
               dict(k=3, values=torch.zeros(1, 5, 4, device=dev))):
        with pytest.raises(PointNetHipError):
            ops.knn_propagate(q, r, **kw)
    with pytest.raises(PointNetHipError):
        ops.knn_propagate(q, torch.zeros(2, 6, 3, device=dev), 3)
    with pytest.raises(PointNetHipError):
        ops.knn_propagate(q, r.double(), 3)


def test_labelled_scan_agreement(dev):
    import test_cpu_scan_propagation as CPU
    from pointcloudprocessing_amd import ops
    xyz, gt = KO.labelled_scan(CPU.LABELLED_SCAN["n"])
    x = torch.from_numpy(xyz).to(dev)
    cent, _, maj = ops.voxel_downsample(x, (CPU.LABELLED_SCAN["leaf"],) * 3, xyz.min(0), labels=torch.from_numpy(gt).to(dev),
                                        n_labels=12)
    fi = ops.farthest_point_sample(cent.unsqueeze(0).contiguous(), CPU.LABELLED_SCAN["samples"])[0].long()
    onehot = torch.nn.functional.one_hot(maj[fi].long(), 12).float().unsqueeze(0).contiguous()
    _, _, _, part = ops.knn_propagate(x.unsqueeze(0), cent[fi].unsqueeze(0).contiguous(), 1, values=onehot)
    agree = float((part[0].cpu().numpy() == gt).mean())
    assert agree >= CPU.LABELLED_AGREEMENT - 1e-3, agree


def test_c5_full_scan_propagation(dev):
    """BASELINE config 5 at full size: N = 131072 -> voxel grid 0.25 m -> FPS 8192 -> PointNet segmentation probabilities ->
    knn_propagate(k = 3) on every scan point; every 8th query bit-exact against the oracle; predict_scan equals this composition."""
    spec = importlib.util.spec_from_file_location("bench_scan", os.path.join(ROOT, "tools", "bench_scan.py"))
    bs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bs)
    from oracle import pointnet_oracle as O            # checker only
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd.pointnet.PointNet import PointNet
    xyz, origin = bs.make_scan(131072)
    x = torch.from_numpy(xyz).to(dev)
    cent, _, _ = ops.voxel_downsample(x, (0.25,) * 3, origin)
    M = 8192
    assert cent.shape[0] > M
    idx = ops.farthest_point_sample(cent.unsqueeze(0).contiguous(), M)
    sampled = cent[idx[0].long()].unsqueeze(0).contiguous()
    params = O.init_params(23, 12, seed=29, vanilla=True, randomize_bn=True)
    model = PointNet(23, 12, 0.3, 42, vanilla=True, precision="bf16", device=dev)
    model.set_weights(params)
    _, seg, _ = model(sampled, training=False)
    seg = seg.contiguous()
    ki, kd, kv, ka = ops.knn_propagate(x.unsqueeze(0), sampled, 3, values=seg)
    sub = xyz[None, ::8].copy()
    ri, rd = KO.knn(sub, sampled.cpu().numpy(), 3)
    rv, ra = KO.interpolate(ri, rd, seg.cpu().numpy())
    assert np.array_equal(ki[:, ::8].cpu().numpy(), ri) and np.array_equal(kd[:, ::8].cpu().numpy(), rd)
    assert np.array_equal(kv[:, ::8].cpu().numpy().view(np.uint32), rv.view(np.uint32))
    assert np.array_equal(ka[:, ::8].cpu().numpy(), ra)
    ci, part, R = model.predict_scan(x, leaf=0.25, samples=M, k=3, origin=origin)
    assert tuple(ci.shape) == (1,) and tuple(part.shape) == (1, 131072) and tuple(R.shape) == (1, 3, 3)
    assert torch.equal(part, ka)
    assert int(ci[0]) == int(model.predict(sampled)[0][0])
    assert int(part.min()) >= 0 and int(part.max()) < 12


def test_predict_scan_small_scan_uses_every_voxel(dev):
    """V <= samples: no FPS, all centroids in voxel order; default origin = the scan's per-axis minimum"""
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd.pointnet.PointNet import PointNet
    from oracle import pointnet_oracle as O
    xyz, _ = KO.labelled_scan(3000, seed=3)
    x = torch.from_numpy(xyz).to(dev)
    model = PointNet(23, 12, 0.3, 42, precision="bf16", device=dev)
    model.set_weights(O.init_params(23, 12, seed=4, randomize_bn=True))
    ci, part, R = model.predict_scan(x, leaf=0.5, samples=100000, k=2)
    cent, _, _ = ops.voxel_downsample(x, (0.5,) * 3, xyz.min(0))
    cls, seg, R2 = model(cent.unsqueeze(0).contiguous(), training=False)
    _, _, _, ref_part = ops.knn_propagate(x.unsqueeze(0), cent.unsqueeze(0).contiguous(), 2, values=seg.contiguous())
    assert torch.equal(part, ref_part) and torch.equal(R, R2) and int(ci[0]) == int(cls.argmax(-1)[0])
