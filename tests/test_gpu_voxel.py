"""pn_voxel_downsample on the MI355X, bit for bit against the NumPy oracle (oracle/sampling_oracle.py) on inputs built so that each
path of the hand-written radix sort is the one that runs (tests/sampler_cases.py; tests/test_cpu_sampler_cases.py checks the
inputs): every digit position alone and in combination, both parities of the pass count and no pass at all, 4 and 16 keys per
thread, the tile-size edges of the sort, heads and look-back kernels, sorted / reversed / skewed input, voxel faces of a
non-dyadic grid, 32 labels and labels out of range, a dirty reused workspace with guard-banded outputs, and the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import sampler_cases as SC
from oracle import sampling_oracle as SO

pytestmark = pytest.mark.gpu
GUARD = 4096          # bytes of fill pattern before and after every output buffer
PAT = 0xA5
PN_ERR_INVALID_ARGUMENT = -1


def _compare(dev, case):
    """ops.voxel_downsample against the oracle on one case: centroids, counts and majority, exactly"""
    from pointcloudprocessing_amd import ops
    xyz, lab = case["xyz"], case["labels"]
    cent, cnt, maj = ops.voxel_downsample(torch.from_numpy(xyz).to(dev), case["leaf"], case["origin"],
                                          torch.from_numpy(lab).to(dev) if lab is not None else None, case["n_labels"])
    rc, rn, rm = SO.voxel_downsample(xyz, case["leaf"], case["origin"], lab, case["n_labels"])
    cent, cnt = cent.cpu().numpy(), cnt.cpu().numpy()
    assert cent.shape == rc.shape and cnt.shape == rn.shape
    assert int(cnt.sum()) == len(xyz)
    assert np.array_equal(cnt, rn), np.flatnonzero(cnt != rn)[:5]
    assert np.array_equal(cent.view(np.uint32), rc.view(np.uint32)), np.argwhere(cent != rc)[:5]
    if lab is None:
        assert maj is None and rm is None
    else:
        assert np.array_equal(maj.cpu().numpy(), rm), np.flatnonzero(maj.cpu().numpy() != rm)[:5]
    return rc, rn, rm


def _live(case):
    return SC.live_positions(SO.voxel_indices(case["xyz"], case["leaf"], case["origin"]))


@pytest.mark.parametrize("live", SC.VOXEL_LIVE_SETS, ids=lambda v: "live" + "".join(map(str, v)))
def test_digit_positions(dev, live):
    """(a) each of the nine digit positions alone, none, and 2, 3, 4 and 9 together: both parities of the pass count"""
    case = SC.voxel_live_case(live)
    assert _live(case) == live
    _compare(dev, case)


@pytest.mark.parametrize("N", SC.VOXEL_SIZES)
def test_sizes(dev, N):
    """(b) nine live passes at the tile edges: below, at and above one wave, the sort tile (1024), the heads tile (2048), eight and
    nine tiles (one and two look-back batches), 256 tiles of 4 keys per thread, and 16 keys per thread with a one-key last tile
    and a partial last wave"""
    case = SC.voxel_size_case(N)
    assert _live(case) == (SC.ALL_POS if N > 1 else [])
    _compare(dev, case)


@pytest.mark.parametrize("kind", SC.VOXEL_ORDERS)
def test_order_and_skew(dev, kind):
    """(c) input already sorted, reversed, and 99 % of the points in one voxel (one digit bin takes nearly every key of every tile)"""
    case = SC.voxel_order_case(kind)
    assert _live(case) == [0, 1, 3, 6]
    _, rn, _ = _compare(dev, case)
    if kind == "skewed":
        assert rn.max() > 19000


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_faces_of_a_non_dyadic_grid(dev, axis):
    """(d) points on and beside the faces of a 0.1 grid at origin -3.7: subtract, divide, floor in fp32, each rounded once"""
    case = SC.voxel_face_case(axis)
    k = SO.voxel_indices(case["xyz"], case["leaf"], case["origin"])
    assert int((k[:, axis] != SC.face_keys_fp64(case)).sum()) >= 300
    _compare(dev, case)


def test_labels_out_of_range_are_ignored(dev):
    """(e) labels outside [0, n_labels) do not vote; a voxel without a valid label reports 0"""
    case = SC.voxel_bad_label_case()
    lab = case["labels"]
    assert ((lab < 0) | (lab >= SC.N_LABELS)).sum() > 900
    _, _, rm = _compare(dev, case)
    assert (rm == 0).sum() >= 50


def test_without_labels_same_centroids_and_counts(dev):
    from pointcloudprocessing_amd import ops
    case = SC.voxel_live_case([0, 3, 6, 7])
    x = torch.from_numpy(case["xyz"]).to(dev)
    with_lab = ops.voxel_downsample(x, case["leaf"], case["origin"], torch.from_numpy(case["labels"]).to(dev), case["n_labels"])
    cent, cnt, maj = ops.voxel_downsample(x, case["leaf"], case["origin"])
    assert maj is None
    assert torch.equal(cent, with_lab[0]) and torch.equal(cnt, with_lab[1])
    rc, rn, _ = SO.voxel_downsample(case["xyz"], case["leaf"], case["origin"])
    assert np.array_equal(cent.cpu().numpy(), rc) and np.array_equal(cnt.cpu().numpy(), rn)


# ----------------------------------------------------------------------------------------------------------------- raw ABI
def _guarded(shape, dtype, dev):
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((GUARD + n + GUARD,), PAT, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + n].view(dtype).view(*shape)


def _intact(buf):
    return bool((buf[:GUARD] == PAT).all()) and bool((buf[-GUARD:] == PAT).all())


def _outputs(N, dev):
    return dict(cent=_guarded((N, 3), torch.float32, dev), cnt=_guarded((N,), torch.int32, dev), maj=_guarded((N,), torch.int32, dev),
                nout=_guarded((1,), torch.int32, dev))


def _call(x, lab, N, leaf, origin, n_labels, bufs, ws_ptr, ws_bytes):
    from pointcloudprocessing_amd import _lib
    p = lambda name: C.c_void_p(bufs[name][1].data_ptr())      # noqa: E731
    rc = _lib.lib().pn_voxel_downsample(_lib.ptr(x), _lib.ptr(lab), N, (C.c_float * 3)(*leaf), (C.c_float * 3)(*origin), n_labels,
                                        p("cent"), p("cnt"), p("maj"), p("nout"), C.c_void_p(ws_ptr), ws_bytes, _lib.current_stream())
    torch.cuda.synchronize()
    return rc


def test_raw_abi_dirty_workspace_guard_bands_and_untouched_rows(dev):
    """(f) one workspace, filled with 0xFF, serves N = 9217 and then N = 1025 (a different layout over the first call's
    leftovers); outputs pre-filled with a byte pattern keep it in rows [V, N) and in the bands around them"""
    from pointcloudprocessing_amd import _lib
    need = _lib.lib().pn_voxel_workspace_bytes(9217)
    assert need >= _lib.lib().pn_voxel_workspace_bytes(1025)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    pat32 = int(np.frombuffer(bytes([PAT] * 4), np.int32)[0])
    for N in (9217, 1025):
        case = SC.voxel_size_case(N)
        x, lab = torch.from_numpy(case["xyz"]).to(dev), torch.from_numpy(case["labels"]).to(dev)
        keep = x.clone(), lab.clone()
        bufs = _outputs(N, dev)
        rc = _call(x, lab, N, case["leaf"], case["origin"], case["n_labels"], bufs, ws.data_ptr(), need)
        _lib.check(rc, "pn_voxel_downsample")
        assert int(ws[:4].view(torch.int32).item()) == 0
        for name, (buf, _) in bufs.items():
            assert _intact(buf), f"{name}: guard band overwritten"
        assert torch.equal(keep[0], x) and torch.equal(keep[1], lab), "an input was modified"
        rcent, rcnt, rmaj = SO.voxel_downsample(case["xyz"], case["leaf"], case["origin"], case["labels"], case["n_labels"])
        V = int(bufs["nout"][1].item())
        assert V == len(rcnt) and V < N
        for name, ref in (("cent", rcent), ("cnt", rcnt), ("maj", rmaj)):
            got = bufs[name][1].cpu().numpy()
            assert np.array_equal(got[:V], ref), name
            assert (got[V:].view(np.int32) == pat32).all(), f"{name}: rows [V, N) were written"


def test_refused_keys_raise_and_leave_the_device_usable(dev):
    """(g) a point below the origin, a key of exactly 2^21, a NaN and a +Inf coordinate: the kernel clamps the key (nothing faults),
    raises the flag, ops raises; the next valid call equals the oracle"""
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd._lib import PointNetHipError
    for kind in SC.VOXEL_REFUSALS:
        case = SC.voxel_refusal_case(kind)
        k = SO.voxel_indices(case["xyz"], case["leaf"], case["origin"])
        assert np.flatnonzero(((k < 0) | (k >= SC.KEY_LIMIT)).any(1)).tolist() == [case["bad"]]
        with pytest.raises(PointNetHipError, match="outside"):
            ops.voxel_downsample(torch.from_numpy(case["xyz"]).to(dev), case["leaf"], case["origin"],
                                 torch.from_numpy(case["labels"]).to(dev), case["n_labels"])
        _compare(dev, SC.voxel_live_case([0, 1]))


def test_invalid_arguments_are_refused_before_any_launch(dev):
    """(g) N = 0, a zero leaf, n_labels = 33, a workspace one byte short or misaligned: the invalid-argument status, and neither
    the outputs nor the workspace are written"""
    from pointcloudprocessing_amd import _lib
    N = 1025
    case = SC.voxel_size_case(N)
    x, lab = torch.from_numpy(case["xyz"]).to(dev), torch.from_numpy(case["labels"]).to(dev)
    need = _lib.lib().pn_voxel_workspace_bytes(N)
    assert _lib.lib().pn_voxel_workspace_bytes(0) == 0
    ws = torch.full((need + 16,), PAT, dtype=torch.uint8, device=dev)
    good = dict(N=N, leaf=case["leaf"], n_labels=32, ws_ptr=ws.data_ptr(), ws_bytes=need)
    assert ws.data_ptr() % 16 == 0
    refusals = [dict(N=0), dict(leaf=(1.0, 0.0, 1.0)), dict(n_labels=33), dict(ws_bytes=need - 1),
                dict(ws_ptr=ws.data_ptr() + 4, ws_bytes=need + 12)]
    for change in refusals:
        a = dict(good, **change)
        bufs = _outputs(N, dev)
        rc = _call(x, lab, a["N"], a["leaf"], case["origin"], a["n_labels"], bufs, a["ws_ptr"], a["ws_bytes"])
        assert rc == PN_ERR_INVALID_ARGUMENT, change
        assert _lib.lib().pn_last_error().startswith(b"pn_voxel_downsample:"), change
        assert bool((ws == PAT).all()), change
        for name, (buf, _) in bufs.items():
            assert bool((buf == PAT).all()), (change, name)
    bufs = _outputs(N, dev)
    _lib.check(_call(x, lab, N, case["leaf"], case["origin"], 32, bufs, good["ws_ptr"], need), "pn_voxel_downsample")
    rcent, rcnt, rmaj = SO.voxel_downsample(case["xyz"], case["leaf"], case["origin"], case["labels"], 32)
    V = int(bufs["nout"][1].item())
    assert V == len(rcnt)
    assert np.array_equal(bufs["cent"][1].cpu().numpy()[:V], rcent) and np.array_equal(bufs["cnt"][1].cpu().numpy()[:V], rcnt)
    assert np.array_equal(bufs["maj"][1].cpu().numpy()[:V], rmaj)
