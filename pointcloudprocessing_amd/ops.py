"""Thin torch-tensor wrappers over the op-level C ABI (include/pointnet_hip.h).

Every function takes contiguous fp32 HIP tensors, allocates its outputs with torch (device memory plumbing
only) and enqueues the HIP kernels on torch's current stream.  Nothing here computes on the CPU.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _lib
from ._lib import check, current_stream, lib, operand, ptr, require_gpu_tensor

F32 = torch.float32


def _tiles(B, N):
    return B * ((N + 127) // 128)


def normalize(xyz: torch.Tensor):
    """PointCloudNormalization.call (reference pointnet/PointNet.py:691-706) -> (normalized, (centroid, scale))."""
    require_gpu_tensor(xyz, "xyz", F32)
    B, N, _ = xyz.shape
    out = torch.empty_like(xyz)
    cen = torch.empty(B, 1, 3, device=xyz.device, dtype=F32)
    scl = torch.empty(B, 1, 1, device=xyz.device, dtype=F32)
    check(lib().pn_normalize(ptr(xyz), B, N, ptr(out), ptr(cen), ptr(scl), current_stream()), "pn_normalize")
    return out, (cen, scl)


def conv3_fwd(x3, w, B, N, per_cloud=False, want_stats=True):
    C_ = w.shape[-1]
    z = torch.empty(B * N, C_, device=x3.device, dtype=F32)
    part = torch.empty(_tiles(B, N), 2, C_, device=x3.device, dtype=F32) if want_stats else None
    check(lib().pn_conv3_fwd(ptr(x3), ptr(w), 3 * C_ if per_cloud else 0, B, N, C_, ptr(z), ptr(part), current_stream()),
          "pn_conv3_fwd")
    return z, part


def conv3_wgrad(x3, dz_op, B, N, C_):
    slabs = torch.empty(_tiles(B, N), 3, C_, device=x3.device, dtype=F32)
    check(lib().pn_conv3_wgrad(ptr(x3), C.byref(dz_op), B, N, C_, ptr(slabs), current_stream()), "pn_conv3_wgrad")
    return slabs


def conv_fwd(x_op, w, B, N, K, C_, prec, w_cloud_stride=0, cloud_bias=None, store=True, want_stats=True):
    """prec | _lib.PN_STORE_BF16: z comes back as a bf16 tensor"""
    dev = w.device
    z = torch.empty(B * N, C_, device=dev, dtype=torch.bfloat16 if prec & _lib.PN_STORE_BF16 else F32) if store else None
    part = torch.empty(_tiles(B, N), 2, C_, device=dev, dtype=F32) if want_stats else None
    check(lib().pn_conv_fwd(C.byref(x_op), ptr(w), w_cloud_stride, B, N, K, C_, ptr(cloud_bias), ptr(z), ptr(part), prec,
                            current_stream()), "pn_conv_fwd")
    return z, part


def conv_fwd_max(x_op, w, B, N, K, C_, sgn, prec):
    dev = w.device
    T = _tiles(B, N)
    pmax = torch.empty(T, C_, device=dev, dtype=F32)
    pidx = torch.empty(T, C_, device=dev, dtype=torch.int32)
    part = torch.empty(T, 2, C_, device=dev, dtype=F32)
    check(lib().pn_conv_fwd_max(C.byref(x_op), ptr(w), B, N, K, C_, ptr(sgn), ptr(pmax), ptr(pidx), ptr(part), prec,
                                current_stream()), "pn_conv_fwd_max")
    return pmax, pidx, part


def weights_prep(w, sgn=None):
    """fragment-ordered bf16 copies (hi, lo) of a Keras kernel (K, C), columns pre-multiplied by sign(sgn) (include/pointnet_hip.h)"""
    K, C_ = w.shape
    hi = torch.empty(C_ * K, device=w.device, dtype=torch.bfloat16)
    lo = torch.empty(C_ * K, device=w.device, dtype=torch.bfloat16)
    check(lib().pn_weights_prep(ptr(w), ptr(sgn), K, C_, ptr(hi), ptr(lo), current_stream()), "pn_weights_prep")
    return hi, lo


def conv_fwd_max_panel(x_op, wf, B, N, K, C_, prec, want_stats=True):
    """the row-panel kernel: per slot (run of 64-row panels) and channel max of sgn*z, the 32-row block holding it and (want_stats)
    sum z^2, and per cloud the column sums of the staged operand rows in 2^-24 fixed point (panel_finalize turns those into the channel sums of z).
    wf = weights_prep(w, gamma)."""
    dev = wf[0].device
    T = B * lib().pn_panel_slots_per_cloud(B, N)
    pmax = torch.empty(T, C_, device=dev, dtype=F32)
    pblk = torch.empty(T, C_, device=dev, dtype=torch.int32)
    sumsq = torch.empty(T, C_, device=dev, dtype=F32) if want_stats else None
    colsum = torch.zeros(B, (2 if (prec & 3) == 3 else 1) * K, device=dev, dtype=torch.int64) if want_stats else None      # accumulators: zero on entry
    check(lib().pn_conv_fwd_max_panel(C.byref(x_op), ptr(wf[0]), ptr(wf[1]), B, N, K, C_, ptr(pmax), ptr(pblk), ptr(sumsq), ptr(colsum), prec,
                                      current_stream()), "pn_conv_fwd_max_panel")
    return pmax, pblk, sumsq, colsum


def weights_copy16(w):
    """bf16 copies of a Keras kernel (K, C): (as it is (K, C), transposed (C, K)) -- what the model plan's row GEMMs stage"""
    K, C_ = w.shape
    nat = torch.empty(K, C_, device=w.device, dtype=torch.bfloat16)
    tr = torch.empty(C_, K, device=w.device, dtype=torch.bfloat16)
    check(lib().pn_weights_copy16(ptr(w), K, C_, ptr(nat), ptr(tr), current_stream()), "pn_weights_copy16")
    return nat, tr


def chain_fwd_max(x_op, xyz, w1, w1t, sc1, sh1, w2t, sc2, sh2, wf_hi, B, N):
    """inference: ConvLayer(3 | 64 -> 64) -> ConvLayer(64 -> 128) -> ConvLayer(128 -> 1024) -> reduce_max in one launch (moving
    statistics); exactly one of x_op (64-channel bf16 lazy operand, with w1t) and xyz ((B*N, 3), with w1).  Returns (pmax, pblock) per
    slot, as conv_fwd_max_panel leaves them."""
    dev = wf_hi.device
    T = B * lib().pn_panel_slots_per_cloud(B, N)
    pmax = torch.empty(T, 1024, device=dev, dtype=F32)
    pblk = torch.empty(T, 1024, device=dev, dtype=torch.int32)
    check(lib().pn_chain_fwd_max(C.byref(x_op) if x_op is not None else None, ptr(xyz), ptr(w1), ptr(w1t), ptr(sc1), ptr(sh1), ptr(w2t),
                                 ptr(sc2), ptr(sh2), ptr(wf_hi), B, N, ptr(pmax), ptr(pblk), current_stream()), "pn_chain_fwd_max")
    return pmax, pblk


def panel_finalize(pmax, pblk, sumsq, colsum, wf, prec, B, N, K, gamma, beta, moving_mean, moving_var, training=True, momentum=0.99, eps=1e-3):
    """BN coefficients of the layer + reduce_max over each cloud's tiles -> (mean, invstd, scale, shift, g, zstar, arg_block);
    wf, prec, K: what the panel launch was given"""
    C_ = pmax.shape[1]
    dev = pmax.device
    mean, invstd, scale, shift = (torch.empty(C_, device=dev, dtype=F32) for _ in range(4))
    g = torch.empty(B, C_, device=dev, dtype=F32)
    zstar = torch.empty(B, C_, device=dev, dtype=F32)
    argb = torch.empty(B, C_, device=dev, dtype=torch.int32)
    check(lib().pn_panel_finalize(ptr(pmax), ptr(pblk), ptr(sumsq), ptr(colsum), ptr(wf[0]), ptr(wf[1]), prec, B, N, K, C_,
                                  ptr(gamma), ptr(beta), ptr(moving_mean), ptr(moving_var), momentum, eps, int(training), int(training),
                                  ptr(mean), ptr(invstd), ptr(scale), ptr(shift), ptr(g), ptr(zstar), ptr(argb), current_stream()),
          "pn_panel_finalize")
    return mean, invstd, scale, shift, g, zstar, argb


def max_resolve(x_op, wf, argb, B, N, K, C_, prec):
    """the row of each (cloud, channel) maximum inside its 32-row block"""
    arg = torch.empty(B, C_, device=argb.device, dtype=torch.int32)
    check(lib().pn_max_resolve(C.byref(x_op), ptr(wf[0]), ptr(wf[1]), ptr(argb), B, N, K, C_, ptr(arg), prec, current_stream()),
          "pn_max_resolve")
    return arg


def maxbwd_scatter(arg, hs, wt, q, B, N, K, C_, store16=False):
    """D[b][n][:] = q + sum over the channels whose maximum sits at row n of hs[b][c] * wt[c][:]   (fp32, or bf16 with store16)"""
    D = torch.empty(B * N, K, device=hs.device, dtype=torch.bfloat16 if store16 else torch.float32)
    check(lib().pn_maxbwd_scatter(ptr(arg), ptr(hs), ptr(wt), ptr(q), B, N, K, C_, ptr(D), int(store16), current_stream()), "pn_maxbwd_scatter")
    return D


def conv_bwd_data(dz_op, w, B, N, K, C_, prec, w_cloud_stride=0, addend=None, zmask=None, msc=None, msh=None,
                  want_stats=True):
    """prec | _lib.PN_STORE_BF16: out comes back as a bf16 tensor and addend / zmask must be bf16 tensors"""
    dev = w.device
    s16 = bool(prec & _lib.PN_STORE_BF16)
    for t, name in ((addend, "addend"), (zmask, "zmask")):
        if t is not None and t.dtype != (torch.bfloat16 if s16 else F32):
            raise _lib.PointNetHipError(f"conv_bwd_data: {name} must be {'bf16' if s16 else 'fp32'} for this prec")
    out = torch.empty(B * N, C_, device=dev, dtype=torch.bfloat16 if s16 else F32)
    part = torch.empty(_tiles(B, N), 2, C_, device=dev, dtype=F32) if want_stats else None
    check(lib().pn_conv_bwd_data(C.byref(dz_op), ptr(w), w_cloud_stride, B, N, K, C_, ptr(addend), ptr(zmask), ptr(msc),
                                 ptr(msh), ptr(out), ptr(part), prec, current_stream()), "pn_conv_bwd_data")
    return out, part


def conv_bwd_data_wgrad(dz_op, w, a_op, B, N, K, C_, prec, slab_rows=128, w_cloud_stride=0, addend=None, zmask=None, msc=None, msh=None,
                        want_stats=True, fill=None):
    """conv_bwd_data whose row tiles also write the slabs of the layer's weight gradient a^T dz (pn_conv_bwd_data_wgrad):
    returns (out, part, slabs) with slabs (B * ceil(N / slab_rows), C_, K) fp32, the bytes conv_wgrad's launch writes.
    fill: a value the three results hold before the launch (tests: NaN, so that nothing unwritten can pass for written)"""
    dev = w.device
    new = torch.empty if fill is None else (lambda *s, **k: torch.full(s, fill, **k))
    out = new(B * N, C_, device=dev, dtype=torch.bfloat16)
    part = new(_tiles(B, N), 2, C_, device=dev, dtype=F32) if want_stats else None
    slabs = new(B * ((N + slab_rows - 1) // slab_rows), C_, K, device=dev, dtype=F32)
    check(lib().pn_conv_bwd_data_wgrad(C.byref(dz_op), ptr(w), w_cloud_stride, B, N, K, C_, ptr(addend), ptr(zmask), ptr(msc), ptr(msh),
                                       ptr(out), ptr(part), C.byref(a_op), C_, slab_rows, ptr(slabs), prec,
                                       current_stream()), "pn_conv_bwd_data_wgrad")
    return out, part, slabs


def conv_wgrad(a_op, b_op, B, N, Ci, Cj, prec, slab_rows=256, per_cloud=False):
    dev = torch.device("cuda")
    spc = (N + slab_rows - 1) // slab_rows
    slabs = torch.empty(B * spc, Ci, Cj, device=dev, dtype=F32)
    check(lib().pn_conv_wgrad(C.byref(a_op), C.byref(b_op), B, N, Ci, Cj, slab_rows, ptr(slabs), prec, current_stream()),
          "pn_conv_wgrad")
    groups = B if per_cloud else 1
    out = torch.empty(groups, Ci, Cj, device=dev, dtype=F32)
    check(lib().pn_slab_reduce(ptr(slabs), B * spc, spc if per_cloud else B * spc, Ci * Cj, ptr(out), current_stream()),
          "pn_slab_reduce")
    return out if per_cloud else out[0]


def slab_reduce(slabs, per_group):
    n = slabs.shape[0]
    elems = slabs[0].numel()
    out = torch.empty(n // per_group, *slabs.shape[1:], device=slabs.device, dtype=F32)
    check(lib().pn_slab_reduce(ptr(slabs), n, per_group, elems, ptr(out), current_stream()), "pn_slab_reduce")
    return out


def bn_finalize(part, count, gamma, beta, moving_mean, moving_var, use_batch_stats=True, update_moving=True,
                momentum=0.99, eps=1e-3):
    C_ = gamma.numel()
    dev = gamma.device
    mean, invstd, scale, shift = (torch.empty(C_, device=dev, dtype=F32) for _ in range(4))
    nt = part.shape[0] if part is not None else 0
    check(lib().pn_bn_finalize(ptr(part), nt, C_, count, ptr(gamma), ptr(beta), ptr(moving_mean), ptr(moving_var), momentum,
                               eps, int(use_batch_stats), int(update_moving), ptr(mean), ptr(invstd), ptr(scale), ptr(shift),
                               current_stream()), "pn_bn_finalize")
    return mean, invstd, scale, shift


def bn_bwd_finalize(part, count, gamma, mean, invstd, batch_stats=True):
    C_ = gamma.numel()
    dev = gamma.device
    dgamma, dbeta, ca, cb, cc = (torch.zeros(C_, device=dev, dtype=F32) for _ in range(5))
    nt = part.shape[0] if part is not None else 0
    check(lib().pn_bn_bwd_finalize(ptr(part), nt, C_, count, ptr(gamma), ptr(mean), ptr(invstd), int(batch_stats), ptr(dgamma),
                                   ptr(dbeta), ptr(ca), ptr(cb), ptr(cc), current_stream()), "pn_bn_bwd_finalize")
    return dgamma, dbeta, ca, cb, cc


def sign(gamma):
    s = torch.empty_like(gamma)
    check(lib().pn_sign(ptr(gamma), gamma.numel(), ptr(s), current_stream()), "pn_sign")
    return s


def max_finalize(pmax, pidx, B, sgn, scale, shift):
    T, C_ = pmax.shape
    dev = pmax.device
    g = torch.empty(B, C_, device=dev, dtype=F32)
    zstar = torch.empty(B, C_, device=dev, dtype=F32)
    arg = torch.empty(B, C_, device=dev, dtype=torch.int32)
    check(lib().pn_max_finalize(ptr(pmax), ptr(pidx), B, T // B, C_, ptr(sgn), ptr(scale), ptr(shift), ptr(g), ptr(zstar),
                                ptr(arg), current_stream()), "pn_max_finalize")
    return g, zstar, arg


def argmax_rows(values: torch.Tensor) -> torch.Tensor:
    """index of the first maximum along the last axis (np.argmax order), int32; any leading shape"""
    require_gpu_tensor(values, "values", F32)
    v = values.contiguous()
    C_ = v.shape[-1]
    out = torch.empty(v.shape[:-1], dtype=torch.int32, device=v.device)
    check(lib().pn_argmax_rows(ptr(v), v.numel() // C_, C_, ptr(out), current_stream()), "pn_argmax_rows")
    return out


def farthest_point_sample(xyz: torch.Tensor, m: int, start_idx: int = 0, return_mindist: bool = False):
    """xyz (B,N,3) -> idx (B,m) int32 in selection order (spec: include/pointnet_hip.h, pn_fps)."""
    require_gpu_tensor(xyz, "xyz", F32)
    B, N, _ = xyz.shape
    idx = torch.empty(B, m, device=xyz.device, dtype=torch.int32)
    md = torch.empty(B, N, device=xyz.device, dtype=F32)
    nbytes = lib().pn_fps_workspace_bytes(B, N)
    ws = torch.empty(nbytes, device=xyz.device, dtype=torch.uint8)
    check(lib().pn_fps(ptr(xyz), B, N, m, start_idx, ptr(idx), ptr(md), ptr(ws), nbytes, current_stream()), "pn_fps")
    if int(ws[:4].view(torch.int32).item()) != 0:
        raise _lib.PointNetHipError("pn_fps: a block timed out waiting for a peer block")
    return (idx, md) if return_mindist else idx


_KEY_LIMIT = "a grid key fell outside [0, {{max_key}}): the {} extends more than {{max_key}} leaves ({{leaf:g}} each) from the origin, or lies below it"
_GRID_ERRORS = {
    1: "a voxel key fell outside [0, 2^21)",
    **{(entry, 1): _KEY_LIMIT.format("cloud") for entry in ("pn_scan_normals", "pn_radius_knn", "pn_dbscan")},
    ("pn_dbscan", 3): "a union-find loop exhausted its bound (N + 1 rounds)",
    ("pn_icp_grid_build", 1): _KEY_LIMIT.format("reference"),
    **{(entry, 4): "the mesh does not fit the capacities it was given, or has more than 2^31 - 1 faces" for entry in ("pn_recon_count", "pn_recon_emit")},
    **{(entry, 5): "a face index is outside [0, {V})" for entry in ("pn_mesh_components", "pn_mesh_simplify")},
    ("pn_mesh_simplify", 6): "a face refers to a vertex with a non-finite coordinate",
    ("pn_mesh_simplify", 7): "the grid has more than 2^21 occupied cells: increase leaf",
    ("pn_mesh_components", 8): "more components than the capacity of sizes",
    2: "a tile's look-back timed out waiting for an earlier tile",
    3: "a union-find loop exhausted its bound",
}


def _f3(v):
    return (C.c_float * 3)(*[float(a) for a in v])


def _leaf3(leaf, what):
    """a scalar leaf or three -> three floats"""
    leaf3 = [float(v) for v in (leaf if hasattr(leaf, "__len__") else (leaf,) * 3)]
    if len(leaf3) != 3:
        raise _lib.PointNetHipError(f"{what}: leaf must be a scalar or three values, got {leaf!r}")
    return leaf3


def _grid_call(entry, sizer, n, dev, *head, size_args=(), floor=None, errors=None, **fmt):
    """One entry on the voxel grid: the workspace (``sizer``(n, *size_args) bytes, and no less than the sizer ``floor`` gives for
    n), the checked call ``entry(*head, ws, bytes, stream)`` and the error word, one host read, raised through _GRID_ERRORS (the
    text of the entry ``errors``, default ``entry`` itself, first; ``fmt`` fills its fields)."""
    nbytes = max(getattr(lib(), sizer)(n, *size_args), getattr(lib(), floor)(n) if floor else 0)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    check(getattr(lib(), entry)(*head, ptr(ws), nbytes, current_stream()), entry)
    flag = int(ws[:4].view(torch.int32).item())
    if flag != 0:
        text = _GRID_ERRORS.get((errors or entry, flag)) or _GRID_ERRORS.get(flag, _GRID_ERRORS[1])
        raise _lib.PointNetHipError(f"{entry}: " + text.format(**fmt))


def _radius_grid(radius):
    """what fills the key-limit text of an entry on pn_radius_knn's grid"""
    return dict(max_key=_lib.PN_RADIUS_KNN_MAX_KEY, leaf=lib().pn_radius_knn_leaf(float(radius)))


def _finite_rows(xyz):
    """the rows (ascending) of a scan (N, 3) without a non-finite coordinate: the no-return pixels of a sensor are NaN"""
    return torch.isfinite(xyz).all(1).nonzero().squeeze(1)


def _compact(xyz, rows, origin, *full):
    """-> (the points of ``rows``, the origin (default: their per-axis minimum), what the entry writes for every full-length output in
    ``full``: the output itself when ``rows`` is every row, else a tensor of the compacted length to scatter back)"""
    whole = rows.numel() == xyz.shape[0]
    pts = xyz if whole else xyz[rows].contiguous()
    if origin is None:
        origin = pts.min(0).values.cpu().tolist()
    return pts, origin, full if whole else tuple(torch.empty((rows.numel(),) + tuple(t.shape[1:]), device=t.device, dtype=t.dtype) for t in full)


def _scan_call(what, xyz, origin, outs, entry, sizer, head, **grid):
    """The one call path of the entries over a raw scan (ops.voxel_clusters, dbscan, radius_knn, estimate_normals, fpfh).  ``xyz`` must
    be (N, 3) fp32 on the device; its rows without a non-finite coordinate (the no-return pixels of a sensor are NaN) are compacted,
    ``entry`` runs on them through _grid_call (``sizer`` and ``grid``: its arguments) and what it wrote is scattered back.  ``outs``
    describes the full-length outputs: (shape tail, dtype, fill, remap) each, or None for one the caller did not ask for.  A masked
    row keeps ``fill``; ``remap`` marks a column of row indices, taken from the compacted rows back to the rows of ``xyz``.
    ``head(pts, n, origin3, part, rows)`` -> the entry's arguments in front of the workspace: the n compacted points, the origin
    (default: their per-axis minimum) and, per output, the tensor the entry writes (the output itself when no row is masked; None
    where ``outs`` is).  -> (the outputs, n); with n = 0 nothing is called."""
    require_gpu_tensor(xyz, "xyz", F32)
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise _lib.PointNetHipError(f"{what} expects (N, 3) points, got {tuple(xyz.shape)}")
    N, dev = xyz.shape[0], xyz.device
    rows = torch.isfinite(xyz).all(1).nonzero().squeeze(1)
    n = rows.numel()
    full = [o and torch.full((N,) + tuple(o[0]), o[2], device=dev, dtype=o[1]) for o in outs]
    if n:
        pts = xyz if n == N else xyz[rows].contiguous()
        if origin is None:
            origin = pts.min(0).values.cpu().tolist()
        part = [t if n == N or t is None else torch.empty((n,) + tuple(t.shape[1:]), device=dev, dtype=t.dtype) for t in full]
        _grid_call(entry, sizer, n, dev, *head(pts, n, _f3(origin), part, rows), **grid)
        for o, f, p in zip(outs, full, part):
            if p is not f:
                f[rows] = torch.where(p >= 0, rows.to(torch.int32)[p.long().clamp(min=0)], p) if o[3] else p
    return full, n


def _label_call(what, xyz, origin, outs, entry, sizer, lead, **grid):
    """_scan_call for the two labellers, whose entries end in (cluster, a second per-point output or NULL, sizes, n_out):
    ``lead(pts, n, origin3)`` -> the arguments in front of those.  -> (the outputs, sizes (K,)); K is one host read, and with no
    finite row sizes is empty."""
    tables = []

    def head(pts, n, org, part, rows):
        tables[:] = torch.empty(n, device=pts.device, dtype=torch.int32), torch.zeros(2, device=pts.device, dtype=torch.int32)
        return (*lead(pts, n, org), ptr(part[0]), ptr(part[1]), ptr(tables[0]), ptr(tables[1]))

    full, n = _scan_call(what, xyz, origin, outs, entry, sizer, head, **grid)
    return full, tables[0][:int(tables[1][1].item())] if n else torch.empty(0, device=xyz.device, dtype=torch.int32)


def voxel_downsample(xyz: torch.Tensor, leaf, origin, labels: Optional[torch.Tensor] = None, n_labels: int = 0):
    """xyz (N,3) -> (centroids (V,3), counts (V,), majority (V,) or None) ordered by ascending (kz,ky,kx)."""
    require_gpu_tensor(xyz, "xyz", F32)
    N = xyz.shape[0]
    dev = xyz.device
    cent = torch.empty(N, 3, device=dev, dtype=F32)
    cnt = torch.empty(N, device=dev, dtype=torch.int32)
    maj = torch.empty(N, device=dev, dtype=torch.int32)
    nout = torch.zeros(1, device=dev, dtype=torch.int32)
    if labels is not None:
        require_gpu_tensor(labels, "labels", torch.int32)
    _grid_call("pn_voxel_downsample", "pn_voxel_workspace_bytes", N, dev, ptr(xyz), ptr(labels), N, _f3(leaf), _f3(origin), n_labels, ptr(cent),
               ptr(cnt), ptr(maj), ptr(nout))
    v = int(nout.item())
    return cent[:v], cnt[:v], (maj[:v] if labels is not None else None)


def voxel_clusters(xyz: torch.Tensor, leaf, origin=None, connectivity: int = 26, return_voxels: bool = False):
    """Voxel connected components (spec: include/pointnet_hip.h, pn_voxel_cluster): xyz (N, 3) fp32 on the device, ``leaf`` a scalar or
    a 3-tuple, ``origin`` default the per-axis minimum over the finite points -> (cluster (N,) int32, sizes (K,) int32): the cluster
    id of every point (ids in ascending order of the clusters' lowest voxel rank) and the number of points in every cluster; with
    ``return_voxels`` a third value follows, voxel (N,) int32, the rank of every point's voxel.  A row with a non-finite coordinate
    (the no-return pixels of a sensor are NaN) is masked out before the call and comes back as cluster -1 (voxel -1).  Host
    reads: the number of finite rows, the minimum when ``origin`` is None, K and the error word."""
    leaf3 = _leaf3(leaf, "voxel_clusters")
    ids = ((), torch.int32, -1, False)
    (cluster, voxel), sizes = _label_call("voxel_clusters", xyz, origin, [ids, ids if return_voxels else None], "pn_voxel_cluster",
                                          "pn_voxel_cluster_workspace_bytes",
                                          lambda pts, n, org: (ptr(pts), n, _f3(leaf3), org, int(connectivity)))
    return (cluster, sizes, voxel) if return_voxels else (cluster, sizes)


def dbscan(xyz: torch.Tensor, eps: float, min_points: int, origin=None, return_core: bool = False):
    """Exact DBSCAN on the voxel grid (spec: include/pointnet_hip.h, pn_dbscan): xyz (N, 3) fp32 on the device -> (cluster (N,) int32,
    sizes (K,) int32), with ``return_core`` a third value, core (N,) bool.  A point is core when it has at least ``min_points`` points
    within ``eps`` (d <= eps^2 in fp32, ops.radius_knn's neighbours; the point counts itself); clusters are the connected components
    of the core points, ids in ascending order of each cluster's lowest core row; a point that is not core joins the cluster of its
    nearest core neighbour (ties -> the lowest row) or is noise, cluster -1.  sizes counts core and border points.  The result is a
    pure function of (xyz, eps, min_points); ops.cluster_mask takes it unchanged.  A row with a non-finite coordinate is masked out
    before the call: it comes back as cluster -1, not core, and is nobody's neighbour.  ``origin`` and the key limit: as in
    ops.radius_knn.  Host reads: the number of finite rows, the minimum when ``origin`` is None, K and the error word."""
    outs = [((), torch.int32, -1, False), ((), torch.uint8, 0, False) if return_core else None]
    (cluster, core), sizes = _label_call("dbscan", xyz, origin, outs, "pn_dbscan", "pn_dbscan_workspace_bytes",
                                         lambda pts, n, org: (ptr(pts), n, float(eps), int(min_points), org), **_radius_grid(eps))
    return (cluster, sizes, core.bool()) if return_core else (cluster, sizes)


def cluster_mask(cluster: torch.Tensor, sizes: torch.Tensor, keep: str = "largest", min_points: int = 1) -> torch.Tensor:
    """bool (N,): the points of ops.voxel_clusters' or ops.dbscan's result to keep.  ``keep="largest"``: the cluster with the most points
    (ties -> lowest id), provided it has at least ``min_points``; ``keep="all"``: every cluster with at least ``min_points`` points.
    A point with cluster -1 is never kept.  torch indexing only: it runs wherever its inputs live."""
    if keep not in ("largest", "all"):
        raise _lib.PointNetHipError(f"cluster_mask: keep must be 'largest' or 'all', got {keep!r}")
    if sizes.numel() == 0:
        return torch.zeros_like(cluster, dtype=torch.bool)
    ok = sizes >= int(min_points)
    if keep == "largest":
        ids = torch.arange(sizes.numel(), device=sizes.device)
        first_max = torch.where(sizes == sizes.max(), ids, ids.numel()).min()         # the lowest id among the maxima
        ok = ok & (ids == first_max)
    return (cluster >= 0) & ok[cluster.long().clamp(min=0)]


def radius_knn(xyz: torch.Tensor, radius: float, k: int, origin=None):
    """Exact fixed-radius k-nearest-neighbour search inside one cloud (spec: include/pointnet_hip.h, pn_radius_knn): xyz (N, 3) fp32 on
    the device -> (idx (N, k) int32, d2 (N, k) fp32, count (N,) int32).  count is the number of OTHER points within ``radius``
    (d <= radius^2 in fp32; not capped by k); idx / d2 hold the k nearest of them by ascending (d, row), unfilled slots (-1, +inf);
    ``k = 0`` only counts.  idx refers to the rows of ``xyz`` as passed in.  A row with a non-finite coordinate is masked out before
    the call: it comes back with count 0 and empty slots and is nobody's neighbour.  ``origin`` (default: the per-axis minimum of the
    finite rows) only places the internal grid, whose keys must stay below 2^14 per axis: the cloud may extend about 16,384 radii
    from it.  Host reads: the number of finite rows, the minimum when ``origin`` is None, and the error word."""
    k = int(k)
    kk = max(k, 0)                        # (a k outside [0, 16] is refused by the library)
    outs = [((kk,), torch.int32, -1, True), ((kk,), F32, float("inf"), False), ((), torch.int32, 0, False)]
    (idx, d2, count), _ = _scan_call("radius_knn", xyz, origin, outs, "pn_radius_knn", "pn_radius_knn_workspace_bytes",
                                     lambda pts, n, org, part, rows: (ptr(pts), n, float(radius), org, k, ptr(part[0]) if kk else None,
                                                                      ptr(part[1]) if kk else None, ptr(part[2])), **_radius_grid(radius))
    return idx, d2, count


def neighbor_stat_mask(d2: torch.Tensor, count: torch.Tensor, k: int, std_ratio: float) -> torch.Tensor:
    """bool (N,): statistical outlier removal on ops.radius_knn's output.  A point is FULL when count >= k; m_i is the mean over its k
    slots of sqrt(d2) in fp64; mu and the population sigma of m are taken over the full points; keep iff full and
    m_i <= mu + std_ratio * sigma.  With no full point nothing is kept.  torch only: it runs wherever its inputs live."""
    k = int(k)
    if d2.dim() != 2 or count.dim() != 1 or d2.shape[0] != count.shape[0] or not 1 <= k <= d2.shape[1]:
        raise _lib.PointNetHipError(f"neighbor_stat_mask: d2 (N, >=k), count (N,) and k >= 1 expected, got {tuple(d2.shape)}, "
                                    f"{tuple(count.shape)}, k={k}")
    full = count >= k
    m = d2[:, :k].to(torch.float64).sqrt().mean(1)
    w = full.to(torch.float64)
    nf = w.sum()
    mz = torch.where(full, m, torch.zeros_like(m))                      # (a partly filled row's mean is +inf: keep it out of the sums)
    mu = mz.sum() / nf
    sigma = (torch.where(full, (m - mu) ** 2, torch.zeros_like(m)).sum() / nf).sqrt()
    return full & (m <= mu + float(std_ratio) * sigma)                  # no full point: mu is NaN and full is all False


def estimate_normals(xyz: torch.Tensor, radius: float, k: int = 8, viewpoint=None, origin=None, return_neighbors: bool = False):
    """Per-point surface normals of a raw scan on the device (spec: include/pointnet_hip.h, pn_scan_normals): xyz (N, 3) fp32 ->
    (normals (N, 3) fp32, curvature (N,) fp32, count (N,) int32), with ``return_neighbors`` a fourth value, idx (N, k) int32.  The
    neighbourhood of a point is itself and its ``k`` nearest others within ``radius`` (ops.radius_knn's, in its order; 2 <= k <= 16);
    the normal is the least eigenvector of their fp64 covariance, curvature = l0 / (l0 + l1 + l2); a point with fewer than two
    neighbours, or whose neighbourhood is collinear or coincident, gets NaN.  count is ops.radius_knn's (not capped by k) and idx its
    slots (-1 padded), rows of ``xyz`` as passed in.  ``viewpoint`` (three floats) turns every normal towards it; without one the
    component of largest magnitude is positive.  A row with a non-finite coordinate is masked out before the call: NaN normal,
    count 0, nobody's neighbour.  ``origin`` and the host reads: as in ops.radius_knn."""
    k = int(k)
    kk = max(k, 0)                        # (a k outside [2, 16] is refused by the library)
    if viewpoint is not None and len(viewpoint) != 3:
        raise _lib.PointNetHipError(f"estimate_normals: viewpoint must be three values, got {viewpoint!r}")
    outs = [((3,), F32, float("nan"), False), ((), F32, float("nan"), False), ((), torch.int32, 0, False),
            ((kk,), torch.int32, -1, True) if return_neighbors else None]
    full, _ = _scan_call("estimate_normals", xyz, origin, outs, "pn_scan_normals", "pn_scan_normals_workspace_bytes",
                         lambda pts, n, org, part, rows: (ptr(pts), n, float(radius), org, k, None if viewpoint is None else _f3(viewpoint),
                                                          *map(ptr, part)), **_radius_grid(radius))
    return tuple(full) if return_neighbors else tuple(full[:3])


def fpfh(xyz: torch.Tensor, normals: torch.Tensor, radius: float, k: int = 16, origin=None, return_spfh: bool = False):
    """FPFH descriptors of a raw scan on the device (spec: include/pointnet_hip.h, pn_fpfh): xyz (N, 3) and normals (N, 3) fp32 (from
    ops.estimate_normals) -> fpfh (N, 33) fp32; with ``return_spfh`` also counts (N, 33) int32, the pair-feature histogram of every
    point, and pairs (N,) int32, the pairs that entered it.  The neighbourhood of a point is ops.radius_knn's list (the ``k`` nearest
    others within ``radius``, 2 <= k <= 16): the descriptors are meant for voxel-downsampled clouds, where 16 neighbours span the
    radius.  A pair with a non-finite normal is left out; a point without neighbours gets a zero row.  A row with a non-finite
    coordinate is masked out before the call: zero row, nobody's neighbour.  ``origin`` and the host reads: as in ops.radius_knn."""
    require_gpu_tensor(xyz, "xyz", F32)
    require_gpu_tensor(normals, "normals", F32)
    if xyz.dim() != 2 or xyz.shape[1] != 3 or normals.shape != xyz.shape:
        raise _lib.PointNetHipError(f"fpfh expects (N, 3) points and normals, got {tuple(xyz.shape)} and {tuple(normals.shape)}")
    W, k = _lib.PN_FPFH_BINS, int(k)
    outs = [((W,), F32, 0, False), ((W,), torch.int32, 0, False) if return_spfh else None, ((), torch.int32, 0, False) if return_spfh else None]
    nrm = [normals]                      # (held here: the compacted copy must outlive the call)

    def head(pts, n, org, part, rows):
        if pts is not xyz:
            nrm[0] = normals[rows].contiguous()
        return (ptr(pts), ptr(nrm[0]), n, float(radius), org, k, *map(ptr, part))

    # the sizer gives 0 for a k outside the limits, which the call refuses: it still gets pn_radius_knn's workspace
    full, _ = _scan_call("fpfh", xyz, origin, outs, "pn_fpfh", "pn_fpfh_workspace_bytes", head, size_args=(k,),
                         floor="pn_radius_knn_workspace_bytes", errors="pn_radius_knn", **_radius_grid(radius))
    return tuple(full) if return_spfh else full[0]


def feature_match(a: torch.Tensor, b: torch.Tensor, mutual: bool = False):
    """Nearest descriptor on the device (spec: include/pointnet_hip.h, pn_feature_match): a (Na, 33), b (Nb, 33) fp32 -> (idx (Na,)
    int32, d2 (Na,) fp32): for every row of ``a`` the row of ``b`` at the least squared distance (ties -> the lower row).  A row of
    ``b`` holding a non-finite value is nobody's partner; a row of ``a`` holding one gets (-1, +inf).  ``mutual=True`` also matches
    ``b`` against ``a`` and sets idx to -1 wherever the partner's own partner is another row (d2 stays).  No host read."""
    require_gpu_tensor(a, "a", F32)
    require_gpu_tensor(b, "b", F32)
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
        raise _lib.PointNetHipError(f"feature_match expects (Na, 33) and (Nb, 33) descriptors, got {tuple(a.shape)} and {tuple(b.shape)}")

    def one(u, v):
        nu, nv = u.shape[0], v.shape[0]
        idx = torch.empty(nu, device=u.device, dtype=torch.int32)
        d2 = torch.empty(nu, device=u.device, dtype=F32)
        nbytes = lib().pn_feature_match_workspace_bytes(nu, nv)
        ws = torch.empty(max(nbytes, 16), device=u.device, dtype=torch.uint8)
        check(lib().pn_feature_match(ptr(u), nu, ptr(v), nv, u.shape[1], ptr(idx), ptr(d2), ptr(ws), nbytes, current_stream()), "pn_feature_match")
        return idx, d2

    idx, d2 = one(a, b)
    if mutual:
        back, _ = one(b, a)
        here = torch.arange(a.shape[0], device=a.device, dtype=torch.int32)
        idx = torch.where((idx >= 0) & (back[idx.long().clamp(min=0)] == here), idx, torch.full_like(idx, -1))
    return idx, d2


def ransac_poses(src: torch.Tensor, tgt: torch.Tensor, max_dist: float, hypotheses: int = 4096, edge_ratio: float = 0.9, seed: int = 0,
                 return_rows: bool = False):
    """RANSAC pose hypotheses on putative correspondences (spec: include/pointnet_hip.h, pn_ransac_poses): src, tgt (C, 3) fp32, paired
    row by row -> (poses (H, 4, 4) fp64, counts (H,) int32, order (H,) int64).  Hypothesis h is the rigid fit p_src ~ R q_tgt + t of
    three drawn pairs; counts[h] is the number of pairs within ``max_dist`` under it, -1 (pose NaN) for a draw that repeats a row,
    holds a non-finite point, fails the edge-length check at ``edge_ratio`` or is collinear.  ``order`` ranks the hypotheses by
    (count descending, h ascending).  ``return_rows`` adds rows (H, 3) int32, the drawn pairs.  No host read."""
    require_gpu_tensor(src, "src", F32)
    require_gpu_tensor(tgt, "tgt", F32)
    if src.dim() != 2 or src.shape[1] != 3 or tgt.shape != src.shape:
        raise _lib.PointNetHipError(f"ransac_poses expects two (C, 3) clouds paired row by row, got {tuple(src.shape)} and {tuple(tgt.shape)}")
    if not 0 <= int(seed) < 1 << 64:
        raise _lib.PointNetHipError(f"ransac_poses: seed must lie in [0, 2^64), got {seed!r}")
    Cn, H, dev = src.shape[0], int(hypotheses), src.device
    Hc = min(max(H, 1), _lib.PN_RANSAC_MAX_HYPOTHESES)
    poses = torch.empty(Hc, 4, 4, device=dev, dtype=torch.float64)
    counts = torch.empty(Hc, device=dev, dtype=torch.int32)
    rows = torch.empty(Hc, 3, device=dev, dtype=torch.int32) if return_rows else None
    nbytes = lib().pn_ransac_poses_workspace_bytes(Cn, H)           # 0 for a shape outside the limits: the call below refuses it
    ws = torch.empty(max(nbytes, 16), device=dev, dtype=torch.uint8)
    check(lib().pn_ransac_poses(ptr(src), ptr(tgt), Cn, float(max_dist), H, float(edge_ratio), int(seed), ptr(poses), ptr(counts), ptr(rows),
                                ptr(ws), nbytes, current_stream()), "pn_ransac_poses")
    order = torch.sort(counts, descending=True, stable=True).indices
    return (poses, counts, order, rows) if return_rows else (poses, counts, order)


def incidence_mask(xyz: torch.Tensor, normals: torch.Tensor, viewpoint, max_angle_deg: float) -> torch.Tensor:
    """bool (N,): the mixed-pixel (grazing-incidence) filter on per-point normals.  In fp64, with v = viewpoint - p: keep a point iff
    its normal is finite and (n.v)^2 >= cos^2(max_angle_deg) * (v.v), i.e. iff the angle between the normal's line and the view ray
    is at most ``max_angle_deg`` (0 < max_angle_deg < 90; the normal's sign does not matter).  A point at the viewpoint (v = 0) and a
    non-finite row are dropped.  torch only: it runs wherever its inputs live."""
    ang = float(max_angle_deg)
    if not 0.0 < ang < 90.0:
        raise _lib.PointNetHipError(f"incidence_mask: max_angle_deg must lie in (0, 90), got {max_angle_deg!r}")
    if xyz.dim() != 2 or xyz.shape[1] != 3 or normals.shape != xyz.shape or len(viewpoint) != 3:
        raise _lib.PointNetHipError(f"incidence_mask: xyz (N, 3), normals (N, 3) and three viewpoint values expected, got "
                                    f"{tuple(xyz.shape)}, {tuple(normals.shape)}, {viewpoint!r}")
    vp = torch.tensor([float(a) for a in viewpoint], dtype=torch.float64, device=xyz.device)
    v = vp - xyz.to(torch.float64)
    n = normals.to(torch.float64)
    nv = (n[:, 0] * v[:, 0] + n[:, 1] * v[:, 1]) + n[:, 2] * v[:, 2]
    vv = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    c = math.cos(math.radians(ang))
    return torch.isfinite(n).all(1) & (vv > 0) & (nv * nv >= (c * c) * vv)           # (a NaN compares false)


def outlier_mask(xyz: torch.Tensor, method: str, radius: float, k: int = 8, min_neighbors: int = 8, std_ratio: float = 2.0, origin=None,
                 viewpoint=(0.0, 0.0, 0.0), max_angle_deg: float = 75.0):
    """bool (N,) keep mask of a raw scan (PCL / Open3D outlier removal on ops.radius_knn).  ``method="radius"``: keep a point with at
    least ``min_neighbors`` other points within ``radius`` (the count-only search).  ``method="statistical"``: ops.neighbor_stat_mask
    on the ``k`` nearest neighbours within ``radius`` (a point with fewer than k is dropped).  ``method="incidence"``: the
    mixed-pixel filter, ops.incidence_mask on ops.estimate_normals(xyz, radius, k, viewpoint, origin): a point whose normal is more
    than ``max_angle_deg`` away from its ray to ``viewpoint`` (default: the sensor origin), or has none, is dropped.  A non-finite
    row is never kept."""
    if method == "radius":
        return (radius_knn(xyz, radius, 0, origin)[2] >= int(min_neighbors)) & torch.isfinite(xyz).all(1)
    if method == "statistical":
        _, d2, count = radius_knn(xyz, radius, k, origin)
        return neighbor_stat_mask(d2, count, k, std_ratio)
    if method == "incidence":
        return incidence_mask(xyz, estimate_normals(xyz, radius, k, viewpoint, origin)[0], viewpoint, max_angle_deg)
    raise _lib.PointNetHipError(f"outlier_mask: method must be 'radius', 'statistical' or 'incidence', got {method!r}")


def plane_segment(xyz: torch.Tensor, threshold: float, max_planes: int = 1, hypotheses: int = 1024, min_inliers: int = 3, seed: int = 0,
                  axis=None, max_angle_deg=None, return_hypotheses: bool = False):
    """RANSAC plane segmentation on the device (spec: include/pointnet_hip.h, pn_plane_segment): xyz (N, 3) fp32 -> (planes (P, 4)
    fp64, counts (P,) int32, plane_id (N,) int32) with P = ``max_planes``.  Round r draws ``hypotheses`` planes through three points
    of what is left, keeps the one with the most points within ``threshold``, refines it over them (fp64 PCA) and puts every point
    within ``threshold`` of the refined plane (n, d), n.p + d = 0, on plane r; a round that finds fewer than ``min_inliers`` ends
    the segmentation, and the rows of planes / counts from there on are zero.  plane_id is -1 for a point on no plane; a row with a
    non-finite coordinate is never drawn and never on a plane.  ``axis`` with ``max_angle_deg`` only admits planes whose normal
    lies within that angle of +-axis (a floor: axis = up).  The draws are a pure function of ``seed``.  With
    ``return_hypotheses`` a fourth value follows, hyp_counts (P, H) int32: every hypothesis's score, -1 for an invalid one and for
    the rounds that did not run.  No host read."""
    require_gpu_tensor(xyz, "xyz", F32)
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise _lib.PointNetHipError(f"plane_segment expects (N, 3) points, got {tuple(xyz.shape)}")
    if (axis is None) != (max_angle_deg is None):
        raise _lib.PointNetHipError("plane_segment: axis and max_angle_deg go together")
    N, dev = xyz.shape[0], xyz.device
    P, H = int(max_planes), int(hypotheses)
    if not 0 <= int(seed) < 1 << 64:
        raise _lib.PointNetHipError(f"plane_segment: seed must lie in [0, 2^64), got {seed!r}")
    axis3, cos_max = None, 0.0
    if axis is not None:
        axis3 = [float(v) for v in (axis.tolist() if hasattr(axis, "tolist") else axis)]
        if len(axis3) != 3:
            raise _lib.PointNetHipError(f"plane_segment: axis must have three components, got {axis!r}")
        if not 0.0 <= float(max_angle_deg) <= 90.0:
            raise _lib.PointNetHipError(f"plane_segment: max_angle_deg must lie in [0, 90], got {max_angle_deg!r}")
        cos_max = math.cos(math.radians(float(max_angle_deg)))
    nbytes = lib().pn_plane_segment_workspace_bytes(N, H, P)        # 0 for a shape outside the limits: the call below refuses it
    Pc, Hc = min(max(P, 1), _lib.PN_PLANE_MAX_PLANES), min(max(H, 1), _lib.PN_PLANE_MAX_HYPOTHESES)
    planes = torch.empty(Pc, 4, device=dev, dtype=torch.float64)
    counts = torch.empty(Pc, device=dev, dtype=torch.int32)
    plane_id = torch.empty(N, device=dev, dtype=torch.int32)
    hyp = torch.empty(Pc, Hc, device=dev, dtype=torch.int32) if return_hypotheses else None
    ws = torch.empty(max(nbytes, 16), device=dev, dtype=torch.uint8)
    check(lib().pn_plane_segment(ptr(xyz), N, float(threshold), H, P, int(min_inliers), int(seed), _f3(axis3) if axis3 else None, cos_max,
                                 ptr(planes), ptr(counts), ptr(plane_id), ptr(hyp), ptr(ws), nbytes, current_stream()), "pn_plane_segment")
    return (planes, counts, plane_id, hyp) if return_hypotheses else (planes, counts, plane_id)


def plane_mask(plane_id: torch.Tensor) -> torch.Tensor:
    """bool (N,) keep mask of ops.plane_segment's result: the points on no plane"""
    return plane_id < 0


def knn_propagate(query: torch.Tensor, ref: torch.Tensor, k: int, values: Optional[torch.Tensor] = None):
    """Exact k nearest refs of every query, and optionally the inverse-distance-weighted mix of the refs' values (spec:
    include/pointnet_hip.h, pn_knn_propagate).  query (B,Nq,3), ref (B,M,3), values (B,M,C) fp32 ->
    (idx (B,Nq,k) int32, d2 (B,Nq,k)) ordered by ascending (distance, ref index), or with values
    (idx, d2, values_out (B,Nq,C), arg (B,Nq) int32: first arg-max of values_out, -1 where no neighbour was found)."""
    require_gpu_tensor(query, "query", F32)
    require_gpu_tensor(ref, "ref", F32)
    if query.dim() != 3 or query.shape[2] != 3 or ref.dim() != 3 or ref.shape[2] != 3 or ref.shape[0] != query.shape[0]:
        raise _lib.PointNetHipError(f"knn_propagate: query (B,Nq,3) and ref (B,M,3) expected, got {tuple(query.shape)} / {tuple(ref.shape)}")
    if ref.device != query.device:
        raise _lib.PointNetHipError("knn_propagate: query and ref must be on the same device")
    B, Nq, _ = query.shape
    M = ref.shape[1]
    dev = query.device
    kk = max(int(k), 0)                   # (a k outside [1, 8] is refused by the library)
    idx = torch.empty(B, Nq, kk, device=dev, dtype=torch.int32)
    d2 = torch.empty(B, Nq, kk, device=dev, dtype=F32)
    vout = arg = None
    C_ = 0
    if values is not None:
        require_gpu_tensor(values, "values", F32)
        if values.dim() != 3 or tuple(values.shape[:2]) != (B, M) or values.device != dev:
            raise _lib.PointNetHipError(f"knn_propagate: values must be (B,M,C) = ({B},{M},C) on {dev}, got {tuple(values.shape)}")
        C_ = values.shape[2]
        vout = torch.empty(B, Nq, C_, device=dev, dtype=F32)
        arg = torch.empty(B, Nq, device=dev, dtype=torch.int32)
    check(lib().pn_knn_propagate(ptr(query), ptr(ref), B, Nq, M, int(k), ptr(values), C_, ptr(idx), ptr(d2), ptr(vout), ptr(arg),
                                 current_stream()), "pn_knn_propagate")
    return (idx, d2) if values is None else (idx, d2, vout, arg)


def _host_array(a, dtype):
    import numpy as np
    return (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(dtype)


def _max_d2(max_dist):
    import numpy as np
    return float(np.float32(float(max_dist) * float(max_dist)))       # fp32(max_dist^2); inf stays inf


class _IcpGrouped:
    """What the grouped references share: the host offsets ``seg`` (label l in rows [seg[l], seg[l + 1])), their copy for the C
    entry points, ``n_parts`` and the primitive count ``M``.  A kind describes itself to the wrappers in class-level data, so that
    none of them asks for a reference's class to serve it: ``_PRIM``, the field that holds the primitives; ``_PASS``, ``_LOOP`` and
    ``_SIZER``, the single-pass entry, the loop entry and the workspace sizer as (point, plane) pairs; ``_LEGACY``, whether those
    are the two cloud entries that predate the general argument list (no mode or metric, normals only in the plane one);
    ``_IS_MESH``, the robust entries' flag; ``_NO_ROBUST``, the refusal of a kind the robust entries do not take; ``_GICP``, the
    plane-to-plane pass, loop and sizer of a kind that has them (a cloud), whose trailing arguments are ``_gicp_tail()``."""
    _NO_ROBUST = None
    _GICP = None
    _INFO = None

    def __init__(self, seg, n_parts):
        self.seg, self.n_parts = tuple(int(v) for v in seg), int(n_parts)
        self._seg_c = (C.c_int32 * len(self.seg))(*self.seg)

    @property
    def M(self):
        return self.seg[-1]

    @property
    def _prim(self):
        return getattr(self, self._PRIM)

    def _serves(self, what, max_dist, plane=False, robust=False):
        """the refusals a reference makes before anything touches the device"""
        if robust and self._NO_ROBUST:
            raise _lib.PointNetHipError(self._NO_ROBUST)

    def _check_normals(self, what, dev, name):
        require_gpu_tensor(self.normals, f"{name}.normals", F32)
        if tuple(self.normals.shape) != (self.M, 3) or self.normals.device != dev:
            raise _lib.PointNetHipError(f"{what}: {name}.normals must be ({self.M}, 3) on {dev}")

    def _tail(self):
        """the trailing arguments of the kind's accelerated entries"""
        return ()


class IcpReference(_IcpGrouped):
    """A labelled reference cloud grouped by label for the ICP entry points (ops.icp_reference): ``xyz`` (M, 3) fp32 on the
    device, label l in rows [seg[l], seg[l + 1]) in the original order; ``index`` (M,) int64 maps a grouped row back to the
    row of the cloud as given; ``n_parts`` labels; ``normals`` (M, 3) fp32 in the same grouped order, or None (point-to-plane
    ICP needs them: ops.icp_reference(normals=...) or ops.icp_normals)."""
    _PRIM, _IS_MESH, _LEGACY = "xyz", 0, True
    _PASS = ("pn_icp_correspond", "pn_icp_plane_sums")
    _LOOP = ("pn_semantic_icp", "pn_semantic_icp_plane")
    _SIZER = ("pn_icp_workspace_bytes", "pn_icp_plane_workspace_bytes")
    _GICP = ("pn_icp_gicp_sums", "pn_semantic_icp_gicp", "pn_icp_gicp_workspace_bytes")
    _INFO = ("pn_icp_information", "pn_icp_information_workspace_bytes")

    def __init__(self, xyz, seg, index, n_parts, normals=None):
        super().__init__(seg, n_parts)
        self.xyz, self.index, self.normals = xyz, index, normals

    def _need_normals(self, what):
        if self.normals is None:
            raise _lib.PointNetHipError(f"{what}: point-to-plane and plane-to-plane ICP needs reference normals (ops.icp_normals or "
                                        "icp_reference(normals=...))")

    def _serves(self, what, max_dist, plane=False, robust=False):
        if plane:
            self._need_normals(what)
        super()._serves(what, max_dist, plane, robust)

    def _check(self, what, dev, plane=False, name="ref"):
        """the kind's own fields as the entries take them on ``dev``; the normals only where the plane metric reads them"""
        if plane:
            self._need_normals(what)
            self._check_normals(what, dev, name)

    def _entry_normals(self, plane):
        return self.normals if plane else None

    def _gicp_tail(self):
        """the plane-to-plane entries' grid arguments: none, the brute-force search"""
        return None, 0.0

    def _with_normals(self, normals):
        """the same reference, of the same kind and over the same tensors, carrying ``normals``"""
        import copy
        ref = copy.copy(self)
        ref.normals = normals
        return ref

    def _score_cloud(self):
        """the grouped cloud the reference is scored against -> (xyz, seg for the C entry, count)"""
        return self.xyz, self._seg_c, self.M

    def _part_moments(self):
        dev = self.xyz.device
        seg = torch.tensor(self.seg, device=dev)
        lab = torch.repeat_interleave(torch.arange(self.n_parts, device=dev, dtype=torch.int32), seg[1:] - seg[:-1], output_size=self.M)
        return part_moments(self.xyz.reshape(1, self.M, 3), lab.reshape(1, self.M).contiguous(), self.n_parts)[0]


class IcpGridReference(IcpReference):
    """An IcpReference with a voxel grid over its points (ops.icp_reference(..., accel="grid", max_dist=...); spec:
    include/pointnet_hip.h, pn_icp_grid_build): ``grid``, the tables as the library wrote them (uint8 on the device); ``max_dist``,
    the largest max_dist a search through them may use, and ``r2`` = fp32(max_dist^2), what the tables were built for; ``origin``,
    the grid's origin.  ops.icp_correspond, ops.icp_plane_sums, ops.semantic_icp (both metrics), the refinement of ops.global_pose
    and PointNet.predict_pose search the grid and return, for every pair within max_dist, bit for bit what they return for the plain
    reference (beyond it: no partner, d2 = +inf), at a cost that no longer grows with the reference; they refuse a max_dist above the
    reference's, the default inf included.  The robust loop does not take it; every other taker of a cloud reference uses the
    fields it shares with one."""

    _LEGACY = False
    _PASS, _LOOP, _SIZER = 2 * ("pn_icp_grid_correspond",), 2 * ("pn_semantic_icp_grid",), 2 * ("pn_icp_plane_workspace_bytes",)
    _NO_ROBUST = ("the robust, confidence-weighted ICP entries (robust=, weights=) search a cloud by brute force and "
                  "take no accelerated reference: build it with ops.icp_reference(..., accel=None)")

    def __init__(self, xyz, seg, index, n_parts, normals, grid, max_dist, r2, origin):
        super().__init__(xyz, seg, index, n_parts, normals=normals)
        self.grid, self.max_dist, self.r2, self.origin = grid, float(max_dist), float(r2), tuple(float(v) for v in origin)

    def _serves(self, what, max_dist, plane=False, robust=False):
        """a grid reference serves max_dist only up to its own"""
        super()._serves(what, max_dist, plane, robust)
        if _max_d2(max_dist) > self.r2 or max_dist != max_dist:
            raise _lib.PointNetHipError(f"{what}: max_dist={max_dist} exceeds the grid reference's max_dist={self.max_dist:g} (a grid search sees no "
                                        "pair beyond it; build the reference with a larger max_dist, or pass max_dist explicitly: the default is inf)")

    def _check(self, what, dev, plane=False, name="ref"):
        super()._check(what, dev, plane, name)
        require_gpu_tensor(self.grid, f"{name}.grid", torch.uint8)
        if self.grid.device != dev or self.grid.numel() < lib().pn_icp_grid_bytes(self.M):
            raise _lib.PointNetHipError(f"{what}: {name}.grid must hold the {lib().pn_icp_grid_bytes(self.M)} bytes of the tables on {dev}")

    def _tail(self):
        return ptr(self.grid), self.r2

    _gicp_tail = _tail


def _grid_max_dist(what, max_dist):
    """the max_dist of a grid reference: positive and finite, with a normal fp32 square"""
    import math
    if max_dist is None:
        raise _lib.PointNetHipError(f"{what}: accel='grid' needs max_dist, the largest max_dist a search will use (the grid's leaf follows it)")
    md = float(max_dist)
    r2 = _max_d2(md) if math.isfinite(md) else float("inf")
    if not (md > 0.0 and 1.17549435e-38 <= r2 <= 3.402823466e38):
        raise _lib.PointNetHipError(f"{what}: accel='grid' needs a positive finite max_dist whose square is a normal fp32 number, got {max_dist!r}")
    return md, r2


def _build_icp_grid(what, xyz, max_dist, r2, origin=None):
    """the tables of a grouped, finite cloud (M, 3) on the device -> (grid, origin); reads the error word back once"""
    M = xyz.shape[0]
    if M < 1:
        raise _lib.PointNetHipError(f"{what}: accel='grid' needs at least one reference point")
    if origin is None:
        origin = xyz.min(0).values.cpu().tolist()
    nbytes = lib().pn_icp_grid_bytes(M)
    grid = torch.zeros(max(nbytes, 16), device=xyz.device, dtype=torch.uint8)
    _grid_call("pn_icp_grid_build", "pn_icp_grid_build_workspace_bytes", M, xyz.device, ptr(xyz), M, r2, _f3(origin), ptr(grid), nbytes,
               max_key=_lib.PN_RADIUS_KNN_MAX_KEY, leaf=lib().pn_icp_grid_leaf(r2))
    return grid, origin


def _with_grid(what, ref, max_dist):
    """an IcpReference on the device -> the IcpGridReference over the same tensors"""
    md, r2 = _grid_max_dist(what, max_dist)
    require_gpu_tensor(ref.xyz, "ref.xyz", F32)
    if not bool(torch.isfinite(ref.xyz).all()):
        raise _lib.PointNetHipError(f"{what}: accel='grid' needs a finite reference (a row of the reference is not finite)")
    grid, origin = _build_icp_grid(what, ref.xyz, md, r2)
    return IcpGridReference(ref.xyz, ref.seg, ref.index, ref.n_parts, ref.normals, grid, md, r2, origin)


def _grid_request(what, accel, max_dist):
    """the accel= / max_dist= request of the calls that may put a grid over their cloud (checked before any other work)"""
    if accel not in (None, "grid"):
        raise _lib.PointNetHipError(f"{what}: accel must be None or 'grid', got {accel!r}")
    if accel == "grid":
        _grid_max_dist(what, max_dist)
    elif max_dist is not None:
        raise _lib.PointNetHipError(f"{what}: max_dist goes with accel='grid'")


def icp_reference(xyz, labels, n_parts: int, device=None, normals=None, accel=None, max_dist=None) -> IcpReference:
    """Group a labelled reference cloud by label, once per reference (host-side): xyz (M0, 3) and labels (M0,) as tensors or
    arrays; points whose label is outside [0, n_parts) are dropped.  ``device`` defaults to xyz's when it is a HIP tensor, else
    the current device.  ``normals`` (M0, 3), optional: unit normals of the points as given (e.g. mesh vertex normals), grouped
    with them into ``IcpReference.normals`` for point-to-plane ICP; a row that is not finite takes no part there.  ``accel`` =
    "grid" with ``max_dist`` (positive, finite: the largest max_dist a search will use) also builds a voxel grid over the grouped
    points on the device (pn_icp_grid_build; one host read of its error word) and returns an IcpGridReference: the same pairs
    within max_dist at a cost that no longer grows with M (meant for references of tens of thousands of points and more).  Every
    kept row must then be finite."""
    import numpy as np
    _grid_request("icp_reference", accel, max_dist)
    if device is None:
        device = xyz.device if isinstance(xyz, torch.Tensor) and xyz.is_cuda else torch.device("cuda", torch.cuda.current_device())
    x = _host_array(xyz, np.float32).reshape(-1, 3)
    lab = _host_array(labels, np.int64).reshape(-1)
    if lab.shape[0] != x.shape[0]:
        raise _lib.PointNetHipError(f"icp_reference: {x.shape[0]} points but {lab.shape[0]} labels")
    keep = np.flatnonzero((lab >= 0) & (lab < n_parts))
    order = keep[np.argsort(lab[keep], kind="stable")]
    seg = np.searchsorted(lab[order], np.arange(n_parts + 1), side="left") if n_parts >= 0 else np.zeros(1, np.int64)
    if accel == "grid":
        bad = np.flatnonzero(~np.isfinite(x[order]).all(1))
        if bad.size:
            raise _lib.PointNetHipError(f"icp_reference: accel='grid' needs a finite reference; row {int(order[bad[0]])} of xyz is "
                                        f"{x[order[bad[0]]].tolist()} ({bad.size} such rows among the kept ones)")
    nrm = None
    if normals is not None:
        nm = _host_array(normals, np.float32)
        if nm.shape != x.shape:
            raise _lib.PointNetHipError(f"icp_reference: normals must be ({x.shape[0]}, 3), got {nm.shape}")
        nrm = torch.from_numpy(np.ascontiguousarray(nm[order])).to(device)
    ref = IcpReference(torch.from_numpy(np.ascontiguousarray(x[order])).to(device), seg, torch.from_numpy(order).to(device),
                       n_parts, normals=nrm)
    return ref if accel is None else _with_grid("icp_reference", ref, max_dist)


class IcpMeshReference(_IcpGrouped):
    """A labelled triangle mesh grouped by label for the ICP entry points (ops.icp_mesh_reference): ``tri`` (T, 3, 3) fp32 on the
    device, the vertices a, b, c of every kept triangle, label l in rows [seg[l], seg[l + 1]) in the original order; ``normals``
    (T, 3) fp32, the unit face normals (cross(b - a, c - a) in fp64 from the fp32 vertices, normalised, rounded; winding does not
    matter to point-to-plane ICP: its terms are invariant under n -> -n); ``area`` (T,) fp64; ``index`` (T,) int64 maps a
    grouped row back to the row of ``faces`` as given; ``n_parts`` labels."""

    _PRIM, _IS_MESH, _LEGACY = "tri", 1, False
    _PASS, _LOOP, _SIZER = 2 * ("pn_icp_mesh_correspond",), 2 * ("pn_semantic_icp_mesh",), 2 * ("pn_icp_mesh_workspace_bytes",)

    def __init__(self, tri, seg, index, n_parts, normals, area):
        super().__init__(seg, n_parts)
        self.tri, self.index, self.normals, self.area = tri, index, normals, area

    T = _IcpGrouped.M    # the primitive count, under the name the mesh entry points give it

    def _check(self, what, dev=None, plane=False, name="ref", normals=True, area=False, trees=False):
        """the kind's own fields as the entries take them on ``dev`` (None: wherever ``tri`` is) -> that device; the ICP entries
        read the face normals under either metric, the sampler ``area``, and only a reference that has trees can be asked for them"""
        require_gpu_tensor(self.tri, f"{name}.tri", F32)
        dev = self.tri.device if dev is None else dev
        if tuple(self.tri.shape) != (self.T, 3, 3):
            raise _lib.PointNetHipError(f"{what}: {name}.tri must be ({self.T}, 3, 3), got {tuple(self.tri.shape)}")
        if normals:
            self._check_normals(what, dev, name)
        if area:
            require_gpu_tensor(self.area, f"{name}.area", torch.float64)
            if tuple(self.area.shape) != (self.T,) or self.area.device != dev:
                raise _lib.PointNetHipError(f"{what}: {name}.area must be ({self.T},) on {dev}, got {tuple(self.area.shape)}")
        if trees:
            self._check_trees(what, dev, name)
        return dev

    def _check_trees(self, what, dev, name):
        raise _lib.PointNetHipError(f"{what}: accel='bvh' needs a reference built by ops.icp_mesh_reference(..., accel=\"bvh\")")

    def _entry_normals(self, plane):
        return self.normals

    def _score_cloud(self):
        """a mesh is scored against its labelled vertices: tri viewed as (3T, 3) with seg * 3, already grouped, no copy"""
        seg = tuple(3 * v for v in self.seg)
        return self.tri.view(3 * self.T, 3), (C.c_int32 * len(seg))(*seg), 3 * self.T

    def _part_moments(self):
        dev = self.tri.device
        seg = torch.tensor(self.seg, device=dev)
        lab = torch.repeat_interleave(torch.arange(self.n_parts, device=dev), seg[1:] - seg[:-1], output_size=self.T)
        area = self.area.double()
        val = torch.cat([area[:, None], self.tri.double().mean(1) * area[:, None]], 1)
        return torch.zeros(self.n_parts, 4, device=dev, dtype=torch.float64).index_add_(0, lab, val)


class IcpBvhMeshReference(IcpMeshReference):
    """An IcpMeshReference with one bounding-volume hierarchy per label (ops.icp_mesh_reference(..., accel="bvh"); spec:
    include/pointnet_hip.h, pn_icp_bvh_build): ``nodes`` (n_nodes, 8) int32 on the device, the 32-byte nodes as the library
    wrote them (lo xyz, hi xyz as fp32 bits, first, count); ``rows`` (T,) int32 on the device, the leaves' grouped rows;
    ``roots``, the root node of every label on the host, -1 for a label without triangles.  ops.icp_mesh_correspond and
    ops.semantic_icp search the trees and return, bit for bit, what they return for the plain reference; ops.lidar_cast and
    ops.lidar_frames (and pointcloud.simulate_dataset) cast their rays through them when called with accel="bvh"; every other
    taker of a mesh reference, and those three without the keyword, use the fields it shares with one."""

    _PASS, _LOOP = 2 * ("pn_icp_bvh_correspond",), 2 * ("pn_semantic_icp_bvh",)
    _NO_ROBUST = ("the robust, confidence-weighted ICP entries (robust=, weights=) search a mesh by brute force and "
                  "take no accelerated reference: build it with ops.icp_mesh_reference(..., accel=None)")

    def __init__(self, tri, seg, index, n_parts, normals, area, nodes, rows, roots):
        super().__init__(tri, seg, index, n_parts, normals, area)
        self.nodes, self.rows, self.roots = nodes, rows, tuple(int(v) for v in roots)
        self._roots_c = (C.c_int32 * len(self.roots))(*self.roots)

    @property
    def n_nodes(self):
        return int(self.nodes.shape[0])

    def _check(self, what, dev=None, plane=False, name="ref", normals=True, area=False, trees=True):
        return super()._check(what, dev, plane, name, normals, area, trees)

    def _check_trees(self, what, dev, name):
        require_gpu_tensor(self.nodes, f"{name}.nodes", torch.int32)
        require_gpu_tensor(self.rows, f"{name}.rows", torch.int32)
        if (self.nodes.dim() != 2 or self.nodes.shape[1] != 8 or tuple(self.rows.shape) != (self.T,) or self.nodes.device != dev
                or self.rows.device != dev or len(self.roots) != self.n_parts):
            raise _lib.PointNetHipError(f"{what}: {name}.nodes must be (n_nodes, 8) int32 and {name}.rows ({self.T},) int32 on {dev}, "
                                        f"{name}.roots {self.n_parts} node indices")

    def _tail(self):
        return ptr(self.nodes), ptr(self.rows), self._roots_c, self.n_nodes


def _build_bvh(tri, seg, n_parts):
    """the trees of a grouped host mesh (T, 3, 3) fp32 through the library's host builder -> (nodes (n_nodes, 8) int32, rows
    (T,) int32, roots (n_parts,) int32), all NumPy"""
    import numpy as np
    T = tri.shape[0]
    tri = np.ascontiguousarray(tri, np.float32)
    cap = lib().pn_icp_bvh_max_nodes(T, n_parts)
    nodes = np.zeros((max(cap, 1), 8), np.int32)
    rows = np.zeros(max(T, 1), np.int32)
    roots = np.zeros(max(n_parts, 1), np.int32)
    n_nodes = C.c_int32(0)
    seg_c = (C.c_int32 * len(seg))(*[int(v) for v in seg])
    check(lib().pn_icp_bvh_build(tri.ctypes.data_as(C.c_void_p), seg_c, T, n_parts, nodes.ctypes.data_as(C.c_void_p),
                                 rows.ctypes.data_as(C.c_void_p), roots.ctypes.data_as(C.c_void_p), C.byref(n_nodes)), "pn_icp_bvh_build")
    return nodes[:n_nodes.value].copy(), rows[:T], roots[:n_parts]


def icp_mesh_reference(vertices, faces, labels, n_parts: int, device=None, accel=None) -> IcpMeshReference:
    """Group a labelled triangle mesh by label, once per reference (host-side): vertices (V, 3), faces (F, 3) vertex indices and
    labels (F,) part ids as tensors or arrays (pointcloud.read_labelled_mesh returns them).  Dropped: triangles whose label is
    outside [0, n_parts), and degenerate ones (a non-finite vertex, or zero area in fp64).  The rest keep their order inside a
    label.  ``device`` defaults to the vertices' when they are a HIP tensor, else the current device.  ``accel`` = "bvh" also
    builds one bounding-volume hierarchy per label on the host (pn_icp_bvh_build) and returns an IcpBvhMeshReference: the same
    answers from ops.icp_mesh_correspond and ops.semantic_icp, and from ops.lidar_cast / ops.lidar_frames called with
    accel="bvh", at a cost that no longer grows with the triangle count (meant for meshes of thousands of triangles and more;
    the robust loop does not take it)."""
    import numpy as np
    if accel not in (None, "bvh"):
        raise _lib.PointNetHipError(f"icp_mesh_reference: accel must be None or 'bvh', got {accel!r}")
    if device is None:
        device = vertices.device if isinstance(vertices, torch.Tensor) and vertices.is_cuda else torch.device("cuda", torch.cuda.current_device())
    v = _host_array(vertices, np.float32).reshape(-1, 3)
    f = _host_array(faces, np.int64).reshape(-1, 3)
    lab = _host_array(labels, np.int64).reshape(-1)
    if lab.shape[0] != f.shape[0]:
        raise _lib.PointNetHipError(f"icp_mesh_reference: {f.shape[0]} faces but {lab.shape[0]} labels")
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise _lib.PointNetHipError(f"icp_mesh_reference: a face index is outside [0, {v.shape[0]})")
    tri = v[f]                                                        # (F, 3, 3) fp32
    t64 = tri.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        cr = np.cross(t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 0])
        nn = np.sqrt((cr * cr).sum(1))
    ok = np.isfinite(tri).all((1, 2)) & np.isfinite(nn) & (nn > 0) & (lab >= 0) & (lab < n_parts)
    keep = np.flatnonzero(ok)
    order = keep[np.argsort(lab[keep], kind="stable")]
    seg = np.searchsorted(lab[order], np.arange(n_parts + 1), side="left")
    nrm = (cr[order] / nn[order, None]).astype(np.float32)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)          # noqa: E731
    if accel is None:
        return IcpMeshReference(to(tri[order]), seg, to(order), n_parts, to(nrm), to(0.5 * nn[order]))
    if order.size == 0:
        raise _lib.PointNetHipError("icp_mesh_reference: accel='bvh' needs at least one kept triangle")
    nodes, rows, roots = _build_bvh(tri[order], seg, n_parts)
    return IcpBvhMeshReference(to(tri[order]), seg, to(order), n_parts, to(nrm), to(0.5 * nn[order]), to(nodes), to(rows), roots)


def icp_normals(ref: IcpReference, k: int = 10):
    """Per-part PCA normals of a grouped reference on the device (spec: include/pointnet_hip.h, pn_icp_normals): the k nearest
    points of the same label (the point included), the fp64 covariance about their mean, its smallest eigenvector signed so that
    the largest component is positive -> (normals (M, 3) fp32, curvature (M,) fp32, the reference carrying the normals).  A
    degenerate point (fewer than 3 neighbours, collinear or coincident neighbours) gets NaN in both: it takes no part in
    point-to-plane ICP.  3 <= k <= 16; one launch, no synchronisation."""
    _family("icp_normals", ref, IcpReference)
    require_gpu_tensor(ref.xyz, "ref.xyz", F32)
    nrm = torch.empty(ref.M, 3, device=ref.xyz.device, dtype=F32)
    curv = torch.empty(ref.M, device=ref.xyz.device, dtype=F32)
    check(lib().pn_icp_normals(ptr(ref.xyz), ref._seg_c, ref.M, ref.n_parts, int(k), ptr(nrm), ptr(curv), None, current_stream()),
          "pn_icp_normals")
    return nrm, curv, ref._with_normals(nrm)


def _family(what, ref, family=_IcpGrouped, name="ref", makers="ops.icp_reference"):
    """The one question a wrapper asks about a reference's class: is it of the family this call takes?  Everything a kind within
    the family does differently comes from the reference itself."""
    if not isinstance(ref, family):
        raise _lib.PointNetHipError(f"{what}: {name} must come from {makers}")


def _icp_inputs(scan, labels, ref, what, plane=False, sizer=None):
    """What every ICP call checks of its scans and reference -> (B, N, the call's workspace, its bytes), sized by the entry
    ``sizer`` names; none with None (the global start's calls, which size their own)."""
    require_gpu_tensor(scan, "scan", F32)
    require_gpu_tensor(labels, "labels", torch.int32)
    if scan.dim() != 3 or scan.shape[2] != 3 or tuple(labels.shape) != tuple(scan.shape[:2]):
        raise _lib.PointNetHipError(f"{what}: scan (B,N,3) and labels (B,N) expected, got {tuple(scan.shape)} / {tuple(labels.shape)}")
    if labels.device != scan.device or ref._prim.device != scan.device:
        raise _lib.PointNetHipError(f"{what}: scan, labels and ref must be on the same device")
    B, N, _ = scan.shape
    ref._check(what, scan.device, plane)
    if sizer is None:
        return B, N, None, 0
    nbytes = getattr(lib(), sizer)(B, N, ref.M, ref.n_parts)
    return B, N, torch.empty(max(nbytes, 1), device=scan.device, dtype=torch.uint8), nbytes


def _icp_pass(what, scan, labels, ref, pose, max_dist, mode, pose_dtype=None, want_q=False, robust=None):
    """The single pass behind icp_correspond, icp_plane_sums, icp_mesh_correspond and icp_robust_sums, through the entry the
    reference names -> (idx (B,N) int32, d2 (B,N) fp32, q (B,N,3) fp32 or None, sums or None, and for the robust entry w (B,N)
    and scale (B,) fp64).  ``mode``: 0 no sums, 1 the point metric's, 2 the plane metric's; ``pose`` (B,4,4): a GPU tensor of
    ``pose_dtype``, or with None any fp32 or fp64 tensor; ``robust``: the robust entry's options as the caller was given them."""
    plane = mode == 2
    ref._serves(what, max_dist, robust=robust is not None)
    B, N, ws, nbytes = _icp_inputs(scan, labels, ref, what, plane, "pn_icp_robust_workspace_bytes" if robust else ref._SIZER[plane])
    if robust:
        robust = _robust_options(what, scan, *robust)
    if pose_dtype is None:
        if not isinstance(pose, torch.Tensor) or tuple(pose.shape) != (B, 4, 4) or pose.dtype not in (F32, torch.float64):
            raise _lib.PointNetHipError(f"{what}: pose must be a ({B},4,4) fp32 or fp64 tensor")
        if plane and pose.dtype != torch.float64:
            raise _lib.PointNetHipError(f"{what}: sums='plane' needs the fp64 pose")
        pose = require_gpu_tensor(pose.contiguous(), "pose")
    else:
        require_gpu_tensor(pose, "pose", pose_dtype)
        if tuple(pose.shape) != (B, 4, 4):
            raise _lib.PointNetHipError(f"{what}: pose must be ({B},4,4), got {tuple(pose.shape)}")
    dev = scan.device
    pose32 = pose.float()                                                             # (the search runs at the fp32 rounding)
    pose64 = pose if plane or robust else None
    idx = torch.empty(B, N, device=dev, dtype=torch.int32)
    d2 = torch.empty(B, N, device=dev, dtype=F32)
    q = torch.empty(B, N, 3, device=dev, dtype=F32) if want_q else None
    so = torch.empty(B, (0, 18, 29)[mode] + bool(robust), device=dev, dtype=torch.float64) if mode else None
    w = sc = None
    head = (ptr(scan), ptr(labels), B, N, ptr(ref._prim), ref._seg_c, ref.M, ref.n_parts)
    out = (ptr(idx), ptr(d2))
    name = "pn_icp_robust_sums" if robust else ref._PASS[plane]
    if robust:
        w = torch.empty(B, N, device=dev, dtype=torch.float64)
        sc = torch.empty(B, device=dev, dtype=torch.float64)
        args = (ref._IS_MESH, ptr(ref.normals) if plane else None, mode, ptr(pose32), ptr(pose64), _max_d2(max_dist), *robust[:4],
                ptr(robust[4]), *out, ptr(q), ptr(w), ptr(sc), ptr(so), ptr(ws), nbytes)
    elif ref._LEGACY:
        args = (ptr(pose32), _max_d2(max_dist), *((ptr(ref.normals), ptr(pose64)) if plane else ()), *out, ptr(so), ptr(ws), nbytes)
    else:
        args = (ptr(pose32), _max_d2(max_dist), mode, ptr(ref._entry_normals(plane)), ptr(pose64), *out, ptr(q), ptr(so), ptr(ws), nbytes,
                *ref._tail())
    check(getattr(lib(), name)(*head, *args, current_stream()), name)
    return idx, d2, q, so, w, sc


def icp_correspond(scan, labels, ref: IcpReference, pose, max_dist=float("inf"), sums: bool = False):
    """One correspondence pass of semantic_icp at a given fp32 pose (B,4,4) (spec: include/pointnet_hip.h, pn_icp_correspond)
    -> (idx (B,N) int32: the partner's row in ref.xyz or -1, d2 (B,N): distance to the nearest same-label reference point, +inf
    when none), and with ``sums`` the (B,18) fp64 sums of the kept pairs.  An IcpGridReference is searched through its grid
    (pn_icp_grid_correspond): the same bits for every point with a reference point within the reference's max_dist, (-1, +inf)
    for the others; ``max_dist`` must then not exceed the reference's."""
    _family("icp_correspond", ref, IcpReference)
    idx, d2, _, so, _, _ = _icp_pass("icp_correspond", scan, labels, ref, pose, max_dist, 1 if sums else 0, F32)
    return (idx, d2, so) if sums else (idx, d2)


def icp_mesh_correspond(scan, labels, ref: IcpMeshReference, pose, max_dist=float("inf"), sums=None):
    """One correspondence pass of semantic_icp against a mesh reference (spec: include/pointnet_hip.h, pn_icp_mesh_correspond):
    every scan point's closest point on the triangles of its label -> (tri (B,N) int32: the winner's row in ref.tri or -1, d2 (B,N)
    fp32, q (B,N,3) fp32: the closest point in the model frame, NaN when there is none), and with ``sums`` = "point" the (B,18) or
    "plane" the (B,29) fp64 sums of the kept pairs.  ``pose`` (B,4,4): fp32, or fp64 (required for "plane": the search runs at
    its fp32 rounding, the plane terms at the pose itself)."""
    _family("icp_mesh_correspond", ref, IcpMeshReference, makers="ops.icp_mesh_reference")
    if sums not in (None, "point", "plane"):
        raise _lib.PointNetHipError(f"icp_mesh_correspond: sums must be None, 'point' or 'plane', got {sums!r}")
    idx, d2, q, so, _, _ = _icp_pass("icp_mesh_correspond", scan, labels, ref, pose, max_dist, {None: 0, "point": 1, "plane": 2}[sums],
                                     want_q=True)
    return (idx, d2, q) if sums is None else (idx, d2, q, so)


def _icp_solve(name, ns, sums, pose, *lead):
    """What the three solves share; ``lead``: the entry's arguments between sums and B"""
    require_gpu_tensor(sums, "sums", torch.float64)
    require_gpu_tensor(pose, "pose", torch.float64)
    B = sums.shape[0]
    if sums.dim() != 2 or sums.shape[1] != ns or tuple(pose.shape) != (B, 4, 4):
        raise _lib.PointNetHipError(f"{name}: sums (B,{ns}) and pose (B,4,4) expected, got {tuple(sums.shape)} / {tuple(pose.shape)}")
    out = pose.clone()
    rmse = torch.empty(B, device=sums.device, dtype=torch.float64)
    status = torch.empty(B, device=sums.device, dtype=torch.int32)
    check(getattr(lib(), "pn_" + name)(ptr(sums), *lead, B, ptr(out), ptr(rmse), ptr(status), current_stream()), "pn_" + name)
    return out, rmse, status


def icp_solve(sums: torch.Tensor, pose: torch.Tensor):
    """The Kabsch solve of semantic_icp on given (B,18) fp64 sums; ``pose`` (B,4,4) fp64 is the previous pose (kept when there
    are fewer than 3 pairs) -> (new pose, rmse (B,) fp64, status (B,) int32)."""
    return _icp_solve("icp_solve", 18, sums, pose)


def icp_plane_sums(scan, labels, ref: IcpReference, pose, max_dist=float("inf")):
    """One correspondence pass of point-to-plane semantic_icp (spec: include/pointnet_hip.h, pn_icp_plane_sums) at the fp64 pose
    (B,4,4): the search runs at its fp32 rounding, the terms at the pose itself -> (idx (B,N) int32 and d2 (B,N), bit for bit
    those of icp_correspond at the rounded pose, and the (B,29) fp64 sums of the pairs whose partner has a finite normal).  An
    IcpGridReference is searched through its grid, as in icp_correspond."""
    _family("icp_plane_sums", ref, IcpReference)
    idx, d2, _, so, _, _ = _icp_pass("icp_plane_sums", scan, labels, ref, pose, max_dist, 2, torch.float64)
    return idx, d2, so


def icp_plane_solve(sums: torch.Tensor, pose: torch.Tensor):
    """The point-to-plane solve of semantic_icp on given (B,29) fp64 sums (spec: pn_icp_plane_solve); ``pose`` (B,4,4) fp64 is
    the pose the terms were taken at (kept when there are fewer than 6 pairs) -> (new pose, rmse (B,) fp64, status (B,) int32:
    PN_ICP_FEW_PAIRS = 2 | PN_ICP_DEGENERATE = 4).  It is also the solve of the plane-to-plane metric: ops.icp_gicp_sums' sums have
    the same layout and meaning (sum J^T W J, sum J^T W d, sum d^T W d)."""
    return _icp_solve("icp_plane_solve", 29, sums, pose)


def _gicp_options(what, scan, ref, scan_normals, eps):
    """What the plane-to-plane calls check beyond _icp_inputs -> eps as a float: a cloud reference, the scans' normals (B, N, 3)
    fp32 beside the scans.  An eps the library refuses (outside (0, 1]) is passed on to it: it reports the error."""
    if ref._GICP is None:
        raise _lib.PointNetHipError(f"{what}: metric 'gicp' (plane to plane) takes a cloud reference (ops.icp_reference), not a mesh")
    if scan_normals is None:
        raise _lib.PointNetHipError(f"{what}: metric 'gicp' needs scan_normals=, the scans' own normals (B,N,3) (ops.estimate_normals per scan)")
    require_gpu_tensor(scan_normals, "scan_normals", F32)
    if isinstance(scan, torch.Tensor) and (tuple(scan_normals.shape) != tuple(scan.shape) or scan_normals.device != scan.device):
        raise _lib.PointNetHipError(f"{what}: scan_normals must be {tuple(scan.shape)} fp32 on {scan.device}, got {tuple(scan_normals.shape)} on "
                                    f"{scan_normals.device}")
    return float(eps)


def icp_gicp_sums(scan, labels, scan_normals, ref: IcpReference, pose, max_dist=float("inf"), eps: float = 1e-3):
    """One pass of plane-to-plane (generalized) semantic_icp at the fp64 pose (B,4,4) (spec: include/pointnet_hip.h,
    pn_icp_gicp_sums): the search of icp_correspond at the pose's fp32 rounding, then every kept pair's terms from the partner's
    normal (``ref.normals``) and the scan point's own (``scan_normals`` (B,N,3) fp32, in the scan's frame; sign and length do not
    matter) -> (idx (B,N) int32 and d2 (B,N), bit for bit icp_correspond's, and the (B,29) fp64 sums of the pairs whose two normals
    are finite and not zero, in icp_plane_sums' layout).  ops.icp_plane_solve is the solve.  An IcpGridReference is searched
    through its grid, as in icp_correspond."""
    what = "icp_gicp_sums"
    _family(what, ref)
    eps = _gicp_options(what, scan, ref, scan_normals, eps)
    ref._serves(what, max_dist, plane=True)
    B, N, ws, nbytes = _icp_inputs(scan, labels, ref, what, True, ref._GICP[2])
    require_gpu_tensor(pose, "pose", torch.float64)
    if tuple(pose.shape) != (B, 4, 4):
        raise _lib.PointNetHipError(f"{what}: pose must be ({B},4,4), got {tuple(pose.shape)}")
    dev = scan.device
    pose32 = pose.float()
    idx = torch.empty(B, N, device=dev, dtype=torch.int32)
    d2 = torch.empty(B, N, device=dev, dtype=F32)
    so = torch.empty(B, 29, device=dev, dtype=torch.float64)
    name = ref._GICP[0]
    check(getattr(lib(), name)(ptr(scan), ptr(labels), ptr(scan_normals), B, N, ptr(ref._prim), ref._seg_c, ref.M, ref.n_parts,
                               ptr(ref.normals), ptr(pose32), ptr(pose), _max_d2(max_dist), eps, ptr(idx), ptr(d2), ptr(so), ptr(ws), nbytes,
                               *ref._gicp_tail(), current_stream()), name)
    return idx, d2, so


ROBUST_KERNELS = {None: 0, "huber": 1, "cauchy": 2, "tukey": 3}
ROBUST_TUNE = {None: 1.0, "huber": 1.345, "cauchy": 2.385, "tukey": 4.685}     # 95 % efficiency on Gaussian residuals


def _robust_options(what, scan, weights, robust, robust_scale, robust_tune, robust_min_scale):
    """The option set the robust ICP entries share -> (kernel, scale (0.0: automatic), tune, min_scale, weights or None).  A
    value the library refuses (a scale < 0, a tune or min_scale <= 0) is passed on to it: it reports the error."""
    if robust not in ROBUST_KERNELS:
        raise _lib.PointNetHipError(f"{what}: robust must be None, 'huber', 'cauchy' or 'tukey', got {robust!r}")
    if isinstance(robust_scale, str):
        if robust_scale != "mad":
            raise _lib.PointNetHipError(f"{what}: robust_scale must be 'mad' or a scale in metres > 0, got {robust_scale!r}")
        scale = 0.0
    else:
        scale = float(robust_scale)
        if scale == 0.0:
            raise _lib.PointNetHipError(f"{what}: robust_scale must be 'mad' or a scale in metres > 0, got {robust_scale!r}")
    tune = ROBUST_TUNE[robust] if robust_tune is None else float(robust_tune)
    if weights is not None:
        require_gpu_tensor(weights, "weights", F32)
        if tuple(weights.shape) != tuple(scan.shape[:2]) or weights.device != scan.device:
            raise _lib.PointNetHipError(f"{what}: weights must be {tuple(scan.shape[:2])} fp32 on {scan.device}, got {tuple(weights.shape)}")
    return ROBUST_KERNELS[robust], scale, tune, float(robust_min_scale), weights


def icp_robust_sums(scan, labels, ref, pose, max_dist=float("inf"), metric: str = "point", weights=None, robust=None,
                    robust_scale="mad", robust_tune=None, robust_min_scale=1e-4):
    """One pass of the robust, confidence-weighted semantic_icp at the fp64 poses ``pose`` (B,4,4) (spec: include/pointnet_hip.h,
    pn_icp_robust_sums): the search of icp_correspond / icp_mesh_correspond at the fp32 rounding of the pose, the scale of the
    robust kernel and every pair's weight -> (idx (B,N) int32, d2 (B,N) fp32, q (B,N,3) fp32: the partner, w (B,N) fp64: the
    pair's weight, scale (B,) fp64, sums (B,19) for metric "point" or (B,30) for "plane": the weighted sums and, last, the
    number of pairs with a positive weight).  ``ref``: an IcpReference or an IcpMeshReference; the options: see semantic_icp."""
    if metric not in ("point", "plane"):
        raise _lib.PointNetHipError(f"icp_robust_sums: metric must be 'point' or 'plane', got {metric!r}")
    _family("icp_robust_sums", ref)
    idx, d2, q, so, w, sc = _icp_pass("icp_robust_sums", scan, labels, ref, pose, max_dist, 2 if metric == "plane" else 1, torch.float64,
                                      want_q=True, robust=(weights, robust, robust_scale, robust_tune, robust_min_scale))
    return idx, d2, q, w, sc, so


def icp_robust_solve(sums: torch.Tensor, pose: torch.Tensor, metric: str = "point"):
    """The solve of the robust semantic_icp on given weighted sums, (B,19) for metric "point" or (B,30) for "plane" (spec:
    pn_icp_robust_solve); ``pose`` (B,4,4) fp64 is the previous pose, kept when fewer than 3 (6) pairs have a positive weight or
    the weights sum to nothing -> (new pose, rmse (B,) fp64: the weighted root mean square, status (B,) int32)."""
    if metric not in ("point", "plane"):
        raise _lib.PointNetHipError(f"icp_robust_solve: metric must be 'point' or 'plane', got {metric!r}")
    plane = metric == "plane"
    return _icp_solve("icp_robust_solve", 30 if plane else 19, sums, pose, 2 if plane else 1)


def semantic_icp(scan, labels, ref, init_pose, max_iters: int = 30, max_dist=float("inf"), tol_rot: float = 1e-6,
                 tol_t: float = 1e-6, metric: str = "point", *, weights=None, robust=None, robust_scale="mad", robust_tune=None,
                 robust_min_scale=1e-4, return_scale: bool = False, scan_normals=None, gicp_eps: float = 1e-3):
    """Label-constrained ICP of the reference against every scan (spec: include/pointnet_hip.h, pn_semantic_icp and
    pn_semantic_icp_plane): scan (B,N,3) fp32, labels (B,N) int32 (part ids in the reference's label space; -1 or any other id
    outside [0, n_parts) takes no part), init_pose (B,4,4) -> (pose (B,4,4) fp64 with p_scan ~= R q_ref + t, rmse (B,) fp64,
    pairs (B,) int32, iters (B,) int32, status (B,) int32: PN_ICP_CONVERGED = 1 | PN_ICP_FEW_PAIRS = 2 | PN_ICP_DEGENERATE = 4).
    ``metric``: "point" (point to point, Kabsch) or "plane" (point to plane against ``ref.normals``, which it requires; rmse is
    then the point-to-plane residual).  ``ref`` may be an IcpMeshReference (ops.icp_mesh_reference): the partner is then the
    exact closest point on the triangles of the scan point's label (pn_semantic_icp_mesh), and "plane" uses the winning
    triangle's face normal; outputs and status bits are the same.  An IcpBvhMeshReference (icp_mesh_reference(accel="bvh"))
    gives the same bits through its trees (pn_semantic_icp_bvh); the robust loop refuses it.  An IcpGridReference
    (icp_reference(accel="grid", max_dist=...)) gives the same pose, rmse, pairs, iters and status through its voxel grid
    (pn_semantic_icp_grid) at any ``max_dist`` up to the reference's (the default inf is refused); the robust loop refuses it too.
    A fixed launch sequence on the current stream, no host synchronisation: capturable into
    a CUDA graph.
    Robust, confidence-weighted loop (spec: pn_semantic_icp_robust), for labels that may be wrong: ``robust`` = "huber", "cauchy"
    or "tukey" weights every pair by that kernel of its distance over a scale c; ``robust_scale`` = "mad" (c = robust_tune *
    1.4826 * sqrt(lower median of the kept pairs' d2), at least ``robust_min_scale`` metres, per scan and iteration) or a fixed c
    in metres; ``robust_tune`` defaults to 1.345 / 2.385 / 4.685; ``weights`` (B,N) fp32 multiplies every point's pair (e.g. the
    confidence PointNet.predict_scan returns; negative, NaN or infinite counts as 0).  pairs is then the number of pairs with a
    positive weight and rmse the weighted root mean square; ``return_scale`` appends scale (B,) fp64, the last c of every scan
    (NaN without a robust kernel).  With ``weights`` None and ``robust`` None the call is the unweighted one above.
    ``metric`` = "gicp": plane to plane (generalized ICP; spec: pn_semantic_icp_gicp), for scan against scan.  A pair's residual
    is weighted by both surfaces' local covariance, from ``ref.normals`` and ``scan_normals`` (B,N,3) fp32, the scans' own normals
    in their own frame (ops.estimate_normals per scan; a NaN or zero row takes no part; sign and length do not matter);
    ``gicp_eps`` in (0, 1] is the covariance along the normal relative to the surface's (1 makes it point to point).  It takes a
    cloud reference, plain or with a grid, and neither ``robust`` nor ``weights``; rmse = sqrt(sum d^T W d / pairs), in metres."""
    if metric not in ("point", "plane", "gicp"):
        raise _lib.PointNetHipError(f"semantic_icp: metric must be 'point', 'plane' or 'gicp', got {metric!r}")
    if robust not in ROBUST_KERNELS:
        raise _lib.PointNetHipError(f"semantic_icp: robust must be None, 'huber', 'cauchy' or 'tukey', got {robust!r}")
    _family("semantic_icp", ref)
    gicp = metric == "gicp"
    plane = metric == "plane" or gicp
    weighted = weights is not None or robust is not None
    if gicp:
        if weighted:
            raise _lib.PointNetHipError("semantic_icp: metric 'gicp' takes neither robust= nor weights=")
        gicp_eps = _gicp_options("semantic_icp", scan, ref, scan_normals, gicp_eps)
    elif scan_normals is not None:
        raise _lib.PointNetHipError(f"semantic_icp: scan_normals goes with metric 'gicp'; metric {metric!r} does not read it")
    ref._serves("semantic_icp", max_dist, plane, weighted)
    sizer = "pn_icp_robust_workspace_bytes" if weighted else ref._GICP[2] if gicp else ref._SIZER[plane]
    B, N, ws, nbytes = _icp_inputs(scan, labels, ref, "semantic_icp", plane, sizer)
    if not isinstance(init_pose, torch.Tensor) or tuple(init_pose.shape) != (B, 4, 4) or init_pose.device != scan.device:
        raise _lib.PointNetHipError(f"semantic_icp: init_pose must be a ({B},4,4) tensor on {scan.device}")
    dev = scan.device
    pose = init_pose.to(torch.float64).contiguous().clone()
    rmse = torch.empty(B, device=dev, dtype=torch.float64)
    pairs = torch.empty(B, device=dev, dtype=torch.int32)
    iters = torch.empty(B, device=dev, dtype=torch.int32)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    sc = None
    head = (ptr(scan), ptr(labels), B, N, ptr(ref._prim), ref._seg_c, ref.M, ref.n_parts)
    run = (ptr(pose), int(max_iters), _max_d2(max_dist), float(tol_rot), float(tol_t))
    out = (ptr(pose), ptr(rmse), ptr(pairs), ptr(iters), ptr(status))
    name = "pn_semantic_icp_robust" if weighted else ref._GICP[1] if gicp else ref._LOOP[plane]
    if gicp:
        if return_scale:
            raise _lib.PointNetHipError("semantic_icp: return_scale goes with robust= or weights=; the plane-to-plane loop has no scale")
        check(getattr(lib(), name)(ptr(scan), ptr(labels), ptr(scan_normals), *head[2:], ptr(ref.normals), *run, gicp_eps, *out, ptr(ws),
                                   nbytes, *ref._gicp_tail(), current_stream()), name)
        return pose, rmse, pairs, iters, status
    if weighted:
        *opts, weights = _robust_options("semantic_icp", scan, weights, robust, robust_scale, robust_tune, robust_min_scale)
        sc = torch.empty(B, device=dev, dtype=torch.float64)
        args = (ref._IS_MESH, ptr(ref.normals) if plane else None, 2 if plane else 1, *run, *opts, ptr(weights), *out, ptr(sc), ptr(ws), nbytes)
    elif return_scale:
        raise _lib.PointNetHipError("semantic_icp: return_scale goes with robust= or weights=; the unweighted loop has no scale")
    elif ref._LEGACY:
        args = (*run, *((ptr(ref.normals),) if plane else ()), *out, ptr(ws), nbytes)
    else:
        args = (ptr(ref._entry_normals(plane)), 2 if plane else 1, *run, *out, ptr(ws), nbytes, *ref._tail())
    check(getattr(lib(), name)(*head, *args, current_stream()), name)
    return (pose, rmse, pairs, iters, status, sc) if weighted and return_scale else (pose, rmse, pairs, iters, status)


def _lidar_mesh(ref, what, area=False, trees=False):
    """the mesh a caster or sampler is handed: its triangles, and the area or the trees where the call reads them -> its device"""
    _family(what, ref, IcpMeshReference, "mesh_ref", "ops.icp_mesh_reference")
    return ref._check(what, name="mesh_ref", normals=False, area=area, trees=trees)


def _lidar_dirs(dirs, dev, what):
    import numpy as np
    d = dirs if isinstance(dirs, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(dirs, np.float32)))
    d = d.to(device=dev, dtype=F32).contiguous()
    if d.dim() != 2 or d.shape[1] != 3 or d.shape[0] < 1:
        raise _lib.PointNetHipError(f"{what}: dirs must be (R, 3) with R >= 1, got {tuple(d.shape)}")
    return d


def lidar_cast(mesh_ref: IcpMeshReference, poses, dirs, t_min: float = 0.0, t_max: float = float("inf"), accel=None):
    """Cast the ray grid ``dirs`` (R, 3) (sensor frame, e.g. pointcloud.pinhole_rays) from the sensor origin of each of the B
    model-in-sensor poses (B, 4, 4) (fp64 or fp32, tensor or array; p_sensor = R q_model + t, rounded to fp32 element by element)
    against the triangles of ``mesh_ref`` (spec: include/pointnet_hip.h, pn_lidar_cast) -> (hit (B, R) int32: the row in
    mesh_ref.tri of the first triangle hit or -1, t (B, R) fp32: the ray parameter of that hit, the range in metres for unit dirs,
    or +inf).  Hits with t outside [t_min, t_max] do not count.  One launch, no synchronisation: capturable.  ``accel`` = None
    tests every ray against every triangle (pn_lidar_cast), whatever the reference's type; "bvh" walks the trees of an
    IcpBvhMeshReference (icp_mesh_reference(..., accel="bvh"); pn_lidar_cast_bvh) and returns the same bits at a cost that no
    longer grows with the triangle count: the choice for meshes of tens of thousands of triangles."""
    import numpy as np
    if accel not in (None, "bvh"):
        raise _lib.PointNetHipError(f"lidar_cast: accel must be None or 'bvh', got {accel!r}")
    dev = _lidar_mesh(mesh_ref, "lidar_cast", trees=accel == "bvh")
    p = poses if isinstance(poses, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(poses)))
    if p.dim() != 3 or tuple(p.shape[1:]) != (4, 4) or p.shape[0] < 1 or p.dtype not in (F32, torch.float64):
        raise _lib.PointNetHipError(f"lidar_cast: poses must be (B, 4, 4) fp32 or fp64 with B >= 1, got {tuple(p.shape)} {p.dtype}")
    p = p.to(device=dev, dtype=F32).contiguous()
    d = _lidar_dirs(dirs, dev, "lidar_cast")
    B, R = p.shape[0], d.shape[0]
    hit = torch.empty(B, R, device=dev, dtype=torch.int32)
    t = torch.empty(B, R, device=dev, dtype=F32)
    name, tail = ("pn_lidar_cast_bvh", mesh_ref._tail()) if accel == "bvh" else ("pn_lidar_cast", ())
    check(getattr(lib(), name)(ptr(mesh_ref.tri), mesh_ref._seg_c, mesh_ref.T, mesh_ref.n_parts, ptr(p), B, ptr(d), R, float(t_min),
                               float(t_max), ptr(hit), ptr(t), *tail, current_stream()), name)
    return hit, t


def lidar_pack(mesh_ref: IcpMeshReference, hit, t, dirs, n: int):
    """The returns of lidar_cast as clouds of ``n`` labelled points per frame (spec: include/pointnet_hip.h, pn_lidar_pack) ->
    (xyz (B, n, 3) fp32 in the sensor frame, part (B, n) int32: the part label of the triangle hit, ray (B, n) int32: the index
    into ``dirs`` each point came from, count (B,) int32: the frame's hits).  A frame with more than n hits keeps an even stride
    of them, one with fewer repeats them cyclically, one with none is NaN / -1 / -1.  Three launches, no synchronisation."""
    dev = _lidar_mesh(mesh_ref, "lidar_pack")
    require_gpu_tensor(hit, "hit", torch.int32)
    require_gpu_tensor(t, "t", F32)
    d = _lidar_dirs(dirs, dev, "lidar_pack")
    if hit.dim() != 2 or tuple(t.shape) != tuple(hit.shape) or hit.shape[1] != d.shape[0] or hit.device != dev or t.device != dev:
        raise _lib.PointNetHipError(f"lidar_pack: hit and t must be (B, {d.shape[0]}) on {dev}, got {tuple(hit.shape)} / {tuple(t.shape)}")
    B, R = hit.shape
    n = int(n)
    nbytes = lib().pn_lidar_workspace_bytes(B, R)
    ws = torch.empty(max(nbytes, 1), device=dev, dtype=torch.uint8)
    xyz = torch.empty(B, max(n, 0), 3, device=dev, dtype=F32)
    part = torch.empty(B, max(n, 0), device=dev, dtype=torch.int32)
    ray = torch.empty(B, max(n, 0), device=dev, dtype=torch.int32)
    count = torch.empty(B, device=dev, dtype=torch.int32)
    check(lib().pn_lidar_pack(ptr(hit), ptr(t), ptr(d), B, R, mesh_ref._seg_c, mesh_ref.T, mesh_ref.n_parts, n, ptr(xyz), ptr(part),
                              ptr(ray), ptr(count), ptr(ws), nbytes, current_stream()), "pn_lidar_pack")
    return xyz, part, ray, count


_SENSOR_KEYS = ("range_sigma", "detection", "max_incidence_deg", "mixed")


def _lidar_sensor(what, range_sigma, detection, max_incidence_deg, mixed):
    """the sensor model's keywords as pn_lidar_sense's seven doubles (sigma0, sigma1, strength, range_ref, min_cos2, jump, p_mix);
    the shapes and the keys are checked here, the values by the library, except those the host transforms"""
    import math
    try:
        s0, s1 = (float(v) for v in range_sigma)
    except (TypeError, ValueError):
        raise _lib.PointNetHipError(f"{what}: range_sigma must be two numbers (metres, metres per metre), got {range_sigma!r}") from None
    strength, range_ref, jump, prob, min_cos2 = float("inf"), 1.0, 0.0, 0.0, 0.0
    if detection is not None:
        if not isinstance(detection, dict) or set(detection) != {"strength", "range_ref"}:
            raise _lib.PointNetHipError(f"{what}: detection must be None or dict(strength=, range_ref=), got {detection!r}")
        strength, range_ref = float(detection["strength"]), float(detection["range_ref"])
    if mixed is not None:
        if not isinstance(mixed, dict) or set(mixed) != {"jump", "prob"}:
            raise _lib.PointNetHipError(f"{what}: mixed must be None or dict(jump=, prob=), got {mixed!r}")
        jump, prob = float(mixed["jump"]), float(mixed["prob"])
        if not 0.0 <= prob <= 1.0:
            raise _lib.PointNetHipError(f"{what}: mixed prob={prob} outside [0, 1]")
    if max_incidence_deg is not None:
        ang = float(max_incidence_deg)
        if not 0.0 <= ang <= 90.0:
            raise _lib.PointNetHipError(f"{what}: max_incidence_deg={ang} outside [0, 90]")
        min_cos2 = math.cos(math.radians(ang)) ** 2
    return s0, s1, strength, range_ref, min_cos2, jump, prob


def _lidar_shape(what, shape, dirs):
    """the raster (H, W) of the ray grid ``dirs`` (R, 3); checked on the host, before anything touches the device"""
    try:
        H, W = (int(v) for v in shape)
    except (TypeError, ValueError):
        raise _lib.PointNetHipError(f"{what}: shape must be (H, W), got {shape!r}") from None
    import numpy as np
    ds = tuple(dirs.shape) if hasattr(dirs, "shape") else np.shape(dirs)
    if H < 1 or W < 1 or len(ds) != 2 or H * W != ds[0]:
        raise _lib.PointNetHipError(f"{what}: shape {H} x {W} does not match dirs {ds}: H * W rays required")
    return H, W


def lidar_sense(mesh_ref: IcpMeshReference, poses, dirs, hit, t, shape, seed: int = 0, frame0: int = 0, range_sigma=(0.0, 0.0),
                detection=None, max_incidence_deg=None, mixed=None):
    """The sensor model between lidar_cast and lidar_pack (spec: include/pointnet_hip.h, pn_lidar_sense): the ideal returns
    ``hit``, ``t`` (B, R) of lidar_cast(mesh_ref, poses, dirs) as a flash LiDAR reports them -> (hit (B, R) int32, t (B, R) fp32,
    which lidar_pack takes, kind (B, R) uint8: pointcloud.LIDAR_KINDS).  ``shape`` = (H, W) is the raster of ``dirs`` (ray
    r * W + c is pixel (r, c), the layout of pointcloud.pinhole_rays).  ``range_sigma`` = (metres, metres per metre of range): the
    standard deviation of the range noise, a sum of four uniforms.  ``detection`` = dict(strength=, range_ref=): a return is kept
    with probability strength * cos(incidence) * (range_ref / range)^2, so strength is the margin at normal incidence at range_ref.
    ``max_incidence_deg``: returns at a larger angle between ray and face normal are lost.  ``mixed`` = dict(jump=, prob=): a return
    whose range differs by more than ``jump`` from a 4-neighbour's in the image lands, with probability ``prob``, somewhere between
    the two surfaces; it keeps its own part label.  A stage left at its default is off; with all off the returns come back
    unchanged.  The draws are a pure function of (``seed``, frame index, ray): frame b of a call with ``frame0`` = s is frame 0 of
    a call with ``frame0`` = s + b.  ``seed`` is taken modulo 2^64.  One launch, no synchronisation: capturable."""
    import numpy as np
    model = _lidar_sensor("lidar_sense", range_sigma, detection, max_incidence_deg, mixed)
    H, W = _lidar_shape("lidar_sense", shape, dirs)
    dev = _lidar_mesh(mesh_ref, "lidar_sense")
    d = _lidar_dirs(dirs, dev, "lidar_sense")
    p = poses if isinstance(poses, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(poses)))
    if p.dim() != 3 or tuple(p.shape[1:]) != (4, 4) or p.shape[0] < 1 or p.dtype not in (F32, torch.float64):
        raise _lib.PointNetHipError(f"lidar_sense: poses must be (B, 4, 4) fp32 or fp64 with B >= 1, got {tuple(p.shape)} {p.dtype}")
    p = p.to(device=dev, dtype=F32).contiguous()
    require_gpu_tensor(hit, "hit", torch.int32)
    require_gpu_tensor(t, "t", F32)
    B, R = p.shape[0], d.shape[0]
    if tuple(hit.shape) != (B, R) or tuple(t.shape) != (B, R) or hit.device != dev or t.device != dev:
        raise _lib.PointNetHipError(f"lidar_sense: hit and t must be ({B}, {R}) on {dev}, got {tuple(hit.shape)} / {tuple(t.shape)}")
    hit_out = torch.empty(B, R, device=dev, dtype=torch.int32)
    t_out = torch.empty(B, R, device=dev, dtype=F32)
    kind = torch.empty(B, R, device=dev, dtype=torch.uint8)
    check(lib().pn_lidar_sense(ptr(mesh_ref.tri), mesh_ref.T, ptr(p), B, ptr(d), H, W, ptr(hit), ptr(t), int(seed) & 0xFFFFFFFFFFFFFFFF,
                               int(frame0), *model, ptr(hit_out), ptr(t_out), ptr(kind), current_stream()), "pn_lidar_sense")
    return hit_out, t_out, kind


def lidar_frames(mesh_ref: IcpMeshReference, poses, dirs, n: int, t_min: float = 0.0, t_max: float = float("inf"), accel=None,
                 sensor=None, seed: int = 0, frame0: int = 0):
    """lidar_cast then lidar_pack: B labelled frames of ``n`` points each, as PointCloudSet.add_data, PointNet.predict_scan and
    semantic_icp take them -> (xyz (B, n, 3), part (B, n), ray (B, n), count (B,)).  ``accel`` is lidar_cast's.  ``sensor`` = a dict
    of lidar_sense's model keywords (range_sigma, detection, max_incidence_deg, mixed) and ``shape``: lidar_sense runs between
    the two with ``seed`` and ``frame0``, and a fifth value follows, kind (B, n) uint8: the kind of the ray each point came from
    (pointcloud.LIDAR_KINDS; 0 where ray is -1)."""
    if sensor is not None:
        if not isinstance(sensor, dict) or "shape" not in sensor or not set(sensor) <= set(_SENSOR_KEYS) | {"shape"}:
            raise _lib.PointNetHipError(f"lidar_frames: sensor must be None or a dict with shape=(H, W) and any of {', '.join(_SENSOR_KEYS)}, "
                                        f"got {sensor!r}")
        _lidar_sensor("lidar_frames", *(sensor.get(k, (0.0, 0.0) if k == "range_sigma" else None) for k in _SENSOR_KEYS))
        _lidar_shape("lidar_frames", sensor["shape"], dirs)
    dev = _lidar_mesh(mesh_ref, "lidar_frames")
    d = _lidar_dirs(dirs, dev, "lidar_frames")
    hit, t = lidar_cast(mesh_ref, poses, d, t_min, t_max, accel=accel)
    if sensor is None:
        return lidar_pack(mesh_ref, hit, t, d, n)
    hit, t, kind = lidar_sense(mesh_ref, poses, d, hit, t, seed=seed, frame0=frame0, **sensor)
    xyz, part, ray, count = lidar_pack(mesh_ref, hit, t, d, n)
    pk = torch.where(ray >= 0, torch.gather(kind, 1, ray.clamp(min=0).long()), torch.zeros((), device=dev, dtype=torch.uint8))
    return xyz, part, ray, count, pk


def mesh_sample(mesh_ref: IcpMeshReference, n: int, seed: int = 0, sets: int = 1, set0: int = 0):
    """``sets`` independent sets of ``n`` area-uniform surface samples of ``mesh_ref`` (spec: include/pointnet_hip.h,
    pn_mesh_sample) -> (xyz (sets, n, 3) fp32 in the model frame, part (sets, n) int32: the part label, row (sets, n) int32: the
    row in mesh_ref.tri the point lies on).  A set comes out in ascending row order, so grouped by part.  The draw is a pure
    function of (mesh, n, seed, set index): set b of a call with ``set0`` = s is set 0 of a call with ``set0`` = s + b.  ``seed`` is
    taken modulo 2^64.  Four launches, no synchronisation: capturable."""
    dev = _lidar_mesh(mesh_ref, "mesh_sample", area=True)
    n, sets, set0 = int(n), int(sets), int(set0)
    nbytes = lib().pn_mesh_sample_workspace_bytes(mesh_ref.T, sets, n)
    ws = torch.empty(max(nbytes, 1), device=dev, dtype=torch.uint8)
    xyz = torch.empty(max(sets, 0), max(n, 0), 3, device=dev, dtype=F32)
    part = torch.empty(max(sets, 0), max(n, 0), device=dev, dtype=torch.int32)
    row = torch.empty(max(sets, 0), max(n, 0), device=dev, dtype=torch.int32)
    check(lib().pn_mesh_sample(ptr(mesh_ref.tri), ptr(mesh_ref.area), mesh_ref._seg_c, mesh_ref.T, mesh_ref.n_parts,
                               int(seed) & 0xFFFFFFFFFFFFFFFF, set0, sets, n, ptr(xyz), ptr(row), ptr(part), ptr(ws), nbytes,
                               current_stream()), "pn_mesh_sample")
    return xyz, part, row


def mesh_sample_reference(mesh_ref: IcpMeshReference, n: int, seed: int = 0, accel=None, max_dist=None) -> IcpReference:
    """A labelled reference cloud with normals from the mesh alone: set 0 of mesh_sample(mesh_ref, n, seed) as an IcpReference.
    The samples are already grouped by part, so ``seg`` is counted from their labels; ``index`` (n,) int64 is the row in
    mesh_ref.tri each point lies on and ``normals`` the face normal of that row, so the cloud serves semantic_icp(metric="plane")
    and global_pose(score_cloud=...) directly.  A set-up call like icp_reference: it reads the part counts back once.  ``accel`` =
    "grid" with ``max_dist``: as in icp_reference, the same cloud as an IcpGridReference."""
    _grid_request("mesh_sample_reference", accel, max_dist)
    xyz, part, row = mesh_sample(mesh_ref, n, seed)
    require_gpu_tensor(mesh_ref.normals, "mesh_ref.normals", F32)
    row = row[0].long()
    cnt = torch.bincount(part[0].clamp(min=-1) + 1, minlength=mesh_ref.n_parts + 1)[1:].cpu()      # label -1: a mesh without area
    seg = [0] + torch.cumsum(cnt, 0).tolist()
    ref = IcpReference(xyz[0, :seg[-1]].contiguous(), seg, row[:seg[-1]], mesh_ref.n_parts,
                       normals=mesh_ref.normals[row[:seg[-1]]].contiguous())
    return ref if accel is None else _with_grid("mesh_sample_reference", ref, max_dist)


def _scan_reference(what, target, max_dist, metric, normals_radius, normals_k, viewpoint, accel):
    """the reference ops.register_scans registers against: the finite rows of ``target`` as one part, with ops.estimate_normals'
    normals for the plane and gicp metrics and the voxel grid for accel="grid" """
    rows = _finite_rows(target)
    if rows.numel() < 1:
        raise _lib.PointNetHipError(f"{what}: target has no finite point")
    pts, _, _ = _compact(target, rows, (0.0, 0.0, 0.0))
    normals = None
    if metric in ("plane", "gicp"):
        normals = estimate_normals(pts, float(max_dist if normals_radius is None else normals_radius), int(normals_k), viewpoint)[0]
    ref = IcpReference(pts, (0, pts.shape[0]), rows, 1, normals=normals)
    return _with_grid(what, ref, max_dist) if accel == "grid" else ref


def _source_normals(what, source, source_normals, radius, k, viewpoint):
    """the scans' own normals for the gicp metric, (B, N, 3) fp32: the caller's, or ops.estimate_normals of every scan (a row
    without a valid normal is NaN and takes no part)"""
    if source_normals is None:
        return torch.stack([estimate_normals(s, float(radius), int(k), viewpoint)[0] for s in source])
    require_gpu_tensor(source_normals, "source_normals", F32)
    if source_normals.dim() == 2:
        source_normals = source_normals.unsqueeze(0)
    if tuple(source_normals.shape) != tuple(source.shape) or source_normals.device != source.device:
        raise _lib.PointNetHipError(f"{what}: source_normals must be {tuple(source.shape)} fp32 on {source.device}, got "
                                    f"{tuple(source_normals.shape)} on {source_normals.device}")
    return source_normals


def register_scans(source, target, max_dist, init_pose=None, metric: str = "plane", normals_radius=None, normals_k: int = 8,
                   viewpoint=None, accel="grid", init=None, feature_radius=None, hypotheses: int = 4096, keep: int = 32, top: int = 4,
                   mutual: bool = False, seed: int = 0, source_viewpoint=None, source_normals=None, **icp):
    """Unlabelled scan-to-scan registration: the pose of every ``source`` scan (B, N, 3) or (N, 3) fp32 against the ``target``
    scan (M, 3) fp32 on the same device -> (pose (B,4,4) fp64 with p_source ~= R q_target + t, rmse (B,), pairs (B,), iters (B,),
    status (B,)): ops.semantic_icp with one part and zero labels, the target as the reference.  Target rows with a non-finite
    coordinate (a sensor's no-return pixels) are dropped first; non-finite source rows take no part.  ``max_dist`` (positive,
    finite) bounds a pair's distance.  ``metric`` "plane" (default) takes the target's normals from ops.estimate_normals(target,
    normals_radius or max_dist, normals_k, viewpoint); a target point without a valid normal (NaN) takes no part in the plane
    terms.  ``metric`` "gicp" (plane to plane, generalized ICP: semantic_icp(metric="gicp")) takes the target's normals the same
    way and the source's from ops.estimate_normals of every source scan at the same radius and ``normals_k`` (turned to
    ``source_viewpoint``, default ``viewpoint``; the metric does not depend on a normal's sign), or from ``source_normals`` (B,N,3)
    or (N,3) fp32 in the source's frame; rows without a valid normal on either side take no part; ``gicp_eps`` reaches the loop.
    ``init_pose`` (B,4,4) or (4,4), default the identity.  ``accel`` = "grid" (default) searches the target through a voxel
    grid (icp_reference(accel="grid")); None runs the brute-force entries on the same reference and returns the same bits, at a
    cost of N * M distances per iteration.  ``icp``: max_iters, tol_rot, tol_t.  ``init`` = "global" finds the start itself
    (ops.global_register with ``feature_radius``, ``hypotheses``, ``keep``, ``top``, ``mutual``, ``seed``; two more values follow,
    cost (B,) fp64 and winner (B,) int32) and excludes ``init_pose``; ``viewpoint`` then turns the target's normals and
    ``source_viewpoint`` (default: ``viewpoint``) the source's, each in its own scan's frame: the descriptors agree only when both
    clouds' normals are turned consistently.  The default None is the local solver alone."""
    import math
    if init not in (None, "global"):
        raise _lib.PointNetHipError(f"register_scans: init must be None or 'global', got {init!r}")
    if init == "global":
        if init_pose is not None:
            raise _lib.PointNetHipError("register_scans: init='global' computes the start; init_pose must be None")
        if feature_radius is None:
            raise _lib.PointNetHipError("register_scans: init='global' needs feature_radius=")
        return global_register(source, target, feature_radius, max_dist, normals_radius=normals_radius, viewpoint=viewpoint,
                               hypotheses=hypotheses, keep=keep, top=top, mutual=mutual, seed=seed, source_viewpoint=source_viewpoint,
                               metric=metric, normals_k=normals_k, accel=accel, source_normals=source_normals, **icp)
    if metric not in ("point", "plane", "gicp"):
        raise _lib.PointNetHipError(f"register_scans: metric must be 'point', 'plane' or 'gicp', got {metric!r}")
    if source_normals is not None and metric != "gicp":
        raise _lib.PointNetHipError(f"register_scans: source_normals goes with metric 'gicp'; metric {metric!r} does not read it")
    if accel not in (None, "grid"):
        raise _lib.PointNetHipError(f"register_scans: accel must be None or 'grid', got {accel!r}")
    if max_dist is None or not math.isfinite(float(max_dist)) or not float(max_dist) > 0.0:
        raise _lib.PointNetHipError(f"register_scans: max_dist={max_dist} must be finite and > 0")
    for key in icp:
        if key not in ("max_iters", "tol_rot", "tol_t") and not (key == "gicp_eps" and metric == "gicp"):
            raise _lib.PointNetHipError(f"register_scans: {key}= is not an argument (max_iters, tol_rot and tol_t reach the loop)")
    require_gpu_tensor(source, "source", F32)
    require_gpu_tensor(target, "target", F32)
    if source.dim() == 2:
        source = source.unsqueeze(0)
    if source.dim() != 3 or source.shape[2] != 3 or target.dim() != 2 or target.shape[1] != 3 or target.device != source.device:
        raise _lib.PointNetHipError(f"register_scans: source (B,N,3) or (N,3) and target (M,3) on one device expected, got "
                                    f"{tuple(source.shape)} / {tuple(target.shape)}")
    B, N, _ = source.shape
    dev = source.device
    ref = _scan_reference("register_scans", target, max_dist, metric, normals_radius, normals_k, viewpoint, accel)
    if init_pose is None:
        init_pose = torch.eye(4, device=dev, dtype=torch.float64).expand(B, 4, 4)
    elif isinstance(init_pose, torch.Tensor) and init_pose.dim() == 2:
        init_pose = init_pose.unsqueeze(0).expand(B, 4, 4)
    labels = torch.zeros(B, N, device=dev, dtype=torch.int32)
    if metric == "gicp":
        icp = dict(icp, scan_normals=_source_normals("register_scans", source, source_normals, max_dist if normals_radius is None else normals_radius,
                                                     normals_k, viewpoint if source_viewpoint is None else source_viewpoint))
    return semantic_icp(source, labels, ref, init_pose, max_dist=max_dist, metric=metric, **icp)


def rotation_grid(n: int):
    """``n`` near-uniform rotations (n, 3, 3) fp64 on the host: the super-Fibonacci spiral on the unit quaternions.  With
    s = i + 1/2, r = sqrt(s / n), R = sqrt(1 - s / n), alpha = 2 pi s / sqrt(2), beta = 2 pi s / 1.533751168755204288118041, the
    quaternion (x, y, z, w) = (r sin alpha, r cos alpha, R sin beta, R cos beta), converted to a rotation matrix."""
    import math
    n = int(n)
    if n < 1:
        raise _lib.PointNetHipError(f"rotation_grid: n={n} must be >= 1")
    s = torch.arange(n, dtype=torch.float64) + 0.5
    r, R = torch.sqrt(s / n), torch.sqrt(1.0 - s / n)
    al, be = 2.0 * math.pi * s / math.sqrt(2.0), 2.0 * math.pi * s / 1.533751168755204288118041
    x, y, z, w = r * torch.sin(al), r * torch.cos(al), R * torch.sin(be), R * torch.cos(be)
    rows = [1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
            2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
            2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]
    return torch.stack(rows, 1).reshape(n, 3, 3)


def part_moments(scan, labels, n_parts: int):
    """Per-part point counts and coordinate sums of labelled scans (spec: include/pointnet_hip.h, pn_part_moments): scan (B,N,3)
    fp32, labels (B,N) int32 -> (B, n_parts, 4) fp64, [n, sum x, sum y, sum z] over the points of every label in [0, n_parts)
    with three finite coordinates."""
    require_gpu_tensor(scan, "scan", F32)
    require_gpu_tensor(labels, "labels", torch.int32)
    if scan.dim() != 3 or scan.shape[2] != 3 or tuple(labels.shape) != tuple(scan.shape[:2]) or labels.device != scan.device:
        raise _lib.PointNetHipError(f"part_moments: scan (B,N,3) and labels (B,N) on one device expected, got {tuple(scan.shape)} / "
                                    f"{tuple(labels.shape)}")
    B, N, _ = scan.shape
    nbytes = lib().pn_part_moments_workspace_bytes(B, N)
    ws = torch.empty(max(nbytes, 1), device=scan.device, dtype=torch.uint8)
    out = torch.empty(B, max(int(n_parts), 0), 4, device=scan.device, dtype=torch.float64)
    check(lib().pn_part_moments(ptr(scan), ptr(labels), B, N, int(n_parts), ptr(out), ptr(ws), nbytes, current_stream()),
          "pn_part_moments")
    return out


def icp_part_moments(ref):
    """The (n_parts, 4) fp64 moments [w_l, sum w q] of a reference, as pn_icp_seed_poses takes them.  An IcpReference: the point
    count and coordinate sum of every part (pn_part_moments on the grouped cloud, the labels taken from ``seg``).  An
    IcpMeshReference: the area and the area-weighted sum of the triangle centroids of every part."""
    _family("icp_part_moments", ref, makers="ops.icp_reference or ops.icp_mesh_reference")
    return ref._part_moments()


def icp_seed_poses(moments, ref_moments, rotations=None):
    """Candidate poses of the global start (spec: include/pointnet_hip.h, pn_icp_seed_poses): moments (B, n_parts, 4) fp64 of
    the scans (ops.part_moments), ref_moments (n_parts, 4) fp64 of the reference (ops.icp_part_moments), rotations (K, 3, 3)
    fp64 or None (K = 0) -> (B, K + 1, 4, 4) fp64: pose k < K turns the reference by rotation k about the centroids of the shared
    labels, pose K is the rigid fit of the shared part centroids."""
    require_gpu_tensor(moments, "moments", torch.float64)
    require_gpu_tensor(ref_moments, "ref_moments", torch.float64)
    if moments.dim() != 3 or moments.shape[2] != 4 or tuple(ref_moments.shape) != (moments.shape[1], 4):
        raise _lib.PointNetHipError(f"icp_seed_poses: moments (B,n_parts,4) and ref_moments (n_parts,4) expected, got "
                                    f"{tuple(moments.shape)} / {tuple(ref_moments.shape)}")
    B, n_parts, _ = moments.shape
    K = 0
    if rotations is not None:
        require_gpu_tensor(rotations, "rotations", torch.float64)
        if rotations.dim() != 3 or tuple(rotations.shape[1:]) != (3, 3):
            raise _lib.PointNetHipError(f"icp_seed_poses: rotations must be (K,3,3), got {tuple(rotations.shape)}")
        K = rotations.shape[0]
    out = torch.empty(B, K + 1, 4, 4, device=moments.device, dtype=torch.float64)
    check(lib().pn_icp_seed_poses(ptr(moments), ptr(ref_moments), B, n_parts, ptr(rotations) if K else None, K, ptr(out),
                                  current_stream()), "pn_icp_seed_poses")
    return out


def icp_score_poses(scan, labels, ref, poses, max_dist, stride: int = 1):
    """Rank K candidate poses per scan by a truncated same-label nearest-neighbour cost (spec: include/pointnet_hip.h,
    pn_icp_score_poses): poses (B,K,4,4) fp64 -> (score (B,K,2) fp64: the number of sampled points within ``max_dist`` of the
    reference and the sum of min(d2, max_dist^2) over the sample, order (B,K) int32: the candidates by ascending (cost, k)).  The
    sample is every ``stride``-th of the scan's points that take part, in bucketed order.  A mesh reference is scored against
    its labelled vertex cloud.  One scoring launch for any K, no host synchronisation."""
    _family("icp_score_poses", ref)
    B, N, _, _ = _icp_inputs(scan, labels, ref, "icp_score_poses")
    require_gpu_tensor(poses, "poses", torch.float64)
    if poses.dim() != 4 or poses.shape[0] != B or tuple(poses.shape[2:]) != (4, 4) or poses.device != scan.device:
        raise _lib.PointNetHipError(f"icp_score_poses: poses must be ({B},K,4,4) on {scan.device}, got {tuple(poses.shape)}")
    K = poses.shape[1]
    xyz, seg_c, M = ref._score_cloud()
    nbytes = lib().pn_icp_score_workspace_bytes(B, N, K)
    ws = torch.empty(max(nbytes, 1), device=scan.device, dtype=torch.uint8)
    score = torch.empty(B, K, 2, device=scan.device, dtype=torch.float64)
    order = torch.empty(B, K, device=scan.device, dtype=torch.int32)
    check(lib().pn_icp_score_poses(ptr(scan), ptr(labels), B, N, ptr(xyz), seg_c, M, ref.n_parts, ptr(poses), K, int(stride),
                                   _max_d2(max_dist), ptr(score), ptr(order), ptr(ws), nbytes, current_stream()), "pn_icp_score_poses")
    return score, order


def global_pose(scan, labels, ref, max_dist, rotations=None, top: int = 4, stride: Optional[int] = None, score_cloud=None, **icp):
    """A pose for every labelled scan without a start: scored multi-start for semantic_icp.  The per-part moments of the scans
    (part_moments) and of the reference (icp_part_moments) give K + 1 seeds (icp_seed_poses; ``rotations`` (K,3,3) fp64, default
    rotation_grid(256)); icp_score_poses ranks them on every ``stride``-th point that takes part (default max(1, N // 8192)); the
    best ``top`` are refined by semantic_icp (``icp``: max_iters, tol_rot, tol_t, metric, robust and its options, not weights; ``ref`` and ``max_dist`` as given), the
    refined poses are scored again on every point that takes part, and the pose of lowest cost is kept (ties: the earlier
    candidate).  With an IcpMeshReference the coarse score runs against the labelled vertices and the final one is the sum of
    min(d2, max_dist^2) over icp_mesh_correspond's point-to-triangle d2; ``score_cloud`` (an IcpReference with the mesh's n_parts
    on the scans' device, e.g. ops.mesh_sample_reference) then replaces the vertices in the coarse score, which on a coarse mesh
    are a poor stand-in for the surface; seeds, refinement and the final selection are unchanged.  -> (pose (B,4,4) fp64, rmse (B,), pairs (B,), iters (B,),
    status (B,) of the kept refinement, cost (B,) fp64, winner (B,) int32: its index among the K + 1 seeds).  ``max_dist`` must be
    finite.  Every step runs on the device on the current stream; nothing is read back to the host."""
    import math
    if not math.isfinite(float(max_dist)) or not float(max_dist) > 0.0:
        raise _lib.PointNetHipError(f"global_pose: max_dist={max_dist} must be finite and > 0")
    if int(top) < 1:
        raise _lib.PointNetHipError(f"global_pose: top={top} must be >= 1")
    if "init_pose" in icp:
        raise _lib.PointNetHipError("global_pose: the start is what it computes; init_pose is not an argument")
    if icp.get("weights") is not None or icp.get("return_scale"):
        raise _lib.PointNetHipError("global_pose: weights and return_scale are not accepted (the refinement runs on repeated scans and "
                                    "the seed scorer is unweighted); robust= reaches the refinement")
    _family("global_pose", ref)
    B, N, _, _ = _icp_inputs(scan, labels, ref, "global_pose")
    dev = scan.device
    if score_cloud is not None:
        if not ref._IS_MESH:
            raise _lib.PointNetHipError("global_pose: score_cloud goes with an IcpMeshReference; a cloud reference is scored against itself")
        _family("global_pose", score_cloud, IcpReference, "score_cloud", "ops.icp_reference or ops.mesh_sample_reference")
        if score_cloud.n_parts != ref.n_parts or score_cloud.xyz.device != dev:
            raise _lib.PointNetHipError(f"global_pose: score_cloud must be an IcpReference with n_parts={ref.n_parts} on {dev}")
    rot = rotation_grid(256) if rotations is None else rotations
    rot = torch.as_tensor(rot, dtype=torch.float64).to(dev).contiguous()
    stride = max(1, N // 8192) if stride is None else int(stride)
    seeds = icp_seed_poses(part_moments(scan, labels, ref.n_parts), icp_part_moments(ref), rot)
    return _scored_multistart(scan, labels, ref, ref if score_cloud is None else score_cloud, seeds, top, stride, max_dist, icp)


def _scored_multistart(scan, labels, ref, coarse_ref, seeds, top, stride, max_dist, icp):
    """The tail ops.global_pose and ops.global_register share: seeds (B, K, 4, 4) fp64 are ranked by icp_score_poses against
    ``coarse_ref`` on every ``stride``-th point, the best ``top`` refined by semantic_icp(**icp) against ``ref``, the refined poses
    scored again on every point, and the pose of lowest cost kept (ties: the earlier candidate) -> semantic_icp's five values of the
    kept refinement, cost (B,) fp64, winner (B,) int32: its index among the seeds."""
    B, dev = scan.shape[0], scan.device
    K1 = seeds.shape[1]
    top = min(int(top), K1)
    _, order = icp_score_poses(scan, labels, coarse_ref, seeds, max_dist, stride)
    pick = order[:, :top].long()                                                           # (B, top) seed indices
    start = torch.gather(seeds, 1, pick[:, :, None, None].expand(B, top, 4, 4)).reshape(B * top, 4, 4)
    rs, rl = scan.repeat_interleave(top, 0), labels.repeat_interleave(top, 0)
    if icp.get("scan_normals") is not None:               # the plane-to-plane metric: the scans' normals are repeated beside them
        icp = dict(icp, scan_normals=icp["scan_normals"].repeat_interleave(top, 0))
    pose, rmse, pairs, iters, status = semantic_icp(rs, rl, ref, start, max_dist=max_dist, **icp)
    if ref._IS_MESH:                                      # a mesh's final score is the point-to-triangle one, not the vertices'
        _, d2, _ = icp_mesh_correspond(rs, rl, ref, pose)
        md = torch.tensor(_max_d2(max_dist), device=dev, dtype=F32)
        seg = torch.tensor(ref.seg, device=dev)
        full = torch.cat([seg[1:] > seg[:-1], torch.zeros(1, dtype=torch.bool, device=dev)])
        lab = rl.long()
        act = (lab >= 0) & (lab < ref.n_parts) & full[lab.clamp(0, ref.n_parts)] & torch.isfinite(rs).all(-1)
        fine = torch.where(act, torch.where(d2 <= md, d2, md).double(), torch.zeros((), device=dev, dtype=torch.float64)).sum(1)
        fine = fine.reshape(B, top)
        best = torch.sort(fine, dim=1, stable=True).indices[:, :1]
    else:
        score, forder = icp_score_poses(scan, labels, ref, pose.reshape(B, top, 4, 4), max_dist, 1)
        fine = score[:, :, 1]
        best = forder[:, :1].long()
    flat = (torch.arange(B, device=dev)[:, None] * top + best).reshape(B)
    return (pose[flat], rmse[flat], pairs[flat], iters[flat], status[flat], torch.gather(fine, 1, best).reshape(B),
            torch.gather(pick, 1, best).reshape(B).to(torch.int32))


def global_register(source, target, feature_radius, max_dist, normals_radius=None, k: int = 16, viewpoint=None, hypotheses: int = 4096,
                    keep: int = 32, top: int = 4, mutual: bool = False, seed: int = 0, edge_ratio: float = 0.9, source_viewpoint=None,
                    target_viewpoint=None, metric: str = "plane", normals_k: int = 8, accel="grid", stride: Optional[int] = None,
                    source_normals=None, **icp):
    """Unlabelled scan-to-scan registration without a start: FPFH descriptors, nearest-feature correspondences, RANSAC on
    three-correspondence hypotheses, then global_pose's scored refinement.  ``source`` (B, N, 3) or (N, 3) and ``target`` (M, 3)
    fp32 on one device.  For both clouds: finite rows -> estimate_normals(``normals_radius`` or ``feature_radius``, ``k``) ->
    fpfh(``feature_radius``, ``k``); feature_match(source -> target; ``mutual`` keeps a pair only when each is the other's nearest);
    ransac_poses on the matched pairs (``hypotheses``, ``edge_ratio``, ``seed``, inliers within ``max_dist``); the ``keep``
    hypotheses of highest count are ranked by icp_score_poses on every ``stride``-th source point (default max(1, N // 8192)), the
    best ``top`` refined by semantic_icp (``icp``: max_iters, tol_rot, tol_t) against the reference register_scans builds from the
    target (``metric``, ``normals_k``, ``accel``), scored again on every point, and the pose of lowest cost kept -> register_scans'
    five values, cost (B,) fp64 and winner (B,) int32: the kept hypothesis h.  With ``metric`` "gicp" the refinement is plane to
    plane; its source normals are register_scans' (``source_normals``, or ops.estimate_normals at ``normals_radius`` or ``max_dist``
    with ``normals_k``), not the descriptors'.
    The descriptors of the two clouds agree only when their normals are turned consistently: pass ``viewpoint`` when both scans
    were taken from one place, ``source_viewpoint`` / ``target_viewpoint`` (each in its own scan's frame) when they were not;
    without any, every normal's largest component is positive, which is consistent only for small rotations.  Limits: k <= 16, so
    the clouds should be voxel-downsampled until 16 neighbours span ``feature_radius``; a body with a symmetry has as many poses
    of equal cost, and the one returned is the first found.  An invalid hypothesis (count -1, NaN pose) among the ``keep`` scores
    the worst possible cost and loses to every valid one.  When no hypothesis is valid (collinear clouds, say) the call does not
    raise: every start is NaN, the refinement finds no pair and keeps it, so the returned pose is NaN with pairs 0, rmse NaN and
    status PN_ICP_CONVERGED | PN_ICP_FEW_PAIRS; test status for PN_ICP_FEW_PAIRS (or the pose for NaN) before using the result.
    Host reads: those of the steps, and the number of matched pairs."""
    import math
    if metric not in ("point", "plane", "gicp"):
        raise _lib.PointNetHipError(f"global_register: metric must be 'point', 'plane' or 'gicp', got {metric!r}")
    if source_normals is not None and metric != "gicp":
        raise _lib.PointNetHipError(f"global_register: source_normals goes with metric 'gicp'; metric {metric!r} does not read it")
    if accel not in (None, "grid"):
        raise _lib.PointNetHipError(f"global_register: accel must be None or 'grid', got {accel!r}")
    for name, v in (("max_dist", max_dist), ("feature_radius", feature_radius)):
        if v is None or not math.isfinite(float(v)) or not float(v) > 0.0:
            raise _lib.PointNetHipError(f"global_register: {name}={v} must be finite and > 0")
    if int(keep) < 1 or int(top) < 1:
        raise _lib.PointNetHipError(f"global_register: keep={keep} and top={top} must be >= 1")
    for key in icp:
        if key not in ("max_iters", "tol_rot", "tol_t") and not (key == "gicp_eps" and metric == "gicp"):
            raise _lib.PointNetHipError(f"global_register: {key}= is not an argument (max_iters, tol_rot and tol_t reach the loop)")
    require_gpu_tensor(source, "source", F32)
    require_gpu_tensor(target, "target", F32)
    if source.dim() == 2:
        source = source.unsqueeze(0)
    if source.dim() != 3 or source.shape[2] != 3 or target.dim() != 2 or target.shape[1] != 3 or target.device != source.device:
        raise _lib.PointNetHipError(f"global_register: source (B,N,3) or (N,3) and target (M,3) on one device expected, got "
                                    f"{tuple(source.shape)} / {tuple(target.shape)}")
    B, N, _ = source.shape
    dev = source.device
    nr = float(feature_radius if normals_radius is None else normals_radius)
    vs, vt = (viewpoint if source_viewpoint is None else source_viewpoint), (viewpoint if target_viewpoint is None else target_viewpoint)
    ref = _scan_reference("global_register", target, max_dist, metric, normals_radius, normals_k, vt, accel)
    ft = fpfh(ref.xyz, estimate_normals(ref.xyz, nr, int(k), vt)[0], float(feature_radius), int(k))
    stride = max(1, N // 8192) if stride is None else int(stride)
    sn = None
    if metric == "gicp":
        sn = _source_normals("global_register", source, source_normals, max_dist if normals_radius is None else normals_radius, normals_k, vs)
    outs = []
    for b in range(B):
        rows = _finite_rows(source[b])
        if rows.numel() < 3:
            raise _lib.PointNetHipError(f"global_register: source scan {b} has fewer than three finite points")
        ps, _, _ = _compact(source[b], rows, (0.0, 0.0, 0.0))
        fs = fpfh(ps, estimate_normals(ps, nr, int(k), vs)[0], float(feature_radius), int(k))
        idx, _ = feature_match(fs, ft, mutual=bool(mutual))
        sel = (idx >= 0).nonzero().squeeze(1)
        if sel.numel() < 3:
            raise _lib.PointNetHipError(f"global_register: source scan {b} has {sel.numel()} matched pairs; three make a hypothesis")
        poses, _, order = ransac_poses(ps[sel].contiguous(), ref.xyz[idx[sel].long()].contiguous(), max_dist, hypotheses, edge_ratio, seed)
        best = order[:min(int(keep), order.numel())]
        res = _scored_multistart(source[b:b + 1], torch.zeros(1, N, device=dev, dtype=torch.int32), ref, ref, poses[best].unsqueeze(0).contiguous(),
                                 top, stride, max_dist, dict(icp, metric=metric, **({} if sn is None else {"scan_normals": sn[b:b + 1]})))
        outs.append(res[:6] + (best[res[6].long()].to(torch.int32),))
    return tuple(torch.cat([o[i] for o in outs]) for i in range(7))


def icp_information(scan, labels, ref: IcpReference, pose, max_dist=float("inf")):
    """The 6x6 information matrix of every scan registered against the reference at ``pose`` (B,4,4) fp32 or fp64 (spec:
    include/pointnet_hip.h, pn_icp_information): the search of icp_correspond at the pose's fp32 rounding, then sum G^T G over the
    kept pairs, G = [-[q]_x | I] at the partner q -> (info (B,6,6) fp64, symmetric, in (omega, v) order; pairs (B,) int32; rmse
    (B,) fp64 = sqrt(sum d2 / pairs), NaN without a pair; idx (B,N) int32 and d2 (B,N) fp32, bit for bit icp_correspond's).  It
    is the weight of the pair's pose as an edge of ops.pose_graph_optimize.  ``ref``: an IcpReference, or an IcpGridReference
    searched through its grid (``max_dist`` must then not exceed the reference's); a mesh reference is refused."""
    what = "icp_information"
    _family(what, ref)
    if ref._INFO is None:
        raise _lib.PointNetHipError(f"{what}: the information pass takes a cloud reference (ops.icp_reference), not a mesh")
    ref._serves(what, max_dist)
    B, N, ws, nbytes = _icp_inputs(scan, labels, ref, what, False, ref._INFO[1])
    if not isinstance(pose, torch.Tensor) or tuple(pose.shape) != (B, 4, 4) or pose.dtype not in (F32, torch.float64):
        raise _lib.PointNetHipError(f"{what}: pose must be a ({B},4,4) fp32 or fp64 tensor")
    pose32 = require_gpu_tensor(pose.float().contiguous(), "pose")
    dev = scan.device
    idx = torch.empty(B, N, device=dev, dtype=torch.int32)
    d2 = torch.empty(B, N, device=dev, dtype=F32)
    so = torch.empty(B, 29, device=dev, dtype=torch.float64)
    name = ref._INFO[0]
    check(getattr(lib(), name)(ptr(scan), ptr(labels), B, N, ptr(ref._prim), ref._seg_c, ref.M, ref.n_parts, ptr(pose32), _max_d2(max_dist),
                               ptr(idx), ptr(d2), ptr(so), ptr(ws), nbytes, *ref._gicp_tail(), current_stream()), name)
    upper = torch.zeros(B, 6, 6, device=dev, dtype=torch.float64)         # (slices only: nothing here reads the host, so it captures)
    at = 1
    for r in range(6):
        upper[:, r, r:] = so[:, at:at + 6 - r]
        at += 6 - r
    info = upper + torch.triu(upper, 1).transpose(1, 2)
    return info, so[:, 0].to(torch.int32), torch.sqrt(so[:, 28] / so[:, 0]), idx, d2


def _pose_graph_edges(what, edges, K):
    """The edge list of a pose graph over K nodes, checked on the host -> (E, 2) int64 array: every index in [0, K), i != j, and
    the graph connected (union-find), each refusal naming the offender."""
    import numpy as np
    if isinstance(edges, torch.Tensor):
        if edges.is_cuda or edges.is_floating_point():
            raise _lib.PointNetHipError(f"{what}: edges must be a Python sequence of pairs or a CPU integer tensor")
        e = edges.numpy().astype(np.int64)
    else:
        try:
            e = np.asarray([[int(v) for v in pair] for pair in edges], np.int64)
        except (TypeError, ValueError):
            raise _lib.PointNetHipError(f"{what}: edges must be a sequence of (i, j) pairs") from None
    if e.ndim != 2 or e.shape[1] != 2:
        raise _lib.PointNetHipError(f"{what}: edges must be (E, 2) pairs, got shape {tuple(e.shape)}")
    if not 2 <= K <= _lib.PN_POSE_GRAPH_MAX_NODES:
        raise _lib.PointNetHipError(f"{what}: {K} nodes outside [2, {_lib.PN_POSE_GRAPH_MAX_NODES}]")
    if not K - 1 <= len(e) <= _lib.PN_POSE_GRAPH_MAX_EDGES:
        raise _lib.PointNetHipError(f"{what}: {len(e)} edges outside [K - 1 = {K - 1}, {_lib.PN_POSE_GRAPH_MAX_EDGES}]")
    root = list(range(K))

    def find(a):
        while root[a] != a:
            root[a] = root[root[a]]
            a = root[a]
        return a

    for k, (i, j) in enumerate(e.tolist()):
        if not (0 <= i < K and 0 <= j < K):
            raise _lib.PointNetHipError(f"{what}: edge {k} = ({i}, {j}) has an index outside [0, {K})")
        if i == j:
            raise _lib.PointNetHipError(f"{what}: edge {k} = ({i}, {j}) joins a node to itself")
        root[find(i)] = find(j)
    apart = [a for a in range(K) if find(a) != find(0)]
    if apart:
        raise _lib.PointNetHipError(f"{what}: the graph is not connected: no path of edges joins node {apart[0]} to node 0 "
                                    f"({len(apart)} such nodes)")
    return e


def pose_graph_optimize(edges, Z, info, poses, edge_weight=None, max_iters: int = 50, tol: float = 1e-10, lambda0: float = 1e-3):
    """Levenberg-Marquardt over the node poses of a pose graph, fp64 on the device in one launch (spec and conventions:
    include/pointnet_hip.h, pn_pose_graph_optimize).  ``poses`` (K,4,4) fp64: X_i maps cloud i's frame into the common frame;
    X_0 is held fixed and comes back bit for bit.  ``edges``: E pairs (i, j), a Python sequence or a CPU integer tensor; edge k
    carries ``Z[k]`` (4,4) fp64 with p_i ~= Z p_j -- what ops.register_scans(source=cloud_i, target=cloud_j) returns -- and the
    information ``info[k]`` (6,6) fp64 (ops.icp_information; read as given, symmetric expected).  ``edge_weight`` (E,) fp64 on the
    device, or None for all 1: a weight of 0 (or a negative or non-finite one) switches its edge off without a host read.
    -> (poses (K,4,4) fp64, cost (2,) fp64: at the input and at the result, iters (1,) int32, status (1,) int32: 0, or
    PN_POSE_GRAPH_MAX_ITERS = 1 | PN_POSE_GRAPH_SINGULAR = 2: a node was left without a live edge, the poses are the last accepted
    ones).  The edge list is checked on the host before any device call (index range, i != j, connectivity); the solve itself
    reads nothing back: capturable."""
    what = "pose_graph_optimize"
    if not isinstance(poses, torch.Tensor) or poses.dim() != 3 or tuple(poses.shape[1:]) != (4, 4):
        raise _lib.PointNetHipError(f"{what}: poses must be a (K,4,4) fp64 tensor")
    K = poses.shape[0]
    e = _pose_graph_edges(what, edges, K)
    E = len(e)
    require_gpu_tensor(poses, "poses", torch.float64)
    require_gpu_tensor(Z, "Z", torch.float64)
    require_gpu_tensor(info, "info", torch.float64)
    dev = poses.device
    if tuple(Z.shape) != (E, 4, 4) or tuple(info.shape) != (E, 6, 6) or Z.device != dev or info.device != dev:
        raise _lib.PointNetHipError(f"{what}: Z ({E},4,4) and info ({E},6,6) on {dev} expected, got {tuple(Z.shape)} / {tuple(info.shape)}")
    if edge_weight is not None:
        require_gpu_tensor(edge_weight, "edge_weight", torch.float64)
        if tuple(edge_weight.shape) != (E,) or edge_weight.device != dev:
            raise _lib.PointNetHipError(f"{what}: edge_weight must be ({E},) fp64 on {dev}, got {tuple(edge_weight.shape)}")
    ed = torch.from_numpy(e.astype("int32")).to(dev)
    out = poses.clone()
    cost = torch.empty(2, device=dev, dtype=torch.float64)
    iters = torch.empty(1, device=dev, dtype=torch.int32)
    status = torch.empty(1, device=dev, dtype=torch.int32)
    nbytes = lib().pn_pose_graph_workspace_bytes(K, E)
    ws = torch.empty(max(nbytes, 8), device=dev, dtype=torch.uint8)
    check(lib().pn_pose_graph_optimize(K, E, ptr(ed), ptr(Z), ptr(info), ptr(edge_weight), ptr(out), int(max_iters), float(tol), float(lambda0),
                                       ptr(cost), ptr(iters), ptr(status), ptr(ws), nbytes, current_stream()), "pn_pose_graph_optimize")
    return out, cost, iters, status


def _rigid_inverse(T):
    """the inverse of (.., 4, 4) poses [R t] with R a rotation, in the poses' own precision"""
    Rt = T[..., :3, :3].transpose(-1, -2)
    out = torch.zeros_like(T)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -(Rt @ T[..., :3, 3:4])[..., 0]
    out[..., 3, 3] = 1.0
    return out


_MULTIWAY_KEYS = ("max_iters", "tol_rot", "tol_t", "normals_radius", "normals_k", "accel")
_MULTIWAY_GLOBAL_KEYS = ("feature_radius", "hypotheses", "keep", "top", "mutual", "seed")


def _register_edges(what, clouds, ks, e, starts, max_dist, metric, min_fitness, reg, Z, info, pairs, weight):
    """the edges ``ks`` (rows of ``e``) registered and weighed, one ops.register_scans call and one ops.icp_information call per
    distinct target, into rows ``ks`` of Z, info, pairs and weight.  ``starts``: {k: (4,4) start of edge k}, or None for
    register_scans(init="global")."""
    dev = clouds[0].device
    for j in sorted({int(e[k, 1]) for k in ks}):
        group = [k for k in ks if int(e[k, 1]) == j]
        n = max(clouds[int(e[k, 0])].shape[0] for k in group)
        src = torch.full((len(group), n, 3), float("nan"), device=dev, dtype=F32)
        for b, k in enumerate(group):
            c = clouds[int(e[k, 0])]
            src[b, :c.shape[0]] = c
        if starts is None:
            res = register_scans(src, clouds[j], max_dist, metric=metric, init="global", **reg)
        else:
            res = register_scans(src, clouds[j], max_dist, init_pose=torch.stack([starts[k] for k in group]), metric=metric, **reg)
        ref = _scan_reference(what, clouds[j], max_dist, "point", None, 8, None, reg.get("accel", "grid"))
        labels = torch.zeros(len(group), n, device=dev, dtype=torch.int32)
        inf, prs, _, _, _ = icp_information(src, labels, ref, res[0], max_dist)
        rows = torch.tensor(group, device=dev)
        Z[rows] = res[0]
        info[rows] = inf
        pairs[rows] = prs
        finite = torch.isfinite(src).all(2).sum(1)
        weight[rows] = (prs.to(torch.float64) >= float(min_fitness) * finite.to(torch.float64)).to(torch.float64)


def multiway_register(clouds, max_dist, edges=None, init=None, metric: str = "plane", min_fitness: float = 0.0, pose_graph=None, **reg):
    """Multiway registration of K scans of one body (PCL's and Open3D's): pairwise registrations as the edges of a pose graph, an
    information matrix per edge, and a pose-graph solve that spreads the edges' disagreement over the nodes, so a loop closes
    instead of the chain's errors adding up.  ``clouds``: K (N_i,3) fp32 tensors on one device (non-finite rows take no part).
    -> (poses (K,4,4) fp64: X_i maps cloud i into the common frame, X_0 fixed; cost (2,), iters (1,), status (1,): those of
    ops.pose_graph_optimize; edges (E,2) int32 on the host; Z (E,4,4) fp64: edge k = (i, j) has p_i ~= Z_k p_j; info (E,6,6)
    fp64; pairs (E,) int32).
    ``edges``: None, the chain (a, a + 1) only (legal, but it closes no loop); "all", every pair i < j; or a list of pairs.
    Edge (i, j) is ops.register_scans(source=cloud_i, target=cloud_j, ``max_dist``, ``metric``), one call per distinct target with
    its sources batched and NaN-padded to a common length, then ops.icp_information at the result.  The start of edge (i, j):
    X_i^-1 X_j when ``init`` gives (K,4,4) poses; with ``init`` None the identity for the chain edges and, for the others, the chain
    composed from their results; with ``init`` = "global" register_scans(init="global") (``feature_radius`` and the other global
    keywords reach it).  The nodes start at ``init``, else at the composed chain (which the edge list must then contain).
    An edge whose kept pairs are fewer than ``min_fitness`` times its source's finite rows gets weight 0, on the device: the graph
    solve drops it without a host read (a node left with no live edge shows as PN_POSE_GRAPH_SINGULAR).  ``reg``: max_iters,
    tol_rot, tol_t, normals_radius, normals_k, accel (and gicp_eps with metric "gicp") reach register_scans; ``pose_graph``: a
    dict of max_iters, tol, lambda0 for the graph solve.  The result merges with ops.merge_scans."""
    what = "multiway_register"
    glob = isinstance(init, str)
    if glob and init != "global":
        raise _lib.PointNetHipError(f"{what}: init must be None, 'global' or (K,4,4) poses, got {init!r}")
    if metric not in ("point", "plane", "gicp"):
        raise _lib.PointNetHipError(f"{what}: metric must be 'point', 'plane' or 'gicp', got {metric!r}")
    for key in reg:
        if key not in _MULTIWAY_KEYS and not (key == "gicp_eps" and metric == "gicp") and not (glob and key in _MULTIWAY_GLOBAL_KEYS):
            raise _lib.PointNetHipError(f"{what}: {key}= is not an argument ({', '.join(_MULTIWAY_KEYS)} reach register_scans, "
                                        f"{', '.join(_MULTIWAY_GLOBAL_KEYS)} with init='global')")
    pg = dict(pose_graph or {})
    for key in pg:
        if key not in ("max_iters", "tol", "lambda0"):
            raise _lib.PointNetHipError(f"{what}: pose_graph has no {key} (max_iters, tol and lambda0 reach the graph solve)")
    if not isinstance(clouds, (list, tuple)) or len(clouds) < 2:
        raise _lib.PointNetHipError(f"{what}: clouds must be a list of at least two (N,3) tensors")
    K = len(clouds)
    if isinstance(edges, str) or edges is None:
        if edges not in (None, "all"):
            raise _lib.PointNetHipError(f"{what}: edges must be None (the chain), 'all' or a list of pairs, got {edges!r}")
        edges = [(a, a + 1) for a in range(K - 1)] if edges is None else [(i, j) for i in range(K) for j in range(i + 1, K)]
    e = _pose_graph_edges(what, edges, K)
    E = len(e)
    poses0 = not glob and init is not None
    chain = {(int(i), int(j)): k for k, (i, j) in reversed(list(enumerate(e.tolist()))) if j == i + 1}
    if not poses0 and len(chain) != K - 1:
        missing = [a for a in range(K - 1) if (a, a + 1) not in chain][0]
        raise _lib.PointNetHipError(f"{what}: without init poses the nodes start at the composed chain: edges must contain "
                                    f"({missing}, {missing + 1}), or pass init=(K,4,4) poses")
    for a, c in enumerate(clouds):
        require_gpu_tensor(c, f"clouds[{a}]", F32)
        if c.dim() != 2 or c.shape[1] != 3 or c.shape[0] < 1 or c.device != clouds[0].device:
            raise _lib.PointNetHipError(f"{what}: clouds[{a}] must be (N,3) on {clouds[0].device}, got {tuple(c.shape)} on {c.device}")
    dev = clouds[0].device
    if poses0:
        if not isinstance(init, torch.Tensor) or tuple(init.shape) != (K, 4, 4) or init.device != dev:
            raise _lib.PointNetHipError(f"{what}: init must be None, 'global' or a ({K},4,4) tensor on {dev}")
        init = init.to(torch.float64).contiguous()
    Z = torch.zeros(E, 4, 4, device=dev, dtype=torch.float64)
    info = torch.zeros(E, 6, 6, device=dev, dtype=torch.float64)
    pairs = torch.zeros(E, device=dev, dtype=torch.int32)
    weight = torch.zeros(E, device=dev, dtype=torch.float64)
    args = (max_dist, metric, min_fitness, reg, Z, info, pairs, weight)
    if poses0:
        rel = _rigid_inverse(init[e[:, 0]]) @ init[e[:, 1]]
        _register_edges(what, clouds, list(range(E)), e, {k: rel[k] for k in range(E)}, *args)
        start = init
    else:
        eye = torch.eye(4, device=dev, dtype=torch.float64)
        first = sorted(chain.values())
        _register_edges(what, clouds, first, e, None if glob else {k: eye for k in first}, *args)
        nodes = [eye]
        for a in range(K - 1):
            nodes.append(nodes[a] @ Z[chain[(a, a + 1)]])
        start = torch.stack(nodes)
        rest = [k for k in range(E) if k not in set(first)]
        if rest:
            rel = _rigid_inverse(start[e[:, 0]]) @ start[e[:, 1]]
            _register_edges(what, clouds, rest, e, None if glob else {k: rel[k] for k in rest}, *args)
    poses, cost, iters, status = pose_graph_optimize(e, Z, info, start, weight, **pg)
    return poses, cost, iters, status, torch.from_numpy(e.astype("int32")), Z, info, pairs


def merge_scans(clouds, poses, leaf, labels=None, n_labels: int = 0):
    """The registered scans as one model: every cloud (N_i,3) fp32 moved by its pose X_i (``poses`` (K,4,4), rounded to fp32: p' =
    R p + t), concatenated, its finite rows voxel-downsampled at ``leaf`` (a scalar or three) from their per-axis minimum ->
    ops.voxel_downsample's (xyz (V,3), counts (V,), majority labels (V,) or None).  ``labels``: the clouds' per-point labels, K
    int32 tensors (e.g. PointNet.predict_scan's), with ``n_labels`` their number.  The model of scans alone then serves as a
    labelled reference: ``ops.icp_reference(xyz, majority, n_labels)`` goes to semantic_icp, predict_pose and the grid like one
    made from a mesh."""
    what = "merge_scans"
    if not isinstance(clouds, (list, tuple)) or len(clouds) < 1:
        raise _lib.PointNetHipError(f"{what}: clouds must be a list of (N,3) tensors")
    K = len(clouds)
    if not isinstance(poses, torch.Tensor) or tuple(poses.shape) != (K, 4, 4):
        raise _lib.PointNetHipError(f"{what}: poses must be a ({K},4,4) tensor, one pose per cloud")
    if labels is not None and (not isinstance(labels, (list, tuple)) or len(labels) != K):
        raise _lib.PointNetHipError(f"{what}: labels must be a list of {K} (N,) int32 tensors, one per cloud")
    P = poses.float()
    moved = []
    for a, c in enumerate(clouds):
        require_gpu_tensor(c, f"clouds[{a}]", F32)
        if c.dim() != 2 or c.shape[1] != 3 or c.device != P.device:
            raise _lib.PointNetHipError(f"{what}: clouds[{a}] must be (N,3) on {P.device}, got {tuple(c.shape)} on {c.device}")
        if labels is not None:
            require_gpu_tensor(labels[a], f"labels[{a}]", torch.int32)
            if tuple(labels[a].shape) != (c.shape[0],):
                raise _lib.PointNetHipError(f"{what}: labels[{a}] must be ({c.shape[0]},), got {tuple(labels[a].shape)}")
        moved.append(c @ P[a, :3, :3].T + P[a, :3, 3])
    xyz = torch.cat(moved)
    rows = _finite_rows(xyz)
    if rows.numel() < 1:
        raise _lib.PointNetHipError(f"{what}: the clouds have no finite point")
    lab = None if labels is None else torch.cat(list(labels))
    pts, origin, _ = _compact(xyz, rows, None)
    if lab is not None and rows.numel() != xyz.shape[0]:
        lab = lab[rows].contiguous()
    return voxel_downsample(pts.contiguous(), _leaf3(leaf, what), origin, lab, int(n_labels))


def _oriented_rows(what, xyz, normals):
    """the checked inputs of the reconstruction entries -> the rows (ascending) with three finite coordinates and a finite normal
    that is not zero"""
    require_gpu_tensor(xyz, "xyz", F32)
    require_gpu_tensor(normals, "normals", F32)
    if xyz.dim() != 2 or xyz.shape[1] != 3 or normals.shape != xyz.shape or normals.device != xyz.device:
        raise _lib.PointNetHipError(f"{what} expects (N, 3) points and normals on one device, got {tuple(xyz.shape)} and {tuple(normals.shape)}")
    nrm = torch.where((normals != 0).any(1, keepdim=True), normals, torch.full_like(normals, float("nan")))
    rows = _finite_rows(torch.cat((xyz, nrm), 1))
    if rows.numel() < 1:
        raise _lib.PointNetHipError(f"{what}: no row has finite coordinates and a finite, non-zero normal")
    return rows


def _lattice(what, pts, voxel, radius, origin, dims):
    """the lattice of a reconstruction call -> (origin: three Python floats (fp64), dims (nx, ny, nz)); the default is the bounding
    box of ``pts`` padded by ``radius``: origin = min - radius, n = ceil(((max + radius) - origin) / voxel) + 1 per axis, in fp64"""
    import math
    if not (voxel > 0 and math.isfinite(voxel)) or not (radius > 0 and math.isfinite(radius)):
        raise _lib.PointNetHipError(f"{what}: voxel and radius must be positive and finite, got {voxel!r} and {radius!r}")
    lo, hi = pts.min(0).values.double().cpu().tolist(), pts.max(0).values.double().cpu().tolist()
    origin = [l - radius for l in lo] if origin is None else [float(o) for o in origin]
    if len(origin) != 3:
        raise _lib.PointNetHipError(f"{what}: origin must be three values, got {origin!r}")
    if dims is None:
        dims = [max(int(math.ceil(((h + radius) - o) / voxel)) + 1, 2) for h, o in zip(hi, origin)]
    dims = tuple(int(d) for d in dims)
    if len(dims) != 3:
        raise _lib.PointNetHipError(f"{what}: dims must be (nx, ny, nz), got {dims!r}")
    return origin, dims


def _implicit_field(pts, nrm, grid_origin, voxel, radius, min_points, origin, dims, want_count=False):
    """pn_recon_field on compacted rows, their internal grid placed at ``grid_origin`` (their minimum) -> (f (nx*ny*nz,), count or
    None)"""
    n, dev = pts.shape[0], pts.device
    P = dims[0] * dims[1] * dims[2]
    big = not (0 < P <= _lib.PN_RECON_MAX_LATTICE)         # (refused by the library: it gets no buffer to write to)
    f = torch.empty(0 if big else P, device=dev, dtype=F32)
    count = torch.empty(0 if big else P, device=dev, dtype=torch.int32) if want_count else None
    _grid_call("pn_recon_field", "pn_recon_field_workspace_bytes", n, dev, ptr(pts), ptr(nrm), n, float(radius),
               _f3(grid_origin), (C.c_double * 3)(*origin), float(voxel), *dims, int(min_points), ptr(f), ptr(count),
               errors="pn_radius_knn", **_radius_grid(radius))
    return f, count


def implicit_field(xyz: torch.Tensor, normals: torch.Tensor, voxel: float, radius: float, min_points: int = 3, origin=None, dims=None,
                   return_count: bool = False):
    """The implicit surface of an oriented cloud on a dense lattice (spec: include/pointnet_hip.h, pn_recon_field): xyz (N, 3) and
    normals (N, 3) fp32 on the device (ops.estimate_normals' with a viewpoint) -> (f (nz, ny, nx) fp32, origin (three floats),
    dims (nx, ny, nz)); with ``return_count`` a fourth value, count (nz, ny, nx) int32.  f is the implicit-moving-least-squares
    field with the weight (1 - d/radius^2)^2 over ALL points within ``radius`` of a lattice point: about the signed distance to
    the surface, negative behind it; NaN where fewer than ``min_points`` points are in reach.  The default lattice is the bounding
    box of the kept points padded by ``radius`` (``origin`` = min - radius, lattice point i at origin + i * voxel); it is dense and
    holds at most 2^28 points.  Rows with a non-finite coordinate or a non-finite or zero normal are dropped first.  Host reads:
    the number of kept rows, their minimum and maximum, the error word."""
    what = "implicit_field"
    rows = _oriented_rows(what, xyz, normals)
    pts, grid_origin, _ = _compact(xyz, rows, None)
    nrm = normals if pts is xyz else normals[rows].contiguous()
    origin, dims = _lattice(what, pts, float(voxel), float(radius), origin, dims)
    f, count = _implicit_field(pts, nrm, grid_origin, voxel, radius, min_points, origin, dims, return_count)
    shape = (dims[2], dims[1], dims[0])
    return (f.view(shape), tuple(origin), dims, count.view(shape)) if return_count else (f.view(shape), tuple(origin), dims)


def _field_surface(f, origin, voxel, dims):
    """marching tetrahedra over a field (pn_recon_count, one host read of the two counts, pn_recon_emit) -> (vertices, faces)"""
    dev = f.device
    n_out = torch.zeros(2, device=dev, dtype=torch.int32)
    _grid_call("pn_recon_count", "pn_recon_workspace_bytes", dims[0], dev, ptr(f), *dims, ptr(n_out), size_args=dims[1:])
    V, Fc = (int(v) for v in n_out.tolist())
    vertices = torch.empty(V, 3, device=dev, dtype=F32)
    faces = torch.empty(Fc, 3, device=dev, dtype=torch.int32)
    _grid_call("pn_recon_emit", "pn_recon_workspace_bytes", dims[0], dev, ptr(f), (C.c_double * 3)(*origin), float(voxel), *dims,
               ptr(vertices), V, ptr(faces), Fc, ptr(n_out), size_args=dims[1:])
    return vertices, faces


def reconstruct_mesh(xyz: torch.Tensor, normals: torch.Tensor, voxel: float, radius: Optional[float] = None, min_points: int = 3,
                     labels: Optional[torch.Tensor] = None, n_labels: int = 0, label_k: int = 3):
    """An indexed triangle mesh from an oriented cloud (spec: include/pointnet_hip.h, pn_recon_field / pn_recon_count /
    pn_recon_emit): ops.implicit_field on its default lattice (``radius`` default 3 * voxel), then marching tetrahedra over the
    lattice -> (vertices (V, 3) fp32, faces (F, 3) int32, face_labels (F,) int32 or None).  Vertices are shared and every one is
    used; every face's normal points the way the input normals do; the result is a pure function of the input.  ``labels`` (N,)
    int32 in [0, n_labels): the points' part labels; a face takes the label that ops.knn_propagate (``label_k`` nearest points,
    one-hot values) gives its centroid.  Limits: a face is degenerate (zero area) where the field is exactly 0 at a lattice point
    -- ops.icp_mesh_reference drops those; a sheet thinner than about 2 * radius mixes its two sides; on a convex surface the
    field's zero lies a little outside the points (IMLS's curvature bias, of the order radius^2 / R for a radius of curvature R).
    Host reads: those of ops.implicit_field and the two counts."""
    what = "reconstruct_mesh"
    rows = _oriented_rows(what, xyz, normals)
    voxel = float(voxel)
    radius = 3.0 * voxel if radius is None else float(radius)
    if labels is not None:
        require_gpu_tensor(labels, "labels", torch.int32)
        if tuple(labels.shape) != (xyz.shape[0],) or not 1 <= int(n_labels) <= 16 or labels.device != xyz.device:
            raise _lib.PointNetHipError(f"{what}: labels must be ({xyz.shape[0]},) int32 on {xyz.device} with 1 <= n_labels <= 16")
    pts, grid_origin, _ = _compact(xyz, rows, None)
    whole = pts is xyz
    nrm = normals if whole else normals[rows].contiguous()
    origin, dims = _lattice(what, pts, voxel, radius, None, None)
    f, _ = _implicit_field(pts, nrm, grid_origin, voxel, radius, min_points, origin, dims)
    vertices, faces = _field_surface(f, origin, voxel, dims)
    if labels is None:
        return vertices, faces, None
    lab = labels if whole else labels[rows]
    if bool(((lab < 0) | (lab >= int(n_labels))).any()):
        raise _lib.PointNetHipError(f"{what}: a kept point's label lies outside [0, {int(n_labels)})")
    if faces.shape[0] == 0:
        return vertices, faces, torch.empty(0, device=xyz.device, dtype=torch.int32)
    centroids = vertices[faces.long()].mean(1)
    onehot = torch.nn.functional.one_hot(lab.long(), int(n_labels)).to(F32)
    face_labels = knn_propagate(centroids[None].contiguous(), pts[None], int(label_k), onehot[None].contiguous())[3][0]
    return vertices, faces, face_labels


def scans_to_mesh(clouds, poses, voxel: float, radius: Optional[float] = None, normals_radius: Optional[float] = None, normals_k: int = 8,
                  labels=None, n_labels: int = 0, min_points: int = 3):
    """Registered scans -> one labelled mesh: per scan ops.estimate_normals (``normals_radius`` default ``radius``, default
    3 * voxel; ``normals_k`` neighbours) turned towards the sensor, which is the scan frame's origin; the points moved by the
    scan's pose X_i (``poses`` (K,4,4), rounded to fp32: p' = R p + t) and the normals rotated by it; rows without a valid normal
    dropped; the scans concatenated; then ops.reconstruct_mesh -> (vertices, faces, face_labels or None).  ``labels``: K int32
    tensors (e.g. PointNet.predict_scan's) with ``n_labels`` their number.  The result goes straight into
    ``ops.icp_mesh_reference(vertices, faces, face_labels, n_labels)``, and from there to the mesh metric of ops.semantic_icp,
    ops.lidar_frames and ops.mesh_sample.  Limits: ops.reconstruct_mesh's (zero-area faces where the field is exactly 0 at a
    lattice point, which icp_mesh_reference drops; a sheet thinner than about 2 * radius mixes its two sides)."""
    what = "scans_to_mesh"
    if not isinstance(clouds, (list, tuple)) or len(clouds) < 1:
        raise _lib.PointNetHipError(f"{what}: clouds must be a list of (N,3) tensors")
    K = len(clouds)
    if not isinstance(poses, torch.Tensor) or tuple(poses.shape) != (K, 4, 4):
        raise _lib.PointNetHipError(f"{what}: poses must be a ({K},4,4) tensor, one pose per cloud")
    if labels is not None and (not isinstance(labels, (list, tuple)) or len(labels) != K):
        raise _lib.PointNetHipError(f"{what}: labels must be a list of {K} (N,) int32 tensors, one per cloud")
    voxel = float(voxel)
    radius = 3.0 * voxel if radius is None else float(radius)
    nr = radius if normals_radius is None else float(normals_radius)
    P = poses.float()
    pts, nrm = [], []
    for a, c in enumerate(clouds):
        require_gpu_tensor(c, f"clouds[{a}]", F32)
        if c.dim() != 2 or c.shape[1] != 3 or c.device != P.device:
            raise _lib.PointNetHipError(f"{what}: clouds[{a}] must be (N,3) on {P.device}, got {tuple(c.shape)} on {c.device}")
        if labels is not None:
            require_gpu_tensor(labels[a], f"labels[{a}]", torch.int32)
            if tuple(labels[a].shape) != (c.shape[0],):
                raise _lib.PointNetHipError(f"{what}: labels[{a}] must be ({c.shape[0]},), got {tuple(labels[a].shape)}")
        n = estimate_normals(c, nr, int(normals_k), viewpoint=(0.0, 0.0, 0.0))[0]
        pts.append(c @ P[a, :3, :3].T + P[a, :3, 3])
        nrm.append(n @ P[a, :3, :3].T)
    lab = None if labels is None else torch.cat(list(labels))
    return reconstruct_mesh(torch.cat(pts).contiguous(), torch.cat(nrm).contiguous(), voxel, radius, min_points, lab, n_labels)


def _indexed_mesh(what, vertices, faces, labels=None):
    """the checked inputs of the mesh-cleaning entries -> (V, F)"""
    require_gpu_tensor(vertices, "vertices", F32)
    require_gpu_tensor(faces, "faces", torch.int32)
    if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or faces.device != vertices.device:
        raise _lib.PointNetHipError(f"{what} expects (V, 3) vertices and (F, 3) faces on one device, got {tuple(vertices.shape)} and {tuple(faces.shape)}")
    if labels is not None:
        require_gpu_tensor(labels, "labels", torch.int32)
        if tuple(labels.shape) != (faces.shape[0],) or labels.device != faces.device:
            raise _lib.PointNetHipError(f"{what}: labels must be ({faces.shape[0]},) int32 on {faces.device}, got {tuple(labels.shape)}")
    return vertices.shape[0], faces.shape[0]


def mesh_components(vertices: torch.Tensor, faces: torch.Tensor):
    """Connected components of an indexed triangle mesh (spec: include/pointnet_hip.h, pn_mesh_components): vertices (V, 3) fp32 and
    faces (F, 3) int32 on the device -> (face_component (F,) int32, sizes (K,) int32).  Two faces are one component when they share
    a vertex INDEX (positions are not compared: weld first, e.g. with ops.simplify_mesh, if the mesh is a triangle soup); ids are in
    ascending order of each component's lowest vertex index; sizes counts faces.  ops.cluster_mask takes the result unchanged
    (``min_points`` then counts faces).  A face index outside [0, V) raises.  Host reads: K and the error word."""
    what = "mesh_components"
    V, Fc = _indexed_mesh(what, vertices, faces)
    dev = vertices.device
    comp = torch.empty(Fc, device=dev, dtype=torch.int32)
    if Fc == 0:
        return comp, torch.empty(0, device=dev, dtype=torch.int32)
    if V == 0:
        raise _lib.PointNetHipError(f"{what}: a face index is outside [0, 0)")
    cap = min(V, Fc)
    sizes = torch.empty(cap, device=dev, dtype=torch.int32)
    n_out = torch.zeros(1, device=dev, dtype=torch.int32)
    _grid_call("pn_mesh_components", "pn_mesh_components_workspace_bytes", V, dev, ptr(vertices), V, ptr(faces), Fc, ptr(comp), ptr(sizes), cap,
               ptr(n_out), V=V)
    return comp, sizes[:int(n_out.item())]


_MESH_PLACEMENT = {"mean": 0, "quadric": 1}


def simplify_mesh(vertices: torch.Tensor, faces: torch.Tensor, leaf, labels: Optional[torch.Tensor] = None, placement: str = "quadric",
                  origin=None, rank_tol: float = 1e-3):
    """Vertex-clustering simplification (spec: include/pointnet_hip.h, pn_mesh_simplify): vertices (V, 3) fp32, faces (F, 3) int32 and
    optional face ``labels`` (F,) int32 on the device -> (vertices (V', 3), faces (F', 3), labels (F',) or None).  All vertices in
    one cell of the grid (``leaf`` a scalar or three values; ``origin`` default the per-axis minimum of the finite vertices) become
    one vertex: ``placement="mean"`` puts it at the mean of the cell's face corners, ``"quadric"`` (Lindstrom) where the planes of
    the cell's faces meet, which keeps edges and corners sharp; directions whose eigenvalue is at most ``rank_tol`` times the
    largest keep the mean, and a position more than one leaf from the mean falls back to it.  Faces that lose a corner to a
    neighbour's cell are dropped, as are later copies of a face (same cells, same orientation); the rest keep their order and
    their label, and every returned vertex is used.  The result is a pure function of the input.  A face index outside [0, V)
    raises, as in ops.icp_mesh_reference; faces with a non-finite vertex are dropped before the call.  More than 2^21 occupied
    cells raise: increase leaf.  Host reads: one of the input's facts (an index out of range, a face to drop, the finite minimum
    for the default origin), the number of faces left when some were dropped, the error word, and one of the two counts."""
    what = "simplify_mesh"
    V, Fc = _indexed_mesh(what, vertices, faces, labels)
    if placement not in _MESH_PLACEMENT:
        raise _lib.PointNetHipError(f"{what}: placement must be 'mean' or 'quadric', got {placement!r}")
    leaf3 = _leaf3(leaf, what)
    dev = vertices.device
    empty = (torch.empty(0, 3, device=dev, dtype=F32), torch.empty(0, 3, device=dev, dtype=torch.int32),
             None if labels is None else torch.empty(0, device=dev, dtype=torch.int32))
    if Fc == 0:
        return empty
    if V == 0:
        raise _lib.PointNetHipError(f"{what}: a face index is outside [0, {V})")
    # one read for the three facts about the input: an index out of range, a face with a non-finite vertex, the finite minimum
    finite = torch.isfinite(vertices).all(1)
    ok = finite[faces.long().clamp(0, V - 1)].all(1)
    low = torch.where(finite[:, None], vertices, torch.full_like(vertices, float("inf"))).min(0).values
    bad_index, dropped, *low = torch.cat((((faces < 0) | (faces >= V)).any().to(F32)[None], (~ok).any().to(F32)[None], low)).tolist()
    if bad_index:
        raise _lib.PointNetHipError(f"{what}: a face index is outside [0, {V})")
    if dropped:
        faces = faces[ok].contiguous()
        labels = None if labels is None else labels[ok].contiguous()
        Fc = faces.shape[0]
        if Fc == 0:
            return empty
    if origin is None:
        origin = low
    v_out = torch.empty(min(V, 3 * Fc), 3, device=dev, dtype=F32)
    f_out = torch.empty(Fc, 3, device=dev, dtype=torch.int32)
    l_out = None if labels is None else torch.empty(Fc, device=dev, dtype=torch.int32)
    n_out = torch.zeros(2, device=dev, dtype=torch.int32)
    _grid_call("pn_mesh_simplify", "pn_mesh_simplify_workspace_bytes", Fc, dev, ptr(vertices), V, ptr(faces), ptr(labels), Fc,
               _f3(leaf3), _f3(origin), _MESH_PLACEMENT[placement], float(rank_tol), ptr(v_out), ptr(f_out), ptr(l_out),
               ptr(n_out), V=V)
    nv, nf = (int(v) for v in n_out.tolist())
    return v_out[:nv], f_out[:nf], None if labels is None else l_out[:nf]


def clean_mesh(vertices: torch.Tensor, faces: torch.Tensor, labels: Optional[torch.Tensor] = None, clean: Optional[dict] = None,
               simplify: Optional[dict] = None):
    """What follows ops.reconstruct_mesh / ops.scans_to_mesh on real scans, in this order: ``clean=dict(keep="largest" | "all",
    min_faces=1)`` keeps the connected components that ops.cluster_mask selects from ops.mesh_components' result (a handful of
    noise points that pass ``min_points`` leave detached shells) and drops the vertices they no longer use;
    ``simplify=dict(leaf=, placement="quadric", rank_tol=1e-3)`` is ops.simplify_mesh -> (vertices, faces, labels or None).  With
    both None the mesh comes back as it is.  The result goes into ``ops.icp_mesh_reference`` as the reconstruction's does."""
    what = "clean_mesh"
    _indexed_mesh(what, vertices, faces, labels)
    for name, opt, keys in (("clean", clean, ("keep", "min_faces")), ("simplify", simplify, ("leaf", "placement", "rank_tol"))):
        if opt is not None and (not isinstance(opt, dict) or set(opt) - set(keys)):
            raise _lib.PointNetHipError(f"{what}: {name} must be a dict with keys among {keys}, got {opt!r}")
    if simplify is not None and "leaf" not in simplify:
        raise _lib.PointNetHipError(f"{what}: simplify needs a leaf")
    if clean is not None and faces.shape[0] > 0:
        comp, sizes = mesh_components(vertices, faces)
        mask = cluster_mask(comp, sizes, keep=clean.get("keep", "largest"), min_points=int(clean.get("min_faces", 1)))
        faces = faces[mask]
        labels = None if labels is None else labels[mask].contiguous()
        used = torch.zeros(vertices.shape[0], device=vertices.device, dtype=torch.bool)
        used[faces.reshape(-1).long()] = True
        new = (torch.cumsum(used.to(torch.int32), 0, dtype=torch.int32) - 1)
        vertices, faces = vertices[used].contiguous(), new[faces.long()].contiguous()
    if simplify is not None:
        return simplify_mesh(vertices, faces, simplify["leaf"], labels, simplify.get("placement", "quadric"), None, simplify.get("rank_tol", 1e-3))
    return vertices, faces, labels


def dense_layer(x, w, trans=False, bias=None, gamma=None, beta=None, moving_mean=None, moving_var=None, bn_mode=0, act=0, keep=None,
                rate=0.0, momentum=0.99, eps=1e-3, counters=None):
    """DenseLayer forward in one launch: returns (z, a, mean, invstd); moving statistics are updated in place (bn_mode 1)."""
    R, K = x.shape
    C_ = w.shape[0] if trans else w.shape[1]
    dev = x.device
    ws = torch.empty(max(1, lib().pn_dense_workspace_floats(R, K, C_)), device=dev, dtype=F32)
    if counters is None:
        counters = torch.zeros(256, device=dev, dtype=torch.int32)
    z = torch.empty(R, C_, device=dev, dtype=F32)
    a = torch.empty(R, C_, device=dev, dtype=F32)
    mean = torch.empty(C_, device=dev, dtype=F32)
    invstd = torch.empty(C_, device=dev, dtype=F32)
    check(lib().pn_dense_layer(ptr(x), x.stride(0), ptr(w), w.stride(0), int(trans), R, K, C_, ptr(ws), ptr(counters), ptr(bias), ptr(gamma),
                               ptr(beta), ptr(moving_mean), ptr(moving_var), momentum, eps, bn_mode, act, ptr(keep),
                               1.0 / (1.0 - rate), ptr(z), ptr(a), ptr(mean), ptr(invstd), current_stream()), "pn_dense_layer")
    return z, a, mean, invstd


def dense_bwd_step(dz_above, w_above, z=None, gamma=None, beta=None, mean=None, invstd=None, bn_mode=0, act=0, keep=None, rate=0.0):
    """one launch of a backward chain: dx = dz_above . W_above^T (w_above: the (C, K) kernel of the layer above) and, with z given,
    the layer below taken backward in the same launch: returns (dx, dz, dgamma, dbeta, dbias)"""
    R, K = dz_above.shape
    C_ = w_above.shape[0]
    dev = dz_above.device
    ws = torch.empty(max(1, lib().pn_dense_workspace_floats(R, K, C_)), device=dev, dtype=F32)
    counters = torch.zeros(256, device=dev, dtype=torch.int32)
    dx = torch.empty(R, C_, device=dev, dtype=F32)
    dz = dg = db = dbias = None
    tail = None
    if z is not None:
        dz = torch.empty(R, C_, device=dev, dtype=F32)
        dg = torch.zeros(C_, device=dev, dtype=F32); db = torch.zeros(C_, device=dev, dtype=F32); dbias = torch.zeros(C_, device=dev, dtype=F32)
        tail = _lib.pn_dense_tail()
        for k, v in dict(z=z, gamma=gamma, beta=beta, mean=mean, invstd=invstd, keep=keep, dz=dz, dgamma=dg, dbeta=db, dbias=dbias).items():
            setattr(tail, k, None if v is None else v.data_ptr())
        tail.keep_scale = 1.0 / (1.0 - rate)
        tail.bn_mode, tail.act = bn_mode, act
    check(lib().pn_dense_bwd_step(ptr(dz_above), dz_above.stride(0), ptr(w_above), w_above.stride(0), R, K, C_, ptr(ws), ptr(counters), ptr(dx),
                                  C.byref(tail) if tail is not None else None, current_stream()), "pn_dense_bwd_step")
    return dx, dz, dg, db, dbias


def dense_wgrad_batch(jobs):
    """jobs: [(x (R, K), dz (R, C), want_db)] -> [(dw (K, C), db (C) or None)] in one launch"""
    arr = (_lib.pn_dense_wgrad_job * len(jobs))()
    outs = []
    for j, (x, dz, want_db) in zip(arr, jobs):
        R, K = x.shape
        C_ = dz.shape[1]
        dw = torch.empty(K, C_, device=x.device, dtype=F32)
        db = torch.empty(C_, device=x.device, dtype=F32) if want_db else None
        j.x, j.ldx, j.dz, j.R, j.K, j.C, j.dw, j.db = x.data_ptr(), x.stride(0), dz.data_ptr(), R, K, C_, dw.data_ptr(), (db.data_ptr() if want_db else None)
        outs.append((dw, db))
    check(lib().pn_dense_wgrad_batch(arr, len(jobs), current_stream()), "pn_dense_wgrad_batch")
    return outs


def dense_bwd(da, z, x, gamma=None, beta=None, mean=None, invstd=None, bn_mode=0, act=0, keep=None, rate=0.0, want_dw=True):
    """backward of the layer tail + parameters: returns (dz, dgamma, dbeta, dbias, dw)"""
    R, C_ = da.shape
    K = x.shape[1]
    dev = da.device
    dz = torch.empty(R, C_, device=dev, dtype=F32)
    dg = torch.zeros(C_, device=dev, dtype=F32); db = torch.zeros(C_, device=dev, dtype=F32); dbias = torch.zeros(C_, device=dev, dtype=F32)
    dw = torch.empty(K, C_, device=dev, dtype=F32) if want_dw else None
    check(lib().pn_dense_bwd(ptr(da), ptr(z), ptr(x), x.stride(0), R, K, C_, ptr(gamma), ptr(beta), ptr(mean), ptr(invstd), bn_mode, act,
                             ptr(keep), 1.0 / (1.0 - rate), ptr(dz), ptr(dg), ptr(db), ptr(dbias), ptr(dw), current_stream()), "pn_dense_bwd")
    return dz, dg, db, dbias, dw
