#!/usr/bin/env python3
"""BASELINE config 5: dense LiDAR scan N=131072 -> voxel-grid (0.25 m) -> FPS (M=8192) -> PointNet inference, one MI355X.

Synthetic scan: 95 % of the points on the hull of the reference's kc-46 cloud (each reference
point replicated with N(0, 0.15 m) noise), 5 % uniform outliers in the bounding box.  Prints one JSON line with the
time of every stage (HIP events on the launch stream), then the
propagation of the samples' segmentation probabilities back onto all N points (k = 3 nearest samples, pn_knn_propagate) and
PointNet.predict_scan end to end, then the label-constrained ICP (ops.semantic_icp) of the labelled kc-46 reference against a
labelled C5-size scan of it under a known pose, from a start about 10 degrees and 1 m off, and PointNet.predict_pose end to end;
then point-to-plane ICP (ops.icp_normals + semantic_icp(metric="plane")): its iteration at C5 against kc-46, and both metrics on a
surface-sampled scene (the labelled analytic aircraft of tests/icp_plane_oracle.py: 3,000 reference samples, 60,000 independent
scan samples with 2 cm noise, the same true pose and start), where copying reference points no longer favours point to point;
then ICP against a triangle mesh (ops.icp_mesh_reference: the procedural aircraft of tests/icp_mesh_oracle.py at three subdivision
levels, scans of 60,000 and of --points surface samples with 2 cm noise): the iteration and the triangle tests per second of both
metrics, their iterations and final pose error, and in the same run the point path against M = T points sampled from the same
mesh (--mesh-only runs this section alone, e.g. under rocprofv3 --kernel-trace --stats for the per-kernel split);
then the global start (ops.global_pose: 256 + 1 seeds, the best 4 refined) on a labelled C5-size scan of kc-46 turned by 150
degrees: the time of the moments, the seeds, the scoring, the refinement and the selection, and as the scorer's yardstick one
pn_icp_correspond call per seed on the same strided sample (--global-only runs this section alone);
then the LiDAR simulator (ops.lidar_cast + ops.lidar_pack): 32 look-at poses x 128 x 128 rays against the aircraft mesh at level 3
(5,120 triangles), packed to 2,048 points per frame: milliseconds per launch and ray-triangle tests per second, and the cast
through the per-part trees (ops.lidar_cast(accel="bvh")) against the brute-force cast on the same frames at levels 3 and 5 (5,120
and 81,920 triangles), measured alternately in one run, medians of 5, with the host build of the trees (--lidar-only runs this
section alone); the sensor model between the two (ops.lidar_sense, all stages on) on the same frames, timed beside both casts and the
pack, and its launch as a share of cast + pack (--sensor-only runs this section alone);
then the mesh sampler (ops.mesh_sample on the aircraft mesh at level 3: one set of 8,192 and 32 sets of 2,048 points, per call
over a loop of calls, and as its yardstick the same stratified draw written with torch ops: cumsum, rand, searchsorted, gathers)
and ops.global_pose against that mesh with the vertex score and with a sampled score cloud (--sample-only runs this section alone);
then the robust, confidence-weighted ICP (ops.semantic_icp(robust=...)) on labelled --points scans with a fifth of the labels
replaced by another part, against kc-46 (both metrics) and against the aircraft mesh at level 3 (plane): the iteration of the
unweighted loop, of the Tukey loop with a fixed scale and of the Tukey loop with the automatic (median) scale, and where each
loop ends (--robust-only runs this section alone, e.g. under rocprofv3 --kernel-trace --stats for the per-kernel split);
then the mesh ICP through the per-part trees (ops.icp_mesh_reference(accel="bvh")) against the brute-force search on the same
mesh, at levels 3 and 5 (5,120 and 81,920 triangles), 60,000 and --points scan points, both metrics: the two iterations measured
alternately in one run, medians of 5, and the host build of the trees (--bvh-only runs this section alone);
then the voxel connected components (ops.voxel_clusters, 26-connectivity) on the C5 scan plus 2 % strays scattered uniformly over a
box 40 m wider than the scan on every side, at leaf 0.25 and 1.0: the call, ops.voxel_downsample on the same input and leaf in the
same run (it shares the sort and so is the yardstick), the two raw C entries on preallocated buffers without their host reads, and
predict_scan with and without isolate="largest" (--cluster-only runs this section alone).
--grid-only runs the voxel-grid cloud ICP section alone (it is not part of the default run): --points scan points against
mesh-sampled references of 2,048 / 16,384 / 131,072 points through ops.icp_reference(accel="grid") and by brute force, alternately
in one run, with the build of the tables and one ops.register_scans call end to end (e.g. under rocprofv3 --kernel-trace --stats
for the per-kernel split; --parent-lib times the brute-force pass of another build of the library on the same buffers).
--fpfh-only runs the start of an unlabelled registration alone (it is not part of the default run either): ops.fpfh beside
ops.estimate_normals' entry, ops.feature_match beside torch.cdist, ops.ransac_poses and one ops.global_register call.
--dbscan-only runs the exact DBSCAN section alone (not part of the default run either): raw pn_dbscan on the --cluster-only scene at
eps 0.25 and 0.5, min_points 8, beside raw pn_voxel_cluster at leaf = eps and the count-only pn_radius_knn (k = 0) at radius = eps
on the same input in the same run (e.g. under rocprofv3 --kernel-trace --stats for the per-kernel split).
--gicp-only runs the plane-to-plane (generalized ICP) section alone (not part of the default run either): two independent samplings
of the aircraft mesh of --points and of 16,384 points each, one plane-to-plane iteration and pass beside the plane metric's on the
same grid reference, alternately in one run, and one ops.register_scans call per metric end to end with its iterations and errors
(e.g. under rocprofv3 --kernel-trace --stats for the sums launch alone).
--recon-only runs the surface reconstruction section alone (not part of the default run either): pn_recon_field, pn_recon_count and
pn_recon_emit on the C5 scan at voxel 0.5 and 0.25 (radius = 3 voxels), beside the count-only pn_radius_knn at the same radius and
pn_voxel_downsample at leaf = voxel on the same cloud in the same run, with the lattice, its valid share, the vertices and faces.
--simplify-only runs the mesh cleaning section alone (not part of the default run either): pn_mesh_components and pn_mesh_simplify
(both placements, leaf 0.5 and 1.0) on the C5 reconstruction at voxel 0.25, beside pn_voxel_downsample over the mesh's vertices and
pn_recon_emit of the same mesh in the same run, the face counts, the distance from the full mesh to the simplified one, and one
brute-force robust mesh-ICP iteration on either.
The same pipeline is checked bit for bit against the NumPy oracle by
tests/test_gpu_ops.py::test_scan_pipeline_c5_matches_oracle (the oracle is test infrastructure: nothing here imports it)."""
import argparse
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_scan(n, seed=20260005):
    rng = np.random.default_rng(seed)
    pts = []
    for line in open(os.path.join(ROOT, "tests", "golden", "kc-46.txt")):
        m = re.match(r"\(([^)]*)\)", line.strip())
        pts.append([float(v) for v in m.group(1).split(",")])
    ref = np.asarray(pts, dtype=np.float32)
    n_hull = int(0.95 * n)
    hull = ref[rng.integers(0, len(ref), n_hull)] + rng.normal(0, 0.15, size=(n_hull, 3)).astype(np.float32)
    lo, hi = ref.min(0) - 1, ref.max(0) + 1
    out = rng.uniform(lo, hi, size=(n - n_hull, 3)).astype(np.float32)
    xyz = np.concatenate([hull, out]).astype(np.float32)
    rng.shuffle(xyz)
    return xyz, lo.astype(np.float32)


PARTS = ["wing", "fuselage", "engine", "hstab", "vstab", "landing_gear", "armament", "boom_wing", "boom_hull", "boom_hose", "dish",
         "probe"]                                   # f15_lidar_config.json part labels


def rot(axis, angle):
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def make_labelled_scan(n, ref, part, pose, seed=20260006):
    """95 % reference points under ``pose`` with N(0, 0.05 m) noise and their part labels, 5 % uniform outliers labelled -1"""
    rng = np.random.default_rng(seed)
    n_hull = int(0.95 * n)
    pick = rng.integers(0, len(ref), n_hull)
    p = ref[pick].astype(np.float64) @ pose[:3, :3].T + pose[:3, 3] + rng.normal(0, 0.05, size=(n_hull, 3))
    o = rng.uniform(p.min(0) - 1, p.max(0) + 1, size=(n - n_hull, 3))
    lab = np.concatenate([part[pick], np.full(n - n_hull, -1)]).astype(np.int32)
    perm = rng.permutation(n)
    return np.concatenate([p, o]).astype(np.float32)[perm], lab[perm]


def timed(fn, reps):
    out, ts = None, []
    for rep in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        if rep:
            ts.append(e0.elapsed_time(e1))
    return out, float(np.median(ts))


def iter_ms(S, L, ref, I, reps, **kw):
    """time of one iteration that runs: (30 forced iterations - 1) / 29"""
    from pointcloudprocessing_amd import ops
    _, one = timed(lambda: ops.semantic_icp(S, L, ref, I, max_iters=1, **kw), reps)
    _, full = timed(lambda: ops.semantic_icp(S, L, ref, I, max_iters=30, tol_rot=0.0, tol_t=0.0, **kw), reps)
    return (full - one) / 29


def bench_icp_plane(args, dev):
    """point to plane: the iteration at C5 against kc-46 (normals k = 10), and both metrics on the surface-sampled scene"""
    import importlib.util
    from pointcloudprocessing_amd import ops, pointcloud
    spec = importlib.util.spec_from_file_location("icp_plane_oracle", os.path.join(ROOT, "tests", "icp_plane_oracle.py"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    po = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(po)                               # the scene generator only
    kx, kp = pointcloud.read_labelled_cloud(os.path.join(ROOT, "tests", "golden", "kc-46.txt"), PARTS)
    _, _, kref = ops.icp_normals(ops.icp_reference(kx, kp, len(PARTS), device=dev), k=10)
    scan, lab = make_labelled_scan(args.points, kx, kp, po.TRUE_POSE)
    S, L, I = (torch.from_numpy(a).to(dev) for a in (scan[None], lab[None], po.START_POSE[None]))
    out = {"icp_plane_iter_ms_c5": iter_ms(S, L, kref, I, args.reps, metric="plane")}
    ref, part, scan, lab = po.aircraft_scene()
    r = ops.icp_reference(ref, part, len(po.AIRCRAFT_PARTS), device=dev)
    _, normals_ms = timed(lambda: ops.icp_normals(r, k=10), args.reps)
    _, _, r = ops.icp_normals(r, k=10)
    S, L = torch.from_numpy(scan[None]).to(dev), torch.from_numpy(lab[None]).to(dev)
    out.update({"surface_normals_ms": normals_ms, "surface_plane_iter_ms": iter_ms(S, L, r, I, args.reps, metric="plane"),
                "surface_point_iter_ms": iter_ms(S, L, r, I, args.reps)})
    true = po.TRUE_POSE
    for metric, iters in (("plane", 30), ("point", 15), ("point", 200)):
        (pose, rmse, pairs, it, st), ms = timed(lambda: ops.semantic_icp(S, L, r, I, max_iters=iters, metric=metric), args.reps)
        pose = pose.cpu().numpy()[0]
        ang = float(np.arccos(np.clip((np.trace(pose[:3, :3].T @ true[:3, :3]) - 1) / 2, -1, 1)))
        out[f"surface_{metric}_{iters}"] = {"iters": int(it[0]), "status": int(st[0]), "ms": ms, "error_deg": float(np.rad2deg(ang)),
                                            "error_m": float(np.linalg.norm(pose[:3, 3] - true[:3, 3])), "rmse_m": float(rmse[0])}
    return out


def _test_module(name):
    import importlib.util
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def bench_icp_mesh(args, dev, levels=(1, 2, 3)):
    """point to triangle against the aircraft mesh, and the point path at equal primitive count (M = T sampled points)"""
    from pointcloudprocessing_amd import ops
    mo, po = _test_module("icp_mesh_oracle"), _test_module("icp_plane_oracle")      # the mesh and scene generators only
    true, I = po.TRUE_POSE, torch.from_numpy(po.START_POSE[None]).to(dev)
    n_parts = len(mo.MESH_PARTS)

    def err(pose):
        pose = pose.cpu().numpy()[0]
        ang = float(np.arccos(np.clip((np.trace(pose[:3, :3].T @ true[:3, :3]) - 1) / 2, -1, 1)))
        return ang, float(np.linalg.norm(pose[:3, 3] - true[:3, 3]))

    out = {}
    for level in levels:
        v, f, p = mo.aircraft_mesh(level)
        mesh = ops.icp_mesh_reference(v, f, p, n_parts, device=dev)
        rx, rp, _ = mo.sample_surface(v, f, p, mesh.T, seed=7)
        cloud = ops.icp_reference(rx.astype(np.float32), rp, n_parts, device=dev)
        for n in (60000, args.points):
            scan, lab = mo.mesh_scan(v, f, p, n, true, noise=0.02, seed=1)
            S, L = torch.from_numpy(scan[None]).to(dev), torch.from_numpy(lab[None]).to(dev)
            tseg, cseg = np.diff(np.asarray(mesh.seg)), np.diff(np.asarray(cloud.seg))
            tests, pairs = int(tseg[lab].sum()), int(cseg[lab].sum())        # same-label primitives of one pass
            r = {"T": mesh.T, "N": n}
            for metric in ("plane", "point"):
                ms = iter_ms(S, L, mesh, I, args.reps, metric=metric)
                (pose, rmse, _, it, st), _ = timed(lambda: ops.semantic_icp(S, L, mesh, I, max_iters=30, metric=metric), 1)
                ang, dt = err(pose)
                r[f"mesh_{metric}"] = {"iter_ms": ms, "tests_per_s": tests / (ms * 1e-3), "iters": int(it[0]), "status": int(st[0]),
                                       "error_rad": ang, "error_m": dt, "rmse_m": float(rmse[0])}
            ms = iter_ms(S, L, cloud, I, args.reps)
            (pose, rmse, _, it, st), _ = timed(lambda: ops.semantic_icp(S, L, cloud, I, max_iters=30), 1)
            ang, dt = err(pose)
            r["cloud_point"] = {"M": cloud.M, "iter_ms": ms, "pairs_per_s": pairs / (ms * 1e-3), "iters": int(it[0]),
                                "status": int(st[0]), "error_rad": ang, "error_m": dt, "rmse_m": float(rmse[0])}
            r["mesh_over_cloud_per_primitive"] = (r["mesh_point"]["iter_ms"] / tests) / (ms / pairs)
            out[f"mesh_T{mesh.T}_N{n}"] = r
    return out


def bench_bvh(args, dev, levels=(3, 5), iters=6, rounds=5):
    """the mesh iteration through the per-part trees (ops.icp_mesh_reference(accel="bvh")) against the brute-force iteration on
    the same grouped mesh, from the 10 degree / 1 m start: one accelerated and one brute-force measurement alternate ``rounds``
    times after a warm-up round, the medians are reported; an iteration is (``iters`` forced iterations - 1 iteration) /
    (iters - 1).  Also the host build of the trees (pn_icp_bvh_build alone, median of 3) and whether both loops end on the
    same bytes."""
    import time
    from pointcloudprocessing_amd import ops
    mo, po = _test_module("icp_mesh_oracle"), _test_module("icp_plane_oracle")      # the mesh and scene generators only
    true, I = po.TRUE_POSE, torch.from_numpy(po.START_POSE[None]).to(dev)
    n_parts = len(mo.MESH_PARTS)

    def once(S, L, ref, n, metric):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        ops.semantic_icp(S, L, ref, I, max_iters=n, tol_rot=0.0, tol_t=0.0, metric=metric)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    out = {}
    for level in levels:
        v, f, p = mo.aircraft_mesh(level)
        plain = ops.icp_mesh_reference(v, f, p, n_parts, device=dev)
        acc = ops.icp_mesh_reference(v, f, p, n_parts, device=dev, accel="bvh")
        tri_host, build = plain.tri.cpu().numpy(), []
        for _ in range(3):
            t0 = time.perf_counter()
            ops._build_bvh(tri_host, plain.seg, n_parts)
            build.append((time.perf_counter() - t0) * 1e3)
        for n in (60000, args.points):
            scan, lab = mo.mesh_scan(v, f, p, n, true, noise=0.02, seed=1)
            S, L = torch.from_numpy(scan[None]).to(dev), torch.from_numpy(lab[None]).to(dev)
            r = {"T": plain.T, "N": n, "nodes": acc.n_nodes, "build_ms": float(np.median(build))}
            for metric in ("plane", "point"):
                ts = {"bvh": [], "brute": []}
                for rnd in range(rounds + 1):
                    for name, ref in (("bvh", acc), ("brute", plain)):
                        one, full = once(S, L, ref, 1, metric), once(S, L, ref, iters, metric)
                        if rnd:
                            ts[name].append((full - one) / (iters - 1))
                a = ops.semantic_icp(S, L, acc, I, max_iters=30, metric=metric)
                b = ops.semantic_icp(S, L, plain, I, max_iters=30, metric=metric)
                bvh_ms, brute_ms = float(np.median(ts["bvh"])), float(np.median(ts["brute"]))
                r[metric] = {"bvh_iter_ms": bvh_ms, "brute_iter_ms": brute_ms, "speedup": brute_ms / bvh_ms, "iters": int(a[3][0]),
                             "same_bytes": all(torch.equal(x, y) for x, y in zip(a, b))}
            out[f"bvh_T{plain.T}_N{n}"] = r
    return out


def bench_grid(args, dev, level=3, sizes=(2048, 16384, 131072), max_dist=0.5, iters=6, rounds=5):
    """the cloud search through the voxel grid (ops.icp_reference / mesh_sample_reference(accel="grid")) against the brute-force
    search on the same grouped cloud: --points surface samples of the aircraft mesh (2 cm noise) against mesh-sampled references of
    ``sizes`` points, with one part and with the labelled aircraft, at ``max_dist``.  Per shape: the single pass with the 18 sums
    (pn_icp_grid_correspond / pn_icp_correspond) at the true pose, where a loop spends its iterations, and the loop's iteration
    from 5 degrees / 0.3 m off ((``iters`` forced iterations - 1 iteration) / (iters - 1), plane metric); grid and brute force
    alternate ``rounds`` times after a warm-up round, medians reported, HIP events on the launch stream.  --parent-lib PATH times
    pn_icp_correspond of another build of the library (the parent commit's) on the same buffers in the same rounds.  Also the
    build of the tables (device launches between events, and the set-up call with its host read, wall clock), whether both loops
    end on the same bytes, and one ops.register_scans call end to end (wall clock, normals and tables included)."""
    import ctypes as C
    import time
    from pointcloudprocessing_amd import _lib, ops
    mo, po = _test_module("icp_mesh_oracle"), _test_module("icp_plane_oracle")      # the mesh and scene generators only
    true = po.TRUE_POSE
    start = true.copy()
    start[:3, :3] = rot([1, -1, 0], np.deg2rad(5.0)) @ true[:3, :3]
    start[:3, 3] += [0.1, -0.2, 0.2]
    I, T32 = torch.from_numpy(start[None]).to(dev), torch.from_numpy(true[None].astype(np.float32)).to(dev)
    v, f, p = mo.aircraft_mesh(level)
    parent = None
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        parent.pn_icp_workspace_bytes.restype = C.c_size_t
        parent.pn_icp_workspace_bytes.argtypes = [C.c_int] * 4
        parent.pn_icp_correspond.restype = C.c_int
        parent.pn_icp_correspond.argtypes = _lib.SIGNATURES["pn_icp_correspond"][1]

    def ev(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    out = {"N": args.points, "max_dist": max_dist, "mesh_T": len(f)}
    for tag, labels, n_parts in (("one_part", np.zeros(len(f), np.int32), 1), ("labelled", p, len(mo.MESH_PARTS))):
        mesh = ops.icp_mesh_reference(v, f, labels, n_parts, device=dev)
        scan, lab = mo.mesh_scan(v, f, labels, args.points, true, noise=0.02, seed=1)
        S, L = torch.from_numpy(scan[None]).to(dev), torch.from_numpy(lab[None].astype(np.int32)).to(dev)
        B, N = 1, args.points
        for M in sizes:
            plain = ops.mesh_sample_reference(mesh, M, seed=1)
            acc = ops.mesh_sample_reference(mesh, M, seed=1, accel="grid", max_dist=max_dist)
            build_dev, build_wall = [], []
            nb, nw = _lib.lib().pn_icp_grid_bytes(plain.M), _lib.lib().pn_icp_grid_build_workspace_bytes(plain.M)
            gbuf, wbuf = torch.empty(nb, device=dev, dtype=torch.uint8), torch.empty(nw, device=dev, dtype=torch.uint8)
            o3 = (C.c_float * 3)(*acc.origin)
            for rnd in range(rounds + 1):
                t = ev(lambda: _lib.check(_lib.lib().pn_icp_grid_build(_lib.ptr(plain.xyz), plain.M, acc.r2, o3, _lib.ptr(gbuf), nb, _lib.ptr(wbuf), nw,
                                                                        _lib.current_stream()), "pn_icp_grid_build"))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ops._with_grid("bench", plain, max_dist)
                torch.cuda.synchronize()
                if rnd:
                    build_dev.append(t)
                    build_wall.append((time.perf_counter() - t0) * 1e3)
            r = {"M": plain.M, "n_parts": n_parts, "voxels": int(acc.grid[:4].view(torch.int32).item()), "build_launches_ms": float(np.median(build_dev)),
                 "build_call_wall_ms": float(np.median(build_wall)), "tables_bytes": nb}
            pws = None
            if parent is not None:
                pbytes = parent.pn_icp_workspace_bytes(B, N, plain.M, n_parts)
                pws = torch.empty(pbytes, device=dev, dtype=torch.uint8)
                pidx, pd2 = torch.empty(B, N, device=dev, dtype=torch.int32), torch.empty(B, N, device=dev)
                psum = torch.empty(B, 18, device=dev, dtype=torch.float64)

                def parent_pass():
                    rc = parent.pn_icp_correspond(_lib.ptr(S), _lib.ptr(L), B, N, _lib.ptr(plain.xyz), plain._seg_c, plain.M, n_parts, _lib.ptr(T32),
                                                  ops._max_d2(max_dist), _lib.ptr(pidx), _lib.ptr(pd2), _lib.ptr(psum), _lib.ptr(pws), pbytes,
                                                  _lib.current_stream())
                    assert rc == 0, rc
            ts = {"grid_pass": [], "brute_pass": [], "parent_pass": [], "grid_iter": [], "brute_iter": []}
            for rnd in range(rounds + 1):
                for name, ref in (("grid", acc), ("brute", plain)):
                    t = ev(lambda: ops.icp_correspond(S, L, ref, T32, max_dist=max_dist, sums=True))
                    kw = dict(max_dist=max_dist, tol_rot=0.0, tol_t=0.0, metric="plane")
                    one = ev(lambda: ops.semantic_icp(S, L, ref, I, max_iters=1, **kw))
                    full = ev(lambda: ops.semantic_icp(S, L, ref, I, max_iters=iters, **kw))
                    if rnd:
                        ts[name + "_pass"].append(t)
                        ts[name + "_iter"].append((full - one) / (iters - 1))
                if parent is not None:
                    t = ev(parent_pass)
                    if rnd:
                        ts["parent_pass"].append(t)
            a = ops.semantic_icp(S, L, acc, I, max_iters=30, max_dist=max_dist, metric="plane")
            b = ops.semantic_icp(S, L, plain, I, max_iters=30, max_dist=max_dist, metric="plane")
            (gi, gd, gs), (bi, bd, bs) = (ops.icp_correspond(S, L, x, T32, max_dist=max_dist, sums=True) for x in (acc, plain))
            r.update({k + "_ms": float(np.median(t)) for k, t in ts.items() if t})
            r.update({"pass_speedup": r["brute_pass_ms"] / r["grid_pass_ms"], "iter_speedup": r["brute_iter_ms"] / r["grid_iter_ms"],
                      "pairs_within_max_dist": int((gi >= 0).sum()), "iters": int(a[3][0]), "loops_same_bytes": all(torch.equal(x, y) for x, y in zip(a, b)),
                      "pass_same_idx_and_sums": bool(torch.equal(gi, bi) and torch.equal(gs, bs))})
            if parent is not None:
                r["pass_speedup_vs_parent"] = r["parent_pass_ms"] / r["grid_pass_ms"]
                r["parent_same_idx_and_sums"] = bool(torch.equal(pidx, bi) and torch.equal(psum, bs))
            out[f"grid_{tag}_M{plain.M}"] = r
    # scan to scan, end to end: two independent samplings of --points points each, the source moved by 1 degree / 10 cm, 2 cm noise
    mesh = ops.icp_mesh_reference(v, f, p, len(mo.MESH_PARTS), device=dev)
    target = ops.mesh_sample(mesh, args.points, seed=11)[0][0].contiguous()
    src = ops.mesh_sample(mesh, args.points, seed=12)[0][0].double()
    move = np.eye(4)
    move[:3, :3] = rot([1, 2, -1], np.deg2rad(1.0))
    move[:3, 3] = [0.06, -0.05, 0.06]
    gen = torch.Generator(device="cpu").manual_seed(5)
    noise = torch.randn(src.shape, generator=gen, dtype=torch.float64).to(dev) * 0.02
    source = (src @ torch.from_numpy(move[:3, :3].T.copy()).to(dev) + torch.from_numpy(move[:3, 3].copy()).to(dev) + noise).float().contiguous()
    walls = {}
    for accel in ("grid", None):
        w = []
        for rnd in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = ops.register_scans(source, target, max_dist, accel=accel)
            torch.cuda.synchronize()
            w.append((time.perf_counter() - t0) * 1e3)
        pose = res[0][0].cpu().numpy()
        M_ = pose[:3, :3].T @ move[:3, :3]
        ang = float(np.arccos(np.clip((np.trace(M_) - 1) / 2, -1, 1)))
        walls[str(accel)] = {"wall_ms": float(np.median(w[1:])), "first_call_wall_ms": w[0], "iters": int(res[3][0]), "pairs": int(res[2][0]),
                             "error_deg": float(np.rad2deg(ang)), "error_m": float(np.linalg.norm(pose[:3, 3] - move[:3, 3]))}
    out["register_scans"] = {"N": args.points, "M": args.points, **walls}
    return out


def bench_gicp(args, dev, level=3, max_dist=0.5, iters=6, rounds=5):
    """plane to plane (ops.semantic_icp(metric="gicp")) beside the plane metric, scan against scan: two independent samplings of the
    aircraft mesh of N points each (N = --points and 16,384), the source moved by 1 degree / 10 cm with 2 cm noise, both searched
    through the target's voxel grid at ``max_dist``, normals at radius ``max_dist`` and k = 8.  Per size: the iteration of either
    loop from the identity ((``iters`` forced iterations - 1 iteration) / (iters - 1)) and the single pass at the true pose
    (pn_icp_gicp_sums / pn_icp_grid_correspond mode 2), the two metrics alternating ``rounds`` times after a warm-up round, medians,
    HIP events on the launch stream; the source normals alone; and one ops.register_scans call per metric end to end (wall clock:
    normals of both clouds, the tables and the loop) with its iterations and final errors."""
    import time
    from pointcloudprocessing_amd import ops
    mo = _test_module("icp_mesh_oracle")                                            # the mesh generator only
    v, f, p = mo.aircraft_mesh(level)
    mesh = ops.icp_mesh_reference(v, f, p, len(mo.MESH_PARTS), device=dev)
    move = np.eye(4)
    move[:3, :3] = rot([1, 2, -1], np.deg2rad(1.0))
    move[:3, 3] = [0.06, -0.05, 0.06]

    def ev(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    out = {"max_dist": max_dist, "mesh_T": len(f)}
    for n in sorted({int(args.points), 16384}, reverse=True):
        target = ops.mesh_sample(mesh, n, seed=11)[0][0].contiguous()
        src = ops.mesh_sample(mesh, n, seed=12)[0][0].double()
        gen = torch.Generator(device="cpu").manual_seed(5)
        noise = torch.randn(src.shape, generator=gen, dtype=torch.float64).to(dev) * 0.02
        source = (src @ torch.from_numpy(move[:3, :3].T.copy()).to(dev) + torch.from_numpy(move[:3, 3].copy()).to(dev) + noise).float().contiguous()
        ref = ops._scan_reference("bench_scan", target, max_dist, "gicp", None, 8, None, "grid")
        S, L = source.unsqueeze(0), torch.zeros(1, n, device=dev, dtype=torch.int32)
        SN = ops.estimate_normals(source, max_dist, 8)[0].unsqueeze(0)
        I = torch.eye(4, device=dev, dtype=torch.float64).unsqueeze(0)
        T = torch.from_numpy(move[None]).to(dev)
        metrics = {"plane": dict(metric="plane"), "gicp": dict(metric="gicp", scan_normals=SN)}
        passes = {"plane": lambda: ops.icp_plane_sums(S, L, ref, T, max_dist), "gicp": lambda: ops.icp_gicp_sums(S, L, SN, ref, T, max_dist)}
        ts = {f"{m}_{w}": [] for m in metrics for w in ("pass", "iter")}
        ts["source_normals"] = []
        for rnd in range(rounds + 1):
            for m, kw in metrics.items():
                t = ev(passes[m])
                loop = dict(max_dist=max_dist, tol_rot=0.0, tol_t=0.0, **kw)
                one = ev(lambda: ops.semantic_icp(S, L, ref, I, max_iters=1, **loop))
                full = ev(lambda: ops.semantic_icp(S, L, ref, I, max_iters=iters, **loop))
                if rnd:
                    ts[m + "_pass"].append(t)
                    ts[m + "_iter"].append((full - one) / (iters - 1))
            t = ev(lambda: ops.estimate_normals(source, max_dist, 8))
            if rnd:
                ts["source_normals"].append(t)
        r = {"N": n, "M": ref.M, **{k + "_ms": float(np.median(t)) for k, t in ts.items()}}
        r["iter_gicp_over_plane"] = r["gicp_iter_ms"] / r["plane_iter_ms"]
        r["source_normals_valid"] = float(torch.isfinite(SN).all(-1).float().mean())
        for m in metrics:
            w = []
            for rnd in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = ops.register_scans(source, target, max_dist, metric=m)
                torch.cuda.synchronize()
                w.append((time.perf_counter() - t0) * 1e3)
            pose = res[0][0].cpu().numpy()
            M_ = pose[:3, :3].T @ move[:3, :3]
            ang = float(np.arccos(np.clip((np.trace(M_) - 1) / 2, -1, 1)))
            r["register_scans_" + m] = {"wall_ms": float(np.median(w[1:])), "first_call_wall_ms": w[0], "iters": int(res[3][0]), "pairs": int(res[2][0]),
                                        "status": int(res[4][0]), "rmse_m": float(res[1][0]), "error_deg": float(np.rad2deg(ang)),
                                        "error_m": float(np.linalg.norm(pose[:3, 3] - move[:3, 3]))}
        out[f"gicp_N{n}"] = r
    return out


def bench_multiway(args, dev, level=3, K=8, n=16384, max_dist=0.5, rounds=5):
    """multiway registration (ops.multiway_register): ``K`` independent samplings of the aircraft mesh of ``n`` points each, cloud i seen
    from a frame 1 degree and about 9 cm from its neighbour's, every pair an edge (K (K - 1) / 2), the plane metric through the
    targets' grids at ``max_dist``.  The whole call (wall clock, the second of two calls) and its parts: the edge registrations (one
    register_scans call per target, wall clock, summed), pn_icp_information beside pn_icp_grid_correspond without sums on the same
    input (the 7 sources of the last target; HIP events, medians of ``rounds``), and pn_pose_graph_optimize on the call's own graph
    (K, E) = (8, 28) and on the oracle's noisy graph (64, 300), beside the NumPy oracle on the host."""
    import time
    from pointcloudprocessing_amd import ops
    mo, pg = _test_module("icp_mesh_oracle"), _test_module("pose_graph_oracle")
    v, f, p = mo.aircraft_mesh(level)
    mesh = ops.icp_mesh_reference(v, f, p, len(mo.MESH_PARTS), device=dev)
    xyz = ops.mesh_sample(mesh, n, seed=31, sets=K)[0].double()
    step = np.eye(4)
    step[:3, :3] = rot([1, 2, -1], np.deg2rad(1.0))
    step[:3, 3] = [0.06, -0.05, 0.06]
    truth = [np.eye(4)]
    for _ in range(K - 1):
        truth.append(truth[-1] @ step)
    clouds = []
    for i in range(K):
        Xi = torch.from_numpy(pg.inv(truth[i])).to(dev)
        clouds.append((xyz[i] @ Xi[:3, :3].T + Xi[:3, 3]).float().contiguous())

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    def ev(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    _, first = wall(lambda: ops.multiway_register(clouds, max_dist, edges="all"))
    res, whole = wall(lambda: ops.multiway_register(clouds, max_dist, edges="all"))
    poses, cost, iters, status, edges, Z, info, pairs = res
    e = edges.numpy()
    init = torch.from_numpy(np.stack(truth)).to(dev)
    reg = 0.0
    for j in range(1, K):
        src = torch.stack(clouds[:j])
        start = ops._rigid_inverse(init[:j]) @ init[j]
        reg += wall(lambda: ops.register_scans(src, clouds[j], max_dist, init_pose=start))[1]
    src = torch.stack(clouds[:K - 1])
    L = torch.zeros(K - 1, n, device=dev, dtype=torch.int32)
    ref = ops._scan_reference("bench_scan", clouds[K - 1], max_dist, "point", None, 8, None, "grid")
    Zl = Z[torch.from_numpy(np.flatnonzero(e[:, 1] == K - 1)).to(dev)].contiguous()
    ts = {"information": [], "grid_correspond": []}
    for rnd in range(rounds + 1):
        a = ev(lambda: ops.icp_information(src, L, ref, Zl, max_dist))
        b = ev(lambda: ops.icp_correspond(src, L, ref, Zl.float(), max_dist))
        if rnd:
            ts["information"].append(a)
            ts["grid_correspond"].append(b)
    err = max(float(np.abs(poses[i].cpu().numpy() - truth[i]).max()) for i in range(K))
    out = {"K": K, "N": n, "E": len(e), "max_dist": max_dist, "whole_call_wall_ms": whole, "first_call_wall_ms": first,
           "edge_registrations_wall_ms": reg, "information_ms": float(np.median(ts["information"])),
           "grid_correspond_ms": float(np.median(ts["grid_correspond"])), "graph_cost": [float(cost[0]), float(cost[1])],
           "graph_iters": int(iters[0]), "graph_status": int(status[0]), "worst_pose_entry_error": err,
           "min_pairs": int(pairs.min())}
    g = pg.graph(64, 300)
    big = tuple(torch.from_numpy(np.array(g[k])).to(dev) for k in ("Z", "info", "start"))
    start8 = poses.clone()
    start8[1:] = init[1:]
    for name, ed, args_, host in (("8_28", e, (Z, info, start8), (K, e, Z.cpu().numpy(), info.cpu().numpy(), start8.cpu().numpy())),
                                  ("64_300", np.array(g["edges"]), big, (64, g["edges"], g["Z"], g["info"], g["start"]))):
        ed_t = torch.from_numpy(np.ascontiguousarray(ed))
        t = [ev(lambda: ops.pose_graph_optimize(ed_t, *args_)) for _ in range(rounds + 1)][1:]
        r = ops.pose_graph_optimize(ed_t, *args_)
        t0 = time.perf_counter()
        o = pg.optimize(*host)
        out["pose_graph_" + name] = {"ms": float(np.median(t)), "iters": int(r[2][0]), "status": int(r[3][0]),
                                     "oracle_host_ms": (time.perf_counter() - t0) * 1e3, "oracle_iters": int(o[2]),
                                     "device_minus_oracle": float(np.abs(r[0].cpu().numpy() - o[0]).max())}
    return out


def bench_global(args, dev, K=256, top=4):
    """the global start at C5: --points points, kc-46, K + 1 seeds, the best ``top`` refined; every stage of ops.global_pose
    timed on its own, and the scorer's yardstick: one pn_icp_correspond call per seed on the same strided sample"""
    import ctypes as C
    from pointcloudprocessing_amd import _lib, ops, pointcloud
    kx, kp = pointcloud.read_labelled_cloud(os.path.join(ROOT, "tests", "golden", "kc-46.txt"), PARTS)
    ref = ops.icp_reference(kx, kp, len(PARTS), device=dev)
    rng = np.random.default_rng(20260007)
    true = np.eye(4)
    true[:3, :3] = rot(rng.normal(size=3), np.deg2rad(150))
    true[:3, 3] = rng.uniform(-30, 30, 3)
    scan, lab = make_labelled_scan(args.points, kx, kp, true)
    S, L = torch.from_numpy(scan[None]).to(dev), torch.from_numpy(lab[None]).to(dev)
    N, max_dist, stride = args.points, 3.0, max(1, args.points // 8192)
    R = ops.rotation_grid(K).to(dev)
    rmom = ops.icp_part_moments(ref)
    mom, moments_ms = timed(lambda: ops.part_moments(S, L, ref.n_parts), args.reps)
    seeds, seeds_ms = timed(lambda: ops.icp_seed_poses(mom, rmom, R), args.reps)
    (score, order), score_ms = timed(lambda: ops.icp_score_poses(S, L, ref, seeds, max_dist, stride), args.reps)
    start = seeds[0, order[0, :top].long()].contiguous()
    rs, rl = S.repeat_interleave(top, 0), L.repeat_interleave(top, 0)
    refined, refine_ms = timed(lambda: ops.semantic_icp(rs, rl, ref, start, max_dist=max_dist, max_iters=30), args.reps)
    _, select_ms = timed(lambda: ops.icp_score_poses(S, L, ref, refined[0].reshape(1, top, 4, 4), max_dist, 1), args.reps)
    (pose, _, _, iters, _, cost, winner), total_ms = timed(
        lambda: ops.global_pose(S, L, ref, max_dist, rotations=R, top=top, stride=stride, max_iters=30), args.reps)
    # the yardstick: the same sample (the points that take part, by (label, index), every stride-th) as a scan of its own, one
    # pn_icp_correspond call per seed on preallocated buffers
    seg = torch.tensor(ref.seg, device=dev)
    nonempty = torch.cat([seg[1:] > seg[:-1], torch.zeros(1, dtype=torch.bool, device=dev)])
    l0 = L[0].long()
    act = (l0 >= 0) & (l0 < ref.n_parts) & nonempty[l0.clamp(0, ref.n_parts)] & torch.isfinite(S[0]).all(-1)
    rows = torch.nonzero(act)[:, 0]
    rows = rows[torch.sort(l0[rows], stable=True).indices][::stride]
    ss, sl = S[:, rows].contiguous(), L[:, rows].contiguous()
    n_s = int(rows.numel())
    p32 = seeds[0].float().contiguous()
    nbytes = _lib.lib().pn_icp_workspace_bytes(1, n_s, ref.M, ref.n_parts)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    idx = torch.empty(1, n_s, device=dev, dtype=torch.int32)
    d2 = torch.empty(1, n_s, device=dev, dtype=torch.float32)
    md2 = float(np.float32(max_dist * max_dist))

    def separate():
        st = _lib.current_stream()
        for k in range(K + 1):
            _lib.check(_lib.lib().pn_icp_correspond(_lib.ptr(ss), _lib.ptr(sl), 1, n_s, _lib.ptr(ref.xyz), ref._seg_c, ref.M, ref.n_parts,
                                                    C.c_void_p(p32[k].data_ptr()), md2, _lib.ptr(idx), _lib.ptr(d2), None, _lib.ptr(ws),
                                                    nbytes, st), "pn_icp_correspond")

    _, separate_ms = timed(separate, args.reps)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        separate()
        with torch.cuda.graph(g, stream=side):
            separate()
    torch.cuda.current_stream().wait_stream(side)
    _, separate_graph_ms = timed(lambda: g.replay(), args.reps)
    # the last seed's d2 from the yardstick against the scorer's figures for it: the two measure the same thing
    c = torch.where(d2[0] <= md2, d2[0], torch.full_like(d2[0], md2)).double().sum()
    pose = pose.cpu().numpy()[0]
    ang = float(np.arccos(np.clip((np.trace(pose[:3, :3].T @ true[:3, :3]) - 1) / 2, -1, 1)))
    return {"global": {"N": N, "seeds": K + 1, "top": top, "stride": stride, "sampled_points": n_s, "moments_ms": moments_ms,
                       "seeds_ms": seeds_ms, "score_ms": score_ms, "refine_ms": refine_ms, "select_ms": select_ms,
                       "global_pose_ms": total_ms, "separate_correspond_ms": separate_ms,
                       "separate_correspond_graph_ms": separate_graph_ms,
                       "score_matches_separate": bool(abs(float(c) - float(score[0, K, 1])) <= 1e-9 * float(c)),
                       "winner": int(winner[0]), "refine_iters": int(iters[0]), "cost": float(cost[0]), "error_rad": ang,
                       "error_m": float(np.linalg.norm(pose[:3, 3] - true[:3, 3]))}}


def bench_lidar(args, dev, level=3, B=32, H=128, W=128, N=2048):
    """the LiDAR simulator: B look-at poses x H x W rays against the aircraft mesh, cast (one launch, B * R * T tests) and pack
    (three launches) timed on their own and together"""
    from pointcloudprocessing_amd import ops, pointcloud
    mo = _test_module("icp_mesh_oracle")                                              # the mesh generator only
    v, f, p = mo.aircraft_mesh(level)
    mesh = ops.icp_mesh_reference(v, f, p, len(mo.MESH_PARTS), device=dev)
    vp = pointcloud.sample_viewpoints(B, (45.0, 80.0), (0.0, 360.0), (-30.0, 60.0), seed=20260008)
    poses = torch.from_numpy(np.stack([pointcloud.look_at_pose(x) for x in vp]).astype(np.float32)).to(dev)
    dirs = torch.from_numpy(pointcloud.pinhole_rays(H, W, 50.0, 50.0)).to(dev)
    (hit, t), cast_ms = timed(lambda: ops.lidar_cast(mesh, poses, dirs), args.reps)
    (_, _, _, count), pack_ms = timed(lambda: ops.lidar_pack(mesh, hit, t, dirs, N), args.reps)
    _, frames_ms = timed(lambda: ops.lidar_frames(mesh, poses, dirs, N), args.reps)
    tests = B * H * W * mesh.T
    out = {"lidar": {"B": B, "rays": H * W, "T": mesh.T, "N": N, "cast_ms": cast_ms, "pack_ms": pack_ms, "frames_ms": frames_ms,
                     "ray_triangle_tests_per_s": tests / (cast_ms * 1e-3), "frames_per_s": B / (frames_ms * 1e-3),
                     "hits_per_frame_min": int(count.min()), "hits_per_frame_max": int(count.max())}}
    out.update(bench_lidar_bvh(dev, poses, dirs))
    return out


def bench_sensor(args, dev, level=3, B=32, H=128, W=128, N=2048):
    """the sensor model (ops.lidar_sense, one launch, all stages on) at the shape of bench_lidar, beside the launches it sits between
    in the same run: the brute-force cast, the cast through the trees and the pack, medians of ``args.reps``; ``share_*`` is the sense
    launch as a share of cast + pack on the same frames"""
    from pointcloudprocessing_amd import ops, pointcloud
    mo = _test_module("icp_mesh_oracle")                                              # the mesh generator only
    v, f, p = mo.aircraft_mesh(level)
    mesh = ops.icp_mesh_reference(v, f, p, len(mo.MESH_PARTS), device=dev, accel="bvh")
    vp = pointcloud.sample_viewpoints(B, (45.0, 80.0), (0.0, 360.0), (-30.0, 60.0), seed=20260008)
    poses = torch.from_numpy(np.stack([pointcloud.look_at_pose(x) for x in vp]).astype(np.float32)).to(dev)
    dirs = torch.from_numpy(pointcloud.pinhole_rays(H, W, 50.0, 50.0)).to(dev)
    model = dict(range_sigma=(0.02, 0.001), detection=dict(strength=1.5, range_ref=60.0), max_incidence_deg=80.0,
                 mixed=dict(jump=0.5, prob=0.5))
    (hit, t), cast_ms = timed(lambda: ops.lidar_cast(mesh, poses, dirs), args.reps)
    _, cast_bvh_ms = timed(lambda: ops.lidar_cast(mesh, poses, dirs, accel="bvh"), args.reps)
    (h2, t2, kind), sense_ms = timed(lambda: ops.lidar_sense(mesh, poses, dirs, hit, t, (H, W), seed=1, **model), args.reps)
    _, pack_ms = timed(lambda: ops.lidar_pack(mesh, h2, t2, dirs, N), args.reps)
    _, frames_ms = timed(lambda: ops.lidar_frames(mesh, poses, dirs, N, sensor=dict(model, shape=(H, W)), seed=1), args.reps)
    # a single call of tens of microseconds is mostly its host side: the same three over windows of back-to-back calls
    _, sense_loop_ms = timed_calls(lambda: ops.lidar_sense(mesh, poses, dirs, hit, t, (H, W), seed=1, **model), args.reps)
    _, cast_bvh_loop_ms = timed_calls(lambda: ops.lidar_cast(mesh, poses, dirs, accel="bvh"), args.reps)
    _, pack_loop_ms = timed_calls(lambda: ops.lidar_pack(mesh, h2, t2, dirs, N), args.reps)
    kinds = torch.bincount(kind.reshape(-1).long(), minlength=4).tolist()
    return {"sensor": {"sense_loop_ms": sense_loop_ms, "cast_bvh_loop_ms": cast_bvh_loop_ms, "pack_loop_ms": pack_loop_ms,
                       "loop_share_of_bvh_cast_plus_pack": sense_loop_ms / (cast_bvh_loop_ms + pack_loop_ms),
                       "B": B, "rays": H * W, "T": mesh.T, "N": N, "cast_ms": cast_ms, "cast_bvh_ms": cast_bvh_ms, "sense_ms": sense_ms,
                       "pack_ms": pack_ms, "frames_with_sensor_ms": frames_ms, "share_of_cast_plus_pack": sense_ms / (cast_ms + pack_ms),
                       "share_of_bvh_cast_plus_pack": sense_ms / (cast_bvh_ms + pack_ms), "rays_per_s": B * H * W / (sense_ms * 1e-3),
                       "kinds": dict(zip(pointcloud.LIDAR_KINDS, kinds))}}


def bench_lidar_bvh(dev, poses, dirs, levels=(3, 5), rounds=5):
    """the cast through the per-part trees (ops.lidar_cast(accel="bvh")) against the brute-force cast on the same grouped mesh and
    the same frames: one tree and one brute-force call alternate ``rounds`` times after a warm-up round, the medians are reported;
    also the host build of the trees (pn_icp_bvh_build alone, median of 3) and whether both casts end on the same bytes"""
    import time
    from pointcloudprocessing_amd import ops
    mo = _test_module("icp_mesh_oracle")                                              # the mesh generator only
    n_parts = len(mo.MESH_PARTS)

    def once(ref, accel):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        res = ops.lidar_cast(ref, poses, dirs, accel=accel)
        e1.record()
        torch.cuda.synchronize()
        return res, e0.elapsed_time(e1)

    out = {}
    for level in levels:
        v, f, p = mo.aircraft_mesh(level)
        acc = ops.icp_mesh_reference(v, f, p, n_parts, device=dev, accel="bvh")
        tri_host, build = acc.tri.cpu().numpy(), []
        for _ in range(3):
            t0 = time.perf_counter()
            ops._build_bvh(tri_host, acc.seg, n_parts)
            build.append((time.perf_counter() - t0) * 1e3)
        ts, res = {"bvh": [], None: []}, {}
        for rnd in range(rounds + 1):
            for accel in ("bvh", None):
                res[accel], ms = once(acc, accel)
                if rnd:
                    ts[accel].append(ms)
        bvh_ms, brute_ms = float(np.median(ts["bvh"])), float(np.median(ts[None]))
        out[f"lidar_bvh_T{acc.T}"] = {"B": int(poses.shape[0]), "rays": int(dirs.shape[0]), "T": acc.T, "nodes": acc.n_nodes,
                                      "build_ms": float(np.median(build)), "bvh_cast_ms": bvh_ms, "brute_cast_ms": brute_ms,
                                      "speedup": brute_ms / bvh_ms, "hits": int((res["bvh"][0] >= 0).sum()),
                                      "same_bytes": all(torch.equal(x.view(torch.int32), y.view(torch.int32))
                                                        for x, y in zip(res["bvh"], res[None]))}
    return out


def timed_calls(fn, reps, calls=200):
    """milliseconds per call: the median over ``reps`` windows of ``calls`` back-to-back calls each (a single call is too short to
    time), after one warm-up window"""
    out, ts = None, []
    for rep in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            out = fn()
        e1.record()
        torch.cuda.synchronize()
        if rep:
            ts.append(e0.elapsed_time(e1) / calls)
    return out, float(np.median(ts))


def bench_sample(args, dev, level=3, K=256, top=4, cloud_n=8192):
    """the mesh sampler against the same stratified area-weighted draw in torch ops, and ops.global_pose against the mesh with
    the vertex score and with a sampled score cloud (the pose, N, seeds and top of bench_global)"""
    from pointcloudprocessing_amd import ops
    mo = _test_module("icp_mesh_oracle")                                              # the mesh and scan generators only
    v, f, p = mo.aircraft_mesh(level)
    n_parts = len(mo.MESH_PARTS)
    mesh = ops.icp_mesh_reference(v, f, p, n_parts, device=dev)
    seg = torch.tensor(mesh.seg[1:], device=dev)

    def torch_draw(sets, n):
        C = torch.cumsum(mesh.area, 0)
        r = torch.rand(sets, n, 3, device=dev, dtype=torch.float64)
        pos = (torch.arange(n, device=dev) + r[..., 0]) * (C[-1] / n)
        row = torch.searchsorted(C, pos, right=True).clamp_(max=mesh.T - 1)
        u, w = r[..., 1].float(), r[..., 2].float()
        fold = u + w > 1.0
        u, w = torch.where(fold, 1.0 - u, u)[..., None], torch.where(fold, 1.0 - w, w)[..., None]
        t = mesh.tri[row]
        xyz = (t[..., 0, :] + u * (t[..., 1, :] - t[..., 0, :])) + w * (t[..., 2, :] - t[..., 0, :])
        return xyz, torch.searchsorted(seg, row, right=True).to(torch.int32), row.to(torch.int32)

    out = {"T": mesh.T}
    for sets, n in ((1, 8192), (32, 2048)):
        (xyz, part, row), ms = timed_calls(lambda: ops.mesh_sample(mesh, n, seed=7, sets=sets), args.reps)
        (txyz, tpart, trow), tms = timed_calls(lambda: torch_draw(sets, n), args.reps)
        cnt, tcnt = torch.bincount(row[0].long(), minlength=mesh.T).double(), torch.bincount(trow[0].long(), minlength=mesh.T).double()
        share = n * mesh.area / mesh.area.sum()
        out[f"sets{sets}_n{n}"] = {"mesh_sample_ms": ms, "torch_ops_ms": tms, "torch_over_mesh_sample": tms / ms,
                                   "samples_per_s": sets * n / (ms * 1e-3), "max_count_minus_share": float((cnt - share).abs().max()),
                                   "torch_max_count_minus_share": float((tcnt - share).abs().max())}
    rng = np.random.default_rng(20260007)
    true = np.eye(4)
    true[:3, :3] = rot(rng.normal(size=3), np.deg2rad(150))
    true[:3, 3] = rng.uniform(-30, 30, 3)
    scan, lab = mo.mesh_scan(v, f, p, args.points, true, noise=0.05, seed=1)
    S, L = torch.from_numpy(scan[None]).to(dev), torch.from_numpy(lab[None]).to(dev)
    max_dist, stride = 3.0, max(1, args.points // 8192)
    R = ops.rotation_grid(K).to(dev)
    _, ref_ms = timed(lambda: ops.mesh_sample_reference(mesh, cloud_n, seed=7), args.reps)
    cloud = ops.mesh_sample_reference(mesh, cloud_n, seed=7)
    g = {"N": args.points, "seeds": K + 1, "top": top, "stride": stride, "vertices": 3 * mesh.T, "score_cloud_points": cloud.M,
         "mesh_sample_reference_ms": ref_ms}
    for name, sc in (("vertices", None), ("score_cloud", cloud)):
        (pose, _, _, iters, _, cost, winner), ms = timed(
            lambda: ops.global_pose(S, L, mesh, max_dist, rotations=R, top=top, stride=stride, max_iters=30, score_cloud=sc), args.reps)
        pose = pose.cpu().numpy()[0]
        ang = float(np.arccos(np.clip((np.trace(pose[:3, :3].T @ true[:3, :3]) - 1) / 2, -1, 1)))
        g[name] = {"global_pose_ms": ms, "winner": int(winner[0]), "refine_iters": int(iters[0]), "cost": float(cost[0]), "error_rad": ang,
                   "error_m": float(np.linalg.norm(pose[:3, 3] - true[:3, 3]))}
    out["global_mesh"] = g
    return {"mesh_sample": out}


def bench_robust(args, dev, share=0.2, level=3):
    """the robust loop against the unweighted one on scans with wrong labels: per-iteration times and final errors"""
    from pointcloudprocessing_amd import ops, pointcloud
    mo, po = _test_module("icp_mesh_oracle"), _test_module("icp_plane_oracle")      # the mesh and scene generators only
    true = po.TRUE_POSE
    start = true.copy()
    start[:3, :3] = rot([1, 2, 3], np.deg2rad(5)) @ true[:3, :3]
    start[:3, 3] += [0.3, -0.3, 0.25]
    I = torch.from_numpy(start[None]).to(dev)

    def spoil(lab, parts, seed=20260007):
        rng = np.random.default_rng(seed)
        lab = lab.copy()
        pick = rng.choice(lab.size, int(round(share * lab.size)), replace=False)
        ok = pick[lab[pick] >= 0]
        lab[ok] = parts[(np.searchsorted(parts, lab[ok]) + rng.integers(1, len(parts), ok.size)) % len(parts)]
        return lab

    kx, kp = pointcloud.read_labelled_cloud(os.path.join(ROOT, "tests", "golden", "kc-46.txt"), PARTS)
    _, _, kref = ops.icp_normals(ops.icp_reference(kx, kp, len(PARTS), device=dev), k=10)
    kscan, klab = make_labelled_scan(args.points, np.asarray(kx, np.float32), np.asarray(kp), true)
    v, f, p = mo.aircraft_mesh(level)
    mesh = ops.icp_mesh_reference(v, f, p, len(mo.MESH_PARTS), device=dev)
    mscan, mlab = mo.mesh_scan(v, f, p, args.points, true, noise=0.02, seed=1)
    cases = [("kc46_plane", kref, kscan, spoil(klab, np.unique(np.asarray(kp))), "plane"),
             ("kc46_point", kref, kscan, spoil(klab, np.unique(np.asarray(kp))), "point"),
             (f"mesh_T{mesh.T}_plane", mesh, mscan, spoil(mlab, np.arange(len(mo.MESH_PARTS))), "plane")]
    out = {}
    for name, ref, scan, lab, metric in cases:
        S, L = torch.from_numpy(scan[None]).to(dev), torch.from_numpy(lab[None]).to(dev)
        r = {"N": args.points, "wrong_labels": share}
        for key, kw in (("unweighted", {}), ("tukey_fixed", {"robust": "tukey", "robust_scale": 0.3}), ("tukey_mad", {"robust": "tukey"})):
            kw = dict(kw, metric=metric, max_dist=3.0)
            ms = iter_ms(S, L, ref, I, args.reps, **kw)
            (pose, rmse, pairs, it, st), _ = timed(lambda: ops.semantic_icp(S, L, ref, I, max_iters=40, **kw), 1)
            pose = pose.cpu().numpy()[0]
            ang = float(np.arccos(np.clip((np.trace(pose[:3, :3].T @ true[:3, :3]) - 1) / 2, -1, 1)))
            r[key] = {"iter_ms": ms, "iters": int(it[0]), "status": int(st[0]), "pairs": int(pairs[0]), "error_rad": ang,
                      "error_m": float(np.linalg.norm(pose[:3, 3] - true[:3, 3])), "rmse_m": float(rmse[0])}
        r["fixed_extra_us"] = 1e3 * (r["tukey_fixed"]["iter_ms"] - r["unweighted"]["iter_ms"])
        r["mad_extra_us"] = 1e3 * (r["tukey_mad"]["iter_ms"] - r["unweighted"]["iter_ms"])
        out[f"robust_{name}"] = r
    return out


def make_cluttered_scan(n, share=0.02, margin=40.0, seed=20260008):
    """the C5 scan with ``share`` of n extra strays, uniform over the scan's bounding box grown by ``margin`` on every side, shuffled in"""
    xyz, _ = make_scan(n)
    rng = np.random.default_rng(seed)
    strays = rng.uniform(xyz.min(0) - margin, xyz.max(0) + margin, size=(int(round(share * n)), 3)).astype(np.float32)
    out = np.concatenate([xyz, strays]).astype(np.float32)
    rng.shuffle(out)
    return out


def bench_cluster(args, dev, model=None):
    import ctypes as C
    from pointcloudprocessing_amd import _lib, ops
    from pointcloudprocessing_amd.pointnet.PointNet import PointNet
    xyz = make_cluttered_scan(args.points)
    x = torch.from_numpy(xyz).to(dev)
    N = x.shape[0]
    origin = xyz.min(0)
    L = _lib.lib()
    out = {"N": N, "strays": N - args.points}
    i32 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.int32)      # noqa: E731
    cl, vx, sz, nout, cnt, maj = i32(N), i32(N), i32(N), i32(2), i32(N), i32(N)
    cent = torch.empty(N, 3, device=dev)
    nb_c, nb_d = L.pn_voxel_cluster_workspace_bytes(N), L.pn_voxel_workspace_bytes(N)
    ws = torch.empty(max(nb_c, nb_d), device=dev, dtype=torch.uint8)
    org_c = (C.c_float * 3)(*[float(v) for v in origin])
    for leaf in (0.25, 1.0):
        leaf3 = (leaf,) * 3
        leaf_c = (C.c_float * 3)(*leaf3)
        (c, s), cluster_ms = timed(lambda: ops.voxel_clusters(x, leaf3, origin), args.reps)
        (ce, _, _), down_ms = timed(lambda: ops.voxel_downsample(x, leaf3, origin), args.reps)
        _, raw_c = timed(lambda: _lib.check(L.pn_voxel_cluster(_lib.ptr(x), N, leaf_c, org_c, 26, _lib.ptr(cl), _lib.ptr(vx), _lib.ptr(sz),
                                                               _lib.ptr(nout), _lib.ptr(ws), nb_c, _lib.current_stream()), "pn_voxel_cluster"),
                         args.reps)
        _, raw_d = timed(lambda: _lib.check(L.pn_voxel_downsample(_lib.ptr(x), None, N, leaf_c, org_c, 0, _lib.ptr(cent), _lib.ptr(cnt),
                                                                  _lib.ptr(maj), _lib.ptr(nout), _lib.ptr(ws), nb_d, _lib.current_stream()),
                                            "pn_voxel_downsample"), args.reps)
        out[f"leaf_{leaf}"] = {"voxels": int(ce.shape[0]), "clusters": int(s.numel()), "largest": int(s.max()),
                               "voxel_clusters_ms": cluster_ms, "voxel_downsample_ms": down_ms, "ratio": cluster_ms / down_ms,
                               "raw_cluster_ms": raw_c, "raw_downsample_ms": raw_d, "raw_ratio": raw_c / raw_d}
    if model is None:
        model = PointNet(23, 12, 0.3, 42, vanilla=True, precision="bf16", device=dev)
    kw = dict(leaf=args.leaf, samples=args.samples, k=args.k)
    _, plain_ms = timed(lambda: model.predict_scan(x, **kw), args.reps)
    (_, part, _), iso_ms = timed(lambda: model.predict_scan(x, isolate="largest", cluster_leaf=1.0, **kw), args.reps)
    out.update({"predict_scan_ms": plain_ms, "predict_scan_isolate_ms": iso_ms, "isolate_dropped": int((part < 0).sum())})
    return {"cluster": out}


def bench_dbscan(args, dev):
    """Exact DBSCAN (--dbscan-only; not part of the default run) on the --cluster-only scene: raw pn_dbscan at eps 0.25 and 0.5,
    min_points 8, beside raw pn_voxel_cluster at leaf = eps and raw pn_radius_knn with k = 0 at radius = eps (the count-only search:
    the design walks the candidates three times where it walks them once), on the same input in the same run, preallocated buffers"""
    import ctypes as C
    from pointcloudprocessing_amd import _lib
    xyz = make_cluttered_scan(args.points)
    x = torch.from_numpy(xyz).to(dev)
    N = x.shape[0]
    L = _lib.lib()
    i32 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.int32)      # noqa: E731
    cl, vx, sz, nout, cnt = i32(N), i32(N), i32(N), i32(2), i32(N)
    core = torch.empty(N, device=dev, dtype=torch.uint8)
    nb_db, nb_c, nb_r = L.pn_dbscan_workspace_bytes(N), L.pn_voxel_cluster_workspace_bytes(N), L.pn_radius_knn_workspace_bytes(N)
    ws = torch.empty(max(nb_db, nb_c, nb_r), device=dev, dtype=torch.uint8)
    org_c = (C.c_float * 3)(*[float(v) for v in xyz.min(0)])
    st = _lib.current_stream
    out = {"N": N, "min_points": 8}
    for eps in (0.25, 0.5):
        leaf_c = (C.c_float * 3)(eps, eps, eps)
        _, db_ms = timed(lambda: _lib.check(L.pn_dbscan(_lib.ptr(x), N, eps, 8, org_c, _lib.ptr(cl), _lib.ptr(core), _lib.ptr(sz), _lib.ptr(nout),
                                                        _lib.ptr(ws), nb_db, st()), "pn_dbscan"), args.reps)
        assert int(ws[:4].view(torch.int32).item()) == 0
        n_core, K = nout.tolist()
        r = {"core_points": n_core, "clusters": K, "largest": int(sz[:K].max()) if K else 0, "noise": int((cl < 0).sum())}
        _, vc_ms = timed(lambda: _lib.check(L.pn_voxel_cluster(_lib.ptr(x), N, leaf_c, org_c, 26, _lib.ptr(cl), _lib.ptr(vx), _lib.ptr(sz),
                                                               _lib.ptr(nout), _lib.ptr(ws), nb_c, st()), "pn_voxel_cluster"), args.reps)
        _, k0_ms = timed(lambda: _lib.check(L.pn_radius_knn(_lib.ptr(x), N, eps, org_c, 0, None, None, _lib.ptr(cnt), _lib.ptr(ws), nb_r, st()),
                                            "pn_radius_knn"), args.reps)
        r.update({"dbscan_ms": db_ms, "voxel_cluster_ms": vc_ms, "radius_knn_k0_ms": k0_ms, "dbscan_over_radius_knn_k0": db_ms / k0_ms,
                  "dbscan_over_voxel_cluster": db_ms / vc_ms, "neighbours_mean": float(cnt.float().mean())})
        out[f"eps_{eps}"] = r
    return {"dbscan": out}


def bench_denoise(args, dev, model=None, radius=0.5):
    """pn_radius_knn on the cluttered C5 scan: the grid search against pn_voxel_downsample (it shares the sort) and against the brute-force
    pn_knn_propagate(query = ref = scan) in the same process, ops.outlier_mask, and predict_scan with and without ``denoise``"""
    import ctypes as C
    from pointcloudprocessing_amd import _lib, ops
    from pointcloudprocessing_amd.pointnet.PointNet import PointNet
    xyz = make_cluttered_scan(args.points)
    x = torch.from_numpy(xyz).to(dev)
    N = x.shape[0]
    origin = xyz.min(0)
    L = _lib.lib()
    i32 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.int32)      # noqa: E731
    idx, cnt, nout, vcnt, maj = i32(N, 8), i32(N), i32(1), i32(N), i32(N)
    d2, cent = torch.empty(N, 8, device=dev), torch.empty(N, 3, device=dev)
    nb_r, nb_d = L.pn_radius_knn_workspace_bytes(N), L.pn_voxel_workspace_bytes(N)
    ws = torch.empty(max(nb_r, nb_d), device=dev, dtype=torch.uint8)
    org_c = (C.c_float * 3)(*[float(v) for v in origin])
    h = float(L.pn_radius_knn_leaf(radius))
    leaf_c = (C.c_float * 3)(h, h, h)
    st = _lib.current_stream
    _, raw8 = timed(lambda: _lib.check(L.pn_radius_knn(_lib.ptr(x), N, radius, org_c, 8, _lib.ptr(idx), _lib.ptr(d2), _lib.ptr(cnt), _lib.ptr(ws),
                                                       nb_r, st()), "pn_radius_knn"), args.reps)
    _, raw0 = timed(lambda: _lib.check(L.pn_radius_knn(_lib.ptr(x), N, radius, org_c, 0, None, None, _lib.ptr(cnt), _lib.ptr(ws), nb_r, st()),
                                       "pn_radius_knn"), args.reps)
    assert int(ws[:4].view(torch.int32).item()) == 0
    count = cnt.clone()
    _, raw_d = timed(lambda: _lib.check(L.pn_voxel_downsample(_lib.ptr(x), None, N, leaf_c, org_c, 0, _lib.ptr(cent), _lib.ptr(vcnt), _lib.ptr(maj),
                                                              _lib.ptr(nout), _lib.ptr(ws), nb_d, st()), "pn_voxel_downsample"), args.reps)
    xb = x.unsqueeze(0)
    (bidx, bd2), brute = timed(lambda: ops.knn_propagate(xb, xb, 8), args.reps)
    # brute force finds the point itself first (d = 0): its next seven are the grid search's first seven wherever those lie within the radius
    same = bool(((bd2[0, :, 1:] == d2[:, :7]) | (bd2[0, :, 1:] > radius * radius)).all())
    _, mask_r = timed(lambda: ops.outlier_mask(x, "radius", radius, min_neighbors=8, origin=origin), args.reps)
    keep, mask_s = timed(lambda: ops.outlier_mask(x, "statistical", radius, k=8, std_ratio=2.0, origin=origin), args.reps)
    if model is None:
        model = PointNet(23, 12, 0.3, 42, vanilla=True, precision="bf16", device=dev)
    kw = dict(leaf=args.leaf, samples=args.samples, k=args.k)
    _, plain_ms = timed(lambda: model.predict_scan(x, **kw), args.reps)
    (_, part, _), den_ms = timed(lambda: model.predict_scan(x, denoise=dict(method="radius", radius=radius, min_neighbors=8), **kw), args.reps)
    V = int(nout.item())
    return {"denoise": {"N": N, "radius": radius, "leaf": h, "voxels": V, "radius_knn_k8_ms": raw8, "radius_knn_k0_ms": raw0,
                        "voxel_downsample_ms": raw_d, "k8_over_downsample": raw8 / raw_d, "brute_force_knn_k8_ms": brute,
                        "brute_over_grid": brute / raw8, "brute_agrees": same, "neighbours_mean": float(count.float().mean()),
                        "neighbours_median": float(count.float().median()), "neighbours_max": int(count.max()),
                        "points_per_voxel_mean": N / max(V, 1), "outlier_mask_radius_ms": mask_r, "outlier_mask_statistical_ms": mask_s,
                        "statistical_kept": int(keep.sum()), "predict_scan_ms": plain_ms, "predict_scan_denoise_ms": den_ms,
                        "denoise_dropped": int((part < 0).sum())}}


def bench_normals(args, dev, radius=0.5):
    """pn_scan_normals on the --denoise-only scan at k = 8 and 16: beside pn_radius_knn at the same radius and k in the same run (the
    fused kernel replaces its search launch, so the difference is what the gather of the winners, the fp64 covariance, the Jacobi
    and the scatter cost), and beside the composition a user would write: ops.radius_knn -> gather -> batched fp64 covariance ->
    torch.linalg.eigh on the device.  The torch composition's normals are compared with the fused ones"""
    import ctypes as C
    from pointcloudprocessing_amd import _lib, ops
    xyz = make_cluttered_scan(args.points)
    x = torch.from_numpy(xyz).to(dev)
    N = x.shape[0]
    origin = xyz.min(0)
    vp = (0.0, 0.0, 0.0)
    L = _lib.lib()
    nb = L.pn_scan_normals_workspace_bytes(N)
    assert nb >= L.pn_radius_knn_workspace_bytes(N)
    ws = torch.empty(nb, device=dev, dtype=torch.uint8)
    org_c, vp_c = (C.c_float * 3)(*[float(v) for v in origin]), (C.c_float * 3)(*vp)
    nrm, curv = torch.empty(N, 3, device=dev), torch.empty(N, device=dev)
    cnt = torch.empty(N, device=dev, dtype=torch.int32)
    st = _lib.current_stream
    x64 = x.double()

    def torch_normals(k):
        idx, _, count = ops.radius_knn(x, radius, k, origin=origin)
        ids = torch.cat([torch.arange(N, device=dev, dtype=torch.int32)[:, None], idx], 1)
        valid = ids >= 0
        c = valid.sum(1, keepdim=True).double()
        pts = torch.where(valid[:, :, None], x64[ids.long().clamp(min=0)], torch.zeros((), device=dev, dtype=torch.float64))
        e = torch.where(valid[:, :, None], pts - pts.sum(1, keepdim=True) / c[:, :, None], torch.zeros((), device=dev, dtype=torch.float64))
        cov = e.transpose(1, 2) @ e / c[:, :, None]
        lam, V = torch.linalg.eigh(cov)
        n = V[:, :, 0]
        s = (n * (torch.tensor(vp, device=dev, dtype=torch.float64) - x64)).sum(1)
        n = torch.where((s < 0)[:, None], -n, n)
        ok = (c[:, 0] >= 3) & (lam[:, 1] > 1e-12 * lam[:, 2])
        return torch.where(ok[:, None], n, torch.full((), float("nan"), device=dev, dtype=torch.float64)).float()

    out = {"N": N, "radius": radius}
    for k in (8, 16):
        idx, d2 = torch.empty(N, k, device=dev, dtype=torch.int32), torch.empty(N, k, device=dev)
        _, knn_ms = timed(lambda: _lib.check(L.pn_radius_knn(_lib.ptr(x), N, radius, org_c, k, _lib.ptr(idx), _lib.ptr(d2), _lib.ptr(cnt), _lib.ptr(ws),
                                                             nb, st()), "pn_radius_knn"), args.reps)
        _, fused_ms = timed(lambda: _lib.check(L.pn_scan_normals(_lib.ptr(x), N, radius, org_c, k, vp_c, _lib.ptr(nrm), _lib.ptr(curv), _lib.ptr(cnt),
                                                                 None, _lib.ptr(ws), nb, st()), "pn_scan_normals"), args.reps)
        _, fused_idx_ms = timed(lambda: _lib.check(L.pn_scan_normals(_lib.ptr(x), N, radius, org_c, k, vp_c, _lib.ptr(nrm), _lib.ptr(curv),
                                                                     _lib.ptr(cnt), _lib.ptr(idx), _lib.ptr(ws), nb, st()), "pn_scan_normals"),
                                args.reps)
        assert int(ws[:4].view(torch.int32).item()) == 0
        _, ops_ms = timed(lambda: ops.estimate_normals(x, radius, k, viewpoint=vp, origin=origin), args.reps)
        tn, torch_ms = timed(lambda: torch_normals(k), args.reps)
        both = torch.isfinite(tn).all(1) & torch.isfinite(nrm).all(1)
        dots = (tn[both].double() * nrm[both].double()).sum(1)
        out.update({f"radius_knn_k{k}_ms": knn_ms, f"scan_normals_k{k}_ms": fused_ms, f"scan_normals_k{k}_with_idx_ms": fused_idx_ms,
                    f"estimate_normals_k{k}_ms": ops_ms, f"torch_composition_k{k}_ms": torch_ms, f"torch_over_fused_k{k}": torch_ms / fused_ms,
                    f"fused_over_radius_knn_k{k}": fused_ms / knn_ms, f"finite_rows_k{k}": int(torch.isfinite(nrm).all(1).sum()),
                    f"finite_masks_equal_k{k}": bool((torch.isfinite(tn).all(1) == torch.isfinite(nrm).all(1)).all()),
                    f"worst_one_minus_abs_dot_k{k}": float((1 - dots.abs()).max()), f"signs_differ_k{k}": int((dots < 0).sum())})
    _, mask_ms = timed(lambda: ops.outlier_mask(x, "incidence", radius, k=8, origin=origin), args.reps)
    out["outlier_mask_incidence_ms"] = mask_ms
    return {"normals": out}


def bench_recon(args, dev, voxels=(0.5, 0.25), normals_radius=0.5):
    """Surface reconstruction on the C5 scan (its rows with a valid normal from ops.estimate_normals at 0.5 m, k = 8, turned
    upwards), at two voxel sizes with radius = 3 voxels on the default lattice: pn_recon_field, pn_recon_count and pn_recon_emit
    each on preallocated buffers, and in the same run the count-only pn_radius_knn (k = 0) at the same radius -- the field's
    yardstick: the same sort and the same candidate walk, with the cloud's own points as queries -- and pn_voxel_downsample at
    leaf = voxel on the same cloud.  Reports the lattice, its valid share, the vertices and faces, and one ops.reconstruct_mesh
    call end to end (with its host reads and allocations)"""
    import ctypes as C
    from pointcloudprocessing_amd import _lib, ops
    xyz, _ = make_scan(args.points)
    x0 = torch.from_numpy(xyz).to(dev)
    n0 = ops.estimate_normals(x0, normals_radius, 8, viewpoint=(0.0, 0.0, 1000.0))[0]
    rows = torch.isfinite(n0).all(1).nonzero().squeeze(1)
    x, nrm = x0[rows].contiguous(), n0[rows].contiguous()
    N = x.shape[0]
    L = _lib.lib()
    st = _lib.current_stream
    lo, hi = x.min(0).values.double().cpu().numpy(), x.max(0).values.double().cpu().numpy()
    go = (C.c_float * 3)(*x.min(0).values.cpu().tolist())
    cnt_n = torch.empty(N, device=dev, dtype=torch.int32)
    out = {"N": N, "rows_without_normal": int(x0.shape[0] - N)}
    for voxel in voxels:
        radius = 3.0 * voxel
        origin = lo - radius
        dims = tuple(int(d) for d in np.maximum(np.ceil(((hi + radius) - origin) / voxel).astype(np.int64) + 1, 2))
        P = dims[0] * dims[1] * dims[2]
        org = (C.c_double * 3)(*origin)
        f = torch.empty(P, device=dev)
        cnt = torch.empty(P, device=dev, dtype=torch.int32)
        fb, sb, kb = L.pn_recon_field_workspace_bytes(N), L.pn_recon_workspace_bytes(*dims), L.pn_radius_knn_workspace_bytes(N)
        vb = L.pn_voxel_workspace_bytes(N)
        ws = torch.empty(max(fb, sb, kb, vb), device=dev, dtype=torch.uint8)
        n_out = torch.zeros(2, device=dev, dtype=torch.int32)
        _, field_ms = timed(lambda: _lib.check(L.pn_recon_field(_lib.ptr(x), _lib.ptr(nrm), N, radius, go, org, voxel, *dims, 3, _lib.ptr(f),
                                                                _lib.ptr(cnt), _lib.ptr(ws), fb, st()), "pn_recon_field"), args.reps)
        assert int(ws[:4].view(torch.int32).item()) == 0
        _, knn_ms = timed(lambda: _lib.check(L.pn_radius_knn(_lib.ptr(x), N, radius, go, 0, None, None, _lib.ptr(cnt_n), _lib.ptr(ws), kb, st()),
                                             "pn_radius_knn"), args.reps)
        cent, vcnt, vn = torch.empty(N, 3, device=dev), torch.empty(N, device=dev, dtype=torch.int32), torch.zeros(1, device=dev, dtype=torch.int32)
        leaf = (C.c_float * 3)(voxel, voxel, voxel)
        _, voxel_ms = timed(lambda: _lib.check(L.pn_voxel_downsample(_lib.ptr(x), None, N, leaf, go, 0, _lib.ptr(cent), _lib.ptr(vcnt), None,
                                                                     _lib.ptr(vn), _lib.ptr(ws), vb, st()), "pn_voxel_downsample"), args.reps)
        _, count_ms = timed(lambda: _lib.check(L.pn_recon_count(_lib.ptr(f), *dims, _lib.ptr(n_out), _lib.ptr(ws), sb, st()), "pn_recon_count"),
                            args.reps)
        V, F = (int(v) for v in n_out.tolist())
        verts, faces = torch.empty(V, 3, device=dev), torch.empty(F, 3, device=dev, dtype=torch.int32)
        _, emit_ms = timed(lambda: _lib.check(L.pn_recon_emit(_lib.ptr(f), org, voxel, *dims, _lib.ptr(verts), V, _lib.ptr(faces), F,
                                                              _lib.ptr(n_out), _lib.ptr(ws), sb, st()), "pn_recon_emit"), args.reps)
        assert int(ws[:4].view(torch.int32).item()) == 0 and n_out.tolist() == [V, F]
        _, ops_ms = timed(lambda: ops.reconstruct_mesh(x, nrm, voxel), args.reps)
        out[f"voxel_{voxel:g}"] = {
            "radius": radius, "lattice": list(dims), "lattice_points": P, "valid_share": float(torch.isfinite(f).double().mean()),
            "mean_neighbours_of_a_valid_point": float(cnt[torch.isfinite(f)].double().mean()), "mean_neighbours_of_a_scan_point": float(cnt_n.double().mean()),
            "vertices": V, "faces": F, "field_ms": field_ms, "count_ms": count_ms, "emit_ms": emit_ms, "radius_knn_count_only_ms": knn_ms,
            "voxel_downsample_ms": voxel_ms, "field_over_radius_knn": field_ms / knn_ms, "reconstruct_mesh_ms": ops_ms}
    return {"recon": out}


def bench_simplify(args, dev, voxel=0.25, leaves=(0.5, 1.0), normals_radius=0.5, scan_n=8192):
    """Mesh cleaning on the C5 reconstruction at voxel 0.25 (ops.reconstruct_mesh on the scan of --recon-only): raw pn_mesh_components
    and pn_mesh_simplify (mean and quadric placement, leaf 0.5 and 1.0) on preallocated buffers, and in the same run
    pn_voxel_downsample over the mesh's vertices at the same leaf and pn_recon_emit of the same mesh; the face counts before and
    after; the distance from 65,536 ops.mesh_sample points of the full mesh to the simplified one (ops.icp_mesh_correspond: RMS and
    maximum); and one brute-force robust (Tukey, MAD scale) plane-metric mesh-ICP iteration of a ``scan_n``-point scan on the full
    mesh and on each simplified one, alternately in the same run"""
    import ctypes as C
    from pointcloudprocessing_amd import _lib, ops
    xyz, _ = make_scan(args.points)
    x0 = torch.from_numpy(xyz).to(dev)
    n0 = ops.estimate_normals(x0, normals_radius, 8, viewpoint=(0.0, 0.0, 1000.0))[0]
    rows = torch.isfinite(n0).all(1).nonzero().squeeze(1)
    x, nrm = x0[rows].contiguous(), n0[rows].contiguous()
    L = _lib.lib()
    st = _lib.current_stream
    f, origin, dims = ops.implicit_field(x, nrm, voxel, 3.0 * voxel)
    f = f.reshape(-1).contiguous()
    v, faces, _ = ops.reconstruct_mesh(x, nrm, voxel)
    V, F = v.shape[0], faces.shape[0]
    lab = torch.zeros(F, device=dev, dtype=torch.int32)
    out = {"voxel": voxel, "vertices": V, "faces": F}
    # the emit phase of the same mesh, and the components
    sb = L.pn_recon_workspace_bytes(*dims)
    ws = torch.empty(sb, device=dev, dtype=torch.uint8)
    n2 = torch.zeros(2, device=dev, dtype=torch.int32)
    ev, ef = torch.empty(V, 3, device=dev), torch.empty(F, 3, device=dev, dtype=torch.int32)
    org = (C.c_double * 3)(*origin)
    _, out["recon_emit_ms"] = timed(lambda: _lib.check(L.pn_recon_emit(_lib.ptr(f), org, voxel, *dims, _lib.ptr(ev), V, _lib.ptr(ef), F, _lib.ptr(n2),
                                                                       _lib.ptr(ws), sb, st()), "pn_recon_emit"), args.reps)
    assert n2.tolist() == [V, F]
    cb = L.pn_mesh_components_workspace_bytes(V)
    wc = torch.empty(cb, device=dev, dtype=torch.uint8)
    comp, sizes, n1 = torch.empty(F, device=dev, dtype=torch.int32), torch.empty(min(V, F), device=dev, dtype=torch.int32), n2[:1]
    _, out["components_ms"] = timed(lambda: _lib.check(L.pn_mesh_components(_lib.ptr(v), V, _lib.ptr(faces), F, _lib.ptr(comp), _lib.ptr(sizes),
                                                                            min(V, F), _lib.ptr(n1), _lib.ptr(wc), cb, st()), "pn_mesh_components"),
                                    args.reps)
    K = int(n1.item())
    assert int(wc[:4].view(torch.int32).item()) == 0
    out["components"], out["largest_component_faces"] = K, int(sizes[:K].max())
    # simplification
    go = (C.c_float * 3)(*v.min(0).values.cpu().tolist())
    mb, vb = L.pn_mesh_simplify_workspace_bytes(F), L.pn_voxel_workspace_bytes(V)
    wm = torch.empty(max(mb, vb), device=dev, dtype=torch.uint8)
    vo, fo, lo = torch.empty(min(V, 3 * F), 3, device=dev), torch.empty(F, 3, device=dev, dtype=torch.int32), torch.empty(F, device=dev, dtype=torch.int32)
    cent, vn = torch.empty(V, 3, device=dev), torch.zeros(1, device=dev, dtype=torch.int32)
    full = ops.icp_mesh_reference(v, faces, lab, 1)
    probe = ops.mesh_sample(full, 65536, seed=7)[0]
    eye = torch.eye(4, device=dev)[None].contiguous()
    zeros = torch.zeros(1, probe.shape[1], device=dev, dtype=torch.int32)
    rng = np.random.default_rng(20260010)
    scan = ops.mesh_sample(full, scan_n, seed=8)[0] + torch.from_numpy(rng.normal(0, 0.02, (1, scan_n, 3)).astype(np.float32)).to(dev)
    start = np.eye(4)
    start[:3, :3] = rot([1, 2, 3], np.deg2rad(2))
    start[:3, 3] = [0.1, -0.1, 0.05]
    I = torch.from_numpy(start[None]).to(dev)
    S, SL = scan.contiguous(), torch.zeros(1, scan_n, device=dev, dtype=torch.int32)
    robust = dict(metric="plane", max_dist=3.0, robust="tukey")
    for leaf in leaves:
        leaf3 = (C.c_float * 3)(leaf, leaf, leaf)
        r = {}
        _, r["voxel_downsample_of_vertices_ms"] = timed(lambda: _lib.check(L.pn_voxel_downsample(_lib.ptr(v), None, V, leaf3, go, 0, _lib.ptr(cent), None,
                                                                                                 None, _lib.ptr(vn), _lib.ptr(wm), vb, st()),
                                                                           "pn_voxel_downsample"), args.reps)
        for name, placement in (("mean", 0), ("quadric", 1)):
            _, ms = timed(lambda: _lib.check(L.pn_mesh_simplify(_lib.ptr(v), V, _lib.ptr(faces), _lib.ptr(lab), F, leaf3, go, placement, 1e-3, _lib.ptr(vo),
                                                                _lib.ptr(fo), _lib.ptr(lo), _lib.ptr(n2), _lib.ptr(wm), mb, st()), "pn_mesh_simplify"),
                          args.reps)
            assert int(wm[:4].view(torch.int32).item()) == 0
            nv, nf = (int(a) for a in n2.tolist())
            small = ops.icp_mesh_reference(vo[:nv], fo[:nf], lo[:nf], 1)
            d2 = ops.icp_mesh_correspond(probe, zeros, small, eye)[1]
            full_ms, small_ms = iter_ms(S, SL, full, I, args.reps, **robust), iter_ms(S, SL, small, I, args.reps, **robust)
            r[name] = {"simplify_ms": ms, "vertices": nv, "faces": nf, "kept_triangles_in_reference": small.T,
                       "error_rms_m": float(d2.double().mean().sqrt()), "error_max_m": float(d2.max().sqrt()),
                       "robust_iter_full_ms": full_ms, "robust_iter_simplified_ms": small_ms}
        out[f"leaf_{leaf:g}"] = r
    return {"simplify": out}


def make_floor_scan(n, share=0.25, seed=20260009):
    """the cluttered C5 scan on a synthetic floor: ``share`` of n extra points, uniform over the scan's footprint, +-0.03 in height,
    half a metre below the scan's lowest point, shuffled in"""
    xyz = make_cluttered_scan(n)
    rng = np.random.default_rng(seed)
    lo, hi = xyz.min(0), xyz.max(0)
    m = int(round(share * n))
    floor = np.stack([rng.uniform(lo[0], hi[0], m), rng.uniform(lo[1], hi[1], m), lo[2] - 0.5 + rng.uniform(-0.03, 0.03, m)], 1)
    out = np.concatenate([xyz, floor.astype(np.float32)]).astype(np.float32)
    rng.shuffle(out)
    return out, m


def bench_plane(args, dev, threshold=0.1, H=1024):
    """pn_plane_segment on the cluttered C5 scan plus a floor: the whole call (one plane, H hypotheses; eager and replayed from a
    graph) and the score pass by difference -- the graph-replayed call at 4 H against H hypotheses, where every other launch does the
    same work: (t(4 H) - t(H)) / 3 is what H further hypotheses cost; the score kernel's own time at H, which includes the hypothesis
    set-up and the tail of a grid of N / 256 workgroups, needs a kernel trace (rocprofv3 --kernel-trace on this command; DESIGN.md
    section 7 records both) -- beside pn_voxel_downsample on the same input and beside the scoring a user would write in torch,
    ((xyz @ normals^T + d).abs() <= thr).sum(0) for the same H planes.  Nothing existed before to compare against."""
    import ctypes as C
    from pointcloudprocessing_amd import _lib, ops
    xyz, n_floor = make_floor_scan(args.points)
    x = torch.from_numpy(xyz).to(dev)
    N = x.shape[0]
    L = _lib.lib()
    planes = torch.empty(1, 4, device=dev, dtype=torch.float64)
    counts = torch.empty(1, device=dev, dtype=torch.int32)
    pid = torch.empty(N, device=dev, dtype=torch.int32)
    nb = L.pn_plane_segment_workspace_bytes(N, 4 * H, 1)
    nb_d = L.pn_voxel_workspace_bytes(N)
    ws = torch.empty(max(nb, nb_d), device=dev, dtype=torch.uint8)

    def call(h):
        _lib.check(L.pn_plane_segment(_lib.ptr(x), N, threshold, h, 1, 1000, 0, None, 1.0, _lib.ptr(planes), _lib.ptr(counts), _lib.ptr(pid), None,
                                      _lib.ptr(ws), nb, _lib.current_stream()), "pn_plane_segment")

    def graphed(h):
        g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call(h)
            with torch.cuda.graph(g, stream=side):
                call(h)
        torch.cuda.current_stream().wait_stream(side)
        return timed_calls(g.replay, args.reps, calls=20)[1]

    _, eager_ms = timed(lambda: call(H), args.reps)
    g1, g4 = graphed(H), graphed(4 * H)
    found, plane = int(counts.item()), planes[0].cpu().tolist()
    score_ms = (g4 - g1) / 3
    pairs = float(N) * H
    _, ops_ms = timed(lambda: ops.plane_segment(x, threshold, hypotheses=H, min_inliers=1000), args.reps)
    # pn_voxel_downsample on the same input
    i32 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.int32)      # noqa: E731
    cent, vcnt, maj, nout = torch.empty(N, 3, device=dev), i32(N), i32(N), i32(1)
    org_c = (C.c_float * 3)(*[float(v) for v in xyz.min(0)])
    leaf_c = (C.c_float * 3)(args.leaf, args.leaf, args.leaf)
    _, down_ms = timed(lambda: _lib.check(L.pn_voxel_downsample(_lib.ptr(x), None, N, leaf_c, org_c, 0, _lib.ptr(cent), _lib.ptr(vcnt), _lib.ptr(maj),
                                                                _lib.ptr(nout), _lib.ptr(ws), nb_d, _lib.current_stream()), "pn_voxel_downsample"),
                       args.reps)
    # the version a user would write: H planes through random triples, scored by one matrix product
    gen = torch.Generator(device="cpu").manual_seed(0)
    tri = x[torch.randint(0, N, (H, 3), generator=gen).to(dev)]
    nrm = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nrm = nrm / nrm.norm(dim=1, keepdim=True).clamp(min=1e-30)
    d = -(nrm * tri[:, 0]).sum(1)
    _, torch_ms = timed(lambda: ((x @ nrm.T + d).abs() <= threshold).sum(0), args.reps)
    valu_rate = 78.6e12          # fp32 VALU operations per second: the 157.3 TFLOP/s vector peak counts a fused multiply-add as two
    return {"plane": {"N": N, "floor_points": n_floor, "hypotheses": H, "threshold": threshold, "floor_found": found, "plane": plane,
                      "plane_segment_ms": eager_ms, "plane_segment_graph_ms": g1, "plane_segment_graph_4H_ms": g4, "score_marginal_ms": score_ms,
                      "score_marginal_pairs_per_s": pairs / (score_ms * 1e-3),
                      "score_marginal_valu_share_at_10_ops": 10 * pairs / (score_ms * 1e-3) / valu_rate,
                      "ops_plane_segment_ms": ops_ms, "voxel_downsample_ms": down_ms, "torch_matmul_score_ms": torch_ms,
                      "torch_over_whole_call": torch_ms / g1, "launches": 1 + 5 + 1}}


def bench_fpfh(args, dev, k=16):
    """The start of an unlabelled registration (--fpfh-only; not part of the default run): pn_fpfh on a bumpy sheet of 16,384 and
    131,072 evenly dense points (64 per square unit, a radius that holds about 24) beside pn_scan_normals at the same radius and k in
    the same run (it shares the sort, the gather and the walk, so it is the yardstick); pn_feature_match at 4,096 x 4,096 and 16,384 x
    16,384 descriptors beside torch.cdist(a, b).argmin(1); pn_ransac_poses at 4,096 correspondences (half of them right) with 4,096
    and 65,536 hypotheses; and one ops.global_register call end to end on the registration fixture of tests/fpfh_oracle.py."""
    from pointcloudprocessing_amd import _lib, ops
    L = _lib.lib()
    st = _lib.current_stream
    out = {}
    radius = float(np.sqrt(24.0 / (64.0 * np.pi)))
    org_c = (_lib.C.c_float * 3)(-1.0, -1.0, -3.0)
    feats = {}
    for N in (16384, 131072):
        rng = np.random.default_rng(N)
        side = np.sqrt(N) / 8.0
        u, v = rng.random(N) * side, rng.random(N) * side
        x = torch.from_numpy(np.stack([u, v, np.sin(u) * np.cos(0.7 * v) + rng.normal(0.0, 0.01, N)], 1).astype(np.float32)).to(dev)
        nb = L.pn_fpfh_workspace_bytes(N, k)
        ws = torch.empty(nb, device=dev, dtype=torch.uint8)
        nrm, curv = torch.empty(N, 3, device=dev), torch.empty(N, device=dev)
        cnt = torch.empty(N, device=dev, dtype=torch.int32)
        f = torch.empty(N, 33, device=dev)
        vp = (_lib.C.c_float * 3)(side / 2, side / 2, 50.0)
        _, nrm_ms = timed(lambda: _lib.check(L.pn_scan_normals(_lib.ptr(x), N, radius, org_c, k, vp, _lib.ptr(nrm), _lib.ptr(curv), _lib.ptr(cnt), None,
                                                               _lib.ptr(ws), nb, st()), "pn_scan_normals"), args.reps)
        _, fpfh_ms = timed(lambda: _lib.check(L.pn_fpfh(_lib.ptr(x), _lib.ptr(nrm), N, radius, org_c, k, _lib.ptr(f), None, None, _lib.ptr(ws), nb, st()),
                                              "pn_fpfh"), args.reps)
        _, ops_ms = timed(lambda: ops.fpfh(x, nrm, radius, k), args.reps)
        assert int(ws[:4].view(torch.int32).item()) == 0 and bool(torch.isfinite(f).all())
        feats[N] = f
        out.update({f"fpfh_n{N}_ms": fpfh_ms, f"scan_normals_n{N}_ms": nrm_ms, f"ops_fpfh_n{N}_ms": ops_ms, f"fpfh_over_normals_n{N}": fpfh_ms / nrm_ms,
                    f"mean_neighbours_n{N}": float(cnt.float().mean())})
    for n in (4096, 16384):
        a, b = feats[16384][:n].contiguous(), feats[131072][:n].contiguous()
        nb = L.pn_feature_match_workspace_bytes(n, n)
        ws = torch.empty(nb, device=dev, dtype=torch.uint8)
        idx, d2 = torch.empty(n, device=dev, dtype=torch.int32), torch.empty(n, device=dev)
        _, ms = timed(lambda: _lib.check(L.pn_feature_match(_lib.ptr(a), n, _lib.ptr(b), n, 33, _lib.ptr(idx), _lib.ptr(d2), _lib.ptr(ws), nb, st()),
                                         "pn_feature_match"), args.reps)
        ti, tms = timed(lambda: torch.cdist(a, b).argmin(1), args.reps)
        out.update({f"feature_match_{n}_ms": ms, f"torch_cdist_argmin_{n}_ms": tms, f"feature_match_{n}_pairs_per_s": n * n / (ms * 1e-3),
                    f"feature_match_{n}_agrees_with_cdist": float((ti == idx.long()).float().mean())})
    rng = np.random.default_rng(7)
    Cn = 4096
    q = rng.uniform(-2.0, 2.0, (Cn, 3))
    p = q @ rot([0.2, -0.4, 0.9], 2.5).T + [1.5, -2.0, 0.8] + rng.normal(0, 0.002, (Cn, 3))
    p[rng.permutation(Cn)[:Cn // 2]] = rng.uniform(-3.0, 3.0, (Cn // 2, 3))
    src, tgt = (torch.from_numpy(a.astype(np.float32)).to(dev) for a in (p, q))
    for H in (4096, 65536):
        nb = L.pn_ransac_poses_workspace_bytes(Cn, H)
        ws = torch.empty(nb, device=dev, dtype=torch.uint8)
        poses, counts = torch.empty(H, 4, 4, device=dev, dtype=torch.float64), torch.empty(H, device=dev, dtype=torch.int32)
        _, ms = timed(lambda: _lib.check(L.pn_ransac_poses(_lib.ptr(src), _lib.ptr(tgt), Cn, 0.02, H, 0.9, 0, _lib.ptr(poses), _lib.ptr(counts), None,
                                                           _lib.ptr(ws), nb, st()), "pn_ransac_poses"), args.reps)
        out.update({f"ransac_poses_h{H}_ms": ms, f"ransac_poses_h{H}_pair_tests_per_s": float((counts >= 0).sum()) * Cn / (ms * 1e-3),
                    f"ransac_poses_h{H}_valid": int((counts >= 0).sum()), f"ransac_poses_h{H}_best": int(counts.max())})
    FO = _test_module("fpfh_oracle")
    sc, S = FO.scene(), FO.SCENE
    s, t = torch.from_numpy(sc["source"]).to(dev), torch.from_numpy(sc["target"]).to(dev)
    res, ms = timed(lambda: ops.global_register(s, t, S["feature_radius"], S["max_dist"], normals_radius=S["normals_radius"], hypotheses=S["hypotheses"],
                                                keep=S["keep"], top=S["top"], seed=S["seed"], source_viewpoint=sc["source_viewpoint"].tolist(),
                                                target_viewpoint=sc["target_viewpoint"].tolist(), max_iters=S["max_iters"]), args.reps)
    err = res[0][0].cpu().numpy() @ np.linalg.inv(sc["pose"])
    out.update({"global_register_ms": ms, "global_register_points": [int(s.shape[0]), int(t.shape[0])], "global_register_winner": int(res[6][0]),
                "global_register_rot_err_deg": float(np.degrees(np.arccos(np.clip((np.trace(err[:3, :3]) - 1) / 2, -1, 1)))),
                "global_register_t_err_m": float(np.linalg.norm(res[0][0].cpu().numpy()[:3, 3] - sc["pose"][:3, 3]))})
    return {"fpfh": out}


def bench_icp(args, model, x, origin, dev):
    from pointcloudprocessing_amd import ops, pointcloud
    kx, kp = pointcloud.read_labelled_cloud(os.path.join(ROOT, "tests", "golden", "kc-46.txt"), PARTS)
    ref = ops.icp_reference(kx, kp, len(PARTS), device=dev)
    true = np.eye(4)
    true[:3, :3] = rot([0.3, -0.5, 0.8], 0.7)
    true[:3, 3] = [12.0, -4.0, 30.0]
    start = np.eye(4)
    start[:3, :3] = rot([1, 1, 0], np.deg2rad(10)) @ true[:3, :3]
    start[:3, 3] = true[:3, 3] + [0.6, -0.5, 0.6]
    scan, lab = make_labelled_scan(args.points, kx, kp, true)
    S = torch.from_numpy(scan[None]).to(dev)
    L = torch.from_numpy(lab[None]).to(dev)
    I = torch.from_numpy(start[None]).to(dev)

    def timed(fn):
        out, ts = None, []
        for rep in range(args.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            if rep:
                ts.append(e0.elapsed_time(e1))
        return out, float(np.median(ts))

    res, icp_ms = timed(lambda: ops.semantic_icp(S, L, ref, I, max_iters=30))
    _, one_ms = timed(lambda: ops.semantic_icp(S, L, ref, I, max_iters=1))
    _, full_ms = timed(lambda: ops.semantic_icp(S, L, ref, I, max_iters=30, tol_rot=0.0, tol_t=0.0))   # all 30 iterations run
    # the same 30 iterations replayed from a CUDA graph (launch overhead gone)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        ops.semantic_icp(S, L, ref, I, max_iters=30, tol_rot=0.0, tol_t=0.0)
        with torch.cuda.graph(g, stream=side):
            ops.semantic_icp(S, L, ref, I, max_iters=30, tol_rot=0.0, tol_t=0.0)
    torch.cuda.current_stream().wait_stream(side)
    _, graph_ms = timed(lambda: g.replay())
    pose, rmse, pairs, iters, status = (t.cpu().numpy() for t in res)
    seg = np.asarray(ref.seg)
    act = (lab >= 0) & (lab < len(PARTS))
    evals = int((seg[1:] - seg[:-1])[lab[act]].sum())           # same-label distances of one correspondence pass
    ang = float(np.arccos(np.clip((np.trace(pose[0, :3, :3].T @ true[:3, :3]) - 1) / 2, -1, 1)))
    _, pp_ms = timed(lambda: model.predict_pose(x, ref, leaf=args.leaf, samples=args.samples, k=args.k, origin=origin))
    return {"icp_ms": icp_ms, "icp_iters": int(iters[0]), "icp_status": int(status[0]),
            "icp_iter_ms": (full_ms - one_ms) / 29, "icp_30_iter_graph_ms": graph_ms,
            "icp_pairs_per_s": evals * 30 / (full_ms * 1e-3), "icp_pairs": int(pairs[0]), "icp_rmse_m": float(rmse[0]),
            "icp_error_rad": ang, "icp_error_m": float(np.linalg.norm(pose[0, :3, 3] - true[:3, 3])), "predict_pose_ms": pp_ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=131072)
    ap.add_argument("--leaf", type=float, default=0.25)
    ap.add_argument("--samples", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--mesh-only", action="store_true", help="only the triangle-mesh ICP section")
    ap.add_argument("--global-only", action="store_true", help="only the global-start section")
    ap.add_argument("--lidar-only", action="store_true", help="only the LiDAR simulator section")
    ap.add_argument("--sensor-only", action="store_true", help="only the LiDAR sensor model section")
    ap.add_argument("--sample-only", action="store_true", help="only the mesh sampler section")
    ap.add_argument("--robust-only", action="store_true", help="only the robust ICP section")
    ap.add_argument("--bvh-only", action="store_true", help="only the accelerated mesh ICP section")
    ap.add_argument("--cluster-only", action="store_true", help="only the voxel connected components section")
    ap.add_argument("--denoise-only", action="store_true", help="only the radius k-NN / outlier removal section")
    ap.add_argument("--dbscan-only", action="store_true", help="only the exact DBSCAN section")
    ap.add_argument("--plane-only", action="store_true", help="only the RANSAC plane segmentation section")
    ap.add_argument("--normals-only", action="store_true", help="only the per-point normals section")
    ap.add_argument("--grid-only", action="store_true", help="only the voxel-grid cloud ICP section")
    ap.add_argument("--fpfh-only", action="store_true", help="only the FPFH / feature matching / RANSAC pose section")
    ap.add_argument("--gicp-only", action="store_true", help="only the plane-to-plane (generalized ICP) section")
    ap.add_argument("--multiway-only", action="store_true", help="only the multiway registration / pose graph section")
    ap.add_argument("--recon-only", action="store_true", help="only the surface reconstruction (IMLS field, marching tetrahedra) section")
    ap.add_argument("--simplify-only", action="store_true", help="only the mesh cleaning (components, vertex-clustering simplification) section")
    ap.add_argument("--parent-lib", default=None, help="--grid-only: another build of libpointnet_hip.so whose pn_icp_correspond is timed alongside")
    args = ap.parse_args()
    from pointcloudprocessing_amd import ops
    from pointcloudprocessing_amd.pointnet.PointNet import PointNet
    dev = torch.device("cuda:0")
    if args.grid_only:
        print(json.dumps(bench_grid(args, dev)))
        return
    if args.fpfh_only:
        print(json.dumps(bench_fpfh(args, dev)))
        return
    if args.recon_only:
        print(json.dumps(bench_recon(args, dev)))
        return
    if args.simplify_only:
        print(json.dumps(bench_simplify(args, dev)))
        return
    if args.dbscan_only:
        print(json.dumps(bench_dbscan(args, dev)))
        return
    if args.gicp_only:
        print(json.dumps(bench_gicp(args, dev)))
        return
    if args.multiway_only:
        print(json.dumps(bench_multiway(args, dev)))
        return
    if args.mesh_only:
        print(json.dumps(bench_icp_mesh(args, dev)))
        return
    if args.global_only:
        print(json.dumps(bench_global(args, dev)))
        return
    if args.lidar_only:
        print(json.dumps(bench_lidar(args, dev)))
        return
    if args.sensor_only:
        print(json.dumps(bench_sensor(args, dev)))
        return
    if args.sample_only:
        print(json.dumps(bench_sample(args, dev)))
        return
    if args.robust_only:
        print(json.dumps(bench_robust(args, dev)))
        return
    if args.bvh_only:
        print(json.dumps(bench_bvh(args, dev)))
        return
    if args.cluster_only:
        print(json.dumps(bench_cluster(args, dev)))
        return
    if args.denoise_only:
        print(json.dumps(bench_denoise(args, dev)))
        return
    if args.plane_only:
        print(json.dumps(bench_plane(args, dev)))
        return
    if args.normals_only:
        print(json.dumps(bench_normals(args, dev)))
        return
    xyz, origin = make_scan(args.points)
    x = torch.from_numpy(xyz).to(dev)
    model = PointNet(23, 12, 0.3, 42, vanilla=True, precision="bf16", device=dev)   # kc46_lidar_config.json: vanilla
    leaf = (args.leaf,) * 3
    times = {"voxel_ms": [], "fps_ms": [], "inference_ms": [], "propagate_ms": [], "full_resolution_ms": []}
    for rep in range(args.reps + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
        ev[0].record()
        cent, cnt, _ = ops.voxel_downsample(x, leaf, origin)
        ev[1].record()
        V = cent.shape[0]
        M = min(args.samples, V)
        idx = ops.farthest_point_sample(cent.unsqueeze(0).contiguous(), M)
        ev[2].record()
        cloud = cent[idx[0].long()].unsqueeze(0).contiguous()
        cls_idx, part_idx, R = model.predict(cloud)          # class index, per-point part indices (device-side arg-max), pose
        ev[3].record()
        _, seg, _ = model(cloud, training=False)              # the probabilities the propagation mixes (untimed)
        ev[4].record()
        ops.knn_propagate(x.unsqueeze(0), cloud, args.k, values=seg)
        ev[5].record()
        torch.cuda.synchronize()
        ev[6].record()
        _, full_part, _ = model.predict_scan(x, leaf=args.leaf, samples=args.samples, k=args.k, origin=origin)
        ev[7].record()
        torch.cuda.synchronize()
        if rep:
            times["voxel_ms"].append(ev[0].elapsed_time(ev[1]))
            times["fps_ms"].append(ev[1].elapsed_time(ev[2]))
            times["inference_ms"].append(ev[2].elapsed_time(ev[3]))
            times["propagate_ms"].append(ev[4].elapsed_time(ev[5]))
            times["full_resolution_ms"].append(ev[6].elapsed_time(ev[7]))
    out = {"workload": f"scan N={args.points} -> voxel {args.leaf} m ({V} voxels) -> FPS M={M} -> PointNet(vanilla) inference -> k={args.k} propagation to all points",
           **{k: float(np.median(v)) for k, v in times.items()},
           "fps_distance_updates_per_s": float(M * V / (np.median(times["fps_ms"]) * 1e-3)),
           "knn_pairs_per_s": float(args.points * M / (np.median(times["propagate_ms"]) * 1e-3)),
           "propagated_part_histogram": torch.bincount(full_part[0].long(), minlength=12).tolist(),
           "class": int(cls_idx[0]), "part_histogram": torch.bincount(part_idx[0].long(), minlength=12).tolist()}
    out.update(bench_icp(args, model, x, origin, dev))
    out.update(bench_icp_plane(args, dev))
    out.update(bench_icp_mesh(args, dev))
    out.update(bench_global(args, dev))
    out.update(bench_lidar(args, dev))
    out.update(bench_sensor(args, dev))
    out.update(bench_sample(args, dev))
    out.update(bench_robust(args, dev))
    out.update(bench_bvh(args, dev))
    out.update(bench_cluster(args, dev, model))
    out.update(bench_denoise(args, dev, model))
    out.update(bench_plane(args, dev))
    out.update(bench_normals(args, dev))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
