"""Simulated flash-LiDAR frames of a labelled part mesh: the sensor's ray grid, random viewpoints, look-at poses, a labelled
dataset rendered by ray casting (ops.lidar_frames: pn_lidar_cast + pn_lidar_pack) in the arrays PointCloudSet.add_data takes, and a
writer for the Aftr text format.  The counterpart of the reference's examples/MeshSampler.py: create_viewpoint_observations, which
samples the surface and removes hidden points with Open3D; here the occlusion, the field of view and the raster pattern are the
sensor's own.  create_full_sample_observations, its un-occluded half, is sample_dataset: area-uniform surface samples drawn on the
device (ops.mesh_sample)."""
from typing import Callable, Optional

import numpy as np


def pinhole_rays(height: int, width: int, hfov_deg: float, vfov_deg: float) -> np.ndarray:
    """The ray directions of a height x width pinhole sensor -> (height * width, 3) float32 unit vectors in the sensor frame (+x
    forward, +y left, +z up).  Row 0 is the top of the image, column 0 its left; pixel (r, c) has index r * width + c and looks
    through the centre of its cell: its direction is proportional to (1, tan(hfov / 2) (1 - (2c + 1) / W), tan(vfov / 2) (1 -
    (2r + 1) / H)), computed in fp64, normalised, rounded."""
    if height < 1 or width < 1 or not (0.0 < hfov_deg < 180.0) or not (0.0 < vfov_deg < 180.0):
        raise ValueError(f"pinhole_rays: height, width >= 1 and fields of view inside (0, 180) deg required, got {height} x {width}, "
                         f"{hfov_deg} x {vfov_deg}")
    th, tv = np.tan(np.deg2rad(hfov_deg) / 2.0), np.tan(np.deg2rad(vfov_deg) / 2.0)
    y = th * (1.0 - (2.0 * np.arange(width) + 1.0) / width)
    z = tv * (1.0 - (2.0 * np.arange(height) + 1.0) / height)
    d = np.stack([np.ones((height, width)), np.broadcast_to(y[None, :], (height, width)), np.broadcast_to(z[:, None], (height, width))], -1)
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    return d.reshape(-1, 3).astype(np.float32)


def sample_viewpoints(n: int, dist_range=(5.0, 10.0), az_range=(0.0, 360.0), elev_range=(-5.0, 20.0), seed=None) -> np.ndarray:
    """``n`` sensor positions in the model frame -> (n, 3) float64: distance from the model origin (mesh units), azimuth about the
    z axis (deg) and elevation (deg; 0 = the xy-plane, 90 = +z, -90 = -z) drawn uniformly from their ranges, the meaning
    MeshSampler's arguments have.  ``seed`` seeds a numpy Generator."""
    rng = np.random.default_rng(seed)
    dist = rng.uniform(dist_range[0], dist_range[1], n)
    az = np.deg2rad(rng.uniform(az_range[0], az_range[1], n))
    el = np.deg2rad(rng.uniform(elev_range[0], elev_range[1], n))
    return np.stack([dist * np.cos(az) * np.cos(el), dist * np.sin(az) * np.cos(el), dist * np.sin(el)], axis=1)


def look_at_pose(viewpoint, roll_deg: float = 0.0) -> np.ndarray:
    """The 4 x 4 model-in-sensor pose [R t; 0 0 0 1] (p_sensor = R q_model + t, the convention of ops.semantic_icp) of a sensor at
    ``viewpoint`` (model frame) whose +x axis points at the model origin.  At zero roll the sensor's +y axis (left) is horizontal,
    z_model x forward, and +z completes the right-handed frame (up); on the model's z axis, where that is undefined, +y is the
    model's +y.  ``roll_deg`` then turns the sensor frame about its own x axis: pose = Rx(roll) pose(0).  The model origin maps to
    (|viewpoint|, 0, 0) whatever the roll."""
    c = np.asarray(viewpoint, np.float64).reshape(3)
    dist = np.linalg.norm(c)
    if not np.isfinite(dist) or dist == 0.0:
        raise ValueError(f"look_at_pose: the viewpoint must be finite and away from the model origin, got {c}")
    fwd = -c / dist
    left = np.cross([0.0, 0.0, 1.0], fwd)
    if np.linalg.norm(left) < 1e-12:
        left = np.array([0.0, 1.0, 0.0])
    left = left / np.linalg.norm(left)
    up = np.cross(fwd, left)
    R = np.stack([fwd, left, up])                 # rows: the sensor axes in the model frame, p_sensor = R (q - c)
    a = np.deg2rad(roll_deg)
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])
    R = Rx @ R
    P = np.eye(4)
    P[:3, :3] = R
    P[:3, 3] = -R @ c
    return P


LIDAR_KINDS = ("miss", "return", "dropped", "mixed")     # the kind codes of ops.lidar_sense (PN_LIDAR_MISS .. PN_LIDAR_MIXED)


def simulate_dataset(mesh_ref, class_id: int, viewpoints, dirs, n_points: int, roll_deg=0.0, t_min: float = 0.0,
                     t_max: float = float("inf"), print_func: Optional[Callable[[str], None]] = print, accel=None, sensor=None,
                     seed: int = 0, frame0: int = 0):
    """Render one labelled frame of ``mesh_ref`` (ops.icp_mesh_reference) per viewpoint (F, 3) with the ray grid ``dirs`` (R, 3) on
    the device and pack each to ``n_points`` returns -> (observations (F', n_points, 3) float32 in the sensor frame, class_labels
    (F',) int32 = class_id, part_labels (F', n_points) int32, se3 (F', 3, 3) float32 = the rotation of each frame's pose, the
    quantity the trainer regresses): the arrays PointCloudSet.add_data takes.  ``roll_deg``: one angle or one per viewpoint.  A
    frame in which no ray hits the mesh is dropped, and the dropped frames are reported through ``print_func`` (None: silent).
    ``accel`` = "bvh" casts through the trees of a reference built with icp_mesh_reference(..., accel="bvh") (ops.lidar_cast): the
    same arrays, faster on large meshes.  ``sensor`` = a dict of ops.lidar_sense's model keywords (range_sigma, detection,
    max_incidence_deg, mixed) and ``shape`` = (H, W) of ``dirs``: the frames carry range noise, lost returns and mixed pixels
    (ops.lidar_frames(sensor=...)); the arrays keep their shapes, and a frame whose every return is lost is dropped like one that
    sees nothing.  Viewpoint i is frame index ``frame0`` + i of ``seed``, so the dataset is a pure function of (mesh, viewpoints,
    rays, sensor, seed) however the viewpoints are split over calls: render viewpoints [a, b) with ``frame0`` = a."""
    from .. import ops
    vp = np.asarray(viewpoints, np.float64).reshape(-1, 3)
    roll = np.broadcast_to(np.asarray(roll_deg, np.float64), (len(vp),))
    poses = np.stack([look_at_pose(v, r) for v, r in zip(vp, roll)]) if len(vp) else np.zeros((0, 4, 4))
    if len(vp) == 0:
        return (np.zeros((0, n_points, 3), np.float32), np.zeros((0,), np.int32), np.zeros((0, n_points), np.int32),
                np.zeros((0, 3, 3), np.float32))
    extra = {} if sensor is None else dict(sensor=sensor, seed=seed, frame0=frame0)
    xyz, part, _, count = ops.lidar_frames(mesh_ref, poses, dirs, n_points, t_min=t_min, t_max=t_max, accel=accel, **extra)[:4]
    keep = count.cpu().numpy() > 0
    if not keep.all() and print_func is not None:
        print_func(f"simulate_dataset: {int((~keep).sum())} of {len(vp)} frames see nothing and are dropped: {np.flatnonzero(~keep).tolist()}")
    return (xyz.cpu().numpy()[keep], np.full(int(keep.sum()), class_id, np.int32), part.cpu().numpy()[keep],
            poses[keep, :3, :3].astype(np.float32))


def sample_dataset(mesh_ref, class_id: int, viewpoints, n_points: int, roll_deg=0.0, seed: int = 0, reproject: bool = True):
    """One un-occluded, area-uniform surface sample of ``mesh_ref`` (ops.icp_mesh_reference) per viewpoint (F, 3), drawn on the
    device (ops.mesh_sample: frame i is set i of ``seed``): the counterpart of MeshSampler's create_full_sample_observations, the
    clouds the reference pre-trains its classifier on.  ``reproject``: each set is taken into the sensor frame of
    look_at_pose(viewpoint_i, roll_i), p = R q + t on the host in fp64, rounded once; otherwise it stays in the model frame (the
    reference's default).  -> the four arrays of simulate_dataset: (observations (F, n_points, 3) float32, class_labels (F,) int32
    = class_id, part_labels (F, n_points) int32, se3 (F, 3, 3) float32 = the rotation of each viewpoint's pose).  A mesh without
    area raises ValueError."""
    from .. import ops
    vp = np.asarray(viewpoints, np.float64).reshape(-1, 3)
    F = len(vp)
    if F == 0:
        return (np.zeros((0, n_points, 3), np.float32), np.zeros((0,), np.int32), np.zeros((0, n_points), np.int32),
                np.zeros((0, 3, 3), np.float32))
    roll = np.broadcast_to(np.asarray(roll_deg, np.float64), (F,))
    poses = np.stack([look_at_pose(v, r) for v, r in zip(vp, roll)])
    xyz, part, _ = ops.mesh_sample(mesh_ref, n_points, seed=seed, sets=F)
    xyz, part = xyz.cpu().numpy(), part.cpu().numpy()
    if (part < 0).any():
        raise ValueError("sample_dataset: the mesh has no triangle with a finite positive area")
    if reproject:
        xyz = (np.einsum("fij,fnj->fni", poses[:, :3, :3], xyz.astype(np.float64)) + poses[:, None, :3, 3]).astype(np.float32)
    return xyz, np.full(F, class_id, np.int32), part, poses[:, :3, :3].astype(np.float32)


def write_labelled_cloud(path: str, xyz, class_label: str, part_names, parts) -> int:
    """Write a labelled cloud in the Aftr text format, one "(x, y, z) <class> <part>" per line with %.9g coordinates, which
    read_labelled_cloud returns with the same float32 bits.  xyz (n, 3), parts (n,) part ids into ``part_names``; rows with
    part < 0 are skipped.  -> the number of lines written."""
    x = np.asarray(xyz, np.float32).reshape(-1, 3)
    p = np.asarray(parts).reshape(-1)
    if len(p) != len(x):
        raise ValueError(f"write_labelled_cloud: {len(x)} points but {len(p)} part ids")
    part_names = list(part_names)
    if len(p) and p.max() >= len(part_names):
        raise ValueError(f"write_labelled_cloud: part id {int(p.max())} but only {len(part_names)} part names")
    n = 0
    with open(path, "w") as f:
        for (a, b, c), k in zip(x.tolist(), p.tolist()):
            if k < 0:
                continue
            f.write("(%.9g, %.9g, %.9g) %s %s\n" % (a, b, c, class_label, part_names[k]))
            n += 1
    return n
