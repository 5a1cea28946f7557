from .labelled import read_labelled_cloud
from .lidar import LIDAR_KINDS, look_at_pose, pinhole_rays, sample_dataset, sample_viewpoints, simulate_dataset, write_labelled_cloud
from .mesh import read_labelled_mesh, write_labelled_mesh

__all__ = ["read_labelled_cloud", "read_labelled_mesh", "write_labelled_mesh", "pinhole_rays", "sample_viewpoints", "look_at_pose", "simulate_dataset",
           "sample_dataset", "write_labelled_cloud", "LIDAR_KINDS"]
