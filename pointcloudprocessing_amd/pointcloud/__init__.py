from .labelled import read_labelled_cloud
from .mesh import read_labelled_mesh

__all__ = ["read_labelled_cloud", "read_labelled_mesh"]
