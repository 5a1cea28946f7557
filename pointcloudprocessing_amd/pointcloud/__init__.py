from .labelled import read_labelled_cloud

__all__ = ["read_labelled_cloud"]
