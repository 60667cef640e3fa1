"""simple-knn's extension module under its import name: distCUDA2(points [P,3] f32 on the GPU) -> [P] f32, the mean squared
distance of every point to its three nearest other points (simple_knn.cu:147-183), computed by gaustar_amd.knn.dist_cuda2
(exact: simple-knn's own search is exact too, its boxes only skip work)."""
from gaustar_amd.knn import dist_cuda2 as distCUDA2  # noqa: F401

__all__ = ["distCUDA2"]
