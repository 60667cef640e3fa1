"""gaustar_amd -- MI355X-native differentiable surface-Gaussian rasterizer (GauSTAR hot path).

    from gaustar_amd import GaussianRasterizationSettings, GaussianRasterizer

is the same API as the reference's `diff_gaussian_rasterization` package; the compute path is
hand-written HIP for gfx950 behind the C ABI of include/gsr.h.  `scene` (numpy only) builds the
synthetic cameras / mesh-bound Gaussians used by tests and bench.py; `dist` is the view-parallel
gradient all-reduce.  Either side of the rasterizer: `producers` (SH -> RGB, mesh-bound
means / scales / quaternions), `losses` (l1 + dssim, masked depth L1, surface-mesh regularisers), `meshes` (single-mesh
stand-ins for pytorch3d's `Meshes` / `mesh_normal_consistency`), `sweep` (forward-only camera sweeps),
`mesh_depth` (a mesh's depth maps, masks and visible faces over the rig: the inputs of a tracked sequence),
`dataprep` (what a sequence needs before frame 0: rectified images, the coloured base mesh, the COLMAP files),
`hull` (shape from silhouettes: the per-frame meshes those inputs are rendered from, carved out of the rig's alpha masks),
`tracking` (points followed on the surface through topology updates: SurfaceTracker, track_faces),
`edit` (what a tracked sequence is for: cutting a model, attaching one that rides on tracked anchors, painting a decal),
`remesh` (quadric mesh decimation and Laplacian / Taubin smoothing: how an init_mesh_100k.obj is made),
`knn` (exact K-nearest neighbours with spatial culling: pytorch3d's knn_points, simple-knn's distCUDA2),
`density` (the Gaussians' density field: SuGaR's compute_density and get_covariance, behind the model's postprocess_mesh),
`evaluate` (how good a result is: point-to-mesh distance, Chamfer distance and F-score of two meshes, PSNR and SSIM of renders) and
`formats` (cameras.json, 3DGS PLY, SuGaR .pt, OBJ, grey and RGB PNG) -- import them as submodules.
"""
from .rasterizer import GaussianRasterizationSettings, GaussianRasterizer, rasterize_gaussians  # noqa: F401
from .tracking import RebindStats, SurfaceTracker, bind_points, track_faces  # noqa: F401
from .remesh import SimplifiedMesh, simplify_mesh, smooth_laplacian, smooth_taubin  # noqa: F401
from .knn import dist_cuda2, knn_points, nearest_neighbors  # noqa: F401

__all__ = ["GaussianRasterizationSettings", "GaussianRasterizer", "rasterize_gaussians", "RebindStats", "SurfaceTracker",
           "bind_points", "track_faces", "SimplifiedMesh", "simplify_mesh", "smooth_laplacian", "smooth_taubin", "nearest_neighbors",
           "knn_points", "dist_cuda2"]
