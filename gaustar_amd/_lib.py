"""ctypes binding of the C-ABI HIP library (include/gsr.h -> gaustar_amd/libgsr_hip.so).

There is deliberately NO fallback: if the shared library is missing or fails to load, every
entry point raises.  The product path never touches oracle/.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_longlong, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GSR_LIB_PATH", os.path.join(_HERE, "libgsr_hip.so"))   # override: experiment variants

ABI_VERSION = 16
ALLOC_FN = ctypes.CFUNCTYPE(c_void_p, c_void_p, c_size_t)

# name -> (restype, argtypes); mirrors include/gsr.h one to one (tests check both directions).
SIGNATURES = {
    "gsr_abi_version": (c_int, []),
    "gsr_last_error": (c_char_p, []),
    "gsr_geom_bytes": (c_size_t, [c_int]),
    "gsr_image_bytes": (c_size_t, [c_int, c_int]),
    "gsr_binning_bytes": (c_size_t, [c_int, c_int]),
    "gsr_binning_bytes_mt": (c_size_t, [c_int, c_int, c_int]),
    "gsr_grad_scratch_bytes": (c_size_t, [c_int]),
    "gsr_forward_stage1": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_float,
                                   c_int, c_void_p, c_void_p, c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_int),
                                   c_void_p]),
    "gsr_forward_stage2": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p]),
    "gsr_forward_stage2_mt": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_forward_fused": (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_float,
                                  c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p,
                                  POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int), c_void_p]),
    "gsr_plan_bytes": (c_size_t, [c_int, c_int]),
    "gsr_plan_info_new": (POINTER(c_int), []),
    "gsr_plan_info_free": (None, [POINTER(c_int)]),
    "gsr_forward_planned": (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_float,
                                    c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p,
                                    POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int), c_void_p, POINTER(c_int),
                                    POINTER(c_int), c_void_p]),
    "gsr_camera_key": (c_int, [c_void_p, c_longlong, c_longlong, POINTER(ctypes.c_ulonglong)]),
    "gsr_camera_key_begin": (c_int, [c_void_p, c_longlong, c_longlong]),
    "gsr_camera_key_end": (c_int, [POINTER(ctypes.c_ulonglong)]),
    "gsr_release_stream_state": (c_int, [c_void_p]),
    "gsr_forward": (c_int, [ALLOC_FN, ALLOC_FN, ALLOC_FN, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int,
                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p,
                            c_void_p, c_void_p, c_float, c_float, c_int, c_void_p, c_void_p, POINTER(c_int),
                            c_void_p]),
    "gsr_backward": (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float,
                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_backward_mt": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                                c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "gsr_mark_visible": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_debug_export": (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_debug_export_masks": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "gsr_debug_export_units": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_sh_to_rgb": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_sh_to_rgb_backward": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p]),
    "gsr_sh_to_rgbd": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "gsr_sh_to_rgbd_backward": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                        c_void_p, c_void_p]),
    "gsr_sh_colors_split": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                    c_void_p, c_void_p]),
    "gsr_sh_colors_split_backward": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "gsr_mesh_gaussians": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float,
                                   c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "gsr_mesh_gaussians_backward": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "gsr_l1_ssim_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "gsr_l1_ssim": (c_int, [c_int, c_int, c_int, c_void_p, c_longlong, c_longlong, c_longlong, c_void_p, c_longlong,
                            c_longlong, c_longlong, c_float, c_void_p, c_void_p, c_void_p, c_longlong, c_longlong,
                            c_longlong, c_void_p]),
    "gsr_depth_l1_workspace_bytes": (c_size_t, []),
    "gsr_depth_l1": (c_int, [c_int, c_int, c_void_p, c_longlong, c_longlong, c_void_p, c_longlong, c_longlong, c_float,
                             c_float, c_float, c_void_p, c_void_p, c_void_p, c_longlong, c_longlong, c_void_p]),
    "gsr_l1_ssim_backward": (c_int, [c_int, c_int, c_int, c_void_p, c_longlong, c_longlong, c_longlong, c_void_p, c_longlong,
                                     c_longlong, c_longlong, c_float, c_void_p, c_void_p, c_void_p, c_longlong, c_longlong,
                                     c_longlong, c_void_p]),
    "gsr_depth_l1_backward": (c_int, [c_int, c_int, c_void_p, c_longlong, c_longlong, c_void_p, c_longlong, c_longlong, c_float,
                                      c_float, c_float, c_void_p, c_void_p, c_void_p, c_longlong, c_longlong, c_void_p]),
    "gsr_rgb_depth_loss": (c_int, [c_int, c_int, c_int, c_void_p, c_longlong, c_longlong, c_longlong, c_void_p, c_longlong,
                                   c_longlong, c_longlong, c_float, c_void_p, c_int, c_int, c_void_p, c_longlong, c_longlong,
                                   c_void_p, c_longlong, c_longlong, c_float, c_float, c_float, c_void_p, c_void_p, c_void_p]),
    "gsr_rgb_depth_loss_backward": (c_int, [c_int, c_int, c_int, c_void_p, c_longlong, c_longlong, c_longlong, c_void_p, c_longlong,
                                            c_longlong, c_longlong, c_float, c_void_p, c_int, c_int, c_void_p, c_longlong, c_longlong,
                                            c_void_p, c_longlong, c_longlong, c_float, c_float, c_float, c_void_p, c_void_p, c_void_p,
                                            c_longlong, c_longlong, c_longlong, c_void_p, c_longlong, c_longlong, c_void_p]),
    # surface-mesh regularisers (refine.py:676-706): int32 topology from gaustar_amd.meshes.MeshTopology
    "gsr_mesh_reg_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "gsr_mesh_reg_forward": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_float, c_float, c_float, c_void_p, c_void_p, c_void_p]),
    "gsr_mesh_reg_backward": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_float, c_float, c_float, c_void_p, c_void_p, c_int, c_void_p]),
    # mesh Laplacian-smoothing loss and small-area regulariser (refine.py:681-683, :713-718): losses.mesh_smoothness_loss
    "gsr_mesh_lap_workspace_bytes": (c_size_t, [c_int, c_int]),
    "gsr_mesh_lap_forward": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float,
                                     c_float, c_void_p, c_void_p, c_void_p]),
    "gsr_mesh_lap_backward": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float,
                                      c_float, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    # regularisers on the Gaussians' own parameters (refine.py:739-748, :663-669): losses.gaussian_param_loss
    "gsr_param_reg_workspace_bytes": (c_size_t, [c_int]),
    "gsr_param_reg_forward": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_longlong, c_longlong, c_float, c_float,
                                      c_void_p, c_float, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    "gsr_param_reg_backward": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_longlong, c_longlong, c_float, c_float,
                                       c_void_p, c_float, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_int, c_void_p]),
    # rig-wide topology-error detection (refined_mesh.py:697-920): gaustar_amd.topology
    "gsr_topo_view_workspace_bytes": (c_size_t, [c_int, c_int]),
    "gsr_topo_view": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float, POINTER(c_double), c_void_p,
                              c_void_p, c_void_p]),
    "gsr_topo_aggregate": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_double, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                   c_void_p]),
    "gsr_topo_propagate": (c_int, [c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p]),
    "gsr_topo_voxel_keys": (c_int, [c_int, c_void_p, c_void_p, c_double, c_void_p, c_void_p, c_void_p]),
    "gsr_topo_voxel_workspace_bytes": (c_size_t, [c_int]),
    "gsr_topo_voxel_interp": (c_int, [c_int, c_void_p, c_void_p, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p]),
    "gsr_topo_faces": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    # scene-flow mesh warping (warp_mesh.py:216-401): gaustar_amd.warp
    "gsr_vertex_normals": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_warp_view_workspace_bytes": (c_size_t, [c_int, c_int]),
    "gsr_warp_view": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_int), c_void_p, c_void_p,
                              POINTER(c_double), POINTER(c_double), c_void_p, c_void_p, c_void_p]),
    "gsr_warp_aggregate": (c_int, [c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_warp_smooth": (c_int, [c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    # a mesh's depth map, mask and visible face per camera (render_depth_from_mesh.py:13-101): gaustar_amd.mesh_depth
    "gsr_mesh_depth_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "gsr_mesh_depth_view": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_void_p, POINTER(c_double), c_double, c_float, c_int,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    # a sequence's inputs before frame 0: rectified images, the first mesh's vertex colours (ahq2gaustar.py:50-81, :124-160):
    # gaustar_amd.dataprep
    "gsr_image_rectify": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, POINTER(c_double), POINTER(c_double),
                                  POINTER(ctypes.c_ubyte), c_void_p]),
    "gsr_mesh_color_view": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, POINTER(c_double), c_double, c_void_p,
                                    c_void_p]),
    "gsr_mesh_color_workspace_bytes": (c_size_t, [c_int]),
    "gsr_mesh_color_finish": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, POINTER(ctypes.c_ubyte), c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p]),
    # TSDF fusion of the rig's renders and mesh extraction (refined_mesh.py:311-459): gaustar_amd.fusion
    "gsr_fusion_prep_workspace_bytes": (c_size_t, [c_int, c_int]),
    "gsr_fusion_volume_bytes": (c_size_t, [POINTER(c_int)]),
    "gsr_fusion_prep": (c_int, [c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_fusion_touch": (c_int, [c_int, c_int, c_void_p, POINTER(c_double), c_double, c_double, POINTER(c_int), c_void_p, c_void_p]),
    "gsr_fusion_integrate": (c_int, [c_int, c_int, c_void_p, c_void_p, POINTER(c_double), c_double, c_double, POINTER(c_int), c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_fusion_count": (c_int, [POINTER(c_int), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_fusion_emit": (c_int, [POINTER(c_int), c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p]),
    # The four mesh-surgery groups below share one err word (csrc/gsr_mesh.h: index = 1, NaN / not finite = 2, duplicate = 4),
    # which gaustar_amd._meshargs.raise_if decodes for them and for the later mesh features (tracking, evaluate, remesh).
    # re-mesh regions at topology errors: edge multiplicity, face components, boxes, cuts (refined_mesh.py:463-693, front
    # half): gaustar_amd.regions; gsr_regions_cut_emit is the tail of every compaction, after either mark call
    "gsr_regions_edge_keys": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_regions_edge_runs": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_regions_components": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_regions_labels": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_regions_select": (c_int, [c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_regions_boxes": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "gsr_regions_inside": (c_int, [c_int, c_void_p, POINTER(c_double), c_void_p, c_void_p]),
    "gsr_regions_cut_mark": (c_int, [c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_regions_cut_emit": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p]),
    "gsr_regions_gather": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_regions_boundary": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_regions_label_mask": (c_int, [c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    # the stitch of the fused patch into the cut base mesh (refined_mesh.py:114-215, :639, :656-658): gaustar_amd.regions;
    # gsr_stitch_mark is select_faces' and the degenerate passes' mark call
    "gsr_stitch_nn_tile": (c_int, []),
    "gsr_stitch_nn_queries": (c_int, []),
    "gsr_stitch_nearest": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_stitch_check_list": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_stitch_snap_groups": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_stitch_mark": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_stitch_hole_components": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_stitch_hole_move": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_stitch_pos_keys": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_stitch_pos_heads": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_stitch_pos_remap": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_stitch_compose_mask": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "gsr_stitch_vert_map": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_stitch_watertight": (c_int, [c_int, c_void_p, c_void_p, c_void_p]),
    # hole filling by the canonical rule, reference areas, mean edge length (refined_mesh.py:589, :617, :652, :683-687, :484-485):
    # gaustar_amd.regions.fill_small_holes / update_mesh_topology
    "gsr_splice_workspace_bytes": (c_size_t, []),
    "gsr_splice_rim_edges": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p]),
    "gsr_splice_rim_census": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_splice_rim_emit": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_splice_face_areas": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_splice_edge_lengths": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_splice_mean": (c_int, [c_longlong, c_void_p, c_void_p, c_void_p, c_void_p]),
    # the colours a frame hands to the next one (sugar_model.py:578-588, :235-240, :386; refined_mesh.py:183):
    # gaustar_amd.handover
    "gsr_handover_face_colors": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "gsr_handover_vertex_to_face": (c_int, [c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "gsr_handover_face_to_vertex": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_handover_sh_dc": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_handover_gather": (c_int, [c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                    c_void_p]),
    # points followed on the surface through topology updates (tracking_util.py:34-148, :20-27): gaustar_amd.tracking; the
    # err word has the mesh kernels' bits and bit 3 = a re-bound barycentric that is not >= 0
    "gsr_track_nn_tile": (c_int, []),
    "gsr_track_nn_queries": (c_int, []),
    "gsr_track_positions": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_track_centres": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_track_rebind_survivors": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_track_todo": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_track_nearest": (c_int, [c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_track_rebind_displaced": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_int, c_void_p, c_void_p]),
    # scoring a result: point-to-mesh distance, surface samples, distance statistics, image SSE: gaustar_amd.evaluate; the
    # err word has the mesh kernels' bits and bit 3 = sampling weights that are not usable
    "gsr_eval_tile": (c_int, []),
    "gsr_eval_queries": (c_int, []),
    "gsr_eval_max_thresholds": (c_int, []),
    "gsr_eval_workspace_bytes": (c_size_t, []),
    "gsr_eval_gather": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_eval_closest": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p]),
    "gsr_eval_areas": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_eval_sample": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, ctypes.c_ulonglong, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p]),
    "gsr_eval_distance_stats": (c_int, [c_longlong, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_eval_image_sse": (c_int, [c_int, c_int, c_int, c_void_p, c_longlong, c_longlong, c_longlong, c_void_p, c_longlong,
                                   c_longlong, c_longlong, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    # quadric decimation and Laplacian / Taubin smoothing (refined_mesh.py:451-458, cmr_convert.py:262-266): gaustar_amd.remesh;
    # the err word is the mesh kernels'
    "gsr_remesh_setup": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_remesh_keys": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_remesh_vertex_quadrics": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_remesh_edge_heads": (c_int, [c_int, c_void_p, c_void_p, c_void_p]),
    "gsr_remesh_edges": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_remesh_candidates": (c_int, [c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_remesh_select": (c_int, [c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_remesh_cap": (c_int, [c_int, c_int, c_int, POINTER(c_int)]),
    "gsr_remesh_apply": (c_int, [c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_remesh_apply_attr": (c_int, [c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_remesh_narrow": (c_int, [c_longlong, c_void_p, c_void_p, c_void_p]),
    "gsr_remesh_smooth": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_double, c_double, c_int, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p]),
    # exact K-nearest-neighbour search with spatial culling (pytorch3d knn_points, simple-knn distCUDA2) and the rows' uses:
    # gaustar_amd.knn
    "gsr_knn_tile": (c_int, []),
    "gsr_knn_seed": (c_int, []),
    "gsr_knn_queries": (c_int, []),
    "gsr_knn_max_k": (c_int, []),
    "gsr_knn_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "gsr_knn_prepare": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_knn_search": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p,
                               c_void_p]),
    "gsr_knn_mean_d2": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "gsr_knn_segment_mean": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_knn_weighted_mean": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_double, c_void_p, c_void_p]),
    # the Gaussians' density field (sugar_model.py:1017-1040, :619-625): gaustar_amd.density; the err word's bit 0 = an index
    # outside [-1, P)
    "gsr_density_queries_per_wave": (c_int, []),
    "gsr_density_queries_per_workgroup": (c_int, []),
    "gsr_density_pack": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_density_eval": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    # editing a tracked sequence: rigid fit's sums, moving a model with its SH, selecting, cutting, painting
    # (gaustar_tools/internal_use_tools/gstar_edit.py): gaustar_amd.edit; the err word is the mesh kernels'
    "gsr_edit_fit_workspace_bytes": (c_size_t, [c_int, c_int]),
    "gsr_edit_fit_sums": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_edit_transform_points": (c_int, [c_longlong, c_int, c_int, c_void_p, POINTER(c_double), POINTER(c_double), c_void_p, c_void_p]),
    "gsr_edit_rotate_sh": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_edit_faces_in_halfspaces": (c_int, [c_int, c_int, c_void_p, c_void_p, c_int, POINTER(c_int), POINTER(c_double), c_void_p,
                                             c_void_p, c_void_p]),
    "gsr_edit_gather_rows": (c_int, [c_int, c_int, c_void_p, c_int, c_int, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_int),
                                     c_void_p, c_void_p]),
    "gsr_edit_paint": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int,
                               c_void_p, c_int, c_double, c_double, c_int, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p]),
    # shape from silhouettes: a mask's signed distance, the carve of a fusion volume by the rig, its TSDF: gaustar_amd.hull
    "gsr_hull_mask_distance_workspace_bytes": (c_size_t, [c_int, c_int]),
    "gsr_hull_mask_distance": (c_int, [c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "gsr_hull_camera_bytes": (c_int, []),
    "gsr_hull_carve": (c_int, [c_int, c_void_p, c_void_p, c_double, POINTER(c_int), c_void_p, c_void_p, c_void_p]),
    "gsr_hull_finish": (c_int, [POINTER(c_int), c_void_p, c_void_p, c_int, c_double, c_void_p, c_void_p, c_void_p, c_void_p]),
    # plane-sweep stereo behind a depth prior, the photo-consistency refinement of the hull: gaustar_amd.stereo
    "gsr_stereo_camera_bytes": (c_int, []),
    "gsr_stereo_luma": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "gsr_stereo_sweep": (c_int, [c_int, c_int, c_void_p, c_void_p, POINTER(c_double), c_int, c_void_p, c_void_p, POINTER(c_double),
                                 c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_stereo_consistency": (c_int, [c_int, c_int, c_void_p, c_void_p, POINTER(c_double), c_int, c_void_p, c_void_p, c_double, c_int,
                                       c_void_p, c_void_p]),
    "gsr_stereo_merge": (c_int, [POINTER(c_int), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p]),
    # RAFT optical flow, the basic model's inference (data_process/RAFT): gaustar_amd.flow; FlowSlice / FlowConvDesc below
    "gsr_flow_packed_k": (c_int, [c_int]),
    "gsr_flow_packed_n": (c_int, [c_int]),
    "gsr_flow_prep_image": (c_int, [c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "gsr_flow_conv": (c_int, [c_void_p, c_void_p]),
    "gsr_flow_pack_features": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "gsr_flow_corr_volume": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_flow_corr_pool": (c_int, [c_longlong, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "gsr_flow_corr_lookup": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_flow_instance_norm_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "gsr_flow_instance_norm": (c_int, [c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_flow_gru_combine": (c_int, [c_longlong, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gsr_flow_upsample": (c_int, [c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "gsr_adam_step": (c_int, [c_longlong, c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_double, c_double, c_double, c_int,
                              c_void_p]),
    "gsr_adam_step_multi": (c_int, [c_int, POINTER(c_longlong), POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p),
                                    POINTER(c_void_p), POINTER(c_double), c_double, c_double, c_double, c_int, c_void_p]),
    "gsr_debug_set_bwd_order": (c_int, [c_void_p]),
    "gsr_debug_preprocess_occupancy": (c_int, [POINTER(c_int), POINTER(c_int)]),
    "gsr_debug_set_trace": (c_int, [c_void_p]),
    "gsr_num_stages": (c_int, []),
    "gsr_stage_name": (c_char_p, [c_int]),
    "gsr_profile_enable": (c_int, [c_int]),
    "gsr_profile_read": (c_int, [POINTER(c_float), POINTER(c_int), c_int]),
    "gsr_debug_host_wait": (c_int, [POINTER(c_longlong), POINTER(c_longlong), c_int]),
}



class PlanInfo(ctypes.Structure):
    """gsr_plan_info of include/gsr.h, field for field: what the GSR_PLAN_INFO_INTS ints of a plan_info block mean."""
    _fields_ = [("state", c_int), ("R_cap", c_int), ("U_cap", c_int), ("max_cap", c_int), ("level", c_int), ("half", c_int),
                ("pending_half", c_int), ("reserved0", c_int), ("header", c_int * 8), ("arrived", c_int), ("pending", c_int),
                ("diag", c_int * 4), ("reserved1", c_int * 10)]


class FlowSlice(ctypes.Structure):
    """gsr_flow_slice of include/gsr.h: `channels` channels from `offset` of a buffer of `stride` floats per pixel."""
    _fields_ = [("base", c_void_p), ("stride", c_longlong), ("offset", c_int), ("channels", c_int)]


class FlowConvDesc(ctypes.Structure):
    """gsr_flow_conv_desc of include/gsr.h, field for field."""
    _fields_ = [("N", c_int), ("H", c_int), ("W", c_int), ("KH", c_int), ("KW", c_int), ("stride", c_int), ("n_in", c_int),
                ("Cout", c_int), ("act", c_int), ("residual_relu", c_int), ("inputs", FlowSlice * 3), ("out", FlowSlice),
                ("residual", FlowSlice), ("weights", c_void_p), ("bias", c_void_p), ("scale", c_void_p), ("shift", c_void_p)]


PLAN_INFO_INTS = 32
PH_VALID, PH_T, PH_R_CAP, PH_U_CAP, PH_MAX_CAP, PH_NONEMPTY, PH_ENTRIES, PH_LONGEST = range(8)   # words of PlanInfo.header

_lib = None


class GsrError(RuntimeError):
    """A C-ABI call returned non-zero (message from gsr_last_error)."""


def load():
    """Load libgsr_hip.so (once).  Raises if the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"gaustar_amd: HIP extension not found at {LIB_PATH}. Build it with "
            "`python -m gaustar_amd.build` (hipcc, gfx950). There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError if the library lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    v = lib.gsr_abi_version()
    if v != ABI_VERSION:
        raise ImportError(f"gaustar_amd: libgsr_hip.so has ABI {v}, Python side expects {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().gsr_last_error()
        raise GsrError(f"{what} failed: {msg.decode() if msg else rc}")


def ptr(t):
    """A tensor's data pointer as a c_void_p argument (None: a null pointer)."""
    return None if t is None else c_void_p(t.data_ptr())
