"""
ctypes binding of the C-ABI shared library (include/topo4d_raster.h).

The library is built in-tree by `__graft_entry__.build()` / `python -m topo4d_amd.build` with
`hipcc --offload-arch=gfx950`.  There is NO fallback: if the shared object is missing or does not load, every
entry point of the product raises — a rasterizer that silently ran on the CPU would void every parity claim.

Every entry point is bound from one table, SIGNATURES (tests/test_abi.py pins it to the header); `ptr`, `stream`, `call`,
`error`, `hip_device`, `on_device`, `scratch` and `read_back` are what the wrappers of the other modules share (their argument
checks for images and masks are in _args.py).
"""
from __future__ import annotations

import ctypes as C
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
# T4D_LIB: load another build of the SAME library (an experiment build next to the shipped one, tools/ab_build.sh); there
# is still no fallback - a path that does not load raises.
LIB_PATH = os.environ.get("T4D_LIB") or os.path.join(HERE, "csrc", "libtopo4d_raster.so")

T4D_ABI_VERSION = 4
T4D_VIEW_FLOATS = 40
T4D_GRAD_PAIR_FLOATS = 10

T4D_OK, T4D_ERR_ARG, T4D_ERR_HIP, T4D_ERR_PAIR_OVERFLOW, T4D_ERR_STATE_SIZE = 0, 1, 2, 3, 4
T4D_FLAG_CHECKED, T4D_FLAG_DEBUG_SYNC, T4D_FLAG_PREFILTERED, T4D_FLAG_ASYNC_STATUS, T4D_FLAG_NO_LONG_BINS = 1, 2, 4, 8, 16
T4D_FLAG_SHORT_BINS = 32
T4D_FLAG_LONG_LISTS = 64
T4D_FLAG_RAW_PARAMS = 128

class T4DProblem(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("n_views", C.c_int32), ("P", C.c_int32), ("H", C.c_int32),
                ("W", C.c_int32), ("sh_degree", C.c_int32), ("sh_coeffs", C.c_int32),
                ("scale_modifier", C.c_float), ("pair_capacity", C.c_int64), ("flags", C.c_uint32),
                ("views_per_param_set", C.c_uint32)]


class T4DStatus(C.Structure):
    _fields_ = [("max_pairs_per_view", C.c_int64), ("total_pairs", C.c_int64), ("overflow", C.c_int32),
                ("max_tile_pairs", C.c_int32)]


class T4DForwardIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "views", "means3D", "opacities", "scales", "rotations", "cov3D_precomp", "colors_precomp", "shs",
        "out_color", "out_depth", "out_alpha", "out_radii", "state")] + [("state_bytes", C.c_size_t)]


class T4DBackwardIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "views", "means3D", "opacities", "scales", "rotations", "cov3D_precomp", "colors_precomp", "shs",
        "radii", "state")] + [("state_bytes", C.c_size_t)] + [(n, C.c_void_p) for n in (
            "dL_dcolor", "dL_ddepth", "dL_dalpha", "dL_dmeans3D", "dL_dmeans2D", "dL_dcolors", "dL_dshs",
            "dL_dopacities", "dL_dscales", "dL_drotations", "dL_dcov3D", "scratch")] + [
                ("scratch_bytes", C.c_size_t), ("cotangent_dot", C.c_void_p)]


class T4DKernelTime(C.Structure):
    _fields_ = [("name", C.c_char_p), ("total_ms", C.c_double), ("launches", C.c_int64)]


T4D_ADAM_MAX_TENSORS = 12
T4D_MAX_MASK_LABELS = 16


class T4DAdamTensor(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("pin_mask", C.c_void_p), ("pin_values", C.c_void_p), ("rows", C.c_int64), ("width", C.c_int32),
                ("lr", C.c_float), ("step", C.c_int32), ("flags", C.c_int32)]


T4D_ADAM_CLEAR_GRAD = 1


T4D_PRIORS_TERMS = 14
T4D_PRIORS_EDGE_TERMS = 6
T4D_PRIORS_REGION_TERMS = 3
T4D_PRIORS_ACCUMULATE = 1


class T4DPriors(C.Structure):
    _fields_ = [("P", C.c_int32), ("K", C.c_int32)] + [(n, C.c_void_p) for n in (
        "nbr", "nbr_dist", "rig_w", "rot_w", "iso_w", "nbr_mask", "nbr_num", "init_scale")] + [
        ("n_edges", C.c_int32 * T4D_PRIORS_EDGE_TERMS), ("edges", C.c_void_p * T4D_PRIORS_EDGE_TERMS),
        ("n_region", C.c_int32 * T4D_PRIORS_REGION_TERMS), ("region", C.c_void_p * T4D_PRIORS_REGION_TERMS),
        ("nbr_t_off", C.c_void_p), ("nbr_t_idx", C.c_void_p), ("rec_off", C.c_void_p * 2), ("rec_idx", C.c_void_p * 2),
        ("weights", C.c_float * T4D_PRIORS_TERMS), ("prev_inv_rot", C.c_void_p), ("prev_offset", C.c_void_p),
        ("cos_init", C.c_void_p * 4)]


T4D_KNN_MAX_K = 15


class T4DDenseMesh(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_vert", "n_uv", "n_quads", "density", "n_tri", "n_rest")] + [
        ("n_points", C.c_int64), ("n_faces", C.c_int64)] + [(n, C.c_void_p) for n in (
            "vertices", "uvs", "quads", "uv_quads", "plan", "src", "tri", "uv_tri", "rest", "uv_rest",
            "dense_vertex", "vertex_father", "vertex_weight", "dense_uvs", "faces", "uv_faces")]


class T4DJpegImage(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "h_samp", "v_samp", "restart_interval", "reserved0")] + [
        (n, C.c_int64) for n in ("data_offset", "data_bytes", "out_offset")] + [
        (n, C.c_uint8 * 3) for n in ("comp_quant", "comp_dc", "comp_ac")] + [
        ("reserved1", C.c_uint8 * 7), ("quant", (C.c_uint16 * 64) * 4), ("huff_bits", (C.c_uint8 * 16) * 8),
        ("huff_vals", (C.c_uint8 * 256) * 8)]


class T4DPngImage(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "channels", "bytes_per_sample", "first_chunk", "n_chunks")] + [
        ("out_offset", C.c_int64)]


class T4DWarpView(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p)] + [(n, C.c_int32) for n in (
        "rows", "cols", "channels", "src_pitch", "out_rows", "out_cols")] + [("matrix", C.c_double * 6), ("cval", C.c_double)]


T4D_LENS_MAX_SUPERSAMPLE = 64


class T4DLensView(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p)] + [(n, C.c_int32) for n in (
        "rows", "cols", "channels", "src_pitch", "out_rows", "out_cols", "supersample", "nearest")] + [
        ("matrix", C.c_double * 6), ("lens", C.c_double * 11), ("cval", C.c_double)]


class T4DJpegEncImage(C.Structure):
    _fields_ = [("src", C.c_void_p)] + [(n, C.c_int32) for n in ("width", "height", "src_pitch", "reserved")] + [
        ("out_offset", C.c_int64)]


_VP, _I32, _I64, _F32, _SZ, _INT =C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_size_t, C.c_int
_PROB = C.POINTER(T4DProblem)

# name -> (restype, argtypes) of every function include/topo4d_raster.h declares, in header order (tests/test_abi.py checks the
# names against the header and the .so, and every signature against its prototype); a data pointer or stream is a c_void_p
SIGNATURES = {
    "t4d_abi_version": (C.c_uint32, []),
    "t4d_last_error": (C.c_char_p, []),
    "t4d_state_bytes": (_SZ, [_PROB]),
    "t4d_backward_scratch_bytes": (_SZ, [_PROB]),
    "t4d_rasterize_forward": (_INT, [_PROB, C.POINTER(T4DForwardIO), C.POINTER(T4DStatus), _VP]),
    "t4d_rasterize_backward": (_INT, [_PROB, C.POINTER(T4DBackwardIO), _VP]),
    "t4d_fetch_status": (_INT, [_PROB, _VP, C.POINTER(T4DStatus), _VP]),
    "t4d_mark_visible": (_INT, [_I32] + [_VP] * 4),
    "t4d_view_dot_scratch_bytes": (_SZ, [_I32]),
    "t4d_view_dot": (_INT, [_I32, _I64] + [_VP] * 5),
    "t4d_sum_views": (_INT, [_I32, _I32, C.POINTER(_VP), C.POINTER(_VP), C.POINTER(_I64), _VP]),
    "t4d_photometric_scratch_bytes": (_SZ, [_I32] * 3),
    "t4d_photometric_loss": (_INT, [_I32] * 3 + [_VP] * 10 + [_SZ, _VP]),
    "t4d_masked_l1_scratch_bytes": (_SZ, [_I32]),
    "t4d_masked_l1_loss": (_INT, [_I32] * 3 + [_VP] * 7 + [_SZ, _VP]),
    "t4d_label_mask_target": (_INT, [_I32, _I32, _I32, _VP, C.POINTER(_F32), _I32, _VP, _F32, _VP, _VP, _VP]),
    "t4d_soft_color_scratch_bytes": (_SZ, []),
    "t4d_soft_color_loss": (_INT, [_I64, _I32, _VP, _VP, _F32, _VP, _VP, _I32, _VP, _SZ, _VP]),
    "t4d_priors_record_layout": (_I64, [C.POINTER(T4DPriors), C.POINTER(_I64)]),
    "t4d_priors_scratch_bytes": (_SZ, [C.POINTER(T4DPriors)]),
    "t4d_priors_eval": (_INT, [C.POINTER(T4DPriors), _I32] + [_VP] * 7 + [C.c_uint32, _VP, _VP, _SZ, _VP]),
    "t4d_adam_pin_step": (_INT, [C.POINTER(T4DAdamTensor), _I32, _F32, _F32, _F32, _VP]),
    "t4d_adam_step_counters": (_I64, [C.POINTER(T4DAdamTensor), _I32]),
    "t4d_adam_pin_step_graph": (_INT, [C.POINTER(T4DAdamTensor), _I32, _F32, _F32, _F32, _VP, _I64, _VP, _VP]),
    "t4d_dense_interpolate": (_INT, [_VP] * 4 + [_I64, _I64, _I32, _VP, _VP]),
    "t4d_dense_scratch_bytes": (_SZ, [C.POINTER(T4DDenseMesh)]),
    "t4d_dense_build": (_INT, [C.POINTER(T4DDenseMesh), _VP, _SZ, _VP]),
    "t4d_knn_scratch_bytes": (_SZ, [_I64, _I32]),
    "t4d_knn_mean_sq_dist": (_INT, [_VP, _I64, _I32, _VP, _VP, _VP, _SZ, _VP]),
    "t4d_activate_forward": (_INT, [_I64] + [_VP] * 7),
    "t4d_activate_backward": (_INT, [_I64] + [_VP] * 10),
    "t4d_texture_bake_scratch_bytes": (_SZ, [_I32, _I32, _I64]),
    "t4d_texture_bake": (_INT, [_VP] * 3 + [_I32] * 7 + [_VP] * 3 + [_SZ, _I64, C.POINTER(_I64), _VP]),
    "t4d_texture_render_colors": (_INT, [_VP] * 4 + [_I32] * 7 + [_VP] * 3 + [_SZ, _I64, C.POINTER(_I64), _VP]),
    "t4d_texture_coverage": (_INT, [_VP, _I32, _I32, _VP, _VP]),
    "t4d_texture_quantize": (_INT, [_VP, _I32, _I32, _I32, _VP, _VP]),
    "t4d_texture_erode": (_INT, [_VP, _I32, _I32, _I32, _VP, _VP]),
    "t4d_texture_pad_scratch_bytes": (_SZ, [_I32, _I32]),
    "t4d_texture_pad": (_INT, [_VP, _VP] + [_I32] * 4 + [_VP] * 3 + [_SZ, _VP]),
    "t4d_texture_halve": (_INT, [_VP, _VP] + [_I32] * 3 + [_VP] * 3),
    "t4d_texture_fill_scratch_bytes": (_SZ, [_I32] * 3),
    "t4d_texture_fill": (_INT, [_VP] * 3 + [_I32] * 3 + [_VP] * 3 + [_SZ, _VP]),
    "t4d_texture_fill16_scratch_bytes": (_SZ, [_I32] * 3),
    "t4d_texture_fill16": (_INT, [_VP] * 3 + [_I32] * 3 + [_VP] * 3 + [_SZ, _VP]),
    "t4d_drift_scratch_bytes": (_SZ, [_I32] * 5),
    "t4d_drift_match": (_INT, [_VP] * 5 + [_I32] * 6 + [_VP, _VP, _SZ, _VP]),
    "t4d_drift_dense": (_INT, [_VP] * 3 + [_I32] * 6 + [_VP] * 3),
    "t4d_drift_warp": (_INT, [_VP] * 4 + [_I32] * 3 + [_VP] * 3),
    "t4d_seqtex_select": (_INT, [C.POINTER(_VP), C.POINTER(_VP)] + [_I32] * 6 + [_VP] * 3),
    "t4d_seqtex_complete": (_INT, [_VP] * 4 + [_I32] * 6 + [_VP] * 3),
    "t4d_png_max_bytes": (_SZ, [_I32] * 3),
    "t4d_png_scratch_bytes": (_SZ, [_I32] * 3),
    "t4d_png_encode": (_INT, [_VP] + [_I32] * 4 + [_VP, _SZ, _VP, _VP, _SZ, _VP]),
    "t4d_png_encode_chw": (_INT, [_VP] + [_I32] * 2 + [_VP, _SZ, _VP, _VP, _SZ, _VP]),
    "t4d_png_max_bytes16": (_SZ, [_I32] * 3),
    "t4d_png_scratch_bytes16": (_SZ, [_I32] * 3),
    "t4d_png_encode16": (_INT, [_VP] + [_I32] * 3 + [_VP, _SZ, _VP, _VP, _SZ, _VP]),
    "t4d_disp_quantize": (_INT, [_VP, _VP, _I32, _I32, C.c_double, _VP, _VP, _VP]),
    "t4d_disp_smooth_scratch_bytes": (_SZ, [_I32] * 2),
    "t4d_disp_smooth": (_INT, [_VP] * 3 + [_I32] * 3 + [_VP, _VP, _SZ, _VP]),
    "t4d_disp_normals": (_INT, [_VP] * 4 + [_I32, _I32, C.c_double, _VP, _VP]),
    "t4d_tess_faces": (_INT, [_VP, _VP] + [_I32] * 4 + [_VP, _VP]),
    "t4d_tess_points": (_INT, [_VP, _I32, _I32, _VP, _I32, _VP, _I32, _I32, _VP, _VP]),
    "t4d_tess_displace": (_INT, [_VP] * 8 + [_I32] * 5 + [_VP] * 3 + [_I32, _I32, C.c_double, _VP, _VP, _VP]),
    "t4d_obj_csr_scratch_bytes": (_SZ, [_I32]),
    "t4d_obj_vertex_faces": (_INT, [_VP, _I64, _I32] + [_VP] * 4 + [_SZ, _VP]),
    "t4d_obj_normals_scratch_bytes": (_SZ, [_I64]),
    "t4d_obj_vertex_normals": (_INT, [_VP, _I32, _I32, _VP, _I64] + [_VP] * 4 + [_SZ, _VP]),
    "t4d_obj_frame_vertices": (_INT, [_VP] * 4 + [_I32, C.POINTER(C.c_double), _VP, _VP]),
    "t4d_obj_format_doubles": (_INT, [_VP, _I64, _VP, _VP, _VP]),
    "t4d_obj_text_max_bytes": (_SZ, [_I32, _I64, _I64]),
    "t4d_obj_text_scratch_bytes": (_SZ, [_I32, _I64, _I64]),
    "t4d_obj_float_lines": (_INT, [_I32, _VP, _I64, _VP, _SZ, _VP, _VP, _SZ, _VP]),
    "t4d_obj_face_lines": (_INT, [_VP] * 3 + [_I64, _I64, _VP, _SZ, _VP, _VP, _SZ, _VP]),
    "t4d_jpeg_scratch_bytes": (_SZ, [C.POINTER(T4DJpegImage), _I32, _I32]),
    "t4d_jpeg_decode": (_INT, [C.POINTER(T4DJpegImage), _VP, _I32, _VP, _I32, _VP, _SZ, _VP, _VP, _SZ, _VP]),
    "t4d_pngdec_scratch_bytes": (_SZ, [C.POINTER(T4DPngImage), _I32, _I32]),
    "t4d_png_decode": (_INT, [C.POINTER(T4DPngImage), _VP, _I32, _VP, _I32, _VP, _VP, _SZ, _VP, _VP, _VP, _SZ, _VP]),
    "t4d_warp_scratch_bytes": (_SZ, [_I32]),
    "t4d_warp_views": (_INT, [C.POINTER(T4DWarpView), _VP, _I32, _VP, _SZ, _VP]),
    "t4d_undistort_views": (_INT, [C.POINTER(T4DLensView), _VP, _I32, _VP]),
    "t4d_jpeg_enc_max_bytes": (_SZ, [_I32] * 3),
    "t4d_jpeg_enc_scratch_bytes": (_SZ, [C.POINTER(T4DJpegEncImage), _I32, _I32]),
    "t4d_jpeg_encode": (_INT, [C.POINTER(T4DJpegEncImage), _VP, _I32, _I32, _I32, _VP, _SZ, _VP, _VP, _SZ, _VP]),
    "t4d_views_to_u8": (_INT, [_VP, _I32, _I32, _I32, _VP, _VP]),
    "t4d_setup_colors_scratch_bytes": (_SZ, [_I64]),
    "t4d_setup_vertex_colors": (_INT, [_VP] + [_I32] * 3 + [_VP, _I64, _VP, _VP, _I32] + [_VP] * 4 + [_SZ, _VP]),
    "t4d_setup_quaternions": (_INT, [_VP, _I32, _VP, _VP]),
    "t4d_setup_one_ring": (_INT, [_VP, _I32, _I32] + [_VP] * 6),
    "t4d_setup_region_scratch_bytes": (_SZ, [_I32]),
    "t4d_setup_region_weights": (_INT, [_VP, _I32, _I32, _VP, _VP, C.POINTER(_I32), _I32, _VP, _VP, _VP, _SZ, _VP]),
    "t4d_setup_edges_scratch_bytes": (_SZ, [_I64]),
    "t4d_setup_flatten_edges": (_INT, [_VP, _I32, _VP, _VP, _VP, _I64] + [_VP] * 4 + [_SZ, _VP]),
    "t4d_setup_neighbor_mask": (_INT, [_VP, _I32, _I32, _VP, _VP]),
    "t4d_mesh_render_scratch_bytes": (_SZ, [_I32] * 4 + [_I64]),
    "t4d_mesh_render": (_INT, [_VP, _I32, _VP, _VP, _I32, _VP, _I32, _VP, _I32, _I32, _I32, _VP, _I32, _I32, _I32,
                               C.POINTER(_F32), _I32] + [_VP] * 4 + [_SZ, _I64, C.POINTER(_I64), _VP]),
    "t4d_image_metrics_scratch_bytes": (_SZ, [_I32] * 3),
    "t4d_image_metrics": (_INT, [_I32] * 3 + [_VP] * 6 + [_SZ, _VP]),
    "t4d_project_texture": (_INT, [_VP] * 3 + [_I32] * 2 + [_VP] + [_I32] * 3 + [_VP] * 2 + [_I32] + [C.c_double] * 3 + [_I32]
                            + [_VP] * 4),
    "t4d_project_texture_gains": (_INT, [_VP] * 3 + [_I32] * 2 + [_VP] + [_I32] * 3 + [_VP] * 3 + [_I32] + [C.c_double] * 3 + [_I32]
                                  + [_VP] * 4),
    "t4d_projtex_pair_stats": (_INT, [_VP] * 3 + [_I32] * 2 + [_VP, _I32] + [_VP] * 3 + [_I32] + [C.c_double] * 6 + [_VP] * 4),
    "t4d_projtex_low_band": (_INT, [_VP] * 2 + [_I32] * 4 + [_VP] * 2),
    "t4d_project_texture_bands": (_INT, [_VP] * 3 + [_I32] * 2 + [_VP] + [_I32] * 3 + [_VP] * 4 + [_I32] + [C.c_double] * 3 + [_VP] * 6),
    "t4d_projtex_consistency": (_INT, [_VP] * 3 + [_I32] * 2 + [_VP, _I32] + [_VP] * 3 + [_I32] + [C.c_double] * 3 + [_VP]
                                + [C.c_double] * 2 + [_I32] + [_VP] * 3),
    "t4d_project_texture_skip": (_INT, [_VP] * 3 + [_I32] * 2 + [_VP] + [_I32] * 3 + [_VP] * 3 + [_I32] + [C.c_double] * 3 + [_I32]
                                 + [_VP] * 4 + [_I32, _VP]),
    "t4d_project_texture_bands_skip": (_INT, [_VP] * 3 + [_I32] * 2 + [_VP] + [_I32] * 3 + [_VP] * 4 + [_I32] + [C.c_double] * 3
                                       + [_VP] * 6 + [_I32, _VP]),
    "t4d_project_texture_flow": (_INT, [_VP] * 3 + [_I32] * 2 + [_VP] + [_I32] * 3 + [_VP] * 3 + [_I32] + [C.c_double] * 3 + [_I32]
                                 + [_VP] * 4 + [_I32, _VP, _VP]),
    "t4d_project_texture_bands_flow": (_INT, [_VP] * 3 + [_I32] * 2 + [_VP] + [_I32] * 3 + [_VP] * 4 + [_I32] + [C.c_double] * 3
                                       + [_VP] * 6 + [_I32, _VP, _VP]),
    "t4d_closest_index_bytes": (_SZ, [_I64, _I64, _VP, C.c_double, _I64]),
    "t4d_closest_build": (_INT, [_VP, _I64, _VP, _I64, _VP, C.c_double, _VP, _SZ, _I64, C.POINTER(_I64), _VP]),
    "t4d_closest_query_scratch_bytes": (_SZ, [_I64]),
    "t4d_closest_query": (_INT, [_VP, _SZ, _VP, _I64, C.c_double, _I32, _VP, _VP, _VP, _VP, _SZ, _VP]),
    "t4d_closest_signed": (_INT, [_VP, _SZ, _VP, _I64] + [_VP] * 4 + [_VP]),
    "t4d_closest_raycast": (_INT, [_VP, _SZ, _VP, _VP, _I64, C.c_double, C.c_double, _I32, _VP, _VP, _VP, _VP, _SZ, _VP]),
    "t4d_align_transform": (_INT, [_VP, _I64, _VP, _VP, _VP]),
    "t4d_align_scratch_bytes": (_SZ, [_I64]),
    "t4d_align_accumulate": (_INT, [_VP, _SZ, _VP, _I64] + [_VP] * 4 + [C.c_double, C.c_double, _VP, _VP, _SZ, _VP]),
    "t4d_profile_begin": (_INT, []),
    "t4d_profile_end": (_INT, [C.POINTER(T4DKernelTime), _INT, C.POINTER(_INT)]),
    "t4d_debug_state_layout": (_INT, [_PROB, _INT, C.POINTER(C.c_uint64), _INT]),
    "t4d_nricp_scratch_bytes": (_SZ, [_I64]),
    "t4d_nricp_classify": (_INT, [_VP, _SZ, _VP, _I64] + [_VP] * 5 + [C.c_double] * 3 + [_VP] * 5 + [_SZ, _VP]),
    "t4d_nricp_assemble": (_INT, [_VP, _I64] + [_VP] * 5 + [C.c_double] * 3 + [_VP] * 4),
    "t4d_nricp_precond": (_INT, [_VP, _I64, _VP, _VP, _VP]),
    "t4d_nricp_apply": (_INT, [_VP, _I64, _VP, _VP, _VP, C.c_double, C.c_double] + [_VP] * 4 + [_SZ, _VP]),
    "t4d_nricp_cg_start": (_INT, [_VP, _I64, _VP, _VP, _VP, C.c_double, C.c_double] + [_VP] * 9 + [_SZ, _VP]),
    "t4d_nricp_cg_run": (_INT, [_VP, _I64, _VP, _VP, _VP, C.c_double, C.c_double] + [_VP] * 7 + [_I32] * 3 + [_VP, _SZ, _VP]),
    "t4d_nricp_positions": (_INT, [_VP, _I64] + [_VP] * 5 + [_SZ, _VP]),
}
EXPORTS = tuple(SIGNATURES)


class ExtensionMissing(RuntimeError):
    pass


_lib = None


def load():
    """Load libtopo4d_raster.so or raise ExtensionMissing.  Never falls back to anything."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ExtensionMissing(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python -m topo4d_amd.build` "
            "(hipcc --offload-arch=gfx950). topo4d_amd has no CPU fallback by design.")
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise ExtensionMissing(f"could not load {LIB_PATH}: {e}") from e
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.t4d_abi_version() != T4D_ABI_VERSION:
        raise ExtensionMissing(f"ABI mismatch: library {lib.t4d_abi_version()} vs python {T4D_ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def profile_begin() -> None:
    load().t4d_profile_begin()


def profile_end() -> dict:
    """{kernel name: (total_ms, launches)} since profile_begin()."""
    arr = (T4DKernelTime * 16)()
    n = C.c_int(0)
    call("t4d_profile_end", arr, 16, C.byref(n))
    return {arr[i].name.decode(): (arr[i].total_ms, arr[i].launches) for i in range(n.value)}


def last_error() -> str:
    return load().t4d_last_error().decode(errors="replace")


# ---- what the wrappers of the other modules share --------------------------------------------------------------------------
def ptr(t):
    """A tensor's data pointer as an argument of the library (None: NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream(device) -> int:
    """hipStream_t of torch's current stream on `device` (the private getter is ~20x cheaper than building a Stream object)."""
    try:
        return torch._C._cuda_getCurrentRawStream(device.index if device.index is not None else torch.cuda.current_device())
    except AttributeError:                                   # pragma: no cover - older/newer torch without the private hook
        return torch.cuda.current_stream(device).cuda_stream


def error(name: str, rc=None, exc=RuntimeError) -> Exception:
    """The exception for a refused call of entry point `name`: its return code (None: a size query that returned 0) and the
    library's message."""
    return exc(f"{name} failed{'' if rc is None else f' (code {rc})'}: {last_error()}")


def call(name: str, *args) -> None:
    """Call entry point `name`; a non-zero return code raises error(name, rc)."""
    rc = getattr(load(), name)(*args)
    if rc != T4D_OK:
        raise error(name, rc)


def hip_device(device, what: str, exc=RuntimeError) -> torch.device:
    """The HIP device a wrapper works on: None is the current one and a device without an index gets the current index.  A device
    of another kind, or a process that sees no HIP device, raises `exc` (the modules differ in the class their tests pin)."""
    dev = torch.device(device if device is not None else "cuda")
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise exc(f"topo4d_amd has no CPU path: {what} needs a HIP device")
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


def on_device(t: torch.Tensor, what: str, device=None, whose: str = "the same") -> torch.Tensor:
    """`t` as the library takes it, contiguous and a bool mask as uint8, once it is known to live on a HIP device (`device` None)
    or on `device`, "`whose` HIP device" in the message; RuntimeError otherwise.  Shapes and dtypes are checked before this."""
    if not t.is_cuda or (device is not None and t.device != device):
        raise RuntimeError(f"topo4d_amd has no CPU path: {what} must live on {'a' if device is None else whose} HIP device")
    return (t.to(torch.uint8) if t.dtype == torch.bool else t).contiguous()


def scratch(query: str, device, *args, exc=ValueError, reuse: torch.Tensor = None):
    """(uint8 scratch tensor on `device`, its size in bytes) for the size query `query`, called with `args`.  No size query of the
    library answers 0 for a problem its entry point takes (an empty problem is returned before the query, at the call site), so 0
    is the library's refusal and raises error(query, exc=exc) before anything is allocated.  reuse: the caller's cached tensor,
    returned as it is when it is large enough."""
    nbytes = int(getattr(load(), query)(*args))
    if nbytes == 0:
        raise error(query, exc=exc)
    if reuse is not None and reuse.numel() >= nbytes:
        return reuse, nbytes
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


# read_back's host buffer, one for the package: only the thread that launches reads back (the prefetch pools of ingest, evaluate
# and projtex submit file reads and parsers, nothing that touches the device)
_pinned = None


def read_back(out: torch.Tensor, length: torch.Tensor, cap: int, name: str, empty_ok: bool = False) -> bytes:
    """The bytes entry point `name` wrote: `out` (uint8, capacity `cap`) up to the int64 `length` it left on the device.  Reading
    the length is the one synchronisation; then exactly that many bytes are copied through the reused pinned buffer.  A length
    outside 1..cap (0..cap with empty_ok) raises RuntimeError."""
    global _pinned
    n = int(length.item())
    if n < (0 if empty_ok else 1) or n > cap:
        raise RuntimeError(f"{name}: bad output length {n} (capacity {cap})")
    if _pinned is None or _pinned.numel() < n:
        _pinned = torch.empty(max(n, 1 << 20), dtype=torch.uint8, pin_memory=True)
    _pinned[:n].copy_(out[:n])
    return _pinned[:n].numpy().tobytes()
