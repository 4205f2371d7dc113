"""Host-side Python mirror of the reference's accelerator / render interface over the rtk C-ABI.

Names follow the reference (paths relative to /root/reference/include/raytracer/):
  parse_scene_file      io/json/loader.hpp:235-265
  KdTreeSimdAccel       render/accel/kd_tree_simd.hpp:63-98 (ctor from a scene, intersect<cull>)
  KdTreeSimdAccel.occluded   render/render.hpp:110-131 (is_occluded)
  KdTreeSimdAccel.radiance   render/render.hpp:64-69, 133-308 (intersect<cull> + color_hit for caller-supplied rays)
  render_frame          render/render.hpp:18-108
  write_ppm             io/image/ppm.hpp:7-25

Everything computes in librtk_hip.so (hand-written HIP for gfx950).  There is no CPU fallback:
if the library is missing this module raises at import, and compute calls raise RtkError
(RTK_ERR_NO_DEVICE) when no GPU is usable.  torch is used only as plumbing (device buffers,
streams, torch.distributed) by the *_device entry points.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("RTK_LIB_OVERRIDE") or os.path.join(_HERE, "librtk_hip.so")     # override: A/B builds (tools/)

RTK_OK, RTK_ERR_INVALID, RTK_ERR_NO_DEVICE, RTK_ERR_HIP, RTK_ERR_IO, RTK_ERR_PARSE, RTK_ERR_UNSUPPORTED = range(7)
MAT_DIFFUSE, MAT_REFLECTIVE, MAT_REFRACTIVE, MAT_CONSTANT, MAT_TEXTURE = 0, 1, 2, 3, 4
TEX_ALBEDO, TEX_EDGES, TEX_CHECKER, TEX_BITMAP = 0, 1, 2, 3
TRACE_AUTO, TRACE_LANE, TRACE_WAVE, TRACE_GROUP4, TRACE_GROUP8, TRACE_GROUP16, TRACE_STREAM, TRACE_TWOPASS = 0, 1, 2, 3, 4, 5, 6, 7
TRAVERSAL_REFERENCE, TRAVERSAL_FAST = 0, 1     # rtk.h RTK_TRAVERSAL_*: leaf order of the wave-cooperative walks (FAST is not the parity mode)
TRACE_REPACK = 8        # batched intersect only: rays sorted by origin / direction cell before the trace (csrc/repack.hip)
OCC_CLEAR, OCC_OCCLUDED, OCC_STEP_LIMIT = 0, 1, 2     # rtk.h RTK_OCC_*: answers of the batched occlusion query
OCCLUDED_MAX_STEPS = 1024                             # rtk.h RTK_OCCLUDED_MAX_STEPS
REGIONS_IN_FRAME, REGIONS_PACKED = 0, 1               # rtk.h RTK_REGIONS_*: where render_regions puts a rectangle's pixels
ORDER_TABLE_FRAMES, ORDER_TABLE_VIEWS, ORDER_TABLE_REGIONS = 0, 1, 2   # rtk.h RTK_ORDER_TABLE_*: whose launch order rtk_debug_order_judge reports
MAX_REGIONS = 65536                                   # rectangles of one render_regions call at most

# every symbol include/rtk.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "rtk_abi_version", "rtk_last_error", "rtk_device_count",
    "rtk_scene_create", "rtk_scene_load_crtscene", "rtk_scene_get_info", "rtk_scene_get_arrays", "rtk_scene_get_textures",
    "rtk_scene_get_bitmaps", "rtk_decode_jpeg",
    "rtk_scene_vertex_normals", "rtk_scene_destroy",
    "rtk_accel_build", "rtk_accel_tree_info", "rtk_accel_tree_dump", "rtk_accel_destroy",
    "rtk_accel_intersect", "rtk_accel_intersect_device", "rtk_accel_intersect_stats",
    "rtk_accel_occluded", "rtk_accel_occluded_device",
    "rtk_accel_radiance", "rtk_accel_radiance_device",
    "rtk_accel_update_vertices", "rtk_accel_update_vertices_device",
    "rtk_accel_update_geometry", "rtk_accel_update_geometry_device",
    "rtk_render_output_floats", "rtk_render_frame", "rtk_render_frame_device", "rtk_render_last_counters",
    "rtk_render_last_critical_path", "rtk_debug_counter_fills", "rtk_debug_order_judge", "rtk_debug_order_lists",
    "rtk_tiles_assemble_device", "rtk_camera_rays", "rtk_camera_rays_device",
    "rtk_accel_get_camera", "rtk_accel_set_camera", "rtk_render_views", "rtk_render_views_device",
    "rtk_render_regions", "rtk_render_regions_device",
    "rtk_render_gbuffer", "rtk_render_gbuffer_device",
    "rtk_render_gbuffer_specular", "rtk_render_gbuffer_specular_device",
    "rtk_render_adaptive", "rtk_render_adaptive_device",
    "rtk_render_frame_noise", "rtk_render_frame_noise_device", "rtk_debug_noise_fallbacks",
    "rtk_denoise_workspace_bytes", "rtk_denoise_frame", "rtk_denoise_frame_device",
    "rtk_temporal_accumulate", "rtk_temporal_accumulate_device",
    "rtk_temporal_accumulate_clamped", "rtk_temporal_accumulate_clamped_device",
    "rtk_render_motion", "rtk_render_motion_device",
    "rtk_accel_get_lights", "rtk_accel_set_lights", "rtk_accel_set_lights_device",
    "rtk_accel_get_materials", "rtk_accel_set_materials", "rtk_accel_get_background", "rtk_accel_set_background",
    "rtk_accel_get_textures", "rtk_accel_get_texture_pixels", "rtk_accel_set_textures", "rtk_accel_set_texture_pixels",
    "rtk_accel_set_texture_pixels_device", "rtk_accel_set_texture_frame_device",
    "rtk_accel_get_uvs", "rtk_accel_set_uvs", "rtk_accel_set_uvs_device",
    "rtk_frame_to_rgb8_device", "rtk_format_ppm_rgb8", "rtk_write_ppm", "rtk_format_ppm",
]


class RtkError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"rtk error {code}: {msg}")
        self.code = code


if not os.path.exists(_LIB_PATH):
    raise ImportError(
        f"{_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "(hipcc --offload-arch=gfx950).  This package has no CPU fallback."
    )

# One HIP runtime per process: PyTorch bundles its own libamdhip64/libhsa-runtime64 (same sonames as the system
# ROCm ones but different files).  If librtk_hip.so pulled in the system copies and torch its bundled ones, the
# second runtime to initialise finds no device.  Importing torch first makes the loader satisfy librtk_hip.so's
# libamdhip64.so.7 / libhsa-runtime64.so.1 from the copies torch already mapped.  Pure C/C++ hosts use system ROCm.
try:
    import torch  # noqa: F401  (plumbing only: device buffers, streams, torch.distributed)
except ImportError:  # pragma: no cover - torch is part of the image
    torch = None

_L = C.CDLL(_LIB_PATH)


class SceneDesc(C.Structure):
    _fields_ = [
        ("n_meshes", C.c_int32), ("mesh_material", C.POINTER(C.c_int32)), ("mesh_nverts", C.POINTER(C.c_int32)),
        ("mesh_ntris", C.POINTER(C.c_int32)), ("vertices", C.POINTER(C.c_float)), ("indices", C.POINTER(C.c_uint32)),
        ("n_materials", C.c_int32), ("mat_kind", C.POINTER(C.c_int32)), ("mat_albedo", C.POINTER(C.c_float)),
        ("mat_ior", C.POINTER(C.c_float)), ("mat_smooth", C.POINTER(C.c_int32)),
        ("mat_texture", C.POINTER(C.c_int32)), ("uvs", C.POINTER(C.c_float)), ("mesh_has_uvs", C.POINTER(C.c_int32)),
        ("n_textures", C.c_int32), ("tex_kind", C.POINTER(C.c_int32)), ("tex_color_a", C.POINTER(C.c_float)),
        ("tex_color_b", C.POINTER(C.c_float)), ("tex_param", C.POINTER(C.c_float)),
        ("n_lights", C.c_int32), ("light_pos", C.POINTER(C.c_float)), ("light_intensity", C.POINTER(C.c_float)),
        ("cam_pos", C.c_float * 3), ("cam_mat", C.c_float * 9), ("background", C.c_float * 3),
        ("width", C.c_int32), ("height", C.c_int32), ("bucket_size", C.c_int32),
        ("tex_pixels", C.POINTER(C.c_uint8)), ("tex_bitmap", C.POINTER(C.c_int32)),
    ]


class SceneInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("n_meshes", "n_materials", "n_lights", "n_vertices", "n_triangles", "width", "height", "bucket_size",
                 "n_textures", "n_uv_vertices", "n_bitmap_bytes")]


class AccelParams(C.Structure):
    _fields_ = [("max_depth", C.c_int32), ("max_leaf_size", C.c_int32), ("eps", C.c_float),
                ("normalize_hit_normal", C.c_int32), ("device", C.c_int32), ("traversal", C.c_int32)]


class TreeInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("n_nodes", "n_inner", "n_leaves", "n_leaf_refs", "max_leaf_refs", "n_triangles", "tree_depth", "reserved")]


class RenderParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("spp", C.c_int32), ("max_ray_depth", C.c_int32),
                ("diffuse_rays", C.c_int32), ("seed", C.c_uint32), ("fov_degrees", C.c_double),
                ("shadow_bias", C.c_float), ("reflection_bias", C.c_float), ("refraction_bias", C.c_float),
                ("trace_mode", C.c_int32), ("rank", C.c_int32), ("world_size", C.c_int32), ("collect_stats", C.c_int32),
                ("sample_begin", C.c_int32), ("sample_count", C.c_int32)]


class RadianceParams(C.Structure):
    _fields_ = [("max_ray_depth", C.c_int32), ("diffuse_rays", C.c_int32), ("seed", C.c_uint32), ("sample", C.c_int32),
                ("shadow_bias", C.c_float), ("reflection_bias", C.c_float), ("refraction_bias", C.c_float),
                ("cull", C.c_int32), ("trace_mode", C.c_int32)]


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("rays", "primary", "hits", "nodes", "boxpass", "leaves", "tris", "packets16")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class OrderJudgeStats(C.Structure):
    """rtk.h rtk_order_judge_stats; 48 bytes."""
    _fields_ = [("sorts", C.c_uint64), ("judges", C.c_uint64), ("taken", C.c_uint64), ("rejected", C.c_uint64),
                ("champion_ticks", C.c_uint32), ("challenger_ticks", C.c_uint32), ("units", C.c_uint32), ("read_set", C.c_int32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class GBuffer(C.Structure):
    """rtk.h rtk_gbuffer: one pointer per plane, NULL = plane not wanted; 64 bytes."""
    _fields_ = [(n, C.c_void_p) for n in ("depth", "position", "normal", "albedo", "bary", "tri", "mesh", "material")]


class SpecularGBuffer(C.Structure):
    """rtk.h rtk_gbuffer_specular: one pointer per plane, NULL = plane not wanted; 96 bytes."""
    _fields_ = [(n, C.c_void_p) for n in ("depth", "position", "normal", "surface_position", "surface_normal", "albedo", "bary",
                                          "tri", "mesh", "material", "bounces", "last_ray")]


class AdaptiveParams(C.Structure):
    """rtk.h rtk_adaptive_params; 16 bytes."""
    _fields_ = [("min_samples", C.c_int32), ("step", C.c_int32), ("threshold", C.c_float), ("floor", C.c_float)]


class DenoiseParams(C.Structure):
    """rtk.h rtk_denoise_params; 32 bytes."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("iterations", C.c_int32), ("normal_power_log2", C.c_int32),
                ("sigma_luminance", C.c_float), ("sigma_plane", C.c_float), ("albedo_floor", C.c_float), ("reserved", C.c_int32)]


class DenoiseInputs(C.Structure):
    """rtk.h rtk_denoise_inputs: one pointer per plane, noise and albedo may be NULL; 48 bytes."""
    _fields_ = [(n, C.c_void_p) for n in ("rgb", "noise", "albedo", "normal", "position", "depth")]


class TemporalParams(C.Structure):
    """rtk.h rtk_temporal_params; 32 bytes."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fov_degrees", C.c_double), ("alpha_min", C.c_float),
                ("plane_tolerance", C.c_float), ("normal_min_dot", C.c_float), ("max_history", C.c_int32)]


class TemporalFrame(C.Structure):
    """rtk.h rtk_temporal_frame: the new frame, one pointer per plane; noise and mesh may be NULL; 48 bytes."""
    _fields_ = [(n, C.c_void_p) for n in ("rgb", "noise", "position", "normal", "depth", "mesh")]


class TemporalHistory(C.Structure):
    """rtk.h rtk_temporal_history: the accumulated frame, the guides and the view (HOST, an rtk_view) of the previous camera; 64 bytes."""
    _fields_ = [(n, C.c_void_p) for n in ("rgb", "noise", "length", "position", "normal", "depth", "mesh", "view")]


class TemporalOutputs(C.Structure):
    """rtk.h rtk_temporal_outputs; 24 bytes."""
    _fields_ = [(n, C.c_void_p) for n in ("rgb", "noise", "length")]


class TemporalClamp(C.Structure):
    """rtk.h rtk_temporal_clamp; 16 bytes."""
    _fields_ = [("radius", C.c_int32), ("gamma", C.c_float), ("history_keep", C.c_float), ("reserved", C.c_int32)]


class MotionParams(C.Structure):
    """rtk.h rtk_motion_params; 16 bytes."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fov_degrees", C.c_double)]


class MotionOutputs(C.Structure):
    """rtk.h rtk_motion_outputs: either plane may be NULL, not both; 16 bytes."""
    _fields_ = [(n, C.c_void_p) for n in ("prev_position", "motion")]


MOTION_MISS_BITS = 0x7FC00000                         # rtk.h: both words of a pixel's motion when there is none to report

# the planes of a g-buffer in the struct's order: name -> (trailing shape, dtype); miss values in rtk.h
GBUFFER_PLANES = {"depth": ((), np.float32), "position": ((3,), np.float32), "normal": ((3,), np.float32),
                  "albedo": ((3,), np.float32), "bary": ((2,), np.float32), "tri": ((), np.uint32), "mesh": ((), np.uint32),
                  "material": ((), np.uint32)}

SPECULAR_GBUFFER_PLANES = {"depth": ((), np.float32), "position": ((3,), np.float32), "normal": ((3,), np.float32),
                           "surface_position": ((3,), np.float32), "surface_normal": ((3,), np.float32),
                           "albedo": ((3,), np.float32), "bary": ((2,), np.float32), "tri": ((), np.uint32), "mesh": ((), np.uint32),
                           "material": ((), np.uint32), "bounces": ((), np.uint32), "last_ray": ((6,), np.float32)}

RAY_DTYPE = np.dtype([("origin", "<f4", (3,)), ("direction", "<f4", (3,))])
LIGHT_DTYPE = np.dtype([("position", "<f4", (3,)), ("intensity", "<f4")])                     # rtk.h rtk_light
MATERIAL_DTYPE = np.dtype([("kind", "<i4"), ("smooth", "<i4"), ("albedo", "<f4", (3,)), ("ior", "<f4"), ("texture", "<i4"),
                           ("reserved", "<i4")])                                             # rtk.h rtk_material
TEXTURE_DTYPE = np.dtype([("kind", "<i4"), ("color_a", "<f4", (3,)), ("color_b", "<f4", (3,)), ("param", "<f4"), ("width", "<i4"),
                          ("height", "<i4")])                                                # rtk.h rtk_texture
assert LIGHT_DTYPE.itemsize == 16 and MATERIAL_DTYPE.itemsize == 32 and TEXTURE_DTYPE.itemsize == 40
HIT_DTYPE = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("tri", "<u4"), ("mesh", "<u4"), ("normal", "<f4", (3,))])
assert RAY_DTYPE.itemsize == 24 and HIT_DTYPE.itemsize == 32

_vp = C.c_void_p
_L.rtk_abi_version.restype = C.c_int
_L.rtk_last_error.restype = C.c_char_p
_L.rtk_device_count.argtypes = [C.POINTER(C.c_int)]
_L.rtk_scene_create.argtypes = [C.POINTER(SceneDesc), C.POINTER(_vp)]
_L.rtk_scene_load_crtscene.argtypes = [C.c_char_p, C.POINTER(_vp)]
_L.rtk_scene_get_info.argtypes = [_vp, C.POINTER(SceneInfo)]
_L.rtk_scene_get_arrays.argtypes = [_vp] * 15
_L.rtk_scene_get_textures.argtypes = [_vp] * 8
_L.rtk_scene_get_bitmaps.argtypes = [_vp] * 3
_L.rtk_decode_jpeg.argtypes = [_vp, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _vp, C.c_size_t]
_L.rtk_scene_vertex_normals.argtypes = [_vp, C.c_int32, _vp]
_L.rtk_scene_destroy.argtypes = [_vp]
_L.rtk_scene_destroy.restype = None
_L.rtk_accel_build.argtypes = [_vp, C.POINTER(AccelParams), C.POINTER(_vp)]
_L.rtk_accel_tree_info.argtypes = [_vp, C.POINTER(TreeInfo)]
_L.rtk_accel_tree_dump.argtypes = [_vp, _vp, _vp, _vp]
_L.rtk_accel_destroy.argtypes = [_vp]
_L.rtk_accel_destroy.restype = None
_L.rtk_accel_intersect.argtypes = [_vp, _vp, C.c_size_t, C.c_int, C.c_int, _vp]
_L.rtk_accel_intersect_device.argtypes = [_vp, _vp, C.c_size_t, C.c_int, C.c_int, _vp, _vp]
_L.rtk_accel_intersect_stats.argtypes = [_vp, _vp, C.c_size_t, C.c_int, C.c_int, _vp, C.POINTER(Counters)]
_L.rtk_accel_occluded.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_float, C.c_int, _vp, C.POINTER(C.c_uint64)]
_L.rtk_accel_occluded_device.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_float, C.c_int, _vp, _vp]
_L.rtk_accel_radiance.argtypes = [_vp, _vp, _vp, C.c_size_t, C.POINTER(RadianceParams), _vp, C.POINTER(Counters)]
_L.rtk_accel_radiance_device.argtypes = [_vp, _vp, _vp, C.c_size_t, C.POINTER(RadianceParams), _vp, _vp]
_L.rtk_accel_update_vertices.argtypes = [_vp, _vp]
_L.rtk_accel_update_vertices_device.argtypes = [_vp, _vp, _vp]
_L.rtk_accel_update_geometry.argtypes = [_vp, _vp, _vp, _vp]
_L.rtk_accel_update_geometry_device.argtypes = [_vp, _vp, _vp, _vp, _vp]
_L.rtk_render_output_floats.argtypes = [_vp, C.POINTER(RenderParams), C.POINTER(C.c_size_t)]
_L.rtk_render_frame.argtypes = [_vp, C.POINTER(RenderParams), _vp, C.POINTER(Counters)]
_L.rtk_render_frame_device.argtypes = [_vp, C.POINTER(RenderParams), _vp, _vp]
_L.rtk_render_last_counters.argtypes = [_vp, C.POINTER(Counters)]
_L.rtk_render_last_critical_path.argtypes = [_vp, C.POINTER(C.c_double)]
if hasattr(_L, "rtk_debug_counter_fills"):            # (an older build loaded through RTK_LIB_OVERRIDE for an A/B run has no such diagnostic)
    _L.rtk_debug_counter_fills.argtypes = [_vp, C.POINTER(C.c_uint64)]
if hasattr(_L, "rtk_debug_order_judge"):              # (likewise)
    _L.rtk_debug_order_judge.argtypes = [_vp, C.c_int32, C.c_int32, C.POINTER(OrderJudgeStats)]
    _L.rtk_debug_order_lists.argtypes = [_vp, C.c_int32, _vp, C.c_size_t, C.POINTER(C.c_size_t)]
_L.rtk_tiles_assemble_device.argtypes = [_vp, C.POINTER(RenderParams), _vp, _vp, _vp]
_L.rtk_camera_rays.argtypes = [_vp, C.POINTER(RenderParams), C.c_int32, _vp]
_L.rtk_camera_rays_device.argtypes = [_vp, C.POINTER(RenderParams), C.c_int32, _vp, _vp]
_L.rtk_accel_get_camera.argtypes = [_vp, _vp]
_L.rtk_accel_set_camera.argtypes = [_vp, _vp]
_L.rtk_render_views.argtypes = [_vp, C.POINTER(RenderParams), _vp, C.c_int32, _vp, C.POINTER(Counters)]
_L.rtk_render_views_device.argtypes = [_vp, C.POINTER(RenderParams), _vp, C.c_int32, _vp, _vp]
_L.rtk_render_regions.argtypes = [_vp, C.POINTER(RenderParams), _vp, C.c_int32, C.c_int, _vp, C.POINTER(Counters)]
_L.rtk_render_regions_device.argtypes = [_vp, C.POINTER(RenderParams), _vp, C.c_int32, C.c_int, _vp, _vp]
_L.rtk_render_gbuffer.argtypes = [_vp, C.POINTER(RenderParams), C.c_int32, _vp, C.c_int32, C.POINTER(GBuffer)]
_L.rtk_render_gbuffer_device.argtypes = [_vp, C.POINTER(RenderParams), C.c_int32, _vp, C.c_int32, C.POINTER(GBuffer), _vp]
if hasattr(_L, "rtk_render_gbuffer_specular"):        # (an older build loaded through RTK_LIB_OVERRIDE for an A/B run has no such call)
    _L.rtk_render_gbuffer_specular.argtypes = [_vp, C.POINTER(RenderParams), C.c_int32, _vp, C.c_int32, C.POINTER(SpecularGBuffer)]
    _L.rtk_render_gbuffer_specular_device.argtypes = [_vp, C.POINTER(RenderParams), C.c_int32, _vp, C.c_int32, C.POINTER(SpecularGBuffer), _vp]
_L.rtk_render_adaptive.argtypes = [_vp, C.POINTER(RenderParams), C.POINTER(AdaptiveParams), _vp, _vp, _vp, C.POINTER(Counters)]
_L.rtk_render_adaptive_device.argtypes = [_vp, C.POINTER(RenderParams), C.POINTER(AdaptiveParams), _vp, _vp, _vp, _vp]
if hasattr(_L, "rtk_render_frame_noise"):             # (as above: an older build under RTK_LIB_OVERRIDE has no such call)
    _L.rtk_render_frame_noise.argtypes = [_vp, C.POINTER(RenderParams), _vp, _vp, C.POINTER(Counters)]
    _L.rtk_render_frame_noise_device.argtypes = [_vp, C.POINTER(RenderParams), _vp, _vp, _vp]
    _L.rtk_debug_noise_fallbacks.argtypes = [_vp, C.POINTER(C.c_uint64)]
_L.rtk_denoise_workspace_bytes.argtypes =[C.POINTER(DenoiseParams), C.c_int32, C.POINTER(C.c_size_t)]
_L.rtk_denoise_frame.argtypes = [C.POINTER(DenoiseParams), C.c_int32, C.POINTER(DenoiseInputs), _vp]
_L.rtk_denoise_frame_device.argtypes = [C.POINTER(DenoiseParams), C.c_int32, C.POINTER(DenoiseInputs), _vp, _vp, C.c_size_t, _vp]
if hasattr(_L, "rtk_temporal_accumulate"):            # (as above: an older build under RTK_LIB_OVERRIDE has no such call)
    _L.rtk_temporal_accumulate.argtypes = [C.POINTER(TemporalParams), C.POINTER(TemporalFrame), C.POINTER(TemporalHistory),
                                           C.POINTER(TemporalOutputs)]
    _L.rtk_temporal_accumulate_device.argtypes = [C.POINTER(TemporalParams), C.POINTER(TemporalFrame), C.POINTER(TemporalHistory),
                                                  C.POINTER(TemporalOutputs), _vp]
if hasattr(_L, "rtk_temporal_accumulate_clamped"):    # (likewise)
    _L.rtk_temporal_accumulate_clamped.argtypes = [C.POINTER(TemporalParams), C.POINTER(TemporalClamp), C.POINTER(TemporalFrame),
                                                   C.POINTER(TemporalHistory), C.POINTER(TemporalOutputs)]
    _L.rtk_temporal_accumulate_clamped_device.argtypes = [C.POINTER(TemporalParams), C.POINTER(TemporalClamp), C.POINTER(TemporalFrame),
                                                          C.POINTER(TemporalHistory), C.POINTER(TemporalOutputs), _vp]
if hasattr(_L, "rtk_render_motion"):                  # (as above: an older build under RTK_LIB_OVERRIDE has no such call)
    _L.rtk_render_motion.argtypes = [_vp, C.POINTER(MotionParams), _vp, _vp, _vp, _vp, C.POINTER(MotionOutputs)]
    _L.rtk_render_motion_device.argtypes = [_vp, C.POINTER(MotionParams), _vp, _vp, _vp, _vp, C.POINTER(MotionOutputs), _vp]
_L.rtk_accel_get_lights.argtypes =[_vp, _vp, C.c_int32, C.POINTER(C.c_int32)]
_L.rtk_accel_set_lights.argtypes = [_vp, _vp, C.c_int32]
_L.rtk_accel_set_lights_device.argtypes = [_vp, _vp, C.c_int32, _vp]
_L.rtk_accel_get_materials.argtypes = [_vp, _vp]
_L.rtk_accel_set_materials.argtypes = [_vp, _vp, C.c_int32]
_L.rtk_accel_get_background.argtypes = [_vp, _vp]
_L.rtk_accel_set_background.argtypes = [_vp, _vp]
_L.rtk_accel_get_textures.argtypes = [_vp, _vp, C.c_int32, C.POINTER(C.c_int32)]
_L.rtk_accel_get_texture_pixels.argtypes = [_vp, C.c_int32, _vp, C.c_size_t, C.POINTER(C.c_size_t)]
_L.rtk_accel_set_textures.argtypes = [_vp, _vp, C.c_int32, _vp]
_L.rtk_accel_set_texture_pixels.argtypes = [_vp, C.c_int32, C.c_int32, C.c_int32, _vp]
_L.rtk_accel_set_texture_pixels_device.argtypes = [_vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp]
_L.rtk_accel_set_texture_frame_device.argtypes = [_vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp]
_L.rtk_accel_get_uvs.argtypes = [_vp, _vp]
_L.rtk_accel_set_uvs.argtypes = [_vp, _vp]
_L.rtk_accel_set_uvs_device.argtypes = [_vp, _vp, _vp]
_L.rtk_frame_to_rgb8_device.argtypes = [_vp, C.c_size_t, _vp, _vp]
_L.rtk_format_ppm_rgb8.argtypes = [_vp, C.c_int32, C.c_int32, _vp, C.c_size_t, C.POINTER(C.c_size_t)]
_L.rtk_write_ppm.argtypes = [_vp, C.c_int32, C.c_int32, C.c_char_p]
_L.rtk_format_ppm.argtypes = [_vp, C.c_int32, C.c_int32, _vp, C.c_size_t, C.POINTER(C.c_size_t)]


def _check(rc: int) -> None:
    if rc != RTK_OK:
        raise RtkError(rc, (_L.rtk_last_error() or b"").decode("utf-8", "replace"))


def lib() -> C.CDLL:
    return _L


def lib_path() -> str:
    return _LIB_PATH


def abi_version() -> int:
    return _L.rtk_abi_version()


def device_count() -> int:
    n = C.c_int(0)
    _check(_L.rtk_device_count(C.byref(n)))
    return n.value


def _fp(a, ty):
    return a.ctypes.data_as(C.POINTER(ty))


class Scene:
    """scene<float> (scene/scene.hpp:14-22) held by the library."""

    def __init__(self, handle):
        self._h = handle
        info = SceneInfo()
        _check(_L.rtk_scene_get_info(self._h, C.byref(info)))
        self.info = info

    @classmethod
    def from_arrays(cls, mesh_material, mesh_nverts, mesh_ntris, vertices, indices, mat_kind, mat_albedo, mat_ior,
                    mat_smooth, light_pos, light_intensity, cam_pos, cam_mat, background, width, height, bucket_size=64,
                    mat_texture=None, uvs=None, mesh_has_uvs=None, tex_kind=None, tex_color_a=None, tex_color_b=None,
                    tex_param=None, tex_pixels=None, tex_bitmap=None):
        n_tex = 0 if tex_kind is None else len(tex_kind)
        keep = dict(
            mt=np.ascontiguousarray(mat_texture if mat_texture is not None else np.full(len(mat_kind), -1), np.int32),
            uv=np.ascontiguousarray(uvs if uvs is not None else np.zeros((0, 2)), np.float32),
            hu=np.ascontiguousarray(mesh_has_uvs if mesh_has_uvs is not None else np.zeros(len(mesh_material)), np.int32),
            tk=np.ascontiguousarray(tex_kind if tex_kind is not None else np.zeros(0), np.int32),
            ta=np.ascontiguousarray(tex_color_a if tex_color_a is not None else np.zeros((n_tex, 3)), np.float32),
            tb=np.ascontiguousarray(tex_color_b if tex_color_b is not None else np.zeros((n_tex, 3)), np.float32),
            tp=np.ascontiguousarray(tex_param if tex_param is not None else np.zeros(n_tex), np.float32),
            px=np.ascontiguousarray(tex_pixels if tex_pixels is not None else np.zeros(0), np.uint8),
            bm=np.ascontiguousarray(tex_bitmap if tex_bitmap is not None else np.zeros((n_tex, 3)), np.int32),
            mm=np.ascontiguousarray(mesh_material, np.int32), nv=np.ascontiguousarray(mesh_nverts, np.int32),
            nt=np.ascontiguousarray(mesh_ntris, np.int32), v=np.ascontiguousarray(vertices, np.float32),
            ix=np.ascontiguousarray(indices, np.uint32), mk=np.ascontiguousarray(mat_kind, np.int32),
            ma=np.ascontiguousarray(mat_albedo, np.float32), mi=np.ascontiguousarray(mat_ior, np.float32),
            ms=np.ascontiguousarray(mat_smooth, np.int32), lp=np.ascontiguousarray(light_pos, np.float32),
            li=np.ascontiguousarray(light_intensity, np.float32),
        )
        d = SceneDesc()
        d.n_meshes = len(keep["mm"])
        d.mesh_material, d.mesh_nverts, d.mesh_ntris = _fp(keep["mm"], C.c_int32), _fp(keep["nv"], C.c_int32), _fp(keep["nt"], C.c_int32)
        d.vertices, d.indices = _fp(keep["v"], C.c_float), _fp(keep["ix"], C.c_uint32)
        d.n_materials = len(keep["mk"])
        d.mat_kind, d.mat_albedo = _fp(keep["mk"], C.c_int32), _fp(keep["ma"], C.c_float)
        d.mat_ior, d.mat_smooth = _fp(keep["mi"], C.c_float), _fp(keep["ms"], C.c_int32)
        d.mat_texture, d.uvs, d.mesh_has_uvs = _fp(keep["mt"], C.c_int32), _fp(keep["uv"], C.c_float), _fp(keep["hu"], C.c_int32)
        d.n_textures = n_tex
        d.tex_kind, d.tex_color_a = _fp(keep["tk"], C.c_int32), _fp(keep["ta"], C.c_float)
        d.tex_color_b, d.tex_param = _fp(keep["tb"], C.c_float), _fp(keep["tp"], C.c_float)
        d.tex_pixels, d.tex_bitmap = _fp(keep["px"], C.c_uint8), _fp(keep["bm"], C.c_int32)
        d.n_lights = len(keep["li"])
        d.light_pos, d.light_intensity = _fp(keep["lp"], C.c_float), _fp(keep["li"], C.c_float)
        d.cam_pos[:] = [float(x) for x in np.asarray(cam_pos, np.float32)]
        d.cam_mat[:] = [float(x) for x in np.asarray(cam_mat, np.float32)]
        d.background[:] = [float(x) for x in np.asarray(background, np.float32)]
        d.width, d.height, d.bucket_size = int(width), int(height), int(bucket_size)
        h = _vp()
        _check(_L.rtk_scene_create(C.byref(d), C.byref(h)))
        return cls(h)

    def arrays(self) -> dict:
        i = self.info
        out = dict(
            mesh_material=np.zeros(i.n_meshes, np.int32), mesh_nverts=np.zeros(i.n_meshes, np.int32),
            mesh_ntris=np.zeros(i.n_meshes, np.int32), vertices=np.zeros((i.n_vertices, 3), np.float32),
            indices=np.zeros((i.n_triangles, 3), np.uint32), mat_kind=np.zeros(i.n_materials, np.int32),
            mat_albedo=np.zeros((i.n_materials, 3), np.float32), mat_ior=np.zeros(i.n_materials, np.float32),
            mat_smooth=np.zeros(i.n_materials, np.int32), light_pos=np.zeros((i.n_lights, 3), np.float32),
            light_intensity=np.zeros(i.n_lights, np.float32), cam_pos=np.zeros(3, np.float32),
            cam_mat=np.zeros(9, np.float32), background=np.zeros(3, np.float32),
        )
        _check(_L.rtk_scene_get_arrays(self._h, *[a.ctypes.data for a in out.values()]))
        tex = dict(
            mat_texture=np.zeros(i.n_materials, np.int32), mesh_has_uvs=np.zeros(i.n_meshes, np.int32),
            uvs=np.zeros((i.n_uv_vertices, 2), np.float32), tex_kind=np.zeros(i.n_textures, np.int32),
            tex_color_a=np.zeros((i.n_textures, 3), np.float32), tex_color_b=np.zeros((i.n_textures, 3), np.float32),
            tex_param=np.zeros(i.n_textures, np.float32),
        )
        _check(_L.rtk_scene_get_textures(self._h, *[a.ctypes.data for a in tex.values()]))
        out.update(tex)
        bmp = dict(tex_bitmap=np.zeros((i.n_textures, 3), np.int32), tex_pixels=np.zeros(i.n_bitmap_bytes, np.uint8))
        _check(_L.rtk_scene_get_bitmaps(self._h, bmp["tex_bitmap"].ctypes.data, bmp["tex_pixels"].ctypes.data))
        out.update(bmp)
        out.update(width=i.width, height=i.height, bucket_size=i.bucket_size)
        return out

    def vertex_normals(self, mesh: int) -> np.ndarray:
        nv = int(self.arrays()["mesh_nverts"][mesh])
        out = np.zeros((nv, 3), np.float32)
        _check(_L.rtk_scene_vertex_normals(self._h, mesh, out.ctypes.data))
        return out

    def __del__(self, _destroy=_L.rtk_scene_destroy):     # bound at definition: module globals may be gone at interpreter exit
        if getattr(self, "_h", None):
            _destroy(self._h)
            self._h = None


def decode_jpeg(data: bytes) -> np.ndarray:
    """uint8 [h][w][channels] as `stbi_load(path, &w, &h, &channels, 0)` (scene/texture/bitmap.hpp:15) returns a baseline JPEG."""
    buf = np.frombuffer(data, np.uint8)
    w, h, ch = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _check(_L.rtk_decode_jpeg(buf.ctypes.data, buf.size, C.byref(w), C.byref(h), C.byref(ch), None, 0))
    out = np.zeros((h.value, w.value, ch.value), np.uint8)
    _check(_L.rtk_decode_jpeg(buf.ctypes.data, buf.size, C.byref(w), C.byref(h), C.byref(ch), out.ctypes.data, out.size))
    return out


def parse_scene_file(path: str) -> Scene:
    """io/json/loader.hpp:235-265 (own JSON reader in csrc/crtscene.cpp)."""
    h = _vp()
    _check(_L.rtk_scene_load_crtscene(os.fsencode(path), C.byref(h)))
    return Scene(h)


@dataclass
class RenderConfig:
    """config.hpp:6-17 as runtime values (+ resolution override and multi-GPU sharding)."""
    width: int = 0
    height: int = 0
    spp: int = 1
    max_ray_depth: int = 5
    diffuse_rays: int = 0
    seed: int = 42
    fov_degrees: float = 90.0
    shadow_bias: float = 1e-4
    reflection_bias: float = 1e-4
    refraction_bias: float = 1e-4
    trace_mode: int = TRACE_AUTO
    rank: int = 0
    world_size: int = 1
    collect_stats: int = 0     # 1 (or True): per-ray work counters of the reference algorithm; 2: of the production path (early-exit occlusion queries; unlit ones untraced, RTK_SKIP_UNLIT_SHADOW)
    sample_begin: int = 0      # progressive accumulation: this call renders samples [sample_begin, sample_begin + sample_count)
    sample_count: int = 0      # 0 = all spp samples in one call

    def to_c(self) -> RenderParams:
        return RenderParams(self.width, self.height, self.spp, self.max_ray_depth, self.diffuse_rays, self.seed,
                            self.fov_degrees, np.float32(self.shadow_bias), np.float32(self.reflection_bias),
                            np.float32(self.refraction_bias), self.trace_mode, self.rank, self.world_size,
                            int(self.collect_stats), self.sample_begin, self.sample_count)


@dataclass
class AdaptiveConfig:
    """rtk.h rtk_adaptive_params: when the 8x8 pixel blocks of render_adaptive stop taking samples (cfg.spp is the ceiling)."""
    min_samples: int = 16      # >= 2: every pixel gets at least this many
    step: int = 16             # >= 1: samples per round after the first
    threshold: float = 0.02    # a block stops once its noise estimate E_B <= threshold
    floor: float = 0.01        # lower bound of the block's mean luminance in E_B's denominator

    def to_c(self) -> AdaptiveParams:
        return AdaptiveParams(self.min_samples, self.step, np.float32(self.threshold), np.float32(self.floor))


@dataclass
class DenoiseConfig:
    """rtk.h rtk_denoise_params without the image size: the edge-avoiding a-trous filter of denoise()."""
    iterations: int = 5            # 1..8: steps 1, 2, 4, ...
    normal_power_log2: int = 2     # 0..8: the normal weight is max(n_p . n_q, 0) ** (2 ** this)
    sigma_luminance: float = 1.5   # in standard deviations of the pixel's own luminance (the noise plane)
    sigma_plane: float = 0.05      # distance from the centre pixel's tangent plane, in scene units
    albedo_floor: float = 0.01     # lower bound of the albedo that the colour is divided by

    def to_c(self, width: int, height: int) -> DenoiseParams:
        return DenoiseParams(width, height, self.iterations, self.normal_power_log2, np.float32(self.sigma_luminance),
                             np.float32(self.sigma_plane), np.float32(self.albedo_floor), 0)


@dataclass
class TemporalConfig:
    """rtk.h rtk_temporal_params without the image size: how temporal_accumulate() accepts and weighs a frame's history."""
    fov_degrees: float = 90.0      # of both frames, as RenderConfig.fov_degrees
    alpha_min: float = 0.05        # in (0, 1]: lower bound of the new frame's weight
    plane_tolerance: float = 0.01  # a tap must lie within this x depth of the pixel's tangent plane
    normal_min_dot: float = 0.9    # in [-1, 1]: the least n_p . n_q of an accepted tap
    max_history: int = 32          # 1..1048576: cap of the history length

    def to_c(self, width: int, height: int) -> TemporalParams:
        return TemporalParams(width, height, float(self.fov_degrees), np.float32(self.alpha_min), np.float32(self.plane_tolerance),
                              np.float32(self.normal_min_dot), self.max_history)


@dataclass
class ClampConfig:
    """rtk.h rtk_temporal_clamp: how temporal_accumulate(..., clamp=) bounds the history by the new frame's neighbourhood."""
    radius: int = 1                # 1..3: the box is (2 * radius + 1)^2 pixels of the new frame
    gamma: float = 1.0             # >= 0: the history is clamped to mean +- gamma * standard deviation of the box, per channel
    history_keep: float = 1.0      # in [0, 1]: the share of its history length a clamped pixel keeps

    def to_c(self) -> TemporalClamp:
        return TemporalClamp(self.radius, np.float32(self.gamma), np.float32(self.history_keep), 0)


@dataclass
class MotionConfig:
    """rtk.h rtk_motion_params without the image size."""
    fov_degrees: float = 90.0      # of the frame whose planes are handed in and of the previous view, as RenderConfig.fov_degrees

    def to_c(self, width: int, height: int) -> MotionParams:
        return MotionParams(width, height, float(self.fov_degrees))


@dataclass(frozen=True)
class Rect:
    """rtk_rect / render_tile (render/tile/tile.hpp): pixels [x0, x1) x [y0, y1) of the frame."""
    x0: int
    y0: int
    x1: int
    y1: int

    @property
    def width(self) -> int:
        return self.x1 - self.x0

    @property
    def height(self) -> int:
        return self.y1 - self.y0

    @property
    def area(self) -> int:
        return self.width * self.height


def _rects_array(rects) -> np.ndarray:
    """Rects, 4-tuples or a (K, 4) integer array -> contiguous (K, 4) int32 rows of x0, y0, x1, y1 (the layout of rtk_rect)."""
    if isinstance(rects, np.ndarray):
        arr = rects
    else:
        arr = np.array([(r.x0, r.y0, r.x1, r.y1) if isinstance(r, Rect) else tuple(r) for r in rects], np.int64).reshape(-1, 4)
    if arr.ndim != 2 or arr.shape[1] != 4 or arr.dtype.kind not in "iu":
        raise ValueError("rects must be Rects or a (K, 4) integer array of x0, y0, x1, y1")
    if arr.size and (int(arr.min()) < -2**31 or int(arr.max()) >= 2**31):
        raise ValueError("rectangle coordinates are 32-bit integers")
    return np.ascontiguousarray(arr, np.int32)


@dataclass
class RadianceConfig:
    """rtk_radiance_params: what color_hit needs of config.hpp:6-17, + the RNG sample and the <cull> of the batch's own rays."""
    max_ray_depth: int = 5
    diffuse_rays: int = 0
    seed: int = 42
    sample: int = 0            # which sample of `seed`'s sequence the rays are (with ids: the RNG root key of every ray)
    shadow_bias: float = 1e-4
    reflection_bias: float = 1e-4
    refraction_bias: float = 1e-4
    cull: bool = True          # True: as render_frame's camera rays (render.hpp:64); False: as a secondary ray
    trace_mode: int = TRACE_AUTO

    def to_c(self) -> RadianceParams:
        return RadianceParams(self.max_ray_depth, self.diffuse_rays, self.seed, self.sample, np.float32(self.shadow_bias),
                              np.float32(self.reflection_bias), np.float32(self.refraction_bias), 1 if self.cull else 0,
                              self.trace_mode)


def _views_array(views) -> np.ndarray:
    """-> contiguous float32 [K, 12]: position and matrix of K cameras (rtk.h rtk_view)"""
    views = np.asarray(views)
    if views.dtype != np.float32 or views.ndim != 2 or views.shape[1] != 12:
        raise ValueError("views must be float32 of shape (K, 12)")
    return np.ascontiguousarray(views)


def _first_pass_buffer(cfg: RenderConfig, shape) -> np.ndarray:
    """the zeros a call renders into when it was given no buffer, which only the first pass of a progressive render can be"""
    if cfg.sample_begin > 0:
        raise ValueError("a pass with sample_begin > 0 needs the buffer the previous passes rendered into")
    return np.zeros(shape, np.float32)


def _plane(a, shape, name: str, dtype=np.float32, required: bool = False):
    """a caller's plane as a contiguous array of `shape`; None for one that was not given and is not required"""
    if a is None:
        if required:
            raise ValueError(f"{name} is required")
        return None
    a = np.ascontiguousarray(a, dtype)
    if a.shape != shape:
        raise ValueError(f"{name} must have shape {shape}, not {a.shape}")
    return a


class KdTreeSimdAccel:
    """kd_tree_simd_accel<float, eps, max_depth, max_leaf_size> (render/accel/kd_tree_simd.hpp:63-98).

    normalize_hit_normal=False gives kd_tree_accel's un-normalised hit_normal (kd_tree.hpp:140)."""

    def __init__(self, scene: Scene, eps: float = 1e-6, max_depth: int = 8, max_leaf_size: int = 64,
                 normalize_hit_normal: bool = True, device: int = -1, traversal: int = TRAVERSAL_REFERENCE):
        self.scene = scene  # the reference keeps scene_ptr public (render.hpp:21)
        p = AccelParams(max_depth, max_leaf_size, np.float32(eps), 1 if normalize_hit_normal else 0, device, traversal)
        h = _vp()
        _check(_L.rtk_accel_build(scene._h, C.byref(p), C.byref(h)))
        self._h = h

    # ---- tree introspection
    def tree_info(self) -> TreeInfo:
        ti = TreeInfo()
        _check(_L.rtk_accel_tree_info(self._h, C.byref(ti)))
        return ti

    def tree_dump(self):
        ti = self.tree_info()
        box = np.zeros((ti.n_nodes, 6), np.float32)
        link = np.zeros((ti.n_nodes, 4), np.int32)
        refs = np.zeros((ti.n_leaf_refs,), np.int32)
        _check(_L.rtk_accel_tree_dump(self._h, box.ctypes.data, link.ctypes.data, refs.ctypes.data))
        return box, link, refs

    # ---- accel.intersect<cull>(ray), batched
    def intersect(self, rays: np.ndarray, cull: bool, trace_mode: int = TRACE_AUTO) -> np.ndarray:
        """rays: [n,6] float32 (origin xyz, direction xyz) in host memory -> HIT_DTYPE[n]."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        out = np.zeros((rays.shape[0],), HIT_DTYPE)
        _check(_L.rtk_accel_intersect(self._h, rays.ctypes.data, rays.shape[0], 1 if cull else 0, trace_mode, out.ctypes.data))
        return out

    def intersect_device(self, d_rays_ptr: int, n: int, cull: bool, d_hits_ptr: int, trace_mode: int = TRACE_AUTO,
                         stream: int = 0) -> None:
        _check(_L.rtk_accel_intersect_device(self._h, d_rays_ptr, n, 1 if cull else 0, trace_mode, d_hits_ptr, stream))

    def intersect_stats(self, d_rays_ptr: int, n: int, cull: bool, d_hits_ptr: int, trace_mode: int = TRACE_AUTO) -> dict:
        c = Counters()
        _check(_L.rtk_accel_intersect_stats(self._h, d_rays_ptr, n, 1 if cull else 0, trace_mode, d_hits_ptr, C.byref(c)))
        return c.as_dict()

    # ---- is_occluded(accel, ray, max_t), batched
    def occluded(self, rays: np.ndarray, max_t: np.ndarray, shadow_bias: float = 1e-4, trace_mode: int = TRACE_AUTO,
                 count: bool = False):
        """is_occluded (render/render.hpp:110-131) for rays [n,6] float32 and max_t [n] float32 in host memory ->
        uint8[n] of OCC_CLEAR / OCC_OCCLUDED / OCC_STEP_LIMIT; with count=True also the number of closest-hit queries made."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        max_t = np.ascontiguousarray(max_t, np.float32).reshape(-1)
        if max_t.shape[0] != rays.shape[0]:
            raise ValueError("one max_t per ray")
        out = np.zeros((rays.shape[0],), np.uint8)
        n_int = C.c_uint64(0)
        _check(_L.rtk_accel_occluded(self._h, rays.ctypes.data, max_t.ctypes.data, rays.shape[0], np.float32(shadow_bias),
                                     trace_mode, out.ctypes.data, C.byref(n_int) if count else None))
        return (out, int(n_int.value)) if count else out

    def occluded_device(self, d_rays_ptr: int, d_max_t_ptr: int, n: int, d_out_ptr: int, shadow_bias: float = 1e-4,
                        trace_mode: int = TRACE_AUTO, stream: int = 0) -> None:
        _check(_L.rtk_accel_occluded_device(self._h, d_rays_ptr, d_max_t_ptr, n, np.float32(shadow_bias), trace_mode,
                                            d_out_ptr, stream))

    # ---- intersect<cull>(ray) + color_hit(accel, hit, 0), batched
    def radiance(self, rays: np.ndarray, ids: np.ndarray | None = None, cfg: RadianceConfig | None = None):
        """The colour every ray sees (render/render.hpp:64-69, 133-308) for rays [n,6] float32 in host memory ->
        ([n,3] float32, counters dict).  ids [n] uint32: the pixel index of each ray's RNG root key (None: the ray's index)."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        n = rays.shape[0]
        if ids is not None:
            ids = np.ascontiguousarray(ids)
            if ids.shape != (n,):
                raise ValueError("one id per ray")
            if ids.dtype.kind not in "iu" or (n and (int(ids.min()) < 0 or int(ids.max()) > 0xFFFFFFFF)):
                raise ValueError("ids are unsigned 32-bit pixel indices")
            ids = np.ascontiguousarray(ids, np.uint32)
        p = (cfg or RadianceConfig()).to_c()
        rgb = np.zeros((n, 3), np.float32)
        c = Counters()
        _check(_L.rtk_accel_radiance(self._h, rays.ctypes.data, None if ids is None else ids.ctypes.data, n, C.byref(p),
                                     rgb.ctypes.data, C.byref(c)))
        return rgb, c.as_dict()

    def radiance_device(self, d_rays_ptr: int, d_ids_ptr: int, n: int, d_rgb_ptr: int, cfg: RadianceConfig | None = None,
                        stream: int = 0) -> None:
        """Device buffers (d_ids_ptr 0 = no ids), stream-ordered; not capturable into a graph (rtk.h)."""
        p = (cfg or RadianceConfig()).to_c()
        _check(_L.rtk_accel_radiance_device(self._h, d_rays_ptr, d_ids_ptr or None, n, C.byref(p), d_rgb_ptr or None, stream))

    # ---- dynamic geometry: the accel of the same scene with its vertices moved (rtk.h, csrc/build.hip)
    def update_vertices(self, vertices: np.ndarray) -> None:
        """vertices: [n_vertices, 3] float32 in host memory, all meshes concatenated as in SceneDesc.  The tree is rebuilt on the
        device; afterwards the accel is bit for bit the one a new build of the moved scene would give."""
        vertices = np.asarray(vertices)
        n = self.scene.info.n_vertices
        if vertices.dtype != np.float32:
            raise ValueError("vertices must be float32")
        if vertices.shape != (n, 3):
            raise ValueError(f"vertices must have shape ({n}, 3)")
        vertices = np.ascontiguousarray(vertices)
        _check(_L.rtk_accel_update_vertices(self._h, vertices.ctypes.data))

    def update_vertices_device(self, d_vertices_ptr: int, stream: int = 0) -> None:
        """d_vertices_ptr: device float32 [n_vertices, 3]; stream-ordered on `stream`, blocks the host once; not capturable (rtk.h)."""
        _check(_L.rtk_accel_update_vertices_device(self._h, d_vertices_ptr or None, stream))

    # ---- dynamic geometry: the same meshes with other triangle lists as well (rtk.h, csrc/topology.hip)
    def _mesh_ntris(self, mesh_ntris) -> np.ndarray:
        mesh_ntris = np.asarray(mesh_ntris)
        if mesh_ntris.dtype.kind not in "iu" or mesh_ntris.shape != (self.scene.info.n_meshes,):
            raise ValueError(f"mesh_ntris must be {self.scene.info.n_meshes} integers, one per mesh")
        return np.ascontiguousarray(mesh_ntris, np.int32)

    def update_geometry(self, vertices: np.ndarray, indices: np.ndarray, mesh_ntris) -> None:
        """vertices: [n_vertices, 3] float32; indices: [sum(mesh_ntris), 3] uint32, mesh-local, the meshes' lists concatenated;
        mesh_ntris: one count per mesh.  All in host memory.  Afterwards the accel is bit for bit the one a new build of the scene
        with these three arrays would give (self.scene goes on describing what the accel was BUILT from; tree_info() has the new
        triangle count).  What the counts and indices hold is judged by the library (RtkError)."""
        vertices, indices = np.asarray(vertices), np.asarray(indices)
        n = self.scene.info.n_vertices
        if vertices.dtype != np.float32 or vertices.shape != (n, 3):
            raise ValueError(f"vertices must be float32 of shape ({n}, 3)")
        mesh_ntris = self._mesh_ntris(mesh_ntris)
        if indices.dtype != np.uint32 or indices.ndim != 2 or indices.shape[1] != 3:
            raise ValueError("indices must be uint32 of shape (n, 3)")
        if (mesh_ntris >= 0).all() and indices.shape[0] != int(mesh_ntris.sum(dtype=np.int64)):
            raise ValueError("indices must have one row per triangle of mesh_ntris")
        vertices, indices = np.ascontiguousarray(vertices), np.ascontiguousarray(indices)
        _check(_L.rtk_accel_update_geometry(self._h, vertices.ctypes.data, indices.ctypes.data if indices.size else None,
                                            mesh_ntris.ctypes.data))

    def update_geometry_device(self, d_vertices_ptr: int, d_indices_ptr: int, mesh_ntris, stream: int = 0) -> None:
        """d_vertices_ptr: device float32 [n_vertices, 3]; d_indices_ptr: device uint32 [sum(mesh_ntris), 3] (0 when there are no
        triangles); mesh_ntris: HOST integers.  Stream-ordered on `stream`, blocks the host once; not capturable (rtk.h)."""
        mesh_ntris = self._mesh_ntris(mesh_ntris)
        _check(_L.rtk_accel_update_geometry_device(self._h, d_vertices_ptr or None, d_indices_ptr or None, mesh_ntris.ctypes.data, stream))

    # ---- frames
    def _frame_size(self, cfg: RenderConfig):
        """(width, height) of a frame of cfg: 0 stands for the scene's own"""
        return cfg.width or self.scene.info.width, cfg.height or self.scene.info.height

    def output_floats(self, cfg: RenderConfig) -> int:
        n = C.c_size_t(0)
        p = cfg.to_c()
        _check(_L.rtk_render_output_floats(self._h, C.byref(p), C.byref(n)))
        return n.value

    def render_frame(self, cfg: RenderConfig, rgb: np.ndarray | None = None):
        """Whole frame into host memory: ([h,w,3] float32, counters dict).  `rgb`: the buffer to render into -- for a later
        pass of a progressive frame (cfg.sample_begin > 0) it holds the running sums of the passes before."""
        w, h = self._frame_size(cfg)
        p = cfg.to_c()
        n = self.output_floats(cfg)
        assert n == w * h * 3
        if rgb is None:
            rgb = _first_pass_buffer(cfg, (h, w, 3))
        assert rgb.dtype == np.float32 and rgb.shape == (h, w, 3) and rgb.flags.c_contiguous
        c = Counters()
        _check(_L.rtk_render_frame(self._h, C.byref(p), rgb.ctypes.data, C.byref(c)))
        return rgb, c.as_dict()

    def render_frame_device(self, cfg: RenderConfig, d_out_ptr: int, stream: int = 0) -> None:
        p = cfg.to_c()
        _check(_L.rtk_render_frame_device(self._h, C.byref(p), d_out_ptr, stream))

    def last_counters(self) -> dict:
        c = Counters()
        _check(_L.rtk_render_last_counters(self._h, C.byref(c)))
        return c.as_dict()

    def camera_rays(self, cfg: RenderConfig, sample: int = 0) -> np.ndarray:
        """[h, w, 6] float32: origin + direction of every pixel's camera ray for sample `sample` (render.hpp:35-62)."""
        w, h = self._frame_size(cfg)
        rays = np.zeros((h, w, 6), np.float32)
        p = cfg.to_c()
        _check(_L.rtk_camera_rays(self._h, C.byref(p), sample, rays.ctypes.data))
        return rays

    def camera_rays_device(self, cfg: RenderConfig, d_rays_ptr: int, sample: int = 0, stream: int = 0) -> None:
        p = cfg.to_c()
        _check(_L.rtk_camera_rays_device(self._h, C.byref(p), sample, d_rays_ptr, stream))

    # ---- the camera of a live accel, and many cameras in one call (rtk.h rtk_view: position[3], matrix[9] row-major)
    def camera(self):
        """(position [3], matrix [9]) float32: the camera later frames are rendered from."""
        v = np.zeros(12, np.float32)
        _check(_L.rtk_accel_get_camera(self._h, v.ctypes.data))
        return v[:3].copy(), v[3:].copy()

    def set_camera(self, position, matrix) -> None:
        """Later frames, camera rays and sharded frames are those of a fresh accel of the scene with this camera; needs no GPU."""
        v = np.concatenate([np.asarray(position, np.float32).reshape(-1), np.asarray(matrix, np.float32).reshape(-1)])
        if v.shape != (12,):
            raise ValueError("position has 3 floats, matrix 9 (row-major)")
        v = np.ascontiguousarray(v)
        _check(_L.rtk_accel_set_camera(self._h, v.ctypes.data))

    def render_views(self, cfg: RenderConfig, views: np.ndarray, rgb: np.ndarray | None = None):
        """views: [K, 12] float32 (position, matrix) in host memory -> ([K, h, w, 3] float32, counters summed over the views).
        View k is what set_camera(views[k]) + render_frame(cfg) gives; the accel's own camera stays.  `rgb`: as for render_frame."""
        views = _views_array(views)
        k = views.shape[0]
        w, h = self._frame_size(cfg)
        if rgb is None:
            rgb = _first_pass_buffer(cfg, (k, h, w, 3))
        assert rgb.dtype == np.float32 and rgb.shape == (k, h, w, 3) and rgb.flags.c_contiguous
        p = cfg.to_c()
        c = Counters()
        _check(_L.rtk_render_views(self._h, C.byref(p), views.ctypes.data if k else None, k, rgb.ctypes.data if k else None, C.byref(c)))
        return rgb, c.as_dict()

    def render_views_device(self, cfg: RenderConfig, d_views_ptr: int, n_views: int, d_out_ptr: int, stream: int = 0) -> None:
        """d_views_ptr: device float32 [n_views, 12]; d_out_ptr: device float32 [n_views, h, w, 3]; stream-ordered (rtk.h)."""
        p = cfg.to_c()
        _check(_L.rtk_render_views_device(self._h, C.byref(p), d_views_ptr or None, n_views, d_out_ptr or None, stream))

    # ---- rectangles of a frame in one call (rtk.h rtk_rect, RTK_REGIONS_*)
    def render_regions(self, cfg: RenderConfig, rects, layout: int = REGIONS_IN_FRAME, rgb: np.ndarray | None = None):
        """rects: Rects or a (K, 4) int32 array of x0, y0, x1, y1.  Every pixel inside a rectangle comes out as render_frame(cfg)
        leaves it; counters are the call's totals.
        REGIONS_IN_FRAME -> ([h, w, 3] float32, counters): only the rectangles' pixels of `rgb` are written (a new buffer is zeros).
        REGIONS_PACKED   -> (list of K views [y1-y0, x1-x0, 3] into one packed float32 array, counters); `rgb`: that packed array
        (1-D, 3 * the sum of the areas), e.g. `views[0].base` of an earlier pass of a progressive render."""
        arr = _rects_array(rects)
        k = arr.shape[0]
        w, h = self._frame_size(cfg)
        if layout == REGIONS_PACKED:
            areas = (arr[:, 2].astype(np.int64) - arr[:, 0]) * (arr[:, 3].astype(np.int64) - arr[:, 1])
            shape = (int(np.maximum(areas, 0).sum()) * 3,)
        else:
            shape = (h, w, 3)
        if rgb is None:
            rgb = _first_pass_buffer(cfg, shape)
        if rgb.dtype != np.float32 or rgb.shape != shape or not rgb.flags.c_contiguous:
            raise ValueError(f"rgb must be contiguous float32 of shape {shape}")
        p = cfg.to_c()
        c = Counters()
        out = rgb if rgb.size else np.zeros(1, np.float32)         # (a packed list without pixels: a valid pointer nothing is written through)
        _check(_L.rtk_render_regions(self._h, C.byref(p), arr.ctypes.data if k else None, k, layout, out.ctypes.data, C.byref(c)))
        if layout != REGIONS_PACKED:
            return rgb, c.as_dict()
        views, at = [], 0
        for x0, y0, x1, y1 in arr.tolist():
            n = (x1 - x0) * (y1 - y0) * 3
            views.append(rgb[at:at + n].reshape(y1 - y0, x1 - x0, 3))
            at += n
        return views, c.as_dict()

    def render_regions_device(self, cfg: RenderConfig, rects, layout: int, d_out_ptr: int, stream: int = 0) -> None:
        """rects in HOST memory (as render_regions); d_out_ptr: device float32, the frame or the packed array; stream-ordered (rtk.h)."""
        arr = _rects_array(rects)
        p = cfg.to_c()
        _check(_L.rtk_render_regions_device(self._h, C.byref(p), arr.ctypes.data if arr.shape[0] else None, arr.shape[0], layout,
                                            d_out_ptr or None, stream))

    # ---- what the camera rays hit, as planes (rtk.h rtk_gbuffer)
    def render_gbuffer(self, cfg: RenderConfig, sample: int = 0, views: np.ndarray | None = None,
                       planes=tuple(GBUFFER_PLANES)) -> dict:
        """First hit of every pixel's camera ray at sample `sample`: {plane name: array [K, h, w(, c)]} for the planes asked for.
        views: [K, 12] float32 (position, matrix), or None for the accel's own camera (K = 1).  Every plane but `albedo` holds the
        bits of camera_rays + intersect(cull=True); the accel's camera, launch orders and counters stay as they are."""
        unknown = [n for n in planes if n not in GBUFFER_PLANES]
        if unknown:
            raise ValueError(f"unknown g-buffer planes {unknown}: choose from {list(GBUFFER_PLANES)}")
        if views is None:
            k, vptr = 1, None
        else:
            views = _views_array(views)
            k = views.shape[0]
            if k == 0:
                views = np.zeros((1, 12), np.float32)               # (no views: a valid pointer nothing is read through)
            vptr = views.ctypes.data
        w, h = self._frame_size(cfg)
        out = {n: np.zeros((k, h, w) + GBUFFER_PLANES[n][0], GBUFFER_PLANES[n][1]) for n in GBUFFER_PLANES if n in planes}
        spare = np.zeros(1, np.uint32)                              # (likewise for planes without pixels)
        gb = GBuffer(**{n: a.ctypes.data if a.size else spare.ctypes.data for n, a in out.items()})
        p = cfg.to_c()
        _check(_L.rtk_render_gbuffer(self._h, C.byref(p), sample, vptr, k, C.byref(gb)))
        return out

    def render_gbuffer_device(self, cfg: RenderConfig, planes: dict, sample: int = 0, d_views_ptr: int = 0, n_views: int = 1,
                              stream: int = 0) -> None:
        """planes: {plane name: device pointer} of float32 / uint32 arrays [n_views, h, w(, c)], 4-byte aligned; d_views_ptr: device
        float32 [n_views, 12], or 0 for the accel's own camera (n_views = 1); stream-ordered, allocates nothing (rtk.h)."""
        unknown = [n for n in planes if n not in GBUFFER_PLANES]
        if unknown:
            raise ValueError(f"unknown g-buffer planes {unknown}: choose from {list(GBUFFER_PLANES)}")
        gb = GBuffer(**{n: (int(ptr) or None) for n, ptr in planes.items()})
        p = cfg.to_c()
        _check(_L.rtk_render_gbuffer_device(self._h, C.byref(p), sample, d_views_ptr or None, n_views, C.byref(gb), stream))

    # ---- the first surface that is shaded behind mirrors and glass, as planes (rtk.h rtk_gbuffer_specular)
    def render_gbuffer_specular(self, cfg: RenderConfig, sample: int = 0, views: np.ndarray | None = None,
                                planes=tuple(SPECULAR_GBUFFER_PLANES)) -> dict:
        """The end of every pixel's specular chain at sample `sample` (reflections, refractions, total internal reflections, at most
        cfg.max_ray_depth of them): {plane name: array [K, h, w(, c)]} for the planes asked for.  views as render_gbuffer.  depth,
        position and normal describe the end hit in the virtual world behind the mirrors (what temporal_accumulate and denoise_frame
        take in place of render_gbuffer's planes); the other planes are the end hit's own, bounces the secondary rays traced and
        last_ray the ray that found it; the accel's camera, launch orders and counters stay as they are."""
        unknown = [n for n in planes if n not in SPECULAR_GBUFFER_PLANES]
        if unknown:
            raise ValueError(f"unknown specular g-buffer planes {unknown}: choose from {list(SPECULAR_GBUFFER_PLANES)}")
        if views is None:
            k, vptr = 1, None
        else:
            views = _views_array(views)
            k = views.shape[0]
            if k == 0:
                views = np.zeros((1, 12), np.float32)               # (no views: a valid pointer nothing is read through)
            vptr = views.ctypes.data
        w, h = self._frame_size(cfg)
        out = {n: np.zeros((k, h, w) + shape, dtype) for n, (shape, dtype) in SPECULAR_GBUFFER_PLANES.items() if n in planes}
        spare = np.zeros(1, np.uint32)                              # (likewise for planes without pixels)
        gb = SpecularGBuffer(**{n: a.ctypes.data if a.size else spare.ctypes.data for n, a in out.items()})
        p = cfg.to_c()
        _check(_L.rtk_render_gbuffer_specular(self._h, C.byref(p), sample, vptr, k, C.byref(gb)))
        return out

    def render_gbuffer_specular_device(self, cfg: RenderConfig, planes: dict, sample: int = 0, d_views_ptr: int = 0, n_views: int = 1,
                                       stream: int = 0) -> None:
        """planes: {plane name: device pointer} of float32 / uint32 arrays [n_views, h, w(, c)], 4-byte aligned; d_views_ptr: device
        float32 [n_views, 12], or 0 for the accel's own camera (n_views = 1); stream-ordered, allocates nothing (rtk.h)."""
        unknown = [n for n in planes if n not in SPECULAR_GBUFFER_PLANES]
        if unknown:
            raise ValueError(f"unknown specular g-buffer planes {unknown}: choose from {list(SPECULAR_GBUFFER_PLANES)}")
        gb = SpecularGBuffer(**{n: (int(ptr) or None) for n, ptr in planes.items()})
        p = cfg.to_c()
        _check(_L.rtk_render_gbuffer_specular_device(self._h, C.byref(p), sample, d_views_ptr or None, n_views, C.byref(gb), stream))

    # ---- where each pixel's surface point was in the previous pose (rtk.h rtk_motion_params)
    def render_motion(self, tri: np.ndarray, bary: np.ndarray, prev_vertices: np.ndarray, prev_view=None,
                      cfg: MotionConfig | None = None, planes=("prev_position", "motion")) -> dict:
        """tri [h, w] uint32 and bary [h, w, 2] float32: planes of render_gbuffer for ONE view; prev_vertices [n_vertices, 3] float32:
        the previous pose, all meshes concatenated as in SceneDesc; prev_view = (position[3], matrix[9]), the previous camera,
        needed for `motion`.  -> {"prev_position": [h, w, 3], "motion": [h, w, 2]} for the planes asked for: the point of the
        previous pose under each pixel (0 on a miss; hand it to temporal_accumulate as cur's position) and previous place minus
        present place in pixels (the bits MOTION_MISS_BITS where there is none).  The accel's current triangle lists are used."""
        tri = np.ascontiguousarray(tri)
        if tri.dtype != np.uint32 or tri.ndim != 2 or tri.size == 0:
            raise ValueError("tri must be uint32 [h, w] and not empty")
        h, w = tri.shape
        bary = _plane(bary, (h, w, 2), "bary", required=True)
        n = self.scene.info.n_vertices
        prev_vertices = _plane(prev_vertices, (n, 3), "prev_vertices", required=True)
        unknown = [p for p in planes if p not in ("prev_position", "motion")]
        if unknown:
            raise ValueError(f"unknown motion planes {unknown}: choose from prev_position, motion")
        out = {}
        if "prev_position" in planes:
            out["prev_position"] = np.zeros((h, w, 3), np.float32)
        if "motion" in planes:
            out["motion"] = np.zeros((h, w, 2), np.float32)
        keep = None if prev_view is None else _view_record(prev_view)
        spare = np.zeros(1, np.float32)                              # (a scene without vertices: a valid pointer nothing is read through)
        outs = MotionOutputs(*(out[k].ctypes.data if k in out else None for k, _ in MotionOutputs._fields_))
        p = (cfg or MotionConfig()).to_c(w, h)
        _check(_L.rtk_render_motion(self._h, C.byref(p), tri.ctypes.data, bary.ctypes.data,
                                    prev_vertices.ctypes.data if prev_vertices.size else spare.ctypes.data,
                                    None if keep is None else keep.ctypes.data, C.byref(outs)))
        return out

    def render_motion_device(self, width: int, height: int, d_tri_ptr: int, d_bary_ptr: int, d_prev_vertices_ptr: int, out: dict,
                             prev_view=None, cfg: MotionConfig | None = None, stream: int = 0) -> None:
        """The same on raw device pointers (ints): out = {"prev_position": ptr, "motion": ptr}, 0 or a missing key = plane not
        wanted; prev_view = (position[3], matrix[9]) as HOST values.  Stream-ordered; allocates nothing and never blocks the host
        once the accel's topology tables exist (the first call on an accel no update has touched makes them) (rtk.h)."""
        keep = None if prev_view is None else _view_record(prev_view)
        outs = MotionOutputs(*((out.get(k) or None) for k, _ in MotionOutputs._fields_))
        p = (cfg or MotionConfig()).to_c(width, height)
        _check(_L.rtk_render_motion_device(self._h, C.byref(p), d_tri_ptr or None, d_bary_ptr or None, d_prev_vertices_ptr or None,
                                           None if keep is None else keep.ctypes.data, C.byref(outs), stream or None))

    # ---- a frame whose pixel blocks stop sampling once they have converged (rtk.h rtk_adaptive_params)
    def render_adaptive(self, cfg: RenderConfig, adaptive: AdaptiveConfig):
        """-> (rgb [h, w, 3] float32, samples [h, w] uint32, noise [h, w] float32, counters).  Every pixel is, bit for bit, the pixel
        of render_frame(cfg with spp = samples[pixel]); samples is constant over an 8x8 block; noise is the standard error of the
        pixel's mean luminance at its final count (the statistic is spelt out in rtk.h)."""
        w, h = self._frame_size(cfg)
        rgb = np.zeros((h, w, 3), np.float32)
        samples = np.zeros((h, w), np.uint32)
        noise = np.zeros((h, w), np.float32)
        p, ap = cfg.to_c(), adaptive.to_c()
        c = Counters()
        _check(_L.rtk_render_adaptive(self._h, C.byref(p), C.byref(ap), rgb.ctypes.data, samples.ctypes.data, noise.ctypes.data, C.byref(c)))
        return rgb, samples, noise, c.as_dict()

    def render_adaptive_device(self, cfg: RenderConfig, adaptive: AdaptiveConfig, d_rgb_ptr: int, d_samples_ptr: int = 0,
                               d_noise_ptr: int = 0, stream: int = 0) -> None:
        """d_rgb_ptr: device float32 [h, w, 3]; d_samples_ptr / d_noise_ptr: device uint32 / float32 [h, w], or 0.  Stream-ordered,
        but blocks the host once per round (rtk.h); not capturable."""
        p, ap = cfg.to_c(), adaptive.to_c()
        _check(_L.rtk_render_adaptive_device(self._h, C.byref(p), C.byref(ap), d_rgb_ptr or None, d_samples_ptr or None,
                                             d_noise_ptr or None, stream))

    # ---- a frame of a fixed sample count with the noise plane the denoiser weights by (rtk.h rtk_render_frame_noise)
    def render_frame_noise(self, cfg: RenderConfig):
        """-> (rgb [h, w, 3] float32, noise [h, w] float32, counters).  rgb and counters are render_frame(cfg)'s, noise is, bit for bit,
        the noise plane of render_adaptive(cfg, min_samples = cfg.spp): the standard error of the pixel's mean luminance after all
        cfg.spp samples.  A streamed frame (TRACE_AUTO means TRACE_STREAM here), cfg.spp >= 2, not progressive, not sharded."""
        w, h = self._frame_size(cfg)
        rgb = np.zeros((h, w, 3), np.float32)
        noise = np.zeros((h, w), np.float32)
        p = cfg.to_c()
        c = Counters()
        _check(_L.rtk_render_frame_noise(self._h, C.byref(p), rgb.ctypes.data, noise.ctypes.data, C.byref(c)))
        return rgb, noise, c.as_dict()

    def render_frame_noise_device(self, cfg: RenderConfig, d_rgb_ptr: int, d_noise_ptr: int, stream: int = 0) -> None:
        """d_rgb_ptr: device float32 [h, w, 3]; d_noise_ptr: device float32 [h, w].  Stream-ordered, but blocks the host once at its
        end, to learn whether a queue overflowed (rtk.h); not capturable."""
        p = cfg.to_c()
        _check(_L.rtk_render_frame_noise_device(self._h, C.byref(p), d_rgb_ptr or None, d_noise_ptr or None, stream))

    def noise_fallbacks(self) -> int:
        """rtk.h rtk_debug_noise_fallbacks: render_frame_noise calls on this accel that were redone because a queue overflowed."""
        n = C.c_uint64(0)
        _check(_L.rtk_debug_noise_fallbacks(self._h, C.byref(n)))
        return n.value

    # ---- lights, materials and background of a live accel (rtk.h rtk_light, rtk_material)
    def lights(self):
        """(positions [n, 3], intensities [n]) float32: the lights later frames are lit by."""
        n = C.c_int32(0)
        _check(_L.rtk_accel_get_lights(self._h, None, 0, C.byref(n)))
        tab = np.zeros(n.value, LIGHT_DTYPE)
        _check(_L.rtk_accel_get_lights(self._h, tab.ctypes.data if n.value else None, n.value, C.byref(n)))
        return tab["position"].copy(), tab["intensity"].copy()

    def set_lights(self, positions, intensities) -> None:
        """positions [n, 3], intensities [n]; n is free.  Later frames are those of a fresh accel of the scene with these lights.
        Needs no GPU on an accel that has not rendered yet."""
        pos, inten = np.asarray(positions, np.float32), np.asarray(intensities, np.float32)
        if inten.ndim != 1 or pos.shape != (inten.shape[0], 3):
            raise ValueError("positions must have shape (n, 3) and intensities (n,)")
        tab = np.zeros(inten.shape[0], LIGHT_DTYPE)
        tab["position"], tab["intensity"] = pos, inten
        _check(_L.rtk_accel_set_lights(self._h, tab.ctypes.data if tab.size else None, tab.shape[0]))

    def set_lights_device(self, d_lights_ptr: int, n: int, stream: int = 0) -> None:
        """d_lights_ptr: device float32 [n, 4] (x, y, z, intensity); copied on `stream`, later work on any stream sees it (rtk.h)."""
        _check(_L.rtk_accel_set_lights_device(self._h, d_lights_ptr or None, n, stream))

    def materials(self) -> dict:
        """kind [m] int32, albedo [m, 3], ior [m] float32, smooth [m], texture [m] int32 (-1 unless kind is MAT_TEXTURE)."""
        tab = np.zeros(self.scene.info.n_materials, MATERIAL_DTYPE)
        _check(_L.rtk_accel_get_materials(self._h, tab.ctypes.data))
        return {k: tab[k].copy() for k in ("kind", "albedo", "ior", "smooth", "texture")}

    def set_materials(self, kind, albedo, ior, smooth, texture=None) -> None:
        """One row per material of the scene (their number is fixed).  What the values hold is judged by the library (RtkError)."""
        m = self.scene.info.n_materials
        kind, smooth = np.asarray(kind), np.asarray(smooth)
        albedo, ior = np.asarray(albedo, np.float32), np.asarray(ior, np.float32)
        texture = np.full(m, -1, np.int32) if texture is None else np.asarray(texture)
        for a in (kind, smooth, texture):
            if a.shape != (m,) or a.dtype.kind not in "iub":
                raise ValueError(f"kind, smooth and texture must be {m} integers, one per material")
        if albedo.shape != (m, 3) or ior.shape != (m,):
            raise ValueError(f"albedo must have shape ({m}, 3) and ior ({m},)")
        tab = np.zeros(m, MATERIAL_DTYPE)
        tab["kind"], tab["smooth"], tab["albedo"], tab["ior"], tab["texture"] = kind, smooth, albedo, ior, texture
        _check(_L.rtk_accel_set_materials(self._h, tab.ctypes.data, m))

    def background(self) -> np.ndarray:
        rgb = np.zeros(3, np.float32)
        _check(_L.rtk_accel_get_background(self._h, rgb.ctypes.data))
        return rgb

    def set_background(self, rgb) -> None:
        rgb = np.asarray(rgb, np.float32)
        if rgb.shape != (3,):
            raise ValueError("the background has 3 floats")
        rgb = np.ascontiguousarray(rgb)
        _check(_L.rtk_accel_set_background(self._h, rgb.ctypes.data))

    # ---- textures and uvs of a live accel (rtk.h rtk_texture)
    def textures(self) -> dict:
        """kind [t] int32, color_a [t, 3], color_b [t, 3], param [t] float32, width [t], height [t] int32 (0 unless TEX_BITMAP)."""
        n = C.c_int32(0)
        _check(_L.rtk_accel_get_textures(self._h, None, 0, C.byref(n)))
        tab = np.zeros(n.value, TEXTURE_DTYPE)
        _check(_L.rtk_accel_get_textures(self._h, tab.ctypes.data if n.value else None, n.value, C.byref(n)))
        return {k: tab[k].copy() for k in TEXTURE_DTYPE.names}

    def set_textures(self, kind, color_a=None, color_b=None, param=None, pixels=None) -> None:
        """Replaces the whole texture table; the number of textures is free.  `pixels`: one entry per texture, uint8 [h, w, 3] for
        a TEX_BITMAP and ignored (None) for every other kind.  What the values hold is judged by the library (RtkError)."""
        kind = np.asarray(kind)
        if kind.ndim != 1 or (kind.size and kind.dtype.kind not in "iub"):
            raise ValueError("kind must be a list of integers, one per texture")
        t = kind.shape[0]
        color_a = np.zeros((t, 3), np.float32) if color_a is None else np.asarray(color_a, np.float32)
        color_b = np.zeros((t, 3), np.float32) if color_b is None else np.asarray(color_b, np.float32)
        param = np.zeros(t, np.float32) if param is None else np.asarray(param, np.float32)
        if color_a.shape != (t, 3) or color_b.shape != (t, 3) or param.shape != (t,):
            raise ValueError(f"color_a and color_b must have shape ({t}, 3) and param ({t},)")
        pixels = [None] * t if pixels is None else list(pixels)
        if len(pixels) != t:
            raise ValueError("pixels must have one entry per texture")
        tab = np.zeros(t, TEXTURE_DTYPE)
        tab["kind"], tab["color_a"], tab["color_b"], tab["param"] = kind, color_a, color_b, param
        keep, ptrs = [], (_vp * max(1, t))()
        for i in range(t):
            if pixels[i] is None or kind[i] != TEX_BITMAP:
                continue
            px = np.ascontiguousarray(pixels[i], np.uint8)
            if px.ndim != 3 or px.shape[2] != 3:
                raise ValueError("the texels of a bitmap are uint8 [height, width, 3]")
            tab["height"][i], tab["width"][i] = px.shape[0], px.shape[1]
            keep.append(px)
            ptrs[i] = px.ctypes.data
        _check(_L.rtk_accel_set_textures(self._h, tab.ctypes.data if t else None, t, ptrs))

    def texture_pixels(self, texture: int) -> np.ndarray:
        """uint8 [h, w, 3] of one bitmap texture (an empty array for another kind), fetched from the device after a device-side
        replacement."""
        n = C.c_size_t(0)
        _check(_L.rtk_accel_get_texture_pixels(self._h, texture, None, 0, C.byref(n)))
        tex = self.textures()
        out = np.zeros((int(tex["height"][texture]), int(tex["width"][texture]), 3), np.uint8)
        assert out.size == n.value
        if out.size:
            _check(_L.rtk_accel_get_texture_pixels(self._h, texture, out.ctypes.data, out.size, C.byref(n)))
        return out

    def set_texture_pixels(self, texture: int, rgb) -> None:
        """New texels for one bitmap texture: uint8 [h, w, 3], rows top-down; the size may differ from before."""
        px = np.asarray(rgb)
        if px.dtype != np.uint8 or px.ndim != 3 or px.shape[2] != 3:
            raise ValueError("the texels of a bitmap are uint8 [height, width, 3]")
        px = np.ascontiguousarray(px)
        _check(_L.rtk_accel_set_texture_pixels(self._h, texture, px.shape[1], px.shape[0], px.ctypes.data if px.size else None))

    def set_texture_pixels_device(self, texture: int, width: int, height: int, d_rgb_ptr: int, stream: int = 0) -> None:
        """d_rgb_ptr: device uint8 [height, width, 3]; copied on `stream`, later work on any stream sees it (rtk.h)."""
        _check(_L.rtk_accel_set_texture_pixels_device(self._h, texture, width, height, d_rgb_ptr or None, stream))

    def set_texture_frame_device(self, texture: int, width: int, height: int, d_rgb_ptr: int, stream: int = 0) -> None:
        """Render to texture: d_rgb_ptr is a device float32 frame [height, width, 3]; the texels become its write_ppm bytes."""
        _check(_L.rtk_accel_set_texture_frame_device(self._h, texture, width, height, d_rgb_ptr or None, stream))

    def uvs(self) -> np.ndarray:
        """float32 [n_vertices, 2]: the uvs of all meshes' vertices, zeros for a mesh that has none."""
        out = np.zeros((self.scene.info.n_vertices, 2), np.float32)
        _check(_L.rtk_accel_get_uvs(self._h, out.ctypes.data))
        return out

    def set_uvs(self, uv) -> None:
        uv = np.asarray(uv, np.float32)
        if uv.shape != (self.scene.info.n_vertices, 2):
            raise ValueError(f"uvs must have shape ({self.scene.info.n_vertices}, 2)")
        uv = np.ascontiguousarray(uv)
        _check(_L.rtk_accel_set_uvs(self._h, uv.ctypes.data))

    def set_uvs_device(self, d_uvs_ptr: int, stream: int = 0) -> None:
        """d_uvs_ptr: device float32 [n_vertices, 2]; read on `stream`, later work on any stream sees the new uvs (rtk.h)."""
        _check(_L.rtk_accel_set_uvs_device(self._h, d_uvs_ptr or None, stream))

    def last_critical_path_ms(self) -> float:
        """Longest 8x8 pixel block of the most recent megakernel frame (ms): the frame's critical path."""
        ms = C.c_double(0.0)
        _check(_L.rtk_render_last_critical_path(self._h, C.byref(ms)))
        return ms.value

    def counter_fills(self) -> int:
        """Diagnostic: fills of the counters issued by this accel's frames, views and regions calls so far (a steady frame issues none)."""
        n = C.c_uint64(0)
        _check(_L.rtk_debug_counter_fills(self._h, C.byref(n)))
        return int(n.value)

    def order_judge(self, table: int = ORDER_TABLE_FRAMES, index: int = 0) -> dict:
        """Diagnostic (rtk.h rtk_debug_order_judge): sorts and judges so far of this accel's frames (or of launch `index` of its views
        / regions calls: ORDER_TABLE_VIEWS / _REGIONS), challengers taken and rejected, the champion's and the newest challenger's
        score in 100 MHz ticks, the units of the lists and the set the next launch reads."""
        st = OrderJudgeStats()
        _check(_L.rtk_debug_order_judge(self._h, table, index, C.byref(st)))
        return st.as_dict()

    def order_lists(self, which: int):
        """Diagnostic (rtk.h rtk_debug_order_lists): set `which` (0 or 1) of the frames' launch lists as the device holds it ->
        (order [units], header [4], workgroup list [units]) as uint32 arrays, or None before any list exists."""
        n = C.c_size_t(0)
        _check(_L.rtk_debug_order_lists(self._h, which, None, 0, C.byref(n)))
        if n.value == 0:
            return None
        words = np.empty(n.value, np.uint32)
        _check(_L.rtk_debug_order_lists(self._h, which, words.ctypes.data, words.size, C.byref(n)))
        units = (n.value - 4) // 2
        return words[:units], words[units:units + 4], words[units + 4:]

    def assemble_device(self, cfg: RenderConfig, d_gathered_ptr: int, d_rgb_ptr: int, stream: int = 0) -> None:
        p = cfg.to_c()
        _check(_L.rtk_tiles_assemble_device(self._h, C.byref(p), d_gathered_ptr, d_rgb_ptr, stream))

    def __del__(self, _destroy=_L.rtk_accel_destroy):
        if getattr(self, "_h", None):
            _destroy(self._h)
            self._h = None


def render_frame(accel: KdTreeSimdAccel, cfg: RenderConfig | None = None):
    """render_frame<A,F>(accel, BUCKET_TILES) (render/render.hpp:18-108)."""
    return accel.render_frame(cfg or RenderConfig())


def format_ppm(rgb: np.ndarray) -> bytes:
    rgb = np.ascontiguousarray(rgb, np.float32)
    h, w, _ = rgb.shape
    n = C.c_size_t(0)
    _check(_L.rtk_format_ppm(rgb.ctypes.data, w, h, None, 0, C.byref(n)))
    buf = C.create_string_buffer(n.value)
    _check(_L.rtk_format_ppm(rgb.ctypes.data, w, h, buf, n.value, C.byref(n)))
    return buf.raw[: n.value]


def frame_to_rgb8_device(d_rgb_ptr: int, n_floats: int, d_out_ptr: int, stream: int = 0) -> None:
    """uint8(255.999 * clamp(c, 0, 1)) per channel on the device (io/image/ppm.hpp:17-19)."""
    _check(_L.rtk_frame_to_rgb8_device(d_rgb_ptr, n_floats, d_out_ptr, stream))


# ---- an edge-avoiding filter of a frame, guided by the g-buffer (rtk.h rtk_denoise_params)
def denoise_workspace_bytes(width: int, height: int, n_images: int = 1, cfg: DenoiseConfig | None = None) -> int:
    """Bytes of device workspace denoise_device needs for n_images images of width x height (at most 64 per pixel)."""
    p = (cfg or DenoiseConfig()).to_c(width, height)
    n = C.c_size_t(0)
    _check(_L.rtk_denoise_workspace_bytes(C.byref(p), n_images, C.byref(n)))
    return n.value


def denoise(rgb: np.ndarray, normal: np.ndarray, position: np.ndarray, depth: np.ndarray, noise: np.ndarray | None = None,
            albedo: np.ndarray | None = None, cfg: DenoiseConfig | None = None) -> np.ndarray:
    """rgb filtered along the surfaces that normal, position and depth describe (the planes render_gbuffer writes), weighted by
    the variance noise ** 2 (the plane render_adaptive writes) and, with albedo, with the texture divided out first.  rgb, normal,
    position, albedo: float32 [h, w, 3] or [K, h, w, 3]; depth, noise: [h, w] or [K, h, w].  -> float32 of rgb's shape.  The
    arithmetic is spelt out in rtk.h; a pixel whose depth is not >= 0 keeps its bits."""
    rgb = np.ascontiguousarray(rgb, np.float32)
    if rgb.ndim not in (3, 4) or rgb.shape[-1] != 3:
        raise ValueError("rgb must be [h, w, 3] or [K, h, w, 3]")
    lead = rgb.shape[:-1]
    k = 1 if rgb.ndim == 3 else lead[0]
    h, w = lead[-2], lead[-1]

    normal, position = _plane(normal, rgb.shape, "normal"), _plane(position, rgb.shape, "position")
    albedo = _plane(albedo, rgb.shape, "albedo")
    depth, noise = _plane(depth, lead, "depth"), _plane(noise, lead, "noise")
    if normal is None or position is None or depth is None:
        raise ValueError("normal, position and depth are required")
    out = np.zeros_like(rgb)
    if rgb.size == 0:
        return out
    ptr = lambda a: None if a is None else a.ctypes.data
    inputs = DenoiseInputs(ptr(rgb), ptr(noise), ptr(albedo), ptr(normal), ptr(position), ptr(depth))
    p = (cfg or DenoiseConfig()).to_c(w, h)
    _check(_L.rtk_denoise_frame(C.byref(p), k, C.byref(inputs), out.ctypes.data))
    return out


def denoise_device(width: int, height: int, d_rgb_ptr: int, d_normal_ptr: int, d_position_ptr: int, d_depth_ptr: int, d_out_ptr: int,
                   d_workspace_ptr: int, workspace_bytes: int, d_noise_ptr: int = 0, d_albedo_ptr: int = 0, n_images: int = 1,
                   cfg: DenoiseConfig | None = None, stream: int = 0) -> None:
    """The same on device planes (float32, 4-byte aligned; d_noise_ptr / d_albedo_ptr may be 0), into d_out_ptr, which may be
    d_rgb_ptr.  d_workspace_ptr: denoise_workspace_bytes(...) bytes of scratch, 16-byte aligned.  Stream-ordered on the current
    device, allocates nothing, never blocks the host (rtk.h)."""
    inputs = DenoiseInputs(d_rgb_ptr or None, d_noise_ptr or None, d_albedo_ptr or None, d_normal_ptr or None, d_position_ptr or None,
                           d_depth_ptr or None)
    p = (cfg or DenoiseConfig()).to_c(width, height)
    _check(_L.rtk_denoise_frame_device(C.byref(p), n_images, C.byref(inputs), d_out_ptr or None, d_workspace_ptr or None,
                                       workspace_bytes, stream or None))


# ---- temporal accumulation: a frame blended with the reprojected history of the previous camera (rtk.h rtk_temporal_params)
def _view_record(view) -> np.ndarray:
    """(position[3], matrix[9] or [3, 3]) -> the 12 floats of an rtk_view"""
    position, matrix = view
    v = np.concatenate([np.asarray(position, np.float32).reshape(3), np.asarray(matrix, np.float32).reshape(9)])
    return np.ascontiguousarray(v, np.float32)


def temporal_accumulate(cur: dict, prev: dict | None, cfg: TemporalConfig | None = None, clamp: ClampConfig | None = None) -> dict:
    """The frame `cur` blended with the history `prev`, fetched where cur's world positions lay in prev's camera.  cur: rgb,
    position, normal [h, w, 3] and depth [h, w] float32 (the planes render_frame_noise and render_gbuffer write), optionally noise
    [h, w] float32 and mesh [h, w] uint32.  prev: None to start a history, else rgb, noise and length of the previous call's
    result, position, normal, depth (and mesh) of the previous frame's g-buffer and view = (position[3], matrix[9]), its camera;
    it has noise / mesh exactly when cur has.  -> dict rgb [h, w, 3], noise [h, w] or None, length [h, w].  The arithmetic is
    spelt out in rtk.h; a pixel without history keeps its bits and gets length 1.  clamp: None for rtk_temporal_accumulate, else
    rtk_temporal_accumulate_clamped, which pulls the history into the colour statistics of cur's neighbourhood first."""
    rgb = np.ascontiguousarray(cur["rgb"], np.float32)
    if rgb.ndim != 3 or rgb.shape[-1] != 3 or rgb.size == 0:
        raise ValueError("rgb must be [h, w, 3] and not empty")
    h, w = rgb.shape[:2]

    def plane(d, name, trailing=(), dtype=np.float32, required=True):
        return _plane(d.get(name), (h, w) + trailing, name, dtype, required)

    def planes(d, history):
        o = dict(rgb=plane(d, "rgb", (3,)), noise=plane(d, "noise", required=False), position=plane(d, "position", (3,)),
                 normal=plane(d, "normal", (3,)), depth=plane(d, "depth"), mesh=plane(d, "mesh", dtype=np.uint32, required=False))
        if history:
            o["length"] = plane(d, "length")
        return o

    ptr = lambda a: None if a is None else a.ctypes.data
    c = planes(cur, False)
    frame = TemporalFrame(*(ptr(c[n]) for n, _ in TemporalFrame._fields_))
    hist = keep = None
    if prev is not None:
        q = planes(prev, True)
        if "view" not in prev or prev["view"] is None:
            raise ValueError("prev needs view = (position, matrix)")
        keep = _view_record(prev["view"])
        q["view"] = keep
        hist = TemporalHistory(*(ptr(q[n]) for n, _ in TemporalHistory._fields_))
    out = dict(rgb=np.zeros((h, w, 3), np.float32), noise=None if c["noise"] is None else np.zeros((h, w), np.float32),
               length=np.zeros((h, w), np.float32))
    outs = TemporalOutputs(ptr(out["rgb"]), ptr(out["noise"]), ptr(out["length"]))
    p = (cfg or TemporalConfig()).to_c(w, h)
    if clamp is None:
        _check(_L.rtk_temporal_accumulate(C.byref(p), C.byref(frame), None if hist is None else C.byref(hist), C.byref(outs)))
    else:
        k = clamp.to_c()
        _check(_L.rtk_temporal_accumulate_clamped(C.byref(p), C.byref(k), C.byref(frame), None if hist is None else C.byref(hist),
                                                  C.byref(outs)))
    return out


def temporal_accumulate_device(width: int, height: int, cur: dict, prev: dict | None, out: dict, cfg: TemporalConfig | None = None,
                               stream: int = 0, clamp: ClampConfig | None = None) -> None:
    """The same on raw device pointers (ints; 0 or a missing key = no such plane): cur with rgb, noise, position, normal, depth,
    mesh; prev (or None) with rgb, noise, length, position, normal, depth, mesh and view = (position[3], matrix[9]) as HOST
    values; out with rgb, noise, length.  out's rgb / noise may be cur's, unless clamp is given (then they are refused: the
    clamped call reads cur's neighbours).  Stream-ordered on the current device, one launch, allocates nothing, never blocks the
    host (rtk.h)."""
    frame = TemporalFrame(*((cur.get(n) or None) for n, _ in TemporalFrame._fields_))
    hist = keep = None
    if prev is not None:
        keep = _view_record(prev["view"]) if prev.get("view") is not None else None
        vals = {n: (prev.get(n) or None) for n, _ in TemporalHistory._fields_ if n != "view"}
        vals["view"] = None if keep is None else keep.ctypes.data
        hist = TemporalHistory(*(vals[n] for n, _ in TemporalHistory._fields_))
    outs = TemporalOutputs(*((out.get(n) or None) for n, _ in TemporalOutputs._fields_))
    p = (cfg or TemporalConfig()).to_c(width, height)
    if clamp is None:
        _check(_L.rtk_temporal_accumulate_device(C.byref(p), C.byref(frame), None if hist is None else C.byref(hist), C.byref(outs),
                                                 stream or None))
    else:
        k = clamp.to_c()
        _check(_L.rtk_temporal_accumulate_clamped_device(C.byref(p), C.byref(k), C.byref(frame), None if hist is None else C.byref(hist),
                                                         C.byref(outs), stream or None))


def format_ppm_rgb8(rgb8: np.ndarray) -> bytes:
    rgb8 = np.ascontiguousarray(rgb8, np.uint8)
    h, w, _ = rgb8.shape
    n = C.c_size_t(0)
    _check(_L.rtk_format_ppm_rgb8(rgb8.ctypes.data, w, h, None, 0, C.byref(n)))
    buf = C.create_string_buffer(n.value)
    _check(_L.rtk_format_ppm_rgb8(rgb8.ctypes.data, w, h, buf, n.value, C.byref(n)))
    return buf.raw[: n.value]


def write_ppm(rgb: np.ndarray, path: str) -> None:
    """write_ppm (io/image/ppm.hpp:7-25)."""
    rgb = np.ascontiguousarray(rgb, np.float32)
    h, w, _ = rgb.shape
    _check(_L.rtk_write_ppm(rgb.ctypes.data, w, h, os.fsencode(path)))
