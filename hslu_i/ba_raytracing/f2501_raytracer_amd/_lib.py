"""Loads librt_hip.so (the HIP path).  There is NO fallback: if the library is missing or a HIP
call fails, this raises -- the product path never routes through a CPU implementation."""
from __future__ import annotations

import ctypes as C
import os

from ._abi import (rt_aux, rt_bvh_info, rt_gather_info, rt_occlusion_batch, rt_occlusion_out, rt_params, rt_point_batch, rt_point_hits, rt_ray_batch, rt_ray_hit_lists, rt_ray_hits, rt_ray_occlusion, rt_ray_order_desc, rt_ray_order_info, rt_ray_radiance, rt_scene_delta, rt_signed_distance_out, rt_solid_batch, rt_solid_out,
                   rt_bvh_quality, rt_pose_desc, rt_rebuild_desc, rt_rebuild_info, rt_rebuild_report, rt_skin_desc, rt_scene_desc, rt_scene_info, rt_stats, rt_update_info, rt_view_adaptive_info, rt_view_camera, rt_view_desc, rt_view_info, rt_view_lens, rt_view_refine)

_HERE = os.path.dirname(os.path.abspath(__file__))
# RT_HIP_LIB selects a diagnostic build of the same library (tools/, A/B timing); default: in-tree
LIB_PATH = os.environ.get("RT_HIP_LIB") or os.path.join(_HERE, "librt_hip.so")
EXPORTS = (
    "rt_device_count", "rt_scene_create", "rt_render", "rt_render_device", "rt_render_collect_stats",
    "rt_scene_destroy", "rt_last_error", "rt_scene_bvh_info", "rt_scene_memory_info", "rt_build_id", "rt_selftest_exact_math",
    "rt_gather_layout", "rt_render_multi", "rt_render_multi_begin", "rt_render_multi_end", "rt_multi_release", "rt_comm_unique_id", "rt_comm_create", "rt_comm_destroy",
    "rt_render_gather_device", "rt_comm_last_gather", "rt_render_begin", "rt_render_poll", "rt_render_end",
    "rt_cast_rays", "rt_cast_rays_device", "rt_any_intersection", "rt_any_intersection_device",
    "rt_closest_points", "rt_closest_points_device", "rt_closest_points_model",
    "rt_list_intersections", "rt_list_intersections_device", "rt_list_intersections_model",
    "rt_ambient_occlusion", "rt_ambient_occlusion_device", "rt_ambient_occlusion_model", "rt_occlusion_rays_model",
    "rt_contains_points", "rt_contains_points_device", "rt_contains_points_model",
    "rt_signed_distance", "rt_signed_distance_device", "rt_signed_distance_model",
    "rt_trace_rays", "rt_trace_rays_device", "rt_scene_update", "rt_scene_update_device",
    "rt_ray_order_create", "rt_ray_order_destroy", "rt_ray_order_build", "rt_ray_order_build_device", "rt_ray_order_set", "rt_ray_order_read",
    "rt_trace_rays_ordered", "rt_trace_rays_ordered_device",
    "rt_view_create", "rt_view_destroy", "rt_view_set_camera", "rt_view_rays_device", "rt_view_rays", "rt_render_view_device", "rt_render_view",
    "rt_view_read", "rt_view_rays_model", "rt_view_resolve_model",
    "rt_view_enable_adaptive", "rt_render_view_adaptive_device", "rt_render_view_adaptive", "rt_view_adaptive_read", "rt_view_refine_model",
    "rt_view_resolve_adaptive_model",
    "rt_view_create_lens", "rt_view_set_lens", "rt_view_lens_rays_model", "rt_view_defocus_model",
    "rt_pose_create", "rt_pose_destroy", "rt_pose_geometry_device", "rt_pose_apply_device", "rt_pose_apply", "rt_pose_read", "rt_pose_model",
    "rt_skin_create", "rt_skin_destroy", "rt_skin_geometry_device", "rt_skin_apply_device", "rt_skin_apply", "rt_skin_read", "rt_skin_model",
    "rt_scene_bvh_quality", "rt_scene_rebuild", "rt_scene_rebuild_device", "rt_scene_rebuild_with", "rt_scene_rebuild_with_device",
)

_lib = None


class RtError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"rt_hip error {code}: {msg}")
        self.code = code


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
            "or `make -C hslu_i/ba_raytracing/f2501_raytracer_amd/csrc`).  There is no CPU fallback."
        )
    lib = C.CDLL(LIB_PATH)
    lib.rt_device_count.restype = C.c_int
    lib.rt_scene_create.restype = C.c_int
    lib.rt_scene_create.argtypes = [C.POINTER(rt_scene_desc), C.c_int, C.POINTER(C.c_void_p)]
    lib.rt_render.restype = C.c_int
    lib.rt_render.argtypes = [C.c_void_p, C.POINTER(rt_params), C.c_void_p, C.POINTER(rt_aux), C.POINTER(rt_stats)]
    lib.rt_render_device.restype = C.c_int
    lib.rt_render_device.argtypes = [C.c_void_p, C.POINTER(rt_params), C.c_void_p, C.POINTER(rt_aux), C.c_void_p]
    lib.rt_render_collect_stats.restype = C.c_int
    lib.rt_render_collect_stats.argtypes = [C.c_void_p, C.POINTER(rt_stats)]
    lib.rt_scene_destroy.restype = None
    lib.rt_scene_destroy.argtypes = [C.c_void_p]
    lib.rt_last_error.restype = C.c_char_p
    lib.rt_build_id.restype = C.c_char_p
    lib.rt_selftest_exact_math.restype = C.c_int
    lib.rt_selftest_exact_math.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    lib.rt_scene_bvh_info.restype = C.c_int
    lib.rt_scene_bvh_info.argtypes = [C.c_void_p, C.POINTER(rt_bvh_info)]
    lib.rt_render_begin.restype = C.c_int
    lib.rt_render_begin.argtypes = [C.c_void_p, C.POINTER(rt_params), C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
    lib.rt_render_poll.restype = C.c_int
    lib.rt_render_poll.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
    lib.rt_render_end.restype = C.c_int
    lib.rt_render_end.argtypes = [C.c_void_p, C.POINTER(rt_stats)]
    lib.rt_scene_memory_info.restype = C.c_int
    lib.rt_scene_memory_info.argtypes = [C.c_void_p, C.POINTER(rt_scene_info)]
    u32p = C.POINTER(C.c_uint32)
    lib.rt_gather_layout.restype = C.c_int
    lib.rt_gather_layout.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u32p, u32p]
    lib.rt_render_multi.restype = C.c_int
    lib.rt_render_multi.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(rt_params), C.c_void_p, C.POINTER(rt_stats)]
    lib.rt_render_multi_begin.restype = C.c_int
    lib.rt_render_multi_begin.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(rt_params), C.c_void_p, C.POINTER(C.c_int)]
    lib.rt_render_multi_end.restype = C.c_int
    lib.rt_render_multi_end.argtypes = [C.c_int, C.POINTER(rt_stats)]
    lib.rt_multi_release.restype = None
    lib.rt_comm_unique_id.restype = C.c_int
    lib.rt_comm_unique_id.argtypes = [C.c_void_p]
    lib.rt_comm_create.restype = C.c_int
    lib.rt_comm_create.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
    lib.rt_comm_destroy.restype = None
    lib.rt_comm_destroy.argtypes = [C.c_void_p]
    lib.rt_render_gather_device.restype = C.c_int
    lib.rt_render_gather_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(rt_params), C.c_void_p, C.c_void_p]
    lib.rt_comm_last_gather.restype = C.c_int
    lib.rt_comm_last_gather.argtypes = [C.c_void_p, C.POINTER(rt_gather_info)]
    for name, out in (("rt_cast_rays", rt_ray_hits), ("rt_any_intersection", rt_ray_occlusion)):
        getattr(lib, name).restype = C.c_int
        getattr(lib, name).argtypes = [C.c_void_p, C.POINTER(rt_ray_batch), C.POINTER(out)]
        getattr(lib, name + "_device").restype = C.c_int
        getattr(lib, name + "_device").argtypes = [C.c_void_p, C.POINTER(rt_ray_batch), C.POINTER(out), C.c_void_p]
    lib.rt_list_intersections.restype = C.c_int
    lib.rt_list_intersections.argtypes = [C.c_void_p, C.POINTER(rt_ray_batch), C.POINTER(rt_ray_hit_lists)]
    lib.rt_list_intersections_device.restype = C.c_int
    lib.rt_list_intersections_device.argtypes = [C.c_void_p, C.POINTER(rt_ray_batch), C.POINTER(rt_ray_hit_lists), C.c_void_p]
    lib.rt_list_intersections_model.restype = C.c_int
    lib.rt_list_intersections_model.argtypes = [C.POINTER(rt_scene_desc), C.POINTER(rt_ray_batch), C.POINTER(rt_ray_hit_lists)]
    lib.rt_ambient_occlusion.restype = C.c_int
    lib.rt_ambient_occlusion.argtypes = [C.c_void_p, C.POINTER(rt_occlusion_batch), C.POINTER(rt_occlusion_out)]
    lib.rt_ambient_occlusion_device.restype = C.c_int
    lib.rt_ambient_occlusion_device.argtypes = [C.c_void_p, C.POINTER(rt_occlusion_batch), C.POINTER(rt_occlusion_out), C.c_void_p]
    lib.rt_ambient_occlusion_model.restype = C.c_int
    lib.rt_ambient_occlusion_model.argtypes = [C.POINTER(rt_scene_desc), C.POINTER(rt_occlusion_batch), C.POINTER(rt_occlusion_out)]
    lib.rt_occlusion_rays_model.restype = C.c_int
    lib.rt_occlusion_rays_model.argtypes = [C.POINTER(rt_occlusion_batch), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rt_closest_points.restype = C.c_int
    lib.rt_closest_points.argtypes = [C.c_void_p, C.POINTER(rt_point_batch), C.POINTER(rt_point_hits)]
    lib.rt_closest_points_device.restype = C.c_int
    lib.rt_closest_points_device.argtypes = [C.c_void_p, C.POINTER(rt_point_batch), C.POINTER(rt_point_hits), C.c_void_p]
    lib.rt_closest_points_model.restype = C.c_int
    lib.rt_closest_points_model.argtypes = [C.POINTER(rt_scene_desc), C.POINTER(rt_point_batch), C.POINTER(rt_point_hits)]
    for name, out in (("rt_contains_points", rt_solid_out), ("rt_signed_distance", rt_signed_distance_out)):
        getattr(lib, name).restype = C.c_int
        getattr(lib, name).argtypes = [C.c_void_p, C.POINTER(rt_solid_batch), C.POINTER(out)]
        getattr(lib, name + "_device").restype = C.c_int
        getattr(lib, name + "_device").argtypes = [C.c_void_p, C.POINTER(rt_solid_batch), C.POINTER(out), C.c_void_p]
        getattr(lib, name + "_model").restype = C.c_int
        getattr(lib, name + "_model").argtypes = [C.POINTER(rt_scene_desc), C.POINTER(rt_solid_batch), C.POINTER(out)]
    lib.rt_trace_rays.restype = C.c_int
    lib.rt_trace_rays.argtypes = [C.c_void_p, C.POINTER(rt_params), C.POINTER(rt_ray_batch), C.POINTER(rt_ray_radiance), C.POINTER(rt_stats)]
    lib.rt_trace_rays_device.restype = C.c_int
    lib.rt_trace_rays_device.argtypes = [C.c_void_p, C.POINTER(rt_params), C.POINTER(rt_ray_batch), C.POINTER(rt_ray_radiance), C.c_void_p]
    lib.rt_scene_update.restype = C.c_int
    lib.rt_scene_update.argtypes = [C.c_void_p, C.POINTER(rt_scene_delta), C.POINTER(rt_update_info)]
    lib.rt_scene_update_device.restype = C.c_int
    lib.rt_scene_update_device.argtypes = [C.c_void_p, C.POINTER(rt_scene_delta), C.c_void_p, C.POINTER(rt_update_info)]
    lib.rt_ray_order_create.restype = C.c_int
    lib.rt_ray_order_create.argtypes = [C.POINTER(rt_ray_order_desc), C.c_int, C.POINTER(C.c_void_p)]
    lib.rt_ray_order_destroy.restype = None
    lib.rt_ray_order_destroy.argtypes = [C.c_void_p]
    lib.rt_ray_order_build.restype = C.c_int
    lib.rt_ray_order_build.argtypes = [C.c_void_p, C.POINTER(rt_ray_batch)]
    lib.rt_ray_order_build_device.restype = C.c_int
    lib.rt_ray_order_build_device.argtypes = [C.c_void_p, C.POINTER(rt_ray_batch), C.c_void_p]
    lib.rt_ray_order_set.restype = C.c_int
    lib.rt_ray_order_set.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    lib.rt_ray_order_read.restype = C.c_int
    lib.rt_ray_order_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(rt_ray_order_info)]
    lib.rt_trace_rays_ordered.restype = C.c_int
    lib.rt_trace_rays_ordered.argtypes = [C.c_void_p, C.POINTER(rt_params), C.POINTER(rt_ray_batch), C.c_void_p, C.POINTER(rt_ray_radiance),
                                          C.POINTER(rt_stats)]
    lib.rt_trace_rays_ordered_device.restype = C.c_int
    lib.rt_trace_rays_ordered_device.argtypes = [C.c_void_p, C.POINTER(rt_params), C.POINTER(rt_ray_batch), C.c_void_p, C.POINTER(rt_ray_radiance),
                                                 C.c_void_p]
    lib.rt_view_create.restype = C.c_int
    lib.rt_view_create.argtypes = [C.POINTER(rt_view_desc), C.c_int, C.POINTER(C.c_void_p)]
    lib.rt_view_destroy.restype = None
    lib.rt_view_destroy.argtypes = [C.c_void_p]
    lib.rt_view_set_camera.restype = C.c_int
    lib.rt_view_set_camera.argtypes = [C.c_void_p, C.POINTER(rt_view_camera)]
    lib.rt_view_rays_device.restype = C.c_int
    lib.rt_view_rays_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rt_view_rays.restype = C.c_int
    lib.rt_view_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rt_render_view_device.restype = C.c_int
    lib.rt_render_view_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(rt_params), C.POINTER(rt_ray_radiance), C.c_void_p]
    lib.rt_render_view.restype = C.c_int
    lib.rt_render_view.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(rt_params), C.POINTER(rt_ray_radiance), C.POINTER(rt_stats)]
    lib.rt_view_read.restype = C.c_int
    lib.rt_view_read.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(rt_view_info)]
    lib.rt_view_rays_model.restype = C.c_int
    lib.rt_view_rays_model.argtypes = [C.POINTER(rt_view_desc), C.POINTER(rt_view_camera), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    lib.rt_view_resolve_model.restype = C.c_int
    lib.rt_view_resolve_model.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(rt_ray_radiance), C.POINTER(rt_ray_radiance)]
    lib.rt_view_enable_adaptive.restype = C.c_int
    lib.rt_view_enable_adaptive.argtypes = [C.c_void_p]
    lib.rt_render_view_adaptive_device.restype = C.c_int
    lib.rt_render_view_adaptive_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(rt_params), C.POINTER(rt_view_refine), C.POINTER(rt_ray_radiance),
                                                   C.c_void_p, C.c_void_p]
    lib.rt_render_view_adaptive.restype = C.c_int
    lib.rt_render_view_adaptive.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(rt_params), C.POINTER(rt_view_refine), C.POINTER(rt_ray_radiance),
                                            C.c_void_p, C.POINTER(rt_stats)]
    lib.rt_view_adaptive_read.restype = C.c_int
    lib.rt_view_adaptive_read.argtypes = [C.c_void_p, C.POINTER(rt_view_adaptive_info)]
    lib.rt_view_refine_model.restype = C.c_int
    lib.rt_view_refine_model.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(rt_view_refine), C.POINTER(rt_ray_radiance), C.c_void_p, C.POINTER(C.c_uint32)]
    lib.rt_view_resolve_adaptive_model.restype = C.c_int
    lib.rt_view_resolve_adaptive_model.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(rt_ray_radiance), C.POINTER(rt_ray_radiance),
                                                   C.POINTER(rt_ray_radiance)]
    lib.rt_view_create_lens.restype = C.c_int
    lib.rt_view_create_lens.argtypes = [C.POINTER(rt_view_desc), C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    lib.rt_view_set_lens.restype = C.c_int
    lib.rt_view_set_lens.argtypes = [C.c_void_p, C.POINTER(rt_view_lens)]
    lib.rt_view_lens_rays_model.restype = C.c_int
    lib.rt_view_lens_rays_model.argtypes = [C.POINTER(rt_view_desc), C.c_void_p, C.POINTER(rt_view_camera), C.POINTER(rt_view_lens), C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.POINTER(C.c_uint32)]
    lib.rt_view_defocus_model.restype = C.c_int
    lib.rt_view_defocus_model.argtypes = [C.POINTER(rt_view_desc), C.POINTER(rt_view_camera), C.POINTER(rt_view_lens), C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.POINTER(C.c_uint32)]
    lib.rt_pose_create.restype = C.c_int
    lib.rt_pose_create.argtypes = [C.POINTER(rt_pose_desc), C.c_int, C.POINTER(C.c_void_p)]
    lib.rt_pose_destroy.restype = None
    lib.rt_pose_destroy.argtypes = [C.c_void_p]
    lib.rt_pose_geometry_device.restype = C.c_int
    lib.rt_pose_geometry_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rt_pose_apply_device.restype = C.c_int
    lib.rt_pose_apply_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(rt_update_info)]
    lib.rt_pose_apply.restype = C.c_int
    lib.rt_pose_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(rt_update_info)]
    lib.rt_pose_read.restype = C.c_int
    lib.rt_pose_read.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.POINTER(C.c_uint32)] * 2 + [C.c_void_p] * 3
    lib.rt_pose_model.restype = C.c_int
    lib.rt_pose_model.argtypes = [C.POINTER(rt_pose_desc), C.c_void_p] + [C.c_void_p] * 7
    lib.rt_skin_create.restype = C.c_int
    lib.rt_skin_create.argtypes = [C.POINTER(rt_skin_desc), C.c_int, C.POINTER(C.c_void_p)]
    lib.rt_skin_destroy.restype = None
    lib.rt_skin_destroy.argtypes = [C.c_void_p]
    lib.rt_skin_geometry_device.restype = C.c_int
    lib.rt_skin_geometry_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rt_skin_apply_device.restype = C.c_int
    lib.rt_skin_apply_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(rt_update_info)]
    lib.rt_skin_apply.restype = C.c_int
    lib.rt_skin_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(rt_update_info)]
    lib.rt_skin_read.restype = C.c_int
    lib.rt_skin_read.argtypes = [C.c_void_p] + [C.c_void_p] * 6
    lib.rt_skin_model.restype = C.c_int
    lib.rt_skin_model.argtypes = [C.POINTER(rt_skin_desc), C.c_void_p] + [C.c_void_p] * 6
    lib.rt_scene_bvh_quality.restype = C.c_int
    lib.rt_scene_bvh_quality.argtypes = [C.c_void_p, C.POINTER(rt_bvh_quality)]
    lib.rt_scene_rebuild.restype = C.c_int
    lib.rt_scene_rebuild.argtypes = [C.c_void_p, C.POINTER(rt_rebuild_info)]
    lib.rt_scene_rebuild_device.restype = C.c_int
    lib.rt_scene_rebuild_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(rt_rebuild_info)]
    lib.rt_scene_rebuild_with.restype = C.c_int
    lib.rt_scene_rebuild_with.argtypes = [C.c_void_p, C.POINTER(rt_rebuild_desc), C.POINTER(rt_rebuild_report)]
    lib.rt_scene_rebuild_with_device.restype = C.c_int
    lib.rt_scene_rebuild_with_device.argtypes = [C.c_void_p, C.POINTER(rt_rebuild_desc), C.c_void_p, C.POINTER(rt_rebuild_report)]
    _lib = lib
    return lib


def check(rc: int):
    if rc != 0:
        raise RtError(rc, load().rt_last_error().decode("utf-8", "replace"))
