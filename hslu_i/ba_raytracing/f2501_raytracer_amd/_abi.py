"""ctypes mirror of include/rt_hip.h (structures only; no library is loaded here)."""
from __future__ import annotations

import ctypes as C

import numpy as np

RT_ABI_VERSION = 4
RT_OK = 0
RT_ERR_INVALID_ARG, RT_ERR_NO_DEVICE, RT_ERR_HIP, RT_ERR_OOM, RT_ERR_UNSUPPORTED = -1, -2, -3, -4, -5
RT_FLAG_REFLECTIONS, RT_FLAG_REFRACTIONS, RT_FLAG_BACKFACE_CULLING, RT_FLAG_ANTI_ALIASING = 1, 2, 4, 8
RT_TRAVERSAL_BVH, RT_TRAVERSAL_LINEAR = 0, 1
RT_CAND_CAP_NONE = 0xFFFFFFFF
RT_TILE_ORDER_DEFAULT, RT_TILE_ORDER_ROW_MAJOR, RT_TILE_ORDER_COST = 0, 1, 2
RT_PHASES_DEFAULT, RT_PHASES_FUSED, RT_PHASES_SPLIT, RT_PHASES_FUSED_DEFER = 0, 1, 2, 3
RT_LEVELS_DEFAULT, RT_LEVELS_CHAINED, RT_LEVELS_MERGED, RT_LEVELS_PIPELINED = 0, 1, 2, 3
(RT_NOTE_RECV_FLAGS_OFF_LIGHTS, RT_NOTE_RECV_FLAGS_OFF_CULLING, RT_NOTE_RECV_FLAGS_OFF_TRAVERSAL, RT_NOTE_RECV_FLAGS_OFF_TUNING,
 RT_NOTE_RECV_FLAGS_OFF_SCENE, RT_NOTE_HARD_PAIRS_OFF, RT_NOTE_FRAME_BATCHED, RT_NOTE_CELL_LISTS_OFF, RT_NOTE_TILE_ORDER_COST_OFF,
 RT_NOTE_FRAME_DROPPED_WORK) = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512
RT_SCENE_BUDGET_DEFAULT = 128 << 20

_fp = C.POINTER(C.c_float)
_up = C.POINTER(C.c_uint32)
_ip = C.POINTER(C.c_int32)


class rt_bvh_tuning(C.Structure):
    _fields_ = [("max_leaf", C.c_uint32), ("tri_cost", C.c_float), ("split_depth", C.c_uint32), ("split_gain", C.c_float)]


class rt_tuning(C.Structure):
    _fields_ = [("shadow_candidate_cap", C.c_uint32), ("chunk_log2", C.c_uint32), ("no_aa_dedup", C.c_uint32),
                ("no_counters", C.c_uint32), ("multi_force_rccl", C.c_uint32), ("no_receiver_flags", C.c_uint32),
                ("tile_order", C.c_uint32), ("sort_bits", C.c_uint32), ("no_cell_lists", C.c_uint32),
                ("sub_frames", C.c_uint32), ("phases", C.c_uint32), ("levels", C.c_uint32)]


class rt_scene_desc(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("n_spheres", C.c_uint32), ("sphere_center", _fp), ("sphere_r_sq", _fp), ("sphere_r_inv", _fp),
        ("sphere_material", _up),
        ("n_triangles", C.c_uint32), ("tri_v1", _fp), ("tri_e1", _fp), ("tri_e2", _fp), ("tri_normal", _fp),
        ("tri_material", _up),
        ("n_materials", C.c_uint32), ("materials", _fp),
        ("n_lights", C.c_uint32), ("lights", _fp),
        ("bvh", rt_bvh_tuning),
        ("device_budget_bytes", C.c_uint64),
    ]


class rt_params(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
        ("focus", C.c_float * 3), ("fw", C.c_float), ("fh", C.c_float), ("fd", C.c_float),
        ("eps_distance", C.c_float), ("air_ior", C.c_float), ("ambient", C.c_float),
        ("flags", C.c_uint32),
        ("aa_rays", C.c_uint32), ("aa_offsets", _fp),
        ("light_mult", C.c_uint32), ("cloud_seed", C.c_uint32), ("n_cloud_sets", C.c_uint32), ("cloud_sets", _fp),
        ("max_depth_reflection", C.c_uint32), ("max_depth_refraction", C.c_uint32),
        ("win_x0", C.c_uint32), ("win_y0", C.c_uint32), ("win_w", C.c_uint32), ("win_h", C.c_uint32),
        ("tile_size", C.c_uint32), ("n_ranks", C.c_uint32), ("rank", C.c_uint32),
        ("traversal", C.c_uint32),
        ("tuning", rt_tuning),
    ]


class rt_aux(C.Structure):
    _fields_ = [("rgb", C.c_void_p), ("hit_id", C.c_void_p), ("hit_t", C.c_void_p)]


class rt_stats(C.Structure):
    _fields_ = [
        ("rays_primary", C.c_uint64), ("rays_reflection", C.c_uint64), ("rays_refraction", C.c_uint64),
        ("rays_shadow", C.c_uint64), ("pixels_written", C.c_uint64), ("rays_traced", C.c_uint64),
        ("kernel_ms", C.c_double), ("total_ms", C.c_double), ("d2h_ms", C.c_double), ("gather_ms", C.c_double),
        ("wave_ray_passes", C.c_uint64), ("wave_ray_lanes", C.c_uint64),
        ("wave_nearest_nodes", C.c_uint64), ("wave_nearest_tris", C.c_uint64),
        ("wave_shadow_nodes", C.c_uint64), ("wave_shadow_tris", C.c_uint64), ("wave_shadow_passes", C.c_uint64),
        ("wave_nearest_tris_exact", C.c_uint64), ("wave_shadow_tris_exact", C.c_uint64),
        ("notes", C.c_uint32), ("reserved0", C.c_uint32), ("queue_bytes", C.c_uint64),
        ("setup_ms", C.c_double), ("scene_bytes", C.c_uint64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class rt_gather_info(C.Structure):
    _fields_ = [
        ("render_ms", C.c_double), ("gather_ms", C.c_double), ("bytes_sent", C.c_uint64), ("bytes_received", C.c_uint64),
        ("n_ranks", C.c_uint32), ("rank", C.c_uint32), ("tiles_owned", C.c_uint32), ("transport", C.c_uint32),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


RT_COMM_ID_BYTES = 128
RT_TRANSPORT_NONE, RT_TRANSPORT_RCCL, RT_TRANSPORT_LOCAL = 0, 1, 2


class rt_bvh_info(C.Structure):
    _fields_ = [
        ("n_nodes", C.c_uint32), ("n_leaves", C.c_uint32), ("max_depth", C.c_uint32), ("max_leaf_size", C.c_uint32),
        ("bytes_nodes", C.c_uint64), ("bytes_triangles", C.c_uint64), ("n_references", C.c_uint32),
    ]


class rt_scene_info(C.Structure):
    _fields_ = [
        ("bytes_geometry", C.c_uint64), ("bytes_bvh", C.c_uint64), ("bytes_flags", C.c_uint64), ("bytes_cell_lists", C.c_uint64),
        ("bytes_tables", C.c_uint64), ("bytes_workspace", C.c_uint64), ("bytes_frames", C.c_uint64), ("bytes_total", C.c_uint64),
        ("budget_bytes", C.c_uint64), ("n_receiver_cells", C.c_uint32), ("cell_lists_built", C.c_uint32),
    ]


class rt_ray_batch(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("n_rays", C.c_uint32), ("origin", C.c_void_p), ("direction", C.c_void_p),
                ("max_distance", C.c_void_p), ("flags", C.c_uint32)]


class rt_ray_hits(C.Structure):
    _fields_ = [("id", C.c_void_p), ("t", C.c_void_p), ("point", C.c_void_p), ("normal", C.c_void_p), ("material", C.c_void_p)]


class rt_ray_occlusion(C.Structure):
    _fields_ = [("has_intersection", C.c_void_p), ("completely_occluded", C.c_void_p), ("combined_opacity", C.c_void_p),
                ("color_filter", C.c_void_p)]


class rt_point_batch(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("n_points", C.c_uint32), ("point", C.c_void_p), ("max_distance", C.c_void_p)]


class rt_point_hits(C.Structure):
    _fields_ = [("id", C.c_void_p), ("distance", C.c_void_p), ("point", C.c_void_p), ("normal", C.c_void_p), ("bary", C.c_void_p),
                ("material", C.c_void_p)]


RT_MAX_HITS_PER_RAY = 16


class rt_ray_hit_lists(C.Structure):
    _fields_ = [("max_hits", C.c_uint32), ("after_t", C.c_void_p), ("after_id", C.c_void_p), ("count", C.c_void_p), ("total", C.c_void_p),
                ("id", C.c_void_p), ("t", C.c_void_p), ("point", C.c_void_p), ("normal", C.c_void_p), ("material", C.c_void_p)]


RT_MAX_OCCLUSION_SAMPLES = 256
RT_OCCLUSION_PASS_TRANSMISSIVE = 0x1


class rt_occlusion_batch(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("n_points", C.c_uint32), ("point", C.c_void_p), ("normal", C.c_void_p), ("n_samples", C.c_uint32),
                ("n_table", C.c_uint32), ("table", C.c_void_p), ("first", C.c_void_p), ("bias", C.c_float), ("max_distance", C.c_float),
                ("flags", C.c_uint32)]


class rt_occlusion_out(C.Structure):
    _fields_ = [("bits", C.c_void_p), ("clear", C.c_void_p), ("visibility", C.c_void_p), ("bent_normal", C.c_void_p)]


RT_MAX_SOLID_DIRECTIONS = 8
RT_SOLID_RULE_PARITY, RT_SOLID_RULE_WINDING = 0, 1


class rt_solid_batch(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("n_points", C.c_uint32), ("point", C.c_void_p), ("max_distance", C.c_void_p),
                ("n_directions", C.c_uint32), ("rule", C.c_uint32), ("directions", C.c_void_p)]


class rt_solid_out(C.Structure):
    _fields_ = [("inside", C.c_void_p), ("votes", C.c_void_p), ("crossings", C.c_void_p), ("winding", C.c_void_p)]


class rt_signed_distance_out(C.Structure):
    _fields_ = [("signed_distance", C.c_void_p), ("solid", rt_solid_out), ("closest", rt_point_hits)]


class rt_ray_radiance(C.Structure):
    _fields_ = [("rgb", C.c_void_p), ("valid", C.c_void_p), ("id", C.c_void_p), ("t", C.c_void_p), ("argb", C.c_void_p)]


class rt_scene_delta(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("sphere_center", C.c_void_p), ("sphere_r_sq", C.c_void_p), ("sphere_r_inv", C.c_void_p),
        ("tri_first", C.c_uint32), ("tri_count", C.c_uint32),
        ("tri_v1", C.c_void_p), ("tri_e1", C.c_void_p), ("tri_e2", C.c_void_p), ("tri_normal", C.c_void_p),
        ("materials", C.c_void_p), ("lights", C.c_void_p),
    ]


class rt_ray_order_desc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("capacity", C.c_uint32), ("origin_bits", C.c_uint32), ("reserved", C.c_uint32)]


class rt_ray_order_info(C.Structure):
    _fields_ = [
        ("n_rays", C.c_uint32), ("n_live", C.c_uint32), ("origin_bits", C.c_uint32), ("direction_bits", C.c_uint32),
        ("n_origin_axes", C.c_uint32), ("n_direction_axes", C.c_uint32), ("bytes", C.c_uint64), ("device_ms", C.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


RT_VIEW_PINHOLE, RT_VIEW_REFERENCE = 0, 1
RT_VIEW_ORDER_ONCE, RT_VIEW_ORDER_ALWAYS, RT_VIEW_ORDER_NONE = 0, 1, 2
RT_VIEW_MAX_SAMPLES = 64


class rt_view_desc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("n_samples", C.c_uint32),
                ("samples", C.c_void_p), ("order", C.c_uint32)]


class rt_view_camera(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("kind", C.c_uint32), ("eye", C.c_float * 3), ("right", C.c_float * 3),
                ("up", C.c_float * 3), ("forward", C.c_float * 3), ("tan_half_fov_y", C.c_float), ("focus", C.c_float * 3),
                ("fw", C.c_float), ("fh", C.c_float)]


class rt_view_info(C.Structure):
    _fields_ = [("n_pixels", C.c_uint32), ("n_samples", C.c_uint32), ("n_distinct", C.c_uint32), ("n_rays", C.c_uint32),
                ("bytes", C.c_uint64), ("order_built", C.c_uint32), ("reserved", C.c_uint32),
                ("rays_ms", C.c_double), ("order_ms", C.c_double), ("resolve_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


RT_REFINE_ID, RT_REFINE_DEPTH, RT_REFINE_COLOUR, RT_REFINE_EVERY = 1, 2, 4, 8


class rt_view_refine(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("criteria", C.c_uint32), ("colour_tol", C.c_float), ("depth_tol", C.c_float)]


class rt_view_adaptive_info(C.Structure):
    _fields_ = [("n_refined", C.c_uint32), ("n_live_rays", C.c_uint32), ("bytes", C.c_uint64), ("pass1_ms", C.c_double),
                ("classify_ms", C.c_double), ("partition_ms", C.c_double), ("pass2_ms", C.c_double), ("resolve_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


RT_VIEW_LENS_MAX_SPREAD = 16


class rt_view_lens(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("spread", C.c_uint32), ("aperture", C.c_float), ("focus_distance", C.c_float),
                ("coc_tol", C.c_float), ("reserved", C.c_uint32)]


RT_UPDATE_INVALIDATES_RECEIVER_TABLES, RT_UPDATE_INVALIDATES_TILE_COSTS, RT_UPDATE_INVALIDATES_QUEUE_SIZES = 1, 2, 4


class rt_update_info(C.Structure):
    _fields_ = [
        ("device_ms", C.c_double), ("total_ms", C.c_double),
        ("nodes_refitted", C.c_uint32), ("slots_rewritten", C.c_uint32), ("receivers_disabled", C.c_uint32),
        ("tables_invalidated", C.c_uint32),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class rt_transform(C.Structure):
    _fields_ = [("translation", C.c_float * 3), ("rotor", C.c_float * 4), ("scale", C.c_float)]


class rt_pose_part(C.Structure):
    _fields_ = [("tri_first", C.c_uint32), ("tri_count", C.c_uint32), ("sphere_first", C.c_uint32), ("sphere_count", C.c_uint32)]


class rt_pose_desc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("n_parts", C.c_uint32), ("parts", C.c_void_p), ("n_triangles", C.c_uint32),
                ("n_spheres", C.c_uint32), ("tri_v1", C.c_void_p), ("tri_v2", C.c_void_p), ("tri_v3", C.c_void_p),
                ("tri_normal", C.c_void_p), ("sphere_center", C.c_void_p), ("sphere_radius", C.c_void_p)]


class rt_skin_desc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("n_vertices", C.c_uint32), ("n_bones", C.c_uint32), ("tri_first", C.c_uint32),
                ("tri_count", C.c_uint32), ("n_triangles", C.c_uint32), ("position", C.c_void_p), ("normal", C.c_void_p),
                ("indices", C.c_void_p), ("bone", C.c_void_p), ("weight", C.c_void_p)]


class rt_bvh_quality(C.Structure):
    _fields_ = [("sah_created", C.c_double), ("sah_now", C.c_double), ("inner_q", C.c_uint64), ("leaf_q", C.c_uint64),
                ("n_bad", C.c_uint32), ("reserved", C.c_uint32), ("device_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class rt_rebuild_info(C.Structure):
    _fields_ = [("device_ms", C.c_double), ("total_ms", C.c_double), ("n_nodes", C.c_uint32), ("n_leaves", C.c_uint32),
                ("max_depth", C.c_uint32), ("max_leaf_size", C.c_uint32), ("tables_invalidated", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


RT_REBUILD_LBVH, RT_REBUILD_PLOC = 0, 1
RT_REBUILD_KEEP_BETTER = 0x1


class rt_rebuild_desc(C.Structure):
    _fields_ = [("method", C.c_uint32), ("radius", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class rt_rebuild_report(C.Structure):
    _fields_ = [("info", rt_rebuild_info), ("inner_q_before", C.c_uint64), ("leaf_q_before", C.c_uint64), ("inner_q_after", C.c_uint64),
                ("leaf_q_after", C.c_uint64), ("sah_before", C.c_double), ("sah_after", C.c_double), ("swapped", C.c_uint32),
                ("iterations", C.c_uint32)]

    def as_dict(self):
        """the fields of `info` and the report's own, flat"""
        out = self.info.as_dict()
        out.update({k: getattr(self, k) for k, _ in self._fields_ if k != "info"})
        return out


def transform_row(t):
    """Similarity3 -> the 8 floats of an rt_transform: translation, rotor s / xy / xz / yz, scale"""
    r = t.rotation
    return [np.float32(v) for v in (t.translation.x, t.translation.y, t.translation.z, r.s, r.xy, r.xz, r.yz, t.scale)]


def transform_rows(transforms):
    """a list of Similarity3, or anything numpy turns into (n, 8) floats -> contiguous (n, 8) float32"""
    if isinstance(transforms, (list, tuple)) and transforms and hasattr(transforms[0], "rotation"):
        transforms = [transform_row(t) for t in transforms]
    a = np.ascontiguousarray(transforms, np.float32)
    if a.ndim != 2 or a.shape[1] != 8:
        raise ValueError(f"transforms must be (n_parts, 8), got {a.shape}")
    return a


def make_pose_desc(parts, n_triangles, n_spheres, v1=None, v2=None, v3=None, normal=None, centre=None, radius=None):
    """rt_pose_desc of `parts` [(tri_first, tri_count, sphere_first, sphere_count)] over rest arrays (float32 numpy, or None).
    Returns (desc, keepalive)."""
    pa = np.ascontiguousarray(parts, np.uint32).reshape(-1, 4)
    keep = [pa]
    d = rt_pose_desc()
    d.abi_version, d.n_parts, d.parts = RT_ABI_VERSION, int(pa.shape[0]), pa.ctypes.data
    d.n_triangles, d.n_spheres = int(n_triangles), int(n_spheres)
    for field, a in (("tri_v1", v1), ("tri_v2", v2), ("tri_v3", v3), ("tri_normal", normal), ("sphere_center", centre), ("sphere_radius", radius)):
        if a is not None:
            a = np.ascontiguousarray(a, np.float32)
            keep.append(a)
            setattr(d, field, a.ctypes.data)
    return d, keep


def make_skin_desc(position, normal, indices, bone, weight, n_bones, tri_first, n_triangles):
    """rt_skin_desc of an indexed mesh: position (V, 3) float32, normal (V, 3) float32 or None, indices (T, 3) uint32, bone
    (V, 4) uint16, weight (V, 4) float32; the mesh is canonical triangles [tri_first, tri_first + T) of a scene of
    n_triangles.  Returns (desc, keepalive)."""
    pos = np.ascontiguousarray(position, np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(indices, np.uint32).reshape(-1, 3)
    b = np.ascontiguousarray(bone, np.uint16).reshape(-1, 4)
    w = np.ascontiguousarray(weight, np.float32).reshape(-1, 4)
    keep = [pos, idx, b, w]
    if b.shape[0] != pos.shape[0] or w.shape[0] != pos.shape[0]:
        raise ValueError(f"bone {b.shape} and weight {w.shape} must be (n_vertices, 4) for {pos.shape[0]} vertices")
    d = rt_skin_desc()
    d.abi_version, d.n_vertices, d.n_bones = RT_ABI_VERSION, int(pos.shape[0]), int(n_bones)
    d.tri_first, d.tri_count, d.n_triangles = int(tri_first), int(idx.shape[0]), int(n_triangles)
    d.position, d.indices, d.bone, d.weight = pos.ctypes.data, idx.ctypes.data, b.ctypes.data, w.ctypes.data
    if normal is not None:
        nrm = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
        if nrm.shape != pos.shape:
            raise ValueError(f"normal {nrm.shape} must match position {pos.shape}")
        keep.append(nrm)
        d.normal = nrm.ctypes.data
    return d, keep


def fptr(a: np.ndarray):
    assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_fp)


def uptr(a: np.ndarray):
    assert a.dtype == np.uint32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_up)


def make_scene_desc(flat, bvh=None, budget=0):
    """flat: FlatScene (contiguous); bvh: dict of rt_bvh_tuning fields; budget: rt_scene_desc.device_budget_bytes (0 = default).
    Returns (desc, keepalive)."""
    f = flat.contiguous()
    d = rt_scene_desc()
    d.abi_version = RT_ABI_VERSION
    d.n_spheres = f.n_spheres
    d.sphere_center, d.sphere_r_sq, d.sphere_r_inv = fptr(f.sphere_center), fptr(f.sphere_r_sq), fptr(f.sphere_r_inv)
    d.sphere_material = uptr(f.sphere_material)
    d.n_triangles = f.n_triangles
    d.tri_v1, d.tri_e1, d.tri_e2, d.tri_normal = fptr(f.tri_v1), fptr(f.tri_e1), fptr(f.tri_e2), fptr(f.tri_normal)
    d.tri_material = uptr(f.tri_material)
    d.n_materials = int(f.materials.shape[0])
    d.materials = fptr(f.materials)
    d.n_lights = int(f.lights.shape[0])
    d.lights = fptr(f.lights)
    for k, v in (bvh or {}).items():
        setattr(d.bvh, k, v)
    d.device_budget_bytes = int(budget)
    return d, f


def make_params(cfg, aa_offsets=None, cloud=None, window=None, n_ranks=1, rank=0, traversal=RT_TRAVERSAL_BVH, tuning=None):
    """cfg: RenderConfig; tuning: dict of rt_tuning fields.  Returns (params, keepalive)."""
    from . import sampling

    p = rt_params()
    p.abi_version = RT_ABI_VERSION
    p.width, p.height = cfg.width, cfg.height
    fo = cfg.focus
    p.focus[0], p.focus[1], p.focus[2] = float(fo.x), float(fo.y), float(fo.z)
    p.fw, p.fh, p.fd = float(cfg.fw), float(cfg.fh), float(cfg.fd)
    p.eps_distance = float(cfg.eps_distance)
    p.air_ior = float(cfg.air_ior)
    p.ambient = float(cfg.ambient)
    flags = 0
    if cfg.has("reflections"):
        flags |= RT_FLAG_REFLECTIONS
    if cfg.has("refractions"):
        flags |= RT_FLAG_REFRACTIONS
    if cfg.has("backface_culling"):
        flags |= RT_FLAG_BACKFACE_CULLING
    keep = []
    if cfg.has("anti_aliasing"):
        flags |= RT_FLAG_ANTI_ALIASING
        if aa_offsets is None:
            aa_offsets = sampling.aa_offsets(cfg)
        aa_offsets = np.ascontiguousarray(aa_offsets, np.float32)
        p.aa_rays = int(aa_offsets.shape[0])
        p.aa_offsets = fptr(aa_offsets)
        keep.append(aa_offsets)
    p.flags = flags
    n = cfg.point_light_multiplicator
    p.light_mult = n
    p.cloud_seed = int(cfg.cloud_seed) & 0xFFFFFFFF
    if n > 1:
        if cloud is None:
            cloud = sampling.cloud_sets(cfg)
        cloud = np.ascontiguousarray(cloud, np.float32)
        assert cloud.shape[1] == n and cloud.shape[2] == 3
        p.n_cloud_sets = int(cloud.shape[0])
        p.cloud_sets = fptr(cloud)
        keep.append(cloud)
    p.max_depth_reflection = cfg.max_depth_reflection
    p.max_depth_refraction = cfg.max_depth_refraction
    if window is not None:
        p.win_x0, p.win_y0, p.win_w, p.win_h = (int(v) for v in window)
    p.tile_size = cfg.render_stride
    p.n_ranks, p.rank = int(n_ranks), int(rank)
    p.traversal = int(traversal)
    for k, v in (tuning or {}).items():
        setattr(p.tuning, k, int(v))
    return p, keep


SPHERE_GROUP = ("sphere_center", "sphere_r_sq", "sphere_r_inv")
TRIANGLE_GROUP = ("tri_v1", "tri_e1", "tri_e2", "tri_normal")


def scene_delta_groups(old, new, full=False):
    """What differs between two contiguous FlatScenes of the same shape, as the groups of an rt_scene_delta:
    {"spheres": bool, "triangles": (first, count) or None, "materials": bool, "lights": bool}.  Arrays are compared as
    bits (a NaN equals itself, -0 differs from +0).  full: every group the scene has objects for, changed or not.
    Raises ValueError when a count or the object -> material assignment differs: an update cannot express that."""
    for name in SPHERE_GROUP + TRIANGLE_GROUP + ("sphere_material", "tri_material", "materials", "lights"):
        if getattr(old, name).shape != getattr(new, name).shape:
            raise ValueError(f"{name}: shape {getattr(new, name).shape} differs from the scene's {getattr(old, name).shape}; "
                             "an update keeps every count (create a new device scene)")
    for name in ("sphere_material", "tri_material"):
        if not np.array_equal(getattr(old, name), getattr(new, name)):
            raise ValueError(f"{name} differs: an update keeps the object -> material assignment (create a new device scene)")
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)  # noqa: E731
    differs = lambda name: not np.array_equal(bits(getattr(old, name)), bits(getattr(new, name)))  # noqa: E731
    tri = None
    if new.n_triangles:
        rows = np.zeros(new.n_triangles, bool)
        for name in TRIANGLE_GROUP:
            rows |= (bits(getattr(old, name)) != bits(getattr(new, name))).reshape(new.n_triangles, -1).any(1)
        if full:
            tri = (0, new.n_triangles)
        elif rows.any():
            idx = np.flatnonzero(rows)
            tri = (int(idx[0]), int(idx[-1]) - int(idx[0]) + 1)
    return {"spheres": bool(new.n_spheres) and (full or any(differs(n) for n in SPHERE_GROUP)), "triangles": tri,
            "materials": bool(new.materials.shape[0]) and (full or differs("materials")),
            "lights": bool(new.lights.shape[0]) and (full or differs("lights"))}


def make_scene_delta(new, groups, ptr=None):
    """rt_scene_delta carrying `groups` (scene_delta_groups) of `new`: a contiguous FlatScene (host arrays; the triangle
    range is cut out of its arrays), or any object with the same attributes whose arrays `ptr` turns into addresses (device
    tensors; its triangle arrays ARE the range).  Returns (delta, keepalive)."""
    if ptr is None:
        ptr = lambda a: a.ctypes.data  # noqa: E731
    d = rt_scene_delta()
    d.abi_version = RT_ABI_VERSION
    keep = []

    def put(field, a):
        keep.append(a)
        setattr(d, field, ptr(a))

    if groups["spheres"]:
        for name in SPHERE_GROUP:
            put(name, getattr(new, name))
    if groups["triangles"]:
        first, count = groups["triangles"]
        d.tri_first, d.tri_count = first, count
        for name in TRIANGLE_GROUP:
            a = getattr(new, name)
            put(name, np.ascontiguousarray(a[first:first + count]) if isinstance(a, np.ndarray) else a)
    if groups["materials"]:
        put("materials", new.materials)
    if groups["lights"]:
        put("lights", new.lights)
    return d, keep
