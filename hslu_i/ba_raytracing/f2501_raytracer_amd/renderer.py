"""`ImageBuffer` and `RaytracerRenderer`: the reference's render boundary over the HIP library.

Reference: `trait Renderer<W,H,C>::render(&self, buffer: &ImageBuffer<W,H>, scene: &Scene<Vec3>)`
(`src/renderer/mod.rs:80-94`), implemented by `RaytracerRenderer<C>`
(`src/renderer/raytracer_renderer.rs:139-140,1360-1378`); `ImageBuffer<W,H>` = `[AtomicU32; W*H]`
(`src/image_buffer.rs:8-44`).
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, NamedTuple, Optional, Tuple

import numpy as np

from . import _abi, _lib
from .config import RenderConfig
from .scene import FlatScene, Scene


class ImageBuffer:
    """W*H packed 0xAARRGGBB pixels, row-major, zero-initialised (image_buffer.rs:27-37)."""

    def __init__(self, width: int, height: int, color: int = 0):
        self.width, self.height = int(width), int(height)
        self.buffer = np.full((self.height * self.width,), color, np.uint32)

    @staticmethod
    def new(width: int, height: int) -> "ImageBuffer":
        return ImageBuffer(width, height, 0)

    @staticmethod
    def new_with_color(width: int, height: int, color: int) -> "ImageBuffer":
        return ImageBuffer(width, height, color)

    def get_u32_slice(self) -> np.ndarray:
        return self.buffer

    def __len__(self) -> int:
        return self.buffer.shape[0]

    def as_rgb8(self) -> np.ndarray:
        """FileOutput::render_buffer's u32 -> RGB8 rows (reference src/output/file.rs:27-49)."""
        b = self.buffer.reshape(self.height, self.width)
        return np.stack([(b >> 16) & 0xFF, (b >> 8) & 0xFF, b & 0xFF], axis=-1).astype(np.uint8)


class RayHits(NamedTuple):
    """Nearest hit per ray (`SurfaceInteraction`, surface_interaction.rs:13-30): canonical object id (-1 = miss), t
    (+inf on a miss), point, normal (0 on a miss) and material row (0xFFFFFFFF on a miss; -1 in an int32 tensor)."""
    id: Any
    t: Any
    point: Any
    normal: Any
    material: Any


class ClosestPoints(NamedTuple):
    """Nearest surface point per query point (`rt_point_hits`): canonical object id (-1 = miss), distance (+inf on a miss),
    the point, the normal there, the barycentric weights of e1 and e2 (0 for spheres) -- all 0 on a miss -- and the material row
    (0xFFFFFFFF on a miss; -1 in an int32 tensor)."""
    id: Any
    distance: Any
    point: Any
    normal: Any
    bary: Any
    material: Any


class RayHitLists(NamedTuple):
    """The first `max_hits` hits per ray (`rt_ray_hit_lists`): `count` (n,) entries are valid in row i of the (n, max_hits) planes
    id, t, material and the (n, max_hits, 3) planes point, normal, ordered by t and on equal t by the larger id first; the entries
    behind them hold the miss values of RayHits.  `total` (n,) is the number of objects hit in all, or None when it was not asked for."""
    count: Any
    id: Any
    t: Any
    point: Any
    normal: Any
    material: Any
    total: Any


class Occlusion(NamedTuple):
    """Hemisphere visibility per surface point (`rt_occlusion_out`): `clear` (n,) samples that are not occluded, `visibility` (n,)
    = clear / samples, `bent_normal` (n, 3) the normalised mean direction of the clear samples (0 where none is clear), and
    `bits` (n, ceil(samples / 32)) with bit s % 32 of word s / 32 set where sample s is occluded, or None when not asked for."""
    clear: Any
    visibility: Any
    bent_normal: Any
    bits: Any


class Containment(NamedTuple):
    """Inside test per point (`rt_solid_out`): `inside` (n,) bool; `votes` (n,) uint8, the directions that voted inside -- a value
    other than 0 or R means the directions disagree: the point lies on or near a surface, or the surface is open or inconsistently
    oriented there; `crossings` (n, R) triangles crossed and `winding` (n, R) leaving minus entering crossings per direction."""
    inside: Any
    votes: Any
    crossings: Any
    winding: Any


class SignedDistance(NamedTuple):
    """Signed distance per point (`rt_signed_distance_out`): `distance` (n,) is negative inside, positive outside, +-inf on a miss
    of the closest-point search; `inside` and `votes` as in Containment; id, point, normal, bary and material as in ClosestPoints."""
    distance: Any
    inside: Any
    votes: Any
    id: Any
    point: Any
    normal: Any
    bary: Any
    material: Any


class IntersectionTest(NamedTuple):
    """`IntersectionTest` (raytracer.rs:17-22) per segment.  color_filter is unspecified where completely_occluded."""
    has_intersection: Any
    completely_occluded: Any
    combined_opacity: Any
    color_filter: Any


class Radiance(NamedTuple):
    """`single_raytrace` per ray (raytracer_renderer.rs:147-264): linear RGB ((0, 0, 0) on a miss), its valid mask, and the
    primary hit's canonical object id (-1 = miss) and distance (+inf on a miss)."""
    rgb: Any
    valid: Any
    id: Any
    t: Any


class AdaptiveRadiance(NamedTuple):
    """The pixel planes of an adaptive view frame (`DeviceScene.render_view(refine=...)`): a Radiance and the mask of the
    pixels that were refined with all their samples."""
    rgb: Any
    valid: Any
    id: Any
    t: Any
    mask: Any


class Refine(NamedTuple):
    """The refine rule of an adaptive view frame (`rt_view_refine`): a pixel takes all its samples when sample 0 differs from a
    neighbour's by more than the tolerances -- criteria: a combination of "id", "depth", "colour", "every" (a string, an
    iterable of them, or the RT_REFINE_* bits); depth_tol relative to the nearer hit, colour_tol per linear RGB channel."""
    criteria: Any = ("depth", "colour")
    colour_tol: float = 0.05
    depth_tol: float = 0.05

    BITS = {"id": _abi.RT_REFINE_ID, "depth": _abi.RT_REFINE_DEPTH, "colour": _abi.RT_REFINE_COLOUR, "every": _abi.RT_REFINE_EVERY}

    def struct(self) -> "_abi.rt_view_refine":
        c = self.criteria
        if not isinstance(c, int):
            bits = 0
            for name in ((c,) if isinstance(c, str) else c):
                if name not in self.BITS:
                    raise ValueError(f"criteria must be among {sorted(self.BITS)}, got {name!r}")
                bits |= self.BITS[name]
            c = bits
        return _abi.rt_view_refine(_abi.RT_ABI_VERSION, int(c), float(self.colour_tol), float(self.depth_tol))


class RayOrder:
    """Owns an `rt_ray_order*`: a permutation of one batch's rays on one device, which `DeviceScene.trace_rays(order=...)`
    reads the batch through so that rays which are neighbours in space share a wavefront.  The results are those of the
    unordered call, bit for bit.  An order belongs to a batch, not to a scene: it survives `DeviceScene.update`, works with
    any scene on its device and may be reused for any batch of the same number of rays."""

    def __init__(self, device: int, capacity: int, origin_bits: int = 0):
        lib = _lib.load()
        desc = _abi.rt_ray_order_desc(_abi.RT_ABI_VERSION, int(capacity), int(origin_bits), 0)
        h = C.c_void_p()
        _lib.check(lib.rt_ray_order_create(C.byref(desc), int(device), C.byref(h)))
        self._h = h
        self.device = int(device)
        self.capacity = int(capacity)

    @staticmethod
    def from_permutation(device: int, perm) -> "RayOrder":
        """The caller's own order (its tiles, say): perm[k] = the ray at position k, a permutation of range(n)."""
        perm = np.ascontiguousarray(perm, np.uint32)
        if perm.ndim != 1 or perm.size == 0:
            raise ValueError("perm must be a non-empty 1-d array")
        order = RayOrder(device, perm.size)
        _lib.check(_lib.load().rt_ray_order_set(order.handle, perm.ctypes.data, perm.size))
        return order

    @property
    def handle(self) -> C.c_void_p:
        if self._h is None:
            raise RuntimeError("ray order destroyed")
        return self._h

    def build(self, batch: "_abi.rt_ray_batch", stream=None) -> "RayOrder":
        """Sorts the rays of `batch`: host arrays (stream None; blocks) or device arrays enqueued on `stream`."""
        lib = _lib.load()
        if stream is None:
            _lib.check(lib.rt_ray_order_build(self.handle, C.byref(batch)))
        else:
            _lib.check(lib.rt_ray_order_build_device(self.handle, C.byref(batch), stream))
        return self

    def _read(self, perm: bool, keys: bool):
        lib = _lib.load()
        info = _abi.rt_ray_order_info()
        _lib.check(lib.rt_ray_order_read(self.handle, None, None, C.byref(info)))  # (the handle knows how many rays it holds)
        if not (perm or keys):
            return None, None, info.as_dict()
        p = np.empty(info.n_rays, np.uint32) if perm else None
        k = np.empty(info.n_rays, np.uint32) if keys else None
        _lib.check(lib.rt_ray_order_read(self.handle, p.ctypes.data if perm else None, k.ctypes.data if keys else None, None))
        return p, k, info.as_dict()

    @property
    def n_rays(self) -> int:
        """rays of the batch the order was last built or set for"""
        return self.info["n_rays"]

    def permutation(self) -> np.ndarray:
        """perm[k] = the ray at position k (blocks until the last build is done)."""
        return self._read(True, False)[0]

    def keys(self) -> np.ndarray:
        """The sort key of every ray, by ray (a built order only)."""
        return self._read(False, True)[1]

    @property
    def info(self) -> Dict:
        """rt_ray_order_info: rays, live rays, the bit split of the key, device bytes, the device time of a blocking build."""
        return self._read(False, False)[2]

    def close(self):
        if self._h is not None:
            _lib.load().rt_ray_order_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceView:
    """Owns an `rt_view*`: a frame shape, a table of sample offsets and a camera on one device, with the device memory a
    frame of it needs -- the rays of every (pixel, distinct sample), their radiance planes and a ray order.
    `DeviceScene.render_view` makes the rays, traces them and resolves the samples into pixels, all on the device.

    samples: (n, 2) float32 offsets (None: one ray through the pixel centre) -- pixels from the pixel centre for a pinhole
    camera, the units of `sampling.aa_offsets` for the reference's (`camera.view_samples`).  order: "once" (the first frame
    builds the ray order, later frames reuse it), "always" or "none"; the image is the same.  camera: an `rt_view_camera`
    (`PinholeCamera.view_camera()`, `camera.reference_view_camera(cfg)`); `set_camera` moves it between frames.

    lens_samples: (n, 2) float32 lens offsets in unit-disk coordinates, one per sample (`camera.lens_samples(n)`) -> a
    thin-lens view (`rt_view_create_lens`): `set_lens(camera.ThinLens(aperture, focus_distance))` opens the lens, frames then
    have depth of field.  lens: a ThinLens set at once.  Without `set_lens`, or with aperture 0, the view is a pinhole's."""

    ORDERS = {"once": _abi.RT_VIEW_ORDER_ONCE, "always": _abi.RT_VIEW_ORDER_ALWAYS, "none": _abi.RT_VIEW_ORDER_NONE}

    def __init__(self, device: int, width: int, height: int, samples=None, order: str = "once", camera=None, lens_samples=None, lens=None):
        if order not in self.ORDERS:
            raise ValueError(f"order must be one of {sorted(self.ORDERS)}")
        smp = np.zeros((1, 2), np.float32) if samples is None else np.ascontiguousarray(samples, np.float32)
        if smp.ndim != 2 or smp.shape[1] != 2:
            raise ValueError(f"samples must be (n, 2), got {smp.shape}")
        lib = _lib.load()
        desc = _abi.rt_view_desc(_abi.RT_ABI_VERSION, int(width), int(height), int(smp.shape[0]), smp.ctypes.data, self.ORDERS[order])
        h = C.c_void_p()
        if lens_samples is None:
            if lens is not None:
                raise ValueError("a lens needs lens_samples")
            _lib.check(lib.rt_view_create(C.byref(desc), int(device), C.byref(h)))
        else:
            ls = np.ascontiguousarray(lens_samples, np.float32)
            if ls.shape != smp.shape:
                raise ValueError(f"lens_samples must be {smp.shape} as the samples, got {ls.shape}")
            _lib.check(lib.rt_view_create_lens(C.byref(desc), ls.ctypes.data, int(device), C.byref(h)))
        self._h = h
        self.device, self.width, self.height, self.n_samples = int(device), int(width), int(height), int(smp.shape[0])
        if camera is not None:
            self.set_camera(camera)
        if lens is not None:
            self.set_lens(lens)

    @property
    def handle(self) -> C.c_void_p:
        if self._h is None:
            raise RuntimeError("view destroyed")
        return self._h

    def set_camera(self, camera: "_abi.rt_view_camera") -> "DeviceView":
        _lib.check(_lib.load().rt_view_set_camera(self.handle, C.byref(camera)))
        return self

    def set_lens(self, lens) -> "DeviceView":
        """The lens of the next frames: a `camera.ThinLens` (or an `rt_view_lens`); a view made with lens_samples only."""
        st = lens.struct() if hasattr(lens, "struct") else lens
        _lib.check(_lib.load().rt_view_set_lens(self.handle, C.byref(st)))
        return self

    @property
    def info(self) -> Dict:
        """rt_view_info: pixels, samples, distinct samples, rays, device bytes, and the stage times of the last host-form frame."""
        info = _abi.rt_view_info()
        _lib.check(_lib.load().rt_view_read(self.handle, None, C.byref(info)))
        return info.as_dict()

    def enable_adaptive(self) -> "DeviceView":
        """Allocates the workspace adaptive frames need (`rt_view_enable_adaptive`; idempotent)."""
        _lib.check(_lib.load().rt_view_enable_adaptive(self.handle))
        return self

    @property
    def adaptive_info(self) -> Dict:
        """rt_view_adaptive_info of the last adaptive frame: refined pixels, live rays of pass 2, workspace bytes, and the
        stage times of the last host-form frame."""
        info = _abi.rt_view_adaptive_info()
        _lib.check(_lib.load().rt_view_adaptive_read(self.handle, C.byref(info)))
        return info.as_dict()

    def plane_of(self) -> np.ndarray:
        """plane_of[k] = the distinct sample (ray plane) sample k reads."""
        out = np.empty(self.n_samples, np.uint8)
        _lib.check(_lib.load().rt_view_read(self.handle, out.ctypes.data, None))
        return out

    def rays(self, torch_device=None):
        """The generator alone -> (origins, directions), (n_rays, 3) float32; ray u * width * height + p belongs to pixel p
        and distinct sample u.  numpy arrays (blocks), or with torch_device=True tensors on the view's device, enqueued on
        torch.cuda.current_stream()."""
        lib = _lib.load()
        n = self.info["n_rays"]
        if not torch_device:
            o, d = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
            _lib.check(lib.rt_view_rays(self.handle, o.ctypes.data, d.ctypes.data))
            return o, d
        import torch

        dev = torch.device("cuda", self.device)
        o, d = torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty((n, 3), dtype=torch.float32, device=dev)
        _lib.check(lib.rt_view_rays_device(self.handle, o.data_ptr(), d.data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return o, d

    def close(self):
        if self._h is not None:
            _lib.load().rt_view_destroy(self._h)  # (waits for the view's device work)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceScene:
    """Owns an `rt_scene*` (device copies + BVH)."""

    def __init__(self, flat: FlatScene, device: int = 0, bvh: Optional[Dict] = None, budget: int = 0):
        """budget: device memory for the optional acceleration tables (rt_scene_desc.device_budget_bytes; 0 = 128 MiB)."""
        lib = _lib.load()
        desc, keep = _abi.make_scene_desc(flat, bvh, budget)
        h = C.c_void_p()
        _lib.check(lib.rt_scene_create(C.byref(desc), int(device), C.byref(h)))
        self._h = h
        self.device = int(device)
        self.flat = keep
        self.last_trace_stats: Optional[Dict] = None  # rt_stats of the last trace_rays call on host arrays
        self._trace_params = None  # (key, rt_params, keepalive) of the last trace_rays call
        self._call_order: Optional[RayOrder] = None  # trace_rays(tensors, order=True): the order of the last such call

    @property
    def handle(self) -> C.c_void_p:
        if self._h is None:
            raise RuntimeError("scene destroyed")
        return self._h

    def bvh_info(self) -> Dict[str, int]:
        info = _abi.rt_bvh_info()
        _lib.check(_lib.load().rt_scene_bvh_info(self.handle, C.byref(info)))
        return {k: int(getattr(info, k)) for k, _ in info._fields_}

    def memory_info(self) -> Dict[str, int]:
        info = _abi.rt_scene_info()
        _lib.check(_lib.load().rt_scene_memory_info(self.handle, C.byref(info)))
        return {k: int(getattr(info, k)) for k, _ in info._fields_}

    def bvh_quality(self) -> Dict:
        """`rt_scene_bvh_quality`: the SAH cost of the tree as it stands (`sah_now`) next to the one it had at creation
        (`sah_created`), the integer sums behind it and the device time of the report.  Blocks; runs on a stream of its own."""
        q = _abi.rt_bvh_quality()
        _lib.check(_lib.load().rt_scene_bvh_quality(self.handle, C.byref(q)))
        return q.as_dict()

    def rebuild(self, info: bool = False, method: str = "lbvh", radius: Optional[int] = None, keep_better: bool = False):
        """`rt_scene_rebuild`: a new tree for this scene, built on the device from the geometry it holds right now -- the
        repair for a tree that `update` / `DevicePose.apply` / `DeviceSkin.apply` have refitted until it decayed (`bvh_quality`).  The tree is an
        LBVH with the leaf size of creation; renders and queries behave as on a DeviceScene created from the current
        description.  Blocks; runs on a stream of its own; waits for the scene's frames in flight.  The description this
        scene holds (`flat`) is unchanged.  Returns None, or with info=True the rt_rebuild_info of the call as a dict.

        Any other argument goes through `rt_scene_rebuild_with`: method="ploc" clusters by surface area inside a window of
        `radius` positions of the Morton order (None: 8; 1 .. 32) -- a tighter tree that takes longer to build; keep_better=True
        builds the candidate, compares its SAH with the tree's in place and swaps only if it is lower.  With info=True these
        calls return the rt_rebuild_report as a dict: the info fields (of the tree in place), the SAH sums before / after,
        `swapped` and `iterations`."""
        if method == "lbvh" and radius is None and not keep_better:
            inf = _abi.rt_rebuild_info()
            _lib.check(_lib.load().rt_scene_rebuild(self.handle, C.byref(inf)))
            return inf.as_dict() if info else None
        methods = {"lbvh": _abi.RT_REBUILD_LBVH, "ploc": _abi.RT_REBUILD_PLOC}
        if method not in methods:
            raise ValueError(f"rebuild: method {method!r} is not one of {sorted(methods)}")
        desc = _abi.rt_rebuild_desc(methods[method], int(radius or 0), _abi.RT_REBUILD_KEEP_BETTER if keep_better else 0, 0)
        rep = _abi.rt_rebuild_report()
        _lib.check(_lib.load().rt_scene_rebuild_with(self.handle, C.byref(desc), C.byref(rep)))
        return rep.as_dict() if info else None

    def update(self, flat, info: bool = False, tri_first: int = 0):
        """New values for the objects this scene already has, in place (`rt_scene_update`): the BVH is refitted on the
        device, not rebuilt, and afterwards every render and query behaves as on a DeviceScene created from the new
        description.  Blocks until the update is done.

        flat: a FlatScene of numpy arrays -- it is compared with the description this scene holds, only the groups that
        differ are sent (spheres, triangles, materials, lights), for triangles the smallest covering range; an equal
        description is no call at all.  ValueError when a count or the object -> material assignment differs.
        Or any object whose arrays are float32 torch tensors on this scene's device (`rt_scene_update_device` on
        torch.cuda.current_stream()): every group it has is sent as given -- attributes that are missing or None are
        unchanged, tri_v1 / tri_e1 / tri_e2 / tri_normal of shape (count, 3) replace triangles [tri_first, tri_first + count).
        Returns None, or with info=True the rt_update_info of the call as a dict (None when nothing was sent)."""
        lib = _lib.load()
        inf = _abi.rt_update_info()
        if isinstance(flat, FlatScene) and isinstance(flat.materials, np.ndarray):
            new = flat.contiguous()
            groups = _abi.scene_delta_groups(self.flat, new)
            if not any(groups.values()):
                return None
            d, keep = _abi.make_scene_delta(new, groups)
            _lib.check(lib.rt_scene_update(self.handle, C.byref(d), C.byref(inf)))
            self.flat = new
            return inf.as_dict() if info else None
        import types

        import torch

        want = torch.device("cuda", self.device)
        got = types.SimpleNamespace(**{k: getattr(flat, k, None) for k in _abi.SPHERE_GROUP + _abi.TRIANGLE_GROUP + ("materials", "lights")})
        old = self.flat
        shapes = {"sphere_center": (old.n_spheres, 3), "sphere_r_sq": (old.n_spheres,), "sphere_r_inv": (old.n_spheres,),
                  "materials": tuple(old.materials.shape), "lights": tuple(old.lights.shape)}
        count = None
        for name, t in vars(got).items():
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != want:
                raise ValueError(f"{name} must be a float32 tensor on {want} (the scene's device)")
            if name in _abi.TRIANGLE_GROUP:
                count = t.shape[0] if count is None else count
                if t.dim() != 2 or tuple(t.shape) != (count, 3) or tri_first + count > old.n_triangles:
                    raise ValueError(f"{name}: shape {tuple(t.shape)} does not replace triangles [{tri_first}, {tri_first} + count) of {old.n_triangles}")
            elif tuple(t.shape) != shapes[name]:
                raise ValueError(f"{name}: shape {tuple(t.shape)} differs from the scene's {shapes[name]}; an update keeps every count")
            setattr(got, name, t.contiguous())
        for group in (_abi.SPHERE_GROUP, _abi.TRIANGLE_GROUP):
            given = [getattr(got, k) is not None for k in group]
            if any(given) and not all(given):
                raise ValueError(f"{', '.join(group)} are given together or not at all")
        groups = {"spheres": got.sphere_center is not None and old.n_spheres > 0, "triangles": (int(tri_first), int(count)) if count else None,
                  "materials": got.materials is not None and old.materials.shape[0] > 0, "lights": got.lights is not None and old.lights.shape[0] > 0}
        if not any(groups.values()):
            return None
        d, keep = _abi.make_scene_delta(got, groups, ptr=lambda a: a.data_ptr())
        stream = self._stream_of(next(t for t in vars(got).values() if t is not None))
        _lib.check(lib.rt_scene_update_device(self.handle, C.byref(d), stream, C.byref(inf)))
        # the description this scene holds follows (the call has synchronised its stream)
        new = {k: np.array(getattr(old, k), copy=True) for k in FlatScene.__dataclass_fields__}
        for name, t in vars(got).items():
            if t is None:
                continue
            if name in _abi.TRIANGLE_GROUP:
                new[name][tri_first:tri_first + count] = t.cpu().numpy()
            else:
                new[name] = t.cpu().numpy()
        self.flat = FlatScene(**new).contiguous()
        return inf.as_dict() if info else None

    def cast_rays(self, origins, directions, backface_culling: bool = False) -> "RayHits":
        """`Raytracer::cast_ray` (raytracer.rs:162-220) for a batch of rays: the nearest hit of each.  origins /
        directions: (n, 3) float32, numpy arrays (the host entry point; numpy results) or torch tensors on this scene's
        device (the _device entry point on torch.cuda.current_stream(); tensor results, no synchronisation)."""
        torch_in, n, o, d, _ = self._batch(origins, directions, None)
        # (the material rows travel as int32 in a tensor: torch has no uint32 arithmetic; a miss is -1 = 0xFFFFFFFF)
        out, ptr = self._planes(RayHits, o, n, ("id", "int32", 1), ("t", "float32", 1), ("point", "float32", 3), ("normal", "float32", 3),
                                ("material", "int32" if torch_in else "uint32", 1))
        b = self._batch_struct(n, o, d, None, backface_culling, ptr)
        h = _abi.rt_ray_hits(ptr(out.id), ptr(out.t), ptr(out.point), ptr(out.normal), ptr(out.material))
        lib = _lib.load()
        if torch_in:
            _lib.check(lib.rt_cast_rays_device(self.handle, C.byref(b), C.byref(h), self._stream_of(o)))
        else:
            _lib.check(lib.rt_cast_rays(self.handle, C.byref(b), C.byref(h)))
        return out

    def any_intersection(self, origins, directions, max_distance=None, backface_culling: bool = False) -> "IntersectionTest":
        """`Raytracer::has_any_intersection` (raytracer.rs:24-106) for a batch of segments: every hit at t <= max_distance
        (None = +inf) counts.  Same input kinds as cast_rays."""
        torch_in, n, o, d, m = self._batch(origins, directions, max_distance)
        out, ptr = self._planes(IntersectionTest, o, n, ("has_intersection", "bool", 1), ("completely_occluded", "bool", 1),
                                ("combined_opacity", "float32", 1), ("color_filter", "float32", 3))
        b = self._batch_struct(n, o, d, m, backface_culling, ptr)
        oc = _abi.rt_ray_occlusion(ptr(out.has_intersection), ptr(out.completely_occluded), ptr(out.combined_opacity),
                                   ptr(out.color_filter))
        lib = _lib.load()
        if torch_in:
            _lib.check(lib.rt_any_intersection_device(self.handle, C.byref(b), C.byref(oc), self._stream_of(o)))
        else:
            _lib.check(lib.rt_any_intersection(self.handle, C.byref(b), C.byref(oc)))
        return out

    def closest_points(self, points, max_distance=None) -> "ClosestPoints":
        """`rt_closest_points` for a batch of points: the nearest point of the scene's surface to each, within max_distance
        (None = +inf; a scalar or (n,) array with numpy points, an (n,) tensor with tensors).  On equal distance the larger
        canonical id wins; a non-finite point is a miss.  Same input kinds as cast_rays: numpy arrays (the host entry point;
        numpy results) or torch tensors on this scene's device (the _device entry point on torch.cuda.current_stream(); tensor
        results, no synchronisation)."""
        torch_in, n, p, _, m = self._batch(points, points, max_distance)
        out, ptr = self._planes(ClosestPoints, p, n, ("id", "int32", 1), ("distance", "float32", 1), ("point", "float32", 3),
                                ("normal", "float32", 3), ("bary", "float32", 2), ("material", "int32" if torch_in else "uint32", 1))
        b = _abi.rt_point_batch(_abi.RT_ABI_VERSION, int(n), ptr(p), ptr(m) if m is not None else None)
        h = _abi.rt_point_hits(ptr(out.id), ptr(out.distance), ptr(out.point), ptr(out.normal), ptr(out.bary), ptr(out.material))
        lib = _lib.load()
        if torch_in:
            _lib.check(lib.rt_closest_points_device(self.handle, C.byref(b), C.byref(h), self._stream_of(p)))
        else:
            _lib.check(lib.rt_closest_points(self.handle, C.byref(b), C.byref(h)))
        return out

    def list_intersections(self, origins, directions, max_hits: int = 8, max_distance=None, backface_culling: bool = False,
                           total: bool = False, after=None) -> "RayHitLists":
        """`rt_list_intersections` for a batch of rays: the first max_hits (1 .. 16) objects each ray passes through at
        t <= max_distance (None = +inf), one hit per object, ordered by t and on equal t by the larger canonical id first -- entry 0
        is cast_rays' answer.  total=True also counts every object hit (rays with max_hits hits or more walk again for it).
        after=(t, id): a cursor per ray, (n,) float32 and (n,) int32 -- only hits strictly behind that key are returned; feeding
        back the last key of each row pages through all hits.  Same input kinds as cast_rays."""
        return self._list_intersections(origins, directions, int(max_hits), max_distance, backface_culling, total, after, True)

    def count_intersections(self, origins, directions, max_distance=None, backface_culling: bool = False):
        """`rt_list_intersections` with the `total` plane alone: the number of objects each ray passes through at
        t <= max_distance, (n,) -- uint32 in numpy, int32 in a tensor."""
        return self._list_intersections(origins, directions, _abi.RT_MAX_HITS_PER_RAY, max_distance, backface_culling, True, None, False).total

    def _list_intersections(self, origins, directions, k, max_distance, backface_culling, total, after, planes):
        torch_in, n, o, d, m = self._batch(origins, directions, max_distance)
        if not 1 <= k <= _abi.RT_MAX_HITS_PER_RAY:
            raise ValueError(f"max_hits must be 1 .. {_abi.RT_MAX_HITS_PER_RAY}, got {k}")
        u32 = "int32" if torch_in else "uint32"  # (torch has no uint32 arithmetic; a miss's material is -1 = 0xFFFFFFFF)
        cnt, ptr = self._planes(dict, o, n, ("count", u32, 1), ("total", u32, 1))
        lists, _ = self._planes(dict, o, n * k, ("id", "int32", 1), ("t", "float32", 1), ("point", "float32", 3), ("normal", "float32", 3),
                                ("material", u32, 1))
        at = ai = None
        if after is not None:
            at, ai = after
            if torch_in:
                import torch

                if not (isinstance(at, torch.Tensor) and isinstance(ai, torch.Tensor) and at.dtype == torch.float32 and ai.dtype == torch.int32
                        and at.device == o.device and ai.device == o.device and tuple(at.shape) == (n,) and tuple(ai.shape) == (n,)):
                    raise ValueError(f"after must be a float32 and an int32 tensor of shape ({n},) on the rays' device")
                at, ai = at.contiguous(), ai.contiguous()
            else:
                at, ai = np.ascontiguousarray(at, np.float32), np.ascontiguousarray(ai, np.int32)
                if at.shape != (n,) or ai.shape != (n,):
                    raise ValueError(f"after must be two arrays of shape ({n},), got {at.shape} and {ai.shape}")
        b = self._batch_struct(n, o, d, m, backface_culling, ptr)
        h = _abi.rt_ray_hit_lists()
        h.max_hits = k
        if at is not None:
            h.after_t, h.after_id = ptr(at), ptr(ai)
        if total:
            h.total = ptr(cnt["total"])
        if planes:
            h.count = ptr(cnt["count"])
            h.id, h.t, h.point, h.normal, h.material = (ptr(lists[name]) for name in ("id", "t", "point", "normal", "material"))
        lib = _lib.load()
        if torch_in:
            _lib.check(lib.rt_list_intersections_device(self.handle, C.byref(b), C.byref(h), self._stream_of(o)))
        else:
            _lib.check(lib.rt_list_intersections(self.handle, C.byref(b), C.byref(h)))
        if not planes:
            return RayHitLists(None, None, None, None, None, None, cnt["total"])
        return RayHitLists(cnt["count"], lists["id"].reshape(n, k), lists["t"].reshape(n, k), lists["point"].reshape(n, k, 3),
                           lists["normal"].reshape(n, k, 3), lists["material"].reshape(n, k), cnt["total"] if total else None)

    def ambient_occlusion(self, points, normals, samples: int = 16, table=None, first=None, bias: float = 1e-4, max_distance=float("inf"),
                          pass_transmissive: bool = False, bits: bool = False) -> "Occlusion":
        """`rt_ambient_occlusion` for a batch of surface points: of `samples` (1 .. 256) directions of the hemisphere above each
        point -- rows first[i], first[i] + 1, ... (modulo its length) of `table`, (m, 3) directions in the local frame with z
        along the normal; None: sampling.hemisphere_samples(samples) -- how many reach max_distance without a hit, from an origin
        moved `bias` along the normal.  pass_transmissive: transmissive objects do not occlude.  bits=True also returns the
        occluded samples as bit words.  normals may have any length; the point and normal planes of cast_rays and
        closest_points plug in directly.  Same input kinds as cast_rays: numpy arrays (the host entry point; numpy results) or
        torch tensors on this scene's device (the _device entry point on torch.cuda.current_stream(); tensor results, no
        synchronisation; a numpy table is uploaded on that stream; `first` is an (n,) int32 tensor there, uint32 in numpy)."""
        from . import sampling

        torch_in, n, p, nrm, _ = self._batch(points, normals, None)
        s = int(samples)
        if not 1 <= s <= _abi.RT_MAX_OCCLUSION_SAMPLES:
            raise ValueError(f"samples must be 1 .. {_abi.RT_MAX_OCCLUSION_SAMPLES}, got {s}")
        if table is None:
            table = sampling.hemisphere_samples(s)
        if torch_in:
            import torch

            if isinstance(table, np.ndarray):
                table = torch.from_numpy(np.ascontiguousarray(table, np.float32)).to(p.device)
            if not (isinstance(table, torch.Tensor) and table.dtype == torch.float32 and table.device == p.device):
                raise ValueError("table must be a float32 array or a float32 tensor on the points' device")
            table = table.contiguous()
            if first is not None:
                if not (isinstance(first, torch.Tensor) and first.dtype == torch.int32 and first.device == p.device and tuple(first.shape) == (n,)):
                    raise ValueError(f"first must be an int32 tensor of shape ({n},) on the points' device")
                first = first.contiguous()
        else:
            table = np.ascontiguousarray(table, np.float32)
            if first is not None:
                first = np.ascontiguousarray(first, np.uint32)
                if first.shape != (n,):
                    raise ValueError(f"first must be ({n},), got {first.shape}")
        if len(table.shape) != 2 or table.shape[1] != 3 or table.shape[0] < 1:
            raise ValueError(f"table must be (m, 3) with m >= 1, got {tuple(table.shape)}")
        u32 = "int32" if torch_in else "uint32"  # (torch has no uint32 arithmetic)
        words = (s + 31) // 32
        out, ptr = self._planes(dict, p, n, ("clear", u32, 1), ("visibility", "float32", 1), ("bent_normal", "float32", 3))
        word_plane, _ = self._planes(dict, p, n * words, ("bits", u32, 1))
        b = _abi.rt_occlusion_batch(_abi.RT_ABI_VERSION, int(n), ptr(p), ptr(nrm), s, int(table.shape[0]), ptr(table),
                                    ptr(first) if first is not None else None, float(bias), float(max_distance),
                                    _abi.RT_OCCLUSION_PASS_TRANSMISSIVE if pass_transmissive else 0)
        o = _abi.rt_occlusion_out(ptr(word_plane["bits"]) if bits else None, ptr(out["clear"]), ptr(out["visibility"]), ptr(out["bent_normal"]))
        lib = _lib.load()
        if torch_in:
            _lib.check(lib.rt_ambient_occlusion_device(self.handle, C.byref(b), C.byref(o), self._stream_of(p)))
        else:
            _lib.check(lib.rt_ambient_occlusion(self.handle, C.byref(b), C.byref(o)))
        return Occlusion(out["clear"], out["visibility"], out["bent_normal"], word_plane["bits"].reshape(n, words) if bits else None)

    def _solid_batch(self, points, max_distance, directions, rule):
        """-> (torch?, n, points, rt_solid_batch, the table it points to) for contains / signed_distance"""
        from . import sampling

        rules = {"parity": _abi.RT_SOLID_RULE_PARITY, "winding": _abi.RT_SOLID_RULE_WINDING}
        if rule not in rules:
            raise ValueError(f"rule {rule!r} is not one of {sorted(rules)}")
        torch_in, n, p, _, m = self._batch(points, points, max_distance)
        # the direction table is a host array in every entry point: it is small, validated by the library and passed by value
        if directions is None:
            table = sampling.solid_directions()
        elif isinstance(directions, np.ndarray) or not hasattr(directions, "cpu"):
            table = np.ascontiguousarray(directions, np.float32)
        else:
            table = np.ascontiguousarray(directions.cpu().numpy(), np.float32)
        if table.ndim != 2 or table.shape[1] != 3 or not 1 <= table.shape[0] <= _abi.RT_MAX_SOLID_DIRECTIONS:
            raise ValueError(f"directions must be (R, 3) with R in 1 .. {_abi.RT_MAX_SOLID_DIRECTIONS}, got {table.shape}")
        ptr = (lambda a: a.data_ptr()) if torch_in else (lambda a: a.ctypes.data)
        b = _abi.rt_solid_batch(_abi.RT_ABI_VERSION, int(n), ptr(p), ptr(m) if m is not None else None, int(table.shape[0]), rules[rule],
                                table.ctypes.data)
        return torch_in, n, p, b, table

    def contains(self, points, directions=None, rule: str = "parity") -> "Containment":
        """`rt_contains_points` for a batch of points: whether each lies inside the closed surfaces of the scene.  Along each of
        the R (1 .. 8) rows of `directions` ((R, 3), any length; None: sampling.solid_directions()) a ray is cast from the point;
        rule="parity": the direction votes inside when the triangles it crosses plus the spheres that contain the point are odd
        in number; rule="winding": when the crossings that leave a surface (by its stored normal) minus those that enter one,
        plus the containing spheres, are positive -- the rules differ where solids overlap.  A point is inside when more than half
        of the directions say so.  `votes` other than 0 or R marks points on or near a surface and open or inconsistently
        oriented surfaces.  Same input kinds as cast_rays: numpy arrays (the host entry point; numpy results) or torch tensors on
        this scene's device (the _device entry point on torch.cuda.current_stream(); tensor results, no synchronisation;
        crossings is int32 there)."""
        torch_in, n, p, b, keep = self._solid_batch(points, None, directions, rule)
        r = b.n_directions
        out, ptr = self._planes(dict, p, n, ("inside", "bool", 1), ("votes", "uint8", 1))
        rows, _ = self._planes(dict, p, n * r, ("crossings", "int32" if torch_in else "uint32", 1), ("winding", "int32", 1))
        o = _abi.rt_solid_out(ptr(out["inside"]), ptr(out["votes"]), ptr(rows["crossings"]), ptr(rows["winding"]))
        lib = _lib.load()
        if torch_in:
            _lib.check(lib.rt_contains_points_device(self.handle, C.byref(b), C.byref(o), self._stream_of(p)))
        else:
            _lib.check(lib.rt_contains_points(self.handle, C.byref(b), C.byref(o)))
        return Containment(out["inside"], out["votes"], rows["crossings"].reshape(n, r), rows["winding"].reshape(n, r))

    def signed_distance(self, points, max_distance=None, directions=None, rule: str = "parity") -> "SignedDistance":
        """`rt_signed_distance` for a batch of points: closest_points' answer for each -- the same bits -- with the distance
        negated where `contains` says inside.  max_distance (None = +inf) bounds the closest-point search only: a point with
        nothing in reach gets +inf outside and -inf inside.  directions and rule as in contains; same input kinds."""
        torch_in, n, p, b, keep = self._solid_batch(points, max_distance, directions, rule)
        out, ptr = self._planes(SignedDistance, p, n, ("distance", "float32", 1), ("inside", "bool", 1), ("votes", "uint8", 1), ("id", "int32", 1),
                                ("point", "float32", 3), ("normal", "float32", 3), ("bary", "float32", 2),
                                ("material", "int32" if torch_in else "uint32", 1))
        o = _abi.rt_signed_distance_out(ptr(out.distance), _abi.rt_solid_out(ptr(out.inside), ptr(out.votes), None, None),
                                        _abi.rt_point_hits(ptr(out.id), None, ptr(out.point), ptr(out.normal), ptr(out.bary), ptr(out.material)))
        lib = _lib.load()
        if torch_in:
            _lib.check(lib.rt_signed_distance_device(self.handle, C.byref(b), C.byref(o), self._stream_of(p)))
        else:
            _lib.check(lib.rt_signed_distance(self.handle, C.byref(b), C.byref(o)))
        return out

    def ray_order(self, origins, directions, origin_bits: int = 0) -> RayOrder:
        """A RayOrder for these rays on this scene's device, sorted on the device by the Morton code of origin and
        direction (origin_bits: bits per origin axis, 0 = default).  Same input kinds as cast_rays: numpy arrays (blocks)
        or torch tensors (enqueued on torch.cuda.current_stream(), no synchronisation)."""
        torch_in, n, o, d, _ = self._batch(origins, directions, None)
        if n == 0:
            raise ValueError("a ray order needs at least one ray")
        order = RayOrder(self.device, n, origin_bits)
        ptr = (lambda a: a.data_ptr()) if torch_in else (lambda a: a.ctypes.data)
        return order.build(self._batch_struct(n, o, d, None, False, ptr), self._stream_of(o) if torch_in else None)

    def _shading_params(self, cfg: RenderConfig, traversal: int, tuning: Optional[Dict]):
        """The rt_params a radiance call shades with: `cfg` without its anti-aliasing (the caller's rays, or a view's samples,
        are the samples).  The parameters of the last configuration are kept: building the light-cloud table is the expensive
        part of a call."""
        if cfg.has("anti_aliasing"):
            cfg = RenderConfig(**{**cfg.__dict__, "features": cfg.features - {"anti_aliasing"}})
        key = (cfg, int(traversal), tuple(sorted((tuning or {}).items())))
        if self._trace_params is None or self._trace_params[0] != key:
            self._trace_params = (key,) + _abi.make_params(cfg, traversal=traversal, tuning=tuning)
        return self._trace_params[1]

    def trace_rays(self, origins, directions, cfg: RenderConfig, tuning: Optional[Dict] = None, traversal: int = _abi.RT_TRAVERSAL_BVH,
                   argb=None, order=None) -> "Radiance":
        """`single_raytrace` (raytracer_renderer.rs:147-264) for a batch of rays: the colour the render gives a pixel whose
        camera ray is that ray, shaded with `cfg` (soft shadows, reflections, refractions, backface culling, depths; its
        camera and anti-aliasing are not used: the caller supplies its samples as rays).  Ray i takes the light-cloud set
        of pixel i.  Same input kinds as cast_rays: numpy arrays (host entry point, numpy results, `last_trace_stats` is
        filled) or torch tensors on this scene's device (the _device entry point on torch.cuda.current_stream(); tensor
        results).  argb: optional uint32 array / int32 tensor of n packed pixels; hits are written, misses keep their
        value.  One radiance or render call per scene at a time.
        order: None = the rays share wavefronts in the order given; True = an order is built on the device for this call;
        a RayOrder (ray_order(), RayOrder.from_permutation) is reused.  The results are the same bits either way.
        With tensors and order=True the order of the call lives in this scene and every such call rebuilds it on its
        stream: the rule above -- one radiance call per scene at a time -- holds across streams too (a second call on
        another stream must be ordered behind the first, as its frame slots and workspaces must)."""
        torch_in, n, o, d, _ = self._batch(origins, directions, None)
        if order is not None and order is not True and not isinstance(order, RayOrder):
            raise ValueError("order must be None, True or a RayOrder")
        p = self._shading_params(cfg, traversal, tuning)
        out, ptr = self._planes(Radiance, o, n, ("rgb", "float32", 3), ("valid", "bool", 1), ("id", "int32", 1), ("t", "float32", 1))
        if torch_in:
            import torch

            if argb is not None and not (isinstance(argb, torch.Tensor) and argb.dtype == torch.int32 and argb.device == o.device and
                                         tuple(argb.shape) == (n,) and argb.is_contiguous()):
                raise ValueError(f"argb must be a contiguous int32 tensor of shape ({n},) on {o.device}")
        elif argb is not None and not (isinstance(argb, np.ndarray) and argb.dtype == np.uint32 and argb.shape == (n,) and
                                       argb.flags["C_CONTIGUOUS"]):
            raise ValueError(f"argb must be a contiguous uint32 array of shape ({n},)")
        b = self._batch_struct(n, o, d, None, False, ptr)
        r = _abi.rt_ray_radiance(ptr(out.rgb), ptr(out.valid), ptr(out.id), ptr(out.t), ptr(argb) if argb is not None else None)
        lib = _lib.load()
        if torch_in:
            stream = self._stream_of(o)
            if order is True and n:
                # the order of this call stays alive in the scene while the stream reads it; a larger batch replaces it once
                # the device has drained (rare: the capacity only grows)
                if self._call_order is None or self._call_order.capacity < n:
                    if self._call_order is not None:
                        import torch

                        torch.cuda.synchronize(o.device)
                        self._call_order.close()
                    self._call_order = RayOrder(self.device, n)
                order = self._call_order.build(b, stream)
            if order is None or order is True:
                _lib.check(lib.rt_trace_rays_device(self.handle, C.byref(p), C.byref(b), C.byref(r), stream))
            else:
                _lib.check(lib.rt_trace_rays_ordered_device(self.handle, C.byref(p), C.byref(b), order.handle, C.byref(r), stream))
        else:
            st = _abi.rt_stats()
            if order is None:
                _lib.check(lib.rt_trace_rays(self.handle, C.byref(p), C.byref(b), C.byref(r), C.byref(st)))
            else:
                _lib.check(lib.rt_trace_rays_ordered(self.handle, C.byref(p), C.byref(b), None if order is True else order.handle, C.byref(r),
                                                     C.byref(st)))
            self.last_trace_stats = st.as_dict()
        return out

    def render_view(self, view: DeviceView, cfg: RenderConfig, tuning: Optional[Dict] = None, traversal: int = _abi.RT_TRAVERSAL_BVH,
                    argb=None, torch_out: bool = False, refine: Optional[Refine] = None) -> "Radiance":
        """A frame of `view` (`rt_render_view*`): its rays are made on the device, traced as `trace_rays` traces them --
        shaded with `cfg`, whose own camera and anti-aliasing are not used: the view's samples are the anti-aliasing -- and
        resolved into pixels with the reference's accumulation.  Returns the per-pixel Radiance planes (rgb, valid, and the id
        and t of sample 0), row-major with row 0 at the top.  argb: optional packed pixels as in trace_rays; pixels without a
        valid sample keep their value.  numpy results (the host entry point; `last_trace_stats` is filled), or with
        torch_out=True (or an argb tensor) tensors on this scene's device, enqueued on torch.cuda.current_stream().
        With soft shadows every distinct sample of a pixel draws its own light-cloud set.
        refine: a Refine -> an adaptive frame (`rt_render_view_adaptive*`; the view needs `enable_adaptive()`): sample 0 of
        every pixel, all samples only where the rule finds an edge.  Returns an AdaptiveRadiance: the planes plus `.mask`."""
        p = self._shading_params(cfg, traversal, tuning)
        n = view.width * view.height
        lib = _lib.load()
        spec = (("rgb", "float32", 3), ("valid", "bool", 1), ("id", "int32", 1), ("t", "float32", 1))
        result = Radiance
        if refine is not None:
            rf = refine.struct()
            spec, result = spec + (("mask", "bool", 1),), AdaptiveRadiance
        if torch_out or (argb is not None and not isinstance(argb, np.ndarray)):
            import torch

            dev = torch.device("cuda", self.device)
            if argb is not None and not (isinstance(argb, torch.Tensor) and argb.dtype == torch.int32 and argb.device == dev and
                                         tuple(argb.shape) == (n,) and argb.is_contiguous()):
                raise ValueError(f"argb must be a contiguous int32 tensor of shape ({n},) on {dev}")
            like = torch.empty(0, device=dev)
            out, ptr = self._planes(result, like, n, *spec)
            r = _abi.rt_ray_radiance(ptr(out.rgb), ptr(out.valid), ptr(out.id), ptr(out.t), ptr(argb) if argb is not None else None)
            if refine is not None:
                _lib.check(lib.rt_render_view_adaptive_device(self.handle, view.handle, C.byref(p), C.byref(rf), C.byref(r), ptr(out.mask),
                                                              self._stream_of(like)))
            else:
                _lib.check(lib.rt_render_view_device(self.handle, view.handle, C.byref(p), C.byref(r), self._stream_of(like)))
            return out
        if argb is not None and not (argb.dtype == np.uint32 and argb.shape == (n,) and argb.flags["C_CONTIGUOUS"]):
            raise ValueError(f"argb must be a contiguous uint32 array of shape ({n},)")
        out, ptr = self._planes(result, np.empty(0), n, *spec)
        r = _abi.rt_ray_radiance(ptr(out.rgb), ptr(out.valid), ptr(out.id), ptr(out.t), ptr(argb) if argb is not None else None)
        st = _abi.rt_stats()
        if refine is not None:
            _lib.check(lib.rt_render_view_adaptive(self.handle, view.handle, C.byref(p), C.byref(rf), C.byref(r), ptr(out.mask), C.byref(st)))
        else:
            _lib.check(lib.rt_render_view(self.handle, view.handle, C.byref(p), C.byref(r), C.byref(st)))
        self.last_trace_stats = st.as_dict()
        return out

    # (bool arrays and tensors hold one byte per element, 0 or 1: the uint8 planes of rt_ray_occlusion / rt_ray_radiance)

    @staticmethod
    def _planes(result, like, n, *spec):
        """-> (result(...), ptr): an entry point's result planes, one per (name, dtype, columns) of `spec`, uninitialised and
        of the kind of `like` -- numpy arrays, or tensors on its device -- and the function that takes a plane's address."""
        if isinstance(like, np.ndarray):
            new, ptr = np.empty, lambda a: a.ctypes.data
        else:
            import torch

            new, ptr = lambda shape, dt: torch.empty(shape, dtype=getattr(torch, dt), device=like.device), lambda a: a.data_ptr()
        return result(**{name: new((n,) if cols == 1 else (n, cols), dt) for name, dt, cols in spec}), ptr

    def _batch(self, origins, directions, max_distance):
        """-> (torch?, n, origins, directions, max_distance) validated and contiguous."""
        if isinstance(origins, np.ndarray) or isinstance(directions, np.ndarray):
            o = np.ascontiguousarray(origins, np.float32)
            d = np.ascontiguousarray(directions, np.float32)
            if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
                raise ValueError(f"origins / directions must both be (n, 3), got {o.shape} and {d.shape}")
            m = None
            if max_distance is not None:
                m = np.ascontiguousarray(np.broadcast_to(np.asarray(max_distance, np.float32), (o.shape[0],)), np.float32)
            return False, o.shape[0], o, d, m
        import torch

        if not (isinstance(origins, torch.Tensor) and isinstance(directions, torch.Tensor)):
            raise ValueError("origins / directions must be numpy arrays or torch tensors")
        want = torch.device("cuda", self.device)
        ts = [("origins", origins), ("directions", directions)]
        if max_distance is not None:
            if not isinstance(max_distance, torch.Tensor):
                raise ValueError("max_distance must be a tensor when the rays are tensors")
            ts.append(("max_distance", max_distance))
        for name, t in ts:
            if t.dtype != torch.float32:
                raise ValueError(f"{name} must be float32, got {t.dtype}")
            if t.device != want:
                raise ValueError(f"{name} must be on {want} (the scene's device), got {t.device}")
        if origins.dim() != 2 or origins.shape[1] != 3 or directions.shape != origins.shape:
            raise ValueError(f"origins / directions must both be (n, 3), got {tuple(origins.shape)} and {tuple(directions.shape)}")
        n = origins.shape[0]
        if max_distance is not None and tuple(max_distance.shape) != (n,):
            raise ValueError(f"max_distance must be ({n},), got {tuple(max_distance.shape)}")
        m = max_distance.contiguous() if max_distance is not None else None
        return True, n, origins.contiguous(), directions.contiguous(), m

    @staticmethod
    def _batch_struct(n, o, d, m, backface_culling, ptr):
        b = _abi.rt_ray_batch()
        b.abi_version = _abi.RT_ABI_VERSION
        b.n_rays = int(n)
        b.origin, b.direction = ptr(o), ptr(d)
        b.max_distance = ptr(m) if m is not None else None
        b.flags = _abi.RT_FLAG_BACKFACE_CULLING if backface_culling else 0
        return b

    @staticmethod
    def _stream_of(t):
        import torch

        return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)

    def close(self):
        if self._h is not None:
            _lib.load().rt_scene_destroy(self._h)  # (waits for the scene's frames and batches)
            self._h = None
        if self._call_order is not None:
            self._call_order.close()
            self._call_order = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DevicePose:
    """Owns an `rt_pose*`: the rest pose of rigid parts of a DeviceScene on its device.  `apply` places every part with a
    similarity transform (32 bytes per part) in one kernel and refits the scene in place, as `DeviceScene.update` would
    with arrays posed on the host.

    parts: [(tri_first, tri_count, sphere_first, sphere_count)], ranges pairwise disjoint.  The rest pose is taken from
    `scene.flat`.  rest_v2 / rest_v3: the rest VERTICES, (n_triangles, 3) float32; default `v1 + e1` / `v1 + e2` in fp32.
    rest_radius: (n_spheres,) float32; default `sqrt(r_sq)` in fp32.  The defaults are rounded reconstructions: pass the exact
    vertices and radii where you have them (a loader's), only then does the identity transform restate the scene bit for
    bit and a posed mesh equal the mesh loaded with that transform."""

    def __init__(self, scene: "DeviceScene", parts, rest_v2=None, rest_v3=None, rest_radius=None):
        f = scene.flat
        v2 = (f.tri_v1 + f.tri_e1).astype(np.float32) if rest_v2 is None else np.ascontiguousarray(rest_v2, np.float32)
        v3 = (f.tri_v1 + f.tri_e2).astype(np.float32) if rest_v3 is None else np.ascontiguousarray(rest_v3, np.float32)
        rad = np.sqrt(f.sphere_r_sq).astype(np.float32) if rest_radius is None else np.ascontiguousarray(rest_radius, np.float32)
        if v2.shape != f.tri_v1.shape or v3.shape != f.tri_v1.shape or rad.shape != f.sphere_r_sq.shape:
            raise ValueError("rest_v2 / rest_v3 must be (n_triangles, 3) and rest_radius (n_spheres,)")
        desc, keep = _abi.make_pose_desc(parts, f.n_triangles, f.n_spheres, f.tri_v1, v2, v3, f.tri_normal, f.sphere_center, rad)
        h = C.c_void_p()
        _lib.check(_lib.load().rt_pose_create(C.byref(desc), scene.device, C.byref(h)))
        self._h = h
        self.scene, self.n_parts = scene, int(desc.n_parts)
        self._parts = keep[0]

    @property
    def handle(self) -> C.c_void_p:
        if self._h is None:
            raise RuntimeError("pose destroyed")
        return self._h

    def geometry(self) -> Dict:
        """`rt_pose_read`: the posed arrays as the last apply left them -- tri_first, tri_count and tri_v1 / tri_e1 / tri_e2 /
        tri_normal over the pose's covering triangle range; sphere_center / sphere_r_sq / sphere_r_inv over all spheres
        (None when no part has spheres)."""
        lib = _lib.load()
        first, count = C.c_uint32(), C.c_uint32()
        _lib.check(lib.rt_pose_read(self.handle, None, None, None, None, C.byref(first), C.byref(count), None, None, None))
        n = int(count.value)
        ns = self.scene.flat.n_spheres if self._has_spheres() else 0
        out = {k: np.empty((n, 3), np.float32) for k in _abi.TRIANGLE_GROUP}
        out.update(sphere_center=np.empty((ns, 3), np.float32), sphere_r_sq=np.empty(ns, np.float32), sphere_r_inv=np.empty(ns, np.float32))
        _lib.check(lib.rt_pose_read(self.handle, *[out[k].ctypes.data for k in _abi.TRIANGLE_GROUP], None, None,
                                    *[out[k].ctypes.data for k in _abi.SPHERE_GROUP]))
        if not ns:
            out.update({k: None for k in _abi.SPHERE_GROUP})
        out.update(tri_first=int(first.value), tri_count=n)
        return out

    def _has_spheres(self) -> bool:
        return bool(self._parts[:, 3].any())

    def apply(self, transforms, info: bool = False):
        """Places every part and refits the scene (`rt_pose_apply`; blocks).  transforms: a list of n_parts `Similarity3`,
        an (n_parts, 8) float32 numpy array of rt_transform rows (`_abi.transform_row`), or a float32 torch tensor of that
        shape on the scene's device (`rt_pose_apply_device` on torch.cuda.current_stream(): no transform crosses the bus).
        `scene.flat` follows.  Returns None, or with info=True the rt_update_info of the call as a dict."""
        lib = _lib.load()
        inf = _abi.rt_update_info()
        if isinstance(transforms, (list, tuple, np.ndarray)):
            rows = _abi.transform_rows(transforms)
            if rows.shape[0] != self.n_parts:
                raise ValueError(f"{rows.shape[0]} transforms for {self.n_parts} parts")
            _lib.check(lib.rt_pose_apply(self.scene.handle, self.handle, rows.ctypes.data, C.byref(inf)))
        else:
            import torch

            want = torch.device("cuda", self.scene.device)
            t = transforms
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != want or tuple(t.shape) != (self.n_parts, 8):
                raise ValueError(f"transforms must be a float32 tensor of shape ({self.n_parts}, 8) on {want} (the scene's device)")
            t = t.contiguous()
            _lib.check(lib.rt_pose_apply_device(self.scene.handle, self.handle, C.c_void_p(t.data_ptr()), DeviceScene._stream_of(t), C.byref(inf)))
        # the description the scene holds follows (the call has synchronised its stream)
        g = self.geometry()
        old = self.scene.flat
        new = {k: np.array(getattr(old, k), copy=True) for k in FlatScene.__dataclass_fields__}
        for k in _abi.TRIANGLE_GROUP:
            new[k][g["tri_first"]:g["tri_first"] + g["tri_count"]] = g[k]
        if g["sphere_center"] is not None:
            for k in _abi.SPHERE_GROUP:
                new[k] = g[k]
        self.scene.flat = FlatScene(**new).contiguous()
        return inf.as_dict() if info else None

    def close(self):
        if self._h is not None:
            _lib.load().rt_pose_destroy(self._h)  # (waits for the pose's device work)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceSkin:
    """Owns an `rt_skin*`: an indexed mesh in rest pose on the device of a DeviceScene, deformed by linear blend skinning.
    `apply` takes 32 bytes per bone, skins the shared vertices, rebuilds the mesh's triangles from them and refits the scene
    in place, as `DeviceScene.update` would with arrays skinned on the host.

    mesh: an `obj.IndexedMesh` (position, normal or None, indices); it IS canonical triangles [tri_first, tri_first + T) of
    the scene.  bone: (V, 4) integers below n_bones, weight: (V, 4) float32; a zero weight skips its slot, weights are not
    normalised.  n_bones: default the largest bone index used + 1."""

    SKIN_OUT = ("position", "normal") + _abi.TRIANGLE_GROUP

    def __init__(self, scene: "DeviceScene", mesh, bone, weight, tri_first: int = 0, n_bones: Optional[int] = None):
        b = np.asarray(bone)
        if b.size and (b.min() < 0 or b.max() > 0xFFFF):
            raise ValueError("bone indices must be in [0, 65536)")
        if n_bones is None:
            n_bones = int(b.max()) + 1 if b.size else 1
        desc, keep = _abi.make_skin_desc(mesh.position, mesh.normal, mesh.indices, b, weight, n_bones, tri_first, scene.flat.n_triangles)
        h = C.c_void_p()
        _lib.check(_lib.load().rt_skin_create(C.byref(desc), scene.device, C.byref(h)))
        self._h = h
        self.scene, self.n_bones, self.has_normals = scene, int(n_bones), mesh.normal is not None
        self.n_vertices, self.tri_first, self.tri_count = int(desc.n_vertices), int(desc.tri_first), int(desc.tri_count)

    @property
    def handle(self) -> C.c_void_p:
        if self._h is None:
            raise RuntimeError("skin destroyed")
        return self._h

    def geometry(self) -> Dict:
        """`rt_skin_read`: the arrays as the last apply left them (before any: the rest mesh) -- position / normal over the
        vertices (normal None for a mesh without vertex normals), tri_v1 / tri_e1 / tri_e2 / tri_normal over the mesh's
        triangles, and tri_first, tri_count."""
        out = {k: np.empty((self.n_vertices if k in ("position", "normal") else self.tri_count, 3), np.float32) for k in self.SKIN_OUT}
        if not self.has_normals:
            out["normal"] = None
        _lib.check(_lib.load().rt_skin_read(self.handle, *[None if out[k] is None else out[k].ctypes.data for k in self.SKIN_OUT]))
        out.update(tri_first=self.tri_first, tri_count=self.tri_count)
        return out

    def apply(self, bones, info: bool = False):
        """Skins the mesh and refits the scene (`rt_skin_apply`; blocks).  bones: a list of n_bones `Similarity3`, an
        (n_bones, 8) float32 numpy array of rt_transform rows (`_abi.transform_row`), or a float32 torch tensor of that shape
        on the scene's device (`rt_skin_apply_device` on torch.cuda.current_stream(): no bone crosses the bus).
        `scene.flat` follows.  Returns None, or with info=True the rt_update_info of the call as a dict."""
        lib = _lib.load()
        inf = _abi.rt_update_info()
        if isinstance(bones, (list, tuple, np.ndarray)):
            if isinstance(bones, np.ndarray) and (bones.dtype != np.float32 or bones.shape != (self.n_bones, 8)):
                raise ValueError(f"bones must be a float32 array of shape ({self.n_bones}, 8), got {bones.dtype} {bones.shape}")
            rows = _abi.transform_rows(bones)
            if rows.shape[0] != self.n_bones:
                raise ValueError(f"{rows.shape[0]} transforms for {self.n_bones} bones")
            _lib.check(lib.rt_skin_apply(self.scene.handle, self.handle, rows.ctypes.data, C.byref(inf)))
        else:
            import torch

            want = torch.device("cuda", self.scene.device)
            t = bones
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != want or tuple(t.shape) != (self.n_bones, 8):
                raise ValueError(f"bones must be a float32 tensor of shape ({self.n_bones}, 8) on {want} (the scene's device)")
            t = t.contiguous()
            _lib.check(lib.rt_skin_apply_device(self.scene.handle, self.handle, C.c_void_p(t.data_ptr()), DeviceScene._stream_of(t), C.byref(inf)))
        # the description the scene holds follows (the call has synchronised its stream)
        g = self.geometry()
        old = self.scene.flat
        new = {k: np.array(getattr(old, k), copy=True) for k in FlatScene.__dataclass_fields__}
        for k in _abi.TRIANGLE_GROUP:
            new[k][self.tri_first:self.tri_first + self.tri_count] = g[k]
        self.scene.flat = FlatScene(**new).contiguous()
        return inf.as_dict() if info else None

    def close(self):
        if self._h is not None:
            _lib.load().rt_skin_destroy(self._h)  # (waits for the skin's device work)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RaytracerRenderer:
    """`RaytracerRenderer::<C>::default().render(&buffer, &scene)` on one MI355X.

    The reference renderer is a stateless ZST configured at compile time; here the configuration is
    a `RenderConfig` and the renderer caches the device scene between calls.
    """

    def __init__(self, cfg: RenderConfig, device: int = 0, traversal: int = _abi.RT_TRAVERSAL_BVH, scene_budget: int = 0,
                 update_in_place: bool = False):
        """scene_budget: rt_scene_desc.device_budget_bytes of the device scenes this renderer creates (0 = the library's
        default, 128 MiB for the optional acceleration tables).
        update_in_place: when a scene differs from the cached one only in values (same counts, same object -> material
        assignment), update the cached device scene (DeviceScene.update: a BVH refit) instead of building a new one."""
        self.update_in_place = bool(update_in_place)
        self.cfg = cfg
        self.device = int(device)
        self.traversal = int(traversal)
        self.scene_budget = int(scene_budget)
        self._cache: Optional[Tuple[bytes, DeviceScene]] = None
        self.last_stats: Optional[Dict] = None

    @staticmethod
    def default(cfg: Optional[RenderConfig] = None) -> "RaytracerRenderer":
        return RaytracerRenderer(cfg if cfg is not None else RenderConfig.from_features(()))

    def device_scene(self, scene) -> DeviceScene:
        """The reference's `render(&buffer, &scene)` reads the scene on every call; so does this: the scene is
        flattened and fingerprinted each time, and the cached device copy (+ BVH) is reused only when the content
        is unchanged.  Pass a `DeviceScene` to skip both."""
        if isinstance(scene, DeviceScene):
            return scene
        flat = scene.flatten() if isinstance(scene, Scene) else scene
        key = flat.fingerprint()
        if self._cache is not None and self._cache[0] == key:
            return self._cache[1]
        if self._cache is not None and self.update_in_place:
            try:
                self._cache[1].update(flat)
                self._cache = (key, self._cache[1])
                return self._cache[1]
            except ValueError:
                pass  # (counts or material assignment differ: a new device scene)
            except _lib.RtError as e:
                if e.code not in (_abi.RT_ERR_INVALID_ARG, _abi.RT_ERR_UNSUPPORTED):
                    raise  # (refused: a transmissive class changed, or the tree was split-clipped -- a new device scene)
        if self._cache is not None:
            self._cache[1].close()
        ds = DeviceScene(flat, self.device, budget=self.scene_budget)
        self._cache = (key, ds)
        return ds

    def render(self, buffer: ImageBuffer, scene, window=None, n_ranks: int = 1, rank: int = 0,
               aux: bool = False, tuning: Optional[Dict] = None):
        """Renders `scene` into `buffer` (hit pixels only).  Returns aux planes when aux=True.
        tuning: rt_tuning fields (execution knobs that never change the image)."""
        cfg = self.cfg
        if buffer.width != cfg.width or buffer.height != cfg.height:
            raise ValueError(f"buffer is {buffer.width}x{buffer.height}, config renders {cfg.width}x{cfg.height}")
        ds = self.device_scene(scene)
        p, keep = _abi.make_params(cfg, window=window, n_ranks=n_ranks, rank=rank, traversal=self.traversal, tuning=tuning)
        st = _abi.rt_stats()
        a = _abi.rt_aux()
        planes = None
        if aux:
            n = cfg.width * cfg.height
            planes = {
                "rgb": np.zeros((n, 3), np.float32),
                "hit_id": np.full((n,), -2, np.int32),
                "hit_t": np.zeros((n,), np.float32),
            }
            a.rgb, a.hit_id, a.hit_t = planes["rgb"].ctypes.data, planes["hit_id"].ctypes.data, planes["hit_t"].ctypes.data
        lib = _lib.load()
        _lib.check(lib.rt_render(ds.handle, C.byref(p), buffer.buffer.ctypes.data, C.byref(a) if aux else None, C.byref(st)))
        self.last_stats = st.as_dict()
        return planes

    def render_camera(self, buffer: ImageBuffer, scene, camera, tuning: Optional[Dict] = None, order=False, samples=None,
                      refine: Optional[Refine] = None, lens=None) -> Radiance:
        """Renders `scene` as `camera` sees it (anything with width, height and rays() -> (origins, directions), row-major
        with row 0 at the top: camera.PinholeCamera) into `buffer`: the rays go through DeviceScene.trace_rays with this
        renderer's configuration, hit pixels are written, misses keep the buffer's fill.  One ray per pixel -- the
        configuration's anti-aliasing belongs to the reference's own view and is not applied.  Returns the Radiance planes.
        order: False = the camera's row-major order; True = a ray order is built on the device for this call; a RayOrder
        (of a camera that does not move relative to its rays' pattern) is reused.  The image is the same.
        samples: None = that path, one ray per pixel made on the host.  "config" (the configuration's anti-aliasing table,
        `camera.view_samples`) or an (n, 2) array of offsets in pixels: the frame goes through a DeviceView (camera needs
        view_camera()) -- rays made, traced in a device-built order (order=False: none) and resolved on the device.
        refine: with samples, a Refine: an adaptive frame (all samples only at edges); returns an AdaptiveRadiance.
        lens: with samples, a `camera.ThinLens`: depth of field -- sample k leaves the lens at `camera.lens_samples(n)[k]`; with
        refine, the lens's coc_tol and spread add the out-of-focus pixels to the refined ones."""
        if refine is not None and samples is None:
            raise ValueError("refine needs samples: there is nothing to refine with one ray per pixel")
        if lens is not None and samples is None:
            raise ValueError("a lens needs samples: one ray per pixel goes through the lens centre")
        if buffer.width != camera.width or buffer.height != camera.height:
            raise ValueError(f"buffer is {buffer.width}x{buffer.height}, the camera renders {camera.width}x{camera.height}")
        ds = self.device_scene(scene)
        if samples is not None:
            from . import camera as _camera

            if isinstance(order, RayOrder):
                raise ValueError("a view builds its own ray order: order must be True or False with samples")
            smp = _camera.view_samples(self.cfg, _abi.RT_VIEW_PINHOLE) if isinstance(samples, str) and samples == "config" else samples
            view = DeviceView(ds.device, camera.width, camera.height, smp, order="once" if order else "none", camera=camera.view_camera(),
                              lens_samples=None if lens is None else _camera.lens_samples(len(smp)), lens=lens)
            try:
                if refine is not None:
                    view.enable_adaptive()
                out = ds.render_view(view, self.cfg, tuning=tuning, traversal=self.traversal, argb=buffer.buffer, refine=refine)
            finally:
                view.close()
            self.last_stats = ds.last_trace_stats
            return out
        o, d = camera.rays()
        out = ds.trace_rays(o, d, self.cfg, tuning=tuning, traversal=self.traversal, argb=buffer.buffer, order=order or None)
        self.last_stats = ds.last_trace_stats
        return out

    def render_progressive(self, buffer: ImageBuffer, scene, on_tiles=None, rows_per_step: Optional[int] = None, poll_s: float = 0.0002,
                           tuning: Optional[Dict] = None):
        """Progressive display (reference: the render thread fills the shared u32 buffer tile by tile while the window loop
        keeps showing it, src/main.rs:327-347, renderer/mod.rs:84-209): `rt_render_begin` starts the library's render thread,
        which renders the frame in bands of `rows_per_step` tile rows (default: one row of RENDER_STRIDE tiles); this thread --
        the viewer's side -- polls, and `on_tiles(buffer, (x0, y0, w, h))` is called for every band once its rows have landed
        in `buffer` (rows below are still the caller's fill at that moment).  The final buffer equals one `render` call.
        Returns the number of bands."""
        import time

        cfg = self.cfg
        if buffer.width != cfg.width or buffer.height != cfg.height:
            raise ValueError(f"buffer is {buffer.width}x{buffer.height}, config renders {cfg.width}x{cfg.height}")
        step = cfg.render_stride * (rows_per_step if rows_per_step else 1)
        ds = self.device_scene(scene)
        p, keep = _abi.make_params(cfg, traversal=self.traversal, tuning=tuning)
        lib = _lib.load()
        h = C.c_void_p()
        _lib.check(lib.rt_render_begin(ds.handle, C.byref(p), buffer.buffer.ctypes.data, int(step), C.byref(h)))
        rows, fin, reported = C.c_uint32(0), C.c_int(0), 0
        n_bands = -(-cfg.height // step)
        try:
            while True:
                _lib.check(lib.rt_render_poll(h, C.byref(rows), C.byref(fin)))
                while reported < n_bands and min((reported + 1) * step, cfg.height) <= rows.value:
                    if on_tiles is not None:
                        on_tiles(buffer, (0, reported * step, cfg.width, min(step, cfg.height - reported * step)))
                    reported += 1
                if fin.value:
                    break
                time.sleep(poll_s)
        finally:
            st = _abi.rt_stats()
            rc = lib.rt_render_end(h, C.byref(st))
        _lib.check(rc)
        self.last_stats = st.as_dict()
        while reported < n_bands:  # (bands that landed between the last poll and the end)
            if on_tiles is not None:
                on_tiles(buffer, (0, reported * step, cfg.width, min(step, cfg.height - reported * step)))
            reported += 1
        return n_bands
