"""Ray sources for `DeviceScene.trace_rays`: the render's own camera rays, and a pinhole camera anywhere in the scene.
The same two cameras as `rt_view_camera`s (`view_camera`, `reference_view_camera`) make their rays on the device
(`renderer.DeviceView`), with the sample offsets of `view_samples`.

The reference has one view, fixed at compile time (`src/lib.rs:81-92`): pixel (x, y) sends a ray from
`(x * fw, y * fh, 0)` in the direction `origin - RENDER_RAY_FOCUS` (`src/renderer/mod.rs:176-180`,
`raytracer_renderer.rs:1190-1357`).  `reference_rays` restates it; `PinholeCamera` is the view the reference cannot take.
Both return `(origins, directions)` as (n, 3) float32 arrays, row-major with row 0 at the top, so ray `y * width + x`
belongs to pixel (x, y) of an `ImageBuffer`.  Directions are not normalised: the library does that, as
`Ray::new_with_mask` does (`ray.rs:52-57`)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Sequence, Tuple

import numpy as np

from . import _abi, sampling
from .config import RenderConfig


def reference_rays(cfg: RenderConfig) -> Tuple[np.ndarray, np.ndarray]:
    """The camera rays of `cfg`'s frame without anti-aliasing, computed in float32 exactly as the render does:
    origin (float(x) * fw, float(y) * fh, 0), direction origin - focus."""
    W, H = cfg.width, cfg.height
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    o = np.zeros((H * W, 3), np.float32)
    o[:, 0] = xs.ravel() * np.float32(cfg.fw)
    o[:, 1] = ys.ravel() * np.float32(cfg.fh)
    f = cfg.focus
    d = o - np.array([f.x, f.y, f.z], np.float32)
    return o, np.ascontiguousarray(d, np.float32)


def _view_camera(kind: int, **members) -> "_abi.rt_view_camera":
    c = _abi.rt_view_camera()
    c.abi_version, c.kind = _abi.RT_ABI_VERSION, kind
    for name, value in members.items():
        if np.ndim(value):
            for k in range(3):
                getattr(c, name)[k] = float(np.float32(value[k]))
        else:
            setattr(c, name, float(np.float32(value)))
    return c


def reference_view_camera(cfg: RenderConfig) -> "_abi.rt_view_camera":
    """The reference's own view (`reference_rays`) as the camera of a DeviceView: RT_VIEW_REFERENCE with cfg's focus, fw, fh."""
    f = cfg.focus
    return _view_camera(_abi.RT_VIEW_REFERENCE, focus=(f.x, f.y, f.z), fw=cfg.fw, fh=cfg.fh)


def view_samples(cfg: RenderConfig, kind: int) -> np.ndarray:
    """The configuration's anti-aliasing table as the (n, 2) float32 sample offsets of a DeviceView: `sampling.aa_offsets(cfg)`
    for RT_VIEW_REFERENCE (scene units); for RT_VIEW_PINHOLE the same offsets in pixels, divided by (fw, fh) in float32."""
    off = np.ascontiguousarray(sampling.aa_offsets(cfg), np.float32)
    if kind == _abi.RT_VIEW_REFERENCE:
        return off
    if kind != _abi.RT_VIEW_PINHOLE:
        raise ValueError(f"unknown camera kind {kind}")
    return np.ascontiguousarray(off / np.array([cfg.fw, cfg.fh], np.float32), np.float32)


def lens_samples(n: int) -> np.ndarray:
    """The (n, 2) float32 lens offsets of a thin-lens DeviceView, in unit-disk coordinates: sample 0 at the lens centre -- so
    that plane 0 of an adaptive frame is the view through it --, sample k at radius sqrt(k / n) and k golden angles: a fixed
    spiral that covers the disk evenly for every n.  Deterministic."""
    if n < 1:
        raise ValueError("n must be at least 1")
    k = np.arange(n, dtype=np.float64)
    r, phi = np.sqrt(k / n), k * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.ascontiguousarray(np.stack([r * np.cos(phi), r * np.sin(phi)], axis=1), np.float32)


@dataclass(frozen=True)
class ThinLens:
    """The lens of a thin-lens DeviceView (`rt_view_lens`): aperture is the lens radius in scene units (0: no lens),
    focus_distance the distance of the plane in focus, measured along the camera's forward axis.  coc_tol and spread belong to
    adaptive frames: a pixel whose circle of confusion exceeds coc_tol pixels is refined, together with the pixels its blur
    reaches, up to `spread` (0 .. 16) pixels away -- wider blur is cut off; coc_tol = inf leaves the mask to the refine rule."""

    aperture: float
    focus_distance: float
    coc_tol: float = float("inf")
    spread: int = 8

    def struct(self) -> "_abi.rt_view_lens":
        return _abi.rt_view_lens(_abi.RT_ABI_VERSION, int(self.spread), float(self.aperture), float(self.focus_distance), float(self.coc_tol), 0)


@dataclass(frozen=True)
class PinholeCamera:
    """A pinhole at `eye` looking at `target`; `fov_y_deg` is the angle between the top and the bottom EDGE of the image,
    pixels are square.  `up` fixes the roll: image rows run against it (row 0 is the top).  In the reference's scenes the
    image's y axis points down (`y * fh` grows with the row), so the view that matches them has up = (0, -1, 0)."""

    eye: Sequence[float]
    target: Sequence[float]
    up: Sequence[float]
    fov_y_deg: float
    width: int
    height: int

    def basis(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(right, up, forward): orthonormal, float64; right grows with the column, up against the row."""
        eye, target, up = (np.asarray(v, np.float64) for v in (self.eye, self.target, self.up))
        fwd = target - eye
        n = np.linalg.norm(fwd)
        if not n > 0.0:
            raise ValueError("eye and target coincide")
        fwd = fwd / n
        right = np.cross(fwd, up)
        n = np.linalg.norm(right)
        if not n > 1e-12 * max(np.linalg.norm(up), 1e-300):
            raise ValueError("up is parallel to the viewing direction")
        right = right / n
        return right, np.cross(right, fwd), fwd

    def direction(self, px, py) -> np.ndarray:
        """Direction (float64, not normalised, forward component 1) through the image point (px, py) in pixel units:
        (0, 0) is the top-left corner of the image, (width, height) the bottom-right one, pixel (x, y) has its centre at
        (x + 0.5, y + 0.5)."""
        if not 0.0 < self.fov_y_deg < 180.0:
            raise ValueError("fov_y_deg must lie in (0, 180)")
        right, up, fwd = self.basis()
        half = np.tan(np.radians(self.fov_y_deg) / 2.0)
        px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
        sx = (2.0 * px - self.width) / self.height * half  # square pixels: both axes in units of the image height
        sy = (self.height - 2.0 * py) / self.height * half
        return fwd + sx[..., None] * right + sy[..., None] * up

    def view_camera(self) -> "_abi.rt_view_camera":
        """This camera for a DeviceView (RT_VIEW_PINHOLE): the eye, the basis of `basis()` and tan(fov_y / 2), rounded to
        float32.  Its width and height belong to the view."""
        if not 0.0 < self.fov_y_deg < 180.0:
            raise ValueError("fov_y_deg must lie in (0, 180)")
        right, up, fwd = self.basis()
        return _view_camera(_abi.RT_VIEW_PINHOLE, eye=self.eye, right=right, up=up, forward=fwd,
                            tan_half_fov_y=np.tan(np.radians(self.fov_y_deg) / 2.0))

    def rays(self) -> Tuple[np.ndarray, np.ndarray]:
        """One ray through the centre of every pixel."""
        W, H = int(self.width), int(self.height)
        if W <= 0 or H <= 0:
            raise ValueError("empty image")
        ys, xs = np.meshgrid(np.arange(H, dtype=np.float64) + 0.5, np.arange(W, dtype=np.float64) + 0.5, indexing="ij")
        d = self.direction(xs.ravel(), ys.ravel())
        o = np.broadcast_to(np.asarray(self.eye, np.float64), d.shape)
        return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
