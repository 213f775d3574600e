"""A frame of semesterbild shaded by ambient occlusion alone: the frame's camera rays (no anti-aliasing) are cast with
DeviceScene.cast_rays, their hit points and normals -- turned towards the camera -- go into DeviceScene.ambient_occlusion as they
are, and every pixel is its `visibility` as a grey value (a pixel whose ray hit nothing is black).  Writes a PNG.

    render_ao.py OUT.png [--samples 64] [--max-distance FRACTION_OF_EXTENT] [--model text|text_lowres] [--high-resolution] [--device 0]
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from PIL import Image  # noqa: E402

from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, scenes  # noqa: E402
from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceScene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--max-distance", type=float, default=0.0, help="as a fraction of the scene's extent (0: +inf)")
    ap.add_argument("--model", default="text_lowres", choices=("text", "text_lowres"))
    ap.add_argument("--high-resolution", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    cfg = RenderConfig.from_features(["high_resolution"] if args.high_resolution else [])
    flat = scenes.semesterbild(cfg, args.model).flatten()
    W, H = cfg.width, cfg.height
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    o = np.zeros((H * W, 3), np.float32)
    o[:, 0], o[:, 1] = xs.ravel() * np.float32(cfg.fw), ys.ravel() * np.float32(cfg.fh)
    f = cfg.focus
    d = o - np.array([f.x, f.y, f.z], np.float32)
    pts = np.concatenate([flat.tri_v1, flat.tri_v1 + flat.tri_e1, flat.tri_v1 + flat.tri_e2,
                          flat.sphere_center - np.sqrt(flat.sphere_r_sq)[:, None], flat.sphere_center + np.sqrt(flat.sphere_r_sq)[:, None]])
    extent = float(np.linalg.norm(pts.max(axis=0) - pts.min(axis=0)))
    ds = DeviceScene(flat, args.device)
    try:
        hits = ds.cast_rays(o, d)
        away = np.einsum("ij,ij->i", hits.normal, d) > 0
        normal = np.where(away[:, None], -hits.normal, hits.normal)
        ao = ds.ambient_occlusion(hits.point, normal, samples=args.samples,
                                  max_distance=args.max_distance * extent if args.max_distance > 0 else float("inf"))
    finally:
        ds.close()
    grey = np.where(hits.id >= 0, ao.visibility, 0.0).reshape(H, W)
    Image.fromarray((np.clip(grey, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8), mode="L").save(args.out)
    print(f"{args.out}: {W}x{H}, {int((hits.id >= 0).sum())} hit pixels, mean visibility {float(ao.visibility[hits.id >= 0].mean()):.3f}")


if __name__ == "__main__":
    main()
