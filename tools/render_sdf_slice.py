"""One z-slice of the signed distance field of semesterbild: a regular grid of points on the plane z = lo + FRACTION (hi - lo) of
the scene's bounds goes into DeviceScene.signed_distance, and every pixel is its distance -- blue inside, red outside, darker
with distance, white at the surface -- with the points whose directions DISAGREE (votes not 0 and not R: on or near a surface, or
beside an open or inconsistently oriented one, as the letters of the text meshes are) marked green.  Writes a PNG.

    render_sdf_slice.py OUT.png [--z 0.5] [--size 512] [--model text|text_lowres] [--rule parity|winding] [--device 0]
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from PIL import Image  # noqa: E402

from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, sampling, scenes  # noqa: E402
from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceScene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--z", type=float, default=0.5, help="height of the slice as a fraction of the bounds' z range")
    ap.add_argument("--size", type=int, default=512, help="pixels along x; y follows the bounds' aspect")
    ap.add_argument("--model", default="text_lowres", choices=("text", "text_lowres"))
    ap.add_argument("--rule", default="parity", choices=("parity", "winding"))
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    cfg = RenderConfig.from_features([])
    flat = scenes.semesterbild(cfg, args.model).flatten()
    pts = np.concatenate([flat.tri_v1, flat.tri_v1 + flat.tri_e1, flat.tri_v1 + flat.tri_e2,
                          flat.sphere_center - np.sqrt(flat.sphere_r_sq)[:, None], flat.sphere_center + np.sqrt(flat.sphere_r_sq)[:, None]])
    lo, hi = pts.min(axis=0).astype(np.float64), pts.max(axis=0).astype(np.float64)
    W = args.size
    H = max(1, int(round(W * (hi[1] - lo[1]) / (hi[0] - lo[0]))))
    z = lo[2] + args.z * (hi[2] - lo[2])
    p = sampling.grid_points((lo[0], lo[1], z), (hi[0], hi[1], z), (W, H, 1))  # x slowest
    r = sampling.solid_directions().shape[0]
    ds = DeviceScene(flat, args.device)
    try:
        sd = ds.signed_distance(p, rule=args.rule)
    finally:
        ds.close()
    d = sd.distance.reshape(W, H).T  # rows are y
    mixed = ((sd.votes != 0) & (sd.votes != r)).reshape(W, H).T
    scale = float(np.abs(d[np.isfinite(d)]).max()) or 1.0
    shade = 1.0 - 0.85 * np.clip(np.abs(d) / scale, 0.0, 1.0) ** 0.5
    rgb = np.zeros((H, W, 3))
    rgb[..., 0] = np.where(d < 0, 0.25, 1.0) * shade
    rgb[..., 1] = np.where(d < 0, 0.45, 0.35) * shade
    rgb[..., 2] = np.where(d < 0, 1.0, 0.25) * shade
    rgb[np.abs(d) < 0.004 * scale] = 1.0
    rgb[mixed] = (0.1, 0.9, 0.2)
    Image.fromarray((np.clip(rgb, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)[::-1], mode="RGB").save(args.out)
    print(f"{args.out}: {W}x{H} at z = {z:.4f}, {int(sd.inside.sum())} points inside, {int(mixed.sum())} with disagreeing directions, "
          f"distances {float(d.min()):.4f} .. {float(d.max()):.4f}")


if __name__ == "__main__":
    main()
