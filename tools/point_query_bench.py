"""Throughput of the closest-point query (rt_closest_points_device) on test_scene, text_lowres and text (semesterbild), one
GPU, device-resident points, three batches per scene:

  random   2^20 seeded points uniform in the scene's bounding box
  grid     a 128^3 grid over that box (x fastest: neighbouring lanes are neighbouring points)
  surface  the hit points of rt_cast_rays on the random rays below, each jittered by up to 1e-3 extents: points near the surface

and, as a yardstick, rt_cast_rays on 2^20 random rays (origins uniform in the box, directions uniform on the sphere).
Every shape is warmed up, then timed with device events over repeated launches until at least --seconds of work.
Prints one JSON line.  RT_HIP_LIB selects another build of the library (an A/B, as the seed's in profiles/point_query.md).

    python tools/point_query_bench.py [--device 0] [--seconds 0.5]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch  # (before the library: one HIP runtime in the process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, _lib, scenes  # noqa: E402
from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceScene  # noqa: E402


def time_it(fn, seconds):
    fn()
    fn()  # warm-up
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    one = e0.elapsed_time(e1) / 1e3
    reps = max(3, int(np.ceil(seconds / max(one, 1e-6))))
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / 1e3 / reps, reps


def flat_of(name):
    if name == "test_scene":
        return scenes.test_scene(RenderConfig.from_features([])).flatten()
    return scenes.semesterbild(RenderConfig.from_features(["high_resolution", "anti_aliasing", "soft_shadows"]), name).flatten()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--seconds", type=float, default=0.5)
    args = ap.parse_args()
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    out = {}
    for name in ("test_scene", "text_lowres", "text"):
        flat = flat_of(name)
        ds = DeviceScene(flat, args.device)
        r = np.sqrt(flat.sphere_r_sq)[:, None]
        pts = np.concatenate([flat.tri_v1, flat.tri_v1 + flat.tri_e1, flat.tri_v1 + flat.tri_e2, flat.sphere_center - r, flat.sphere_center + r])
        lo, hi = pts.min(axis=0).astype(np.float64), pts.max(axis=0).astype(np.float64)
        ext = float(np.linalg.norm(hi - lo))
        rng = np.random.default_rng(1)
        n = 1 << 20
        rnd = torch.from_numpy((lo + rng.random((n, 3)) * (hi - lo)).astype(np.float32)).to(dev)
        g = np.linspace(0.0, 1.0, 128)
        zz, yy, xx = np.meshgrid(g, g, g, indexing="ij")
        grid = torch.from_numpy((lo + np.stack([xx.ravel(), yy.ravel(), zz.ravel()], axis=1) * (hi - lo)).astype(np.float32)).to(dev)
        v = rng.standard_normal((n, 3))
        ray_d = torch.from_numpy((v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)).to(dev)
        hits = ds.cast_rays(rnd, ray_d)
        torch.cuda.synchronize()
        on = hits.point[hits.id >= 0]
        jit = torch.from_numpy(rng.uniform(-1e-3 * ext, 1e-3 * ext, (on.shape[0], 3)).astype(np.float32)).to(dev)
        surf = (on + jit).contiguous()
        res = {}
        for what, p in (("random", rnd), ("grid", grid), ("surface", surf)):
            sec, reps = time_it(lambda: ds.closest_points(p), args.seconds)
            c = ds.closest_points(p)
            torch.cuda.synchronize()
            res[what] = dict(points=int(p.shape[0]), ms=round(sec * 1e3, 4), mpoints_per_s=round(p.shape[0] / sec / 1e6, 1), reps=reps,
                             mean_distance_in_extents=round(float(c.distance.mean()) / ext, 5), on_triangles=round(float((c.id >= flat.n_spheres).float().mean()), 4))
        sec, reps = time_it(lambda: ds.cast_rays(rnd, ray_d), args.seconds)
        res["cast_rays_random"] = dict(rays=n, ms=round(sec * 1e3, 4), mrays_per_s=round(n / sec / 1e6, 1), reps=reps,
                                       hit_fraction=round(float((hits.id >= 0).float().mean()), 4))
        out[name] = dict(n_triangles=flat.n_triangles, n_spheres=flat.n_spheres, **res)
        ds.close()
    print(json.dumps(dict(metric="closest-point queries, Mpoint/s (device-resident points)", gpu=torch.cuda.get_device_name(dev),
                          library=os.path.basename(_lib.LIB_PATH), scenes=out)))


if __name__ == "__main__":
    main()
