"""Throughput of the multi-hit ray query (rt_list_intersections_device) on semesterbild with text, one GPU, device-resident
rays, the two batches of tools/query_bench.py:

  camera   the 1620 x 1350 = 2 187 000 camera rays of a frame without anti-aliasing (config 3's rays)
  random   2^22 seeded rays, origins uniform in the scene's bounding box, directions uniform on the sphere

For each batch: rt_list_intersections_device at max_hits 1, 4 and 16, with every plane, with and without `total`;
count_intersections (total alone); rt_cast_rays_device on the same batch as the yardstick; the histogram of hits per ray and
the share of rays that needed a second pass for `total` at each K (total >= K).  Every shape is warmed up, then timed with
device events over repeated launches until at least --seconds of work.  Prints one JSON line.

    python tools/multi_hit_bench.py [--device 0] [--seconds 0.5] [--scene text]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--scene", default="text", choices=("text", "text_lowres"))
    args = ap.parse_args()
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    cfg = RenderConfig.from_features(["high_resolution", "anti_aliasing", "soft_shadows"])
    flat = scenes.semesterbild(cfg, args.scene).flatten()
    ds = DeviceScene(flat, args.device)

    W, H = cfg.width, cfg.height
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    o = np.zeros((H * W, 3), np.float32)
    o[:, 0], o[:, 1] = xs.ravel() * np.float32(cfg.fw), ys.ravel() * np.float32(cfg.fh)
    f = cfg.focus
    cam_o = torch.from_numpy(o).to(dev)
    cam_d = torch.from_numpy(o - np.array([f.x, f.y, f.z], np.float32)).to(dev)
    pts = np.concatenate([flat.tri_v1, flat.tri_v1 + flat.tri_e1, flat.tri_v1 + flat.tri_e2,
                          flat.sphere_center - np.sqrt(flat.sphere_r_sq)[:, None], flat.sphere_center + np.sqrt(flat.sphere_r_sq)[:, None]])
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    rng = np.random.default_rng(1)
    n_rand = 1 << 22
    rnd_o = torch.from_numpy((lo + rng.random((n_rand, 3)) * (hi - lo)).astype(np.float32)).to(dev)
    v = rng.standard_normal((n_rand, 3))
    rnd_d = torch.from_numpy((v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)).to(dev)

    out = {}
    for batch, ro, rd in (("camera", cam_o, cam_d), ("random", rnd_o, rnd_d)):
        n = int(ro.shape[0])
        res = {"rays": n}
        sec, reps = time_it(lambda: ds.cast_rays(ro, rd), args.seconds)
        res["cast_rays"] = dict(ms=round(sec * 1e3, 4), mrays_per_s=round(n / sec / 1e6, 1), reps=reps)
        total = ds.count_intersections(ro, rd)
        torch.cuda.synchronize()
        hist = torch.bincount(total.to(torch.int64)).cpu().numpy()
        res["hits_per_ray_histogram"] = [int(c) for c in hist]
        res["mean_hits_per_ray"] = round(float(total.float().mean()), 4)
        sec, reps = time_it(lambda: ds.count_intersections(ro, rd), args.seconds)
        res["count_intersections"] = dict(ms=round(sec * 1e3, 4), mrays_per_s=round(n / sec / 1e6, 1), reps=reps)
        for k in (1, 4, 16):
            for with_total in (False, True):
                sec, reps = time_it(lambda: ds.list_intersections(ro, rd, max_hits=k, total=with_total), args.seconds)
                res[f"K{k}{'_total' if with_total else ''}"] = dict(ms=round(sec * 1e3, 4), mrays_per_s=round(n / sec / 1e6, 1), reps=reps,
                                                                    vs_cast_rays=round(sec * 1e3 / res["cast_rays"]["ms"], 3))
            res[f"K{k}_second_pass_share"] = round(float((total >= k).float().mean()), 4)
        out[batch] = res
    ds.close()
    print(json.dumps(dict(metric="multi-hit ray queries, Mray/s (device-resident rays, every plane written)", gpu=torch.cuda.get_device_name(dev),
                          library=os.path.basename(_lib.LIB_PATH), scene=args.scene, n_triangles=flat.n_triangles, n_spheres=flat.n_spheres,
                          batches=out)))


if __name__ == "__main__":
    main()
