"""Throughput of the ray queries (rt_cast_rays_device / rt_any_intersection_device) on the config-3 scene (semesterbild with
text.obj), one GPU, device-resident rays:

  camera     the 1620 x 1350 = 2 187 000 camera rays of a frame without anti-aliasing (origin (x fw, y fh, 0), direction
             origin - focus): nearest hit
  random     2^22 seeded rays, origins uniform in the scene's bounding box, directions uniform on the sphere: nearest hit
  occlusion  from the hits of `camera` to every light, the origin pushed by eps_distance as the render does it: any hit

Every shape is warmed up, then timed with device events over repeated launches until at least --seconds of work.
Prints one JSON line.  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/query_bench.py`.

    python tools/query_bench.py [--device 0] [--seconds 1.0]
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

from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, scenes  # noqa: E402
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
    ap.add_argument("--seconds", type=float, default=1.0)
    args = ap.parse_args()
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    cfg = RenderConfig.from_features(["high_resolution", "anti_aliasing", "soft_shadows"])
    flat = scenes.semesterbild(cfg, "text").flatten()
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

    hits = ds.cast_rays(cam_o, cam_d)
    torch.cuda.synchronize()
    p = hits.point[hits.id >= 0]
    L = torch.from_numpy(flat.lights.reshape(-1, 7)[:, :3].astype(np.float32)).to(dev)
    lp = L[None].expand(p.shape[0], -1, -1).reshape(-1, 3)
    pp = p[:, None].expand(-1, L.shape[0], -1).reshape(-1, 3)
    ltp = lp - pp
    ld = ltp / torch.linalg.norm(ltp, dim=1, keepdim=True)
    sh_o = (pp + ld * float(cfg.eps_distance)).contiguous()
    sh_d = ld.contiguous()
    sh_m = torch.linalg.norm(lp - sh_o, dim=1).contiguous()

    res = {}
    for name, n, fn in (
        ("camera", cam_o.shape[0], lambda: ds.cast_rays(cam_o, cam_d)),
        ("random", n_rand, lambda: ds.cast_rays(rnd_o, rnd_d)),
        ("occlusion", sh_o.shape[0], lambda: ds.any_intersection(sh_o, sh_d, sh_m)),
    ):
        sec, reps = time_it(fn, args.seconds)
        res[name] = dict(rays=int(n), ms=round(sec * 1e3, 4), mrays_per_s=round(n / sec / 1e6, 1), reps=reps)
    occ = ds.any_intersection(sh_o, sh_d, sh_m)
    torch.cuda.synchronize()
    res["camera"]["hit_fraction"] = round(float((hits.id >= 0).float().mean()), 4)
    res["random"]["hit_fraction"] = round(float((ds.cast_rays(rnd_o, rnd_d).id >= 0).float().mean()), 4)
    res["occlusion"]["occluded_fraction"] = round(float(occ.completely_occluded.float().mean()), 4)
    print(json.dumps(dict(metric="ray queries, Mray/s (device-resident rays, config-3 scene, text.obj)", gpu=torch.cuda.get_device_name(dev),
                          n_triangles=flat.n_triangles, n_spheres=flat.n_spheres, n_lights=int(L.shape[0]), workloads=res)))
    ds.close()


if __name__ == "__main__":
    main()
