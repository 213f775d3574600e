"""Throughput of the radiance queries (rt_trace_rays_device) on the config-3 scene (semesterbild with text.obj), one GPU,
device-resident rays, next to rt_render_device of the SAME frame without anti-aliasing in the same process:

  direct     the 1620 x 1350 = 2 187 000 camera rays of the frame as a batch, direct light only
  soft       the same with soft shadows (10 samples per light)
  realistic  the same with reflections and refractions (no soft shadows)
  tiled      `direct` and `soft` again with the rays permuted into the frame's own launch order (16x16 super-tiles of 4x4
             tiles): what the order of the caller's rays is worth
  random     2^22 seeded rays, origins uniform in the scene's bounding box, directions uniform on the sphere, direct light

The batch and the frame compute the same colours (tests/test_trace_rays_gpu.py), so the ratio batch / frame is what the
caller's rays cost over the library's own: 24 bytes in and up to 33 bytes out per ray, the linear ray order instead of
the frame's 16x16 super-tiles, and -- with secondary rays -- the chained level schedule and the verification of every
batch, where a frame of a verified shape runs merged levels without waiting.  Every shape is warmed up, then timed with
device events over repeated calls until at least --seconds of work.  Prints one JSON line.  Kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python tools/trace_rays_bench.py`.

    python tools/trace_rays_bench.py [--device 0] [--seconds 1.0]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import torch  # (before the library: one HIP runtime in the process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, _abi, _lib, camera, scenes  # noqa: E402
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
    base = RenderConfig.from_features(["high_resolution"])
    flat = scenes.semesterbild(base, "text").flatten()
    ds = DeviceScene(flat, args.device)
    lib = _lib.load()

    o, d = camera.reference_rays(base)
    cam_o, cam_d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    n_cam = o.shape[0]
    pts = np.concatenate([flat.tri_v1, flat.tri_v1 + flat.tri_e1, flat.tri_v1 + flat.tri_e2,
                          flat.sphere_center - np.sqrt(flat.sphere_r_sq)[:, None], flat.sphere_center + np.sqrt(flat.sphere_r_sq)[:, None]])
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    rng = np.random.default_rng(1)
    n_rand = 1 << 22
    rnd_o = torch.from_numpy((lo + rng.random((n_rand, 3)) * (hi - lo)).astype(np.float32)).to(dev)
    v = rng.standard_normal((n_rand, 3))
    rnd_d = torch.from_numpy((v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)).to(dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    # the frame's launch order: super-tile (16x16) -> tile (4x4) -> pixel
    ys, xs = np.meshgrid(np.arange(base.height), np.arange(base.width), indexing="ij")
    st_x = (base.width + 15) // 16
    tile_key = (((ys // 16) * st_x + xs // 16) * 256 + ((ys % 16) // 4 * 4 + (xs % 16) // 4) * 16 + (ys % 4) * 4 + xs % 4).ravel()
    perm = torch.from_numpy(np.argsort(tile_key, kind="stable")).to(dev)
    til_o, til_d = cam_o[perm].contiguous(), cam_d[perm].contiguous()

    res = {}
    for name, features in (("direct", []), ("soft", ["soft_shadows"]), ("realistic", ["realistic"])):
        cfg = RenderConfig.from_features(["high_resolution"] + features)
        p, keep = _abi.make_params(cfg)
        frame = torch.zeros(n_cam, dtype=torch.int32, device=dev)
        batch_argb = torch.zeros(n_cam, dtype=torch.int32, device=dev)

        def run_frame():
            _lib.check(lib.rt_render_device(ds.handle, C.byref(p), frame.data_ptr(), None, stream))

        def run_batch():
            return ds.trace_rays(cam_o, cam_d, cfg, argb=batch_argb)

        sec_b, reps_b = time_it(run_batch, args.seconds)
        sec_f, reps_f = time_it(run_frame, args.seconds)
        sec_b2, _ = time_it(run_batch, args.seconds)  # (again, behind the frame: the spread between the two is the noise)
        out = run_batch()
        torch.cuda.synchronize()
        res[name] = dict(rays=n_cam, batch_ms=round(sec_b * 1e3, 4), batch_again_ms=round(sec_b2 * 1e3, 4), frame_ms=round(sec_f * 1e3, 4),
                         batch_over_frame=round(min(sec_b, sec_b2) / sec_f, 3), mrays_per_s=round(n_cam / min(sec_b, sec_b2) / 1e6, 1),
                         reps=[reps_b, reps_f], valid_fraction=round(float(out.valid.float().mean()), 4),
                         argb_equals_frame=bool(torch.equal(batch_argb, frame)))
        if name != "realistic":
            # (the light clouds go with the ray index, so the permuted soft batch is another image: timing only)
            sec_t, reps_t = time_it(lambda: ds.trace_rays(til_o, til_d, cfg), args.seconds)
            res[name].update(tiled_ms=round(sec_t * 1e3, 4), tiled_over_frame=round(sec_t / sec_f, 3))
    cfg = RenderConfig.from_features(["high_resolution"])
    sec, reps = time_it(lambda: ds.trace_rays(rnd_o, rnd_d, cfg), args.seconds)
    out = ds.trace_rays(rnd_o, rnd_d, cfg)
    torch.cuda.synchronize()
    res["random"] = dict(rays=n_rand, batch_ms=round(sec * 1e3, 4), mrays_per_s=round(n_rand / sec / 1e6, 1), reps=reps,
                         valid_fraction=round(float(out.valid.float().mean()), 4))
    print(json.dumps(dict(metric="radiance queries: ms per batch, batch / frame, Mray/s (device-resident rays, config-3 scene, text.obj)",
                          gpu=torch.cuda.get_device_name(dev), n_triangles=flat.n_triangles, n_spheres=flat.n_spheres,
                          n_lights=int(flat.lights.reshape(-1, 7).shape[0]), workloads=res)))
    ds.close()


if __name__ == "__main__":
    main()
