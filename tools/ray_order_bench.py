"""What a ray order (rt_ray_order*, rt_trace_rays_ordered_device) is worth, on the config-3 scene (semesterbild with
text.obj), one GPU, device-resident rays, every figure from the same process:

  direct / soft / realistic   the 1620 x 1350 = 2 187 000 camera rays of the frame, row-major, as a batch:
      unordered       rt_trace_rays_device as the caller's order has it (64 consecutive pixels of a row per wavefront)
      ordered         the same call through an order built once and reused
      build+trace     an order built for every call (DeviceScene.trace_rays(order=True))
      tiled           the caller permutes its own arrays into the frame's tile order (another image with soft shadows:
                      the light clouds go with the ray index -- timing only)
      frame           rt_render_device of the same frame without anti-aliasing
      build           rt_ray_order_build_device alone, and the bytes the order holds
  random              2^22 seeded unrelated rays, direct light: unordered, and ordered with origin_bits 0 (default), 5, 7

Every shape is warmed up, then timed with device events over repeated calls until at least --seconds of work.  Every
ordered result is compared with the unordered one (equal bits) before anything is timed.  Prints one JSON line; two runs
give the spread.  Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/ray_order_bench.py --seconds 0.2`.

    python tools/ray_order_bench.py [--device 0] [--seconds 1.0] [--only direct,soft,realistic,random]
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
    return round(e0.elapsed_time(e1) / reps, 4)  # ms


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--only", default="direct,soft,realistic,random")
    args = ap.parse_args()
    only = set(args.only.split(","))
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    base = RenderConfig.from_features(["high_resolution"])
    flat = scenes.semesterbild(base, "text").flatten()
    ds = DeviceScene(flat, args.device)
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    o, d = camera.reference_rays(base)
    cam_o, cam_d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    n_cam = o.shape[0]
    # the frame's launch order: super-tile (16x16) -> tile (4x4) -> pixel
    ys, xs = np.meshgrid(np.arange(base.height), np.arange(base.width), indexing="ij")
    st_x = (base.width + 15) // 16
    tile_key = (((ys // 16) * st_x + xs // 16) * 256 + ((ys % 16) // 4 * 4 + (xs % 16) // 4) * 16 + (ys % 4) * 4 + xs % 4).ravel()
    perm = torch.from_numpy(np.argsort(tile_key, kind="stable")).to(dev)
    til_o, til_d = cam_o[perm].contiguous(), cam_d[perm].contiguous()

    res = {}
    order = ds.ray_order(cam_o, cam_d)
    b = ds._batch_struct(n_cam, cam_o, cam_d, None, False, lambda a: a.data_ptr())
    info = order.info
    for name, features in (("direct", []), ("soft", ["soft_shadows"]), ("realistic", ["realistic"])):
        if name not in only:
            continue
        cfg = RenderConfig.from_features(["high_resolution"] + features)
        p, keep = _abi.make_params(cfg)
        frame = torch.zeros(n_cam, dtype=torch.int32, device=dev)
        plain = ds.trace_rays(cam_o, cam_d, cfg)
        equal = same(plain, ds.trace_rays(cam_o, cam_d, cfg, order=order)) and same(plain, ds.trace_rays(cam_o, cam_d, cfg, order=True))
        r = dict(rays=n_cam, ordered_equals_unordered=bool(equal))
        r["unordered_ms"] = time_it(lambda: ds.trace_rays(cam_o, cam_d, cfg), args.seconds)
        r["ordered_ms"] = time_it(lambda: ds.trace_rays(cam_o, cam_d, cfg, order=order), args.seconds)
        r["build_and_trace_ms"] = time_it(lambda: ds.trace_rays(cam_o, cam_d, cfg, order=True), args.seconds)
        r["tiled_ms"] = time_it(lambda: ds.trace_rays(til_o, til_d, cfg), args.seconds)
        r["frame_ms"] = time_it(lambda: _lib.check(lib.rt_render_device(ds.handle, C.byref(p), frame.data_ptr(), None, stream)), args.seconds)
        # (again, behind the others: the spread between the two is the noise inside one run)
        r["unordered_again_ms"] = time_it(lambda: ds.trace_rays(cam_o, cam_d, cfg), args.seconds)
        r["ordered_again_ms"] = time_it(lambda: ds.trace_rays(cam_o, cam_d, cfg, order=order), args.seconds)
        r["ordered_over_unordered"] = round(min(r["ordered_ms"], r["ordered_again_ms"]) / min(r["unordered_ms"], r["unordered_again_ms"]), 3)
        res[name] = r
    res["build"] = dict(rays=n_cam, build_ms=time_it(lambda: order.build(b, stream), args.seconds), **info)
    order.close()

    if "random" in only:
        pts = np.concatenate([flat.tri_v1, flat.tri_v1 + flat.tri_e1, flat.tri_v1 + flat.tri_e2,
                              flat.sphere_center - np.sqrt(flat.sphere_r_sq)[:, None], flat.sphere_center + np.sqrt(flat.sphere_r_sq)[:, None]])
        lo, hi = pts.min(axis=0), pts.max(axis=0)
        rng = np.random.default_rng(1)
        n_rand = 1 << 22
        rnd_o = torch.from_numpy((lo + rng.random((n_rand, 3)) * (hi - lo)).astype(np.float32)).to(dev)
        v = rng.standard_normal((n_rand, 3))
        rnd_d = torch.from_numpy((v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)).to(dev)
        cfg = RenderConfig.from_features(["high_resolution"])
        plain = ds.trace_rays(rnd_o, rnd_d, cfg)
        r = dict(rays=n_rand, unordered_ms=time_it(lambda: ds.trace_rays(rnd_o, rnd_d, cfg), args.seconds))
        rb = ds._batch_struct(n_rand, rnd_o, rnd_d, None, False, lambda a: a.data_ptr())
        for bits in (0, 5, 7):
            ro = ds.ray_order(rnd_o, rnd_d, origin_bits=bits)
            i = ro.info
            r[f"origin_bits_{bits}"] = dict(ordered_ms=time_it(lambda: ds.trace_rays(rnd_o, rnd_d, cfg, order=ro), args.seconds),
                                            build_ms=time_it(lambda: ro.build(rb, stream), args.seconds),
                                            equals_unordered=bool(same(plain, ds.trace_rays(rnd_o, rnd_d, cfg, order=ro))),
                                            split=[i["n_origin_axes"], i["origin_bits"], i["n_direction_axes"], i["direction_bits"]])
            torch.cuda.synchronize()
            ro.close()
        res["random"] = r
    torch.cuda.synchronize()
    print(json.dumps(dict(metric="ray orders: ms per batch (device-resident rays, config-3 scene, text.obj)", gpu=torch.cuda.get_device_name(dev),
                          build_id=lib.rt_build_id().decode(), workloads=res)))
    ds.close()


if __name__ == "__main__":
    main()
