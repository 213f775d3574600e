"""Time of the ambient-occlusion query (rt_ambient_occlusion_device) on semesterbild with text, one GPU, device-resident inputs,
against the route the library offered before it: the same rays made in torch on the device from the definition's formulas,
rt_any_intersection_device on all n x S of them, and a torch reduction.

  camera   the primary hits of the 1620 x 1350 = 2 187 000 camera rays of a frame without anti-aliasing (config 3's rays): the
           point and normal planes of cast_rays as they are (a miss is a dead point)
  random   2^20 seeded free-space points in the scene's bounding box with random normals

For each batch, S = 16 and 64, max_distance = +inf and a tenth of the scene's extent: the new call (clear, visibility and bent
normal written; the bit plane as well in a second figure); the baseline's any-hit kernel ALONE on rays made beforehand; the whole
baseline route.  Every shape is warmed up; every figure is the median of --runs runs, each between two device events, with the
smallest and the largest beside it.  The new call's `clear` is compared with the baseline's (torch's float32 formulas are not
the single-rounding ones, so a few rays at an edge may differ; the count is reported).  Prints one JSON line.

    python tools/occlusion_bench.py [--device 0] [--runs 9] [--scene text] [--points N]
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

from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, _lib, sampling, scenes  # noqa: E402
from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceScene  # noqa: E402


def timed(fn, runs):
    fn()
    fn()  # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return dict(median_ms=round(ms[len(ms) // 2], 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4), runs=runs)


def make_rays(p, nrm, tab, bias):
    """the definition's rays in torch: (n S, 3) origins and world directions"""
    n = nrm / nrm.norm(dim=1, keepdim=True)
    sg = torch.copysign(torch.ones_like(n[:, 2]), n[:, 2])
    a = -1.0 / (sg + n[:, 2])
    b = n[:, 0] * n[:, 1] * a
    tx = torch.stack([1.0 + sg * n[:, 0] * n[:, 0] * a, sg * b, -sg * n[:, 0]], dim=1)
    ty = torch.stack([b, sg + n[:, 1] * n[:, 1] * a, -n[:, 1]], dim=1)
    o = p + n * bias
    w = tab[None, :, 0:1] * tx[:, None, :] + tab[None, :, 1:2] * ty[:, None, :] + tab[None, :, 2:3] * n[:, None, :]
    s = tab.shape[0]
    return o[:, None, :].expand(-1, s, -1).reshape(-1, 3).contiguous(), w.reshape(-1, 3)


def reduce_any(has, w, n, s):
    """clear, visibility and bent normal from the any-hit plane of the n S rays"""
    open_ = ~has.view(n, s)
    clear = open_.sum(dim=1, dtype=torch.int32)
    u = w / w.norm(dim=1, keepdim=True)
    bent = (u.view(n, s, 3) * open_[:, :, None]).sum(dim=1)
    return clear, clear.float() / s, bent / bent.norm(dim=1, keepdim=True).clamp_min(1e-30)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--scene", default="text", choices=("text", "text_lowres"))
    ap.add_argument("--points", type=int, default=0, help="use only the first N points of each batch (0: all)")
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
    hits = ds.cast_rays(torch.from_numpy(o).to(dev), torch.from_numpy(o - np.array([f.x, f.y, f.z], np.float32)).to(dev))
    pts = np.concatenate([flat.tri_v1, flat.tri_v1 + flat.tri_e1, flat.tri_v1 + flat.tri_e2,
                          flat.sphere_center - np.sqrt(flat.sphere_r_sq)[:, None], flat.sphere_center + np.sqrt(flat.sphere_r_sq)[:, None]])
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    extent = float(np.linalg.norm(hi - lo))
    rng = np.random.default_rng(1)
    n_rand = 1 << 20
    rnd_p = torch.from_numpy((lo + rng.random((n_rand, 3)) * (hi - lo)).astype(np.float32)).to(dev)
    rnd_n = torch.from_numpy(rng.standard_normal((n_rand, 3)).astype(np.float32)).to(dev)
    bias = 1e-4

    out = {}
    for batch, p, nrm in (("camera", hits.point, hits.normal), ("random", rnd_p, rnd_n)):
        if args.points:
            p, nrm = p[:args.points].contiguous(), nrm[:args.points].contiguous()
        n = int(p.shape[0])
        res = {"points": n}
        if batch == "camera":
            res["primary_hits"] = int((hits.id[:n] >= 0).sum())
        for s in (16, 64):
            tab = torch.from_numpy(sampling.hemisphere_samples(s)).to(dev)
            for kind, max_d in (("inf", float("inf")), ("tenth", 0.1 * extent)):
                new = timed(lambda: ds.ambient_occlusion(p, nrm, samples=s, table=tab, bias=bias, max_distance=max_d), args.runs)
                new_bits = timed(lambda: ds.ambient_occlusion(p, nrm, samples=s, table=tab, bias=bias, max_distance=max_d, bits=True), args.runs)
                ro, rd = make_rays(p, nrm, tab, bias)
                rm = torch.full((n * s,), max_d, dtype=torch.float32, device=dev)
                any_alone = timed(lambda: ds.any_intersection(ro, rd, rm), args.runs)

                def route():
                    qo, qd = make_rays(p, nrm, tab, bias)
                    qm = torch.full((n * s,), max_d, dtype=torch.float32, device=dev)
                    return reduce_any(ds.any_intersection(qo, qd, qm).has_intersection, qd, n, s)

                whole = timed(route, max(3, args.runs // 3))
                got = ds.ambient_occlusion(p, nrm, samples=s, table=tab, bias=bias, max_distance=max_d)
                base_clear = route()[0]
                live = torch.isfinite(nrm).all(dim=1) & (nrm != 0).any(dim=1) & torch.isfinite(p).all(dim=1)
                differ = int(((got.clear != base_clear) & live).sum())
                occluded = 1.0 - float(got.clear[live].float().mean()) / s if bool(live.any()) else 0.0
                del ro, rd, rm
                res[f"S{s}_{kind}"] = dict(rays=n * s, new=new, new_with_bits=new_bits, baseline_any_hit_alone=any_alone, baseline_whole_route=whole,
                                           new_over_any_hit_alone=round(new["median_ms"] / any_alone["median_ms"], 4),
                                           new_over_whole_route=round(new["median_ms"] / whole["median_ms"], 4),
                                           grays_per_s=round(n * s / new["median_ms"] / 1e6, 2), occluded_share=round(occluded, 4),
                                           points_whose_clear_differs_from_the_torch_route=differ)
        out[batch] = res
    ds.close()
    print(json.dumps(dict(metric="ambient occlusion, ms per call (device-resident inputs; median, min, max of repeated runs)", gpu=torch.cuda.get_device_name(dev),
                          library=os.path.basename(_lib.LIB_PATH), scene=args.scene, n_triangles=flat.n_triangles, n_spheres=flat.n_spheres,
                          extent=round(extent, 4), batches=out)))


if __name__ == "__main__":
    main()
