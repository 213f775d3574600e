"""Time of the containment and signed-distance queries (rt_contains_points_device, rt_signed_distance_device) on semesterbild with
text, one GPU, device-resident inputs, against the route the library offered before them: rt_list_intersections_device with the
`total` plane alone on the n x R rays, `& 1` in torch, rt_closest_points_device and a torch `where`.  (That route is WRONG for
spheres: a ray gets one hit from inside a sphere and one from outside.  It is timed, and its disagreement is counted.)

  grid     the 128^3 = 2 097 152 points of a regular grid over the scene's bounds
  random   2^20 seeded points in the bounds

For each batch, with the default R = 3 table: the new contains call; the new signed_distance call; the old route's counting kernel
ALONE on rays made beforehand; rt_closest_points_device alone; the torch glue alone (making the rays, the parity, the where); the
whole old route.  Then contains at R = 1, 3 and 8.  Every shape is warmed up; every figure is the median of --runs runs, each
between two device events, with the smallest and the largest beside it; the new call and the old kernel are timed ALTERNATELY in
one loop, so that they see the same machine.  Prints one JSON line.

    python tools/solid_bench.py [--device 0] [--runs 9] [--scene text] [--points N]
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


def summary(ms):
    ms = sorted(ms)
    return dict(median_ms=round(ms[len(ms) // 2], 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4), runs=len(ms))


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed(runs, *fns):
    """the calls timed alternately: run k times fns[0], fns[1], ... in turn -> one summary per call"""
    for fn in fns:
        fn()
        fn()  # warm-up
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(runs):
        for k, fn in enumerate(fns):
            ms[k].append(once(fn))
    return [summary(m) for m in ms]


def make_rays(p, table):
    """(n R, 3) origins and directions of the old route"""
    r = table.shape[0]
    return p[:, None, :].expand(-1, r, -1).reshape(-1, 3).contiguous(), table[None].expand(p.shape[0], -1, -1).reshape(-1, 3).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--scene", default="text", choices=("text", "text_lowres"))
    ap.add_argument("--points", type=int, default=0, help="use only the first N points of each batch (0: all)")
    ap.add_argument("--grid", type=int, default=128, help="points per axis of the grid batch")
    args = ap.parse_args()
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    cfg = RenderConfig.from_features(["high_resolution", "anti_aliasing", "soft_shadows"])
    flat = scenes.semesterbild(cfg, args.scene).flatten()
    ds = DeviceScene(flat, args.device)
    pts = np.concatenate([flat.tri_v1, flat.tri_v1 + flat.tri_e1, flat.tri_v1 + flat.tri_e2,
                          flat.sphere_center - np.sqrt(flat.sphere_r_sq)[:, None], flat.sphere_center + np.sqrt(flat.sphere_r_sq)[:, None]])
    lo, hi = pts.min(axis=0).astype(np.float64), pts.max(axis=0).astype(np.float64)
    rng = np.random.default_rng(1)
    batches = (("grid", sampling.grid_points(lo, hi, (args.grid,) * 3)), ("random", (lo + rng.random((1 << 20, 3)) * (hi - lo)).astype(np.float32)))
    default = sampling.solid_directions()
    tables = {1: default[:1], 3: default, 8: np.concatenate([default, -default, np.array([(3, 1, -2), (-1, 3, 2)], np.float32)])}

    out = {}
    for batch, host_p in batches:
        p = torch.from_numpy(host_p[:args.points] if args.points else host_p).to(dev).contiguous()
        n = int(p.shape[0])
        res = {"points": n}
        table = torch.from_numpy(default).to(dev)
        ro, rd = make_rays(p, table)

        def glue(total=None, near=None):
            """the torch part of the old route: the rays, the parity vote, the sign"""
            qo, qd = make_rays(p, table)
            if total is None:
                return qo, qd
            inside = ((total.view(n, 3) & 1).sum(dim=1) * 2) > 3
            return inside, torch.where(inside, -near.distance, near.distance)

        def old_route():
            qo, qd = glue()
            return glue(ds.count_intersections(qo, qd), ds.closest_points(p))

        total0, near0 = ds.count_intersections(ro, rd), ds.closest_points(p)
        new_c, old_count = timed(args.runs, lambda: ds.contains(p), lambda: ds.count_intersections(ro, rd))
        new_sd, old_near = timed(args.runs, lambda: ds.signed_distance(p), lambda: ds.closest_points(p))
        glue_only, whole = timed(max(3, args.runs // 3), lambda: (glue(), glue(total0, near0)), old_route)
        got = ds.contains(p)
        sd = ds.signed_distance(p)
        old_inside, old_sd = old_route()
        votes = got.votes.to(torch.int32)
        res.update(rays=n * 3, contains=new_c, signed_distance=new_sd, old_count_kernel_alone=old_count, old_closest_points_alone=old_near,
                   old_torch_glue_alone=glue_only, old_whole_route=whole,
                   contains_over_old_count_kernel=round(new_c["median_ms"] / old_count["median_ms"], 4),
                   signed_distance_over_old_whole_route=round(new_sd["median_ms"] / whole["median_ms"], 4),
                   inside_share=round(float(got.inside.float().mean()), 5),
                   non_unanimous_share=round(float(((votes != 0) & (votes != 3)).float().mean()), 5),
                   points_where_the_old_route_disagrees=int((old_inside != got.inside).sum()),
                   distance_bits_equal_closest_points=bool(torch.equal(sd.distance.abs().view(torch.int32), near0.distance.view(torch.int32))),
                   crossings_equal_old_totals=bool(torch.equal(got.crossings.reshape(-1), total0.reshape(-1))))
        del ro, rd, total0
        by_r = timed(args.runs, *[(lambda t=tables[r]: ds.contains(p, t)) for r in (1, 3, 8)])
        res["contains_by_R"] = {f"R{r}": s for r, s in zip((1, 3, 8), by_r)}
        out[batch] = res
    ds.close()
    print(json.dumps(dict(metric="containment and signed distance, ms per call (device-resident inputs; median, min, max of alternated runs)",
                          gpu=torch.cuda.get_device_name(dev), library=os.path.basename(_lib.LIB_PATH), scene=args.scene, n_triangles=flat.n_triangles,
                          n_spheres=flat.n_spheres, batches=out)))


if __name__ == "__main__":
    main()
