#!/usr/bin/env python3
"""What a device-side BVH rebuild buys and what it costs (semesterbild with the text_lowres and the full text mesh, direct
lighting, a 320 x 240 pinhole view of 4 samples).

Per mesh and per jitter amplitude of scene_update_cases.jitter: sah_now and the wall time of one render_view frame (enqueue to
synchronised) of
  the refitted handle   created from the rest geometry, rt_scene_update to the jittered one,
  the rebuilt handle    the same handle after rt_scene_rebuild,
  a fresh handle        rt_scene_create of the jittered geometry (the binned-SAH builder on the host).
Then the cost of the repair by either route, on the deformed handle: rt_scene_rebuild (wall, and the device time it reports)
next to rt_scene_destroy + rt_scene_create + the first frame, which pays for the workspaces the new handle lacks.
There is no acceptance threshold on any of these figures: profiles/rebuild.md is where a later heuristic reads its threshold
from.  Every figure is the median of at least 5 repeats and at least --seconds; the whole measurement runs --runs times, and
the spread is max - min over the runs' medians.  Prints one JSON line and the markdown tables of profiles/rebuild.md.

--method ploc adds, in the same run, a second handle per row that is repaired with rt_scene_rebuild_with(RT_REBUILD_PLOC)
(--radius R, --keep-better): its SAH, its frame, the cost of the call and its iteration count, next to the LBVH columns."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
AMPLITUDES = (0.0, 0.01, 0.02, 0.05, 0.1, 0.2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="text_lowres,text")
    ap.add_argument("--seconds", type=float, default=0.3, help="repeat every figure for at least this long")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--method", choices=("lbvh", "ploc"), default="lbvh", help="ploc: a PLOC column next to the LBVH's")
    ap.add_argument("--radius", type=int, default=None, help="PLOC: positions of the Morton order searched on either side (default 8)")
    ap.add_argument("--keep-better", action="store_true", help="PLOC: swap only if the candidate's SAH is lower (RT_REBUILD_KEEP_BETTER)")
    args = ap.parse_args()

    import torch  # (before the library is loaded)

    import scene_update_cases as cases
    import view_cases as vc
    from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, _lib, scenes
    from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceScene, DeviceView

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    cfg = RenderConfig.from_features([])
    W, H = 320, 240
    view = DeviceView(0, W, H, np.array([[-.25, -.25], [.25, -.25], [-.25, .25], [.25, .25]], np.float32), camera=vc.pinhole(W, H).view_camera())

    def frame(ds):
        t0 = time.perf_counter()
        ds.render_view(view, cfg, torch_out=True)
        torch.cuda.current_stream(dev).synchronize()
        return (time.perf_counter() - t0) * 1e3

    def repeat(fn):
        out, t0 = [], time.perf_counter()
        while len(out) < 5 or time.perf_counter() - t0 < args.seconds:
            out.append(fn())
        return float(np.median(out))

    def over_runs(fn):
        m = [repeat(fn) for _ in range(args.runs)]
        return {"median": float(np.median(m)), "spread": float(max(m) - min(m))}

    ploc = dict(method="ploc", radius=args.radius, keep_better=args.keep_better)
    result = {"view": [W, H, 4], "runs": args.runs, "method": args.method, "radius": args.radius, "keep_better": args.keep_better, "seconds": args.seconds, "build_id": lib.rt_build_id().decode(), "models": {}}
    for model in args.models.split(","):
        flat = scenes.semesterbild(cfg, model=model).flatten().contiguous()
        rows = []
        for amp in AMPLITUDES:
            moved = cases.jitter(flat, amp) if amp else flat
            ds = DeviceScene(flat, 0)
            if amp:
                ds.update(moved)
            refit_q = ds.bvh_quality()
            frame(ds)
            refit_ms = over_runs(lambda: frame(ds))
            info = ds.rebuild(info=True)
            rebuilt_q = ds.bvh_quality()
            frame(ds)
            rebuilt_ms = over_runs(lambda: frame(ds))

            def rebuild_once():  # (a rebuild of a rebuilt tree does the same work)
                t0 = time.perf_counter()
                ds.rebuild()
                return (time.perf_counter() - t0) * 1e3

            rebuild_wall = over_runs(rebuild_once)
            rebuild_device = over_runs(lambda: ds.rebuild(info=True)["device_ms"])
            ds.close()
            extra = {}
            if args.method == "ploc":  # (a second handle with the same history, repaired the other way)
                ds = DeviceScene(flat, 0)
                if amp:
                    ds.update(moved)
                rep = ds.rebuild(info=True, **ploc)
                ploc_q = ds.bvh_quality()
                frame(ds)
                ploc_ms = over_runs(lambda: frame(ds))

                def ploc_once():
                    t0 = time.perf_counter()
                    ds.rebuild(**ploc)
                    return (time.perf_counter() - t0) * 1e3

                extra = {"sah_ploc": ploc_q["sah_now"], "sah_ploc_candidate": rep["sah_after"], "ploc_swapped": rep["swapped"], "frame_ploc_ms": ploc_ms,
                         "ploc_wall_ms": over_runs(ploc_once), "ploc_device_ms": over_runs(lambda: ds.rebuild(info=True, **ploc)["device_ms"]),
                         "first_ploc_ms": rep["total_ms"], "ploc_iterations": rep["iterations"], "n_nodes_ploc": rep["n_nodes"], "max_depth_ploc": rep["max_depth"]}
                ds.close()
            fresh = DeviceScene(moved, 0)
            fresh_q = fresh.bvh_quality()
            frame(fresh)
            fresh_ms = over_runs(lambda: frame(fresh))
            fresh.close()

            def recreate_once():
                t0 = time.perf_counter()
                s = DeviceScene(moved, 0)
                t1 = time.perf_counter()
                frame(s)
                t2 = time.perf_counter()
                s.close()
                return (t1 - t0) * 1e3, (t2 - t0) * 1e3

            pairs = [recreate_once() for _ in range(max(5, args.runs))]
            rows.append({"amplitude": amp, "sah_created": refit_q["sah_created"], "sah_refitted": refit_q["sah_now"], "sah_rebuilt": rebuilt_q["sah_now"],
                         "sah_fresh": fresh_q["sah_now"], "frame_refitted_ms": refit_ms, "frame_rebuilt_ms": rebuilt_ms, "frame_fresh_ms": fresh_ms,
                         "rebuild_wall_ms": rebuild_wall, "rebuild_device_ms": rebuild_device, "first_rebuild_ms": info["total_ms"],
                         "create_ms": float(np.median([p[0] for p in pairs])), "create_and_first_frame_ms": float(np.median([p[1] for p in pairs])),
                         "n_nodes_rebuilt": info["n_nodes"], "max_depth_rebuilt": info["max_depth"], **extra})
        result["models"][model] = {"triangles": flat.n_triangles, "rows": rows}
    print(json.dumps(result))
    for model, r in result["models"].items():
        print(f"\n### {model} ({r['triangles']} triangles)\n")
        print("| jitter amplitude | SAH refitted | SAH rebuilt | SAH fresh | frame refitted, ms | spread | frame rebuilt, ms | spread | frame fresh, ms | spread |")
        print("|---|---|---|---|---|---|---|---|---|---|")
        for x in r["rows"]:
            print(f"| {x['amplitude']:g} | {x['sah_refitted']:.2f} | {x['sah_rebuilt']:.2f} | {x['sah_fresh']:.2f} | {x['frame_refitted_ms']['median']:.3f} | "
                  f"{x['frame_refitted_ms']['spread']:.3f} | {x['frame_rebuilt_ms']['median']:.3f} | {x['frame_rebuilt_ms']['spread']:.3f} | "
                  f"{x['frame_fresh_ms']['median']:.3f} | {x['frame_fresh_ms']['spread']:.3f} |")
        print("\n| jitter amplitude | rt_scene_rebuild, wall ms | spread | ... device ms | first rebuild of the handle, wall ms | rt_scene_create, wall ms | destroy + create + first frame, wall ms |")
        print("|---|---|---|---|---|---|---|")
        for x in r["rows"]:
            print(f"| {x['amplitude']:g} | {x['rebuild_wall_ms']['median']:.3f} | {x['rebuild_wall_ms']['spread']:.3f} | {x['rebuild_device_ms']['median']:.3f} | "
                  f"{x['first_rebuild_ms']:.3f} | {x['create_ms']:.3f} | {x['create_and_first_frame_ms']:.3f} |")
        if args.method == "ploc":
            print(f"\nPLOC, radius {args.radius or 8}{', keep-better' if args.keep_better else ''}:\n")
            print("| jitter amplitude | SAH LBVH | SAH PLOC (candidate) | swapped | frame LBVH, ms | frame PLOC, ms | spread | PLOC rebuild, wall ms | spread | ... device ms | iterations | "
                  "extra cost over the LBVH, ms | frames to repay it |")
            print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
            for x in r["rows"]:
                cost = x["ploc_wall_ms"]["median"] - x["rebuild_wall_ms"]["median"]
                gain = x["frame_rebuilt_ms"]["median"] - x["frame_ploc_ms"]["median"]
                print(f"| {x['amplitude']:g} | {x['sah_rebuilt']:.2f} | {x['sah_ploc_candidate']:.2f} | {x['ploc_swapped']} | {x['frame_rebuilt_ms']['median']:.3f} | "
                      f"{x['frame_ploc_ms']['median']:.3f} | {x['frame_ploc_ms']['spread']:.3f} | {x['ploc_wall_ms']['median']:.3f} | {x['ploc_wall_ms']['spread']:.3f} | "
                      f"{x['ploc_device_ms']['median']:.3f} | {x['ploc_iterations']} | {cost:.3f} | {f'{cost / gain:.0f}' if gain > 0 else 'never'} |")
    view.close()


if __name__ == "__main__":
    main()
