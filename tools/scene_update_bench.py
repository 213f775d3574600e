#!/usr/bin/env python3
"""What an in-place scene update costs next to the only other route, destroy + create (semesterbild / text.obj, config 3).

For a light-only, a sphere-only and a full-mesh update (every mesh triangle turned): the update itself (wall time of the
blocking call, and the device time of its kernels and copies from rt_update_info), the next soft-shadow frame (device
events around rt_render_device; it rebuilds the receiver flags), and the pair's wall time.  The baseline, in the same
process and run: rt_scene_destroy + rt_scene_create + the first frame.  Every figure is repeated for at least
--seconds, the scene alternating between two states so that every update changes something; the whole measurement runs
--runs times and the spread is max - min over the runs' medians.  Prints one JSON line and a markdown table."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="repeat every figure for at least this long")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--budget", type=int, default=None, help="rt_scene_desc.device_budget_bytes (default: bench.py's)")
    args = ap.parse_args()

    import torch

    import bench
    import scene_update_cases as cases
    from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, _lib
    from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceScene

    cfg, flat, name = bench.build_workload("c3")
    flat = flat.contiguous()
    budget = bench.SCENE_BUDGET if args.budget is None else args.budget
    n_mesh = flat.n_triangles - 4 * cases.plane_triangles()
    states = {"light": cases.orbit_lights(flat, 10.0), "sphere": cases.move_spheres(flat), "mesh": cases.turn_mesh(flat, (0, n_mesh), 20.0)}
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    fb = torch.zeros(cfg.width * cfg.height, dtype=torch.int32, device=dev)
    p, keep = _abi.make_params(cfg)

    def frame(ds):
        """one frame alone on the stream -> (device ms, wall ms until it is done)"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        _lib.check(lib.rt_render_device(ds.handle, C.byref(p), C.c_void_p(fb.data_ptr()), None, C.c_void_p(stream.cuda_stream)))
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    def repeat(fn):
        rows, t0 = [], time.perf_counter()
        while len(rows) < 5 or time.perf_counter() - t0 < args.seconds:
            rows.append(fn())
        return {k: float(np.median([r[k] for r in rows])) for k in rows[0]}, len(rows)

    ds = DeviceScene(flat, 0, budget=budget)
    for _ in range(5):
        frame(ds)
    steady = repeat(lambda: dict(zip(("frame_device_ms", "frame_wall_ms"), frame(ds))))[0]
    runs = []
    for run in range(args.runs):
        out = {}
        for kind, other in states.items():
            flip = [other, flat]
            k = [0]

            def once():
                t0 = time.perf_counter()
                info = ds.update(flip[k[0] % 2], info=True)
                t1 = time.perf_counter()
                fd, fw = frame(ds)
                k[0] += 1
                return {"update_wall_ms": (t1 - t0) * 1e3, "update_call_ms": info["total_ms"], "update_device_ms": info["device_ms"],
                        "frame_device_ms": fd, "pair_wall_ms": (t1 - t0) * 1e3 + fw}

            once(), once()  # warm-up: staging buffers
            out[kind], n = repeat(once)
            out[kind]["reps"] = n
            if k[0] % 2:
                ds.update(flat)

        def recreate():
            nonlocal ds
            t0 = time.perf_counter()
            ds.close()
            ds = DeviceScene(flat, 0, budget=budget)
            t1 = time.perf_counter()
            fd, fw = frame(ds)
            return {"recreate_wall_ms": (t1 - t0) * 1e3, "frame_device_ms": fd, "pair_wall_ms": (t1 - t0) * 1e3 + fw}

        recreate()
        out["recreate"], n = repeat(recreate)
        out["recreate"]["reps"] = n
        runs.append(out)

    kinds = list(states) + ["recreate"]
    summary = {}
    for kind in kinds:
        summary[kind] = {}
        for key in runs[0][kind]:
            v = [r[kind][key] for r in runs]
            summary[kind][key] = {"median": float(np.median(v)), "spread": float(max(v) - min(v))}
    base = summary["recreate"]["pair_wall_ms"]
    verdict = {}
    for kind in states:
        u = summary[kind]["pair_wall_ms"]
        verdict[kind] = {"margin_ms": base["median"] - u["median"], "spreads_ms": base["spread"] + u["spread"],
                         "ok": bool(base["median"] - u["median"] > base["spread"] + u["spread"])}
    print(json.dumps({"workload": name, "triangles": flat.n_triangles, "mesh_triangles": n_mesh, "budget": budget, "steady_frame": steady,
                      "build_id": lib.rt_build_id().decode(), "summary": summary, "verdict": verdict, "bvh": ds.bvh_info()}))
    print(f"\n| what ({args.runs} runs, >= {args.seconds:g} s each) | call, wall ms | call, device ms | next frame, device ms | call + frame, wall ms | spread |")
    print("|---|---|---|---|---|---|")
    for kind in kinds:
        s = summary[kind]
        call = s.get("update_wall_ms", s.get("recreate_wall_ms"))
        devms = f"{s['update_device_ms']['median']:.3f}" if "update_device_ms" in s else "-"
        label = {"light": "light-only update", "sphere": "sphere-only update", "mesh": f"full-mesh update ({n_mesh} triangles)",
                 "recreate": "destroy + create"}[kind]
        print(f"| {label} | {call['median']:.3f} | {devms} | {s['frame_device_ms']['median']:.3f} | {s['pair_wall_ms']['median']:.3f} | "
              f"{s['pair_wall_ms']['spread']:.3f} |")
    print(f"\nsteady frame: {steady['frame_device_ms']:.3f} ms device")
    for kind, v in verdict.items():
        print(f"{kind}: margin {v['margin_ms']:.3f} ms vs sum of spreads {v['spreads_ms']:.3f} ms -> {'ok' if v['ok'] else 'NOT shorter'}")
    ds.close()


if __name__ == "__main__":
    main()
