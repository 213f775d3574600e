#!/usr/bin/env python3
"""What a posed frame costs by each route, and how a refitted tree's SAH report relates to its frame time
(semesterbild / text_lowres, direct lighting, a 320 x 240 pinhole view of 4 samples).

Section 1 turns the text mesh through --steps poses.  Per step, the wall time of the blocking call that moves the mesh:
  (a) the host route: the pose formulas in numpy float32 + rt_scene_update with the posed arrays,
  (b) rt_pose_apply with host transforms (32 bytes per part staged),
  (c) rt_pose_apply_device with the transforms already on the device,
and next to each the wall time of one render_view frame behind it (enqueue to synchronised).
Section 2 applies scene_update_cases.jitter at growing amplitudes and records sah_now / sah_created next to the frame time
of the refitted handle and of a handle freshly created from the same description.
There is no acceptance threshold on any of these figures.  Every figure is the median of at least 5 repeats and at least
--seconds; the whole measurement runs --runs times, and the spread is max - min over the runs' medians.
Prints one JSON line and the markdown tables of profiles/pose.md."""
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
    ap.add_argument("--steps", type=int, default=16, help="poses of one turn of the mesh")
    ap.add_argument("--seconds", type=float, default=0.3, help="repeat every figure for at least this long")
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()

    import torch  # (before the library is loaded)

    import pose_cases as P
    import scene_update_cases as cases
    import view_cases as vc
    from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, _abi, _lib
    from hslu_i.ba_raytracing.f2501_raytracer_amd.f32math import Rotor3, Similarity3, Vec3
    from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DevicePose, DeviceScene, DeviceView

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    cfg = RenderConfig.from_features([])
    flat = cases.flat_semesterbild(cfg)
    rest = P.rest_of(flat)
    first, count = cases.mesh_range("semesterbild", flat)
    parts = [(first, count, 0, 0)]
    W, H = 320, 240
    view = DeviceView(0, W, H, np.array([[-.25, -.25], [.25, -.25], [-.25, .25], [.25, .25]], np.float32),
                      camera=vc.pinhole(W, H).view_camera())
    s = slice(first, first + count)
    c = Vec3(*np.concatenate([rest["v1"][s], rest["v2"][s], rest["v3"][s]]).astype(np.float64).mean(0))

    def pose_of(k):
        rotor = Rotor3.from_euler_angles(0.0, 0.0, 6.2831853 * k / args.steps)
        return Similarity3(c - rotor.rotate_vec(c), rotor, 1.0)

    rows = [_abi.transform_rows([pose_of(k)]) for k in range(args.steps)]
    rows_dev = [torch.from_numpy(r).to(dev) for r in rows]
    torch.cuda.synchronize(dev)

    def frame(ds):
        t0 = time.perf_counter()
        ds.render_view(view, cfg, torch_out=True)
        torch.cuda.current_stream(dev).synchronize()
        return (time.perf_counter() - t0) * 1e3

    def repeat(fn):
        out, t0 = [], time.perf_counter()
        while len(out) < 5 or time.perf_counter() - t0 < args.seconds:
            out.append(fn())
        return {k: float(np.median([r[k] for r in out])) for k in out[0]}

    ds = DeviceScene(flat, 0)
    pose = DevicePose(ds, parts, rest_v2=rest["v2"], rest_v3=rest["v3"], rest_radius=rest["radius"])
    inf = _abi.rt_update_info()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    k = [0]

    def route_a():
        r = rows[k[0] % args.steps]
        t0 = time.perf_counter()
        g = P.expected(rest, parts, r)
        d = _abi.rt_scene_delta()
        d.abi_version, d.tri_first, d.tri_count = _abi.RT_ABI_VERSION, first, count
        d.tri_v1, d.tri_e1, d.tri_e2, d.tri_normal = (g[n].ctypes.data for n in P.TRI_OUT)
        t1 = time.perf_counter()
        _lib.check(lib.rt_scene_update(ds.handle, C.byref(d), C.byref(inf)))
        t2 = time.perf_counter()
        k[0] += 1
        return {"pose_ms": (t1 - t0) * 1e3, "call_ms": (t2 - t1) * 1e3, "step_ms": (t2 - t0) * 1e3, "device_ms": inf.device_ms, "frame_ms": frame(ds)}

    def route_b():
        r = rows[k[0] % args.steps]
        t0 = time.perf_counter()
        _lib.check(lib.rt_pose_apply(ds.handle, pose.handle, r.ctypes.data, C.byref(inf)))
        t1 = time.perf_counter()
        k[0] += 1
        return {"pose_ms": 0.0, "call_ms": (t1 - t0) * 1e3, "step_ms": (t1 - t0) * 1e3, "device_ms": inf.device_ms, "frame_ms": frame(ds)}

    def route_c():
        r = rows_dev[k[0] % args.steps]
        t0 = time.perf_counter()
        _lib.check(lib.rt_pose_apply_device(ds.handle, pose.handle, C.c_void_p(r.data_ptr()), stream, C.byref(inf)))
        t1 = time.perf_counter()
        k[0] += 1
        return {"pose_ms": 0.0, "call_ms": (t1 - t0) * 1e3, "step_ms": (t1 - t0) * 1e3, "device_ms": inf.device_ms, "frame_ms": frame(ds)}

    routes = {"a: numpy pose + rt_scene_update": route_a, "b: rt_pose_apply (host transforms)": route_b, "c: rt_pose_apply_device": route_c}
    for fn in routes.values():  # warm-up: staging buffers, the view's ray order
        fn(), fn()
    runs = [{name: repeat(fn) for name, fn in routes.items()} for _ in range(args.runs)]
    section1 = {name: {key: {"median": float(np.median([r[name][key] for r in runs])), "spread": float(max(r[name][key] for r in runs) - min(r[name][key] for r in runs))}
                       for key in runs[0][name]} for name in routes}
    pose.apply(_abi.transform_rows([Similarity3.identity()]))
    pose.close()

    # ---- section 2: SAH ratio against frame time ------------------------------------------------------------------------------------
    section2 = []
    ds.update(flat)
    base = repeat(lambda: {"frame_ms": frame(ds)})["frame_ms"]
    for amp in (0.005, 0.01, 0.02, 0.05, 0.1, 0.2):
        moved = cases.jitter(flat, amp)
        ds.update(moved)
        q = ds.bvh_quality()
        fresh = DeviceScene(moved, 0)
        qf = fresh.bvh_quality()
        frame(ds), frame(fresh)
        per_run = [(repeat(lambda: {"frame_ms": frame(ds)})["frame_ms"], repeat(lambda: {"frame_ms": frame(fresh)})["frame_ms"]) for _ in range(args.runs)]
        fresh.close()
        ds.update(flat)
        refit_ms, fresh_ms = [p[0] for p in per_run], [p[1] for p in per_run]
        section2.append({"amplitude": amp, "sah_created": q["sah_created"], "sah_now": q["sah_now"], "ratio": q["sah_now"] / q["sah_created"],
                         "sah_fresh": qf["sah_now"], "report_ms": q["device_ms"],
                         "frame_refit_ms": float(np.median(refit_ms)), "frame_refit_spread": float(max(refit_ms) - min(refit_ms)),
                         "frame_fresh_ms": float(np.median(fresh_ms)), "frame_fresh_spread": float(max(fresh_ms) - min(fresh_ms))})

    print(json.dumps({"workload": "semesterbild / text_lowres, direct lighting", "view": [W, H, 4], "mesh_triangles": count, "triangles": flat.n_triangles,
                      "steps": args.steps, "runs": args.runs, "seconds": args.seconds, "build_id": lib.rt_build_id().decode(), "bvh": ds.bvh_info(),
                      "routes": section1, "frame_rest_ms": base, "jitter": section2}))
    print(f"\n| route ({args.runs} runs, >= {args.seconds:g} s each) | pose on host, ms | blocking call, wall ms | call, device ms | step (pose + call), wall ms | spread | "
          "view frame behind it, wall ms |")
    print("|---|---|---|---|---|---|---|")
    for name, r in section1.items():
        print(f"| {name} | {r['pose_ms']['median']:.3f} | {r['call_ms']['median']:.3f} | {r['device_ms']['median']:.3f} | {r['step_ms']['median']:.3f} | "
              f"{r['step_ms']['spread']:.3f} | {r['frame_ms']['median']:.3f} |")
    print(f"\nview frame of the rest pose: {base:.3f} ms wall\n")
    print("| jitter amplitude (of the scene diagonal) | sah_now / sah_created | sah_now | sah of a fresh handle | frame, refitted handle, ms | spread | frame, fresh handle, ms | spread |")
    print("|---|---|---|---|---|---|---|---|")
    for r in section2:
        print(f"| {r['amplitude']:g} | {r['ratio']:.3f} | {r['sah_now']:.2f} | {r['sah_fresh']:.2f} | {r['frame_refit_ms']:.3f} | {r['frame_refit_spread']:.3f} | "
              f"{r['frame_fresh_ms']:.3f} | {r['frame_fresh_spread']:.3f} |")
    view.close(), ds.close()


if __name__ == "__main__":
    main()
