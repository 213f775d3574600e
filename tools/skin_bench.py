#!/usr/bin/env python3
"""What skinning on the device costs, and what a BENT mesh does to a refitted tree (semesterbild with the text_lowres and the
full text mesh, direct lighting, a 320 x 240 pinhole view of 4 samples: the workload of tools/rebuild_bench.py, so that the
tables of profiles/skin.md line up with those of profiles/rebuild.md).

The text mesh is an indexed mesh of two bones (tests/skin_cases.py: semesterbild_skin).  Bone 0 is the identity, bone 1 a turn
about the vertical axis through the mesh's centre; the weight of bone 1 ramps linearly from 0 to 1 along the mesh's long axis.

Per mesh, the wall time of one apply at a 15 degree bend by three routes:
  rt_skin_apply_device   bones in a torch tensor on the device (64 bytes never cross the bus), through ctypes,
  rt_skin_apply          bones on the host, through ctypes,
  numpy + update         the formulas in numpy float32 on the host, then DeviceScene.update with the arrays (48 bytes per
                         triangle cross the bus); the two parts are also given apart.
Per mesh and per angle: sah_now and the wall time of one render_view frame (enqueue to synchronised) of
  the refitted handle    created at rest, rt_skin_apply to the bend,
  the rebuilt handle     the same handle after rt_scene_rebuild,
  a fresh handle         rt_scene_create of the bent geometry (the binned-SAH builder on the host).
There is no acceptance threshold on any of these figures: profiles/skin.md is where a later rebuild trigger reads from.  Every
figure is the median of at least 5 repeats and at least --seconds; the whole measurement runs --runs times, and the spread is
max - min over the runs' medians.  Prints one JSON line and the markdown tables of profiles/skin.md."""
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
ANGLES = (0.0, 5.0, 15.0, 30.0, 60.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="text_lowres,text")
    ap.add_argument("--seconds", type=float, default=0.3, help="repeat every figure for at least this long")
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()

    import torch  # (before the library is loaded)

    import scene_update_cases as cases
    import skin_cases as S
    import view_cases as vc
    from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, _abi, _lib
    from hslu_i.ba_raytracing.f2501_raytracer_amd.obj import IndexedMesh
    from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceScene, DeviceSkin, DeviceView

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

    def timed(fn):
        def once():
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3
        return once

    def repeat(fn):
        out, t0 = [], time.perf_counter()
        while len(out) < 5 or time.perf_counter() - t0 < args.seconds:
            out.append(fn())
        return float(np.median(out))

    def over_runs(fn):
        m = [repeat(fn) for _ in range(args.runs)]
        return {"median": float(np.median(m)), "spread": float(max(m) - min(m))}

    result = {"view": [W, H, 4], "runs": args.runs, "seconds": args.seconds, "build_id": lib.rt_build_id().decode(), "models": {}}
    for model in args.models.split(","):
        flat0, mesh = S.semesterbild_skin(model)
        nt, nv = len(mesh["indices"]), len(mesh["position"])

        def new_skin(ds):
            return DeviceSkin(ds, IndexedMesh(mesh["position"], mesh["normal"], mesh["indices"]), mesh["bone"], mesh["weight"], tri_first=0, n_bones=2)

        # ---- the cost of one apply, by three routes ------------------------------------------------------------------------------
        ds = DeviceScene(flat0, 0)
        skin = new_skin(ds)
        two = [S.bend(mesh, 15.0), S.bend(mesh, 16.0)]  # (alternating: no apply restates what is there)
        on_dev = [torch.from_numpy(b).to(dev) for b in two]
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        k = [0]

        def apply_device():
            k[0] ^= 1
            _lib.check(lib.rt_skin_apply_device(ds.handle, skin.handle, C.c_void_p(on_dev[k[0]].data_ptr()), stream, None))

        def apply_host():
            k[0] ^= 1
            _lib.check(lib.rt_skin_apply(ds.handle, skin.handle, two[k[0]].ctypes.data, None))

        inf = _abi.rt_update_info()

        def device_ms():
            k[0] ^= 1
            _lib.check(lib.rt_skin_apply(ds.handle, skin.handle, two[k[0]].ctypes.data, C.byref(inf)))
            return inf.device_ms

        def numpy_skin():
            k[0] ^= 1
            S.expected(mesh, two[k[0]])

        def update_only():
            k[0] ^= 1
            ds.update(bent[k[0]])

        def numpy_and_update():
            k[0] ^= 1
            g = S.expected(mesh, two[k[0]])
            ds.update(cases.copy(flat0, **{name: np.concatenate([g[name], getattr(flat0, name)[nt:]]) for name in S.TRI_OUT}))

        apply_device(), apply_host()
        cost = {"apply_device_ms": over_runs(timed(apply_device)), "apply_host_ms": over_runs(timed(apply_host)), "apply_reported_device_ms": over_runs(device_ms)}
        skin.close()
        bent = [S.with_mesh(flat0, mesh, b) for b in two]
        update_only(), numpy_and_update()
        cost.update(numpy_ms=over_runs(timed(numpy_skin)), update_ms=over_runs(timed(update_only)), numpy_and_update_ms=over_runs(timed(numpy_and_update)))
        ds.close()

        # ---- per angle: SAH and frame time of refitted, rebuilt and fresh handles ------------------------------------------------
        rows = []
        for angle in ANGLES:
            bones = S.bend(mesh, angle)
            ds = DeviceScene(flat0, 0)
            skin = new_skin(ds)
            skin.apply(bones)
            refit_q = ds.bvh_quality()
            frame(ds)
            refit_ms = over_runs(lambda: frame(ds))
            info = ds.rebuild(info=True)
            rebuilt_q = ds.bvh_quality()
            frame(ds)
            rebuilt_ms = over_runs(lambda: frame(ds))
            skin.close(), ds.close()
            fresh = DeviceScene(S.with_mesh(flat0, mesh, bones), 0)
            fresh_q = fresh.bvh_quality()
            frame(fresh)
            fresh_ms = over_runs(lambda: frame(fresh))
            fresh.close()
            rows.append({"angle": angle, "sah_created": refit_q["sah_created"], "sah_refitted": refit_q["sah_now"], "sah_rebuilt": rebuilt_q["sah_now"],
                         "sah_fresh": fresh_q["sah_now"], "frame_refitted_ms": refit_ms, "frame_rebuilt_ms": rebuilt_ms, "frame_fresh_ms": fresh_ms,
                         "rebuild_ms": info["total_ms"], "n_nodes_rebuilt": info["n_nodes"]})
        result["models"][model] = {"triangles": int(flat0.n_triangles), "mesh_triangles": nt, "mesh_vertices": nv, "cost": cost, "rows": rows}
    print(json.dumps(result))
    print("\n| mesh | vertices | triangles | rt_skin_apply_device, wall ms | spread | rt_skin_apply, wall ms | spread | ... device ms it reports | "
          "numpy skinning, ms | DeviceScene.update, ms | numpy + update, ms | spread |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for model, r in result["models"].items():
        c = r["cost"]
        print(f"| {model} | {r['mesh_vertices']} | {r['mesh_triangles']} | {c['apply_device_ms']['median']:.3f} | {c['apply_device_ms']['spread']:.3f} | "
              f"{c['apply_host_ms']['median']:.3f} | {c['apply_host_ms']['spread']:.3f} | {c['apply_reported_device_ms']['median']:.3f} | "
              f"{c['numpy_ms']['median']:.3f} | {c['update_ms']['median']:.3f} | {c['numpy_and_update_ms']['median']:.3f} | {c['numpy_and_update_ms']['spread']:.3f} |")
    for model, r in result["models"].items():
        print(f"\n### {model} ({r['triangles']} triangles, {r['mesh_triangles']} of them the skinned mesh)\n")
        print("| bend, degrees | SAH refitted | SAH rebuilt | SAH fresh | frame refitted, ms | spread | frame rebuilt, ms | spread | frame fresh, ms | spread |")
        print("|---|---|---|---|---|---|---|---|---|---|")
        for x in r["rows"]:
            print(f"| {x['angle']:g} | {x['sah_refitted']:.2f} | {x['sah_rebuilt']:.2f} | {x['sah_fresh']:.2f} | {x['frame_refitted_ms']['median']:.3f} | "
                  f"{x['frame_refitted_ms']['spread']:.3f} | {x['frame_rebuilt_ms']['median']:.3f} | {x['frame_rebuilt_ms']['spread']:.3f} | "
                  f"{x['frame_fresh_ms']['median']:.3f} | {x['frame_fresh_ms']['spread']:.3f} |")
    view.close()


if __name__ == "__main__":
    main()
