"""What a device-side camera view (rt_view*, rt_render_view_device) costs, on the config-3 scene (semesterbild with
text.obj) and config 3's frame shape, 1620 x 1350, one GPU, every figure from the same process:

  per shading (direct light; soft shadows = config 3) and camera (the reference's; a pinhole elsewhere in the scene):
      view_1 / view_16      rt_render_view_device end to end, 1 sample and the configuration's 16 (9 distinct), for the order
                            modes none / once (the order is reused: a steady frame) / always (rebuilt every frame)
      stages                device time of generator, order build, trace and resolve of one frame (the view's own events,
                            host form, median of 5 frames), mode always
      frame_aa / frame_1    rt_render_device of the same configuration's frame with and without anti-aliasing, beside them
                            (the reference's camera; merged levels, one set of light clouds per pixel)
      host_rays_1           today's host path for one sample: numpy rays + upload + trace_rays, wall time to a synchronise

  with --adaptive, beside view_16 (order mode once, the steady frame, against once_ms of the same build):
      adaptive_ms           rt_render_view_adaptive_device end to end with Refine's default rule (DEPTH | COLOUR, 0.05 / 0.05)
      refined               the fraction of pixels that rule refines
      adaptive_stages_ms    device time of pass 1, classify, partition (with the sparse generator), pass 2 and the adaptive
                            resolve (the view's own events, host form, median of 5 frames)
      sweep / break_even    adaptive_ms over the refined fraction -- criteria 0, colour_tol from loose to tight, EVERY -- and the
                            fraction at which the adaptive frame costs what the full frame costs (linear between sweep points;
                            null: adaptive wins, or loses, at every fraction)

  with --lens, for the pinhole camera (a reference camera has no lens), the configuration's 16 pixel offsets and
  `camera.lens_samples(16)` -- 16 planes where view_16 has 9 --, order mode once:
      plain_config16        view_16 again (the configuration's table on a plain view: 9 planes), timed beside the others
      plain_16_planes       a plain view of 16 distinct pixel offsets: frame and generator time -- the parent's pinhole path at
                            the lens view's ray count
      lens_off / lens_on    the lens view with A == 0 (the pinhole generator on its planes) and with the lens open: frame time,
                            generator time (the view's own events, host form, median of 5 frames)
      adaptive              per aperture (0.5 % and 2 % of the focus distance, focused on the camera's target): the adaptive
                            lens frame with coc_tol 1 pixel and spread 8 against the full lens frame, its refined share, the
                            share the refine rule alone gives (coc_tol = inf), and the classify stage with and without the coc
                            and spread kernels (their cost is the difference), and that stage at spread 0, 4, 8 and 16
  --lens-only skips every column but these (a short run for the lens figures alone).

Every shape is warmed up, then timed with device events over repeated calls until at least --seconds of work.  The three
order modes are compared (equal bits) before anything is timed.  Prints one JSON line; two runs give the spread.

    python tools/view_bench.py [--device 0] [--seconds 1.0] [--only direct,soft] [--size 1620x1350] [--adaptive] [--lens [--lens-only]]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import torch  # (before the library: one HIP runtime in the process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, _abi, _lib, camera, scenes  # noqa: E402
from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceScene, DeviceView, Refine  # noqa: E402


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


SWEEP = (("none", Refine(criteria=0)), ("0.5", Refine(colour_tol=0.5)), ("0.2", Refine(colour_tol=0.2)), ("0.1", Refine(colour_tol=0.1)),
         ("0.05", Refine()), ("0.02", Refine(colour_tol=0.02)), ("0.005", Refine(colour_tol=0.005, depth_tol=0.005)), ("every", Refine(criteria="every")))


def adaptive_columns(ds, cfg, view, full_ms, full_frame, seconds):
    """the three columns of --adaptive for one (shading, camera): `view` is the order-once view that has been timed"""
    view.enable_adaptive()
    n = view.width * view.height
    e = {}
    every = ds.render_view(view, cfg, torch_out=True, refine=Refine(criteria="every"))
    e["every_equals_full"] = bool(same(every[:4], full_frame))
    e["adaptive_ms"] = time_it(lambda: ds.render_view(view, cfg, torch_out=True, refine=Refine()), seconds)
    info = view.adaptive_info
    e["refined"] = round(info["n_refined"] / n, 4)
    e["adaptive_bytes"] = info["bytes"]
    stages = []
    for _ in range(6):  # (host form: the view records its stage events; the first frame warms the staging up)
        ds.render_view(view, cfg, refine=Refine())
        i = view.adaptive_info
        stages.append([i[k] for k in ("pass1_ms", "classify_ms", "partition_ms", "pass2_ms", "resolve_ms")])
    med = np.median(np.array(stages[1:]), axis=0)
    e["adaptive_stages_ms"] = dict(zip(("pass1", "classify", "partition", "pass2", "resolve"), (round(float(x), 4) for x in med)))
    sweep = []
    for label, rf in SWEEP:
        ms = time_it(lambda: ds.render_view(view, cfg, torch_out=True, refine=rf), seconds / 2)
        sweep.append((label, round(view.adaptive_info["n_refined"] / n, 4), ms))
    e["sweep"] = sweep
    pts = sorted((f, ms) for _, f, ms in sweep)
    e["break_even"] = None
    for (f0, m0), (f1, m1) in zip(pts, pts[1:]):
        if m0 <= full_ms < m1 and f1 > f0:
            e["break_even"] = round(f0 + (f1 - f0) * (full_ms - m0) / (m1 - m0), 4)
    return e


def stage_medians(ds, cfg, view, keys, adaptive=False, refine=None):
    """median over 5 host-form frames (after one that warms the staging up) of the view's own stage times"""
    rows = []
    for _ in range(6):
        ds.render_view(view, cfg, refine=refine)
        i = view.adaptive_info if adaptive else view.info
        rows.append([i[k] for k in keys])
    return [round(float(x), 4) for x in np.median(np.array(rows[1:]), axis=0)]


def lens_columns(ds, cfg, device, w, h, pin, base, seconds):
    """the columns of --lens for one shading: plain and lens views of 16 planes on the pinhole camera"""
    cam = pin.view_camera()
    smp = camera.view_samples(base, _abi.RT_VIEW_PINHOLE)
    ls = camera.lens_samples(smp.shape[0])
    focus = float(np.linalg.norm(np.asarray(pin.target, np.float64) - np.asarray(pin.eye, np.float64)))
    rng = np.random.default_rng(1)
    distinct16 = (smp + rng.uniform(-1e-3, 1e-3, smp.shape)).astype(np.float32)  # (no repeated pixel offset: 16 planes)
    out = dict(focus_distance=round(focus, 4))
    nine = DeviceView(device, w, h, smp, order="once", camera=cam)  # (view_16 of the other columns: 9 distinct pixel offsets)
    out["plain_config16"] = dict(rays=nine.info["n_rays"], frame_ms=time_it(lambda: ds.render_view(nine, cfg, torch_out=True), seconds),
                                 generator_ms=stage_medians(ds, cfg, nine, ("rays_ms",))[0])
    nine.close()
    plain = DeviceView(device, w, h, distinct16, order="once", camera=cam)
    out["plain_16_planes"] = dict(rays=plain.info["n_rays"], frame_ms=time_it(lambda: ds.render_view(plain, cfg, torch_out=True), seconds),
                                  generator_ms=stage_medians(ds, cfg, plain, ("rays_ms",))[0])
    plain.close()
    view = DeviceView(device, w, h, smp, order="once", camera=cam, lens_samples=ls)
    out["rays"], out["view_bytes"] = view.info["n_rays"], view.info["bytes"]
    out["lens_off"] = dict(frame_ms=time_it(lambda: ds.render_view(view, cfg, torch_out=True), seconds),
                           generator_ms=stage_medians(ds, cfg, view, ("rays_ms",))[0])
    view.enable_adaptive()
    n = w * h
    adaptive = {}
    for share in (0.005, 0.02):
        A = share * focus
        view.set_lens(camera.ThinLens(A, focus, coc_tol=1.0, spread=8))
        e = dict(aperture=round(A, 5), full_ms=time_it(lambda: ds.render_view(view, cfg, torch_out=True), seconds),
                 generator_ms=stage_medians(ds, cfg, view, ("rays_ms",))[0])
        full = ds.render_view(view, cfg, torch_out=True)
        every = ds.render_view(view, cfg, torch_out=True, refine=Refine(criteria="every"))
        e["every_equals_full"] = bool(same(every[:4], full))
        del full, every
        e["adaptive_ms"] = time_it(lambda: ds.render_view(view, cfg, torch_out=True, refine=Refine()), seconds)
        e["refined"] = round(view.adaptive_info["n_refined"] / n, 4)
        keys = ("pass1_ms", "classify_ms", "partition_ms", "pass2_ms", "resolve_ms")
        e["stages_ms"] = dict(zip(keys, stage_medians(ds, cfg, view, keys, adaptive=True, refine=Refine())))
        view.set_lens(camera.ThinLens(A, focus, coc_tol=float("inf"), spread=8))
        e["adaptive_rule_only_ms"] = time_it(lambda: ds.render_view(view, cfg, torch_out=True, refine=Refine()), seconds)
        e["refined_rule_only"] = round(view.adaptive_info["n_refined"] / n, 4)
        e["classify_rule_only_ms"] = stage_medians(ds, cfg, view, ("classify_ms",), adaptive=True, refine=Refine())[0]
        e["coc_and_spread_ms"] = round(e["stages_ms"]["classify_ms"] - e["classify_rule_only_ms"], 4)
        sweep = {}
        for spread in (0, 4, 8, 16):  # (the classify stage with the coc kernel and a spread kernel of that halo)
            view.set_lens(camera.ThinLens(A, focus, coc_tol=1.0, spread=spread))
            sweep[str(spread)] = [stage_medians(ds, cfg, view, ("classify_ms",), adaptive=True, refine=Refine())[0], round(view.adaptive_info["n_refined"] / n, 4)]
        e["classify_ms_and_refined_by_spread"] = sweep
        adaptive[f"{share:g}"] = e
        if "lens_on" not in out:
            out["lens_on"] = dict(frame_ms=e["full_ms"], generator_ms=e["generator_ms"])
    out["adaptive"] = adaptive
    view.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--only", default="direct,soft")
    ap.add_argument("--size", default="1620x1350")
    ap.add_argument("--adaptive", action="store_true", help="add the adaptive frame, the refined fraction and the stage times beside view_16")
    ap.add_argument("--lens", action="store_true", help="add the thin-lens columns (pinhole camera, 16 planes) per shading")
    ap.add_argument("--lens-only", action="store_true", help="with --lens: skip every other column")
    args = ap.parse_args()
    only = set(args.only.split(","))
    w, h = (int(v) for v in args.size.split("x"))
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    size = dict(width_override=w, height_override=h)
    base = RenderConfig.from_features(["anti_aliasing"], **size)
    flat = scenes.semesterbild(base, "text").flatten()
    ds = DeviceScene(flat, args.device)
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    scale = (float(base.scene_width), float(base.scene_height), float(base.scene_depth))
    pin = camera.PinholeCamera([v * s for v, s in zip((-0.45, 0.25, -1.1), scale)], [v * s for v, s in zip((0.5, 0.5, 0.6), scale)],
                               (0.0, -1.0, 0.0), 38.0, w, h)
    cams = {"reference": (_abi.RT_VIEW_REFERENCE, camera.reference_view_camera(base)), "pinhole": (_abi.RT_VIEW_PINHOLE, pin.view_camera())}

    res = {}
    for name, features in (("direct", []), ("soft", ["soft_shadows"])):
        if name not in only:
            continue
        cfg = RenderConfig.from_features(features, **size)
        r = {}
        if args.lens:
            r["lens"] = lens_columns(ds, cfg, args.device, w, h, pin, base, args.seconds)
        if args.lens and args.lens_only:
            res[name] = r
            continue
        for cam_name, (kind, cam) in cams.items():
            c = {}
            for label, smp in (("view_1", None), ("view_16", camera.view_samples(base, kind))):
                views = {mode: DeviceView(args.device, w, h, smp, order=mode, camera=cam) for mode in ("none", "once", "always")}
                frames = {mode: ds.render_view(v, cfg, torch_out=True) for mode, v in views.items()}
                info = views["always"].info
                e = dict(rays=info["n_rays"], distinct=info["n_distinct"], view_bytes=info["bytes"],
                         modes_equal=bool(same(frames["none"], frames["once"]) and same(frames["none"], frames["always"])))
                full_frame = frames["once"]
                del frames
                for mode, v in views.items():
                    e[f"{mode}_ms"] = time_it(lambda: ds.render_view(v, cfg, torch_out=True), args.seconds)
                stages = []
                for _ in range(6):  # (host form: the view records its stage events; the first frame warms the staging up)
                    ds.render_view(views["always"], cfg)
                    i, st = views["always"].info, ds.last_trace_stats
                    stages.append((i["rays_ms"], i["order_ms"], st["kernel_ms"] - i["rays_ms"] - i["order_ms"] - i["resolve_ms"], i["resolve_ms"]))
                med = np.median(np.array(stages[1:]), axis=0)
                e["stages_ms"] = dict(zip(("generator", "order", "trace", "resolve"), (round(float(x), 4) for x in med)))
                if args.adaptive and smp is not None:
                    e.update(adaptive_columns(ds, cfg, views["once"], e["once_ms"], full_frame, args.seconds))
                del full_frame
                for v in views.values():
                    v.close()
                c[label] = e
            r[cam_name] = c
        frame = torch.zeros(w * h, dtype=torch.int32, device=dev)
        for label, feats in (("frame_aa_ms", features + ["anti_aliasing"]), ("frame_1_ms", features)):
            p, keep = _abi.make_params(RenderConfig.from_features(feats, **size))
            r[label] = time_it(lambda: _lib.check(lib.rt_render_device(ds.handle, C.byref(p), frame.data_ptr(), None, stream)), args.seconds)

        def host_path():
            o, d = pin.rays()
            ds.trace_rays(torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev), cfg)
            torch.cuda.synchronize()

        host_path()
        t = time.perf_counter()
        for _ in range(3):
            host_path()
        r["host_rays_1_wall_ms"] = round((time.perf_counter() - t) / 3 * 1e3, 3)
        res[name] = r
    torch.cuda.synchronize()
    print(json.dumps(dict(metric=f"camera views: ms per {w}x{h} frame (config-3 scene, text.obj)", gpu=torch.cuda.get_device_name(dev),
                          build_id=lib.rt_build_id().decode(), workloads=res)))
    ds.close()


if __name__ == "__main__":
    main()
