#!/usr/bin/env python3
"""Renders semesterbild on GPU 0 from a viewpoint of the caller's choosing (the reference has one, fixed at compile
time) and writes a PNG: camera.PinholeCamera -> RaytracerRenderer.render_camera -> rt_trace_rays, or with --aa through a
device-side view (rt_render_view: rays made, traced and resolved on the device, the configuration's anti-aliasing table);
--aa --adaptive takes all samples only where the first sample of neighbouring pixels differs (rt_render_view_adaptive);
--aa --aperture A --focus-distance F renders through a thin lens (depth of field: rt_view_create_lens), and with --adaptive
--coc-tol T also refines what is blurred by more than T pixels, and what that blur reaches.

    render_view.py OUT.png [--eye X,Y,Z] [--target X,Y,Z] [--fov DEG] [--size WxH] [--features f,g] [--model text|text_lowres] [--order] [--aa [--aperture A --focus-distance F] [--adaptive [--colour-tol X] [--depth-tol X] [--coc-tol T] [--spread N]]]

eye / target are in units of the scene's width, height and depth (the reference's own focus is 0.5,0.5,-1.9; image y points
down, so the camera's up vector is (0, -1, 0)); aperture (the lens radius) and focus distance are in units of the scene's width
(default focus: the target)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from PIL import Image  # noqa: E402

from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, camera, scenes  # noqa: E402
from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import ImageBuffer, RaytracerRenderer, Refine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--eye", default="-0.45,0.25,-1.1")
    ap.add_argument("--target", default="0.5,0.5,0.6")
    ap.add_argument("--fov", type=float, default=38.0)
    ap.add_argument("--size", default="1280x960")
    ap.add_argument("--features", default="soft_shadows,realistic")
    ap.add_argument("--model", default="text")
    ap.add_argument("--fill", default="0xFF101010")
    ap.add_argument("--order", action="store_true", help="pack the camera's rays into coherent wavefronts (a ray order built on the device)")
    ap.add_argument("--aa", action="store_true", help="anti-aliased: the configuration's sample table through a device-side view")
    ap.add_argument("--adaptive", action="store_true", help="with --aa: refine only edge pixels (depth and colour criteria)")
    ap.add_argument("--colour-tol", type=float, default=Refine().colour_tol, help="largest step of a linear RGB channel between neighbours that is not an edge")
    ap.add_argument("--depth-tol", type=float, default=Refine().depth_tol, help="largest step of the hit distance, relative to the nearer hit, that is not an edge")
    ap.add_argument("--aperture", type=float, default=0.0, help="with --aa: lens radius in scene widths (0: a pinhole)")
    ap.add_argument("--focus-distance", type=float, default=None, help="distance of the plane in focus along the viewing direction, in scene widths")
    ap.add_argument("--coc-tol", type=float, default=float("inf"), help="with --adaptive and a lens: refine pixels blurred by more than this many pixels")
    ap.add_argument("--spread", type=int, default=8, help="how many pixels (0..16) a blur may reach in the defocus criterion")
    args = ap.parse_args()
    if args.adaptive and not args.aa:
        ap.error("--adaptive needs --aa")
    if args.aperture < 0.0:
        ap.error("--aperture must not be negative")
    if args.aperture and not args.aa:
        ap.error("--aperture needs --aa")
    if not args.aperture and (args.focus_distance is not None or args.coc_tol != ap.get_default("coc_tol") or args.spread != ap.get_default("spread")):
        ap.error("--focus-distance, --coc-tol and --spread need --aperture")
    if not args.adaptive and (args.coc_tol != ap.get_default("coc_tol") or args.spread != ap.get_default("spread")):
        ap.error("--coc-tol and --spread need --adaptive")
    refine = Refine(colour_tol=args.colour_tol, depth_tol=args.depth_tol) if args.adaptive else None
    cfg = RenderConfig.from_features([f for f in args.features.split(",") if f])
    scale = (float(cfg.scene_width), float(cfg.scene_height), float(cfg.scene_depth))
    eye = [float(v) * s for v, s in zip(args.eye.split(","), scale)]
    target = [float(v) * s for v, s in zip(args.target.split(","), scale)]
    w, h = (int(v) for v in args.size.split("x"))
    cam = camera.PinholeCamera(eye, target, (0.0, -1.0, 0.0), args.fov, w, h)
    lens = None
    if args.aperture:
        focus = args.focus_distance * scale[0] if args.focus_distance else sum((t - e) ** 2 for t, e in zip(target, eye)) ** 0.5
        lens = camera.ThinLens(args.aperture * scale[0], focus, coc_tol=args.coc_tol, spread=args.spread)
    scene = scenes.semesterbild(cfg, args.model)
    buf = ImageBuffer.new_with_color(w, h, int(args.fill, 0))
    r = RaytracerRenderer(cfg)
    t = time.time()
    out = r.render_camera(buf, scene, cam, order=args.order, samples="config" if args.aa else None, refine=refine, lens=lens)
    refined = f" refined={float(out.mask.mean()):.3f}" if args.adaptive else ""
    print(f"semesterbild {w}x{h} from eye={eye} features={sorted(cfg.features)} order={args.order} aa={args.aa} lens={lens}{refined} valid={float(out.valid.mean()):.3f} "
          f"wall={time.time() - t:.3f}s stats={r.last_stats}")
    Image.fromarray(buf.as_rgb8()).save(args.out)


if __name__ == "__main__":
    main()
