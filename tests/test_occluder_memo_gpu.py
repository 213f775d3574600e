"""The memo of the last transmissive shadow occluder (OccMemo in csrc/rt_kernels.hip, kept per (wavefront, light) by
rt_primary_soft*_kernel) changes no bit of a frame.

Hand-built scenes, 64x48, anti-aliasing, soft shadows with 10 samples per light: a sloped opaque floor, transmissive panes
above it and the light above the panes, so that the shadow rays of the floor cross the panes in an order that depends on
the wavefront.  Every scene is rendered

* as the library renders it under a 2 GiB scene budget: rt_primary_soft10_kernel, shared candidate lists (the memo),
* with shadow_candidate_cap = 1: the same kernel, but every set with more than one candidate walks the BVH per sample
  (the memo on the walk route),
* with shadow_candidate_cap = RT_CAND_CAP_NONE: a walk per sample in rt_primary_kernel, which keeps no memo and runs the
  unsplit shadow_accumulate,
* and all three once more in a process with RT_PRIMARY_GENERIC=1 (rt_primary_kernel, no memo).

(The streaming path with its pairs deferred to rt_hard_kernel is not among them: it needs secondary rays -- the library
refuses them with depth 0, and with depth 1 the panes refract -- and it sums the lights' shares in fixed point, so its frame
is another frame.  test_parity_gpu.py holds that path to the in-kernel one.)

All of them must be the same frame, bit for bit, in the packed pixels and in the float planes, every pixel included; and
the frame must be within 1e-4 of the oracle.  The switch and the launch trace are read once per process, so the renders run
in two child processes started before any GPU call; the parent compares what they wrote."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

W, H = 64, 48
FEATURES = ["anti_aliasing", "soft_shadows"]
BUDGET = 2 << 30
RGB_TOL = 1e-4  # the project's bar against the oracle (test_parity_gpu.py)
CHILD_TIMEOUT_S = 240
ROUTES = ("lists", "walk", "no_sharing")
SCENES = ("alternating", "one_material", "sphere_and_pane", "opaque_between", "second_light")


def config():
    from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig

    return RenderConfig.from_features(FEATURES, width_override=W, height_override=H, n_cloud_sets=64)


def build_scene(name, cfg, panes=True):
    """y points down.  The floor rises from the bottom edge of the image at z = 0 to 0.55 SH at the back, so the camera (rays
    nearly parallel to z) sees it in the lower half of the frame; the panes lie parallel to it, 0.25 SH (A) and 0.15 SH (B)
    above it, and are narrower than it."""
    from hslu_i.ba_raytracing.f2501_raytracer_amd.f32math import F, Vec3
    from hslu_i.ba_raytracing.f2501_raytracer_amd.scene import (ColorType, Material, PointLight, Scene, SphereData,
                                                                 TransmissionProperties as TP, TriangleData)

    SW, SH, SD = float(cfg.scene_width), float(cfg.scene_height), float(cfg.scene_depth)
    scene = Scene.new()

    def floor_y(z):
        return SH * (1.0 - 0.45 * z / SD)

    def quad(x0, x1, z0, z1, lift, material):
        p = [Vec3.new(F(x), F(floor_y(z) - lift), F(z)) for x, z in ((x0, z0), (x1, z0), (x0, z1), (x1, z1))]
        scene.add_triangle(TriangleData.with_material(p[0], p[1], p[2], material))
        scene.add_triangle(TriangleData.with_material(p[1], p[3], p[2], material))

    opaque = Material.new(ColorType.new(0.8, 0.8, 0.7), 0.0, 0.0, TP.none())
    quad(-0.5 * SW, 1.5 * SW, -0.1 * SD, 1.3 * SD, 0.0, opaque)
    # A: not reflective (metallic 0: the decrement depends on the lane); B: reflective (metallic > 0: a wave-uniform decrement)
    mat_a = Material.new(ColorType.new(0.9, 0.4, 0.3), 0.0, 0.3, TP.new(0.7, 1.5))
    mat_b = Material.new(ColorType.new(0.3, 0.5, 0.95), 0.15, 0.1, TP.new(0.45, 1.2))
    if panes:
        quad(0.12 * SW, 0.80 * SW, 0.25 * SD, 0.95 * SD, 0.25 * SH, mat_a)
        quad(0.22 * SW, 0.88 * SW, 0.20 * SD, 0.90 * SD, 0.15 * SH, mat_a if name == "one_material" else mat_b)
        if name == "sphere_and_pane":
            scene.add_sphere(SphereData.with_material(Vec3.new(F(0.45 * SW), F(floor_y(0.5 * SD) - 0.36 * SH), F(0.5 * SD)), F(0.07 * SW),
                                                      Material.new(ColorType.new(0.6, 0.9, 0.5), 0.0, 0.2, TP.new(0.6, 1.33))))
        if name == "opaque_between":
            quad(0.40 * SW, 0.55 * SW, 0.45 * SD, 0.60 * SD, 0.20 * SH, opaque)
    scene.add_light(PointLight.new(Vec3.new(F(0.5 * SW), F(0.02 * SH), F(0.45 * SD)), ColorType.new(0.9, 0.8, 0.7), 1.0).into())
    if name == "second_light":
        # between the panes (above B, below A) and well inside A's outline: its rays to the floor cross B only
        scene.add_light(PointLight.new(Vec3.new(F(0.5 * SW), F(floor_y(0.55 * SD) - 0.20 * SH), F(0.55 * SD)),
                                       ColorType.new(0.6, 0.9, 0.8), 0.5).into())
    return scene.flatten()


def child(out_dir):
    """One process = one value of RT_PRIMARY_GENERIC: every scene on every route, written to out_dir."""
    sys.path.insert(0, ROOT)
    from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi
    from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import ImageBuffer, RaytracerRenderer

    routes = {"lists": {}, "walk": dict(shadow_candidate_cap=1), "no_sharing": dict(shadow_candidate_cap=_abi.RT_CAND_CAP_NONE)}
    for name in SCENES:
        for route, tuning in routes.items():
            cfg = config()
            flat = build_scene(name, cfg)
            print(f"[child] {name} {route}", file=sys.stderr, flush=True)
            buf = ImageBuffer.new(cfg.width, cfg.height)
            r = RaytracerRenderer(cfg, device=0, scene_budget=BUDGET)
            planes = r.render(buf, flat, aux=True, tuning=tuning)
            np.savez(os.path.join(out_dir, f"{name}_{route}.npz"), argb=np.asarray(buf.buffer), rgb=planes["rgb"], hit_id=planes["hit_id"])
    with open(os.path.join(out_dir, "done.json"), "w") as fh:
        json.dump({"scenes": SCENES, "routes": sorted(routes)}, fh)


def run_child(tmp, generic):
    out = tmp / ("generic" if generic else "default")
    out.mkdir()
    env = dict(os.environ, RT_TRACE_LAUNCHES="1")
    env.pop("RT_PRIMARY_GENERIC", None)
    if generic:
        env["RT_PRIMARY_GENERIC"] = "1"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), str(out)]
    proc = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    assert proc.returncode == 0, (cmd, proc.returncode, proc.stderr[-4000:])
    # the launch trace per (scene, route)
    logs, key = {}, None
    for line in proc.stderr.splitlines():
        if line.startswith("[child] "):
            key = tuple(line.split()[1:3])
            logs[key] = ""
        elif key:
            logs[key] += line + "\n"
    return out, logs


@pytest.fixture(scope="module")
def frames(tmp_path_factory):
    """(directory, launch traces) of the default child and of the RT_PRIMARY_GENERIC=1 child; the second starts only if the
    first came back clean"""
    tmp = tmp_path_factory.mktemp("occluder_memo")
    return run_child(tmp, generic=False), run_child(tmp, generic=True)


def load(d, name, route):
    return np.load(d / f"{name}_{route}.npz")


def same_frame(a, b, what):
    for plane in ("argb", "rgb", "hit_id"):
        assert a[plane].shape == b[plane].shape and a[plane].dtype == b[plane].dtype and a[plane].dtype.itemsize == 4, (what, plane)
        # every pixel, the float planes as their bits
        x, y = a[plane].view(np.uint32), b[plane].view(np.uint32)
        assert np.array_equal(x, y), (what, plane, int((x != y).sum()), "values differ")


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_memo_frame_equals_every_unmemoised_route(frames, name):
    (d_def, logs), (d_gen, logs_gen) = frames
    ref = load(d_def, name, "lists")
    assert ref["argb"].any() and (ref["hit_id"] >= 0).any(), name
    # which kernel rendered what
    assert "rt_primary_soft10_kernel: workgroups" in logs[(name, "lists")], logs[(name, "lists")][-1500:]
    assert "rt_primary_soft10_kernel: workgroups" in logs[(name, "walk")], logs[(name, "walk")][-1500:]
    assert "rt_primary_kernel: workgroups" in logs[(name, "no_sharing")], logs[(name, "no_sharing")][-1500:]
    for route in ROUTES:
        assert "rt_primary_soft" not in logs_gen[(name, route)], (route, logs_gen[(name, route)][-1500:])
    same_frame(load(d_def, name, "walk"), ref, (name, "per-sample walks in the memo kernel"))
    same_frame(load(d_def, name, "no_sharing"), ref, (name, "per-sample walks in rt_primary_kernel"))
    for route in ROUTES:
        same_frame(load(d_gen, name, route), ref, (name, route, "RT_PRIMARY_GENERIC=1"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_memo_frame_is_the_oracles_frame_and_the_panes_matter(frames, name):
    import oracle_lib

    (d_def, _), _ = frames
    cfg = config()
    ref = load(d_def, name, "lists")
    argb_o, planes_o, _ = oracle_lib.render(build_scene(name, cfg), cfg)
    assert np.array_equal(ref["hit_id"], planes_o["hit_id"])
    d = np.abs(ref["rgb"] - planes_o["rgb"]).max(axis=1)
    print(f"{name}: max |dRGB| vs oracle = {float(d.max()):.3e}")
    assert float(d.max()) <= RGB_TOL, (name, float(d.max()))
    # the scene does what it is meant to do: without the panes a good part of the floor is brighter
    _, bare, _ = oracle_lib.render(build_scene(name, cfg, panes=False), cfg)
    # (the floor's two triangles come first; spheres take the ids before the triangles', and the bare scene has none)
    ns = 1 if name == "sphere_and_pane" else 0
    floor = np.isin(planes_o["hit_id"], (ns, ns + 1)) & np.isin(bare["hit_id"], (0, 1))
    shaded = floor & (np.abs(bare["rgb"] - planes_o["rgb"]).max(axis=1) > 1e-3)
    assert int(shaded.sum()) >= 150, (name, int(shaded.sum()), int(floor.sum()))


if __name__ == "__main__":
    child(sys.argv[1])
