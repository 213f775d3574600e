"""Thin-lens camera views on the GPU (rt_view_create_lens, rt_view_set_lens): the lens generator against its host model, word
for word; a lens frame against the resolve model of a GPU trace of the model's rays, bit for bit, and against the CPU
reference; the lens switched off against a plain view; a lens that changes on a reused order; adaptive frames -- the mask
against the refine model OR-ed with the defocus model on the GPU's own plane 0, the frame against the adaptive resolve model;
the device forms with torch tensors; the refusals that need a view; the C example.

Plane 0 of an adaptive frame stays inside the view.  The frame of a ONE-sample lens view with the table's sample 0 and the same
lens holds the same rays with the same batch indices traced by the same kernels: it stands for the base planes here, as in
tests/test_view_adaptive_gpu.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, _abi, _lib, camera
from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceView, ImageBuffer, RaytracerRenderer

import trace_rays_cases as tr
import view_adapt_cases as va
import view_cases as vc
import view_lens_cases as vl
from test_scene_pack_host import ROOT
from test_view_gpu import SOFT, _scene

gpu = pytest.mark.gpu
PLANES = ("rgb", "valid", "id", "t")
# the spheres scene, a "realistic" case (reflections and refractions: the trace blocks) and a soft-shadow case
CASES = [("spheres", ["realistic", "soft_shadows"], SOFT), ("test_scene", ["realistic"], {}), ("test_scene", ["soft_shadows"], SOFT)]
ORDERS = ("once", "none")
# sample counts 1, 7, 9, 16 and 24 over both frames
VIEWS = ((37, 29, "repeats9"), (64, 4, "repeats24"), (64, 4, "centre1"), (37, 29, "distinct7"), (37, 29, "config16"))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return tr.build_ref(tmp_path_factory.mktemp("lensref"))


def lens_view(w, h, table, order="once", ln=None, adaptive=False):
    smp, ls = vl.lens_tables()[table]
    view = DeviceView(0, w, h, smp, order=order, camera=vc.pinhole(w, h).view_camera(), lens_samples=ls)
    view.set_lens(vl.frame_lens(w, h) if ln is None else ln)
    return view.enable_adaptive() if adaptive else view


def planes(r, argb=None):
    out = {k: np.asarray(getattr(r, k)) for k in PLANES}
    out["valid"] = out["valid"].astype(bool)
    if argb is not None:
        out["argb"] = argb
    return out


def expected(ds, cfg, w, h, table, ln):
    """the resolve model of a GPU trace of the lens model's rays -> (pixel planes, the trace's per-ray planes, its stats, plane_of)"""
    smp, ls = vl.lens_tables()[table]
    o, d, plane_of, nd = vl.model_rays(w, h, smp, ls, vc.pinhole(w, h).view_camera(), ln)
    rays = ds.trace_rays(o, d, cfg)
    return vc.resolve_model(w * h, smp.shape[0], plane_of, rays), rays, dict(ds.last_trace_stats), plane_of


# ---- the generator ------------------------------------------------------------------------------------------------------------
@gpu
def test_device_lens_rays_equal_the_model():
    """rt_view_rays on a lens view (the kernel, staged) equals rt_view_lens_rays_model in every word, for every table and both
    frames; with the aperture set to 0 afterwards, the pinhole rays of the planes' pixel offsets; the coc plane is in the bytes"""
    for w, h in vc.FRAMES:
        cam = vc.pinhole(w, h).view_camera()
        for table, (smp, ls) in vl.lens_tables().items():
            view = lens_view(w, h, table)
            info = view.info
            for ln in (vl.frame_lens(w, h), vl.lens(aperture=0.0)):
                view.set_lens(ln)
                o, d, plane_of, nd = vl.model_rays(w, h, smp, ls, cam, ln)
                go, gd = view.rays()
                n_o, n_d = int((vc.bits(go) != vc.bits(o)).sum()), int((vc.bits(gd) != vc.bits(d)).sum())
                print(f"{w}x{h} {table} A={ln.aperture}: {info['n_rays']} rays of {nd} planes; origin words differing {n_o}, direction {n_d}")
                assert info["n_distinct"] == nd and info["n_rays"] == nd * w * h == o.shape[0]
                assert np.array_equal(view.plane_of(), plane_of) and n_o == 0 and n_d == 0
            if vc.brute_dedup(smp)[1] == nd:
                plain = DeviceView(0, w, h, smp, camera=cam)
                assert info["bytes"] >= plain.info["bytes"] + 4 * w * h
                plain.close()
            view.close()


# ---- a lens frame is the resolve model of a GPU trace ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("scene,features,kw", CASES)
def test_lens_frame_equals_the_resolve_model_of_a_gpu_trace(scene, features, kw, order):
    flat, ds = _scene(scene)
    cfg = RenderConfig.from_features(features, **kw)
    for w, h, table in VIEWS:
        ln = vl.frame_lens(w, h)
        want, _, want_stats, _ = expected(ds, cfg, w, h, table, ln)
        view = lens_view(w, h, table, order=order)
        argb = np.full(w * h, vc.FILL, np.uint32)
        got = ds.render_view(view, cfg, argb=argb)
        st = ds.last_trace_stats
        label = f"{scene} {features} order={order} {w}x{h} {table}"
        print(f"{label}: {int(want['valid'].sum())} of {w * h} pixels written")
        vc.assert_pixels_equal(got, want, label)
        assert np.array_equal(argb, want["argb"]) and np.all(argb[~want["valid"]] == vc.FILL), label
        for k in tr.COUNTERS + ("rays_traced",):
            assert st[k] == want_stats[k], (label, k, st[k], want_stats[k])
        view.close()


@gpu
@pytest.mark.parametrize("scene,features,kw", CASES)
def test_lens_frame_against_the_cpu_reference(ref, scene, features, kw):
    """the resolve model applied to trace_rays_cases.ref_trace of the lens model's rays (ray i keeps light-cloud key i), the bars
    of test_view_against_the_cpu_reference: valid and id equal, t bit-exact, |dRGB| <= 1e-4 with no pixel excluded, counters equal"""
    flat, ds = _scene(scene)
    cfg = RenderConfig.from_features(features, **kw)
    for w, h, table in VIEWS:
        smp, ls = vl.lens_tables()[table]
        ln = vl.frame_lens(w, h)
        o, d, plane_of, nd = vl.model_rays(w, h, smp, ls, vc.pinhole(w, h).view_camera(), ln)
        rays = tr.ref_trace(ref, flat, cfg, o, d, index=np.arange(o.shape[0], dtype=np.uint32))
        want = vc.resolve_model(w * h, smp.shape[0], plane_of, rays)
        want["counters"] = rays["counters"]
        view = lens_view(w, h, table)
        got = ds.render_view(view, cfg)
        tr.check_against_ref(got, ds.last_trace_stats, want, what=f"{scene} {features} {w}x{h} {table}")
        view.close()


# ---- the lens switched off --------------------------------------------------------------------------------------------------------
@gpu
def test_aperture_zero_is_the_plain_view():
    """distinct7 has no repeated pixel offset: the lens view's planes are the plain view's, ray for ray, so the frames are equal
    in every case, soft shadows included, whether the lens was never set or set to A == 0.  config16 with 16 distinct lens offsets
    has 16 planes where the plain view has 9: other ray indices, hence other light clouds -- equal without soft shadows."""
    w, h = vc.FRAMES[0]
    cam = vc.pinhole(w, h).view_camera()
    for scene, features, kw in CASES + [("test_scene", [], {})]:
        flat, ds = _scene(scene)
        cfg = RenderConfig.from_features(features, **kw)
        for table in ("distinct7", "config16"):
            if table == "config16" and "soft_shadows" in features:
                continue
            smp, ls = vl.lens_tables()[table]
            plain = DeviceView(0, w, h, smp, camera=cam)
            a0 = np.full(w * h, vc.FILL, np.uint32)
            want = planes(ds.render_view(plain, cfg, argb=a0), a0)
            plain.close()
            view = DeviceView(0, w, h, smp, camera=cam, lens_samples=ls)
            for step in ("never set", "set to 0", "opened and closed again"):
                if step == "set to 0":
                    view.set_lens(vl.lens(aperture=0.0))
                if step == "opened and closed again":
                    view.set_lens(vl.frame_lens(w, h))
                    opened = ds.render_view(view, cfg)
                    assert (vc.bits(np.asarray(opened.rgb)) != vc.bits(want["rgb"])).any(), "the lens changed nothing"
                    view.set_lens(vl.lens(aperture=0.0, focus_distance=9.0))
                a1 = np.full(w * h, vc.FILL, np.uint32)
                got = ds.render_view(view, cfg, argb=a1)
                vc.assert_pixels_equal(got, want, f"{scene} {features} {table} {step}")
                assert np.array_equal(a1, a0)
            view.close()


@gpu
def test_a_changed_lens_on_a_reused_order_renders_what_a_fresh_view_renders():
    flat, ds = _scene("test_scene")
    cfg = RenderConfig.from_features(["soft_shadows"], **SOFT)
    w, h, table = VIEWS[0]
    view = lens_view(w, h, table)
    first = ds.render_view(view, cfg)
    assert view.info["order_ms"] > 0.0
    for ln in (vl.lens(aperture=0.4, focus_distance=2.5), vl.lens(aperture=0.25, focus_distance=2.0), vl.lens(aperture=0.0)):
        view.set_lens(ln)
        a1, a2 = np.full(w * h, vc.FILL, np.uint32), np.full(w * h, vc.FILL, np.uint32)
        got = ds.render_view(view, cfg, argb=a1)
        assert view.info["order_built"] and view.info["order_ms"] == 0.0  # (the first lens's order, reused)
        fresh = lens_view(w, h, table, ln=ln)
        want = ds.render_view(fresh, cfg, argb=a2)
        vc.assert_pixels_equal(got, planes(want), f"A={ln.aperture} F={ln.focus_distance}")
        assert np.array_equal(a1, a2) and (vc.bits(np.asarray(first.rgb)) != vc.bits(np.asarray(got.rgb))).any()
        fresh.close()
    view.close()


# ---- adaptive frames ------------------------------------------------------------------------------------------------------------
def adaptive_references(ds, cfg, w, h, table, ln):
    """-> (the full lens frame by rt_render_view, plane 0 = the frame of the one-sample lens view, the per-ray planes of a GPU
    trace of the model's rays, plane_of)"""
    smp, ls = vl.lens_tables()[table]
    cam = vc.pinhole(w, h).view_camera()
    full_view = lens_view(w, h, table, ln=ln)
    one_view = DeviceView(0, w, h, smp[:1], camera=cam, lens_samples=ls[:1]).set_lens(ln)
    a_full, a_one = np.full(w * h, vc.FILL, np.uint32), np.full(w * h, vc.FILL, np.uint32)
    full = planes(ds.render_view(full_view, cfg, argb=a_full), a_full)
    one = planes(ds.render_view(one_view, cfg, argb=a_one), a_one)
    full_view.close(), one_view.close()
    _, rays, _, plane_of = expected(ds, cfg, w, h, table, ln)
    return full, one, rays, plane_of


def check_adaptive(label, got, mask, info, w, h, table, rf, ln, one, rays, plane_of):
    """mask and n_refined: rt_view_refine_model OR-ed with rt_view_defocus_model on plane 0; frame: rt_view_resolve_adaptive_model"""
    smp, _ = vl.lens_tables()[table]
    n = w * h
    edges, n_edges = va.refine_model(w, h, rf, one)
    coc, want_mask, added = vl.defocus_model(w, h, smp[0], vc.pinhole(w, h).view_camera(), ln, one["valid"], one["t"], mask=edges)
    mask = np.asarray(mask).astype(bool)
    print(f"{label}: {int(mask.sum())} of {n} refined (rule {n_edges}, criterion +{added}); mask differs in {int((mask != want_mask).sum())}; info {info}")
    assert np.array_equal(mask, want_mask), label
    assert info["n_refined"] == int(mask.sum()) == n_edges + added and info["n_live_rays"] == info["n_refined"] * (int(plane_of.max())), label
    want = va.resolve_adaptive_model(n, smp.shape[0], plane_of, mask, one, rays if plane_of.max() else None)
    vc.assert_pixels_equal(got, want, label)
    assert np.array_equal(got["argb"], want["argb"]), label
    return edges, mask, added


@gpu
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("features,kw", va.SHADINGS)
def test_adaptive_lens_frame_mask_and_pixels(features, kw, order):
    """two frames each (the second reuses the order and its plane-0 part in mode "once"); the criterion adds pixels and leaves others"""
    flat, ds = _scene("test_scene")
    cfg = RenderConfig.from_features(features, **kw)
    rf = va.refine()
    for w, h, table in (VIEWS[0], VIEWS[1], VIEWS[4]):
        ln = vl.frame_lens(w, h, adaptive=True)
        full, one, rays, plane_of = adaptive_references(ds, cfg, w, h, table, ln)
        view = lens_view(w, h, table, order=order, ln=ln, adaptive=True)
        for frame in range(2):
            argb = np.full(w * h, vc.FILL, np.uint32)
            got = ds.render_view(view, cfg, argb=argb, refine=va_rule())
            edges, mask, added = check_adaptive(f"{features} order={order} {w}x{h} {table} frame {frame}", planes(got, argb), got.mask, view.adaptive_info,
                                                w, h, table, rf, ln, one, rays, plane_of)
            assert added > 0 and not mask.all()
            # a refined pixel is the full lens frame's pixel
            for k in PLANES:
                assert np.array_equal(vc.bits(np.asarray(getattr(got, k))[mask]), vc.bits(full[k][mask])), k
        view.close()


def va_rule(criteria=va.DEPTH | va.COLOUR):
    from hslu_i.ba_raytracing.f2501_raytracer_amd import Refine

    return Refine(criteria=criteria, colour_tol=va.COLOUR_TOL, depth_tol=va.DEPTH_TOL)


@gpu
def test_every_gives_the_full_lens_frame_and_an_infinite_tolerance_todays_mask():
    flat, ds = _scene("test_scene")
    cfg = RenderConfig.from_features(["soft_shadows"], **SOFT)
    for w, h, table in (VIEWS[0], VIEWS[1]):
        ln = vl.frame_lens(w, h, adaptive=True)
        full, one, rays, plane_of = adaptive_references(ds, cfg, w, h, table, ln)
        view = lens_view(w, h, table, ln=ln, adaptive=True)
        argb = np.full(w * h, vc.FILL, np.uint32)
        got = ds.render_view(view, cfg, argb=argb, refine=va_rule(va.EVERY))
        assert np.asarray(got.mask).all() and view.adaptive_info["n_refined"] == w * h  # (the criterion counts no pixel twice)
        vc.assert_pixels_equal(planes(got, argb), full, f"{w}x{h} {table} every")
        assert np.array_equal(argb, full["argb"])
        # coc_tol = +inf: the mask is the refine rule's alone, on the same lens frame
        off = vl.frame_lens(w, h, adaptive=True, coc_tol=vl.INF)
        view.set_lens(off)
        argb = np.full(w * h, vc.FILL, np.uint32)
        got = ds.render_view(view, cfg, argb=argb, refine=va_rule())
        edges, mask, added = check_adaptive(f"{w}x{h} {table} coc_tol inf", planes(got, argb), got.mask, view.adaptive_info, w, h, table, va.refine(), off,
                                            one, rays, plane_of)
        assert added == 0 and np.array_equal(mask, edges)
        # and no criterion at all but the lens's: the mask is the defocus model's alone
        view.set_lens(ln)
        argb = np.full(w * h, vc.FILL, np.uint32)
        got = ds.render_view(view, cfg, argb=argb, refine=va_rule(0))
        edges, mask, added = check_adaptive(f"{w}x{h} {table} criteria 0", planes(got, argb), got.mask, view.adaptive_info, w, h, table, va.refine(0), ln,
                                            one, rays, plane_of)
        assert not edges.any() and added == int(mask.sum()) > 0
        view.close()


@gpu
@pytest.mark.parametrize("spread", [0, 1, 16])
def test_the_spread_kernel_at_its_narrowest_and_widest_halo(spread):
    """spread 0 (the pixel alone), 1, and 16 (a halo as wide as the tile: the 37 x 29 frame's six tiles read far outside the frame,
    the 64 x 4 frame's tiles are higher than the frame) with tolerances that let few and many pixels through; no refine criterion,
    so the mask is the criterion's alone"""
    flat, ds = _scene("test_scene")
    cfg = RenderConfig.from_features([])
    for w, h, table in (VIEWS[0], VIEWS[1]):
        refs = {}
        view = lens_view(w, h, table, adaptive=True)
        for aperture in (vl.APERTURES[(w, h)], 8 * vl.APERTURES[(w, h)]):
            for tol in (0.25, 2.0):
                ln = vl.lens(aperture=aperture, focus_distance=vl.FOCUS, coc_tol=tol, spread=spread)
                if aperture not in refs:
                    refs[aperture] = adaptive_references(ds, cfg, w, h, table, ln)
                full, one, rays, plane_of = refs[aperture]
                view.set_lens(ln)
                argb = np.full(w * h, vc.FILL, np.uint32)
                got = ds.render_view(view, cfg, argb=argb, refine=va_rule(0))
                check_adaptive(f"{w}x{h} {table} A={aperture} tol={tol} spread={spread}", planes(got, argb), got.mask, view.adaptive_info, w, h, table,
                               va.refine(0), ln, one, rays, plane_of)
        view.close()


@gpu
def test_render_camera_with_a_lens():
    w, h = vc.FRAMES[0]
    cfg = vc.frame_config(["anti_aliasing"], w, h)
    cam = vc.pinhole(w, h)
    flat = va.scene_flat()
    r = RaytracerRenderer(cfg, device=0)
    thin = camera.ThinLens(vl.APERTURE, vl.FOCUS, *vl.ADAPTIVE[(w, h)])
    bufs = [ImageBuffer.new_with_color(w, h, vc.FILL) for _ in range(3)]
    sharp = r.render_camera(bufs[0], flat, cam, samples="config", order=True)
    full = r.render_camera(bufs[1], flat, cam, samples="config", order=True, lens=thin)
    n_full = r.last_stats["rays_primary"]
    got = r.render_camera(bufs[2], flat, cam, samples="config", order=True, lens=thin, refine=va_rule())
    mask = np.asarray(got.mask).astype(bool)
    assert (vc.bits(np.asarray(sharp.rgb)) != vc.bits(np.asarray(full.rgb))).any() and 0 < mask.sum() < w * h and r.last_stats["rays_primary"] < n_full
    assert np.array_equal(vc.bits(np.asarray(got.rgb)[mask]), vc.bits(np.asarray(full.rgb)[mask]))
    assert np.array_equal(bufs[2].buffer[mask], bufs[1].buffer[mask])
    with pytest.raises(ValueError):
        r.render_camera(bufs[0], flat, cam, lens=thin)


# ---- torch device tensors ------------------------------------------------------------------------------------------------------
# torch is imported BEFORE librt_hip.so is loaded, so the test that hands tensors to the library runs in a child process of
# its own, under its own time limit (as in tests/test_view_gpu.py)
CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import torch  # noqa: F401  (first)
import test_view_lens_gpu as T
T.device_forms_with_torch_tensors()
print("CHILD-OK")
"""


@gpu
def test_device_forms_with_torch_tensors():
    """rt_view_rays_device, rt_render_view_device and rt_render_view_adaptive_device on a lens view, tensors on a non-default
    stream: the model's rays; the resolve model of a GPU trace; the adaptive mask and frame -- two frames each, both order modes"""
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, "-c", CHILD.format(root=os.path.dirname(here), tests=here)], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "CHILD-OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def device_forms_with_torch_tensors():
    import torch

    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    flat, ds = _scene("test_scene")
    cfg = RenderConfig.from_features(["soft_shadows"], **SOFT)
    rf = va.refine()
    for w, h, table in (VIEWS[0], VIEWS[1]):
        smp, ls = vl.lens_tables()[table]
        ln = vl.frame_lens(w, h, adaptive=True)
        o, d, _, _ = vl.model_rays(w, h, smp, ls, vc.pinhole(w, h).view_camera(), ln)
        want, _, _, _ = expected(ds, cfg, w, h, table, ln)
        full, one, rays, plane_of = adaptive_references(ds, cfg, w, h, table, ln)
        for order in ORDERS:
            view = lens_view(w, h, table, order=order, ln=ln, adaptive=True)
            with torch.cuda.stream(s):
                to, td = view.rays(torch_device=True)
            s.synchronize()
            assert np.array_equal(vc.bits(to.cpu().numpy()), vc.bits(o)) and np.array_equal(vc.bits(td.cpu().numpy()), vc.bits(d)), (table, order)
            for frame in range(2):
                label = f"order={order} {w}x{h} {table} device frame {frame}"
                with torch.cuda.stream(s):
                    targb = torch.full((w * h,), vc.FILL, dtype=torch.int32, device=dev)
                    got = ds.render_view(view, cfg, argb=targb)
                s.synchronize()
                assert isinstance(got.rgb, torch.Tensor) and got.rgb.device == dev
                vc.assert_pixels_equal({k: getattr(got, k).cpu().numpy() for k in PLANES}, want, label)
                assert np.array_equal(targb.cpu().numpy().view(np.uint32), want["argb"]), label
                with torch.cuda.stream(s):
                    targb = torch.full((w * h,), vc.FILL, dtype=torch.int32, device=dev)
                    got = ds.render_view(view, cfg, argb=targb, refine=va_rule())
                s.synchronize()
                host = {k: getattr(got, k).cpu().numpy() for k in PLANES}
                host["valid"], host["argb"] = host["valid"].astype(bool), targb.cpu().numpy().view(np.uint32)
                _, mask, added = check_adaptive(label + " adaptive", host, got.mask.cpu().numpy(), view.adaptive_info, w, h, table, rf, ln, one, rays, plane_of)
                assert added > 0
            view.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals_that_need_a_view():
    lib = _lib.load()
    flat, ds = _scene("test_scene")
    smp, ls = vl.lens_tables()["repeats9"]
    p, keep = _abi.make_params(RenderConfig.from_features([]))
    buf = np.zeros((64, 3), np.float32)
    out = _abi.rt_ray_radiance(buf.ctypes.data, None, None, None, None)
    rf = va.refine()

    def refused(rc, part):
        msg = lib.rt_last_error().decode()
        assert rc == _abi.RT_ERR_INVALID_ARG and part in msg, (rc, msg)

    plain = DeviceView(0, 8, 8, smp, camera=vc.pinhole(8, 8).view_camera())
    refused(lib.rt_view_set_lens(plain.handle, C.byref(vl.lens())), "rt_view_create_lens")
    plain.close()
    # a reference camera has no lens: refused while the lens is open, allowed once it is closed
    ref_cam = camera.reference_view_camera(vc.frame_config([], 8, 8))
    view = DeviceView(0, 8, 8, smp, camera=ref_cam, lens_samples=ls).enable_adaptive()
    _lib.check(lib.rt_render_view(ds.handle, view.handle, C.byref(p), C.byref(out), None))  # (no rt_view_set_lens yet: A == 0)
    view.set_lens(vl.lens())
    rays = np.zeros((9 * 64, 3), np.float32)
    refused(lib.rt_render_view(ds.handle, view.handle, C.byref(p), C.byref(out), None), "has no lens")
    refused(lib.rt_render_view_device(ds.handle, view.handle, C.byref(p), C.byref(out), None), "has no lens")
    refused(lib.rt_render_view_adaptive(ds.handle, view.handle, C.byref(p), C.byref(rf), C.byref(out), None, None), "has no lens")
    refused(lib.rt_view_rays(view.handle, rays.ctypes.data, rays.ctypes.data), "has no lens")
    for ln, part in ((vl.lens(spread=17), "spread"), (vl.lens(aperture=-1.0), "aperture"), (vl.lens(focus_distance=0.0), "focus_distance")):
        refused(lib.rt_view_set_lens(view.handle, C.byref(ln)), part)
    refused(lib.rt_render_view(ds.handle, view.handle, C.byref(p), C.byref(out), None), "has no lens")  # (a refused lens changed nothing)
    view.set_lens(vl.lens(aperture=0.0))
    _lib.check(lib.rt_render_view(ds.handle, view.handle, C.byref(p), C.byref(out), None))
    _lib.check(lib.rt_render_view_adaptive(ds.handle, view.handle, C.byref(p), C.byref(rf), C.byref(out), None, None))
    view.close()


# ---- the C example ------------------------------------------------------------------------------------------------------------
def build_example(out_dir):
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    exe = os.path.join(str(out_dir), "c_view_lens_example")
    subprocess.check_call(["gcc", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_view_lens_example.c"),
                           "-L", lib_dir, "-lrt_hip", f"-Wl,-rpath,{lib_dir}", "-lm", "-o", exe])
    return exe


def test_lens_example_links_against_the_abi(tmp_path):
    _lib.load()
    out = subprocess.run([build_example(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "lens model: 9 planes" in out.stdout
    assert "no HIP device" in out.stdout or "the mask equals the host models' mask" in out.stdout


@gpu
def test_lens_example_renders_on_the_gpu(tmp_path):
    out = subprocess.run([build_example(tmp_path)], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "the mask equals the host models' mask" in out.stdout and "every refined pixel equals the full lens frame's pixel" in out.stdout
