"""Thin-lens camera views without a device: the host models of the lens generator and of the defocus criterion (compiled from
csrc/rt_view_lens.h, the source of the kernels) against numpy restatements, bit for bit; the 4-tuple planes against a
brute-force comparison; the focus plane in float64; the lens switched off; and every refusal that needs no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, _lib, camera

import view_cases as vc
import view_lens_cases as vl

F32 = np.float32
TABLES = ("centre1", "distinct7", "repeats9", "config16", "repeats24")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cameras(w, h):
    return [vc.pinhole(w, h).view_camera(), vc.pinhole(w, h, eye=(0.62, 0.30, -1.4), target=(0.45, 0.5, 0.5), fov=47.0).view_camera()]


# ---- the lens ray ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", vc.FRAMES)
@pytest.mark.parametrize("table", TABLES)
def test_lens_rays_model_equals_the_numpy_formula(frame, table):
    """sample counts 1, 7, 9, 16, 24; two cameras; two lenses: every origin and direction word"""
    w, h = frame
    smp, ls = vl.lens_tables()[table]
    for cam in cameras(w, h):
        for ln in (vl.lens(), vl.lens(aperture=0.31, focus_distance=7.25)):
            o, d, plane_of, nd = vl.model_rays(w, h, smp, ls, cam, ln)
            wo, wd, wpo, wnd = vl.numpy_rays(w, h, smp, ls, cam, ln)
            assert nd == wnd and np.array_equal(plane_of, wpo)
            print(f"{table} {w}x{h}: {nd} planes; origin words differing {int((vc.bits(o) != vc.bits(wo)).sum())}, direction "
                  f"{int((vc.bits(d) != vc.bits(wd)).sum())}")
            assert np.array_equal(vc.bits(o), vc.bits(wo)) and np.array_equal(vc.bits(d), vc.bits(wd))


def test_planes_are_the_bit_distinct_four_tuples_in_first_occurrence_order():
    """same pixel offset with another lens offset: two planes; all four floats equal: one plane; a repeat of sample 0 in the second
    packet reads plane 0; -0.0 and 0.0 differ as bits"""
    w, h = 5, 3
    cam, ln = vc.pinhole(w, h).view_camera(), vl.lens()
    expected = {"centre1": 1, "distinct7": 7, "repeats9": 8, "config16": 16, "repeats24": 22}
    for table, (smp, ls) in vl.lens_tables().items():
        _, _, plane_of, nd = vl.model_rays(w, h, smp, ls, cam, ln)
        wpo, wnd, _ = vl.brute_dedup4(smp, ls)
        assert nd == wnd == expected[table] and np.array_equal(plane_of, wpo), table
        assert nd >= vc.brute_dedup(smp)[1]
    smp, ls = vl.lens_tables()["repeats9"]
    _, _, plane_of, _ = vl.model_rays(w, h, smp, ls, cam, ln)
    assert plane_of[8] == 0 and plane_of[5] != plane_of[2] and np.array_equal(smp[5], smp[2])
    zero = np.zeros((3, 2), F32)
    ls = np.zeros((3, 2), F32)
    ls[1, 1] = -0.0
    _, _, plane_of, nd = vl.model_rays(w, h, zero, ls, cam, ln)
    assert nd == 2 and list(plane_of) == [0, 1, 0]
    # with the lens off the planes stay those of the 4-tuples
    _, _, plane_of0, nd0 = vl.model_rays(w, h, zero, ls, cam, vl.lens(aperture=0.0))
    assert nd0 == 2 and list(plane_of0) == [0, 1, 0]


@pytest.mark.parametrize("frame", vc.FRAMES)
def test_all_lens_samples_of_a_pixel_offset_meet_in_the_focus_plane(frame):
    """In float64, from the model's float32 rays.  P = eye + F d0, with d0 the float32 direction the pinhole model gives the pixel
    offset.  The lens ray is o = fl(eye + off), d = fl(fl(F d0) - off) with the SAME float `off` on both sides, so the point o + d
    of its line differs from P by three roundings only (u = 2^-24 each):
        o + d - P = (eye + off) e1 + F d0 e2 (1 + e3) + (F d0 - off) e3
        |o + d - P|_k <= u (|eye_k| + 2 |off_k| + 2 |F d0_k|) (1 + u)
    -- the roundings inside off cancel, those inside d0 are part of P's definition.  The distance of P from the line is at most
    the distance from that point.  The bound is also far below the lens offsets: the lines are distinct lines."""
    w, h = frame
    u = 2.0 ** -24
    smp = np.tile(vc.sample_tables(_abi.RT_VIEW_PINHOLE)["distinct7"][:3], (8, 1))  # 3 pixel offsets x 8 lens offsets
    ls = camera.lens_samples(24)
    n = w * h
    for cam in cameras(w, h):
        for ln in (vl.lens(), vl.lens(aperture=0.31, focus_distance=7.25)):
            A, F = float(F32(ln.aperture)), float(F32(ln.focus_distance))
            o, d, plane_of, nd = vl.model_rays(w, h, smp, ls, cam, ln)
            assert nd == 24
            _, d0, _, nd0 = vc.model_rays(w, h, smp[:3], cam)
            assert nd0 == 3
            eye = np.array(list(cam.eye), np.float64)
            worst = 0.0
            for k in range(24):
                P = eye + F * d0[(k % 3) * n:(k % 3 + 1) * n].astype(np.float64)
                ok, dk = o[k * n:(k + 1) * n].astype(np.float64), d[k * n:(k + 1) * n].astype(np.float64)
                off = ok - eye  # (|off| up to its own rounding: (1 + u) covers it)
                bound = np.linalg.norm(u * (np.abs(eye) + 2 * np.abs(off) * (1 + u) + 2 * np.abs(P - eye)) * (1 + u), axis=1)
                to_p = P - ok
                dist = np.linalg.norm(np.cross(to_p, dk), axis=1) / np.linalg.norm(dk, axis=1)
                worst = max(worst, float((dist / bound).max()))
                assert np.all(dist <= bound), (k, float(dist.max()), float(bound.min()))
                if k >= 3:
                    assert np.linalg.norm(ok[0] - o[(k % 3) * n].astype(np.float64)) > 1e3 * bound.max()  # another point of the lens
            print(f"{w}x{h} A={A} F={F}: the largest distance from the focus point is {worst:.3f} of its bound")


@pytest.mark.parametrize("table", TABLES)
def test_aperture_zero_gives_the_pinhole_rays_of_the_planes_pixel_offsets(table):
    """bit for bit rt_view_rays_model's rays, for both camera kinds (a reference camera is allowed while the lens is off)"""
    w, h = vc.FRAMES[0]
    smp, ls = vl.lens_tables()[table]
    cfg = vc.frame_config([], w, h)
    _, _, firsts = vl.brute_dedup4(smp, ls)
    for kind in vc.KINDS.values():
        cam = vc.view_camera(kind, cfg, w, h)
        o, d, plane_of, nd = vl.model_rays(w, h, smp, ls, cam, vl.lens(aperture=0.0))
        assert nd == len(firsts)
        n = w * h
        for u_, k0 in enumerate(firsts):
            wo, wd, _, _ = vc.model_rays(w, h, smp[k0:k0 + 1], cam)
            assert np.array_equal(vc.bits(o[u_ * n:(u_ + 1) * n]), vc.bits(wo)) and np.array_equal(vc.bits(d[u_ * n:(u_ + 1) * n]), vc.bits(wd))


def test_lens_samples_are_a_fixed_spiral_in_the_unit_disk():
    for n in (1, 7, 9, 16, 24, 64):
        s = camera.lens_samples(n)
        assert s.shape == (n, 2) and s.dtype == np.float32 and np.array_equal(s[0], [0.0, 0.0])
        assert np.all(np.hypot(s[:, 0].astype(np.float64), s[:, 1].astype(np.float64)) < 1.0)
        assert np.array_equal(s, camera.lens_samples(n)) and len({tuple(r) for r in s.tolist()}) == n
    with pytest.raises(ValueError):
        camera.lens_samples(0)
    st = camera.ThinLens(0.25, 3.0).struct()
    assert (st.abi_version, st.spread, st.aperture, st.focus_distance, st.coc_tol, st.reserved) == (_abi.RT_ABI_VERSION, 8, 0.25, 3.0, vl.INF, 0)


# ---- the defocus criterion ------------------------------------------------------------------------------------------------------
def synthetic(w, h, seed):
    """plane 0 with misses, depths on both sides of the focus plane, a NaN t, and all four corners far out of focus"""
    rng = np.random.default_rng(seed)
    n = w * h
    valid = rng.uniform(size=n) < 0.75
    t = rng.choice(F32([2.5, 2.5, 2.6, 2.4, 1.0, 1.9, 3.5, 9.0, 40.0, 1e-30, 3e38]), n).astype(F32)
    t[rng.integers(0, n)] = np.nan
    for c in (0, w - 1, n - w, n - 1):
        valid[c], t[c] = True, F32(0.3)
    t[~valid] = np.inf
    return valid, t


@pytest.mark.parametrize("size", [(37, 29), (64, 4), (1, 1), (1, 9), (40, 35)])
def test_defocus_model_equals_the_numpy_coc_and_the_brute_force_spread(size):
    """spread 0, 1, 8 and 16 (wider than the 64 x 4 frame is high; 40 x 35 spans several 16 x 16 tiles with the widest halo);
    tolerances from 0 up; misses have coc 0 and pick nothing; a valid pixel with a NaN t picks its whole window"""
    w, h = size
    cam = vc.pinhole(w, h).view_camera()
    s0 = F32([0.25, -0.125])
    for seed in range(2):
        valid, t = synthetic(w, h, seed)
        for spread in (0, 1, 8, 16):
            for tol in (0.0, 0.75, 3.0, 1e9):
                ln = vl.lens(coc_tol=tol, spread=spread)
                coc, mask, added = vl.defocus_model(w, h, s0, cam, ln, valid, t)
                want_coc = vl.numpy_coc(w, h, s0, cam, ln, valid, t)
                assert np.array_equal(vc.bits(coc), vc.bits(want_coc)), (size, seed)
                assert np.all(coc[~valid] == 0.0) and np.isnan(coc[valid & np.isnan(t)]).all()
                want = vl.brute_spread(w, h, coc, valid, tol, spread)
                assert np.array_equal(mask, want) and added == int(want.sum()), (size, seed, spread, tol, int(mask.sum()), int(want.sum()))
                # a NaN picks every pixel of its window, a corner its quadrant of one
                ys, xs = np.divmod(np.flatnonzero(valid & np.isnan(t)), w)
                for y, x in zip(ys, xs):
                    assert mask.reshape(h, w)[max(0, y - spread):y + spread + 1, max(0, x - spread):x + spread + 1].all()
        print(f"{w}x{h}: coc range {np.nanmin(coc):.3g} .. {np.nanmax(coc):.3g}, last mask {int(mask.sum())} of {w * h}")


def exact_case():
    """a camera whose centre pixel has d0 = forward = (0, 0, 1) exactly and whose H / (2 tan_half) is 16: at the centre pixel of
    the 37 x 29 frame coc = 16 A |t - F| / (t F) without a rounding error: A = 1/4, F = 1, t = 2 -> coc = 2 exactly"""
    w, h = 37, 29
    cam = _abi.rt_view_camera()
    cam.abi_version, cam.kind = _abi.RT_ABI_VERSION, _abi.RT_VIEW_PINHOLE
    cam.right[0], cam.up[1], cam.forward[2] = 1.0, 1.0, 1.0
    cam.tan_half_fov_y = 29.0 / 32.0
    centre = 14 * w + 18
    valid = np.zeros(w * h, bool)
    valid[centre] = True
    t = np.full(w * h, np.inf, F32)
    t[centre] = 2.0
    return w, h, cam, centre, valid, t


def test_a_coc_equal_to_the_tolerance_is_in_focus_and_one_equal_to_the_distance_reaches():
    w, h, cam, centre, valid, t = exact_case()
    zero = F32([0.0, 0.0])
    coc, mask, added = vl.defocus_model(w, h, zero, cam, vl.lens(aperture=0.25, focus_distance=1.0, coc_tol=1.0, spread=8), valid, t)
    assert coc[centre] == 2.0 and np.count_nonzero(coc) == 1
    want = np.zeros((h, w), bool)
    want[12:17, 16:21] = True  # distance 2 is covered (NOT 2 < 2), distance 3 is not
    assert np.array_equal(mask, want.ravel()) and added == 25
    # spread cuts the blur off
    _, mask, added = vl.defocus_model(w, h, zero, cam, vl.lens(aperture=0.25, focus_distance=1.0, coc_tol=1.0, spread=1), valid, t)
    want[:] = False
    want[13:16, 17:20] = True
    assert np.array_equal(mask, want.ravel()) and added == 9
    # coc == coc_tol exactly: not out of focus; the next float below the tolerance: out of focus
    _, mask, added = vl.defocus_model(w, h, zero, cam, vl.lens(aperture=0.25, focus_distance=1.0, coc_tol=2.0, spread=8), valid, t)
    assert not mask.any() and added == 0
    below = float(np.nextafter(F32(2.0), F32(0.0)))
    _, mask, added = vl.defocus_model(w, h, zero, cam, vl.lens(aperture=0.25, focus_distance=1.0, coc_tol=below, spread=8), valid, t)
    assert added == 25
    # in front of the focus plane as well: t = 1/2 -> coc = 4
    t[centre] = 0.5
    coc, mask, added = vl.defocus_model(w, h, zero, cam, vl.lens(aperture=0.25, focus_distance=1.0, coc_tol=1.0, spread=16), valid, t)
    assert coc[centre] == 4.0 and added == 81


def test_the_criterion_off_adds_nothing_and_masked_pixels_are_not_counted_twice():
    w, h, cam, centre, valid, t = exact_case()
    zero = F32([0.0, 0.0])
    before = np.zeros(w * h, bool)
    before[::3] = True
    for ln in (vl.lens(aperture=0.25, focus_distance=1.0, coc_tol=vl.INF), vl.lens(aperture=0.0, focus_distance=1.0, coc_tol=1.0)):
        coc, mask, added = vl.defocus_model(w, h, zero, cam, ln, valid, t, mask=before)
        assert added == 0 and np.array_equal(mask, before) and not coc.any()
    coc, mask, added = vl.defocus_model(w, h, zero, cam, vl.lens(aperture=0.25, focus_distance=1.0, coc_tol=1.0), valid, t, mask=before)
    picked = np.zeros((h, w), bool)
    picked[12:17, 16:21] = True
    assert np.array_equal(mask, before | picked.ravel()) and added == int((picked.ravel() & ~before).sum()) < 25


@pytest.mark.parametrize("frame", vc.FRAMES)
def test_the_gpu_lenses_add_some_pixels_and_not_all(frame, tmp_path):
    """a criterion that adds nothing, or a mask that is full, proves nothing: on the CPU reference's trace of plane 0 the lens of
    the GPU tests adds pixels the refine rule left out and leaves others unrefined"""
    from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig

    import trace_rays_cases as tr
    import view_adapt_cases as va

    w, h = frame
    ref = tr.build_ref(tmp_path)
    cam = vc.pinhole(w, h).view_camera()
    smp, ls = vl.lens_tables()["repeats9"]
    ln = vl.frame_lens(w, h, adaptive=True)
    o, d, _, _ = vl.model_rays(w, h, smp, ls, cam, ln)
    n = w * h
    rays = tr.ref_trace(ref, va.scene_flat(), RenderConfig.from_features([]), o[:n], d[:n], index=np.arange(n, dtype=np.uint32))
    edges, _ = va.refine_model(w, h, va.refine(), rays)
    coc, mask, added = vl.defocus_model(w, h, smp[0], cam, ln, rays["valid"], rays["t"], mask=edges)
    print(f"{w}x{h}: {int(edges.sum())} refined by the rule, {added} added by the criterion, {int(mask.sum())} of {n} in all; coc up to {coc.max():.2f}")
    assert added > 0 and mask.sum() < n and np.all(mask[edges])


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _refused(rc, part):
    msg = _lib.load().rt_last_error().decode()
    assert rc == _abi.RT_ERR_INVALID_ARG and part in msg, (rc, msg)


def bad_lenses():
    """(an rt_view_lens, a part of the message it is refused with)"""
    out = [(vl.lens(version=2), "rt_view_lens.abi_version"), (vl.lens(spread=17), "spread"), (vl.lens(reserved=1), "reserved")]
    out += [(vl.lens(aperture=a), "aperture") for a in (-1e-9, float("nan"), vl.INF)]
    out += [(vl.lens(focus_distance=f), "focus_distance") for f in (0.0, -1.0, float("nan"), vl.INF)]
    out += [(vl.lens(coc_tol=c), "coc_tol") for c in (-1e-9, float("nan"), -vl.INF)]
    return out


def test_lens_calls_are_refused_before_any_device_is_touched():
    lib = _lib.load()
    fake = C.c_void_p(0x1000)  # never dereferenced: every check below comes first
    w, h = 8, 8
    smp, ls = vl.lens_tables()["repeats9"]
    d, keep = vc.desc(w, h, smp)
    cam = vc.pinhole(w, h).view_camera()
    good = vl.lens()
    out = C.c_void_p()
    nd = C.c_uint32()
    po = np.zeros(64, np.uint8)
    valid, t = np.ones(w * h, np.uint8), np.ones(w * h, F32)
    create = lambda dd, l: lib.rt_view_create_lens(dd, l, 0, C.byref(out))  # noqa: E731
    rays = lambda dd, l, c, ln: lib.rt_view_lens_rays_model(dd, l, c, ln, None, None, po.ctypes.data, C.byref(nd))  # noqa: E731
    defocus = lambda dd, c, ln, v=valid.ctypes.data, tt=t.ctypes.data: lib.rt_view_defocus_model(dd, c, ln, v, tt, None, None, None)  # noqa: E731
    # NULL pointers and versions
    _refused(create(None, ls.ctypes.data), "null")
    _refused(lib.rt_view_create_lens(C.byref(d), ls.ctypes.data, 0, None), "null")
    _refused(create(C.byref(d), None), "null lens sample table")
    _refused(rays(C.byref(d), None, C.byref(cam), C.byref(good)), "null lens sample table")
    _refused(rays(None, ls.ctypes.data, C.byref(cam), C.byref(good)), "null view description")
    _refused(rays(C.byref(d), ls.ctypes.data, None, C.byref(good)), "null camera")
    _refused(rays(C.byref(d), ls.ctypes.data, C.byref(cam), None), "null lens")
    _refused(lib.rt_view_set_lens(None, C.byref(good)), "null view")
    _refused(lib.rt_view_set_lens(fake, None), "null lens")
    _refused(defocus(None, C.byref(cam), C.byref(good)), "null view description")
    _refused(defocus(C.byref(d), None, C.byref(good)), "null camera")
    _refused(defocus(C.byref(d), C.byref(cam), None), "null lens")
    _refused(defocus(C.byref(d), C.byref(cam), C.byref(good), None), "both required")
    _refused(defocus(C.byref(d), C.byref(cam), C.byref(good), valid.ctypes.data, None), "both required")
    bad_d, keep2 = vc.desc(w, h, smp)
    bad_d.abi_version = 2
    _refused(create(C.byref(bad_d), ls.ctypes.data), "rt_view_desc.abi_version")
    # a non-finite lens offset
    for v in (np.nan, np.inf, -np.inf):
        bad = ls.copy()
        bad[4, 1] = v
        _refused(create(C.byref(d), bad.ctypes.data), "sample 4 has a non-finite lens offset")
        _refused(rays(C.byref(d), bad.ctypes.data, C.byref(cam), C.byref(good)), "non-finite lens offset")
    # the lens struct, through every call that takes one
    for ln, part in bad_lenses():
        _refused(lib.rt_view_set_lens(fake, C.byref(ln)), part)
        _refused(rays(C.byref(d), ls.ctypes.data, C.byref(cam), C.byref(ln)), part)
        _refused(defocus(C.byref(d), C.byref(cam), C.byref(ln)), part)
    assert "rt_view_defocus_model" in lib.rt_last_error().decode()
    # a reference camera has no lens; with the lens off it is allowed
    ref_cam = vc.view_camera(_abi.RT_VIEW_REFERENCE, vc.frame_config([], w, h), w, h)
    _refused(rays(C.byref(d), ls.ctypes.data, C.byref(ref_cam), C.byref(good)), "has no lens")
    _refused(defocus(C.byref(d), C.byref(ref_cam), C.byref(vl.lens(coc_tol=1.0))), "has no lens")
    assert rays(C.byref(d), ls.ctypes.data, C.byref(ref_cam), C.byref(vl.lens(aperture=0.0))) == _abi.RT_OK
    assert rays(C.byref(d), ls.ctypes.data, C.byref(cam), C.byref(vl.lens(coc_tol=vl.INF, spread=16))) == _abi.RT_OK and nd.value == 8


def test_the_ray_limit_counts_four_tuple_planes():
    """4096 x 4096 pixels: one pixel offset nine times is one plane for rt_view_create; with 8 distinct lens offsets it is 2^27
    rays, allowed; with 9 it is refused"""
    lib = _lib.load()
    cam = vc.pinhole(4096, 4096).view_camera()
    out, nd = C.c_void_p(), C.c_uint32()
    for n, allowed in ((8, True), (9, False)):
        d, keep = vc.desc(4096, 4096, np.zeros((n, 2), F32))
        assert lib.rt_view_rays_model(C.byref(d), C.byref(cam), None, None, None, C.byref(nd)) == _abi.RT_OK and nd.value == 1
        ls = camera.lens_samples(n)
        rc = lib.rt_view_lens_rays_model(C.byref(d), ls.ctypes.data, C.byref(cam), C.byref(vl.lens()), None, None, None, C.byref(nd))
        if allowed:
            assert rc == _abi.RT_OK and nd.value == 8
        else:
            _refused(rc, "exceed the 2^27 rays")
            _refused(lib.rt_view_create_lens(C.byref(d), ls.ctypes.data, 0, C.byref(out)), "exceed the 2^27 rays")


def test_abi_struct_matches_the_header(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(rt_view_lens),'
                    " offsetof(rt_view_lens, spread), offsetof(rt_view_lens, aperture), offsetof(rt_view_lens, focus_distance),"
                    " offsetof(rt_view_lens, coc_tol), offsetof(rt_view_lens, reserved)); return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    L = _abi.rt_view_lens
    assert got == [C.sizeof(L), L.spread.offset, L.aperture.offset, L.focus_distance.offset, L.coc_tol.offset, L.reserved.offset] == [24, 4, 8, 12, 16, 20]
