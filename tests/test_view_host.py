"""Camera views without a device: the host models of the ray generator and the sample resolve (compiled from csrc/rt_view.h,
the source of the kernels) against independent formulas -- PinholeCamera.direction in float64, the oracle's render_pixel
restated in numpy, a brute-force dedup, the oracle's own anti-aliased frame and its pixel pack -- and every refusal."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, _abi, _lib, camera, sampling, scenes

import oracle_lib
import trace_rays_cases as tr
import view_cases as vc

U = 2.0 ** -24  # the relative error of one fp32 rounding to nearest


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return tr.build_ref(tmp_path_factory.mktemp("viewref"))


# ---- rays -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", vc.FRAMES)
@pytest.mark.parametrize("table", ["centre1", "distinct7", "repeats9", "config16", "repeats24"])
def test_pinhole_rays_against_the_float64_camera(size, table):
    """The model's pinhole rays against PinholeCamera.direction (float64, the independent formula), per component.

    The bound counts the roundings of the formula as rt_view.h writes it.  With u = 2^-24, P = W + 1 >= |x + 0.5 + sx|,
    A = P / H * tan and B = (H + 1) / H * tan the largest |a| and |b|:
      a: x + 0.5 is exact; + sx rounds (u P); 2 * is exact (2 u P); - W rounds (3 u P in all); / H rounds (4 u P / H);
         * tan rounds, and tan itself is a rounded fp32 (6 u A).  b likewise: 6 u B.
      a * right[k]: the error of a (6 u A), of the fp32 basis component (u A) and of the product (u A): 8 u A; b * up[k]: 8 u B.
      forward[k] is a rounded fp32: u.  The two additions round sums of magnitude <= 1 + A + B: 2 u (1 + A + B).
    Sum: u (3 + 10 A + 10 B); second-order terms are covered by the factor 1 + 2^-10.  1 + A + B bounds the largest
    component, so the bound is below 10 u (1 + A + B) = 5 ulp at that magnitude.  Origins are the fp32 eye, exactly."""
    W, H = size
    cam = vc.pinhole(W, H)
    smp = vc.sample_tables(_abi.RT_VIEW_PINHOLE)[table]
    o, d, plane_of, nd = vc.model_rays(W, H, smp, cam.view_camera())
    firsts = [int(np.flatnonzero(plane_of == u)[0]) for u in range(nd)]
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    tan = np.tan(np.radians(cam.fov_y_deg) / 2.0)
    A, B = (W + 1) / H * tan, (H + 1) / H * tan
    bound = U * (3 + 10 * A + 10 * B) * (1 + 2.0 ** -10)
    worst = 0.0
    for u, k in enumerate(firsts):
        want = cam.direction(xs.ravel() + 0.5 + float(smp[k, 0]), ys.ravel() + 0.5 + float(smp[k, 1]))
        got = d[u * W * H:(u + 1) * W * H].astype(np.float64)
        worst = max(worst, float(np.abs(got - want).max()))
    print(f"{W}x{H} {table}: {nd} distinct of {smp.shape[0]}, max |d - d64| = {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound
    assert np.array_equal(vc.bits(o), vc.bits(np.broadcast_to(np.asarray(cam.eye, np.float32), o.shape)))


@pytest.mark.parametrize("size", vc.FRAMES)
def test_reference_rays_equal_the_render_camera(size):
    """offset (0, 0): camera.reference_rays, bit for bit; aa_offsets(cfg): the oracle's render_pixel (rt_oracle.c:517-533)
    restated in numpy float32 -- origin = coords + offset, direction = coords - focus without the offset."""
    W, H = size
    cfg = vc.frame_config(["anti_aliasing"], W, H)
    cam = camera.reference_view_camera(cfg)
    o, d, _, nd = vc.model_rays(W, H, np.zeros((1, 2), np.float32), cam)
    ro, rd = camera.reference_rays(cfg)
    assert nd == 1 and np.array_equal(vc.bits(o), vc.bits(ro)) and np.array_equal(vc.bits(d), vc.bits(rd))
    off = sampling.aa_offsets(cfg)
    o, d, plane_of, nd = vc.model_rays(W, H, off, cam)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    cx, cy = xs.ravel() * np.float32(cfg.fw), ys.ravel() * np.float32(cfg.fh)
    f = cfg.focus
    want_d = np.stack([cx - np.float32(f.x), cy - np.float32(f.y), np.float32(0.0) - np.full_like(cx, np.float32(f.z))], axis=1)
    for k in range(off.shape[0]):
        u = int(plane_of[k])
        want_o = np.stack([cx + off[k, 0], cy + off[k, 1], np.zeros_like(cx)], axis=1)
        sl = slice(u * W * H, (u + 1) * W * H)
        assert np.array_equal(vc.bits(o[sl]), vc.bits(want_o)), k
        assert np.array_equal(vc.bits(d[sl]), vc.bits(want_d)), k
    assert nd < off.shape[0], "the deterministic table repeats samples"


@pytest.mark.parametrize("kind", sorted(vc.KINDS))
def test_distinct_samples_against_a_brute_force_dedup(kind):
    cfg = RenderConfig.from_features(["anti_aliasing"])
    cam = vc.view_camera(vc.KINDS[kind], cfg, 5, 3)
    tables = vc.sample_tables(vc.KINDS[kind], cfg)
    tables["signed_zero"] = np.float32([[0.0, 0.0], [-0.0, 0.0], [0.0, 0.0], [0.0, -0.0], [-0.0, 0.0]])  # bits, not values
    for name, smp in tables.items():
        _, _, plane_of, nd = vc.model_rays(5, 3, smp, cam)
        want, want_nd = vc.brute_dedup(smp)
        print(kind, name, smp.shape[0], "samples,", nd, "distinct", plane_of.tolist())
        assert nd == want_nd and np.array_equal(plane_of, want), name
    assert vc.brute_dedup(tables["repeats9"])[0][8] == 0 and vc.brute_dedup(tables["config16"])[1] == 9


# ---- resolve ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("features,spheres_only", [(["anti_aliasing"], True), (["anti_aliasing", "realistic"], False),
                                                  (["anti_aliasing", "extreme_quality"], True)])
def test_resolve_model_is_the_oracles_accumulation(ref, features, spheres_only):
    """resolve(trace(model rays)) is the oracle's anti-aliased frame, bit for bit: both sides run the oracle's `trace` on the
    same rays (reference kind, light_mult == 1 -- `extreme_quality` is taken for its 24-sample table alone), so only the
    resolve is new: aux.rgb, hit_id, hit_t and the packed pixels.  Without its triangles the scene leaves pixels that no
    sample hits, and pixels at the spheres' rims that only some samples hit."""
    W, H = 37, 29
    feats = set(RenderConfig.from_features(features).features) - {"soft_shadows"}
    cfg = RenderConfig(features=frozenset(feats), width_override=W, height_override=H)
    assert cfg.point_light_multiplicator == 1
    flat = scenes.test_scene(cfg).flatten()
    if spheres_only:
        flat = flat.without_triangles()
    off = sampling.aa_offsets(cfg)
    o, d, plane_of, nd = vc.model_rays(W, H, off, camera.reference_view_camera(cfg))
    rays = tr.ref_trace(ref, flat, cfg, o, d, index=np.arange(o.shape[0], dtype=np.uint32))
    got = vc.resolve_model(W * H, off.shape[0], plane_of, rays, fill=0)
    argb, planes, _ = oracle_lib.render(flat, cfg)
    hit0, any_hit = planes["hit_id"] >= 0, got["valid"]
    print(f"{features}: {off.shape[0]} samples, {nd} distinct, {int(any_hit.sum())} of {W * H} pixels written, {int(hit0.sum())} hit by sample 0")
    some = rays["valid"].reshape(nd, W * H)
    print(f"pixels hit by some but not all distinct samples: {int((some.any(0) & ~some.all(0)).sum())}")
    assert any_hit.any() and (not spheres_only or ((~any_hit).any() and (some.any(0) & ~some.all(0)).any()))
    assert np.array_equal(got["id"], planes["hit_id"])
    assert np.array_equal(vc.bits(got["t"][hit0]), vc.bits(planes["hit_t"][hit0])) and np.all(np.isposinf(got["t"][~hit0]))
    assert np.array_equal(vc.bits(got["rgb"][any_hit]), vc.bits(planes["rgb"][any_hit])) and np.all(got["rgb"][~any_hit] == 0)
    assert np.array_equal(got["argb"], argb) and np.all(argb[~any_hit] == 0) and np.all(argb[any_hit] >> 24 == 0xFF)


@pytest.mark.parametrize("plane_of", [[0, 1, 2, 3, 4, 5, 6], [0, 1, 2, 3, 4, 5, 6, 7, 0], [0, 1, 0, 2, 3, 3, 4, 5, 6, 7, 8, 9, 1, 10, 11, 12, 13, 14, 15, 16, 17]],
                         ids=["7 in one packet", "9 with sample 0 repeated", "21 in three packets"])
def test_resolve_weights_repeats_and_ignores_invalid_samples(plane_of):
    """Hand-made cases against the accumulation written out in numpy float32: 7 samples (one packet with an empty lane: the
    weight is 1/8 and there is no `rest`), 9 samples (sample 8 repeats sample 0; 1/16) and 21 (a ragged third packet, repeats
    inside a packet and across packets; 1/24) -- each with one sample of pixel 0 invalid and a pixel without any valid
    sample; and one sample, which is taken unscaled."""
    rng = np.random.default_rng(3)
    plane_of = np.array(plane_of, np.uint8)
    n_pix, n, nd = 3, plane_of.shape[0], int(plane_of.max()) + 1
    rays = dict(rgb=rng.uniform(0, 2, (nd * n_pix, 3)).astype(np.float32), valid=np.ones(nd * n_pix, bool),
                id=np.arange(nd * n_pix, dtype=np.int32), t=rng.uniform(1, 2, nd * n_pix).astype(np.float32))
    rays["valid"][3 * n_pix + 0] = False          # distinct sample 3 of pixel 0
    rays["valid"][1::n_pix] = False               # pixel 1: nothing valid
    rays["rgb"][~rays["valid"]] = 0.0
    rays["id"][~rays["valid"]], rays["t"][~rays["valid"]] = -1, np.inf
    got = vc.resolve_model(n_pix, n, plane_of, rays)
    scale = np.float32(1.0) / np.float32(8 * ((n + 7) // 8))
    for p in range(n_pix):
        first, rest = np.zeros((8, 3), np.float32), np.zeros((8, 3), np.float32)
        for k in range(n):
            i = int(plane_of[k]) * n_pix + p
            if rays["valid"][i]:
                cs = rays["rgb"][i] * scale
                if k < 8:
                    first[k] = cs
                else:
                    rest[k & 7] = cs + rest[k & 7]
        lane = rest + first
        want = ((lane[0] + lane[4]) + (lane[2] + lane[6])) + ((lane[1] + lane[5]) + (lane[3] + lane[7]))
        if p == 1:
            assert not got["valid"][p] and np.all(got["rgb"][p] == 0) and got["argb"][p] == vc.FILL and got["id"][p] == -1 and np.isposinf(got["t"][p])
        else:
            assert got["valid"][p] and np.array_equal(vc.bits(got["rgb"][p]), vc.bits(want)), p
            assert got["id"][p] == rays["id"][p] and got["t"][p] == rays["t"][p] and got["argb"][p] >> 24 == 0xFF
    one = {k: v[:n_pix] for k, v in rays.items()}
    got = vc.resolve_model(n_pix, 1, plane_of[:1], one)
    assert np.array_equal(vc.bits(got["rgb"]), vc.bits(one["rgb"])) and np.array_equal(got["valid"], one["valid"])
    assert np.all(got["argb"][~one["valid"]] == vc.FILL) and np.all(got["argb"][one["valid"]] >> 24 == 0xFF)


def test_pack_against_the_oracle(oracle):
    """clamp, x 255, round half to even, NaN -> 0: edge values and the ties at (k + 0.5) / 255"""
    ties = [(k + 0.5) / 255.0 for k in range(0, 255, 7)]
    vals = np.float32([np.nan, -np.nan, -1.0, -0.0, 0.0, 1e-9, 0.5, 1.0, 1.0000001, 2.0, np.inf, -np.inf, 0.999999, 254.5 / 255, 0.5 / 255] + ties)
    vals = np.concatenate([vals, np.nextafter(vals, np.float32(2)), np.nextafter(vals, np.float32(-2))]).astype(np.float32)
    rgb = np.stack([vals, np.roll(vals, 1), np.roll(vals, 5)], axis=1)
    n = rgb.shape[0]
    rays = dict(rgb=rgb, valid=np.ones(n, bool), id=np.zeros(n, np.int32), t=np.ones(n, np.float32))
    got = vc.resolve_model(n, 1, np.zeros(1, np.uint8), rays)["argb"]
    want = np.array([oracle.rt_oracle_pack(float(r), float(g), float(b)) for r, g, b in rgb], np.uint32)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _refused(rc, part):
    msg = _lib.load().rt_last_error().decode()
    assert rc == _abi.RT_ERR_INVALID_ARG and part in msg, (rc, msg)


def test_view_descriptions_and_cameras_are_refused_before_any_device_is_touched():
    lib = _lib.load()
    cfg = RenderConfig.from_features([])
    good_cam = vc.pinhole(8, 8).view_camera()
    smp = np.zeros((2, 2), np.float32)
    smp[1] = 0.25
    h = C.c_void_p()

    def both(d, part, keep=None):
        """rt_view_create and the model refuse the same descriptions"""
        _refused(lib.rt_view_create(C.byref(d), 0, C.byref(h)), part)
        assert not h.value
        _refused(lib.rt_view_rays_model(C.byref(d), C.byref(good_cam), None, None, None, None), part)

    _refused(lib.rt_view_create(None, 0, C.byref(h)), "null")
    _refused(lib.rt_view_create(C.byref(vc.desc(8, 8, smp)[0]), 0, None), "null")
    d, keep = vc.desc(8, 8, smp)
    d.abi_version = 3
    both(d, "abi_version")
    both(vc.desc(0, 8, smp)[0], "empty frame")
    both(vc.desc(8, 0, smp)[0], "empty frame")
    d, keep = vc.desc(8, 8, smp)
    d.n_samples = 0
    both(d, "n_samples")
    big = np.zeros((65, 2), np.float32)
    both(vc.desc(8, 8, big)[0], "n_samples")
    d, keep = vc.desc(8, 8, smp)
    d.samples = None
    both(d, "null sample table")
    for bad in (np.nan, np.inf, -np.inf):
        s = smp.copy()
        s[1, 1] = bad
        both(vc.desc(8, 8, s)[0], "non-finite")
    both(vc.desc(8, 8, smp, order=3)[0], "order mode")
    both(vc.desc(1 << 14, 1 << 13, smp)[0], "2^27")            # 2 distinct samples x 2^27 pixels
    both(vc.desc(1 << 16, 1 << 16, smp[:1])[0], "2^27")        # the pixel count alone overflows 32 bits
    # exactly 2^27 rays pass the checks (the model with no output only validates)
    assert lib.rt_view_rays_model(C.byref(vc.desc(1 << 14, 1 << 12, smp)[0]), C.byref(good_cam), None, None, None, None) == _abi.RT_OK
    # a description that is fine reaches the device count: no device here, or a view is made
    rc = lib.rt_view_create(C.byref(vc.desc(8, 8, smp)[0]), 0, C.byref(h))
    if lib.rt_device_count() == 0:
        assert rc == _abi.RT_ERR_NO_DEVICE and not h.value
    else:
        assert rc == _abi.RT_OK
        lib.rt_view_destroy(h)

    d, keep = vc.desc(8, 8, smp)
    fake = C.c_void_p(0x1000)  # never dereferenced: every check below comes first

    def cam_refused(c, part):
        _refused(lib.rt_view_set_camera(fake, C.byref(c)), part)
        _refused(lib.rt_view_rays_model(C.byref(d), C.byref(c), None, None, None, None), part)

    _refused(lib.rt_view_set_camera(None, C.byref(good_cam)), "null view")
    _refused(lib.rt_view_set_camera(fake, None), "null camera")
    c = vc.pinhole(8, 8).view_camera()
    c.abi_version = 5
    cam_refused(c, "abi_version")
    c = vc.pinhole(8, 8).view_camera()
    c.kind = 2
    cam_refused(c, "camera kind")
    for kind in (_abi.RT_VIEW_PINHOLE, _abi.RT_VIEW_REFERENCE):
        for member in ("eye", "right", "up", "forward", "focus"):
            c = vc.view_camera(kind, cfg, 8, 8)
            getattr(c, member)[1] = float("nan")
            cam_refused(c, "not finite")
        for member in ("tan_half_fov_y", "fw", "fh"):
            c = vc.view_camera(kind, cfg, 8, 8)
            setattr(c, member, float("inf"))
            cam_refused(c, "not finite")
    for bad in (0.0, -0.5):
        c = vc.pinhole(8, 8).view_camera()
        c.tan_half_fov_y = bad
        cam_refused(c, "must be positive")
    assert lib.rt_view_rays_model(C.byref(d), C.byref(good_cam), None, None, None, None) == _abi.RT_OK
    lib.rt_view_destroy(None)  # a no-op


def test_renders_are_refused_before_any_device_is_touched():
    """NULL pointers, every output plane NULL and whatever rt_trace_rays refuses in `shading` -- checked before the scene or
    the view is looked at.  (A render before rt_view_set_camera and a view on another device need a view: test_view_gpu.py.)"""
    lib = _lib.load()
    fake = C.c_void_p(0x1000)
    p, keep = _abi.make_params(RenderConfig.from_features([]))
    planes = np.zeros(4, np.float32)
    out = _abi.rt_ray_radiance(planes.ctypes.data, None, None, None, None)
    st = _abi.rt_stats()
    calls = {"rt_render_view_device": lambda s, v, pp, o: lib.rt_render_view_device(s, v, pp, o, None),
             "rt_render_view": lambda s, v, pp, o: lib.rt_render_view(s, v, pp, o, C.byref(st))}
    for name, call in calls.items():
        _refused(call(None, fake, C.byref(p), C.byref(out)), "null scene")
        _refused(call(fake, None, C.byref(p), C.byref(out)), "null view")
        _refused(call(fake, fake, None, C.byref(out)), "null shading")
        _refused(call(fake, fake, C.byref(p), None), "null output")
        _refused(call(fake, fake, C.byref(p), C.byref(_abi.rt_ray_radiance())), "every output plane is NULL")
        bad, keep2 = _abi.make_params(RenderConfig.from_features([]))
        bad.abi_version = 1
        _refused(call(fake, fake, C.byref(bad), C.byref(out)), "rt_params.abi_version")
        aa, keep3 = _abi.make_params(RenderConfig.from_features(["anti_aliasing"]))
        _refused(call(fake, fake, C.byref(aa), C.byref(out)), "RT_FLAG_ANTI_ALIASING")
        assert name in lib.rt_last_error().decode()
        soft, keep4 = _abi.make_params(RenderConfig.from_features(["soft_shadows"], n_cloud_sets=8))
        soft.n_cloud_sets = 0
        assert call(fake, fake, C.byref(soft), C.byref(out)) == _abi.RT_ERR_INVALID_ARG
        deep, keep5 = _abi.make_params(RenderConfig.from_features(["realistic"]))
        deep.max_depth_reflection = deep.max_depth_refraction = 0
        _refused(call(fake, fake, C.byref(deep), C.byref(out)), "depth 0")
    for rc in (lib.rt_view_rays_device(None, fake, fake, None), lib.rt_view_rays(None, fake, fake), lib.rt_view_read(None, None, None)):
        _refused(rc, "null view")
    _refused(lib.rt_view_rays_device(fake, None, fake, None), "missing")
    _refused(lib.rt_view_rays(fake, fake, None), "missing")
    ok = _abi.rt_ray_radiance(planes.ctypes.data, planes.ctypes.data, planes.ctypes.data, planes.ctypes.data, None)
    po = np.zeros(2, np.uint8)
    _refused(lib.rt_view_resolve_model(1, 0, po.ctypes.data, C.byref(ok), C.byref(ok)), "n_samples")
    _refused(lib.rt_view_resolve_model(1, 65, po.ctypes.data, C.byref(ok), C.byref(ok)), "n_samples")
    _refused(lib.rt_view_resolve_model(1, 1, po.ctypes.data, C.byref(out), C.byref(ok)), "all required")
    _refused(lib.rt_view_resolve_model(1, 1, None, C.byref(ok), C.byref(ok)), "null")
    po[1] = 2
    _refused(lib.rt_view_resolve_model(1, 2, po.ctypes.data, C.byref(ok), C.byref(ok)), "first-occurrence")


# ---- the C example ------------------------------------------------------------------------------------------------------------
def build_example(out_dir):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    exe = os.path.join(str(out_dir), "c_view_example")
    subprocess.check_call(["gcc", "-Wall", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "c_view_example.c"),
                           "-L", lib_dir, "-lrt_hip", f"-Wl,-rpath,{lib_dir}", "-lm", "-o", exe])
    return exe


def test_view_example_links_against_the_abi(tmp_path):
    _lib.load()
    out = subprocess.run([build_example(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "9 samples, 8 distinct -> 153600 rays" in out.stdout
    assert "no HIP device" in out.stdout or "the frame equals the host models' frame" in out.stdout
