"""Adaptive camera views without a device: the host models of the refine rule and the adaptive resolve (compiled from
csrc/rt_view_adapt.h, the source of the kernels) against numpy restatements, bit for bit; the tolerances the GPU tests use; the
stable partition's host model and the workspace layout, printed by a small stand-alone program; and every refusal that needs
no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, _abi, _lib

import trace_rays_cases as tr
import view_adapt_cases as va
import view_cases as vc
from test_scene_pack_host import CSRC, HIPCC, ROOT

CRITERIA = (va.ID, va.DEPTH, va.COLOUR, va.ID | va.DEPTH | va.COLOUR, va.EVERY, va.EVERY | va.ID, 0)
_plane0 = {}


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return tr.build_ref(tmp_path_factory.mktemp("adaptref"))


def plane0_of(ref, features, kw, what):
    """the CPU reference's trace of sample 0 of every pixel (ray p keeps light-cloud key p), computed once per (shading, view)"""
    key = (tuple(features), what)
    if key not in _plane0:
        label, w, h, smp, cam = next(v for v in va.views() if v[0] == what)
        o, d, _, _ = vc.model_rays(w, h, smp, cam)
        n = w * h
        rays = tr.ref_trace(ref, va.scene_flat(), RenderConfig.from_features(features, **kw), o[:n], d[:n], index=np.arange(n, dtype=np.uint32))
        _plane0[key] = (w, h, {k: rays[k] for k in ("rgb", "valid", "id", "t")})
    return _plane0[key]


WHATS = [v[0] for v in va.views()]


# ---- the refine rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", WHATS)
def test_refine_model_equals_the_numpy_rule_on_the_reference_trace(ref, what):
    """every criterion alone, all three, EVERY, none; the tests' tolerances and a tolerance of 0"""
    w, h, rays = plane0_of(ref, [], {}, what)
    for crit in CRITERIA:
        for ct, dt in ((va.COLOUR_TOL, va.DEPTH_TOL), (0.0, 0.0), (0.01, 0.5)):
            rf = va.refine(crit, ct, dt)
            got, n = va.refine_model(w, h, rf, rays)
            want = va.refine_numpy(w, h, rf, rays)
            print(f"{what} criteria {crit} tol ({ct}, {dt}): {n} of {w * h} refined; differing {int((got != want).sum())}")
            assert np.array_equal(got, want) and n == int(want.sum())
            if crit & va.EVERY:
                assert got.all()
            if crit == 0:
                assert not got.any()


def synthetic(w, h, seed):
    """planes with flat regions, hit/miss borders, equal neighbours and steps of every size around the tolerances"""
    rng = np.random.default_rng(seed)
    n = w * h
    valid = rng.uniform(size=n) < 0.7
    t = np.where(valid, rng.choice(np.float32([1.0, 1.0, 1.05, 1.1250001, 1.125, 2.0, 1e-30, 3e38]), n), np.float32(np.inf)).astype(np.float32)
    rgb = rng.choice(np.float32([0.0, 0.5, 0.5, 0.625, 0.62500006, 0.51, 1.5]), (n, 3)).astype(np.float32)
    rgb[~valid] = 0.0
    ids = np.where(valid, rng.integers(0, 3, n), -1).astype(np.int32)
    return dict(rgb=rgb, valid=valid, id=ids, t=t)


@pytest.mark.parametrize("size", [(37, 29), (64, 4), (1, 1), (1, 9), (9, 1), (2, 2), (3, 1)])
def test_refine_model_equals_the_numpy_rule_on_synthetic_planes(size):
    """frames one pixel wide or high (no neighbour on two sides) among them; a NaN colour and a NaN t refine the pixel and all
    its valid neighbours under their criterion and nothing under the others"""
    w, h = size
    for seed in range(3):
        rays = synthetic(w, h, seed)
        for crit in CRITERIA:
            for ct, dt in ((0.125, 0.125), (0.0, 0.0)):
                rf = va.refine(crit, ct, dt)
                got, n = va.refine_model(w, h, rf, rays)
                assert np.array_equal(got, va.refine_numpy(w, h, rf, rays)), (size, seed, crit, ct, dt)
                assert n == int(got.sum())


def test_a_nan_refines():
    w, h = 5, 5
    centre = 2 * w + 2
    ring = [y * w + x for y in (1, 2, 3) for x in (1, 2, 3)]
    for crit, plane, nan_refines in ((va.COLOUR, "rgb", True), (va.DEPTH, "t", True), (va.COLOUR, "t", False), (va.DEPTH, "rgb", False),
                                     (va.ID, "t", False)):
        rays = dict(rgb=np.full((w * h, 3), 0.5, np.float32), valid=np.ones(w * h, bool), id=np.zeros(w * h, np.int32), t=np.ones(w * h, np.float32))
        if plane == "rgb":
            rays["rgb"][centre, 1] = np.nan
        else:
            rays["t"][centre] = np.nan
        got, n = va.refine_model(w, h, va.refine(crit, 10.0, 10.0), rays)
        want = np.zeros(w * h, bool)
        if nan_refines:
            want[ring] = True
        assert np.array_equal(got, want), (crit, plane)
        assert np.array_equal(got, va.refine_numpy(w, h, va.refine(crit, 10.0, 10.0), rays))


def test_hit_miss_borders_refine_on_both_sides_and_a_tolerance_of_zero_keeps_equal_neighbours():
    w, h = 6, 4
    valid = np.zeros((h, w), bool)
    valid[:, 3:] = True  # columns 0..2 miss, 3..5 hit: columns 2 and 3 refine
    rays = dict(rgb=np.where(valid.ravel()[:, None], np.full((w * h, 3), 0.25, np.float32), np.float32(0)).astype(np.float32), valid=valid.ravel(),
                id=np.where(valid.ravel(), 4, -1).astype(np.int32), t=np.where(valid.ravel(), np.float32(2), np.float32(np.inf)).astype(np.float32))
    want = np.zeros((h, w), bool)
    want[:, 2:4] = True
    for crit in (va.ID, va.DEPTH, va.COLOUR):
        got, _ = va.refine_model(w, h, va.refine(crit, 0.0, 0.0), rays)
        assert np.array_equal(got, want.ravel()), crit
    # the smallest step above zero refines under a tolerance of zero
    rays["t"][3] = np.nextafter(np.float32(2), np.float32(3))
    got, _ = va.refine_model(w, h, va.refine(va.DEPTH, 0.0, 0.0), rays)
    want[0:2, 3:5] = True
    assert np.array_equal(got, want.ravel())


@pytest.mark.parametrize("features,kw,what", [(f, kw, w) for f, kw in va.SHADINGS for w in WHATS] + [va.REALISTIC + (w,) for w in va.REALISTIC_VIEWS])
def test_the_gpu_tolerances_refine_some_pixels_and_not_all(ref, features, kw, what):
    """a mask that is empty or full proves nothing: between 5 % and 95 % of the pixels on every (shading, view) of the GPU tests"""
    w, h, rays = plane0_of(ref, features, kw, what)
    got, n = va.refine_model(w, h, va.refine(), rays)
    print(f"{features} {what}: {n} of {w * h} refined = {n / (w * h):.3f}")
    assert 0.05 <= n / (w * h) <= 0.95


# ---- the adaptive resolve -------------------------------------------------------------------------------------------------------
def random_rays(n_pix, nd, seed=3):
    rng = np.random.default_rng(seed)
    rays = dict(rgb=rng.uniform(0, 2, (nd * n_pix, 3)).astype(np.float32), valid=rng.uniform(size=nd * n_pix) < 0.8,
                id=rng.integers(-1, 9, nd * n_pix).astype(np.int32), t=rng.uniform(1, 2, nd * n_pix).astype(np.float32))
    rays["valid"][1::n_pix] = False  # pixel 1: nothing valid
    rays["rgb"][~rays["valid"]] = 0.0
    return rays


@pytest.mark.parametrize("table", ["centre1", "distinct7", "repeats9", "config16", "repeats24"])
def test_adaptive_resolve_with_a_full_and_an_empty_mask(table):
    """all ones: rt_view_resolve_model; all zeros: rt_view_resolve_model with plane_of zeroed (n_samples and scale unchanged, so
    the reference's 1 / (8 ceil(n / 8)) for 7, 9 and 24 samples); a mixed mask: the one or the other per pixel.  The per-ray
    plane 0 handed to the adaptive model is poisoned: it must not be read."""
    smp = vc.sample_tables(_abi.RT_VIEW_PINHOLE)[table]
    plane_of, nd = vc.brute_dedup(smp)
    n_pix, n = 13, smp.shape[0]
    rays = random_rays(n_pix, nd)
    full = vc.resolve_model(n_pix, n, plane_of, rays)
    flat = vc.resolve_model(n_pix, n, np.zeros_like(plane_of), {k: v[:n_pix] for k, v in rays.items()})
    base = {k: v[:n_pix].copy() for k, v in rays.items()}
    poisoned = {k: v.copy() for k, v in rays.items()}
    poisoned["rgb"][:n_pix], poisoned["valid"][:n_pix] = np.nan, True
    mixed = np.arange(n_pix) % 3 == 0
    for mask, want in ((np.ones(n_pix, bool), full), (np.zeros(n_pix, bool), flat), (mixed, va.where_pixels(mixed, full, flat))):
        got = va.resolve_adaptive_model(n_pix, n, plane_of, mask, base, poisoned if nd > 1 else None)
        vc.assert_pixels_equal(got, want, f"{table} mask {int(mask.sum())}/{n_pix}")
        assert np.array_equal(got["argb"], want["argb"])
    assert np.all(full["argb"][~full["valid"]] == vc.FILL)
    if n > 1:
        # a pixel whose samples all agree: the flat rule gives what the full resolve gives
        same = {k: np.tile(v[:n_pix], (nd,) + (1,) * (v.ndim - 1)) for k, v in rays.items()}
        assert np.array_equal(vc.bits(vc.resolve_model(n_pix, n, plane_of, same)["rgb"]), vc.bits(flat["rgb"]))


# ---- the partition and the workspace ----------------------------------------------------------------------------------------------
PROGRAM = r'''
#include <cstdio>
#include <vector>
#include "rt_host.h"
#include "rt_view_adapt.h"
int main() {
  const size_t shapes[][2] = {%(shapes)s};
  for (const auto& s : shapes) {
    RtArena lay;
    RtViewAdaptWs ws{};
    rt_view_adapt_ws_add(lay, s[0], s[1], RT_ORDER_SCAN_BLOCKS, &ws);
    std::vector<char> mem(lay.total());
    lay.bind(mem.data());
    printf("layout");
    for (const void* p : {(const void*)ws.rgb0, (const void*)ws.id0, (const void*)ws.t0, (const void*)ws.valid0, (const void*)ws.mask, (const void*)ws.perm2,
                          (const void*)ws.order0, (const void*)ws.flags, (const void*)ws.counts, (const void*)ws.sums, (const void*)ws.n_refined})
      printf(" %%td", (const char*)p - mem.data());
    printf(" %%zu %%zu\n", lay.total(), rt_partition_counts(s[1]));
  }
  const std::vector<std::vector<uint32_t>> perms = {%(perms)s};
  const std::vector<std::vector<uint8_t>> flags = {%(flags)s};
  const uint32_t n_outs[] = {%(n_outs)s};
  for (size_t c = 0; c < flags.size(); c++) {
    const uint32_t n = (uint32_t)flags[c].size();
    std::vector<uint32_t> out(n_outs[c], 0xFFFFFFFFu);
    const uint32_t n_set = rt_partition_model(perms[c].empty() ? nullptr : perms[c].data(), flags[c].data(), n, n_outs[c], out.data());
    printf("partition %%u", n_set);
    for (uint32_t v : out) printf(" %%u", v);
    printf("\n");
  }
  return 0;
}
'''
SHAPES = ((1, 1), (37 * 29, 7 * 37 * 29), (256, 20 * 256), (1 << 20, 9 << 20))


def partition_cases():
    """(perm or None, flags, n_out): all set, none set, one set, a length that is no multiple of 256, a truncated output"""
    rng = np.random.default_rng(11)
    cases = [(None, np.ones(5, bool), 5), (None, np.zeros(5, bool), 5), (None, np.arange(7) == 4, 7)]
    for n in (300, 513):
        cases.append((rng.permutation(n).astype(np.uint32), rng.uniform(size=n) < 0.4, n))
        cases.append((rng.permutation(n).astype(np.uint32), rng.uniform(size=n) < 0.4, n // 3))
    return cases


@pytest.fixture(scope="module")
def program_lines(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("adapt_layout")
    src, exe = d / "layout.cpp", d / "layout"
    cases = partition_cases()
    braces = lambda rows: ", ".join("{" + ", ".join(str(int(x)) for x in r) + "}" for r in rows)  # noqa: E731
    src.write_text(PROGRAM % {"shapes": ", ".join(f"{{(size_t){a}, (size_t){b}}}" for a, b in SHAPES),
                              "perms": braces([[] if p is None else p for p, _, _ in cases]), "flags": braces([f for _, f, _ in cases]),
                              "n_outs": ", ".join(str(k) for _, _, k in cases)})
    out = subprocess.run([HIPCC, "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", "-x", "hip", "--cuda-host-only", "-I", CSRC, "-I",
                          os.path.join(ROOT, "include"), "-o", str(exe), str(src)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr[-3000:]
    rows = [l.split() for l in run.stdout.splitlines()]
    return [[int(x) for x in r[1:]] for r in rows if r[0] == "layout"], [[int(x) for x in r[1:]] for r in rows if r[0] == "partition"]


def test_workspace_layout(program_lines):
    """base planes of 12 + 4 + 4 + 1 bytes per pixel, the mask, 4 bytes per ray of second permutation, 4 per pixel of plane-0
    order, a flag byte per ray, one count per 256 rays and one for the total rounded up to 8, the scan's block sums, one word"""
    layouts, _ = program_lines
    from test_host_layout import RT_ORDER_SCAN_BLOCKS, laid_out

    for (n_pix, n_rays), row in zip(SHAPES, layouts):
        counts = ((n_rays + 255) // 256 + 1 + 7) // 8 * 8
        offsets, total = laid_out([12 * n_pix, 4 * n_pix, 4 * n_pix, n_pix, n_pix, 4 * n_rays, 4 * n_pix, n_rays, 4 * counts, 4 * RT_ORDER_SCAN_BLOCKS, 4])
        assert row == offsets + [total, counts], (n_pix, n_rays)
        assert counts % 8 == 0 and counts > (n_rays + 255) // 256 and counts <= RT_ORDER_SCAN_BLOCKS * 2048


def test_partition_model_equals_the_numpy_partition(program_lines):
    _, parts = program_lines
    cases = partition_cases()
    assert len(parts) == len(cases)
    for (perm, flags, n_out), row in zip(cases, parts):
        want = va.partition_numpy(perm, flags, n_out)
        assert row[0] == int(np.asarray(flags).sum())
        assert np.array_equal(np.array(row[1:], np.uint32), want)


def test_numpy_partition_is_a_stable_permutation():
    """set entries first, each group in the order it had; the liveness predicate of pass 2 puts exactly the refined pixels' rays
    of planes 1.. in front; the plane-0 predicate puts a permutation of the first n_pixels rays in front"""
    rng = np.random.default_rng(2)
    n_pix, nd = 50, 4
    n = n_pix * nd
    perm = rng.permutation(n).astype(np.uint32)
    mask = rng.uniform(size=n_pix) < 0.3
    flags = va.live_flags_numpy(perm, n_pix, mask)
    out = va.partition_numpy(perm, flags)
    n_live = int(mask.sum()) * (nd - 1)
    assert int(flags.sum()) == n_live and np.array_equal(np.sort(out), np.arange(n))
    where = np.empty(n, np.int64)
    where[perm] = np.arange(n)
    for part in (out[:n_live], out[n_live:]):
        assert np.all(np.diff(where[part]) > 0)  # each side keeps the order of `perm`
    assert np.all((out[:n_live] >= n_pix) & mask[out[:n_live] % n_pix])
    p0 = va.partition_numpy(perm, perm < n_pix, n_pix)
    assert np.array_equal(np.sort(p0), np.arange(n_pix)) and np.all(np.diff(where[p0]) > 0)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _refused(rc, part):
    msg = _lib.load().rt_last_error().decode()
    assert rc == _abi.RT_ERR_INVALID_ARG and part in msg, (rc, msg)


def test_adaptive_calls_are_refused_before_any_device_is_touched():
    """NULL pointers, a wrong version, unknown criteria bits, a negative or NaN tolerance, and what rt_render_view refuses --
    before the scene or the view is looked at.  (A view without rt_view_enable_adaptive needs a view: test_view_adaptive_gpu.py.)"""
    lib = _lib.load()
    fake = C.c_void_p(0x1000)  # never dereferenced: every check below comes first
    p, keep = _abi.make_params(RenderConfig.from_features([]))
    planes = np.zeros(4, np.float32)
    out = _abi.rt_ray_radiance(planes.ctypes.data, None, None, None, None)
    ok = _abi.rt_ray_radiance(planes.ctypes.data, planes.ctypes.data, planes.ctypes.data, planes.ctypes.data, None)
    st = _abi.rt_stats()
    good = va.refine()
    calls = {"rt_render_view_adaptive_device": lambda s, v, pp, rf, o: lib.rt_render_view_adaptive_device(s, v, pp, rf, o, None, None),
             "rt_render_view_adaptive": lambda s, v, pp, rf, o: lib.rt_render_view_adaptive(s, v, pp, rf, o, None, C.byref(st)),
             "rt_view_refine_model": lambda s, v, pp, rf, o: lib.rt_view_refine_model(2, 2, rf, C.byref(ok), None, None)}
    for name, call in calls.items():
        model = name == "rt_view_refine_model"
        _refused(call(fake, fake, C.byref(p), None, C.byref(out)), "null refine")
        bad = va.refine()
        bad.abi_version = 2
        _refused(call(fake, fake, C.byref(p), C.byref(bad), C.byref(out)), "rt_view_refine.abi_version")
        _refused(call(fake, fake, C.byref(p), C.byref(va.refine(criteria=16)), C.byref(out)), "unknown criteria bits")
        _refused(call(fake, fake, C.byref(p), C.byref(va.refine(criteria=va.ID | 0x100)), C.byref(out)), "unknown criteria bits")
        for tol in (-1e-9, float("nan"), -float("inf")):
            _refused(call(fake, fake, C.byref(p), C.byref(va.refine(colour_tol=tol)), C.byref(out)), "colour_tol")
            _refused(call(fake, fake, C.byref(p), C.byref(va.refine(depth_tol=tol)), C.byref(out)), "depth_tol")
        assert name in lib.rt_last_error().decode()
        if model:
            continue
        _refused(call(None, fake, C.byref(p), C.byref(good), C.byref(out)), "null scene")
        _refused(call(fake, None, C.byref(p), C.byref(good), C.byref(out)), "null view")
        _refused(call(fake, fake, None, C.byref(good), C.byref(out)), "null shading")
        _refused(call(fake, fake, C.byref(p), C.byref(good), None), "null output")
        _refused(call(fake, fake, C.byref(p), C.byref(good), C.byref(_abi.rt_ray_radiance())), "every output plane is NULL")
        aa, keep3 = _abi.make_params(RenderConfig.from_features(["anti_aliasing"]))
        _refused(call(fake, fake, C.byref(aa), C.byref(good), C.byref(out)), "RT_FLAG_ANTI_ALIASING")
        deep, keep5 = _abi.make_params(RenderConfig.from_features(["realistic"]))
        deep.max_depth_reflection = deep.max_depth_refraction = 0
        _refused(call(fake, fake, C.byref(deep), C.byref(good), C.byref(out)), "depth 0")
    _refused(lib.rt_view_enable_adaptive(None), "null view")
    _refused(lib.rt_view_adaptive_read(None, None), "null view")
    _refused(lib.rt_view_adaptive_read(fake, None), "null info")
    # the models
    _refused(lib.rt_view_refine_model(0, 2, C.byref(good), C.byref(ok), None, None), "a frame of")
    _refused(lib.rt_view_refine_model(2, 2, C.byref(good), C.byref(out), None, None), "all required")
    _refused(lib.rt_view_refine_model(2, 2, C.byref(good), None, None, None), "all required")
    assert lib.rt_view_refine_model(2, 2, C.byref(va.refine(colour_tol=float("inf"), depth_tol=0.0)), C.byref(ok), None, None) == _abi.RT_OK
    po = np.zeros(2, np.uint8)
    m = np.zeros(4, np.uint8)
    _refused(lib.rt_view_resolve_adaptive_model(1, 0, po.ctypes.data, m.ctypes.data, C.byref(ok), None, C.byref(ok)), "n_samples")
    _refused(lib.rt_view_resolve_adaptive_model(1, 65, po.ctypes.data, m.ctypes.data, C.byref(ok), None, C.byref(ok)), "n_samples")
    _refused(lib.rt_view_resolve_adaptive_model(1, 1, po.ctypes.data, None, C.byref(ok), None, C.byref(ok)), "null")
    _refused(lib.rt_view_resolve_adaptive_model(1, 1, po.ctypes.data, m.ctypes.data, C.byref(out), None, C.byref(ok)), "all required")
    po[1] = 1
    _refused(lib.rt_view_resolve_adaptive_model(1, 2, po.ctypes.data, m.ctypes.data, C.byref(ok), None, C.byref(ok)), "per-ray rgb and valid")
    po[1] = 2
    _refused(lib.rt_view_resolve_adaptive_model(1, 2, po.ctypes.data, m.ctypes.data, C.byref(ok), C.byref(ok), C.byref(ok)), "first-occurrence")


def test_python_refine_defaults_and_criteria_names():
    from hslu_i.ba_raytracing.f2501_raytracer_amd import Refine

    s = Refine().struct()
    assert s.criteria == va.DEPTH | va.COLOUR and s.abi_version == _abi.RT_ABI_VERSION
    assert Refine(criteria="id").struct().criteria == va.ID and Refine(criteria=("every", "colour")).struct().criteria == va.EVERY | va.COLOUR
    assert Refine(criteria=0).struct().criteria == 0
    with pytest.raises(ValueError):
        Refine(criteria="edges").struct()


def test_abi_structs_match_the_header(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(rt_view_refine),'
                    " sizeof(rt_view_adaptive_info), offsetof(rt_view_adaptive_info, bytes), offsetof(rt_view_adaptive_info, pass1_ms),"
                    " offsetof(rt_view_refine, depth_tol)); return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_abi.rt_view_refine), C.sizeof(_abi.rt_view_adaptive_info), _abi.rt_view_adaptive_info.bytes.offset,
                   _abi.rt_view_adaptive_info.pass1_ms.offset, _abi.rt_view_refine.depth_tol.offset]
