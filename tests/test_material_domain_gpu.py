"""The GPU across the material domain: the variants of material_cases.py against the float64 model (the intervals, guards and
counters test_material_domain.py holds the oracle to) in the forms of test_f64_model_gpu.FORMS, against the oracle (hit ids
equal, t bit-equal, the same pixels written, |dRGB| <= 1e-4) and form against form bit for bit; stacks of panes through
rt_any_intersection and rt_trace_rays, up to the capacity of the fixed-point filter sums."""
import numpy as np
import pytest

import f64_query_cases as qc
import material_cases as mc
import oracle_lib
from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceScene
from test_f64_model_gpu import FORMS
from test_parity_gpu import RGB_TOL, gpu_render

pytestmark = pytest.mark.gpu

FEATURE_SETS = ["c1", "c3", "c4d3"]
VARIANTS = sorted(mc.VARIANTS)


def _fields(r):
    return {k: np.asarray(getattr(r, k)) for k in r._fields}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("fs", FEATURE_SETS)
def test_gpu_frame_within_the_float64_intervals_and_the_oracle(fs, variant):
    cfg, flat = mc.workload(fs, variant)
    argb_o, po, so = oracle_lib.render(flat, cfg)
    hit = po["hit_id"] >= 0
    first = None
    for form in ["fused", "split"] + (["chained"] if fs == "c4d3" else []):
        argb, planes, st = gpu_render(cfg, flat, None, **FORMS[form])
        name = f"gpu {fs} {variant} {form}"
        s = mc.check_frame(name, fs, variant, planes, st)
        if variant == "zero_filter":
            assert np.isfinite(planes["rgb"]).all() and np.isfinite(planes["hit_t"]).all(), name
        # against the oracle, every pixel
        assert np.array_equal(planes["hit_id"], po["hit_id"]), name
        assert np.array_equal(_bits(planes["hit_t"][hit]), _bits(po["hit_t"][hit])), name
        assert np.array_equal(argb != 0, argb_o != 0) and st["pixels_written"] == so["pixels_written"], name
        d = float(np.abs(planes["rgb"].astype(np.float64) - po["rgb"]).max())
        print(f"{name}: max |dRGB| vs the oracle {d:.3e}, worst excess over the model's interval {s['worst']:.2e}")
        assert d <= RGB_TOL, (name, d)  # (NaN fails)
        # between the forms, as test_phases_gpu.py holds them: with secondary rays every share reaches the pixel as the same
        # fixed-point term, so the frames are the same bits; without, the fused kernel sums floats over all lights and the
        # split form per light: fp32 reassociation, 2e-6 at values up to 1 and in proportion above (`shiny` reaches 2.5)
        if first is None:
            first = argb, planes
            continue
        assert np.array_equal(_bits(planes["hit_t"]), _bits(first[1]["hit_t"])), name
        if fs == "c4d3":
            assert np.array_equal(argb, first[0]) and np.array_equal(_bits(planes["rgb"]), _bits(first[1]["rgb"])), name
        else:
            df = float(np.abs(planes["rgb"] - first[1]["rgb"]).max())
            print(f"{name}: max |dRGB| vs fused {df:.3e}")
            assert df <= 2e-6 * max(1.0, float(first[1]["rgb"].max())), (name, df)
            for sh in (16, 8, 0):
                assert np.abs(((argb >> sh) & 0xFF).astype(np.int32) - ((first[0] >> sh) & 0xFF).astype(np.int32)).max() <= 1, name


STACKS = {
    "white1": (1, mc.WHITE, 0.5), "white2": (2, mc.WHITE, 0.5), "white3": (3, mc.WHITE, 0.5), "white4": (4, mc.WHITE, 0.5),
    "coloured4": (4, mc.COLOURED, 0.5), "tiny1": (1, mc.WHITE, mc.TINY_OPACITY), "capacity": (mc.CAPACITY_K, mc.WHITE, mc.CAPACITY_OPACITY),
}


@pytest.mark.parametrize("name", sorted(STACKS))
def test_gpu_chain_through_a_stack_of_panes(name):
    """rt_any_intersection reports the chain, not the shading: filter and opacity as they sum, below 0 included.  A batch of
    65 copies of the ray: a full wavefront and a ragged one give the same row."""
    k, colour, opacity = STACKS[name]
    flat = mc.pane_stack(k, colour, opacity)
    o, d = mc.pane_rays(65)
    res = qc.model_answers("any", flat, qc.query_config(), o[:1], d[:1]) * 65
    ds = DeviceScene(flat, 0)
    got = _fields(ds.any_intersection(o, d))
    ds.close()
    s = qc.check_any(res, got)
    print(f"{name}: model opacity {res[0]['op']}, filter {res[0]['filt'][0]}; gpu {got['combined_opacity'][0]}, {got['color_filter'][0]}, "
          f"worst excess {s['worst']:.2e}")
    assert s["ambiguous"] == 0 and not s["bad"], s
    assert (res[0]["has"], res[0]["occluded"]) == (True, False)
    for f in ("combined_opacity", "color_filter"):
        assert (_bits(got[f]) == _bits(got[f][:1])).all(), f
    if name == "tiny1":
        mc.assert_tiny_opacity(res[0], got)
    if name == "capacity":
        # the integer sum is exact: k times the one absorption in 2^-24 units, converted to float once
        one = np.float32(1.0) - np.float32(opacity)  # white: absorption = 1 - opacity, a multiple of 2^-24
        units = k * int(np.float64(one) * 2.0 ** 24)
        assert units < 2 ** 32 and float(one) * 2.0 ** 24 == int(np.float64(one) * 2.0 ** 24)
        want = np.float32(1.0) - np.float32(units) * np.float32(2.0 ** -24)
        assert np.all(got["color_filter"][0] == want), (got["color_filter"][0], want)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_gpu_radiance_on_a_wall_lit_through_a_stack(k):
    flat = mc.pane_stack(k, wall=True)
    dark = mc.pane_stack(k, wall=True)
    dark.lights[0, 6] = 0.0
    o, d = mc.wall_rays()
    tcfg = qc.trace_config("plain", False)
    ds, dd = DeviceScene(flat, 0), DeviceScene(dark, 0)
    got, unlit = _fields(ds.trace_rays(o, d, tcfg)), _fields(dd.trace_rays(o, d, tcfg))
    ds.close(), dd.close()
    s = qc.check_trace(flat, qc.model_answers("trace", flat, tcfg, o, d), o, d, got)
    print(f"wall behind {k} panes: rgb {got['rgb'].tolist()}, worst excess {s['worst']:.2e}, ambiguous {s['ambiguous']}")
    assert s["ambiguous"] == 0 and s["hits"] == o.shape[0] and not s["bad"], s
    assert np.isfinite(got["rgb"]).all()
    if k >= 2:  # nothing of the light in front of the stack arrives: the wall is lit as it is without that light
        assert np.array_equal(unlit["rgb"], got["rgb"])
    else:
        assert np.abs(unlit["rgb"] - got["rgb"]).max() > 1e-3
