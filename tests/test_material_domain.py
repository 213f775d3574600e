"""The CPU oracle against the float64 model (tests/f64_model.py) across the material domain: the variants of
material_cases.py at four feature sets through f64_cases.check, stacks of panes through the oracle's ray-query wrappers, and
what the cases must be to say anything -- the variants change the picture, the zero-filter variant puts lattice pixels where
the reference's colour / filter * opacity was NaN (DESIGN D10), a model without the floor of the specular exponent rejects the
oracle.  test_material_domain_gpu.py holds the GPU to the same model and to this oracle."""
import numpy as np
import pytest

import f64_cases as fc
import f64_query_cases as qc
import material_cases as mc
import oracle_lib
import ray_query_cases as rq
import trace_rays_cases as tr

FEATURE_SETS = sorted(mc.FEATURE_SETS)
VARIANTS = sorted(mc.VARIANTS)


@pytest.fixture(scope="module")
def rq_ref(tmp_path_factory):
    return rq.build_ref(tmp_path_factory.mktemp("rqref"))


@pytest.fixture(scope="module")
def tr_ref(tmp_path_factory):
    return tr.build_ref(tmp_path_factory.mktemp("trref"))


def test_check_never_passes_a_non_finite_value():
    """NaN > TOL is false: a non-finite observed channel or model bound is `bad` by name"""
    one = dict(px=(0, 0), amb=None, id=0, t=1.0, written=True, lo=np.zeros(3), hi=np.zeros(3), nom=np.zeros(3), pen=False)
    ids, ts = np.zeros(1, np.int32), np.ones(1, np.float32)
    assert not fc.check([one], 1, np.zeros((1, 3), np.float32), ids, ts, t_rel=1e-5)["bad"]
    for v in (np.nan, np.inf, -np.inf):
        s = fc.check([one], 1, np.array([[0, v, 0]], np.float32), ids, ts, t_rel=1e-5)
        assert [b[1] for b in s["bad"]] == ["non-finite rgb"], s
        for k in ("lo", "hi"):
            s = fc.check([dict(one, **{k: np.array([0, 0, v])})], 1, np.zeros((1, 3), np.float32), ids, ts, t_rel=1e-5)
            assert [b[1] for b in s["bad"]] == ["non-finite model bound"], s
    s = fc.check([one], 1, np.zeros((1, 3), np.float32), ids, np.full(1, np.nan, np.float32), t_rel=1e-5)
    assert [b[1] for b in s["bad"]] == ["t"], s


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("fs", FEATURE_SETS)
def test_oracle_frame_within_the_float64_intervals(fs, variant):
    cfg, flat = mc.workload(fs, variant)
    argb, planes, st = oracle_lib.render(flat, cfg)
    mc.check_frame(f"oracle {fs} {variant}", fs, variant, planes, st)
    if variant == "zero_filter":
        assert np.isfinite(planes["rgb"]).all() and np.isfinite(planes["hit_t"]).all()


@pytest.mark.parametrize("fs", ["c2d3", "c3", "c4d3"])
def test_zero_filter_lattice_holds_pixels_the_reference_leaves_undefined(fs):
    """at least 5 % of the lattice pixels are ones whose bounds were NaN before D10 (the model with d10=False computes
    colour / filter * opacity as the reference does)"""
    res = mc.intervals(fs, "zero_filter", (("d10", False),))
    now = {r["px"]: r for r in mc.intervals(fs, "zero_filter")}
    nan = [r["px"] for r in res if r["amb"] is None and r["lo"] is not None and not (np.isfinite(r["lo"]).all() and np.isfinite(r["hi"]).all())]
    print(f"zero_filter {fs}: {len(nan)} of {len(res)} lattice pixels had NaN bounds before D10")
    assert len(nan) >= 0.05 * len(res)
    assert all(now[p]["amb"] is not None or np.isfinite(now[p]["lo"]).all() and np.isfinite(now[p]["hi"]).all() for p in nan)


@pytest.mark.parametrize("fs", ["c1", "c3"])
def test_model_without_the_exponent_floor_rejects_the_oracle(fs):
    """the model-side counterpart of a kernel that drops max(512 * shininess, 1): row 2 of `shiny` has 512 * 0.001"""
    cfg, flat = mc.workload(fs, "shiny")
    argb, planes, st = oracle_lib.render(flat, cfg)
    s = fc.check(mc.intervals(fs, "shiny", (("shininess_clamp", False),)), cfg.width, planes["rgb"], planes["hit_id"], planes["hit_t"], t_rel=1e-5)
    print(f"shiny {fs}: the oracle leaves the interval of the model without the floor on {len(s['bad'])} pixels")
    assert s["bad"]


# ---- stacks of panes -------------------------------------------------------------------------------------------------
STACKS = {
    "white1": (1, mc.WHITE, 0.5), "white2": (2, mc.WHITE, 0.5), "white3": (3, mc.WHITE, 0.5), "white4": (4, mc.WHITE, 0.5),
    "coloured4": (4, mc.COLOURED, 0.5), "tiny1": (1, mc.WHITE, mc.TINY_OPACITY),
}


@pytest.mark.parametrize("name", sorted(STACKS))
def test_oracle_chain_through_a_stack_of_panes(rq_ref, name):
    k, colour, opacity = STACKS[name]
    flat = mc.pane_stack(k, colour, opacity)
    o, d = mc.pane_rays()
    res = qc.model_answers("any", flat, qc.query_config(), o, d)
    got = rq.ref_any(rq_ref, flat, o, d)
    s = qc.check_any(res, got)
    print(f"{name}: model opacity {res[0]['op']}, filter {res[0]['filt'][0]}; oracle {got['combined_opacity'][0]}, {got['color_filter'][0]}")
    assert s["ambiguous"] == 0 and not s["bad"], s
    assert (res[0]["has"], res[0]["occluded"]) == (True, False)
    if name == "tiny1":
        mc.assert_tiny_opacity(res[0], got)
    elif colour == mc.WHITE:
        f, op = mc.WHITE_TABLE[k]
        assert np.abs(res[0]["filt"][0] - f).max() < 1e-12 and abs(res[0]["op"][0] - op) < 1e-6
    else:
        assert np.abs(res[0]["filt"][0] - (1 - k * 0.5 * np.asarray(colour))).max() < 1e-12


def test_capacity_stack_in_the_model():
    """255 panes of opacity 1e-3: the per-channel absorption stays under the fixed-point capacity of 256.  (The oracle's
    running float subtraction is 8e-4 off there: the GPU is compared with the model alone.)"""
    flat = mc.pane_stack(mc.CAPACITY_K, mc.WHITE, mc.CAPACITY_OPACITY)
    o, d = mc.pane_rays()
    r = qc.model_answers("any", flat, qc.query_config(), o, d)[0]
    assert not qc.is_amb(r) and (r["has"], r["occluded"]) == (True, False)
    absorbed = 1 - r["filt"][0]
    assert 254 < absorbed.max() < 256 and r["op"] == (0.0, 0.0)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_oracle_radiance_on_a_wall_lit_through_a_stack(tr_ref, k):
    flat = mc.pane_stack(k, wall=True)
    o, d = mc.wall_rays()
    tcfg = qc.trace_config("plain", False)
    got = tr.ref_trace(tr_ref, flat, tcfg, o, d)
    s = qc.check_trace(flat, qc.model_answers("trace", flat, tcfg, o, d), o, d, got)
    print(f"wall behind {k} panes: rgb {got['rgb'].tolist()}, worst excess {s['worst']:.2e}, ambiguous {s['ambiguous']}")
    assert s["ambiguous"] == 0 and s["hits"] == o.shape[0] and not s["bad"], s
    assert np.isfinite(got["rgb"]).all()
    if k >= 2:
        # nothing of the light in front of the stack arrives: the wall is lit as it is without that light
        dark = mc.pane_stack(k, wall=True)
        dark.lights[0, 6] = 0.0
        assert np.array_equal(tr.ref_trace(tr_ref, dark, tcfg, o, d)["rgb"], got["rgb"])
    else:
        dark = mc.pane_stack(k, wall=True)
        dark.lights[0, 6] = 0.0
        assert np.abs(tr.ref_trace(tr_ref, dark, tcfg, o, d)["rgb"] - got["rgb"]).max() > 1e-3
