"""The ray queries on the GPU (DeviceScene.cast_rays, .any_intersection, .trace_rays) against the independent float64 model
(tests/f64_model.py): the ray sets, bars and checks of f64_query_cases.py, which test_f64_model_queries.py applies to the
oracle wrappers on CPU -- back-face culling off and on, an ordered radiance batch per scene, small batches cut from a set,
and the refitted tree after an in-place scene update.  The model's answers are computed once per set, in worker processes."""
import numpy as np
import pytest

import f64_query_cases as qc
import scene_update_cases as su
from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceScene

pytestmark = pytest.mark.gpu

CULL = [False, True]
_cache = {}


def _scene(name):
    if name not in _cache:
        _cache[name] = DeviceScene(qc.workload(name)[1], 0)
    return _cache[name]


def _fields(r):
    return {k: np.asarray(getattr(r, k)) for k in r._fields}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint8) if a.dtype == np.bool_ else a


@pytest.mark.parametrize("cull", CULL)
@pytest.mark.parametrize("name", qc.SCENES)
def test_gpu_nearest_hit_within_the_model(name, cull):
    cfg, flat = qc.workload(name)
    o, d, kind, md = qc.rays(name)
    got = _fields(_scene(name).cast_rays(o, d, backface_culling=cull))
    s = qc.check_nearest(flat, qc.nearest_answers(name, cull), o, d, got)
    print(f"gpu cast_rays {name} cull={cull}: {s['n']} rays, {s['hits']} hits, ambiguous {s['ambiguous']}, worst t {s['worst_t']:.2f} U "
          f"(bar {qc.BAR_T:.1f}), point {s['worst_point']:.2f} U (bar {qc.BAR_POINT:.1f}), sphere normal {s['worst_normal']:.2f} "
          f"(bar {qc.BAR_NORMAL:.1f}), differ {len(s['bad'])}")
    assert s["hits"] >= 0.5 * s["n"]
    assert not s["bad"], s["bad"][:5]


@pytest.mark.parametrize("with_max", [True, False], ids=["max_distance", "unbounded"])
@pytest.mark.parametrize("cull", CULL)
@pytest.mark.parametrize("name", qc.SCENES)
def test_gpu_occlusion_within_the_model(name, cull, with_max):
    o, d, kind, md = qc.rays(name)
    got = _fields(_scene(name).any_intersection(o, d, md if with_max else None, backface_culling=cull))
    s = qc.check_any(qc.any_answers(name, cull, with_max), got)
    print(f"gpu any_intersection {name} cull={cull} max_distance={with_max}: {s['n']} segments, ambiguous {s['ambiguous']}, partially "
          f"transmitted {s['partial']}, occluded {s['occluded']}, worst excess {s['worst']:.2e}, differ {len(s['bad'])}")
    assert s["partial"] > 0 and s["occluded"] > 0
    assert not s["bad"], s["bad"][:5]


def _check_radiance(name, key, cull, order=None):
    cfg, flat = qc.workload(name)
    o, d, kind, md = qc.rays(name, near=True)
    tcfg = qc.trace_config(key, cull)
    ds = _scene(name)
    res = qc.trace_answers(name, key, cull)
    s = qc.check_trace(flat, res, o, d, _fields(ds.trace_rays(o, d, tcfg, order=order)))
    print(f"gpu trace_rays {name} {key} cull={cull} order={order}: {s['n']} rays, {s['hits']} hits, ambiguous {s['ambiguous']}, narrow "
          f"{s['narrow']}, worst excess {s['worst']:.2e}, worst t {s['worst_t']:.2f} U, differ {len(s['bad'])}")
    assert s["narrow"] >= 0.8 * s["hits"], s
    assert not s["bad"], s["bad"][:5]
    return ds, res, o, d, tcfg, s


@pytest.mark.parametrize("key", sorted(qc.TRACE_FEATURES))
@pytest.mark.parametrize("cull", CULL)
@pytest.mark.parametrize("name", qc.SCENES)
def test_gpu_radiance_within_the_model(name, cull, key):
    ds, res, o, d, tcfg, s = _check_radiance(name, key, cull)
    # the counters, on the rays the model decides: a batch of them alone casts what the model counts
    ua = qc.unambiguous(res)
    ds.trace_rays(o[ua], d[ua], tcfg)
    st = ds.last_trace_stats
    assert {k: st[k] for k in qc.COUNTERS} == s["counts"], (st, s["counts"])
    assert st["pixels_written"] == s["hits"]


@pytest.mark.parametrize("name", qc.SCENES)
def test_gpu_ordered_radiance_within_the_model(name):
    _check_radiance(name, "realistic_soft", True, order=True)


@pytest.mark.parametrize("n", [1, 63, 257])
def test_batches_cut_from_a_set_give_the_rows_of_the_full_batch(n):
    """(radiance with hard shadows: with soft shadows a ray's index in its batch keys its light clouds)"""
    name, first = "text_lowres", 300
    o, d, kind, md = qc.rays(name)
    ds = _scene(name)
    cut = slice(first, first + n)
    tcfg = qc.trace_config("plain", True)
    pairs = [(ds.cast_rays(o, d, backface_culling=True), ds.cast_rays(o[cut], d[cut], backface_culling=True)),
             (ds.any_intersection(o, d, md, backface_culling=True), ds.any_intersection(o[cut], d[cut], md[cut], backface_culling=True)),
             (ds.trace_rays(o, d, tcfg), ds.trace_rays(o[cut], d[cut], tcfg))]
    for full, part in pairs:
        for k in full._fields:
            a, b = np.asarray(getattr(full, k))[cut], np.asarray(getattr(part, k))
            assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), (type(full).__name__, k)


def updated_text_lowres():
    """text_lowres with every sphere moved and triangles [200, 700) of the text mesh turned and shifted"""
    flat = qc.workload("text_lowres")[1].contiguous()
    new = su.turn_mesh(su.move_spheres(flat), (200, 500), 20.0, (0.01 * su.diagonal(flat), -0.005 * su.diagonal(flat), 0.0))
    return flat, new


@pytest.mark.parametrize("cull", CULL)
def test_queries_after_an_update_agree_with_a_model_of_the_updated_scene(cull):
    """The refitted tree against the model, not against a fresh pack: after DeviceScene.update the nearest hits and the
    occlusion chain are those of a Model built from the new description."""
    flat, new = updated_text_lowres()
    o, d, kind, md = qc.rays("text_lowres")
    ds = DeviceScene(flat, 0)
    before = ds.cast_rays(o, d, backface_culling=cull)
    ds.update(new)
    hits = _fields(ds.cast_rays(o, d, backface_culling=cull))
    assert (_bits(hits["t"]) != _bits(before.t)).mean() > 0.05, "the update moved too little of what the rays see"
    s = qc.check_nearest(new, qc.model_answers("nearest", new, qc.query_config(cull), o, d), o, d, hits)
    print(f"after the update, cast_rays cull={cull}: {s['hits']} hits, ambiguous {s['ambiguous']}, worst t {s['worst_t']:.2f} U, differ {len(s['bad'])}")
    assert s["ambiguous"] <= 0.1 * s["n"] and s["hits"] >= 0.5 * s["n"]
    assert not s["bad"], s["bad"][:5]
    a = qc.check_any(qc.model_answers("any", new, qc.query_config(cull), o, d, md), _fields(ds.any_intersection(o, d, md, backface_culling=cull)))
    print(f"after the update, any_intersection cull={cull}: ambiguous {a['ambiguous']}, partially transmitted {a['partial']}, differ {len(a['bad'])}")
    assert a["ambiguous"] <= 0.1 * a["n"] and a["partial"] > 0
    assert not a["bad"], a["bad"][:5]
    ds.close()
