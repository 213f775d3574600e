"""The oracle wrappers of the ray queries (tests/ray_query_ref.c, tests/trace_rays_ref.c) against the independent float64
model (tests/f64_model.py), on CPU, with back-face culling off and on: nearest hits, the opacity / filter chain of
any_intersection with and without max_distance, and radiance at depth 3 with hard and soft shadows.  The ray sets, the
bars and the checks are f64_query_cases.py's; the GPU is held to the same ones in test_f64_model_queries_gpu.py.

What the sets must be to say anything is asserted here, where no GPU is needed: at most 10 % ambiguous rays, culling
changing the nearest hit of at least a quarter of the from-behind rays, at least 5 % of the segments partially
transmitted.  A model whose culling rule is mutated (threshold 0, no exemption for transmissive materials, no culling on
the shadow chain) must reject the oracle's culling-on output.
"""
import numpy as np
import pytest

import f64_query_cases as qc
import ray_query_cases as rq
import trace_rays_cases as tr

CULL = [False, True]


@pytest.fixture(scope="module")
def rq_ref(tmp_path_factory):
    return rq.build_ref(tmp_path_factory.mktemp("rqref"))


@pytest.fixture(scope="module")
def tr_ref(tmp_path_factory):
    return tr.build_ref(tmp_path_factory.mktemp("trref"))


def _nearest_id(r):
    return -1 if r is None else r[0]


@pytest.mark.parametrize("cull", CULL)
@pytest.mark.parametrize("name", qc.SCENES)
def test_nearest_hit_of_the_oracle_within_the_model(rq_ref, name, cull):
    cfg, flat = qc.workload(name)
    o, d, kind, md = qc.rays(name)
    res = qc.nearest_answers(name, cull)
    s = qc.check_nearest(flat, res, o, d, rq.ref_nearest(rq_ref, flat, o, d, cull))
    print(f"rq_nearest {name} cull={cull}: {s['n']} rays, {s['hits']} hits, ambiguous {s['ambiguous']}, worst t {s['worst_t']:.2f} U "
          f"(bar {qc.BAR_T:.1f}), point {s['worst_point']:.2f} U (bar {qc.BAR_POINT:.1f}), sphere normal {s['worst_normal']:.2f} "
          f"(bar {qc.BAR_NORMAL:.1f}), differ {len(s['bad'])}")
    assert s["ambiguous"] <= 0.1 * s["n"], s
    assert s["hits"] >= 0.5 * s["n"]
    assert not s["bad"], s["bad"][:5]


@pytest.mark.parametrize("name", qc.SCENES)
def test_culling_changes_the_from_behind_rays(name):
    o, d, kind, md = qc.rays(name)
    off, on = qc.nearest_answers(name, False), qc.nearest_answers(name, True)
    behind = np.flatnonzero((kind == qc.KIND_BEHIND_TRI) | (kind == qc.KIND_BEHIND_SPHERE))
    changed = sum(1 for i in behind if not qc.is_amb(off[i]) and not qc.is_amb(on[i]) and _nearest_id(off[i]) != _nearest_id(on[i]))
    print(f"{name}: culling changes the model's nearest id on {changed} of {behind.size} from-behind rays")
    assert changed >= 0.25 * behind.size


@pytest.mark.parametrize("with_max", [True, False], ids=["max_distance", "unbounded"])
@pytest.mark.parametrize("cull", CULL)
@pytest.mark.parametrize("name", qc.SCENES)
def test_occlusion_of_the_oracle_within_the_model(rq_ref, name, cull, with_max):
    cfg, flat = qc.workload(name)
    o, d, kind, md = qc.rays(name)
    got = rq.ref_any(rq_ref, flat, o, d, md if with_max else None, cull)
    s = qc.check_any(qc.any_answers(name, cull, with_max), got)
    partial = int(((got["has_intersection"] != 0) & (got["completely_occluded"] == 0)).sum())
    print(f"rq_any {name} cull={cull} max_distance={with_max}: {s['n']} segments, ambiguous {s['ambiguous']}, partially transmitted "
          f"{partial} ({s['partial']} of them compared), occluded {s['occluded']}, worst excess {s['worst']:.2e}, differ {len(s['bad'])}")
    assert s["ambiguous"] <= 0.1 * s["n"], s
    assert partial >= 0.05 * s["n"], partial
    assert not s["bad"], s["bad"][:5]


@pytest.mark.parametrize("key", sorted(qc.TRACE_FEATURES))
@pytest.mark.parametrize("cull", CULL)
@pytest.mark.parametrize("name", qc.SCENES)
def test_radiance_of_the_oracle_within_the_model(tr_ref, name, cull, key):
    cfg, flat = qc.workload(name)
    o, d, kind, md = qc.rays(name, near=True)
    tcfg = qc.trace_config(key, cull)
    res = qc.trace_answers(name, key, cull)
    s = qc.check_trace(flat, res, o, d, tr.ref_trace(tr_ref, flat, tcfg, o, d))
    print(f"tr_trace {name} {key} cull={cull}: {s['n']} rays, {s['hits']} hits, ambiguous {s['ambiguous']}, narrow {s['narrow']}, "
          f"worst excess {s['worst']:.2e}, worst t {s['worst_t']:.2f} U, differ {len(s['bad'])}")
    assert s["ambiguous"] <= 0.1 * s["n"], s
    assert s["narrow"] >= 0.8 * s["hits"], s
    assert not s["bad"], s["bad"][:5]
    # the counters, on the rays the model decides: a batch of them alone casts what the model counts
    ua = qc.unambiguous(res)
    alone = tr.ref_trace(tr_ref, flat, tcfg, o[ua], d[ua])
    assert {k: alone["counters"][k] for k in qc.COUNTERS} == s["counts"]


MUTATIONS = {
    "threshold_0": (("cull_threshold", 0.0),),
    "transmissive_not_exempt": (("cull_exempts_transmissive", False),),
    "shadow_chain_does_not_cull": (("cull_shadows", False),),
}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_mutated_culling_rejects_the_oracle(rq_ref, mutation):
    """The checks are sensitive to the rule: a model with another threshold, without the exemption, or whose shadow chain
    does not cull finds unambiguous rays on which the oracle (cull = 1) differs from it."""
    for name in ("test_scene", "synthetic"):
        cfg, flat = qc.workload(name)
        o, d, kind, md = qc.rays(name)
        n = qc.check_nearest(flat, qc.nearest_answers(name, True, MUTATIONS[mutation]), o, d, rq.ref_nearest(rq_ref, flat, o, d, True))
        a = qc.check_any(qc.any_answers(name, True, False, MUTATIONS[mutation]), rq.ref_any(rq_ref, flat, o, d, None, True))
        print(f"{mutation} on {name}: the oracle differs from the mutated model on {len(n['bad'])} nearest hits and {len(a['bad'])} segments")
        assert len(n["bad"]) + len(a["bad"]) > 0
    if mutation == "shadow_chain_does_not_cull":
        assert not n["bad"], "cast_ray does not walk the shadow chain"
