"""Pipeline-level known answers in float64.

`tests/golden/known_answers.json` pins single functions.  This file pins the PIPELINE: a float64 model of one pixel of
the reference's Whitted loop, written from the reference's formulas (`single_raytrace`,
`calculate_lighting` + `PointLight::calculate_contribution_at`, `has_any_intersection` with its opacity / filter
chain, `calculate_reflection`, `calculate_refractions`, `compute_fresnel`, distance attenuation) and NOT from
oracle/rt_oracle.c -- textbook ray/sphere and Moeller-Trumbore ray/triangle tests instead of the matrix-inverse form,
numpy float64 throughout (the model lives in tests/f64_model.py).  The fp32 oracle must agree with it on pixels chosen to exercise each term: lit diffuse +
specular, a shadow filtered through glass (opacity chain + absorption filter), an opaque shadow, one bounce of
reflection on a metallic sphere, and refraction through a glass sphere with Fresnel weights.  CPU only.
"""
import numpy as np
import pytest

import oracle_lib
from f64_model import Model, build_scene
from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig


@pytest.mark.parametrize("features", [[], ["reflections"], ["refractions"], ["reflections", "refractions"]])
def test_oracle_matches_float64_pipeline_model(features):
    cfg = RenderConfig.from_features(features, width_override=96, height_override=80, depth_override=3)
    flat = build_scene(cfg)
    model = Model(flat, cfg, "reflections" in features, "refractions" in features)
    argb, planes, st = oracle_lib.render(flat, cfg, n_threads=4)
    rgb = planes["rgb"].reshape(cfg.height, cfg.width, 3)
    ids = planes["hit_id"].reshape(cfg.height, cfg.width)
    seen = set()
    worst = 0.0
    for gy in range(2, cfg.height, 7):
        for gx in range(1, cfg.width, 5):
            want = model.pixel(gx, gy)
            if want is None:
                assert ids[gy, gx] == -1
                continue
            seen.add(int(ids[gy, gx]))
            d = float(np.abs(rgb[gy, gx] - want).max())
            worst = max(worst, d)
            assert d <= 5e-5, (gx, gy, int(ids[gy, gx]), rgb[gy, gx], want)
    # the sample covers the glass sphere, the opaque sphere, the mirror and the wall
    assert {0, 1, 2}.issubset(seen) and (3 in seen or 4 in seen), seen
    print(f"{features}: max |dRGB| oracle(fp32) vs float64 model = {worst:.2e} over {len(seen)} objects")
