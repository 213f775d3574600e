"""Soft shadows and anti-aliasing against the independent float64 model (tests/f64_model.py), on CPU.

The fp32 oracle renders small synthetic scenes at config-3 features (AA with the plain and the randomness table, 10
cloud points per light) and config-4 features (reflections, refractions, 24 spp, 28 cloud points, depth 3 and 8), and both
again with back-face culling on a scene where it decides primary and shadow rays; every
sampled pixel must lie in the model's per-pixel interval widened by TOL, and the ray counters must match exactly.  The
committed at-spec fixtures spec_c3 / spec_c3lowres are checked on 48 fixed pixels each (hit id, t to 1e-5 relative,
RGB).  Oracle renders made with a rotated cloud table or y-negated AA offsets must be rejected.
"""
import os
import subprocess

import numpy as np
import pytest

import f64_cases as fc
import oracle_lib
from f64_model import cloud_hash
from hslu_i.ba_raytracing.f2501_raytracer_amd import sampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = ("rays_primary", "rays_reflection", "rays_refraction", "rays_shadow", "pixels_written")


def test_cloud_hash_matches_the_header(tmp_path):
    grid = [(s, p, l) for s in (0, 1, 7, 0xFFFFFFFF) for p in (0, 1, 1619, 2186999, 0x7FFFFFFF) for l in range(6)]
    prog = tmp_path / "h.c"
    prog.write_text('#include <stdio.h>\n#include "rt_hip.h"\nint main(void){unsigned g[][3]={' +
                    ",".join("{%du,%du,%du}" % g for g in grid) + '};for(unsigned i=0;i<sizeof g/sizeof g[0];i++)'
                    'printf("%u ", rt_cloud_hash(g[i][0],g[i][1],g[i][2])); return 0;}\n')
    exe = tmp_path / "h"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [cloud_hash(*g) for g in grid]


@pytest.mark.parametrize("key", sorted(fc.SYN_CASES))
def test_oracle_synthetic_scene_within_the_float64_intervals(key):
    cfg, flat = fc.syn_workload(key)
    argb, planes, st = oracle_lib.render(flat, cfg)
    s = fc.check(fc.syn_intervals(key), cfg.width, planes["rgb"], planes["hit_id"], planes["hit_t"], t_rel=1e-5)
    fc.assert_guards(f"oracle {key}", s)
    assert not s["bad"], s["bad"][:5]
    want = fc.model_counts(key)
    assert {k: st[k] for k in STATS} == want


@pytest.mark.parametrize("key", [k for k in sorted(fc.SYN_CASES) if k.endswith("cull")])
def test_culling_decides_a_tenth_of_the_synthetic_lattice(key):
    """The culling cases say something only if culling changes the picture: the model's nominal colour with culling on
    and with culling off differ by more than TOL on at least 10 % of the lattice pixels."""
    on = fc.syn_intervals(key)
    off = fc.model_intervals("syn", key, fc.syn_pixels(), cull=False)
    assert [r["px"] for r in on] == [r["px"] for r in off]
    z = np.zeros(3)
    differ = sum(1 for a, b in zip(on, off) if a["amb"] is None and b["amb"] is None and
                 np.abs((z if a["nom"] is None else a["nom"]) - (z if b["nom"] is None else b["nom"])).max() > fc.TOL)
    print(f"{key}: culling changes {differ} of {len(on)} lattice pixels by more than {fc.TOL:g}")
    assert differ >= 0.1 * len(on)


@pytest.mark.parametrize("name", fc.SPEC_NAMES)
def test_at_spec_fixture_pixels_within_the_float64_intervals(name):
    cfg, flat, meta, z = fc.spec_workload(name)
    s = fc.check(fc.spec_intervals(name), cfg.width, *fc.spec_planes(cfg, meta, z), t_rel=1e-5)
    fc.assert_guards(f"fixture {name}", s, penumbra=False)
    assert s["n"] >= 48 and not s["bad"], s["bad"][:5]


def _rotated_cloud(cfg):
    return np.roll(sampling.cloud_sets(cfg), 1, axis=0)


def _y_negated_aa(cfg):
    off = sampling.aa_offsets(cfg).copy()
    off[:, 1] = -off[:, 1]
    return off


@pytest.mark.parametrize("mutation", ["cloud_rotated", "aa_y_negated"])
def test_model_rejects_renders_with_mutated_tables(mutation):
    key = "c3rand"
    cfg, flat = fc.syn_workload(key)
    kw = dict(cloud=_rotated_cloud(cfg)) if mutation == "cloud_rotated" else dict(aa_offsets=_y_negated_aa(cfg))
    argb, planes, st = oracle_lib.render(flat, cfg, **kw)
    s = fc.check(fc.syn_intervals(key), cfg.width, planes["rgb"], planes["hit_id"], planes["hit_t"], t_rel=1e-5)
    print(f"{mutation}: {len(s['bad'])} of {s['n']} sampled pixels outside the intervals")
    assert len(s["bad"]) > 0.1 * s["n"]
