"""Cases shared by test_material_domain.py (CPU, the oracle) and test_material_domain_gpu.py: the synthetic soft-shadow scene
of f64_model.build_scene with its material rows and lights replaced by values at the edges of the material domain, and
stacks of parallel panes for the ray queries.  Every other renderer test draws its materials from a narrow box (shininess
up to 0.6, ior 1.1 to 1.9, opacity 0.55 to 1, light intensity up to 0.8); these are the values at which the kernels' colour
terms decide differently: the specular exponent max(512 * shininess, 1) from its floor to 2048, rgb above 1, ior below,
at and just above 1, opacity at EPS, near 0, at 1 and above it (DESIGN D9), reflective transmissive rows, and shadow chains
whose filter reaches 0 or goes below it (DESIGN D10).

The float64 model's intervals are computed once per (feature set, variant), in worker processes (f64_cases)."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import f64_cases as fc
from f64_model import TOL, build_scene
from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig
from hslu_i.ba_raytracing.f2501_raytracer_amd.scene import FlatScene

# feature sets: features, depth.  c3 and c4d3 are f64_cases.SYN_CASES' (the unmodified scene's intervals are shared with it)
FEATURE_SETS = {
    "c1": ([], None),
    "c2d3": (["realistic"], 3),
    "c3": fc.SYN_CASES["c3"],
    "c4d3": fc.SYN_CASES["c4d3"],
}
SOFT = ("c3", "c4d3")  # the feature sets with soft shadows: the penumbra guard applies
STATS = ("rays_primary", "rays_reflection", "rays_refraction", "rays_shadow", "pixels_written")
# material columns: r, g, b, metallic, shininess, ior, opacity, boost, has_opacity
SHININESS, IOR, OPACITY = 4, 5, 6


def _shiny(m, l):
    m[:, SHININESS] = [1.0, 2.0, 0.001, 1.0, 4.0]  # exponents 512, 1024, the floor 1, 512, 2048
    l[:, 6] *= 2.5  # rgb goes above 1


def _glass(m, l):
    m[1] = [1, 1, 1, 0, 0.2, 2.4, 0.05, 0.1, 1]
    m[4] = [0.7, 0.8, 0.9, 0, 0.1, 0.8, 1.0, 0, 1]  # ior below 1; opacity at both ends


def _metglass(m, l):
    m[1] = [0.6, 0.9, 0.7, 0.3, 0.2, 1.5, 0.7, 1.0, 1]  # transmissive and reflective, boost 1
    m[4] = [0.7, 0.8, 0.9, 0.05, 0.1, 1.0, 0.4, 0, 1]   # ior exactly 1


def _tiny(m, l):
    m[1, IOR], m[1, OPACITY] = 1.000293, 2e-7  # air; an opacity just above EPS
    m[4, 0], m[4, OPACITY] = 0.0, 1.19e-7      # |opacity| <= EPS: not transmissive
    m[2, 0:3] = [0, 1, 0]
    l[0, 3:6] = [1, 0, 0]
    l[1, 6] = 0.0


def _over(m, l):
    m[4, OPACITY] = 1.5  # DESIGN D9


def _neg_filter(m, l):
    for r in (1, 4):
        m[r, 0:3], m[r, OPACITY] = [1, 0.9, 0.6], 0.3  # two of them: filter -0.4


def _zero_filter(m, l):
    for r in (1, 4):
        m[r, 0:3], m[r, OPACITY] = [1, 1, 1], 0.5  # two of them: filter 0, combined opacity 0


def _backpane(m, l):
    m[4, IOR], m[4, OPACITY] = 2.4, 0.4  # with BACK_PANE: total internal reflection beyond 24.6 degrees, and not saturated


# variants that also turn the stored normals of the glass pane (triangles 2 and 3): every shadow ray from the wall then meets
# the pane from its back, the `inside` side of the occluder Fresnel term, which no ray of the scene as built does on a triangle
BACK_PANE = ("backpane",)

VARIANTS = {"backpane": _backpane, "shiny": _shiny, "glass": _glass, "metglass": _metglass, "tiny": _tiny, "over": _over, "neg_filter": _neg_filter,
            "zero_filter": _zero_filter}


def config(fs):
    feats, depth = FEATURE_SETS[fs]
    return RenderConfig.from_features(feats, width_override=fc.SYN_W, height_override=fc.SYN_H, depth_override=depth, n_cloud_sets=64)


def workload(fs, variant=None):
    """-> (cfg, flat): build_scene(cfg, soft=True) at 48 x 40, materials and lights as the variant sets them (None: as built)"""
    cfg = config(fs)
    flat = build_scene(cfg, soft=True)
    if variant is None:
        return cfg, flat
    m, l = flat.materials.astype(np.float32).copy(), flat.lights.astype(np.float32).reshape(-1, 7).copy()
    VARIANTS[variant](m, l)
    flat = dataclasses.replace(flat, materials=m, lights=l.reshape(flat.lights.shape))
    if variant in BACK_PANE:
        n = flat.tri_normal.copy()
        n.reshape(-1, 3)[2:4] *= -1
        flat = dataclasses.replace(flat, tri_normal=n)
    return cfg, flat


@functools.lru_cache(maxsize=None)
def intervals(fs, variant=None, mutation=()):
    """the model's intervals on the lattice of f64_cases.syn_pixels(); mutation: Model keywords as a tuple of pairs"""
    if variant is None and not mutation and fs in fc.SYN_CASES:
        return fc.syn_intervals(fs)
    return fc.model_intervals("scene", workload(fs, variant), fc.syn_pixels(), **dict(mutation))


@functools.lru_cache(maxsize=None)
def counts(fs, variant):
    return fc.scene_counts(*workload(fs, variant))


def differing(fs, variant):
    """lattice pixels whose nominal model colour differs from the unmodified scene's by more than TOL"""
    n = 0
    for a, b in zip(intervals(fs, variant), intervals(fs)):
        assert a["px"] == b["px"]
        if a["amb"] is not None or b["amb"] is not None:
            continue
        na = np.zeros(3) if a["nom"] is None else a["nom"]
        nb = np.zeros(3) if b["nom"] is None else b["nom"]
        n += bool(np.abs(na - nb).max() > TOL)  # (NaN compares false: a non-finite pixel does not count)
    return n


def check_frame(name, fs, variant, planes, stats):
    """the frame checks both files share: the interval check with its guards, the counters, and the no-op guard"""
    cfg = config(fs)
    s = fc.check(intervals(fs, variant), cfg.width, planes["rgb"], planes["hit_id"], planes["hit_t"], t_rel=1e-5)
    fc.assert_guards(name, s, penumbra=fs in SOFT)
    assert not s["bad"], (name, s["bad"][:5])
    assert {k: stats[k] for k in STATS} == counts(fs, variant), name
    assert differing(fs, variant) >= 0.1 * s["n"], (name, differing(fs, variant))
    return s


# ---- stacks of panes for the ray queries -----------------------------------------------------------------------------
PANE_O, PANE_D = (0.0, 0.0, 0.0), (0.05, 0.02, 1.0)
WHITE, COLOURED = (1.0, 1.0, 1.0), (1.0, 0.5, 0.25)
# the filter sums are 2^-24 fixed point in 32 bits: a channel's absorption may sum to just under 256 (include/rt_hip.h)
CAPACITY_K, CAPACITY_OPACITY = 255, 1e-3
# an opacity just above EPS = 2^-23, below which a material is not transmissive: the pane must still be read as transmissive
TINY_OPACITY = 2e-7
# what oracle and model give for k white panes of opacity 0.5 (ior 1.3): filter, combined opacity
WHITE_TABLE = {1: (0.5, 0.4914934), 2: (0.0, 0.0), 3: (-0.5, 0.0), 4: (-1.0, 0.0)}


def _triangles(tris, mats, tri_mat, lights):
    f32 = np.float32
    v = np.asarray(tris, np.float64)
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    n = np.cross(e1, e2)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    z = np.zeros(0, f32)
    return FlatScene(np.zeros((0, 3), f32), z, z, np.zeros(0, np.uint32), v[:, 0].astype(f32), e1.astype(f32), e2.astype(f32), n.astype(f32),
                     np.asarray(tri_mat, np.uint32), np.asarray(mats, f32), np.asarray(lights, f32).reshape(-1, 7))


def _pane(z, flip):
    """one triangle in the plane z, so wide that the ray of PANE_O / PANE_D stays more than 0.1 off its edges; flip turns its
    normal (the ray meets every other pane from its back: both branches of the Fresnel term)"""
    a, b, c = (-1.0, -1.0, z), (3.0, -1.0, z), (-1.0, 3.0, z)
    return (a, c, b) if flip else (a, b, c)


def pane_stack(k, colour=WHITE, opacity=0.5, wall=False):
    """k parallel panes at z = 0.1 + 0.01 i, of one transmissive material (ior 1.3).  wall=True adds an opaque wall at z = 1,
    a light in front of the stack (every shadow ray from the wall to it crosses the k panes) and one behind it"""
    tris = [_pane(0.1 + 0.01 * i, i % 2 == 1) for i in range(k)]
    mats = [[*colour, 0.0, 0.1, 1.3, opacity, 0.0, 1]]
    tri_mat, lights = [0] * k, [[0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0]]
    if wall:
        tris.append(((-1.0, -1.0, 1.0), (-1.0, 3.0, 1.0), (3.0, -1.0, 1.0)))  # faces -z
        mats.append([0.8, 0.7, 0.6, 0.0, 0.3, 1.0, 0.0, 0.0, 0])
        tri_mat.append(1)
        lights = [[0.2, 0.1, 0.0, 1.0, 0.95, 0.9, 0.8], [0.4, 0.3, 0.6, 0.9, 1.0, 1.0, 0.5]]
    return _triangles(tris, mats, tri_mat, lights)


def pane_rays(n=1):
    return np.tile(np.asarray(PANE_O, np.float32), (n, 1)), np.tile(np.asarray(PANE_D, np.float32), (n, 1))


def wall_rays():
    """rays that start behind the stack and meet the wall: the stack's ray, and three more whose shadow rays cross the panes
    elsewhere"""
    o = np.asarray([(0.025, 0.01, 0.5), (0.3, 0.2, 0.5), (0.1, 0.5, 0.4), (0.6, 0.1, 0.7)], np.float32)
    d = np.asarray([PANE_D, (0.0, 0.0, 1.0), (0.1, -0.1, 1.0), (-0.2, 0.1, 0.5)], np.float32)
    return o, d


def assert_tiny_opacity(want, got):
    """one pane of TINY_OPACITY: what it lets through is far below TOL, so the interval check cannot tell it from an opaque
    reading of the row.  1 - io is rounded once to fp32 next to 1 (half an ulp, 2^-24) and once to 2^-28 fixed point: the
    opacity is positive and within 2^-23 of the model's"""
    op = float(got["combined_opacity"][0])
    assert not got["completely_occluded"][0] and op > 0.0, op
    assert abs(op - want["op"][0]) <= 2.0 ** -23, (op, want["op"])
