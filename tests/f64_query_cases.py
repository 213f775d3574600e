"""Cases and checks shared by test_f64_model_queries.py (CPU, the oracle wrappers) and test_f64_model_queries_gpu.py: the
seeded ray sets of the ray queries, what the float64 model (tests/f64_model.py) says about each ray -- computed once per
set in worker processes -- and the comparison of an observed batch with it.

Ray sets.  One set of N_RAYS = 1021 rays per scene (a prime: a ragged last wavefront and a ragged last workgroup), made of
  * kinds 1 to 6 of ray_query_cases.rays (inside, outside, 100 extents away, non-unit, zero components, grazing); its
    kinds 7 and 8 start on a surface and stay out, for the reason written in test_ray_query_host.py;
  * "from behind": a point on a triangle of opaque material, a direction with d . n uniform in [0.55, 0.95] (n the
    stored normal), the origin 2e-4 of the extent before the point so that nothing intervenes (test_scene's planes are boxes 1e-3
    of its depth thick); and the same from inside an
    opaque sphere, aimed at a point of its surface.  Half of these are culled when culling is on;
  * "through the glass": from 0.05 to 0.4 extents away at a point of a transmissive object, every other one towards the
    open side of the scene, so that the opacity and filter chain of rt_any_intersection has something to do.

Bars for t, point and normal of a caller ray.  The render's 1e-5 relative bar on t does not fit origins 100 extents away
or grazing hits, so the error is measured in units of
    U = (|o|_inf + t) * eps32 / |d . n|,
the fp32 rounding of the coordinates the hit is computed from, amplified by the angle to the surface.  The error of t is
|dt| / U, of the point max|dp| / U.  A triangle's normal is its stored normal and must be equal bit for bit; a sphere's is
(p - c) / r, so its error is max|dn| / (U / r + eps32).  Measured with the CPU oracle against the model over the three
seeded sets, culling off and on (printed by test_nearest_hit_of_the_oracle_within_the_model):
    worst t 45.37 U, worst point 41.55 U, worst sphere normal 26.23   (text_lowres; test_scene 3.49 / 2.48 / 2.84,
    synthetic 12.65 / 9.41 / 4.80)
The large values are spheres met from outside the scene: the reference's quadratic subtracts |v|^2 - r^2 from (d . v)^2,
which costs eps32 |v|^2 / (2 r |d . n|) in t, |v| / r times what U allows for.  The bars are four times the worst measured
value -- room for other seeds, within an order of magnitude of the measured worst -- and the GPU is held to the same bars:
    BAR_T = 181.5, BAR_POINT = 166.2, BAR_NORMAL = 104.9
Colour, opacity and filter use the project's TOL = 1e-4 on the model's interval.
"""
from __future__ import annotations

import functools
import multiprocessing

import numpy as np

import f64_cases as fc
import f64_model as fm
import ray_query_cases as rq
from f64_model import EPS, TOL, Model
from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig

SCENES = ("test_scene", "text_lowres", "synthetic")
N_RAYS = 1021
K_GENERAL, N_BEHIND, N_GLASS = 72, 256, 333  # 6 * K_GENERAL + N_BEHIND + N_GLASS = N_RAYS
KIND_BEHIND_TRI, KIND_BEHIND_SPHERE, KIND_GLASS = 6, 7, 8
BEHIND = 2e-4  # how far before its point a from-behind ray starts, in extents
BAR_T, BAR_POINT, BAR_NORMAL = 4 * 45.37, 4 * 41.55, 4 * 26.23
TRACE_FEATURES = {"plain": [], "soft": ["soft_shadows"], "realistic_soft": ["realistic", "soft_shadows"]}
COUNTERS = ("rays_primary", "rays_reflection", "rays_refraction", "rays_shadow")


@functools.lru_cache(maxsize=None)
def workload(name):
    """-> (cfg, flat) of a scene; "synthetic" is f64_model.build_scene(cfg, soft=True) as the synthetic frames use it"""
    if name == "synthetic":
        return fc.syn_workload("c3")
    return rq.scene(name)


def query_config(cull=False):
    return RenderConfig.from_features(["backface_culling"] if cull else [])


def trace_config(key, cull):
    return RenderConfig.from_features(TRACE_FEATURES[key] + (["backface_culling"] if cull else []), depth_override=3, n_cloud_sets=64)


def _transmissive(flat):
    m = flat.materials.astype(np.float64)
    return (m[:, 8] != 0) & ~(np.abs(m[:, 6]) <= EPS)


def _perp(rng, n):
    """unit vectors perpendicular to the rows of n"""
    u = np.cross(n, rq._unit(rng, n.shape[0]))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def _on_triangles(rng, flat, ti):
    v1, e1, e2 = (a.astype(np.float64).reshape(-1, 3) for a in (flat.tri_v1, flat.tri_e1, flat.tri_e2))
    u = 0.05 + 0.9 * rng.random((ti.size, 2))
    u = np.where(u.sum(axis=1, keepdims=True) > 1, 1 - u, u) * 0.95
    return v1[ti] + e1[ti] * u[:, :1] + e2[ti] * u[:, 1:]


@functools.lru_cache(maxsize=None)
def rays(name, near=False):
    """-> (origins (N_RAYS, 3) float32, directions float32, kind (N_RAYS,) int, max_distance (N_RAYS,) float32 seeded in
    [0, extent]).  near=True is the set the radiance queries use: the rays of kind 3 start on the same lines 3 extents
    from the centre instead of 100 (shading a hit needs its position to eps_distance, about 1e-5, which fp32 cannot give
    from 100 extents away: the model calls every such ray ambiguous, and a set must stay under 10 % of those)."""
    if near:
        o, d, kind, max_d = rays(name)
        lo, hi = rq.bounds(workload(name)[1])
        ext = float(np.linalg.norm(hi - lo))
        o64, d64 = o.astype(np.float64), d.astype(np.float64)
        far = kind == 2
        o64[far] += d64[far] / np.linalg.norm(d64[far], axis=1, keepdims=True) * (97.0 * ext)
        return np.ascontiguousarray(o64, np.float32), d, kind, max_d
    cfg, flat = workload(name)
    seed = 31 + SCENES.index(name)
    o6, d6 = rq.rays(flat, 8 * K_GENERAL, seed)
    O, D, kind = [o6[:6 * K_GENERAL].astype(np.float64)], [d6[:6 * K_GENERAL].astype(np.float64)], [np.repeat(np.arange(6), K_GENERAL)]
    rng = np.random.default_rng(1000 + seed)
    lo, hi = rq.bounds(flat)
    ext = float(np.linalg.norm(hi - lo))
    tr = _transmissive(flat)
    tri_tr, sph_tr = tr[flat.tri_material.astype(np.int64)], tr[flat.sphere_material.astype(np.int64)]
    sc, sr = flat.sphere_center.astype(np.float64).reshape(-1, 3), np.sqrt(flat.sphere_r_sq.astype(np.float64))
    # from behind: opaque triangles, and from inside opaque spheres
    n_sph = N_BEHIND // 4 if (~sph_tr).any() else 0
    ti = rng.choice(np.flatnonzero(~tri_tr), N_BEHIND - n_sph)
    n = flat.tri_normal.astype(np.float64).reshape(-1, 3)[ti]
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    c = rng.uniform(0.55, 0.95, (ti.size, 1))
    d = n * c + _perp(rng, n) * np.sqrt(1 - c * c)
    O.append(_on_triangles(rng, flat, ti) - d * (BEHIND * ext)), D.append(d), kind.append(np.full(ti.size, KIND_BEHIND_TRI))
    if n_sph:
        si = rng.choice(np.flatnonzero(~sph_tr), n_sph)
        n = rq._unit(rng, n_sph)
        c = rng.uniform(0.55, 0.95, (n_sph, 1))
        d = n * c + _perp(rng, n) * np.sqrt(1 - c * c)
        back = np.minimum(BEHIND * ext, 0.5 * sr[si])[:, None]  # (the chord is 2 r c long: the origin stays inside)
        O.append(sc[si] + n * sr[si, None] - d * back), D.append(d), kind.append(np.full(n_sph, KIND_BEHIND_SPHERE))
    # through the glass
    objs = np.concatenate([np.flatnonzero(sph_tr), flat.n_spheres + np.flatnonzero(tri_tr)])
    pick = rng.choice(objs, N_GLASS)
    target = np.zeros((N_GLASS, 3))
    is_s = pick < flat.n_spheres
    target[is_s] = sc[pick[is_s]] + rq._unit(rng, int(is_s.sum())) * (sr[pick[is_s]] * rng.uniform(0, 0.8, int(is_s.sum())))[:, None]
    target[~is_s] = _on_triangles(rng, flat, pick[~is_s] - flat.n_spheres)
    away = rq._unit(rng, N_GLASS)
    away[::2, 2] = np.abs(away[::2, 2])  # every other one travels towards -z, where all three scenes are open
    o = target + away * ext * rng.uniform(0.05, 0.4, (N_GLASS, 1))
    O.append(o), D.append(target - o), kind.append(np.full(N_GLASS, KIND_GLASS))
    O, D, kind = np.concatenate(O), np.concatenate(D), np.concatenate(kind)
    assert O.shape == (N_RAYS, 3) and kind.shape == (N_RAYS,)
    max_d = rng.uniform(0.0, ext, N_RAYS).astype(np.float32)
    return np.ascontiguousarray(O, np.float32), np.ascontiguousarray(D, np.float32), kind, max_d


# ---- the model's answers, in worker processes ----------------------------------------------------------------------
_W = {}


def _init(flat, cfg, kw):
    _W["m"] = Model(flat, cfg, **kw)


def _eval(job):
    what, idx, o, d, md = job
    m = _W["m"]
    out = []
    for j, i in enumerate(idx):
        try:
            if what == "nearest":
                r = m.cast_ray(o[j], d[j])
            elif what == "any":
                r = m.any_intersection(o[j], d[j], None if md is None else md[j])
            else:
                r = m.trace_ray(o[j], d[j], int(i))
                if r["iv"] is not None:
                    r = dict(r, lo=r["iv"].lo, hi=r["iv"].hi, nom=r["iv"].nom)
                r.pop("iv")
        except fm.Ambiguous as e:
            r = fm.Ambiguous(str(e))
        out.append((int(i), r))
    return out


def model_answers(what, flat, cfg, o, d, max_d=None, index=None, **model_kw):
    """what: "nearest" | "any" | "trace".  -> one entry per ray: the model's answer, or an Ambiguous instance"""
    n = o.shape[0]
    index = np.arange(n) if index is None else np.asarray(index)
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    md = None if max_d is None else np.asarray(max_d, np.float32).astype(np.float64)
    k = fc.n_procs() * 4
    jobs = [(what, index[s::k], o64[s::k], d64[s::k], None if md is None else md[s::k]) for s in range(k) if s < n]
    # spawned, not forked: the GPU tests call this after the parent has opened the device
    with multiprocessing.get_context("spawn").Pool(fc.n_procs(), initializer=_init, initargs=(flat, cfg, model_kw)) as p:
        parts = p.map(_eval, jobs)
    res = dict(r for part in parts for r in part)
    return [res[int(i)] for i in index]


@functools.lru_cache(maxsize=None)
def nearest_answers(name, cull, mutation=()):
    cfg, flat = workload(name)
    o, d, kind, md = rays(name)
    return model_answers("nearest", flat, query_config(cull), o, d, **dict(mutation))


@functools.lru_cache(maxsize=None)
def any_answers(name, cull, with_max, mutation=()):
    cfg, flat = workload(name)
    o, d, kind, md = rays(name)
    return model_answers("any", flat, query_config(cull), o, d, md if with_max else None, **dict(mutation))


@functools.lru_cache(maxsize=None)
def trace_answers(name, key, cull):
    cfg, flat = workload(name)
    o, d, kind, md = rays(name, near=True)
    return model_answers("trace", flat, trace_config(key, cull), o, d)


def is_amb(r):
    return isinstance(r, fm.Ambiguous)


# ---- the checks ----------------------------------------------------------------------------------------------------
def _unit_error(flat, o, d, t, n):
    """U of the module docstring for one ray"""
    dd = d.astype(np.float64)
    dd = dd / np.sqrt(dd @ dd)
    return (float(np.abs(o).max()) + t) * EPS / max(abs(float(dd @ n)), 1e-300)


def check_nearest(flat, res, o, d, got):
    """got: id, t, point, normal, material arrays of a batch.  -> summary; `bad` lists the rays that differ from the
    model, worst_* the largest errors in the units of the module docstring"""
    s = dict(n=len(res), ambiguous=0, hits=0, worst_t=0.0, worst_point=0.0, worst_normal=0.0, bad=[])
    r_sph = np.sqrt(flat.sphere_r_sq.astype(np.float64))
    for i, r in enumerate(res):
        if is_amb(r):
            s["ambiguous"] += 1
            continue
        want = -1 if r is None else r[0]
        if int(got["id"][i]) != want:
            s["bad"].append((i, "id", int(got["id"][i]), want))
            continue
        if r is None:
            continue
        oid, t, p, n, row = r
        s["hits"] += 1
        if int(np.uint32(got["material"][i])) != row:
            s["bad"].append((i, "material", int(got["material"][i]), row))
            continue
        U = _unit_error(flat, o[i], d[i], t, n)
        et = abs(float(got["t"][i]) - t) / U
        ep = float(np.abs(got["point"][i].astype(np.float64) - p).max()) / U
        dn = float(np.abs(got["normal"][i].astype(np.float64) - n).max())
        en = dn / (U / r_sph[oid] + EPS) if oid < flat.n_spheres else (0.0 if dn == 0.0 else np.inf)
        s["worst_t"], s["worst_point"], s["worst_normal"] = max(s["worst_t"], et), max(s["worst_point"], ep), max(s["worst_normal"], en)
        if et > BAR_T or ep > BAR_POINT or en > BAR_NORMAL:
            s["bad"].append((i, "t / point / normal", et, ep, en))
    return s


def check_any(res, got):
    """got: has_intersection, completely_occluded, combined_opacity, color_filter of a batch"""
    s = dict(n=len(res), ambiguous=0, partial=0, occluded=0, worst=0.0, bad=[])
    for i, r in enumerate(res):
        if is_amb(r):
            s["ambiguous"] += 1
            continue
        has, occ = bool(got["has_intersection"][i]), bool(got["completely_occluded"][i])
        if (has, occ) != (r["has"], r["occluded"]):
            s["bad"].append((i, "has / occluded", (has, occ), (r["has"], r["occluded"])))
            continue
        s["partial"] += has and not occ
        s["occluded"] += occ
        op = float(got["combined_opacity"][i])
        ex = max(r["op"][0] - op, op - r["op"][1])
        if not occ:  # (an occluded ray's opacity is 0, its filter is whatever the chain had reached)
            f = got["color_filter"][i].astype(np.float64)
            ex = max(ex, float(np.maximum(r["filt"][0] - f, f - r["filt"][1]).max()))
        ex = np.inf if np.isnan(ex) else ex
        s["worst"] = max(s["worst"], ex)
        if ex > TOL:
            s["bad"].append((i, "opacity / filter", op, r["op"], got["color_filter"][i].tolist()))
    return s


def check_trace(flat, res, o, d, got):
    """got: valid, id, t, rgb of a batch"""
    s = dict(n=len(res), ambiguous=0, hits=0, narrow=0, worst=0.0, worst_t=0.0, bad=[], counts=dict.fromkeys(COUNTERS, 0))
    for i, r in enumerate(res):
        if is_amb(r):
            s["ambiguous"] += 1
            continue
        for k in COUNTERS:
            s["counts"][k] += r["counts"][k]
        if bool(got["valid"][i]) != r["valid"] or int(got["id"][i]) != r["id"]:
            s["bad"].append((i, "valid / id", bool(got["valid"][i]), int(got["id"][i]), r["valid"], r["id"]))
            continue
        if not r["valid"]:
            if np.any(got["rgb"][i] != 0):
                s["bad"].append((i, "rgb of a miss", got["rgb"][i].tolist()))
            continue
        s["hits"] += 1
        dd = d[i].astype(np.float64)
        dd = dd / np.sqrt(dd @ dd)
        p = o[i].astype(np.float64) + dd * r["t"]
        n = fm.norm(p - flat.sphere_center[r["id"]].astype(np.float64)) if r["id"] < flat.n_spheres else \
            flat.tri_normal[r["id"] - flat.n_spheres].astype(np.float64)
        et = abs(float(got["t"][i]) - r["t"]) / _unit_error(flat, o[i], d[i], r["t"], n)
        s["worst_t"] = max(s["worst_t"], et)
        if et > BAR_T:
            s["bad"].append((i, "t", float(got["t"][i]), r["t"], et))
            continue
        obs = got["rgb"][i].astype(np.float64)
        ex = float(np.maximum(r["lo"] - obs, obs - r["hi"]).max())
        ex = np.inf if np.isnan(ex) else ex
        s["worst"] = max(s["worst"], ex)
        s["narrow"] += float((r["hi"] - r["lo"]).max()) < TOL
        if ex > TOL:
            s["bad"].append((i, "rgb", obs.tolist(), r["lo"].tolist(), r["hi"].tolist()))
    return s


def unambiguous(res):
    return np.array([not is_amb(r) for r in res])
