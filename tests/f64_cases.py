"""Cases and checks shared by test_f64_model_soft_shadows.py (CPU) and test_f64_model_gpu.py: the synthetic scenes at
config-3 and config-4 features, the sampled pixels of the at-spec config-3 windows, the float64 model's per-pixel
intervals for them (computed in worker processes) and the interval check of an observed frame."""
from __future__ import annotations

import functools
import multiprocessing

import numpy as np

import f64_model as fm
import oracle_lib
from f64_model import TOL, Model, build_scene
from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig

SYN_W, SYN_H = 48, 40
# synthetic cases: features, depth.  c3 = AA (plain table) + soft shadows; c3rand = the anti_aliasing_randomness table;
# c4 = reflections + refractions, 24 spp, 28 cloud points per light, depth 3 and 8; c3cull / c4d3cull = c3 / c4d3 with
# back-face culling, on the scene that has something to cull
SYN_CASES = {
    "c3": (["anti_aliasing", "soft_shadows"], None),
    "c3rand": (["anti_aliasing_randomness", "soft_shadows"], None),
    "c4d3": (["realistic", "extreme_quality"], 3),
    "c4d8": (["realistic", "extreme_quality"], 8),
    "c3cull": (["anti_aliasing", "soft_shadows", "backface_culling"], None),
    "c4d3cull": (["realistic", "extreme_quality", "backface_culling"], 3),
}
SPEC_NAMES = ("spec_c3", "spec_c3lowres")
SPEC_PER_WINDOW = 12  # 48 fixed pixels over the four windows


def syn_workload(key):
    feats, depth = SYN_CASES[key]
    cfg = RenderConfig.from_features(feats, width_override=SYN_W, height_override=SYN_H, depth_override=depth,
                                     n_cloud_sets=64)
    return cfg, build_scene(cfg, soft=True, cull=cfg.has("backface_culling"))


def syn_pixels():
    """a fixed lattice over the frame: every 9th pixel"""
    return [(gx, gy) for gy in range(1, SYN_H, 3) for gx in range((gy // 3) % 3, SYN_W, 3)]


def spec_pixels(win):
    """SPEC_PER_WINDOW fixed pixels of one window (x0, y0, w, h): a 4 x 3 lattice"""
    x0, y0, w, h = win
    return [(x0 + (2 * i + 1) * w // 8, y0 + (2 * j + 1) * h // 6) for j in range(3) for i in range(4)]


def spec_planes(cfg, meta, z):
    """the fixture's windows as full-frame rgb / hit_id / hit_t planes (hit id -2 outside the windows)"""
    n = cfg.width * cfg.height
    rgb, hid, ht = np.zeros((n, 3), np.float32), np.full(n, -2, np.int32), np.zeros(n, np.float32)
    for i, (x0, y0, w, h) in enumerate(meta["windows"]):
        idx = (np.arange(y0, y0 + h)[:, None] * cfg.width + np.arange(x0, x0 + w)[None]).ravel()
        rgb[idx], hid[idx], ht[idx] = z[f"w{i}_rgb"].reshape(-1, 3), z[f"w{i}_hit_id"].ravel(), z[f"w{i}_hit_t"].ravel()
    return rgb, hid, ht


def spec_workload(name):
    import bench
    from test_oracle_golden import make_spec_golden

    meta, z = make_spec_golden.load(name)
    cfg, flat, _ = bench.build_workload(meta["workload"])
    return cfg, flat, meta, z


def n_procs():
    return max(1, min(oracle_lib.host_cores(), 16))


# ---- model evaluation in worker processes -------------------------------------------------------------------------
_W = {}


def _init(kind, key, kw):
    cfg, flat = syn_workload(key) if kind == "syn" else key if kind == "scene" else spec_workload(key)[:2]
    _W["m"] = Model(flat, cfg, **kw)


def _eval(px):
    m = _W["m"]
    out = []
    for gx, gy in px:
        try:
            r = m.render_pixel(gx, gy)
        except fm.Ambiguous as e:
            out.append(dict(px=(gx, gy), amb=str(e)))
            continue
        pen = False
        if r["reach"] is not None and m.N > 1:
            c = np.asarray(r["reach"]).reshape(-1, m.N).sum(axis=1)
            pen = bool(((c > 0) & (c < m.N)).any())
        iv = r["iv"]
        out.append(dict(px=(gx, gy), amb=None, id=r["id"], t=r["t"], written=r["written"],
                        lo=None if iv is None else iv.lo, hi=None if iv is None else iv.hi, nom=None if iv is None else iv.nom,
                        pen=pen))
    return out


def _count(rows):
    m = _W["m"]
    tot = {}
    for gy in rows:
        c = m.count_frame((0, gy, m.cfg.width, 1))
        for k, v in c.items():
            tot[k] = tot.get(k, 0) + v
    return tot


def _pool(kind, key, kw):
    # spawned, not forked: the GPU tests call this after the parent has opened the device, and CPU-only workers must not
    # inherit it
    return multiprocessing.get_context("spawn").Pool(n_procs(), initializer=_init, initargs=(kind, key, kw))


@functools.lru_cache(maxsize=None)
def syn_intervals(key):
    return model_intervals("syn", key, syn_pixels())


@functools.lru_cache(maxsize=None)
def spec_intervals(name):
    meta = spec_workload(name)[2]
    return model_intervals("spec", name, [p for w in meta["windows"] for p in spec_pixels(w)])


def model_intervals(kind, key, pixels, **kw):
    """float64 intervals of `pixels` ([(gx, gy)]) of a synthetic case (kind "syn"), an at-spec workload ("spec") or any
    scene (kind "scene", key = (cfg, flat)); kw goes to the Model"""
    chunks = [pixels[i::n_procs() * 4] for i in range(n_procs() * 4)]
    with _pool(kind, key, kw) as p:
        res = [r for part in p.map(_eval, [c for c in chunks if c]) for r in part]
    return sorted(res, key=lambda r: (r["px"][1], r["px"][0]))


@functools.lru_cache(maxsize=None)
def model_counts(key, **kw):
    """the synthetic case's full-frame ray counters and written pixels"""
    return _counts("syn", key, kw)


def scene_counts(cfg, flat, **kw):
    """the same for any scene at the synthetic frame size"""
    assert (cfg.width, cfg.height) == (SYN_W, SYN_H)
    return _counts("scene", (cfg, flat), kw)


def _counts(kind, key, kw):
    rows = list(range(SYN_H))
    with _pool(kind, key, kw) as p:
        parts = p.map(_count, [rows[i::n_procs()] for i in range(n_procs())])
    tot = {}
    for c in parts:
        for k, v in c.items():
            tot[k] = tot.get(k, 0) + v
    return tot


# ---- the check --------------------------------------------------------------------------------------------------
def check(res, width, rgb, hit_id, hit_t, t_rel=None):
    """Compare an observed frame (full-frame planes, row-major over `width`) with the model's intervals.
    Returns a summary; `bad` lists the pixels outside their interval or with another hit id / t."""
    n, amb, narrow, pen, worst, bad = len(res), 0, 0, 0, 0.0, []
    for r in res:
        if r["amb"] is not None:
            amb += 1
            continue
        gx, gy = r["px"]
        i = gy * width + gx
        if int(hit_id[i]) != r["id"]:
            bad.append((r["px"], "hit id", int(hit_id[i]), r["id"]))
            continue
        if t_rel is not None and r["id"] >= 0 and not abs(float(hit_t[i]) - r["t"]) <= t_rel * abs(r["t"]):
            bad.append((r["px"], "t", float(hit_t[i]), r["t"]))
            continue
        lo = np.zeros(3) if r["lo"] is None else r["lo"]
        hi = np.zeros(3) if r["hi"] is None else r["hi"]
        obs = np.asarray(rgb[i], np.float64)
        # a non-finite value never passes: NaN > TOL is false, so it is rejected by name and not by the comparison
        if not np.all(np.isfinite(obs)):
            bad.append((r["px"], "non-finite rgb", obs.tolist()))
            continue
        if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
            bad.append((r["px"], "non-finite model bound", lo.tolist(), hi.tolist()))
            continue
        ex = float(np.maximum(lo - obs, obs - hi).max())
        worst = max(worst, ex)
        narrow += float((hi - lo).max()) < TOL
        pen += r["pen"]
        if ex > TOL:
            bad.append((r["px"], "rgb", obs.tolist(), lo.tolist(), hi.tolist()))
    return dict(n=n, ambiguous=amb, narrow=narrow, penumbra=pen, worst=worst, bad=bad)


def assert_guards(name, s, penumbra=True):
    """the intervals must be informative: >= 80 % narrower than TOL, <= 10 % ambiguous, >= a third in penumbra (the
    synthetic scenes; the at-spec windows hold about one penumbra pixel in 800 at 10 cloud points of 2.2 pixels)"""
    print(f"{name}: {s['n']} pixels, worst excess over the interval {s['worst']:.2e} (tol {TOL:g}), "
          f"narrow {s['narrow']}/{s['n']}, ambiguous {s['ambiguous']}, penumbra {s['penumbra']}, outside {len(s['bad'])}")
    assert s["narrow"] >= 0.8 * s["n"], s
    assert s["ambiguous"] <= 0.1 * s["n"], s
    if penumbra:
        assert s["penumbra"] * 3 >= s["n"], s
