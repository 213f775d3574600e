"""Shared pieces of the radiance-query tests: the test-side reference (tests/trace_rays_ref.c over oracle/rt_oracle.c,
compiled on demand with the oracle's flags) and the comparison the GPU tests apply."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, _abi

import oracle_lib
from ray_query_cases import CFLAGS, HERE, ROOT

COUNTERS = ("rays_primary", "rays_reflection", "rays_refraction", "rays_shadow", "pixels_written")


def build_ref(out_dir) -> C.CDLL:
    so = os.path.join(str(out_dir), "libtrace_rays_ref.so")
    subprocess.check_call(["gcc", *CFLAGS, "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-o", so,
                           os.path.join(HERE, "trace_rays_ref.c"), "-lm", "-lpthread"])
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.tr_trace.restype = C.c_int
    lib.tr_trace.argtypes = [C.POINTER(_abi.rt_scene_desc), C.POINTER(_abi.rt_params), C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int]
    return lib


def without_aa(cfg: RenderConfig) -> RenderConfig:
    return RenderConfig(**{**cfg.__dict__, "features": cfg.features - {"anti_aliasing"}})


def ref_trace(lib, flat, cfg, o, d, argb_fill=0, n_threads=None, index=None):
    """The wrapper's answer for rays (o, d) shaded with cfg (its anti-aliasing ignored): dict of rgb, valid, id, t, argb
    and the five counters.  index: the position of each ray in the batch it was sampled from (its light-cloud key)."""
    o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
    n = o.shape[0]
    desc, keep = _abi.make_scene_desc(flat)
    p, keep2 = _abi.make_params(without_aa(cfg))
    out = dict(rgb=np.empty((n, 3), np.float32), valid=np.empty(n, np.uint8), id=np.empty(n, np.int32), t=np.empty(n, np.float32),
               argb=np.full(n, argb_fill, np.uint32))
    cnt = (C.c_uint64 * 5)()
    if n_threads is None:
        n_threads = min(oracle_lib.host_cores(), 16)
    idx = None if index is None else np.ascontiguousarray(index, np.uint32)
    assert idx is None or idx.shape == (n,)
    rc = lib.tr_trace(C.byref(desc), C.byref(p), n, o.ctypes.data, d.ctypes.data, None if idx is None else idx.ctypes.data, out["rgb"].ctypes.data, out["valid"].ctypes.data,
                      out["id"].ctypes.data, out["t"].ctypes.data, out["argb"].ctypes.data, cnt, int(n_threads))
    assert rc == 0, rc
    out["valid"] = out["valid"].astype(bool)
    out["counters"] = dict(zip(COUNTERS, (int(v) for v in cnt)))
    return out


def check_against_ref(got, stats, ref, tol=1e-4, what=""):
    """The bars of tests/test_parity_gpu.py: valid and id equal, t bit-exact, |dRGB| <= tol with no ray excluded,
    counters equal.  Prints every figure before it asserts; a ray over the bar is reported with its index."""
    valid, ids = np.asarray(got.valid, bool), np.asarray(got.id)
    t, rgb = np.asarray(got.t), np.asarray(got.rgb)
    n_valid_diff = int((valid != ref["valid"]).sum())
    n_id_diff = int((ids != ref["id"]).sum())
    n_t_diff = int((t.view(np.uint32) != ref["t"].view(np.uint32)).sum())
    err = np.abs(rgb.astype(np.float64) - ref["rgb"].astype(np.float64)).max(axis=1) if rgb.size else np.zeros(0)
    err = np.where(np.isnan(err), np.inf, err)
    worst = int(err.argmax()) if err.size else -1
    print(f"{what}: n={valid.size} valid share={ref['valid'].mean() if valid.size else 0:.3f} valid diffs={n_valid_diff} id diffs={n_id_diff} "
          f"t bit diffs={n_t_diff} max|dRGB|={err.max() if err.size else 0:.3e} (ray {worst}) over {tol:g}: {int((err > tol).sum())}")
    if stats is not None:
        print(f"{what}: counters gpu={ {k: stats[k] for k in COUNTERS} } ref={ref['counters']} rays_traced={stats['rays_traced']}")
    assert n_valid_diff == 0, np.flatnonzero(valid != ref["valid"])[:10]
    assert n_id_diff == 0, np.flatnonzero(ids != ref["id"])[:10]
    assert n_t_diff == 0, np.flatnonzero(t.view(np.uint32) != ref["t"].view(np.uint32))[:10]
    assert err.size == 0 or err.max() <= tol, (worst, err[worst], rgb[worst], ref["rgb"][worst])
    if stats is not None:
        for k in COUNTERS:
            assert stats[k] == ref["counters"][k], (k, stats[k], ref["counters"][k])
        assert stats["rays_traced"] == sum(ref["counters"][k] for k in COUNTERS[:3])
