"""What rt_cell_prune_kernel removes from the per-cell shadow candidate lists of a scene and what rt_cell_resolve_kernel
makes of the overflowed ones, counted on the GPU.

Packs the scene with the library's own packer under --budget (default 2 GiB: bench.py's, the per-cell lists fit), runs
rt_flags_kernel with lists, reads lists and flags back, runs rt_cell_prune_kernel and reads them back again.  Reports, before
and after pruning: listed slots, non-empty lists, lists emptied, triangle-clear bits gained per light, and the overflowed
lists (more than 8 candidates: left alone by that kernel, the render walks the tree for such a cell).  Then it runs
rt_cell_resolve_kernel with survivor counts and reports the overflowed lists before and after it, a histogram of the
survivors per formerly overflowed list (0, 1-4, 5-8, 9-16, more; and of those above 8: 9-16, 17-24, 25-32, 33-64, more) and the
stage's device time (timed in a run of its own without the counts, as the render launches it: once without and once with the
pool of wide records, whose records it then counts).  Last it runs rt_cell_through_kernel on the final lists (the run with the
pool) and reports, per light: the listed transmissive entries, the entries marked as crossed for certain, the lists whose every
entry is marked, and the stage's device time.  A probe compiled on the fly links against the built librt_hip.so, so the
kernels counted here are the ones that ship.  Prints one JSON line.

    python tools/cell_list_stats.py [--scene semesterbild] [--model text] [--budget BYTES]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, _abi, _lib, sampling, scenes  # noqa: E402

CSRC = os.path.join(ROOT, "hslu_i", "ba_raytracing", "f2501_raytracer_amd", "csrc")
PROBE = r'''
#include <hip/hip_runtime_api.h>
#include <cstring>
#include "rt_cell_through.h"
#include "rt_scene_pack.h"
static RtPackedScene g;
#define TRY(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return 1000 + (int)e_; } while (0)
extern "C" {
const char* probe_error() { return rt_last_error(); }
int probe_pack(const rt_scene_desc* d, uint64_t budget, uint32_t* out) {
  const int rc = rt_pack_scene(d, budget, &g);
  out[0] = g.n_cells, out[1] = g.n_tri_cells, out[2] = g.dev.n_lights, out[3] = g.dev.n_slots;
  return rc;
}
// lists [n_cells][n_lights][8] and flags [n_cells]: raw_* as rt_flags_kernel leaves them, out_* after rt_cell_prune_kernel,
// res_* after rt_cell_resolve_kernel; counts [n_cells][n_lights]: survivors of every formerly overflowed list (capped at 255);
// ms = {resolve with the pool of wide records, prune, resolve as the render launches it without a pool, resolve with counts};
// wide = {records the pool has room for, records asked for, pool bytes}, wide_lists: the lists after the run with the pool
int probe_run(const float* cloud, uint64_t n_floats, const float* f, float eps, uint64_t budget, uint16_t* raw_lists, uint16_t* raw_flags, uint16_t* out_lists,
              uint16_t* out_flags, uint16_t* res_lists, uint16_t* res_flags, uint8_t* counts, float* ms, uint64_t* wide, uint16_t* wide_lists, uint8_t* marks,
              uint32_t* tri_id, float* through_ms) {
  if (!g.n_cells || g.dev.n_lights > 8u || g.dev.n_slots > 65533u) return -100;
  std::vector<float> scaled;
  float ball[4];
  rt_scale_cloud(cloud, n_floats, f, &scaled, ball);
  RtDevParams P{};
  memcpy(P.cloud_centre, ball, 12);
  P.cloud_delta = ball[3], P.eps_distance = eps, P.cand_cap = 64u;
  rt_beam_constants(eps, &P);
  const size_t list_bytes = (size_t)g.n_cells * g.dev.n_lights * 16u, flag_bytes = (size_t)g.n_cells * 2u;
  char* blob = nullptr;
  float* geo = nullptr;
  uint16_t *lists = nullptr, *flags = nullptr;
  hipEvent_t e[3];
  TRY(hipSetDevice(0));
  for (auto& x : e) TRY(hipEventCreate(&x));
  TRY(hipMalloc((void**)&blob, g.blob.size()));
  TRY(hipMalloc((void**)&geo, g.flag_geo.size() * 4));
  TRY(hipMalloc((void**)&lists, list_bytes + 64));
  TRY(hipMalloc((void**)&flags, flag_bytes + 64));
  TRY(hipMemcpy(blob, g.blob.data(), g.blob.size(), hipMemcpyHostToDevice));
  TRY(hipMemcpy(geo, g.flag_geo.data(), g.flag_geo.size() * 4, hipMemcpyHostToDevice));
  TRY(hipMemset(lists, 0xFF, list_bytes));
  TRY(hipMemset(flags, 0, flag_bytes));
  RtDevScene sc = g.dev;
  sc.base = blob;
  P.flag_out = flags, P.flag_geo = (const float4*)geo, P.cell_list_out = lists;
  P.n_cells = g.n_cells, P.n_tri_cells = g.n_tri_cells;
  TRY(hipEventRecord(e[0], nullptr));
  TRY((hipError_t)rt_launch_flags(sc, P, nullptr));
  TRY(hipEventRecord(e[1], nullptr));
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(raw_lists, lists, list_bytes, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(raw_flags, flags, flag_bytes, hipMemcpyDeviceToHost));
  RtCellPruneArgs a{};
  a.flag_geo = geo, a.lists = lists, a.flags = flags;
  a.n_cells = g.n_cells, a.n_tri_cells = g.n_tri_cells;
  memcpy(a.cloud_centre, ball, 12);
  a.beam_delta = P.beam_delta, a.beam_eps_o = P.beam_eps_o;
  a.mode = RT_PRUNE_FULL;
  TRY(hipEventRecord(e[1], nullptr));
  TRY((hipError_t)rt_launch_cell_prune(sc, a, nullptr));
  TRY(hipEventRecord(e[2], nullptr));
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(out_lists, lists, list_bytes, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(out_flags, flags, flag_bytes, hipMemcpyDeviceToHost));
  ms[0] = ms[1] = ms[2] = ms[3] = 0.f;
  TRY(hipEventElapsedTime(&ms[1], e[1], e[2]));
  // the third stage, twice from the same input: as the render launches it (timed), then with survivor counts
  RtCellResolveArgs r{};
  r.cell = a;
  r.eps_push = P.beam_eps_push, r.eps_ulp = P.beam_eps_ulp;
  const size_t used = list_bytes + flag_bytes + g.flag_geo.size() * 4;
  const size_t temp = rt_cell_resolve_temp_bytes(g.n_cells, budget > used ? budget - used : 0, &r.chunk_cells);
  if (!temp) return -101;
  uint8_t* dcounts = nullptr;
  TRY(hipMalloc((void**)&r.work, temp));
  TRY(hipMalloc((void**)&dcounts, (size_t)g.n_cells * g.dev.n_lights + 64));
  TRY(hipMemset(dcounts, 0, (size_t)g.n_cells * g.dev.n_lights));
  for (int pass = 0; pass < 2; pass++) {
    TRY(hipMemcpy(lists, out_lists, list_bytes, hipMemcpyHostToDevice));
    TRY(hipMemcpy(flags, out_flags, flag_bytes, hipMemcpyHostToDevice));
    r.counts = pass ? dcounts : nullptr;
    TRY(hipEventRecord(e[1], nullptr));
    TRY((hipError_t)rt_launch_cell_resolve(sc, r, nullptr));
    TRY(hipEventRecord(e[2], nullptr));
    TRY(hipDeviceSynchronize());
    TRY(hipEventElapsedTime(&ms[2 + pass], e[1], e[2]));
  }
  TRY(hipMemcpy(res_lists, lists, list_bytes, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(res_flags, flags, flag_bytes, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(counts, dcounts, (size_t)g.n_cells * g.dev.n_lights, hipMemcpyDeviceToHost));
  // ... and a third time with the pool of wide records, sized as the render sizes it
  wide[0] = wide[1] = wide[2] = 0;
  uint32_t cap = 0;
  const size_t pool_bytes = budget > used + temp ? rt_cell_wide_pool_bytes(g.n_cells, g.dev.n_lights, budget - used - temp, &cap) : 0;
  if (pool_bytes) {
    char* pool = nullptr;
    TRY(hipMalloc((void**)&pool, pool_bytes));
    TRY(hipMemcpy(lists, out_lists, list_bytes, hipMemcpyHostToDevice));
    TRY(hipMemcpy(flags, out_flags, flag_bytes, hipMemcpyHostToDevice));
    r.counts = nullptr, r.wide = (uint16_t*)pool, r.wide_cap = cap, r.wide_count = (uint32_t*)(pool + (size_t)cap * 2u * RT_CELL_WIDE_SLOTS);
    TRY(hipEventRecord(e[1], nullptr));
    TRY((hipError_t)rt_launch_cell_resolve(sc, r, nullptr));
    TRY(hipEventRecord(e[2], nullptr));
    TRY(hipDeviceSynchronize());
    TRY(hipEventElapsedTime(&ms[0], e[1], e[2]));
    uint32_t asked = 0;
    TRY(hipMemcpy(&asked, r.wide_count, 4, hipMemcpyDeviceToHost));
    TRY(hipMemcpy(wide_lists, lists, list_bytes, hipMemcpyDeviceToHost));
    wide[0] = cap, wide[1] = asked, wide[2] = pool_bytes;
    TRY(hipFree(pool));
  } else {
    TRY(hipMemcpy(wide_lists, lists, list_bytes, hipMemcpyDeviceToHost));
  }
  // the fourth stage on the final lists: marks[n_cells * n_lights], backwards from the end (rt_cell_through.h)
  {
    const size_t n_marks = (size_t)g.n_cells * g.dev.n_lights;
    uint8_t* dmarks = nullptr;
    TRY(hipMalloc((void**)&dmarks, n_marks + 64));
    RtCellThroughArgs t{};
    t.cell = a;
    t.marks_end = dmarks + n_marks;
    TRY(hipEventRecord(e[1], nullptr));
    TRY((hipError_t)rt_launch_cell_through(sc, t, nullptr));
    TRY(hipEventRecord(e[2], nullptr));
    TRY(hipDeviceSynchronize());
    TRY(hipEventElapsedTime(through_ms, e[1], e[2]));
    TRY(hipMemcpy(marks, dmarks, n_marks, hipMemcpyDeviceToHost));
    TRY(hipFree(dmarks));
    memcpy(tri_id, g.blob.data() + g.dev.off_tri_id, 4u * (size_t)g.dev.n_slots);
  }
  TRY(hipFree(r.work));
  TRY(hipFree(dcounts));
  TRY(hipFree(blob));
  TRY(hipFree(geo));
  TRY(hipFree(lists));
  TRY(hipFree(flags));
  return 0;
}
}
'''


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def resolve_report(over, new_l, res_l, new_f, res_f, counts, nl):
    """rt_cell_resolve_kernel: overflowed lists before and after, survivors per formerly overflowed list, what else changed"""
    still = res_l[:, :, 0] == 0xFFFE
    n = counts[over]
    same = (new_l == res_l).all(2)
    return {"overflowed_lists_before": int(over.sum()), "overflowed_lists_after": int(still.sum()),
            "cells_with_an_overflowed_list_before": int(over.any(1).sum()), "cells_with_an_overflowed_list_after": int(still.any(1).sum()),
            "overflowed_lists_after_per_light": [int(v) for v in still.sum(0)],
            "survivors_per_formerly_overflowed_list": {"0": int((n == 0).sum()), "1-4": int(((n >= 1) & (n <= 4)).sum()), "5-8": int(((n >= 5) & (n <= 8)).sum()),
                                                       "9-16": int(((n >= 9) & (n <= 16)).sum()), ">16": int((n > 16).sum())},
            # (the counts saturate at 255: every bin below is exact)
            "survivors_of_the_lists_still_overflowed": {"9-16": int(((n >= 9) & (n <= 16)).sum()), "17-24": int(((n >= 17) & (n <= 24)).sum()),
                                                        "25-32": int(((n >= 25) & (n <= 32)).sum()), "33-64": int(((n >= 33) & (n <= 64)).sum()),
                                                        ">64": int((n > 64).sum())},
            "slots_listed_by_the_stage": int(((res_l < 0xFFFE) & (over & ~still)[:, :, None]).sum()),
            "clear_bits_gained_per_light": [int((((res_f & ~new_f) >> l) & 1).sum()) for l in range(nl)],
            "lists_that_were_not_overflowed_and_changed": int((~same & ~over).sum()),
            "resolved_lists_that_disagree_with_their_count": int(((counts <= 8) & over & still).sum() + ((counts > 8) & over & ~still).sum())}


def through_of(lists, marks, transmissive, ms):
    """rt_cell_through_kernel on the final lists: per light, the listed transmissive entries, the marked ones, the short lists
    with an entry, and those of them whose every entry is marked (the sets that could go without so and tmax)"""
    out = {"stage_ms": ms, "table_bytes": int(marks.size)}
    rows = {k: [] for k in ("short_lists_with_an_entry", "listed_entries", "listed_transmissive_entries", "marked_entries", "marked_share_of_transmissive",
                            "lists_whose_every_entry_is_marked")}
    shifts = np.arange(8, dtype=np.uint8)[None, :]
    for l in range(lists.shape[1]):  # (light by light: the index arrays of a whole scene are large)
        w = lists[:, l, :]
        entry = (w < 0xFFFE) & (w[:, :1] < 0xFFFE)
        trans = entry & transmissive[np.minimum(w, len(transmissive) - 1)]
        bits = ((marks[:, l, None] >> shifts) & 1).astype(bool)
        assert not (bits & ~trans).any(), "only listed transmissive entries are marked"
        n_entry, n_bits = entry.sum(1), bits.sum(1)
        for k, v in zip(rows, (int((n_entry > 0).sum()), int(n_entry.sum()), int(trans.sum()), int(n_bits.sum()), float(n_bits.sum() / max(1, trans.sum())),
                               int(((n_entry > 0) & (n_bits == n_entry)).sum()))):
            rows[k].append(v)
    out.update({k + "_per_light": v for k, v in rows.items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="semesterbild", choices=["semesterbild", "test_scene"])
    ap.add_argument("--model", default="text")
    ap.add_argument("--budget", type=int, default=2 << 30)
    args = ap.parse_args()
    cfg = RenderConfig.from_features(["high_resolution", "anti_aliasing", "soft_shadows"])  # bench.py's c3
    flat = (scenes.semesterbild(cfg, args.model) if args.scene == "semesterbild" else scenes.test_scene(cfg)).flatten().contiguous()
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    with tempfile.TemporaryDirectory() as d:
        src, so = os.path.join(d, "probe.cpp"), os.path.join(d, "probe.so")
        with open(src, "w") as fh:
            fh.write(PROBE)
        lib_dir, lib_name = os.path.split(os.path.abspath(_lib.LIB_PATH))
        subprocess.run([hipcc, "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip", "--cuda-host-only", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                        "-shared", "-o", so, src, "-L", lib_dir, f"-l:{lib_name}", f"-Wl,-rpath,{lib_dir}"], check=True)
        probe = C.CDLL(so)
    probe.probe_error.restype = C.c_char_p
    desc, keep = _abi.make_scene_desc(flat)
    out = np.zeros(4, np.uint32)
    rc = probe.probe_pack(C.byref(desc), C.c_uint64(args.budget), ptr(out))
    assert rc == 0, probe.probe_error()
    n_cells, n_tri_cells, nl, ns = (int(v) for v in out)
    cs = np.ascontiguousarray(sampling.cloud_sets(cfg), np.float32)
    f = np.array([cfg.fw, cfg.fh, cfg.fd], np.float32)
    raw_l, new_l, res_l = (np.zeros((n_cells, nl, 8), np.uint16) for _ in range(3))
    raw_f, new_f, res_f = (np.zeros(n_cells, np.uint16) for _ in range(3))
    counts = np.zeros((n_cells, nl), np.uint8)
    ms = np.zeros(4, np.float32)
    wide, wide_l = np.zeros(3, np.uint64), np.zeros((n_cells, nl, 8), np.uint16)
    marks, tri_id, through_ms = np.zeros(n_cells * nl, np.uint8), np.zeros(ns, np.uint32), np.zeros(1, np.float32)
    rc = probe.probe_run(ptr(cs), C.c_uint64(cs.size), ptr(f), C.c_float(cfg.eps_distance), C.c_uint64(args.budget), ptr(raw_l), ptr(raw_f), ptr(new_l), ptr(new_f),
                         ptr(res_l), ptr(res_f), ptr(counts), ptr(ms), ptr(wide), ptr(wide_l), ptr(marks), ptr(tri_id), ptr(through_ms))
    assert rc == 0, f"probe_run: {rc}"
    through_report = through_of(wide_l, marks[::-1].reshape(n_cells, nl), (tri_id & 0x40000000) != 0, float(through_ms[0]))
    marked = (wide_l[:, :, 0] == 0xFFFE) & (wide_l[:, :, 1] == 0xFFFD)
    wide_report = {"pool_records": int(wide[0]), "records_asked_for": int(wide[1]), "pool_bytes": int(wide[2]), "wide_lists": int(marked.sum()),
                   "wide_lists_per_light": [int(v) for v in marked.sum(0)], "plain_overflowed_lists_left": int(((wide_l[:, :, 0] == 0xFFFE) & ~marked).sum()),
                   "lists_without_a_record_that_differ": int((~marked & (wide_l != res_l).any(2)).sum()), "resolve_stage_with_pool_ms": float(ms[0])}
    over = raw_l[:, :, 0] == 0xFFFE
    usable = ~over

    def count(lists, flags):
        listed = (lists < 0xFFFE) & usable[:, :, None]
        per_list = listed.sum(2)
        return {"listed_slots": int(listed.sum()), "non_empty_lists": int((per_list > 0).sum()),
                "mean_slots_per_non_empty_list": float(listed.sum() / max(1, (per_list > 0).sum())),
                "histogram_slots_per_list": [int((per_list[usable] == k).sum()) for k in range(9)],
                "triangle_clear_bits_per_light": [int(((flags >> l) & 1).sum()) for l in range(nl)]}
    before, after = count(raw_l, raw_f), count(new_l, new_f)
    emptied = ((raw_l[:, :, 0] < 0xFFFE) & (new_l[:, :, 0] == 0xFFFF)).sum(0)
    res = {"scene": args.scene, "model": args.model, "budget": args.budget, "n_cells": n_cells, "n_tri_cells": n_tri_cells, "n_lights": nl, "n_slots": ns,
           "overflowed_lists_left_alone": int(over.sum()), "overflowed_lists_per_light": [int(v) for v in over.sum(0)],
           "cells_with_an_overflowed_list": int(over.any(1).sum()), "before": before, "after": after,
           "lists_emptied_per_light": [int(v) for v in emptied],
           "clear_bits_gained_per_light": [a - b for a, b in zip(after["triangle_clear_bits_per_light"], before["triangle_clear_bits_per_light"])],
           "slots_removed": before["listed_slots"] - after["listed_slots"],
           "slots_removed_fraction": (before["listed_slots"] - after["listed_slots"]) / max(1, before["listed_slots"]),
           "prune_kernel_ms": float(ms[1]),
           "resolve": resolve_report(over, new_l, res_l, new_f, res_f, counts, nl), "resolve_stage_ms": float(ms[2]), "resolve_stage_with_counts_ms": float(ms[3]),
           "wide": wide_report, "through": through_report,
           "build_id": _lib.load().rt_build_id().decode()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
