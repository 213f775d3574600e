"""Wide records of the per-cell shadow candidate lists on the GPU (csrc/rt_cell_resolve.hip writes them, the list-union block of
process_ray in csrc/rt_kernels.hip reads them): the device writes what the host model writes, and no frame changes.

1. Words.  The probe pattern of test_cell_resolve_gpu.py with a pool: rt_flags_kernel, rt_cell_prune_kernel, read back,
   rt_cell_resolve_kernel with a pool of wide records, read back; rt_cell_resolve_packed with a pool of its own on the copy
   read back after stage two.  Which record a list gets depends on the order of the device's atomics, so the lists are
   compared word for word where neither side has a record, and where one has, both have, and the records hold the same
   slots.  Flags word for word.  At most 4096 cells; one run goes chunk by chunk (work_cells=300), one has a pool of five.
2. Frames.  Soft shadows x 10 on a 64 x 64 window over three fans of panes that stand beside the camera's view, between the
   receivers and a light off to the side: "wide" (12 panes over every receiver cell: wavefronts of one cell with a record, and
   of neighbouring cells whose records share their slots), "mixed" (40 panes that reach differently far down, so that the
   receiver's rows of cells keep from none to all 40 of them: records beside plain overflowed lists and beside short
   lists) and "corner" (four receivers at four depths that meet in one pixel, each under 18 panes of its own: a union of 72
   slots).  Every frame is, packed pixels and float planes bit for bit, the same with the records, with RT_CELL_WIDE=0 and
   with tuning.no_cell_lists; RT_CELL_WIDE is read once per process, so each arm renders in a child process of its own.
   The host model, on the scene packed as the render packs it, then says for the cells under the rendered pixels
   (flags_cases.receiver_cell, float32) that the cases are there: hit points in cells with a record whose light is above
   their horizon; neighbouring pixels in different cells with records that share slots; a record next to a list of more
   than 32; four cells with records around one pixel corner whose union exceeds 64."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import test_cell_prune_gpu as pg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
W, MARK, END, OVERFLOW = 32, 0xFFFD, 0xFFFF, 0xFFFE

PROBE = r'''
#include <hip/hip_runtime_api.h>
#include <cstring>
#include "rt_cell_resolve.h"
#include "rt_scene_pack.h"
static RtPackedScene g;
static int dead = 0;  // the first HIP error, sticky: nothing further is started on the device after it
#define TRY(x)                                                 \
  do {                                                         \
    const hipError_t e_ = (x);                                 \
    if (e_ != hipSuccess) return dead = 1000 + (int)e_;        \
  } while (0)
extern "C" {
const char* probe_error() { return rt_last_error(); }
int probe_pack(const rt_scene_desc* d, uint64_t budget, uint32_t* out) {
  const int rc = rt_pack_scene(d, budget, &g);
  out[0] = g.n_cells, out[1] = g.n_tri_cells, out[2] = g.dev.n_lights, out[3] = g.dev.n_slots;
  return rc;
}
// the three stages on the device, the third with a pool of `cap` wide records; host_*: rt_cell_resolve_packed with a pool of
// the same size on the lists read back after stage two.  pools: [cap][32]; asked[2]: records asked for on the device, on the host
int probe_run(const float* cloud, uint64_t n_floats, const float* f, float eps, uint32_t work_cells, uint32_t cap, uint16_t* two_lists, uint16_t* dev_lists,
              uint16_t* dev_flags, uint16_t* dev_pool, uint16_t* host_lists, uint16_t* host_flags, uint16_t* host_pool, uint32_t* asked) {
  if (dead) return dead;
  if (!g.n_cells || g.dev.n_lights > 8u || g.dev.n_slots > 65533u || cap == 0u) return -100;
  std::vector<float> scaled;
  float ball[4];
  rt_scale_cloud(cloud, n_floats, f, &scaled, ball);
  RtDevParams P{};
  memcpy(P.cloud_centre, ball, 12);
  P.cloud_delta = ball[3];
  P.eps_distance = eps;
  rt_beam_constants(eps, &P);
  P.cand_cap = 64u;
  const size_t list_bytes = (size_t)g.n_cells * g.dev.n_lights * 16u, flag_bytes = (size_t)g.n_cells * 2u, pool_bytes = (size_t)cap * 2u * RT_CELL_WIDE_SLOTS;
  RtCellResolveArgs r{};
  const size_t temp = rt_cell_resolve_temp_bytes(g.n_cells, work_cells ? 4096u + 4u * (size_t)work_cells : (size_t)64u << 20, &r.chunk_cells);
  if (!temp || (work_cells && r.chunk_cells != (work_cells < g.n_cells ? work_cells : g.n_cells))) return -101;
  char *blob = nullptr, *pool = nullptr;
  float* geo = nullptr;
  uint16_t *lists = nullptr, *flags = nullptr;
  uint32_t* work = nullptr;
  TRY(hipSetDevice(0));
  TRY(hipMalloc((void**)&blob, g.blob.size()));
  TRY(hipMalloc((void**)&geo, g.flag_geo.size() * 4));
  TRY(hipMalloc((void**)&lists, list_bytes + 64));
  TRY(hipMalloc((void**)&flags, flag_bytes + 64));
  TRY(hipMalloc((void**)&work, temp));
  TRY(hipMalloc((void**)&pool, pool_bytes + 64));
  TRY(hipMemcpy(blob, g.blob.data(), g.blob.size(), hipMemcpyHostToDevice));
  TRY(hipMemcpy(geo, g.flag_geo.data(), g.flag_geo.size() * 4, hipMemcpyHostToDevice));
  TRY(hipMemset(lists, 0xFF, list_bytes));
  TRY(hipMemset(flags, 0, flag_bytes));
  TRY(hipMemset(pool, 0xAB, pool_bytes + 64));  // (the stage clears the counter itself)
  RtDevScene sc = g.dev;
  sc.base = blob;
  P.flag_out = flags, P.flag_geo = (const float4*)geo, P.cell_list_out = lists;
  P.n_cells = g.n_cells, P.n_tri_cells = g.n_tri_cells;
  TRY((hipError_t)rt_launch_flags(sc, P, nullptr));
  RtCellPruneArgs a{};
  a.flag_geo = geo, a.lists = lists, a.flags = flags;
  a.n_cells = g.n_cells, a.n_tri_cells = g.n_tri_cells;
  memcpy(a.cloud_centre, ball, 12);
  a.beam_delta = P.beam_delta, a.beam_eps_o = P.beam_eps_o;
  a.mode = RT_PRUNE_FULL;
  TRY((hipError_t)rt_launch_cell_prune(sc, a, nullptr));
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(two_lists, lists, list_bytes, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(host_flags, flags, flag_bytes, hipMemcpyDeviceToHost));
  r.cell = a;
  r.eps_push = P.beam_eps_push, r.eps_ulp = P.beam_eps_ulp;
  r.work = work, r.wide = (uint16_t*)pool, r.wide_cap = cap, r.wide_count = (uint32_t*)(pool + pool_bytes);
  TRY((hipError_t)rt_launch_cell_resolve(sc, r, nullptr));
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(dev_lists, lists, list_bytes, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(dev_flags, flags, flag_bytes, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(dev_pool, pool, pool_bytes, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(&asked[0], pool + pool_bytes, 4, hipMemcpyDeviceToHost));
  memcpy(host_lists, two_lists, list_bytes);
  asked[1] = 0u;
  r.cell.lists = host_lists, r.cell.flags = host_flags, r.work = nullptr, r.wide = host_pool, r.wide_count = &asked[1];
  rt_cell_resolve_packed(g, r);
  TRY(hipFree(blob));
  TRY(hipFree(geo));
  TRY(hipFree(lists));
  TRY(hipFree(flags));
  TRY(hipFree(work));
  TRY(hipFree(pool));
  return 0;
}
}
'''


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    from test_scene_pack_host import CSRC, HIPCC
    from hslu_i.ba_raytracing.f2501_raytracer_amd import _lib
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("cell_wide_gpu_probe")
    src = d / "probe.cpp"
    src.write_text(PROBE)
    so = d / "probe.so"
    lib_dir, lib_name = os.path.split(os.path.abspath(_lib.LIB_PATH))
    out = subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip", "--cuda-host-only", "-I", CSRC,
                          "-I", os.path.join(ROOT, "include"), "-shared", "-o", str(so), str(src),
                          "-L", lib_dir, f"-l:{lib_name}", f"-Wl,-rpath,{lib_dir}"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lib = C.CDLL(str(so))
    lib.probe_error.restype = C.c_char_p
    return lib


def wide_of(lists, pool, n_slots):
    """{(cell, light): frozenset(slots)} of the lists that carry the mark, the record's form checked on the way"""
    out, seen = {}, set()
    for c, l in zip(*np.nonzero((lists[:, :, 0] == OVERFLOW) & (lists[:, :, 1] == MARK))):
        w = lists[c, l]
        at = int(w[2]) | (int(w[3]) << 15)
        assert w[2] < 0x8000 and w[3] < 0x8000 and list(w[4:]) == [END] * 4 and at < len(pool) and at not in seen, (c, l, w)
        seen.add(at)
        rec = pool[at]
        n = int((rec != END).sum())
        assert 8 < n <= W and (rec[:n] < n_slots).all() and (rec[n:] == END).all() and len(set(rec[:n].tolist())) == n, (c, l, rec)
        out[int(c), int(l)] = frozenset(rec[:n].tolist())
    return out


# ---- 1. words ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name, work_cells, cap", [("fan_between", 0, 0), ("fan_32", 0, 0), ("fan_33", 0, 0), ("fan_mixed", 0, 0), ("semesterbild", 0, 0),
                                                   ("semesterbild", 300, 0), ("fan_between", 0, 5)])
def test_kernel_writes_the_host_models_lists_and_records(probe, name, work_cells, cap):
    import flags_cases
    import test_cell_wide_host as wh
    from test_scene_pack_host import ptr
    from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, sampling
    cfg, flat, _ = wh.host.CASES[name]()
    desc, keep = _abi.make_scene_desc(flat)
    out = np.zeros(4, np.uint32)
    budget = 48 * flat.n_triangles + 8192  # the flags' input and at most 4096 cells
    assert probe.probe_pack(C.byref(desc), C.c_uint64(budget), ptr(out)) == 0, probe.probe_error()
    n_cells, n_tri_cells, nl, ns = (int(v) for v in out)
    assert 0 < n_cells <= 4096
    cs = np.ascontiguousarray(sampling.cloud_sets(cfg), np.float32)
    f = np.array([cfg.fw, cfg.fh, cfg.fd], np.float32)

    def run(pool_cap):
        two_l, dev_l, host_l = (np.zeros((n_cells, nl, 8), np.uint16) for _ in range(3))
        dev_f, host_f = np.zeros(n_cells, np.uint16), np.zeros(n_cells, np.uint16)
        dev_p, host_p = np.zeros((pool_cap, W), np.uint16), wh.new_pool(pool_cap)
        asked = np.zeros(2, np.uint32)
        rc = probe.probe_run(ptr(cs), C.c_uint64(cs.size), ptr(f), C.c_float(cfg.eps_distance), C.c_uint32(work_cells), C.c_uint32(pool_cap), ptr(two_l), ptr(dev_l),
                             ptr(dev_f), ptr(dev_p), ptr(host_l), ptr(host_f), ptr(host_p), ptr(asked))
        assert rc == 0, f"probe_run: {rc}"
        return two_l, dev_l, dev_f, wide_of(dev_l, dev_p, ns), host_l, host_f, wide_of(host_l, host_p, ns), asked

    two_l, dev_l, dev_f, dev_w, host_l, host_f, host_w, asked = run(n_cells * nl)
    over2 = two_l[:, :, 0] == OVERFLOW
    print(f"{name}: {n_cells} cells, {nl} lights, work list of {work_cells or 'all'} cells; overflowed lists {int(over2.sum())} -> "
          f"{int((dev_l[:, :, 0] == OVERFLOW).sum())}, of them with a record {len(dev_w)} (host model {len(host_w)}); records asked for {asked.tolist()}")
    assert np.array_equal(dev_f, host_f), f"{int((dev_f != host_f).sum())} flag words differ"
    flags_cases.check_shape(dev_l, None, ns)
    assert np.array_equal(dev_l[~over2], two_l[~over2]), "a list that is not overflowed is not touched"
    assert asked[0] == asked[1] == len(dev_w) and set(dev_w) == set(host_w), "the same lists get a record"
    assert all(dev_w[k] == host_w[k] for k in dev_w), "the records hold the same slots"
    plain = np.ones(dev_l.shape[:2], bool)
    for c, l in dev_w:
        plain[c, l] = False
    assert np.array_equal(dev_l[plain], host_l[plain]), f"{int((dev_l[plain] != host_l[plain]).sum())} list words differ"
    if name not in ("fan_33", "fan_mixed"):
        assert dev_w, "there are wide lists here"
    if cap:  # a pool that runs out: which lists get its records is the atomics' business; every record is the right one
        assert cap < len(host_w)
        _, few_l, few_f, few_w, _, _, host_few, few_asked = run(cap)
        assert len(few_w) == len(host_few) == cap and few_asked[0] == few_asked[1] == len(host_w), "the counter runs on, the pool does not"
        assert all(k in host_w and rec == host_w[k] for k, rec in few_w.items())
        rest = (few_l[:, :, 0] == OVERFLOW) & (few_l[:, :, 1] != MARK)
        assert np.array_equal(few_l[rest], two_l[rest]) and np.array_equal(few_f, dev_f), "a list that found the pool full stays as it was"
        short = few_l[:, :, 0] != OVERFLOW
        assert np.array_equal(few_l[short], dev_l[short])
    del keep


# ---- 2. frames -----------------------------------------------------------------------------------------------------------------
WIN = (352, 288, 64, 64)
LIGHT = [1.4, 0.41666666, 0.05, 1.0, 0.9, 0.8, 3.0]
FAR = ([5.0, 5.0, 30.0], [0.01, 0.0, 0.0], [0.0, 0.01, 0.0])  # stretches the scene's diagonal: receiver cells of about 0.03


def _scene(quads, panes):
    import dataclasses
    import test_cell_prune_host as host
    flat = host._soup(quads, lights=[LIGHT])
    panes = list(panes) + [FAR]
    v1, e1, e2 = (np.array([p[i] for p in panes], np.float32) for i in range(3))
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    cat = lambda a, b: np.concatenate([a, b.astype(a.dtype)])  # noqa: E731
    return dataclasses.replace(flat, tri_v1=cat(flat.tri_v1, v1), tri_e1=cat(flat.tri_e1, e1), tri_e2=cat(flat.tri_e2, e2), tri_normal=cat(flat.tri_normal, nrm.astype(np.float32)),
                               tri_material=cat(flat.tri_material, np.zeros(len(panes), np.uint32))).contiguous()


def _quad_at(x0, y0, z, w, h):
    """a receiver that faces the camera (normal -z)"""
    return ([x0, y0, z], [0.0, h, 0.0], [w, 0.0, 0.0])


def frame_scenes():
    """name -> flat scene.  The camera looks along +z from the plane z = 0 through the window; the light stands off to the
    side at +x, in front of the receivers; the panes are single triangles in planes x = const beyond the camera's view"""
    big = _quad_at(0.42, 0.33666666, 0.5, 0.16, 0.16)
    wide = [([0.75 + 0.004 * i, 0.28, 0.18], [0.0, 0.5, 0.0], [0.0, 0.0, 0.6]) for i in range(12)]
    mixed = [([0.75 + 0.004 * i, 0.397 + 0.065 * i / 39.0, 0.18], [0.0, 0.5, 0.0], [0.0, 0.0, 0.6]) for i in range(40)]
    cx, cy, depths = 0.5, 0.41666666, (0.5, 0.62, 0.74, 0.86)
    quads = [_quad_at(cx - 0.08, cy - 0.08, depths[0], 0.08, 0.08), _quad_at(cx, cy - 0.08, depths[1], 0.08, 0.08),
             _quad_at(cx - 0.08, cy, depths[2], 0.08, 0.08), _quad_at(cx, cy, depths[3], 0.08, 0.08)]
    corner = []
    for g, zq in enumerate(depths):  # 18 narrow panes per receiver, across the beams from its corner at (cx, cy) alone
        for i in range(18):
            x = 0.75 + 0.027 * g + 0.0015 * i
            s = (x - cx) / (LIGHT[0] - cx)
            corner.append(([x, 0.25, zq - (zq - LIGHT[2]) * s - 0.018], [0.0, 0.4, 0.0], [0.0, 0.0, 0.07]))
    return {"wide": _scene([big], wide), "mixed": _scene([big], mixed), "corner": _scene(quads, corner)}


def frame_cfg():
    from test_cell_prune_host import soft_cfg
    return soft_cfg()  # anti-aliasing and soft shadows x 10, 768 x 640


BUDGET = 64 << 20


def child(out_dir, arm):
    """one process = one arm: the three frames, written to out_dir"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceScene, ImageBuffer, RaytracerRenderer
    cfg = frame_cfg()
    for name, flat in frame_scenes().items():
        ds = DeviceScene(flat, 0, budget=BUDGET)
        r = RaytracerRenderer(cfg, device=0)
        buf = ImageBuffer.new(cfg.width, cfg.height)
        planes = r.render(buf, ds, window=WIN, aux=True, tuning=dict(no_cell_lists=1) if arm == "nolists" else None)
        info = ds.memory_info()
        assert info["cell_lists_built"] == 1, "the lists exist"
        np.savez(os.path.join(out_dir, f"{name}.npz"), argb=np.asarray(buf.buffer), rgb=planes["rgb"], hit_id=planes["hit_id"], hit_t=planes["hit_t"],
                 bytes_cell_lists=info["bytes_cell_lists"])
        ds.close()


def run_child(tmp_path, arm):
    out = tmp_path / arm
    out.mkdir()
    env = dict(os.environ, RT_TRACE_LAUNCHES="1")
    for v in ("RT_CELL_PRUNE", "RT_CELL_RESOLVE", "RT_CELL_WIDE"):
        env.pop(v, None)
    if arm == "off":
        env["RT_CELL_WIDE"] = "0"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), str(out), arm]
    proc = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=pg.CHILD_TIMEOUT_S)
    assert proc.returncode == 0, (cmd, proc.returncode, proc.stderr[-4000:])
    return out, proc.stderr


class Plan:
    """what the host model says about the cells under the pixels of WIN in one of the frame scenes, packed as the render packs it"""

    def __init__(self, host_probe, name, flat, hit_id):
        import flags_cases
        import test_cell_wide_host as wh
        cfg = frame_cfg()
        wh.host.CASES["frame_" + name] = lambda: (cfg, flat, None)
        k = wh.load(host_probe, "frame_" + name, BUDGET)
        self.k = k
        x0, y0, w, h = WIN
        f = np.array([cfg.focus.x, cfg.focus.y, cfg.focus.z], np.float64)
        ns = k.dev["n_spheres"]
        self.cell = np.full((h, w), -1, np.int64)
        for j in range(h):
            for i in range(w):
                prim = int(hit_id[y0 + j, x0 + i])
                if prim < 0:
                    continue
                t = prim - ns
                v1, e1, e2 = (np.asarray(a[t], np.float64) for a in (flat.tri_v1, flat.tri_e1, flat.tri_e2))
                if abs(e1[2]) + abs(e2[2]) > 0:
                    continue  # (a pane: they stand outside the window's view)
                cells = set()
                for dx, dy in ((0.0, 0.0), (-0.45, -0.45), (0.45, -0.45), (-0.45, 0.45), (0.45, 0.45)):  # the centre ray and the reach of the pixel's samples
                    o = np.array([np.float32(x0 + i + dx) * np.float32(cfg.fw), np.float32(y0 + j + dy) * np.float32(cfg.fh), 0.0])
                    p = o + (o - f) * (v1[2] / (o[2] - f[2]))
                    cells.add(flags_cases.receiver_cell(k, prim, p.astype(np.float32)))
                if len(cells) == 1 and None not in cells:
                    self.cell[j, i] = cells.pop()  # every sample of this pixel lies in this cell
        used = sorted(set(self.cell[self.cell >= 0].tolist()))
        lists, _, pool, _ = wh.resolve(host_probe, k, used, cap=len(used) * k.dev["n_lights"])
        recs = wh.records(host_probe, lists, pool, k.dev["n_slots"])
        self.kept = {c: frozenset(np.nonzero(wh.kept_of(host_probe, k, c)[0])[0].tolist()) for c in used}
        self.wide = {used[i]: frozenset(r) for (i, l), r in recs.items() if l == 0}
        self.above = set()  # cells whose light is above the horizon: the receivers face -z and the light stands in front of them
        for c in used:
            pm, _ = wh.host.hull_of(host_probe, c)
            if LIGHT[2] < pm[2]:
                self.above.add(c)

    def neighbours(self):
        """pairs of different cells under pixels one or two apart in a row or a column (a pixel between two cells has samples
        in both and carries no cell here: the wavefront of its samples is where the two meet)"""
        c = self.cell
        out = set()
        for d in (1, 2):
            for a, b in ((c[:, :-d], c[:, d:]), (c[:-d, :], c[d:, :])):
                m = (a >= 0) & (b >= 0) & (a != b)
                out |= set(zip(a[m].tolist(), b[m].tolist()))
        return out

    def corners(self):
        """the cells at the four corners of every 3 x 3 block of pixels"""
        c = self.cell
        blocks = np.stack([c[:-2, :-2], c[:-2, 2:], c[2:, :-2], c[2:, 2:]], -1).reshape(-1, 4)
        return {tuple(sorted(set(b.tolist()))) for b in blocks if (b >= 0).all()}


@pytest.fixture(scope="module")
def host_probe(tmp_path_factory):
    import test_cell_wide_host as wh
    if not os.path.exists(wh.rh.HIPCC):
        pytest.skip("no hipcc")
    lib = wh.rh.build_probe(tmp_path_factory.mktemp("cell_wide_plan_probe"), wh.PROBE)
    lib.probe_wide_index.restype = lib.probe_resolve_wide.restype = C.c_uint32
    return lib


def check_plan(name, plan):
    """the cases the frames are there for, by the host model"""
    lit = [c for c in plan.wide if c in plan.above]
    assert lit, f"{name}: a rendered hit point lies in a cell with a wide list whose light is above its horizon"
    pairs = plan.neighbours()
    if name == "wide":
        assert any(a in plan.wide and b in plan.wide and plan.wide[a] & plan.wide[b] for a, b in pairs), "neighbouring cells whose records share slots"
        assert int(np.isin(plan.cell, list(plan.wide)).sum()) > 1000, "most of the window lies in cells with a record"
    if name == "mixed":
        plain = {c for c, kept in plan.kept.items() if len(kept) > W}
        short = {c for c, kept in plan.kept.items() if len(kept) <= 8}
        assert plain and short and not plain & set(plan.wide)
        assert any((a in plan.wide and b in plain) or (b in plan.wide and a in plain) for a, b in pairs), "a record next to a plain overflowed list"
        assert any((a in plan.wide and b in short) or (b in plan.wide and a in short) for a, b in pairs), "a record next to a short list"
    if name == "corner":
        big = [b for b in plan.corners() if len(b) >= 3 and all(c in plan.wide for c in b) and len(frozenset().union(*(plan.wide[c] for c in b))) > 64]
        assert big, "cells with records around one pixel corner whose union exceeds 64 slots"


@pytest.mark.gpu
def test_frames_are_the_same_with_the_records_without_them_and_without_lists(tmp_path, host_probe):
    on, log_on = run_child(tmp_path, "on")
    off, log_off = run_child(tmp_path, "off")
    nolists, log_no = run_child(tmp_path, "nolists")
    for text in (log_on, log_off):
        assert "rt_primary_soft10_kernel: workgroups" in text and "rt_cell_resolve_kernel" in text, text[-2000:]
    assert "rt_primary_soft10_flags_kernel: workgroups" in log_no and "rt_primary_soft10_kernel:" not in log_no, log_no[-2000:]  # (no list is read)
    for name, flat in frame_scenes().items():
        a, b = np.load(on / f"{name}.npz"), np.load(off / f"{name}.npz")
        x0, y0, w, h = WIN
        hit = a["hit_id"].reshape(frame_cfg().height, frame_cfg().width)
        assert a["argb"].any() and (hit[y0:y0 + h, x0:x0 + w] >= 0).sum() > 3000, f"{name}: the receivers fill the window"
        pg.same(a, b, f"{name}: RT_CELL_WIDE=0")
        pg.same(a, np.load(nolists / f"{name}.npz"), f"{name}: tuning.no_cell_lists")
        assert int(a["bytes_cell_lists"]) > int(b["bytes_cell_lists"]), f"{name}: the pool counts in bytes_cell_lists, and RT_CELL_WIDE=0 leaves it out"
        shadowed = np.unique(a["argb"][a["argb"] != 0]).size
        print(f"{name}: {int((hit >= 0).sum())} pixels hit, {shadowed} distinct colours")
        check_plan(name, Plan(host_probe, name, flat, hit))


if __name__ == "__main__":
    child(sys.argv[1], sys.argv[2])
