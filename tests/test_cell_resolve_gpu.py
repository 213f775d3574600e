"""rt_cell_resolve_kernel (csrc/rt_cell_resolve.hip) on the GPU: it writes what its host model writes, and the frames do not change.

1. Words.  A probe links against the built librt_hip.so, as the one of test_cell_prune_gpu.py does, and runs the three stages
   on a packed scene of at most 4096 receiver cells: rt_flags_kernel with per-cell lists, rt_cell_prune_kernel, read back,
   rt_cell_resolve_kernel, read back; rt_cell_resolve_packed on the copy read back after stage two.  Every list word and
   every flag word is equal.  Scenes: the synthetic one, the sphere receiver, semesterbild and the fans of
   test_cell_resolve_host.py, in each of which at least one list goes from overflowed to resolved.  The work list is also
   given room for 300 cells only, so that the stage goes chunk by chunk: same words.
2. Frames.  The frames of test_cell_prune_gpu.py (semesterbild text_lowres at config 3's settings on the 96 x 80 window over
   the text, the synthetic 48 x 40 frame; lists opted in): the frame with the stage on is, packed pixels and float planes bit
   for bit, the frame with RT_CELL_RESOLVE=0, the frame with shadow_candidate_cap = RT_CAND_CAP_NONE and the union of a 3-rank
   tile partition.  RT_CELL_RESOLVE is read once per process: every setting renders in a child process of its own, started
   before any GPU call, under its own time limit; RT_TRACE_LAUNCHES shows that the kernel ran where it should and only
   there -- not with RT_CELL_RESOLVE=0 and not with RT_CELL_PRUNE=0.
3. After rt_scene_update the lists are rebuilt, pruned and resolved again: the frame equals a fresh scene's."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import test_cell_prune_gpu as pg

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
// flags and lists of the packed scene for one light-cloud table: raw_* as rt_flags_kernel leaves them, two_* after
// rt_cell_prune_kernel, dev_* after rt_cell_resolve_kernel, host_* = rt_cell_resolve_packed of the two_* ones.  work_cells: room of
// the work list (0 = what rt_cell_resolve_temp_bytes gives for 64 MiB)
int probe_run(const float* cloud, uint64_t n_floats, const float* f, float eps, uint32_t work_cells, uint16_t* raw_lists, uint16_t* two_lists, uint16_t* two_flags,
              uint16_t* dev_lists, uint16_t* dev_flags, uint16_t* host_lists, uint16_t* host_flags) {
  if (dead) return dead;
  if (!g.n_cells || g.dev.n_lights > 8u || g.dev.n_slots > 65533u) return -100;
  std::vector<float> scaled;
  float ball[4];
  rt_scale_cloud(cloud, n_floats, f, &scaled, ball);
  RtDevParams P{};
  memcpy(P.cloud_centre, ball, 12);
  P.cloud_delta = ball[3];
  P.eps_distance = eps;
  rt_beam_constants(eps, &P);
  P.cand_cap = 64u;
  const size_t list_bytes = (size_t)g.n_cells * g.dev.n_lights * 16u, flag_bytes = (size_t)g.n_cells * 2u;
  RtCellResolveArgs r{};
  const size_t temp = rt_cell_resolve_temp_bytes(g.n_cells, work_cells ? 4096u + 4u * (size_t)work_cells : (size_t)64u << 20, &r.chunk_cells);
  if (!temp || (work_cells && r.chunk_cells != (work_cells < g.n_cells ? work_cells : g.n_cells))) return -101;
  char* blob = nullptr;
  float* geo = nullptr;
  uint16_t *lists = nullptr, *flags = nullptr;
  TRY(hipSetDevice(0));
  TRY(hipMalloc((void**)&blob, g.blob.size()));
  TRY(hipMalloc((void**)&geo, g.flag_geo.size() * 4));
  TRY(hipMalloc((void**)&lists, list_bytes + 64));
  TRY(hipMalloc((void**)&flags, flag_bytes + 64));
  uint32_t* work = nullptr;
  TRY(hipMalloc((void**)&work, temp));
  r.work = work;
  TRY(hipMemcpy(blob, g.blob.data(), g.blob.size(), hipMemcpyHostToDevice));
  TRY(hipMemcpy(geo, g.flag_geo.data(), g.flag_geo.size() * 4, hipMemcpyHostToDevice));
  TRY(hipMemset(lists, 0xFF, list_bytes));
  TRY(hipMemset(flags, 0, flag_bytes));
  RtDevScene sc = g.dev;
  sc.base = blob;
  P.flag_out = flags, P.flag_geo = (const float4*)geo, P.cell_list_out = lists;
  P.n_cells = g.n_cells, P.n_tri_cells = g.n_tri_cells;
  TRY((hipError_t)rt_launch_flags(sc, P, nullptr));
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(raw_lists, lists, list_bytes, hipMemcpyDeviceToHost));
  RtCellPruneArgs a{};
  a.flag_geo = geo, a.lists = lists, a.flags = flags;
  a.n_cells = g.n_cells, a.n_tri_cells = g.n_tri_cells;
  memcpy(a.cloud_centre, ball, 12);
  a.beam_delta = P.beam_delta, a.beam_eps_o = P.beam_eps_o;
  a.mode = RT_PRUNE_FULL;
  TRY((hipError_t)rt_launch_cell_prune(sc, a, nullptr));
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(two_lists, lists, list_bytes, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(two_flags, flags, flag_bytes, hipMemcpyDeviceToHost));
  r.cell = a;
  r.eps_push = P.beam_eps_push, r.eps_ulp = P.beam_eps_ulp;
  TRY((hipError_t)rt_launch_cell_resolve(sc, r, nullptr));
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(dev_lists, lists, list_bytes, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(dev_flags, flags, flag_bytes, hipMemcpyDeviceToHost));
  memcpy(host_lists, two_lists, list_bytes), memcpy(host_flags, two_flags, flag_bytes);
  r.cell.lists = host_lists, r.cell.flags = host_flags, r.work = nullptr;
  rt_cell_resolve_packed(g, r);
  TRY(hipFree(blob));
  TRY(hipFree(geo));
  TRY(hipFree(lists));
  TRY(hipFree(flags));
  TRY(hipFree(work));
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
    d = tmp_path_factory.mktemp("cell_resolve_gpu_probe")
    src = d / "probe.cpp"
    src.write_text(PROBE)
    so = d / "probe.so"
    lib_dir, lib_name = os.path.split(os.path.abspath(_lib.LIB_PATH))
    out = subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip", "--cuda-host-only", "-I", CSRC,
                          "-I", os.path.join(pg.ROOT, "include"), "-shared", "-o", str(so), str(src),
                          "-L", lib_dir, f"-l:{lib_name}", f"-Wl,-rpath,{lib_dir}"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lib = C.CDLL(str(so))
    lib.probe_error.restype = C.c_char_p
    return lib


# ---- 1. words ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name, work_cells", [("synthetic", 0), ("sphere_receiver", 0), ("semesterbild", 0), ("semesterbild", 300), ("fan_behind", 0),
                                              ("fan_mixed", 0), ("fan_between", 0)])
def test_kernel_writes_the_host_models_words(probe, name, work_cells):
    import flags_cases
    import test_cell_resolve_host as rh
    from test_scene_pack_host import ptr
    from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, sampling
    host = rh.host
    cfg, flat, _ = host.CASES[name]()
    desc, keep = _abi.make_scene_desc(flat)
    out = np.zeros(4, np.uint32)
    budget = 48 * flat.n_triangles + 8192  # the flags' input and at most 4096 cells
    assert name not in rh.FANS or budget == rh.FAN_BUDGET
    assert probe.probe_pack(C.byref(desc), C.c_uint64(budget), ptr(out)) == 0, probe.probe_error()
    n_cells, n_tri_cells, nl, ns = (int(v) for v in out)
    assert 0 < n_cells <= 4096 and (name not in rh.FANS and name != "sphere_receiver" or n_cells > n_tri_cells), (n_cells, n_tri_cells)
    cs = np.ascontiguousarray(sampling.cloud_sets(cfg), np.float32)
    f = np.array([cfg.fw, cfg.fh, cfg.fd], np.float32)
    raw_l, two_l, dev_l, host_l = (np.zeros((n_cells, nl, 8), np.uint16) for _ in range(4))
    two_f, dev_f, host_f = (np.zeros(n_cells, np.uint16) for _ in range(3))
    rc = probe.probe_run(ptr(cs), C.c_uint64(cs.size), ptr(f), C.c_float(cfg.eps_distance), C.c_uint32(work_cells), ptr(raw_l), ptr(two_l), ptr(two_f),
                         ptr(dev_l), ptr(dev_f), ptr(host_l), ptr(host_f))
    assert rc == 0, f"probe_run: {rc}"
    over2, over3 = two_l[:, :, 0] == host.OVERFLOW, dev_l[:, :, 0] == host.OVERFLOW
    clear = lambda a: int(sum(bin(int(v) & 0xFF).count("1") for v in a))  # noqa: E731
    print(f"{name}: {n_cells} cells, {nl} lights, work list of {work_cells or 'all'} cells; overflowed lists {int(over2.sum())} -> {int(over3.sum())} "
          f"({int((over2 & ~over3 & (dev_l[:, :, 0] == host.END)).sum())} emptied), triangle-clear bits {clear(two_f)} -> {clear(dev_f)}")
    assert sum(flags_cases.check_shape(raw_l, None, ns)) > 0, "rt_flags_kernel listed something, in well-formed lists"
    assert np.array_equal(raw_l[:, :, 0] == host.OVERFLOW, over2), "stage two leaves overflowed lists alone"
    assert np.array_equal(dev_l, host_l), f"{int((dev_l != host_l).sum())} list words differ"
    assert np.array_equal(dev_f, host_f), f"{int((dev_f != host_f).sum())} flag words differ"
    assert np.array_equal(dev_l[~over2], two_l[~over2]), "a list that is not overflowed is not touched"
    assert not (over3 & ~over2).any() and ((dev_f & ~two_f) >> 8 == 0).all() and ((two_f & ~dev_f) == 0).all(), "only triangle-clear bits are added"
    if name in rh.FANS or name == "semesterbild":
        assert (over2 & ~over3).any(), "at least one list goes from overflowed to resolved"
    if name == "fan_between":
        assert over3.any(), "under 12 panes the list stays overflowed"


# ---- 2. frames -----------------------------------------------------------------------------------------------------------------
def run_child(tmp_path, tag, variants, off=None):
    """the frames of test_cell_prune_gpu.py (its child()) in a fresh process with RT_CELL_RESOLVE / RT_CELL_PRUNE set to 0 or unset"""
    out = tmp_path / tag
    out.mkdir()
    env = dict(os.environ, RT_TRACE_LAUNCHES="1")
    env.pop("RT_CELL_PRUNE", None), env.pop("RT_CELL_RESOLVE", None)
    if off:
        env[off] = "0"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(pg.__file__), str(out), ",".join(variants)]
    proc = subprocess.run(cmd, cwd=pg.ROOT, env=env, capture_output=True, text=True, timeout=pg.CHILD_TIMEOUT_S)
    assert proc.returncode == 0, (cmd, proc.returncode, proc.stderr[-4000:])
    return out, proc.stderr


@pytest.mark.gpu
def test_resolved_lists_render_the_same_frames(tmp_path):
    on, log = run_child(tmp_path, "on", ["plain", "capnone", "ranks"])
    off, log0 = run_child(tmp_path, "off", ["plain"], off="RT_CELL_RESOLVE")
    unpruned, log00 = run_child(tmp_path, "unpruned", ["plain"], off="RT_CELL_PRUNE")
    for text in (log, log0, log00):
        assert "rt_primary_soft10_kernel: workgroups" in text, text[-2000:]
    assert "rt_cell_resolve_kernel" in log and "rt_cell_prune_kernel" in log, log[-2000:]
    assert "rt_cell_resolve_kernel" not in log0 and "rt_cell_prune_kernel" in log0, log0[-2000:]
    assert "rt_cell_resolve_kernel" not in log00 and "rt_cell_prune_kernel" not in log00, log00[-2000:]
    for name in ("synthetic", "semesterbild"):
        a = np.load(on / f"{name}_plain.npz")
        assert a["argb"].any() and (a["hit_id"] >= 0).any(), name  # (a frame was rendered at all)
        pg.same(a, np.load(off / f"{name}_plain.npz"), f"{name}: RT_CELL_RESOLVE=0")
        pg.same(a, np.load(unpruned / f"{name}_plain.npz"), f"{name}: RT_CELL_PRUNE=0")
        pg.same(a, np.load(on / f"{name}_capnone.npz"), f"{name}: RT_CAND_CAP_NONE")
        parts = [np.load(on / f"{name}_rank{k}.npz") for k in range(3)]
        written = [p["argb"] != 0 for p in parts]
        assert not (written[0] & written[1]).any() and not (written[0] & written[2]).any() and not (written[1] & written[2]).any()
        assert np.array_equal(written[0] | written[1] | written[2], a["argb"] != 0), f"{name}: the ranks' tiles cover the frame"
        for p, w in zip(parts, written):
            assert np.array_equal(p["argb"][w], a["argb"][w]), f"{name}: 3-rank tile union, packed pixels"
            assert np.array_equal(p["rgb"].reshape(-1, 3)[w].view(np.uint32), a["rgb"].reshape(-1, 3)[w].view(np.uint32)), f"{name}: 3-rank tile union, rgb"


# ---- 3. updates ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lists_are_resolved_again_after_a_scene_update():
    import scene_update_cases as cases
    from test_scene_update_gpu import CONFIGS, assert_same_frame, render
    from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceScene
    cfg, win = CONFIGS["soft"](), (200, 150, 96, 80)
    flat = cases.flat_semesterbild()
    moved = cases.orbit_lights(cases.turn_mesh(flat, cases.mesh_range("semesterbild", flat), degrees=-25.0))
    ds = DeviceScene(flat, 0, budget=2 << 30)
    render(cfg, ds, win)
    before = ds.memory_info()
    assert before["cell_lists_built"] == 1
    ds.update(moved)
    assert ds.memory_info()["cell_lists_built"] == 0
    got = render(cfg, ds, win)
    after = ds.memory_info()
    assert after["cell_lists_built"] == 1 and got[2]["setup_ms"] > 0.0, "flags and lists were rebuilt by this frame"
    assert after["bytes_cell_lists"] == before["bytes_cell_lists"] and before["bytes_cell_lists"] + before["bytes_flags"] <= before["budget_bytes"]
    fresh = DeviceScene(moved, 0, budget=2 << 30)
    want = render(cfg, fresh, win)
    assert assert_same_frame(got, want, "update, lists resolved"), "the float rgb plane too"
    ds.close(), fresh.close()
