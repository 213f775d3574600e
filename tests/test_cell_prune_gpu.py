"""rt_cell_prune_kernel (csrc/rt_cell_prune.hip) on the GPU: it writes what its host model writes, and the frames do not change.

1. Words.  A probe links against the built librt_hip.so -- the packer, rt_launch_flags, rt_launch_cell_prune and the host
   model come from the library, so the kernels driven here are the ones that ship.  It uploads a packed scene of a few
   thousand receiver cells, runs rt_flags_kernel with per-cell lists, reads lists and flags back, runs the prune kernel on
   the device and rt_cell_prune_packed on the copy read back: every list word and every flag word is equal.
2. Frames.  Semesterbild (text_lowres) at config 3's settings on a 96 x 80 window and the synthetic soft-shadow scene with the
   same features on its whole 48 x 40 frame, with the lists opted in (2 GiB budget): the frame with pruned lists
   is, packed pixels and float planes bit for bit, the frame with RT_CELL_PRUNE=0, the frame with
   shadow_candidate_cap = RT_CAND_CAP_NONE (a walk per sample: no list is read) and the union of a 3-rank tile partition.
   RT_CELL_PRUNE is read once per process, so each setting renders in a child process of its own, started before any GPU
   call, under its own time limit; RT_TRACE_LAUNCHES shows that the kernel ran where it should and only there.
3. After rt_scene_update the lists are rebuilt and pruned again: the frame equals a fresh scene's."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CHILD_TIMEOUT_S = 240
WIN = (330, 250, 96, 80)
SEM_WIN = (760, 560, 96, 80)
PLANES = ("argb", "rgb", "hit_id", "hit_t")

PROBE = r'''
#include <hip/hip_runtime_api.h>
#include <cstring>
#include "rt_cell_prune.h"
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
// flags and lists of the packed scene for one light-cloud table: raw_* as rt_flags_kernel leaves them, dev_* after
// rt_cell_prune_kernel, host_* = rt_cell_prune_packed of the raw ones
int probe_run(const float* cloud, uint64_t n_floats, const float* f, float eps, uint16_t* raw_lists, uint16_t* raw_flags, uint16_t* dev_lists,
              uint16_t* dev_flags, uint16_t* host_lists, uint16_t* host_flags) {
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
  char* blob = nullptr;
  float* geo = nullptr;
  uint16_t *lists = nullptr, *flags = nullptr;
  TRY(hipSetDevice(0));
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
  TRY((hipError_t)rt_launch_flags(sc, P, nullptr));
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(raw_lists, lists, list_bytes, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(raw_flags, flags, flag_bytes, hipMemcpyDeviceToHost));
  RtCellPruneArgs a{};
  a.flag_geo = geo, a.lists = lists, a.flags = flags;
  a.n_cells = g.n_cells, a.n_tri_cells = g.n_tri_cells;
  memcpy(a.cloud_centre, ball, 12);
  a.beam_delta = P.beam_delta, a.beam_eps_o = P.beam_eps_o;
  a.mode = RT_PRUNE_FULL;
  TRY((hipError_t)rt_launch_cell_prune(sc, a, nullptr));
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(dev_lists, lists, list_bytes, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(dev_flags, flags, flag_bytes, hipMemcpyDeviceToHost));
  memcpy(host_lists, raw_lists, list_bytes), memcpy(host_flags, raw_flags, flag_bytes);
  a.lists = host_lists, a.flags = host_flags;
  rt_cell_prune_packed(g, a);
  TRY(hipFree(blob));
  TRY(hipFree(geo));
  TRY(hipFree(lists));
  TRY(hipFree(flags));
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
    d = tmp_path_factory.mktemp("cell_prune_gpu_probe")
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


# ---- 1. words ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["synthetic", "sphere_receiver", "semesterbild"])
def test_kernel_writes_the_host_models_words(probe, name):
    import flags_cases
    import test_cell_prune_host as host
    from test_scene_pack_host import ptr
    from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, sampling
    cfg, flat, _ = host.CASES[name]()
    desc, keep = _abi.make_scene_desc(flat)
    out = np.zeros(4, np.uint32)
    budget = 48 * flat.n_triangles + 8192  # the flags' input and at most 4096 cells
    assert probe.probe_pack(C.byref(desc), C.c_uint64(budget), ptr(out)) == 0, probe.probe_error()
    n_cells, n_tri_cells, nl, ns = (int(v) for v in out)
    assert 0 < n_cells <= 4096 and (name != "sphere_receiver" or n_cells > n_tri_cells), (n_cells, n_tri_cells)
    cs = np.ascontiguousarray(sampling.cloud_sets(cfg), np.float32)
    f = np.array([cfg.fw, cfg.fh, cfg.fd], np.float32)
    lists = [np.zeros((n_cells, nl, 8), np.uint16) for _ in range(3)]
    flags = [np.zeros(n_cells, np.uint16) for _ in range(3)]
    rc = probe.probe_run(ptr(cs), C.c_uint64(cs.size), ptr(f), C.c_float(cfg.eps_distance), ptr(lists[0]), ptr(flags[0]), ptr(lists[1]), ptr(flags[1]),
                         ptr(lists[2]), ptr(flags[2]))
    assert rc == 0, f"probe_run: {rc}"
    (raw_l, dev_l, host_l), (raw_f, dev_f, host_f) = lists, flags
    listed = lambda a: int((a < host.OVERFLOW).sum())  # noqa: E731
    clear = lambda a: int(sum(bin(int(v) & 0xFF).count("1") for v in a))  # noqa: E731
    print(f"{name}: {n_cells} cells, {nl} lights; listed slots {listed(raw_l)} -> {listed(dev_l)}, overflowed lists {int((raw_l[:, :, 0] == host.OVERFLOW).sum())}, "
          f"triangle-clear bits {clear(raw_f)} -> {clear(dev_f)}")
    assert sum(flags_cases.check_shape(raw_l, raw_f, ns)) > 0, "rt_flags_kernel listed something, in well-formed lists"
    assert np.array_equal(dev_l, host_l), f"{int((dev_l != host_l).sum())} list words differ"
    assert np.array_equal(dev_f, host_f), f"{int((dev_f != host_f).sum())} flag words differ"
    assert np.array_equal(raw_l[:, :, 0] == host.OVERFLOW, dev_l[:, :, 0] == host.OVERFLOW), "overflowed lists are left alone"
    assert ((dev_f & ~raw_f) >> 8 == 0).all() and ((raw_f & ~dev_f) == 0).all(), "only triangle-clear bits are added"


# ---- 2. frames -----------------------------------------------------------------------------------------------------------------
def _scenes():
    import material_cases as mc
    import scene_update_cases as cases
    from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig
    cfg3 = RenderConfig.from_features(["high_resolution", "anti_aliasing", "soft_shadows"])  # bench.py's c3
    syn_cfg, syn = mc.workload("c3")
    return {"synthetic": (syn_cfg, syn, None), "semesterbild": (cfg3, cases.flat_semesterbild(cfg3), SEM_WIN)}


def child(out_dir, variants):
    """One process = one value of RT_CELL_PRUNE: renders every scene in every listed variant and writes the frames to out_dir."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi
    from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceScene, ImageBuffer, RaytracerRenderer
    for name, (cfg, flat, win) in _scenes().items():
        ds = DeviceScene(flat, 0, budget=2 << 30)
        r = RaytracerRenderer(cfg, device=0)

        def frame(tag, **kw):
            buf = ImageBuffer.new(cfg.width, cfg.height)
            planes = r.render(buf, ds, window=win, aux=True, **kw)
            np.savez(os.path.join(out_dir, f"{name}_{tag}.npz"), argb=np.asarray(buf.buffer), rgb=planes["rgb"], hit_id=planes["hit_id"], hit_t=planes["hit_t"])
        for v in variants:
            if v == "plain":
                frame("plain")
                assert ds.memory_info()["cell_lists_built"] == 1, "the lists exist"
            elif v == "capnone":
                frame("capnone", tuning=dict(shadow_candidate_cap=_abi.RT_CAND_CAP_NONE))
            elif v == "ranks":
                for rank in range(3):
                    frame(f"rank{rank}", n_ranks=3, rank=rank)
        ds.close()


def run_child(tmp_path, tag, variants, prune):
    out = tmp_path / tag
    out.mkdir()
    env = dict(os.environ, RT_TRACE_LAUNCHES="1")
    env.pop("RT_CELL_PRUNE", None)
    if not prune:
        env["RT_CELL_PRUNE"] = "0"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), str(out), ",".join(variants)]
    proc = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    assert proc.returncode == 0, (cmd, proc.returncode, proc.stderr[-4000:])
    return out, proc.stderr


def same(a, b, what):
    for plane in PLANES:
        assert a[plane].dtype == b[plane].dtype and a[plane].dtype.itemsize == 4, (plane, a[plane].dtype)
        assert np.array_equal(a[plane].view(np.uint32), b[plane].view(np.uint32)), (what, plane, int((a[plane].view(np.uint32) != b[plane].view(np.uint32)).sum()))


@pytest.mark.gpu
def test_pruned_lists_render_the_same_frames(tmp_path):
    pruned, log = run_child(tmp_path, "pruned", ["plain", "capnone", "ranks"], prune=True)
    unpruned, log0 = run_child(tmp_path, "unpruned", ["plain"], prune=False)
    assert "rt_cell_prune_kernel" in log and "rt_primary_soft10_kernel: workgroups" in log, log[-2000:]
    assert "rt_cell_prune_kernel" not in log0 and "rt_primary_soft10_kernel: workgroups" in log0, log0[-2000:]
    for name in ("synthetic", "semesterbild"):
        a = np.load(pruned / f"{name}_plain.npz")
        assert a["argb"].any() and (a["hit_id"] >= 0).any(), name  # (a frame was rendered at all)
        same(a, np.load(unpruned / f"{name}_plain.npz"), f"{name}: RT_CELL_PRUNE=0")
        same(a, np.load(pruned / f"{name}_capnone.npz"), f"{name}: RT_CAND_CAP_NONE")
        parts = [np.load(pruned / f"{name}_rank{k}.npz") for k in range(3)]
        written = [p["argb"] != 0 for p in parts]
        assert not (written[0] & written[1]).any() and not (written[0] & written[2]).any() and not (written[1] & written[2]).any()
        assert np.array_equal(written[0] | written[1] | written[2], a["argb"] != 0), f"{name}: the ranks' tiles cover the frame"
        for p, w in zip(parts, written):
            assert np.array_equal(p["argb"][w], a["argb"][w]), f"{name}: 3-rank tile union, packed pixels"
            assert np.array_equal(p["rgb"].reshape(-1, 3)[w].view(np.uint32), a["rgb"].reshape(-1, 3)[w].view(np.uint32)), f"{name}: 3-rank tile union, rgb"


# ---- 3. updates ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lists_are_pruned_again_after_a_scene_update():
    import scene_update_cases as cases
    from test_scene_update_gpu import CONFIGS, assert_same_frame, render
    from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceScene
    cfg, win = CONFIGS["soft"](), (200, 150, 96, 80)
    flat = cases.flat_semesterbild()
    moved = cases.orbit_lights(cases.turn_mesh(flat, cases.mesh_range("semesterbild", flat), degrees=15.0))
    ds = DeviceScene(flat, 0, budget=2 << 30)
    render(cfg, ds, win)
    ds.update(moved)
    assert ds.memory_info()["cell_lists_built"] == 0
    got = render(cfg, ds, win)
    assert ds.memory_info()["cell_lists_built"] == 1 and got[2]["setup_ms"] > 0.0, "flags and lists were rebuilt by this frame"
    fresh = DeviceScene(moved, 0, budget=2 << 30)
    want = render(cfg, fresh, win)
    assert assert_same_frame(got, want, "update, lists on"), "the float rgb plane too"
    ds.close(), fresh.close()


if __name__ == "__main__":
    child(sys.argv[1], sys.argv[2].split(","))
