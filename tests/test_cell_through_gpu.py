"""The marks of certain glass-pane crossings on the GPU (csrc/rt_cell_through.hip writes them, the list-union block and the
sample loop of the list kernels in csrc/rt_kernels.hip read them): the device writes what the host model writes, and no frame
changes.

1. Words.  rt_flags_kernel, rt_cell_prune_kernel, rt_cell_resolve_kernel with a pool of wide records, read back;
   rt_cell_through_kernel, read back: the lists are untouched, every byte of the marks table is written, and the table is,
   byte for byte, what rt_cell_through_packed writes for the lists read back.  On the panes of test_cell_through_host.py and on
   semesterbild with text_lowres (at most 4096 cells).
2. Frames.  Soft shadows x 10 on a 64 x 64 window of the 768 x 640 frame; the camera looks along +z at receivers that face
   it, the light stands off to the side at +x, the panes stand in planes x = const beyond the camera's view, between the
   receivers and the light.  Every frame is, packed pixels and float planes bit for bit, the same with the marks, with
   RT_CELL_THROUGH=0 and with tuning.no_cell_lists; RT_CELL_THROUGH is read once per process, so each arm renders in a child
   process of its own.  The stages run again in the probe on each scene, packed as the render packs it, then say for the
   cells under the rendered pixels (flags_cases.receiver_cell, float32) that the cases are there:
     across     a glass pane across all beams: every cell under the window lists it as marked
     edge       a pane whose edge runs through the window's beams: neighbouring pixels in a marked and in an unmarked cell
     materials  two panes of two glass materials, both marked (the occluder memo changes rows between marked entries)
     opaque     a marked pane and an opaque triangle behind it in one list
     quad       a two-triangle quad with its diagonal in the beams: cells with one half marked, cells with neither
     wide       ten panes that start differently far up: a cell with a wide record next to a cell with marked entries
     lights     the pane across all beams under two lights: marks for both"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import test_cell_prune_gpu as pg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
END, OVERFLOW, MARK = 0xFFFF, 0xFFFE, 0xFFFD
TRANSMISSIVE = 0x40000000

PROBE = r'''
#include <hip/hip_runtime_api.h>
#include <cstring>
#include "rt_cell_through.h"
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
int probe_pack(const rt_scene_desc* d, uint64_t budget, uint32_t* out, unsigned char* blob, uint32_t* dev) {
  const int rc = rt_pack_scene(d, budget, &g);
  out[0] = g.n_cells, out[1] = g.n_tri_cells, out[2] = g.dev.n_lights, out[3] = g.dev.n_slots, out[4] = (uint32_t)g.blob.size();
  if (blob && !g.blob.empty()) memcpy(blob, g.blob.data(), g.blob.size());
  if (dev) memcpy(dev, &g.dev.off_spheres, 19 * 4);
  return rc;
}
// the four stages on the device.  three: the lists after the third stage, four: after the fourth; dev_marks / host_marks: the table
// ([n_cells * n_lights] bytes, backwards from its end) as the kernel and as rt_cell_through_packed write it for `three`
int probe_run(const float* cloud, uint64_t n_floats, const float* f, float eps, uint16_t* three, uint16_t* four, uint8_t* dev_marks, uint8_t* host_marks) {
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
  const size_t n_lists = (size_t)g.n_cells * g.dev.n_lights, list_bytes = n_lists * 16u, flag_bytes = (size_t)g.n_cells * 2u;
  const uint32_t cap = (uint32_t)(n_lists / 8u + 1u);
  const size_t pool_bytes = (size_t)cap * 2u * RT_CELL_WIDE_SLOTS;
  RtCellResolveArgs r{};
  const size_t temp = rt_cell_resolve_temp_bytes(g.n_cells, (size_t)64u << 20, &r.chunk_cells);
  if (!temp) return -101;
  char *blob = nullptr, *pool = nullptr;
  float* geo = nullptr;
  uint16_t *lists = nullptr, *flags = nullptr;
  uint32_t* work = nullptr;
  uint8_t* marks = nullptr;
  TRY(hipSetDevice(0));
  TRY(hipMalloc((void**)&blob, g.blob.size()));
  TRY(hipMalloc((void**)&geo, g.flag_geo.size() * 4));
  TRY(hipMalloc((void**)&lists, list_bytes + 64));
  TRY(hipMalloc((void**)&flags, flag_bytes + 64));
  TRY(hipMalloc((void**)&work, temp));
  TRY(hipMalloc((void**)&pool, pool_bytes + 64));
  TRY(hipMalloc((void**)&marks, n_lists + 64));
  TRY(hipMemcpy(blob, g.blob.data(), g.blob.size(), hipMemcpyHostToDevice));
  TRY(hipMemcpy(geo, g.flag_geo.data(), g.flag_geo.size() * 4, hipMemcpyHostToDevice));
  TRY(hipMemset(lists, 0xFF, list_bytes));
  TRY(hipMemset(flags, 0, flag_bytes));
  TRY(hipMemset(pool, 0xAB, pool_bytes + 64));
  TRY(hipMemset(marks, 0xAB, n_lists + 64));  // (the stage writes every byte of the table itself)
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
  r.cell = a;
  r.eps_push = P.beam_eps_push, r.eps_ulp = P.beam_eps_ulp;
  r.work = work, r.wide = (uint16_t*)pool, r.wide_cap = cap, r.wide_count = (uint32_t*)(pool + pool_bytes);
  TRY((hipError_t)rt_launch_cell_resolve(sc, r, nullptr));
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(three, lists, list_bytes, hipMemcpyDeviceToHost));
  RtCellThroughArgs t{};
  t.cell = a;
  t.marks_end = marks + n_lists;
  TRY((hipError_t)rt_launch_cell_through(sc, t, nullptr));
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(four, lists, list_bytes, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(dev_marks, marks, n_lists, hipMemcpyDeviceToHost));
  t.cell.lists = three, t.cell.flags = nullptr, t.marks_end = host_marks + n_lists;
  rt_cell_through_packed(g, t);
  TRY(hipFree(blob));
  TRY(hipFree(geo));
  TRY(hipFree(lists));
  TRY(hipFree(flags));
  TRY(hipFree(work));
  TRY(hipFree(pool));
  TRY(hipFree(marks));
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
    d = tmp_path_factory.mktemp("cell_through_gpu_probe")
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


class Stages:
    """the four stages run on the device for one scene: lists, marks[cell, light] of the kernel and of the host model"""

    def __init__(self, probe, cfg, flat, budget):
        from test_scene_pack_host import DEV_FIELDS, ptr
        from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, sampling
        desc, keep = _abi.make_scene_desc(flat)
        out = np.zeros(5, np.uint32)
        assert probe.probe_pack(C.byref(desc), C.c_uint64(budget), ptr(out), None, None) == 0, probe.probe_error()
        self.n_cells, self.n_tri_cells, self.nl, self.ns = (int(v) for v in out[:4])
        self.blob, dev = np.zeros(int(out[4]), np.uint8), np.zeros(19, np.uint32)
        assert probe.probe_pack(C.byref(desc), C.c_uint64(budget), ptr(out), ptr(self.blob), ptr(dev)) == 0
        self.dev = {n: int(v) for n, v in zip(DEV_FIELDS, dev)}
        o = self.dev["off_tri_id"]
        ids = self.blob[o:o + 4 * self.ns].view(np.uint32)
        self.tri_of_slot, self.transmissive = ids & 0x3FFFFFFF, (ids & TRANSMISSIVE) != 0
        cs = np.ascontiguousarray(sampling.cloud_sets(cfg), np.float32)
        f = np.array([cfg.fw, cfg.fh, cfg.fd], np.float32)
        n = self.n_cells * self.nl
        self.three, self.four = np.zeros((self.n_cells, self.nl, 8), np.uint16), np.zeros((self.n_cells, self.nl, 8), np.uint16)
        dev_m, host_m = np.zeros(n, np.uint8), np.full(n, 0xCD, np.uint8)
        rc = probe.probe_run(ptr(cs), C.c_uint64(cs.size), ptr(f), C.c_float(cfg.eps_distance), ptr(self.three), ptr(self.four), ptr(dev_m), ptr(host_m))
        assert rc == 0, f"probe_run: {rc}"
        self.dev_marks, self.host_marks = dev_m[::-1].reshape(self.n_cells, self.nl).copy(), host_m[::-1].reshape(self.n_cells, self.nl).copy()
        del keep

    def check(self, what):
        assert np.array_equal(self.three, self.four), f"{what}: the stage only reads the lists"
        assert np.array_equal(self.dev_marks, self.host_marks), f"{what}: {int((self.dev_marks != self.host_marks).sum())} mark bytes differ"
        lists, m = self.four, self.dev_marks
        short = lists[:, :, 0] < OVERFLOW
        assert not m[~short].any(), f"{what}: empty and overflowed lists carry no marks"
        for k in range(8):
            on = (m >> k) & 1 == 1
            s = lists[:, :, k][on]
            assert (s < self.ns).all() and self.transmissive[s].all(), f"{what}: only listed transmissive slots are marked"

    def marked_tris(self, c, l=0):
        """canonical triangles listed for (c, l), and those of them that are marked; None: the list is overflowed"""
        w = self.four[c, l]
        if w[0] == OVERFLOW:
            return None, None
        n = int(np.argmax(w >= OVERFLOW)) if (w >= OVERFLOW).any() else 8
        listed = [int(self.tri_of_slot[s]) for s in w[:n]]
        return listed, [t for k, t in enumerate(listed) if (int(self.dev_marks[c, l]) >> k) & 1]


# ---- 1. words ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["panes", "panes_two_lights", "semesterbild"])
def test_kernel_writes_the_host_models_marks(probe, name):
    import test_cell_through_host as th
    cfg, flat, _ = th.host.CASES[name]()
    st = Stages(probe, cfg, flat, th.PANE_BUDGET if name.startswith("panes") else 48 * flat.n_triangles + 8192)
    st.check(name)
    listed = int((st.four[st.four[:, :, 0] < OVERFLOW] < OVERFLOW).sum())
    print(f"{name}: {st.n_cells} cells, {st.nl} lights, {listed} listed entries, marked {int(np.unpackbits(st.dev_marks).sum())}")
    if name.startswith("panes"):
        assert st.dev_marks[:, 0].any() and (name == "panes" or st.dev_marks[:, 1].any()), "there are marks here"


# ---- 2. frames -----------------------------------------------------------------------------------------------------------------
WIN = (352, 288, 64, 64)
LIGHT = [1.4, 0.41666666, 0.05, 1.0, 0.9, 0.8, 3.0]
LIGHT2 = [1.3, 0.55, 0.2, 0.3, 0.4, 0.9, 2.0]
# stretches the scene's diagonal: receiver cells of about 0.01, four pixels wide.  Its own 5000 cells list nothing, and the pool of
# wide records is sized by the number of lists: they leave records for the receiver's cells
FAR = ([2.0, 2.0, 10.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0])
BUDGET = 64 << 20
GLASS, GLASS2, DIFFUSE = 1, 2, 0
MAT_GLASS2 = [0.6, 0.9, 0.7, 0.0, 0.2, 1.3, 0.6, 0.3, 1.0]


def _scene(panes, mats, lights=(LIGHT,)):
    """the receiver quad (canonical triangles 0, 1), then the panes in order (2, 3, ...), then the far triangle"""
    import test_cell_prune_host as host
    from test_scene_pack_host import MAT_DIFFUSE, MAT_GLASS, flat_of
    v1, e1, e2 = host._quad([0.42, 0.33666666, 0.5], [0.0, 0.16, 0.0], [0.16, 0.0, 0.0])  # faces the camera (normal -z)
    for p in list(panes) + [FAR]:
        v1, e1, e2 = v1 + [np.asarray(p[0], np.float64)], e1 + [np.asarray(p[1], np.float64)], e2 + [np.asarray(p[2], np.float64)]
    nrm = np.cross(np.asarray(e1), np.asarray(e2))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return flat_of(v1=v1, e1=e1, e2=e2, nrm=nrm, tm=[DIFFUSE, DIFFUSE] + list(mats) + [DIFFUSE], mats=[MAT_DIFFUSE, MAT_GLASS, MAT_GLASS2], lights=list(lights)).contiguous()


def _pane(x, y0=0.28, z0=0.18, h=0.5, d=0.6):
    """a triangle in the plane x = const: corner (y0, z0), legs h along y and d along z"""
    return ([x, y0, z0], [0.0, h, 0.0], [0.0, 0.0, d])


def frame_scenes():
    """name -> flat scene.  A beam from the receiver (z = 0.5, y in 0.34 .. 0.50) to the light crosses x = 0.75 at y in 0.36 .. 0.48,
    z about 0.37"""
    y_mid = LIGHT[1]
    quad = [([0.75, 0.27, 0.0], [0.0, 0.3, 0.0], [0.0, 0.0, 0.75]), ([0.75, 0.57, 0.75], [0.0, -0.3, 0.0], [0.0, 0.0, -0.75])]  # diagonal through (y, z) = (0.42, 0.375)
    # ten narrow panes, each starting 0.004 further up than the one before: the receiver's rows of cells cross none to all ten
    stairs = [_pane(0.75 + 0.004 * i, y0=0.40 + 0.004 * i, z0=0.25, h=0.15, d=0.4) for i in range(10)]
    return {"across": _scene([_pane(0.75)], [GLASS]),
            "edge": _scene([_pane(0.75, y0=y_mid)], [GLASS]),
            "materials": _scene([_pane(0.75), _pane(0.76)], [GLASS, GLASS2]),
            "opaque": _scene([_pane(0.75), _pane(0.8, y0=y_mid + 0.02)], [GLASS, DIFFUSE]),
            "quad": _scene(quad, [GLASS, GLASS]),
            "wide": _scene(stairs, [GLASS] * 10),
            "lights": _scene([_pane(0.75)], [GLASS], lights=(LIGHT, LIGHT2))}


def frame_cfg():
    from test_cell_prune_host import soft_cfg
    return soft_cfg()  # anti-aliasing and soft shadows x 10, 768 x 640


def child(out_dir, arm):
    """one process = one arm: every frame, written to out_dir"""
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
    for v in ("RT_CELL_PRUNE", "RT_CELL_RESOLVE", "RT_CELL_WIDE", "RT_CELL_THROUGH"):
        env.pop(v, None)
    if arm == "off":
        env["RT_CELL_THROUGH"] = "0"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), str(out), arm]
    proc = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=pg.CHILD_TIMEOUT_S)
    assert proc.returncode == 0, (cmd, proc.returncode, proc.stderr[-4000:])
    return out, proc.stderr


def cells_under_window(st, flat, cfg, hit_id):
    """[h, w] receiver cell of every pixel of WIN all of whose samples lie in one cell of the receiver quad (-1: none)"""
    import flags_cases
    x0, y0, w, h = WIN
    f = np.array([cfg.focus.x, cfg.focus.y, cfg.focus.z], np.float64)
    k = type("K", (), {"dev": st.dev, "blob": st.blob})()
    cell = np.full((h, w), -1, np.int64)
    for j in range(h):
        for i in range(w):
            prim = int(hit_id[y0 + j, x0 + i])
            if prim not in (0, 1):  # (no spheres: primitives 0 and 1 are the receiver's triangles)
                continue
            cells = set()
            for dx, dy in ((0.0, 0.0), (-0.45, -0.45), (0.45, -0.45), (-0.45, 0.45), (0.45, 0.45)):  # the centre ray and the reach of the pixel's samples
                o = np.array([np.float32(x0 + i + dx) * np.float32(cfg.fw), np.float32(y0 + j + dy) * np.float32(cfg.fh), 0.0])
                p = o + (o - f) * (0.5 / (o[2] - f[2]))
                cells.add(flags_cases.receiver_cell(k, prim, p.astype(np.float32)))
            if len(cells) == 1 and None not in cells:
                cell[j, i] = cells.pop()
    return cell


def neighbours(cell):
    """pairs of different cells under pixels one or two apart in a row or a column"""
    out = set()
    for d in (1, 2):
        for a, b in ((cell[:, :-d], cell[:, d:]), (cell[:-d, :], cell[d:, :])):
            m = (a >= 0) & (b >= 0) & (a != b)
            out |= set(zip(a[m].tolist(), b[m].tolist()))
    return out


def check_plan(name, st, cell):
    """the cases the frames are there for, by the stages run on the scene as the render packs it"""
    used = sorted(set(cell[cell >= 0].tolist()))
    assert len(used) >= 4, f"{name}: the window covers several receiver cells"
    got = {c: st.marked_tris(c) for c in used}
    marked = {c: set(m) for c, (_, m) in got.items() if m}
    pairs = neighbours(cell)
    if name in ("across", "lights"):
        assert all(marked.get(c) == {2} for c in used), f"{name}: every cell under the window lists the pane as marked"
    if name == "lights":
        assert all(st.marked_tris(c, 1)[1] == [2] for c in used), "the second light's lists are marked too"
    if name == "edge":
        plain = {c for c in used if got[c][0] is not None and not got[c][1]}
        assert marked and plain and any((a in marked and b in plain) or (b in marked and a in plain) for a, b in pairs), "a marked cell next to an unmarked one"
        assert any(2 in got[c][0] for c in plain), "a cell that lists the pane unmarked: its edge cuts the beam"
    if name == "materials":
        assert any(m == {2, 3} for m in marked.values()), "two marked panes of two materials in one list"
    if name == "opaque":
        assert any(m == {2} and 3 in got[c][0] for c, m in marked.items()), "a marked pane and an opaque triangle in one list"
        assert any(a in marked and b in marked and (3 in got[a][0]) != (3 in got[b][0]) for a, b in pairs), "... next to a cell without the opaque one"
    if name == "quad":
        one = {c for c, m in marked.items() if len(m) == 1}
        none = {c for c in used if got[c][0] is not None and {2, 3} <= set(got[c][0]) and not got[c][1]}
        assert one and none, "cells with one half marked, cells on the diagonal with neither"
        assert {t for c in one for t in marked[c]} == {2, 3}, "each half is the marked one somewhere"
    if name == "wide":
        wide = {c for c in used if st.four[c, 0, 0] == OVERFLOW and st.four[c, 0, 1] == MARK}
        assert wide and marked and any((a in wide and b in marked) or (b in wide and a in marked) for a, b in pairs), "a wide record next to a list with marked entries"


@pytest.mark.gpu
def test_frames_are_the_same_with_the_marks_without_them_and_without_lists(tmp_path, probe):
    on, log_on = run_child(tmp_path, "on")
    off, log_off = run_child(tmp_path, "off")
    nolists, log_no = run_child(tmp_path, "nolists")
    assert "rt_primary_soft10_kernel: workgroups" in log_on and "rt_cell_through_kernel" in log_on, log_on[-2000:]
    assert "rt_primary_soft10_kernel: workgroups" in log_off and "rt_cell_through_kernel" not in log_off, log_off[-2000:]
    assert "rt_primary_soft10_flags_kernel: workgroups" in log_no and "rt_primary_soft10_kernel:" not in log_no, log_no[-2000:]  # (no list is read)
    cfg = frame_cfg()
    for name, flat in frame_scenes().items():
        a, b = np.load(on / f"{name}.npz"), np.load(off / f"{name}.npz")
        x0, y0, w, h = WIN
        hit = a["hit_id"].reshape(cfg.height, cfg.width)
        assert a["argb"].any() and (hit[y0:y0 + h, x0:x0 + w] >= 0).sum() > 3000, f"{name}: the receiver fills the window"
        pg.same(a, b, f"{name}: RT_CELL_THROUGH=0")
        pg.same(a, np.load(nolists / f"{name}.npz"), f"{name}: tuning.no_cell_lists")
        assert int(a["bytes_cell_lists"]) > int(b["bytes_cell_lists"]), f"{name}: the marks count in bytes_cell_lists, and RT_CELL_THROUGH=0 leaves them out"
        st = Stages(probe, cfg, flat, BUDGET)
        st.check(name)
        cell = cells_under_window(st, flat, cfg, hit)
        print(f"{name}: {int((hit >= 0).sum())} pixels hit, {np.unique(a['argb'][a['argb'] != 0]).size} distinct colours, {len(set(cell[cell >= 0].tolist()))} cells under the window")
        used = sorted(set(cell[cell >= 0].tolist()))
        head = st.four[used, 0, :2]
        print(f"  lists of those cells for light 0: empty {int((head[:, 0] == END).sum())}, short {int((head[:, 0] < OVERFLOW).sum())}, "
              f"wide {int(((head[:, 0] == OVERFLOW) & (head[:, 1] == MARK)).sum())}, plain overflowed {int(((head[:, 0] == OVERFLOW) & (head[:, 1] != MARK)).sum())}, "
              f"with a marked entry {int((st.dev_marks[used, 0] != 0).sum())}")
        check_plan(name, st, cell)


if __name__ == "__main__":
    child(sys.argv[1], sys.argv[2])
