"""The device half of "one specification, compiled twice" (csrc/rt_lbvh.h), measured: the kernels of a BVH rebuild
(csrc/rt_rebuild.hip, the sort and scan of csrc/rt_order.hip, the refit of csrc/rt_update.hip) held word for word to
rt_rebuild_packed, the host model that tests/test_rebuild_host.py holds to numpy restatements.  The probe of
tests/test_scene_update_kernels_gpu.py, extended: it links against the built librt_hip.so, uploads a packed scene, runs
rt_rebuild_device -- the function rt_scene_rebuild* itself runs, so the launches driven here are the ones that ship -- and
reads back every word of the new blob, the plan and the bounds.  All comparisons are array_equal on 32-bit words; only the
case with a NaN vertex asks for that file's exemption (two words that are both NaN as fp32, inside float words).  The plan's
groups are compared group by group, sorted: the device fills a group in the order its atomics land."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rebuild_cases as rc
from test_rebuild_host import check_rebuilt, declare, info_of, prepared, rebuilt, resize
from test_scene_pack_host import CSRC, HIPCC, ROOT
from test_scene_update_host import get, plan_of
from test_scene_update_kernels_gpu import PROBE, assert_device_equals_host, hip_ok
from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, _lib

gpu = pytest.mark.gpu

PROBE_REBUILD = r'''
#include "rt_host.h"
#include "rt_lbvh.h"
#include "rt_sah.h"
extern "C" {
int probe_rebuild(int k, uint32_t max_leaf) { return rt_rebuild_packed(&g[k], max_leaf); }
void probe_sizes(int k, uint64_t* sizes) {
  const RtRefitPlan& p = g[k].plan;
  sizes[0] = g[k].blob.size(), sizes[1] = g[k].flag_geo.size(), sizes[2] = p.height_nodes.size(), sizes[3] = p.height_offset.size();
  sizes[4] = p.thr_src.size(), sizes[5] = p.recv_cell.size(), sizes[6] = p.tri_slot.size(), sizes[7] = p.mat_class.size();
}
void probe_info(int k, uint64_t* out) {
  const rt_bvh_info& i = g[k].info;
  out[0] = i.n_nodes, out[1] = i.n_leaves, out[2] = i.max_depth, out[3] = i.max_leaf_size, out[4] = i.n_references;
  out[5] = i.bytes_nodes, out[6] = i.bytes_triangles, out[7] = g[k].bytes_bvh, out[8] = g[k].max_leaf;
}
void probe_sah(int k, uint64_t* sums, uint32_t* n_bad) { rt_sah_packed(g[k], sums, n_bad); }
// the uploaded scene rebuilt on the device; the device state becomes the rebuilt scene
int probe_rebuild_device(uint32_t max_leaf) {
  if (dead) return dead;
  if (D.slot < 0) return -100;
  int rc = rt_check_rebuild(D.up.dev);
  if (rc != RT_OK) return rc;
  RtRebuildIn in{};
  in.dev = D.up.dev, in.dev.base = D.blob;
  in.recv_cell = D.plan[2], in.tri_slot = D.plan[3];
  in.max_leaf = rt_lbvh_max_leaf(max_leaf), in.n_materials = (uint32_t)D.up.plan.mat_class.size();
  RtRebuildOut o;
  rc = rt_rebuild_device(in, stream, &o);
  if (rc == RT_ERR_HIP || rc == RT_ERR_OOM) return dead = 1000;  // (sticky: nothing further is started)
  if (rc != RT_OK) return rc;
  const size_t part[4] = {o.height_nodes.size() * 4, o.thr_src.size() * 4, D.up.plan.recv_cell.size() * 4, o.tri_slot.size() * 4};
  uint32_t* fresh[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int i = 0; i < 4; i++)
    if (part[i]) {
      TRY(hipMalloc((void**)&fresh[i], part[i]));
      TRY(hipMemcpy(fresh[i], (const char*)o.plan_dev.p + o.plan_off[i], part[i], hipMemcpyDeviceToDevice));
    }
  TRY(hipMemcpy(D.bounds, (const char*)o.plan_dev.p + o.plan_off[4], 32, hipMemcpyDeviceToDevice));
  TRY(hipFree(D.blob));
  for (int i = 0; i < 4; i++)
    if (D.plan[i]) TRY(hipFree(D.plan[i]));
  TRY(hipFree(o.plan_dev.p));
  D.blob = (char*)o.blob.p;
  for (int i = 0; i < 4; i++) D.plan[i] = fresh[i];
  D.bounds_live = true;
  RtPackedScene& up = D.up;
  up.blob.assign(o.blob.cap, 0);
  up.dev = o.dev, up.dev.base = nullptr;
  up.plan.height_nodes = o.height_nodes, up.plan.thr_src = o.thr_src, up.plan.tri_slot = o.tri_slot;
  up.plan.height_offset = o.shape.group_offset;
  rt_rebuild_info_of(o.shape, up.dev.n_triangles, &up.info, &up.bytes_bvh);
  return 0;
}
}
'''


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("rebuild_kernels_probe")
    src = d / "probe.cpp"
    src.write_text(PROBE + PROBE_REBUILD)
    so = d / "probe.so"
    lib_dir, lib_name = os.path.split(os.path.abspath(_lib.LIB_PATH))
    out = subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip", "--cuda-host-only", "-I", CSRC,
                          "-I", os.path.join(ROOT, "include"), "-shared", "-o", str(so), str(src),
                          "-L", lib_dir, f"-l:{lib_name}", f"-Wl,-rpath,{lib_dir}"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lib = declare(C.CDLL(str(so)))
    yield lib
    lib.probe_release()


def test_the_probe_builds_against_the_library(probe):
    """without a GPU: the probe links, and the library's host model is the one of the host tests"""
    before, plan_before, flat = prepared(probe, "max_leaf_plus_1")
    after, plan_after = rebuilt(probe, flat)
    check_rebuilt(probe, before, plan_before, after, plan_after, flat)


def rebuild_both(probe, name, max_leaf=0):
    """slot 0: the case, uploaded and rebuilt on the device (read back into slot 1); slot 2: the same through the host model"""
    before, plan_before, flat = prepared(probe, name)
    hip_ok(probe.probe_upload(0), "probe_upload")
    probe.probe_copy(0, 2)
    assert probe.probe_rebuild(2, max_leaf) == 0, probe.probe_error()
    resize(probe, 2)
    host, plan_host = get(probe, 2, flat), plan_of(probe, 2)
    hip_ok(probe.probe_rebuild_device(max_leaf), "probe_rebuild_device")
    hip_ok(probe.probe_download(1), "probe_download")
    resize(probe, 1)
    dev, plan_dev = get(probe, 1, flat), plan_of(probe, 1)
    return before, plan_before, flat, (dev, plan_dev), (host, plan_host)


def assert_plans_equal(plan_dev, plan_host, what):
    for part in ("height_offset", "thr_src", "recv_cell", "tri_slot", "mat_class"):
        assert np.array_equal(plan_dev[part], plan_host[part]), f"{what}: {part}"
    off = plan_host["height_offset"].astype(np.int64)
    for g in range(len(off) - 1):
        assert np.array_equal(np.sort(plan_dev["height_nodes"][off[g]:off[g + 1]]), np.sort(plan_host["height_nodes"][off[g]:off[g + 1]])), f"{what}: group {g}"


@gpu
@pytest.mark.parametrize("name", rc.ALL)
def test_device_rebuild_equals_the_host_model(probe, name):
    before, plan_before, flat, (dev, plan_dev), (host, plan_host) = rebuild_both(probe, name)
    exempted = assert_device_equals_host(dev, host, nan_ok=(name == "nan_vertex"), what=name)
    assert_plans_equal(plan_dev, plan_host, name)
    assert info_of(probe, 1) == info_of(probe, 2)
    # the device against the independent restatements directly, not only through the shared header
    check_rebuilt(probe, before, plan_before, dev, plan_dev, flat, k=1)
    print(f"{name}: {dev.dev['n_nodes']} nodes, {len(dev.blob)} bytes equal; {exempted} words NaN on both sides with different bits")


@gpu
@pytest.mark.parametrize("max_leaf", [1, 64])
def test_other_leaf_sizes_on_the_device(probe, max_leaf):
    before, plan_before, flat, (dev, plan_dev), (host, plan_host) = rebuild_both(probe, "heightfield", max_leaf)
    assert_device_equals_host(dev, host, what=f"max_leaf {max_leaf}")
    assert_plans_equal(plan_dev, plan_host, f"max_leaf {max_leaf}")
    assert dev.dev["n_nodes"] == (flat.n_triangles - 1 if max_leaf == 1 else dev.dev["n_nodes"])


@gpu
def test_rebuild_then_update_then_rebuild_on_one_device_state(probe):
    """the rebuilt state is a scene like any other: a jitter through the update kernels, then a second rebuild, the host model alongside"""
    import scene_update_cases as cases
    from test_scene_update_host import refit
    from test_scene_update_kernels_gpu import update_device

    before, plan_before, flat, (dev, plan_dev), (host, plan_host) = rebuild_both(probe, "semesterbild")
    probe.probe_copy(2, 0)  # (slot 0, which the update probe takes layout and plan from, := the rebuilt scene)
    resize(probe, 0)
    probe._uploaded = 0
    new = cases.jitter(flat, 0.05)
    hip_ok(update_device(probe, flat, new), "probe_update_device")
    assert refit(probe, 2, flat, new) == 0, probe.probe_error()
    hip_ok(probe.probe_download(1), "probe_download")
    assert_device_equals_host(get(probe, 1, new), get(probe, 2, new), what="jitter on the rebuilt tree")
    mid, plan_mid = get(probe, 2, new), plan_of(probe, 2)
    assert probe.probe_rebuild(2, 0) == 0, probe.probe_error()
    resize(probe, 2)
    hip_ok(probe.probe_rebuild_device(0), "probe_rebuild_device")
    hip_ok(probe.probe_download(1), "probe_download")
    resize(probe, 1)
    dev2, host2 = get(probe, 1, new), get(probe, 2, new)
    assert_device_equals_host(dev2, host2, what="second rebuild")
    assert_plans_equal(plan_of(probe, 1), plan_of(probe, 2), "second rebuild")
    check_rebuilt(probe, mid, plan_mid, dev2, plan_of(probe, 1), new, k=1)


@gpu
def test_refusals_reach_no_kernel(probe):
    from test_scene_pack_host import mesh_with_glass
    from test_scene_update_host import pack

    flat = mesh_with_glass().contiguous()
    a = pack(probe, 0, flat, bvh=dict(split_depth=8, split_gain=0.99))
    hip_ok(probe.probe_upload(0), "probe_upload")
    assert probe.probe_rebuild_device(0) == _abi.RT_ERR_UNSUPPORTED and b"split clipping" in probe.probe_error()
    hip_ok(probe.probe_download(1), "probe_download")
    probe._sizes[1] = probe._sizes[0]
    assert_device_equals_host(get(probe, 1, flat), a, what="the device state after the refusal")
