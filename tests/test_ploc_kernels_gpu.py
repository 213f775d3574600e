"""The device half of "one specification, compiled twice" (csrc/rt_ploc.h), measured: the kernels of a PLOC rebuild
(csrc/rt_ploc.hip, the order kernels of csrc/rt_rebuild.hip, the sort and scan of csrc/rt_order.hip, the refit of
csrc/rt_update.hip) held word for word to rt_rebuild_ploc_packed, the host model that tests/test_ploc_host.py holds to a numpy
restatement.  The probe of tests/test_rebuild_kernels_gpu.py with one more function: it runs rt_rebuild_device with
method = RT_REBUILD_PLOC -- the function rt_scene_rebuild_with* itself runs, read-back batches included -- and reads back
every word of the new blob, the plan and the bounds.  All comparisons are array_equal on 32-bit words; only the case with a
NaN vertex asks for the exemption of tests/test_scene_update_kernels_gpu.py.  The plan's groups are compared group by group,
sorted: the device fills a group in the order its atomics land.  After any HIP error the probe starts nothing further."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ploc_cases as pc
from test_ploc_host import check_against_restatement, check_structure, prepared
from test_rebuild_host import declare, info_of, resize
from test_rebuild_kernels_gpu import PROBE_REBUILD, assert_plans_equal
from test_scene_pack_host import CSRC, HIPCC, ROOT, ptr
from test_scene_update_host import get, plan_of
from test_scene_update_kernels_gpu import PROBE, assert_device_equals_host, hip_ok
from hslu_i.ba_raytracing.f2501_raytracer_amd import _lib

gpu = pytest.mark.gpu

PROBE_PLOC = r'''
extern "C" {
int probe_rebuild_ploc(int k, uint32_t max_leaf, uint32_t radius, uint32_t* iterations) {
  return rt_rebuild_ploc_packed(&g[k], max_leaf, radius, iterations);
}
// the uploaded scene rebuilt on the device with PLOC; the device state becomes the rebuilt scene
int probe_rebuild_ploc_device(uint32_t max_leaf, uint32_t radius, uint32_t* iterations) {
  if (dead) return dead;
  if (D.slot < 0) return -100;
  int rc = rt_check_rebuild(D.up.dev);
  if (rc == RT_OK) rc = rt_check_ploc_radius(radius, &radius);
  if (rc != RT_OK) return rc;
  RtRebuildIn in{};
  in.dev = D.up.dev, in.dev.base = D.blob;
  in.recv_cell = D.plan[2], in.tri_slot = D.plan[3];
  in.max_leaf = rt_lbvh_max_leaf(max_leaf), in.n_materials = (uint32_t)D.up.plan.mat_class.size();
  in.method = RT_REBUILD_PLOC, in.radius = radius;
  RtRebuildOut o;
  rc = rt_rebuild_device(in, stream, &o);
  if (rc == RT_ERR_HIP || rc == RT_ERR_OOM) return dead = 1000;  // (sticky: nothing further is started)
  if (rc != RT_OK) return rc;
  *iterations = o.iterations;
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
    d = tmp_path_factory.mktemp("ploc_kernels_probe")
    src = d / "probe.cpp"
    src.write_text(PROBE + PROBE_REBUILD + PROBE_PLOC)
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
    before, plan_before, flat = prepared(probe, "soup_18")
    it = np.zeros(1, np.uint32)
    assert probe.probe_rebuild_ploc(0, 0, 0, ptr(it)) == 0, probe.probe_error()
    resize(probe, 0)
    after, plan_after = get(probe, 0, flat), plan_of(probe, 0)
    check_against_restatement(before, plan_before, after, plan_after, int(it[0]), 4, pc.RADIUS)
    check_structure(probe, before, plan_before, after, plan_after, flat)


def rebuild_both(probe, name, radius=0, max_leaf=0):
    """slot 0: the case, uploaded and rebuilt on the device (read back into slot 1); slot 2: the same through the host model"""
    before, plan_before, flat = prepared(probe, name)
    hip_ok(probe.probe_upload(0), "probe_upload")
    probe.probe_copy(0, 2)
    it_host, it_dev = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    assert probe.probe_rebuild_ploc(2, max_leaf, radius, ptr(it_host)) == 0, probe.probe_error()
    resize(probe, 2)
    host, plan_host = get(probe, 2, flat), plan_of(probe, 2)
    hip_ok(probe.probe_rebuild_ploc_device(max_leaf, radius, ptr(it_dev)), "probe_rebuild_ploc_device")
    hip_ok(probe.probe_download(1), "probe_download")
    resize(probe, 1)
    dev, plan_dev = get(probe, 1, flat), plan_of(probe, 1)
    return before, plan_before, flat, (dev, plan_dev, int(it_dev[0])), (host, plan_host, int(it_host[0]))


@gpu
@pytest.mark.parametrize("name,radius", pc.DEVICE)
def test_device_ploc_equals_the_host_model(probe, name, radius):
    before, plan_before, flat, (dev, plan_dev, it_dev), (host, plan_host, it_host) = rebuild_both(probe, name, radius)
    exempted = assert_device_equals_host(dev, host, nan_ok=(name == "nan_vertex"), what=name)
    assert_plans_equal(plan_dev, plan_host, name)
    assert it_dev == it_host, (it_dev, it_host)
    assert info_of(probe, 1) == info_of(probe, 2)
    if name == "copies_256":
        assert it_dev == pc.BATCH, "one cluster left exactly when the first read-back batch ends"
    if name == "copies_257":
        assert it_dev == pc.BATCH + 1, "... and one iteration into the second"
    if name == "heightfield":
        assert it_dev > 3 * pc.BATCH, "several read-back batches"
    # the device against the independent restatement directly, not only through the shared header (groups sorted)
    sorted_plan = dict(plan_dev)
    off = plan_dev["height_offset"].astype(np.int64)
    sorted_plan["height_nodes"] = np.concatenate([np.sort(plan_dev["height_nodes"][off[g]:off[g + 1]]) for g in range(len(off) - 1)])
    check_against_restatement(before, plan_before, dev, sorted_plan, it_dev, 4, radius or pc.RADIUS)
    print(f"{name} radius {radius or pc.RADIUS}: {it_dev} iterations, {dev.dev['n_nodes']} nodes, {len(dev.blob)} bytes equal; "
          f"{exempted} words NaN on both sides with different bits")


@gpu
@pytest.mark.parametrize("max_leaf", [1, 64])
def test_other_leaf_sizes_on_the_device(probe, max_leaf):
    before, plan_before, flat, (dev, plan_dev, it_dev), (host, plan_host, it_host) = rebuild_both(probe, "soup_100", max_leaf=max_leaf)
    assert_device_equals_host(dev, host, what=f"max_leaf {max_leaf}")
    assert_plans_equal(plan_dev, plan_host, f"max_leaf {max_leaf}")
    assert it_dev == it_host and dev.dev["n_nodes"] == (flat.n_triangles - 1 if max_leaf == 1 else dev.dev["n_nodes"])


@gpu
def test_zero_initialised_input_is_still_the_lbvh(probe):
    """RtRebuildIn.method = 0: the probe function of test_rebuild_kernels_gpu.py, which knows nothing of the new fields"""
    before, plan_before, flat = prepared(probe, "semesterbild")
    hip_ok(probe.probe_upload(0), "probe_upload")
    probe.probe_copy(0, 2)
    assert probe.probe_rebuild(2, 0) == 0, probe.probe_error()
    resize(probe, 2)
    hip_ok(probe.probe_rebuild_device(0), "probe_rebuild_device")
    hip_ok(probe.probe_download(1), "probe_download")
    resize(probe, 1)
    assert_device_equals_host(get(probe, 1, flat), get(probe, 2, flat), what="LBVH")
    assert_plans_equal(plan_of(probe, 1), plan_of(probe, 2), "LBVH")
