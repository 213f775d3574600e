// rt_pose.cpp -- the host side of device-side part poses (rt_pose*): validation (before any HIP call), the handle and its
// one device allocation, the launch of rt_pose_kernel, the delta handed to rt_scene_update_device, and the host model (the
// functions of rt_pose.h in loops).
//
// A pose is built ON TOP of the in-place update: it makes the arrays of an rt_scene_delta on the device and hands them to
// rt_scene_update_device through its public entry point, so every blocking, invalidation and refusal rule of an apply is
// that call's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "rt_host.h"
#include "rt_pose.h"

static_assert(sizeof(rt_transform) == 32, "a transform is 8 floats");

struct rt_pose {
  int device = 0;
  uint32_t n_parts = 0, n_triangles = 0, n_spheres = 0;
  bool has_spheres = false;       // some part has spheres: the sphere group travels with every apply
  RtPoseArrays a{};               // device pointers into `buf`
  DevBuf buf;                     // part tables, rest pose, posed arrays, the staged transforms
  rt_transform* xf_dev = nullptr;
  rt_transform* xf_stage = nullptr;  // pinned, [n_parts]
  hipEvent_t done_ev = nullptr;      // behind the last kernel enqueued for this pose
  bool pending = false;
};

namespace {

struct Cover {
  uint32_t lo = 0, n_cover = 0;
  bool has_spheres = false;
};

// the checks of an rt_pose_desc; no device needed
int check_desc(const rt_pose_desc* d, const char* fn, Cover* cover) {
  if (!d) return fail(RT_ERR_INVALID_ARG, "%s: null pose description", fn);
  if (d->abi_version != RT_ABI_VERSION) return fail(RT_ERR_INVALID_ARG, "%s: rt_pose_desc.abi_version %u != %u", fn, d->abi_version, RT_ABI_VERSION);
  if (d->n_parts == 0) return fail(RT_ERR_INVALID_ARG, "%s: n_parts is 0", fn);
  if (!d->parts) return fail(RT_ERR_INVALID_ARG, "%s: null parts", fn);
  if ((uint64_t)d->n_triangles + d->n_spheres >= ((uint64_t)1 << 31))
    return fail(RT_ERR_INVALID_ARG, "%s: n_triangles %u + n_spheres %u exceed 2^31 objects", fn, d->n_triangles, d->n_spheres);
  uint32_t lo = 0xFFFFFFFFu, hi = 0;
  bool tris = false, spheres = false;
  for (uint32_t p = 0; p < d->n_parts; p++) {
    const rt_pose_part& q = d->parts[p];
    if (q.tri_count == 0 && q.sphere_count == 0) return fail(RT_ERR_INVALID_ARG, "%s: part %u is empty (tri_count and sphere_count are 0)", fn, p);
    if (q.tri_count && (uint64_t)q.tri_first + q.tri_count > d->n_triangles)
      return fail(RT_ERR_INVALID_ARG, "%s: part %u: tri_first %u + tri_count %u > n_triangles %u", fn, p, q.tri_first, q.tri_count, d->n_triangles);
    if (q.sphere_count && (uint64_t)q.sphere_first + q.sphere_count > d->n_spheres)
      return fail(RT_ERR_INVALID_ARG, "%s: part %u: sphere_first %u + sphere_count %u > n_spheres %u", fn, p, q.sphere_first, q.sphere_count,
                  d->n_spheres);
    if (q.tri_count) tris = true, lo = std::min(lo, q.tri_first), hi = std::max(hi, q.tri_first + q.tri_count);
    if (q.sphere_count) spheres = true;
  }
  for (int kind = 0; kind < 2; kind++) {  // pairwise disjoint: sorted by start, each range ends before the next begins
    std::vector<std::pair<uint32_t, uint32_t>> r;
    for (uint32_t p = 0; p < d->n_parts; p++) {
      const rt_pose_part& q = d->parts[p];
      if (kind ? q.sphere_count : q.tri_count) r.push_back(kind ? std::make_pair(q.sphere_first, q.sphere_count) : std::make_pair(q.tri_first, q.tri_count));
    }
    std::sort(r.begin(), r.end());
    for (size_t k = 1; k < r.size(); k++)
      if ((uint64_t)r[k - 1].first + r[k - 1].second > r[k].first)
        return fail(RT_ERR_INVALID_ARG, "%s: %s ranges overlap: [%u, +%u) and [%u, +%u)", fn, kind ? "sphere" : "triangle", r[k - 1].first,
                    r[k - 1].second, r[k].first, r[k].second);
  }
  if (tris && (!d->tri_v1 || !d->tri_v2 || !d->tri_v3 || !d->tri_normal))
    return fail(RT_ERR_INVALID_ARG, "%s: a part has triangles: tri_v1, tri_v2, tri_v3 and tri_normal are all required", fn);
  if (spheres && (!d->sphere_center || !d->sphere_radius))
    return fail(RT_ERR_INVALID_ARG, "%s: a part has spheres: sphere_center and sphere_radius are required", fn);
  cover->lo = tris ? lo : 0u, cover->n_cover = tris ? hi - lo : 0u, cover->has_spheres = spheres;
  return RT_OK;
}

// the part of every triangle of the covering range and of every sphere
void part_tables(const rt_pose_desc* d, const Cover& c, std::vector<uint32_t>* tri_part, std::vector<uint32_t>* sphere_part) {
  tri_part->assign(c.n_cover, RT_POSE_NONE);
  sphere_part->assign(c.has_spheres ? d->n_spheres : 0u, RT_POSE_NONE);
  for (uint32_t p = 0; p < d->n_parts; p++) {
    const rt_pose_part& q = d->parts[p];
    for (uint32_t k = 0; k < q.tri_count; k++) (*tri_part)[q.tri_first - c.lo + k] = p;
    for (uint32_t k = 0; k < q.sphere_count; k++) (*sphere_part)[q.sphere_first + k] = p;
  }
}

int check_transforms(const rt_transform* t, uint32_t n, const char* fn) {
  for (uint32_t p = 0; p < n; p++) {
    const float* q = (const float*)(t + p);
    for (int k = 0; k < 8; k++)
      if (!rt_finite(q[k])) return fail(RT_ERR_INVALID_ARG, "%s: transform %u has a non-finite member", fn, p);
  }
  return RT_OK;
}

void pose_free(rt_pose* p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  if (p->pending) (void)hipEventSynchronize(p->done_ev);
  if (p->done_ev) (void)hipEventDestroy(p->done_ev);
  if (p->xf_stage) (void)hipHostFree(p->xf_stage);
  p->buf.release();
  delete p;
}

int pose_wait(rt_pose* p) {
  if (p->pending) {
    HIP_TRY(hipEventSynchronize(p->done_ev));
    p->pending = false;
  }
  return RT_OK;
}

int kernel_enqueue(rt_pose* p, const rt_transform* transforms_dev, hipStream_t stream) {
  const hipError_t e = (hipError_t)rt_launch_pose(p->a, transforms_dev, stream);
  if (e != hipSuccess) return fail(RT_ERR_HIP, "pose kernel launch failed: %s", hipGetErrorString(e));
  HIP_TRY(hipEventRecord(p->done_ev, stream));
  p->pending = true;
  return RT_OK;
}

// what an apply refuses itself, before any HIP call, and the delta it hands on
int check_apply(const rt_scene* s, const rt_pose* p, const rt_transform* t, const char* fn, rt_scene_delta* delta) {
  if (!s) return fail(RT_ERR_INVALID_ARG, "%s: null scene", fn);
  if (!p) return fail(RT_ERR_INVALID_ARG, "%s: null pose", fn);
  if (!t) return fail(RT_ERR_INVALID_ARG, "%s: null transforms", fn);
  if (p->n_triangles != s->dev.n_triangles || p->n_spheres != s->dev.n_spheres)
    return fail(RT_ERR_INVALID_ARG, "%s: the pose is for %u triangles and %u spheres, the scene has %u and %u", fn, p->n_triangles, p->n_spheres,
                s->dev.n_triangles, s->dev.n_spheres);
  if (p->device != s->device) return fail(RT_ERR_INVALID_ARG, "%s: the pose lives on device %d, the scene on device %d", fn, p->device, s->device);
  rt_scene_delta d{};
  d.abi_version = RT_ABI_VERSION;
  if (p->a.n_cover) {
    d.tri_first = p->a.lo, d.tri_count = p->a.n_cover;
    d.tri_v1 = p->a.o_v1, d.tri_e1 = p->a.o_e1, d.tri_e2 = p->a.o_e2, d.tri_normal = p->a.o_normal;
  }
  if (p->has_spheres) d.sphere_center = p->a.o_centre, d.sphere_r_sq = p->a.o_r_sq, d.sphere_r_inv = p->a.o_r_inv;
  // rt_scene_update_device's own refusals, made here too so that a refused apply has not run the kernel
  if (s->progress_active) return fail(RT_ERR_INVALID_ARG, "a progressive render owns this scene until rt_render_end");
  const int rc = rt_check_scene_delta(s->dev, s->plan, &d, nullptr);
  if (rc != RT_OK) return rc;
  *delta = d;
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_pose_create(const rt_pose_desc* d, int device, rt_pose** out) {
  const char* fn = "rt_pose_create";
  if (!d || !out) return fail(RT_ERR_INVALID_ARG, "%s: null argument", fn);
  *out = nullptr;
  Cover c;
  int rc = check_desc(d, fn, &c);
  if (rc != RT_OK) return rc;
  const int ndev = rt_device_count();
  if (ndev <= 0) return fail(RT_ERR_NO_DEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(RT_ERR_INVALID_ARG, "device %d out of range (%d visible)", device, ndev);
  HIP_TRY(hipSetDevice(device));
  rt_pose* p = new rt_pose();
  p->device = device, p->n_parts = d->n_parts, p->n_triangles = d->n_triangles, p->n_spheres = d->n_spheres, p->has_spheres = c.has_spheres;
  // one host image of the allocation, every array on a multiple of 256 bytes, uploaded in one copy
  const size_t nc = c.n_cover, ns = c.has_spheres ? d->n_spheres : 0u;
  const size_t t1 = rt_pad256(nc * 4), t3 = rt_pad256(nc * 12), s1 = rt_pad256(ns * 4), s3 = rt_pad256(ns * 12), xf = rt_pad256((size_t)d->n_parts * 32);
  const size_t total = t1 + 8 * t3 + s1 + 2 * s3 + 3 * s1 + xf;
  std::vector<unsigned char> img(total, 0);
  size_t used = 0;
  auto take = [&](size_t bytes) {
    unsigned char* at = img.data() + used;
    used += bytes;
    return at;
  };
  uint32_t* tri_part = (uint32_t*)take(t1);
  float *v1 = (float*)take(t3), *v2 = (float*)take(t3), *v3 = (float*)take(t3), *nrm = (float*)take(t3);
  float *o_v1 = (float*)take(t3), *o_e1 = (float*)take(t3), *o_e2 = (float*)take(t3), *o_n = (float*)take(t3);
  uint32_t* sphere_part = (uint32_t*)take(s1);
  float *centre = (float*)take(s3), *radius = (float*)take(s1);
  float *o_c = (float*)take(s3), *o_rsq = (float*)take(s1), *o_rinv = (float*)take(s1);
  unsigned char* xf_at = take(xf);
  std::vector<uint32_t> tp, sp;
  part_tables(d, c, &tp, &sp);
  if (nc) {
    memcpy(tri_part, tp.data(), nc * 4);
    memcpy(v1, d->tri_v1 + 3 * (size_t)c.lo, nc * 12), memcpy(v2, d->tri_v2 + 3 * (size_t)c.lo, nc * 12);
    memcpy(v3, d->tri_v3 + 3 * (size_t)c.lo, nc * 12), memcpy(nrm, d->tri_normal + 3 * (size_t)c.lo, nc * 12);
  }
  if (ns) memcpy(sphere_part, sp.data(), ns * 4), memcpy(centre, d->sphere_center, ns * 12), memcpy(radius, d->sphere_radius, ns * 4);
  RtPoseArrays host{c.lo, (uint32_t)nc, (uint32_t)ns, tri_part, sphere_part, v1, v2, v3, nrm, centre, radius, o_v1, o_e1, o_e2, o_n, o_c, o_rsq, o_rinv};
  for (uint32_t k = 0; k < nc; k++) rt_pose_tri(host, k, nullptr);  // the posed arrays start as the rest pose
  for (uint32_t i = 0; i < ns; i++) rt_pose_sphere(host, i, nullptr);
  rc = p->buf.ensure(total);
  if (rc == RT_OK) {
    const hipError_t e = hipMemcpy(p->buf.p, img.data(), total, hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = fail(RT_ERR_HIP, "hipMemcpy H2D failed: %s", hipGetErrorString(e));
  }
  if (rc == RT_OK && hipHostMalloc((void**)&p->xf_stage, (size_t)d->n_parts * 32, hipHostMallocDefault) != hipSuccess)
    p->xf_stage = nullptr, rc = fail(RT_ERR_OOM, "hipHostMalloc(%zu) failed", (size_t)d->n_parts * 32);
  if (rc == RT_OK && hipEventCreate(&p->done_ev) != hipSuccess) p->done_ev = nullptr, rc = fail(RT_ERR_HIP, "hipEventCreate failed");
  if (rc != RT_OK) {
    pose_free(p);
    return rc;
  }
  char* base = (char*)p->buf.p;
  auto dev = [&](const void* host_at) { return base + ((const unsigned char*)host_at - img.data()); };
  p->a = RtPoseArrays{c.lo, (uint32_t)nc, (uint32_t)ns, (const uint32_t*)dev(tri_part), (const uint32_t*)dev(sphere_part),
                      (const float*)dev(v1), (const float*)dev(v2), (const float*)dev(v3), (const float*)dev(nrm),
                      (const float*)dev(centre), (const float*)dev(radius), (float*)dev(o_v1), (float*)dev(o_e1), (float*)dev(o_e2),
                      (float*)dev(o_n), (float*)dev(o_c), (float*)dev(o_rsq), (float*)dev(o_rinv)};
  p->xf_dev = (rt_transform*)dev(xf_at);
  *out = p;
  return RT_OK;
}

void rt_pose_destroy(rt_pose* p) { pose_free(p); }

int rt_pose_geometry_device(rt_pose* p, const rt_transform* transforms_dev, void* hip_stream) {
  const char* fn = "rt_pose_geometry_device";
  if (!p) return fail(RT_ERR_INVALID_ARG, "%s: null pose", fn);
  if (!transforms_dev) return fail(RT_ERR_INVALID_ARG, "%s: null transforms", fn);
  HIP_TRY(hipSetDevice(p->device));
  return kernel_enqueue(p, transforms_dev, (hipStream_t)hip_stream);
}

int rt_pose_apply_device(rt_scene* s, rt_pose* p, const rt_transform* transforms_dev, void* hip_stream, rt_update_info* info) {
  rt_scene_delta d;
  int rc = check_apply(s, p, transforms_dev, "rt_pose_apply_device", &d);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(p->device));
  if ((rc = kernel_enqueue(p, transforms_dev, (hipStream_t)hip_stream)) != RT_OK) return rc;
  rc = rt_scene_update_device(s, &d, hip_stream, info);  // (blocks: the stream has drained)
  if (rc == RT_OK) p->pending = false;
  return rc;
}

int rt_pose_apply(rt_scene* s, rt_pose* p, const rt_transform* transforms_host, rt_update_info* info) {
  const char* fn = "rt_pose_apply";
  rt_scene_delta d;
  int rc = check_apply(s, p, transforms_host, fn, &d);
  if (rc == RT_OK) rc = check_transforms(transforms_host, p->n_parts, fn);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(p->device));
  if ((rc = pose_wait(p)) != RT_OK) return rc;  // (a kernel still in flight reads the staged transforms)
  memcpy(p->xf_stage, transforms_host, (size_t)p->n_parts * 32);
  HIP_TRY(hipMemcpyAsync(p->xf_dev, p->xf_stage, (size_t)p->n_parts * 32, hipMemcpyHostToDevice, nullptr));
  if ((rc = kernel_enqueue(p, p->xf_dev, nullptr)) != RT_OK) return rc;
  rc = rt_scene_update_device(s, &d, nullptr, info);
  if (rc == RT_OK) p->pending = false;
  return rc;
}

int rt_pose_read(rt_pose* p, float* tri_v1, float* tri_e1, float* tri_e2, float* tri_normal, uint32_t* tri_first, uint32_t* tri_count,
                 float* sphere_center, float* sphere_r_sq, float* sphere_r_inv) {
  if (!p) return fail(RT_ERR_INVALID_ARG, "rt_pose_read: null pose");
  HIP_TRY(hipSetDevice(p->device));
  const int rc = pose_wait(p);
  if (rc != RT_OK) return rc;
  const size_t nc = p->a.n_cover, ns = p->a.n_spheres;
  if (tri_first) *tri_first = p->a.lo;
  if (tri_count) *tri_count = p->a.n_cover;
  const struct {
    float* host;
    const float* dev;
    size_t bytes;
  } arrays[7] = {{tri_v1, p->a.o_v1, nc * 12},  {tri_e1, p->a.o_e1, nc * 12},      {tri_e2, p->a.o_e2, nc * 12},     {tri_normal, p->a.o_normal, nc * 12},
                 {sphere_center, p->a.o_centre, ns * 12}, {sphere_r_sq, p->a.o_r_sq, ns * 4}, {sphere_r_inv, p->a.o_r_inv, ns * 4}};
  for (const auto& a : arrays)
    if (a.host && a.bytes) HIP_TRY(hipMemcpy(a.host, a.dev, a.bytes, hipMemcpyDeviceToHost));
  return RT_OK;
}

int rt_pose_model(const rt_pose_desc* d, const rt_transform* transforms, float* tri_v1, float* tri_e1, float* tri_e2, float* tri_normal,
                  float* sphere_center, float* sphere_r_sq, float* sphere_r_inv) {
  const char* fn = "rt_pose_model";
  Cover c;
  const int rc = check_desc(d, fn, &c);
  if (rc != RT_OK) return rc;
  if (!transforms) return fail(RT_ERR_INVALID_ARG, "%s: null transforms", fn);
  std::vector<uint32_t> tp, sp;
  part_tables(d, c, &tp, &sp);
  const size_t nc = c.n_cover, ns = sp.size();
  // outputs the caller does not want land in scratch arrays
  std::vector<float> scratch[7];
  float* o[7] = {tri_v1, tri_e1, tri_e2, tri_normal, sphere_center, sphere_r_sq, sphere_r_inv};
  const size_t floats[7] = {3 * nc, 3 * nc, 3 * nc, 3 * nc, 3 * ns, ns, ns};
  for (int k = 0; k < 7; k++)
    if (!o[k]) scratch[k].resize(floats[k] + 1), o[k] = scratch[k].data();
  const size_t off = 3 * (size_t)c.lo;
  const RtPoseArrays a{c.lo, (uint32_t)nc, (uint32_t)ns, tp.data(), sp.data(),
                       nc ? d->tri_v1 + off : nullptr, nc ? d->tri_v2 + off : nullptr, nc ? d->tri_v3 + off : nullptr, nc ? d->tri_normal + off : nullptr,
                       d->sphere_center, d->sphere_radius, o[0], o[1], o[2], o[3], o[4], o[5], o[6]};
  for (uint32_t k = 0; k < nc; k++) rt_pose_tri(a, k, tp[k] == RT_POSE_NONE ? nullptr : (const float*)(transforms + tp[k]));
  for (uint32_t i = 0; i < ns; i++) rt_pose_sphere(a, i, sp[i] == RT_POSE_NONE ? nullptr : (const float*)(transforms + sp[i]));
  return RT_OK;
}

}  // extern "C"
