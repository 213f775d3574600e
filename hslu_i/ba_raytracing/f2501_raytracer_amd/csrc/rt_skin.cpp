// rt_skin.cpp -- the host side of device-side skinned meshes (rt_skin*): validation (before any HIP call), the handle and its
// one device allocation, the launch of the two kernels, the delta handed to rt_scene_update_device, and the host model (the
// functions of rt_skin.h in loops).
//
// A skin is built ON TOP of the in-place update, as a pose is (rt_pose.cpp): it makes the triangle arrays of an
// rt_scene_delta on the device and hands them to rt_scene_update_device through its public entry point, so every blocking,
// invalidation and refusal rule of an apply is that call's.
#include <hip/hip_runtime.h>

#include <cstring>

#include "rt_host.h"
#include "rt_skin.h"

static_assert(sizeof(rt_transform) == 32, "a bone is 8 floats");
static_assert(sizeof(RtSkinBones) == 8 && sizeof(RtSkinWeights) == 16, "one 8-byte and one 16-byte load per vertex");

struct rt_skin {
  int device = 0;
  uint32_t n_bones = 0, n_triangles = 0, tri_first = 0;
  RtSkinArrays a{};               // device pointers into `buf`
  DevBuf buf;                     // rest mesh, tables, skinned vertices, posed triangle arrays, the staged bones
  rt_transform* xf_dev = nullptr;
  rt_transform* xf_stage = nullptr;  // pinned, [n_bones]
  hipEvent_t done_ev = nullptr;      // behind the last kernel enqueued for this skin
  bool pending = false;
};

namespace {

// the checks of an rt_skin_desc; no device needed
int check_desc(const rt_skin_desc* d, const char* fn) {
  if (!d) return fail(RT_ERR_INVALID_ARG, "%s: null skin description", fn);
  if (d->abi_version != RT_ABI_VERSION) return fail(RT_ERR_INVALID_ARG, "%s: rt_skin_desc.abi_version %u != %u", fn, d->abi_version, RT_ABI_VERSION);
  if (d->n_vertices == 0) return fail(RT_ERR_INVALID_ARG, "%s: n_vertices is 0", fn);
  if (d->n_vertices >= (1u << 31)) return fail(RT_ERR_INVALID_ARG, "%s: n_vertices %u exceeds 2^31 - 1", fn, d->n_vertices);
  if (d->n_bones == 0) return fail(RT_ERR_INVALID_ARG, "%s: n_bones is 0", fn);
  if (d->n_bones > 65536u) return fail(RT_ERR_INVALID_ARG, "%s: n_bones %u > 65536 (a bone index is 16 bits)", fn, d->n_bones);
  if (d->tri_count == 0) return fail(RT_ERR_INVALID_ARG, "%s: tri_count is 0", fn);
  if (d->n_triangles >= (1u << 31)) return fail(RT_ERR_INVALID_ARG, "%s: n_triangles %u exceeds 2^31 - 1", fn, d->n_triangles);
  if ((uint64_t)d->tri_first + d->tri_count > d->n_triangles)
    return fail(RT_ERR_INVALID_ARG, "%s: tri_first %u + tri_count %u > n_triangles %u", fn, d->tri_first, d->tri_count, d->n_triangles);
  if (!d->position) return fail(RT_ERR_INVALID_ARG, "%s: null position", fn);
  if (!d->indices) return fail(RT_ERR_INVALID_ARG, "%s: null indices", fn);
  if (!d->bone) return fail(RT_ERR_INVALID_ARG, "%s: null bone", fn);
  if (!d->weight) return fail(RT_ERR_INVALID_ARG, "%s: null weight", fn);
  for (uint32_t t = 0; t < d->tri_count; t++)
    for (int c = 0; c < 3; c++)
      if (d->indices[3 * (size_t)t + c] >= d->n_vertices)
        return fail(RT_ERR_INVALID_ARG, "%s: indices of triangle %u: %u >= n_vertices %u", fn, t, d->indices[3 * (size_t)t + c], d->n_vertices);
  for (uint32_t i = 0; i < d->n_vertices; i++)
    for (int k = 0; k < RT_SKIN_INFLUENCES; k++) {
      const size_t at = RT_SKIN_INFLUENCES * (size_t)i + k;
      if (d->bone[at] >= d->n_bones) return fail(RT_ERR_INVALID_ARG, "%s: bone of vertex %u, slot %d: %u >= n_bones %u", fn, i, k, d->bone[at], d->n_bones);
      if (!rt_finite(d->weight[at])) return fail(RT_ERR_INVALID_ARG, "%s: weight of vertex %u, slot %d is not finite", fn, i, k);
    }
  return RT_OK;
}

int check_bones(const rt_transform* t, uint32_t n, const char* fn) {
  for (uint32_t b = 0; b < n; b++) {
    const float* q = (const float*)(t + b);
    for (int k = 0; k < 8; k++)
      if (!rt_finite(q[k])) return fail(RT_ERR_INVALID_ARG, "%s: bone %u has a non-finite member", fn, b);
  }
  return RT_OK;
}

// the whole mesh through the formulas on the host (bones null: the rest mesh through the triangle formula)
void skin_on_host(const RtSkinArrays& a, const float* bones) {
  for (uint32_t i = 0; i < a.n_vertices; i++) rt_skin_vertex(a, i, bones);
  for (uint32_t t = 0; t < a.n_tris; t++) a.normal ? rt_skin_tri(a, t) : rt_skin_face(a, t);
}

void skin_free(rt_skin* p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  if (p->pending) (void)hipEventSynchronize(p->done_ev);
  if (p->done_ev) (void)hipEventDestroy(p->done_ev);
  if (p->xf_stage) (void)hipHostFree(p->xf_stage);
  p->buf.release();
  delete p;
}

int skin_wait(rt_skin* p) {
  if (p->pending) {
    HIP_TRY(hipEventSynchronize(p->done_ev));
    p->pending = false;
  }
  return RT_OK;
}

int kernel_enqueue(rt_skin* p, const rt_transform* bones_dev, hipStream_t stream) {
  const hipError_t e = (hipError_t)rt_launch_skin(p->a, bones_dev, stream);
  if (e != hipSuccess) return fail(RT_ERR_HIP, "skin kernel launch failed: %s", hipGetErrorString(e));
  HIP_TRY(hipEventRecord(p->done_ev, stream));
  p->pending = true;
  return RT_OK;
}

// what an apply refuses itself, before any HIP call, and the delta it hands on
int check_apply(const rt_scene* s, const rt_skin* p, const rt_transform* t, const char* fn, rt_scene_delta* delta) {
  if (!s) return fail(RT_ERR_INVALID_ARG, "%s: null scene", fn);
  if (!p) return fail(RT_ERR_INVALID_ARG, "%s: null skin", fn);
  if (!t) return fail(RT_ERR_INVALID_ARG, "%s: null bones", fn);
  if (p->n_triangles != s->dev.n_triangles)
    return fail(RT_ERR_INVALID_ARG, "%s: the skin is for n_triangles %u, the scene has %u", fn, p->n_triangles, s->dev.n_triangles);
  if (p->device != s->device) return fail(RT_ERR_INVALID_ARG, "%s: the skin lives on device %d, the scene on device %d", fn, p->device, s->device);
  rt_scene_delta d{};
  d.abi_version = RT_ABI_VERSION;
  d.tri_first = p->tri_first, d.tri_count = p->a.n_tris;
  d.tri_v1 = p->a.o_v1, d.tri_e1 = p->a.o_e1, d.tri_e2 = p->a.o_e2, d.tri_normal = p->a.o_normal;
  // rt_scene_update_device's own refusals, made here too so that a refused apply has not run the kernels
  if (s->progress_active) return fail(RT_ERR_INVALID_ARG, "a progressive render owns this scene until rt_render_end");
  const int rc = rt_check_scene_delta(s->dev, s->plan, &d, nullptr);
  if (rc != RT_OK) return rc;
  *delta = d;
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_skin_create(const rt_skin_desc* d, int device, rt_skin** out) {
  const char* fn = "rt_skin_create";
  if (!d || !out) return fail(RT_ERR_INVALID_ARG, "%s: null argument", fn);
  *out = nullptr;
  int rc = check_desc(d, fn);
  if (rc != RT_OK) return rc;
  const int ndev = rt_device_count();
  if (ndev <= 0) return fail(RT_ERR_NO_DEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(RT_ERR_INVALID_ARG, "device %d out of range (%d visible)", device, ndev);
  HIP_TRY(hipSetDevice(device));
  rt_skin* p = new rt_skin();
  p->device = device, p->n_bones = d->n_bones, p->n_triangles = d->n_triangles, p->tri_first = d->tri_first;
  // one host image of the allocation, every array on a multiple of 256 bytes, uploaded in one copy
  const size_t nv = d->n_vertices, nt = d->tri_count;
  const bool has_n = d->normal != nullptr;
  const size_t v3 = rt_pad256(nv * 12), n3 = has_n ? v3 : 0, vb = rt_pad256(nv * 8), vw = rt_pad256(nv * 16), t3 = rt_pad256(nt * 12);
  const size_t xf = rt_pad256((size_t)d->n_bones * 32);
  const size_t total = 2 * v3 + 2 * n3 + vb + vw + 5 * t3 + xf;
  std::vector<unsigned char> img(total, 0);
  size_t used = 0;
  auto take = [&](size_t bytes) {
    unsigned char* at = img.data() + used;
    used += bytes;
    return at;
  };
  float *pos = (float*)take(v3), *nrm = has_n ? (float*)take(n3) : nullptr;
  uint16_t* bone = (uint16_t*)take(vb);
  float* weight = (float*)take(vw);
  uint32_t* idx = (uint32_t*)take(t3);
  float *V = (float*)take(v3), *N = has_n ? (float*)take(n3) : nullptr;
  float *o_v1 = (float*)take(t3), *o_e1 = (float*)take(t3), *o_e2 = (float*)take(t3), *o_n = (float*)take(t3);
  unsigned char* xf_at = take(xf);
  memcpy(pos, d->position, nv * 12);
  if (has_n) memcpy(nrm, d->normal, nv * 12);
  memcpy(bone, d->bone, nv * 8), memcpy(weight, d->weight, nv * 16), memcpy(idx, d->indices, nt * 12);
  const RtSkinArrays host{(uint32_t)nv, (uint32_t)nt, pos, nrm, bone, weight, idx, V, N, o_v1, o_e1, o_e2, o_n};
  skin_on_host(host, nullptr);  // the skinned and posed arrays start as the rest mesh
  rc = p->buf.ensure(total);
  if (rc == RT_OK) {
    const hipError_t e = hipMemcpy(p->buf.p, img.data(), total, hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = fail(RT_ERR_HIP, "hipMemcpy H2D failed: %s", hipGetErrorString(e));
  }
  if (rc == RT_OK && hipHostMalloc((void**)&p->xf_stage, (size_t)d->n_bones * 32, hipHostMallocDefault) != hipSuccess)
    p->xf_stage = nullptr, rc = fail(RT_ERR_OOM, "hipHostMalloc(%zu) failed", (size_t)d->n_bones * 32);
  if (rc == RT_OK && hipEventCreate(&p->done_ev) != hipSuccess) p->done_ev = nullptr, rc = fail(RT_ERR_HIP, "hipEventCreate failed");
  if (rc != RT_OK) {
    skin_free(p);
    return rc;
  }
  char* base = (char*)p->buf.p;
  auto dev = [&](const void* host_at) { return host_at ? base + ((const unsigned char*)host_at - img.data()) : nullptr; };
  p->a = RtSkinArrays{(uint32_t)nv, (uint32_t)nt, (const float*)dev(pos), (const float*)dev(nrm), (const uint16_t*)dev(bone),
                      (const float*)dev(weight), (const uint32_t*)dev(idx), (float*)dev(V), (float*)dev(N),
                      (float*)dev(o_v1), (float*)dev(o_e1), (float*)dev(o_e2), (float*)dev(o_n)};
  p->xf_dev = (rt_transform*)dev(xf_at);
  *out = p;
  return RT_OK;
}

void rt_skin_destroy(rt_skin* p) { skin_free(p); }

int rt_skin_geometry_device(rt_skin* p, const rt_transform* bones_dev, void* hip_stream) {
  const char* fn = "rt_skin_geometry_device";
  if (!p) return fail(RT_ERR_INVALID_ARG, "%s: null skin", fn);
  if (!bones_dev) return fail(RT_ERR_INVALID_ARG, "%s: null bones", fn);
  HIP_TRY(hipSetDevice(p->device));
  return kernel_enqueue(p, bones_dev, (hipStream_t)hip_stream);
}

int rt_skin_apply_device(rt_scene* s, rt_skin* p, const rt_transform* bones_dev, void* hip_stream, rt_update_info* info) {
  rt_scene_delta d;
  int rc = check_apply(s, p, bones_dev, "rt_skin_apply_device", &d);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(p->device));
  if ((rc = kernel_enqueue(p, bones_dev, (hipStream_t)hip_stream)) != RT_OK) return rc;
  rc = rt_scene_update_device(s, &d, hip_stream, info);  // (blocks: the stream has drained)
  if (rc == RT_OK) p->pending = false;
  return rc;
}

int rt_skin_apply(rt_scene* s, rt_skin* p, const rt_transform* bones_host, rt_update_info* info) {
  const char* fn = "rt_skin_apply";
  rt_scene_delta d;
  int rc = check_apply(s, p, bones_host, fn, &d);
  if (rc == RT_OK) rc = check_bones(bones_host, p->n_bones, fn);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(p->device));
  if ((rc = skin_wait(p)) != RT_OK) return rc;  // (a kernel still in flight reads the staged bones)
  memcpy(p->xf_stage, bones_host, (size_t)p->n_bones * 32);
  HIP_TRY(hipMemcpyAsync(p->xf_dev, p->xf_stage, (size_t)p->n_bones * 32, hipMemcpyHostToDevice, nullptr));
  if ((rc = kernel_enqueue(p, p->xf_dev, nullptr)) != RT_OK) return rc;
  rc = rt_scene_update_device(s, &d, nullptr, info);
  if (rc == RT_OK) p->pending = false;
  return rc;
}

int rt_skin_read(rt_skin* p, float* position, float* normal, float* tri_v1, float* tri_e1, float* tri_e2, float* tri_normal) {
  if (!p) return fail(RT_ERR_INVALID_ARG, "rt_skin_read: null skin");
  HIP_TRY(hipSetDevice(p->device));
  const int rc = skin_wait(p);
  if (rc != RT_OK) return rc;
  const size_t nv = p->a.n_vertices, nt = p->a.n_tris;
  const struct {
    float* host;
    const float* dev;
    size_t bytes;
  } arrays[6] = {{position, p->a.V, nv * 12},  {normal, p->a.N, nv * 12},   {tri_v1, p->a.o_v1, nt * 12},
                 {tri_e1, p->a.o_e1, nt * 12}, {tri_e2, p->a.o_e2, nt * 12}, {tri_normal, p->a.o_normal, nt * 12}};
  for (const auto& a : arrays)
    if (a.host && a.dev) HIP_TRY(hipMemcpy(a.host, a.dev, a.bytes, hipMemcpyDeviceToHost));
  return RT_OK;
}

int rt_skin_model(const rt_skin_desc* d, const rt_transform* bones, float* position, float* normal, float* tri_v1, float* tri_e1, float* tri_e2,
                  float* tri_normal) {
  const char* fn = "rt_skin_model";
  const int rc = check_desc(d, fn);
  if (rc != RT_OK) return rc;
  if (!bones) return fail(RT_ERR_INVALID_ARG, "%s: null bones", fn);
  const size_t nv = d->n_vertices, nt = d->tri_count;
  // outputs the caller does not want land in scratch arrays
  std::vector<float> scratch[6];
  float* o[6] = {position, normal, tri_v1, tri_e1, tri_e2, tri_normal};
  const size_t floats[6] = {3 * nv, 3 * nv, 3 * nt, 3 * nt, 3 * nt, 3 * nt};
  for (int k = 0; k < 6; k++)
    if (!o[k]) scratch[k].resize(floats[k]), o[k] = scratch[k].data();
  const RtSkinArrays a{(uint32_t)nv, (uint32_t)nt, d->position, d->normal, d->bone, d->weight, d->indices, o[0], d->normal ? o[1] : nullptr,
                       o[2], o[3], o[4], o[5]};
  skin_on_host(a, (const float*)bones);
  return RT_OK;
}

}  // extern "C"
