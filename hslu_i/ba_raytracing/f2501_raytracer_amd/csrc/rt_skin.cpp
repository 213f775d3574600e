// rt_skin.cpp -- the host side of device-side skinned meshes (rt_skin*): validation (before any HIP call), the handle and its
// one device allocation, the launch of the two kernels, the delta handed to rt_scene_update_device, and the host model (the
// functions of rt_skin.h in loops).
//
// A skin is built ON TOP of the in-place update, as a pose is (rt_pose.cpp): it makes the triangle arrays of an
// rt_scene_delta on the device and hands them to rt_scene_update_device through its public entry point, so every blocking,
// invalidation and refusal rule of an apply is that call's.
#include <hip/hip_runtime.h>

#include <cstring>

#include "rt_deform.h"
#include "rt_skin.h"

static_assert(sizeof(RtSkinBones) == 8 && sizeof(RtSkinWeights) == 16, "one 8-byte and one 16-byte load per vertex");

struct rt_skin {
  RtDeformer m;                   // (n_xf: bones; buf: rest mesh, tables, skinned vertices, posed triangle arrays, the staged bones)
  uint32_t n_triangles = 0, tri_first = 0;
  RtSkinArrays a{};               // device pointers into m.buf
  int launch(const rt_transform* bones_dev, hipStream_t stream) {
    const hipError_t e = (hipError_t)rt_launch_skin(a, bones_dev, stream);
    return e == hipSuccess ? RT_OK : fail(RT_ERR_HIP, "skin kernel launch failed: %s", hipGetErrorString(e));
  }
  static int check_apply(const rt_scene* s, const rt_skin* p, const rt_transform* t, const char* fn, rt_scene_delta* delta);
  static int check_table(const rt_transform* t, uint32_t n, const char* fn) {
    const int64_t bad = rt_deform_first_non_finite(t, n);
    return bad < 0 ? RT_OK : fail(RT_ERR_INVALID_ARG, "%s: bone %u has a non-finite member", fn, (uint32_t)bad);
  }
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

// the whole mesh through the formulas on the host (bones null: the rest mesh through the triangle formula)
void skin_on_host(const RtSkinArrays& a, const float* bones) {
  for (uint32_t i = 0; i < a.n_vertices; i++) rt_skin_vertex(a, i, bones);
  for (uint32_t t = 0; t < a.n_tris; t++) a.normal ? rt_skin_tri(a, t) : rt_skin_face(a, t);
}

}  // namespace

// what an apply refuses itself, before any HIP call, and the delta it hands on
int rt_skin::check_apply(const rt_scene* s, const rt_skin* p, const rt_transform* t, const char* fn, rt_scene_delta* delta) {
  if (!s) return fail(RT_ERR_INVALID_ARG, "%s: null scene", fn);
  if (!p) return fail(RT_ERR_INVALID_ARG, "%s: null skin", fn);
  if (!t) return fail(RT_ERR_INVALID_ARG, "%s: null bones", fn);
  if (p->n_triangles != s->dev.n_triangles)
    return fail(RT_ERR_INVALID_ARG, "%s: the skin is for n_triangles %u, the scene has %u", fn, p->n_triangles, s->dev.n_triangles);
  if (p->m.device != s->device) return fail(RT_ERR_INVALID_ARG, "%s: the skin lives on device %d, the scene on device %d", fn, p->m.device, s->device);
  rt_scene_delta d{};
  d.abi_version = RT_ABI_VERSION;
  d.tri_first = p->tri_first, d.tri_count = p->a.n_tris;
  d.tri_v1 = p->a.o_v1, d.tri_e1 = p->a.o_e1, d.tri_e2 = p->a.o_e2, d.tri_normal = p->a.o_normal;
  return rt_deform_check_delta(s, d, delta);
}

extern "C" {

int rt_skin_create(const rt_skin_desc* d, int device, rt_skin** out) {
  const char* fn = "rt_skin_create";
  if (!d || !out) return fail(RT_ERR_INVALID_ARG, "%s: null argument", fn);
  *out = nullptr;
  int rc = check_desc(d, fn);
  if (rc != RT_OK) return rc;
  if ((rc = rt_open_device(device)) != RT_OK) return rc;
  rt_skin* p = new rt_skin();
  p->m.device = device, p->m.n_xf = d->n_bones, p->n_triangles = d->n_triangles, p->tri_first = d->tri_first;
  // one host image of the allocation: p->a points into it until it is uploaded.  No normals: no parts, null pointers.
  const size_t nv = d->n_vertices, nt = d->tri_count;
  const bool has_n = d->normal != nullptr;
  RtSkinArrays& a = p->a;
  a.n_vertices = (uint32_t)nv, a.n_tris = (uint32_t)nt;
  RtArena lay;
  lay.add(nv * 12, &a.position);
  if (has_n) lay.add(nv * 12, &a.normal);
  lay.add(nv * 8, &a.bone), lay.add(nv * 16, &a.weight), lay.add(nt * 12, &a.indices);
  lay.add(nv * 12, &a.V);
  if (has_n) lay.add(nv * 12, &a.N);
  for (float** o : {&a.o_v1, &a.o_e1, &a.o_e2, &a.o_normal}) lay.add(nt * 12, o);
  lay.add((size_t)d->n_bones * 32, &p->m.xf_dev);
  std::vector<unsigned char> img(lay.total(), 0);
  lay.bind(img.data());
  memcpy((void*)a.position, d->position, nv * 12);
  if (has_n) memcpy((void*)a.normal, d->normal, nv * 12);
  memcpy((void*)a.bone, d->bone, nv * 8), memcpy((void*)a.weight, d->weight, nv * 16), memcpy((void*)a.indices, d->indices, nt * 12);
  skin_on_host(a, nullptr);  // the skinned and posed arrays start as the rest mesh
  if ((rc = rt_deform_upload(p, lay, img)) != RT_OK) return rc;
  *out = p;
  return RT_OK;
}

void rt_skin_destroy(rt_skin* p) { rt_deform_free(p); }

int rt_skin_geometry_device(rt_skin* p, const rt_transform* bones_dev, void* hip_stream) {
  const char* fn = "rt_skin_geometry_device";
  if (!p) return fail(RT_ERR_INVALID_ARG, "%s: null skin", fn);
  if (!bones_dev) return fail(RT_ERR_INVALID_ARG, "%s: null bones", fn);
  return rt_deform_geometry_device(p, bones_dev, hip_stream);
}

int rt_skin_apply_device(rt_scene* s, rt_skin* p, const rt_transform* bones_dev, void* hip_stream, rt_update_info* info) {
  return rt_deform_apply_device(s, p, bones_dev, hip_stream, info, "rt_skin_apply_device");
}

int rt_skin_apply(rt_scene* s, rt_skin* p, const rt_transform* bones_host, rt_update_info* info) {
  return rt_deform_apply(s, p, bones_host, info, "rt_skin_apply");
}

int rt_skin_read(rt_skin* p, float* position, float* normal, float* tri_v1, float* tri_e1, float* tri_e2, float* tri_normal) {
  if (!p) return fail(RT_ERR_INVALID_ARG, "rt_skin_read: null skin");
  const int rc = rt_deform_wait(p->m);
  if (rc != RT_OK) return rc;
  const size_t nv = p->a.n_vertices, nt = p->a.n_tris;
  const RtReadBack arrays[6] = {{position, p->a.V, nv * 12},  {normal, p->a.N, nv * 12},   {tri_v1, p->a.o_v1, nt * 12},
                                {tri_e1, p->a.o_e1, nt * 12}, {tri_e2, p->a.o_e2, nt * 12}, {tri_normal, p->a.o_normal, nt * 12}};
  return rt_deform_read(arrays);
}

int rt_skin_model(const rt_skin_desc* d, const rt_transform* bones, float* position, float* normal, float* tri_v1, float* tri_e1, float* tri_e2,
                  float* tri_normal) {
  const char* fn = "rt_skin_model";
  const int rc = check_desc(d, fn);
  if (rc != RT_OK) return rc;
  if (!bones) return fail(RT_ERR_INVALID_ARG, "%s: null bones", fn);
  const size_t nv = d->n_vertices, nt = d->tri_count;
  std::vector<float> scratch[6];
  float* o[6] = {position, normal, tri_v1, tri_e1, tri_e2, tri_normal};
  const size_t floats[6] = {3 * nv, 3 * nv, 3 * nt, 3 * nt, 3 * nt, 3 * nt};
  rt_deform_scratch(o, floats, scratch);
  const RtSkinArrays a{(uint32_t)nv, (uint32_t)nt, d->position, d->normal, d->bone, d->weight, d->indices, o[0], d->normal ? o[1] : nullptr,
                       o[2], o[3], o[4], o[5]};
  skin_on_host(a, (const float*)bones);
  return RT_OK;
}

}  // extern "C"
