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

#include "rt_deform.h"
#include "rt_pose.h"

struct rt_pose {
  RtDeformer m;                   // (n_xf: parts; buf: part tables, rest pose, posed arrays, the staged transforms)
  uint32_t n_triangles = 0, n_spheres = 0;
  bool has_spheres = false;       // some part has spheres: the sphere group travels with every apply
  RtPoseArrays a{};               // device pointers into m.buf
  int launch(const rt_transform* transforms_dev, hipStream_t stream) {
    const hipError_t e = (hipError_t)rt_launch_pose(a, transforms_dev, stream);
    return e == hipSuccess ? RT_OK : fail(RT_ERR_HIP, "pose kernel launch failed: %s", hipGetErrorString(e));
  }
  static int check_apply(const rt_scene* s, const rt_pose* p, const rt_transform* t, const char* fn, rt_scene_delta* delta);
  static int check_table(const rt_transform* t, uint32_t n, const char* fn) {
    const int64_t bad = rt_deform_first_non_finite(t, n);
    return bad < 0 ? RT_OK : fail(RT_ERR_INVALID_ARG, "%s: transform %u has a non-finite member", fn, (uint32_t)bad);
  }
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

}  // namespace

// what an apply refuses itself, before any HIP call, and the delta it hands on
int rt_pose::check_apply(const rt_scene* s, const rt_pose* p, const rt_transform* t, const char* fn, rt_scene_delta* delta) {
  if (!s) return fail(RT_ERR_INVALID_ARG, "%s: null scene", fn);
  if (!p) return fail(RT_ERR_INVALID_ARG, "%s: null pose", fn);
  if (!t) return fail(RT_ERR_INVALID_ARG, "%s: null transforms", fn);
  if (p->n_triangles != s->dev.n_triangles || p->n_spheres != s->dev.n_spheres)
    return fail(RT_ERR_INVALID_ARG, "%s: the pose is for %u triangles and %u spheres, the scene has %u and %u", fn, p->n_triangles, p->n_spheres,
                s->dev.n_triangles, s->dev.n_spheres);
  if (p->m.device != s->device) return fail(RT_ERR_INVALID_ARG, "%s: the pose lives on device %d, the scene on device %d", fn, p->m.device, s->device);
  rt_scene_delta d{};
  d.abi_version = RT_ABI_VERSION;
  if (p->a.n_cover) {
    d.tri_first = p->a.lo, d.tri_count = p->a.n_cover;
    d.tri_v1 = p->a.o_v1, d.tri_e1 = p->a.o_e1, d.tri_e2 = p->a.o_e2, d.tri_normal = p->a.o_normal;
  }
  if (p->has_spheres) d.sphere_center = p->a.o_centre, d.sphere_r_sq = p->a.o_r_sq, d.sphere_r_inv = p->a.o_r_inv;
  return rt_deform_check_delta(s, d, delta);
}

extern "C" {

int rt_pose_create(const rt_pose_desc* d, int device, rt_pose** out) {
  const char* fn = "rt_pose_create";
  if (!d || !out) return fail(RT_ERR_INVALID_ARG, "%s: null argument", fn);
  *out = nullptr;
  Cover c;
  int rc = check_desc(d, fn, &c);
  if (rc != RT_OK) return rc;
  if ((rc = rt_open_device(device)) != RT_OK) return rc;
  rt_pose* p = new rt_pose();
  p->m.device = device, p->m.n_xf = d->n_parts, p->n_triangles = d->n_triangles, p->n_spheres = d->n_spheres, p->has_spheres = c.has_spheres;
  // one host image of the allocation: p->a points into it until it is uploaded
  const size_t nc = c.n_cover, ns = c.has_spheres ? d->n_spheres : 0u;
  RtPoseArrays& a = p->a;
  a.lo = c.lo, a.n_cover = (uint32_t)nc, a.n_spheres = (uint32_t)ns;
  RtArena lay;
  lay.add(nc * 4, &a.tri_part);
  for (const float** in : {&a.v1, &a.v2, &a.v3, &a.normal}) lay.add(nc * 12, in);
  for (float** o : {&a.o_v1, &a.o_e1, &a.o_e2, &a.o_normal}) lay.add(nc * 12, o);
  lay.add(ns * 4, &a.sphere_part), lay.add(ns * 12, &a.centre), lay.add(ns * 4, &a.radius);
  lay.add(ns * 12, &a.o_centre), lay.add(ns * 4, &a.o_r_sq), lay.add(ns * 4, &a.o_r_inv);
  lay.add((size_t)d->n_parts * 32, &p->m.xf_dev);
  std::vector<unsigned char> img(lay.total(), 0);
  lay.bind(img.data());
  std::vector<uint32_t> tp, sp;
  part_tables(d, c, &tp, &sp);
  const size_t off = 3 * (size_t)c.lo;
  if (nc) {
    memcpy((void*)a.tri_part, tp.data(), nc * 4);
    memcpy((void*)a.v1, d->tri_v1 + off, nc * 12), memcpy((void*)a.v2, d->tri_v2 + off, nc * 12);
    memcpy((void*)a.v3, d->tri_v3 + off, nc * 12), memcpy((void*)a.normal, d->tri_normal + off, nc * 12);
  }
  if (ns) memcpy((void*)a.sphere_part, sp.data(), ns * 4), memcpy((void*)a.centre, d->sphere_center, ns * 12), memcpy((void*)a.radius, d->sphere_radius, ns * 4);
  for (uint32_t k = 0; k < nc; k++) rt_pose_tri(a, k, nullptr);  // the posed arrays start as the rest pose
  for (uint32_t i = 0; i < ns; i++) rt_pose_sphere(a, i, nullptr);
  if ((rc = rt_deform_upload(p, lay, img)) != RT_OK) return rc;
  *out = p;
  return RT_OK;
}

void rt_pose_destroy(rt_pose* p) { rt_deform_free(p); }

int rt_pose_geometry_device(rt_pose* p, const rt_transform* transforms_dev, void* hip_stream) {
  const char* fn = "rt_pose_geometry_device";
  if (!p) return fail(RT_ERR_INVALID_ARG, "%s: null pose", fn);
  if (!transforms_dev) return fail(RT_ERR_INVALID_ARG, "%s: null transforms", fn);
  return rt_deform_geometry_device(p, transforms_dev, hip_stream);
}

int rt_pose_apply_device(rt_scene* s, rt_pose* p, const rt_transform* transforms_dev, void* hip_stream, rt_update_info* info) {
  return rt_deform_apply_device(s, p, transforms_dev, hip_stream, info, "rt_pose_apply_device");
}

int rt_pose_apply(rt_scene* s, rt_pose* p, const rt_transform* transforms_host, rt_update_info* info) {
  return rt_deform_apply(s, p, transforms_host, info, "rt_pose_apply");
}

int rt_pose_read(rt_pose* p, float* tri_v1, float* tri_e1, float* tri_e2, float* tri_normal, uint32_t* tri_first, uint32_t* tri_count,
                 float* sphere_center, float* sphere_r_sq, float* sphere_r_inv) {
  if (!p) return fail(RT_ERR_INVALID_ARG, "rt_pose_read: null pose");
  const int rc = rt_deform_wait(p->m);
  if (rc != RT_OK) return rc;
  const size_t nc = p->a.n_cover, ns = p->a.n_spheres;
  if (tri_first) *tri_first = p->a.lo;
  if (tri_count) *tri_count = p->a.n_cover;
  const RtReadBack arrays[7] = {{tri_v1, p->a.o_v1, nc * 12}, {tri_e1, p->a.o_e1, nc * 12}, {tri_e2, p->a.o_e2, nc * 12}, {tri_normal, p->a.o_normal, nc * 12},
                                {sphere_center, p->a.o_centre, ns * 12}, {sphere_r_sq, p->a.o_r_sq, ns * 4}, {sphere_r_inv, p->a.o_r_inv, ns * 4}};
  return rt_deform_read(arrays);
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
  std::vector<float> scratch[7];
  float* o[7] = {tri_v1, tri_e1, tri_e2, tri_normal, sphere_center, sphere_r_sq, sphere_r_inv};
  const size_t floats[7] = {3 * nc, 3 * nc, 3 * nc, 3 * nc, 3 * ns, ns, ns};
  rt_deform_scratch(o, floats, scratch);
  const size_t off = 3 * (size_t)c.lo;
  const RtPoseArrays a{c.lo, (uint32_t)nc, (uint32_t)ns, tp.data(), sp.data(),
                       nc ? d->tri_v1 + off : nullptr, nc ? d->tri_v2 + off : nullptr, nc ? d->tri_v3 + off : nullptr, nc ? d->tri_normal + off : nullptr,
                       d->sphere_center, d->sphere_radius, o[0], o[1], o[2], o[3], o[4], o[5], o[6]};
  for (uint32_t k = 0; k < nc; k++) rt_pose_tri(a, k, tp[k] == RT_POSE_NONE ? nullptr : (const float*)(transforms + tp[k]));
  for (uint32_t i = 0; i < ns; i++) rt_pose_sphere(a, i, sp[i] == RT_POSE_NONE ? nullptr : (const float*)(transforms + sp[i]));
  return RT_OK;
}

}  // extern "C"
