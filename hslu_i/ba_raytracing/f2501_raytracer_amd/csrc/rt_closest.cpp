// rt_closest.cpp -- the closest-point entry points of include/rt_hip.h: rt_closest_points[_device] on a scene handle and
// rt_closest_points_model, the specification: a linear scan of a scene description with the functions of rt_closest.h.
//
// As the ray queries (rt_query.cpp), a query reads only the scene's device arrays (RtDevScene): no frame slot, counter block
// or parameter table is touched, so it may run on any stream beside renders.  The _device form allocates nothing and only
// enqueues; the host form stages the batch through device memory of its own for the call.
#include <hip/hip_runtime.h>

#include <cstring>

#include "rt_host.h"

namespace {

bool any_plane(const rt_point_hits* h) { return h && (h->id || h->distance || h->point || h->normal || h->bary || h->material); }

// validation shared by the three entry points; runs before any HIP call
int check_batch(bool have_scene, const rt_point_batch* b, const rt_point_hits* h, const char* fn) {
  if (!have_scene) return fail(RT_ERR_INVALID_ARG, "%s: null scene", fn);
  if (!b) return fail(RT_ERR_INVALID_ARG, "%s: null point batch", fn);
  if (!h) return fail(RT_ERR_INVALID_ARG, "%s: null output struct", fn);
  if (b->abi_version != RT_ABI_VERSION)
    return fail(RT_ERR_INVALID_ARG, "%s: rt_point_batch.abi_version %u != %u", fn, b->abi_version, RT_ABI_VERSION);
  if (b->n_points && !b->point) return fail(RT_ERR_INVALID_ARG, "%s: point missing", fn);
  if (!any_plane(h)) return fail(RT_ERR_INVALID_ARG, "%s: every output plane is NULL", fn);
  return RT_OK;
}

RtClosestArgs args_of(const rt_point_batch* b, const rt_point_hits* h) {
  RtClosestArgs a;
  memset(&a, 0, sizeof(a));
  a.point = b->point, a.max_distance = b->max_distance, a.n = b->n_points;
  a.id = h->id, a.distance = h->distance, a.out_point = h->point, a.normal = h->normal, a.bary = h->bary, a.material = h->material;
  return a;
}

int launch(rt_scene* s, const RtClosestArgs& a, hipStream_t stream) {
  const hipError_t e = (hipError_t)rt_launch_closest(s->dev, a, stream);
  if (e != hipSuccess) return fail(RT_ERR_HIP, "closest-point launch failed: %s", hipGetErrorString(e));
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_closest_points(rt_scene* s, const rt_point_batch* b, const rt_point_hits* h) {
  const int rc0 = check_batch(s != nullptr, b, h, "rt_closest_points");
  if (rc0 != RT_OK || b->n_points == 0) return rc0;
  HIP_TRY(hipSetDevice(s->device));
  const size_t n = b->n_points;
  RtClosestArgs a = args_of(b, h);
  HostCall c;
  c.in(&a.point, n * 12), c.in(&a.max_distance, n * 4);
  c.out(&a.id, n * 4), c.out(&a.distance, n * 4), c.out(&a.out_point, n * 12), c.out(&a.normal, n * 12), c.out(&a.bary, n * 8),
      c.out(&a.material, n * 4);
  int rc = c.begin();
  if (rc == RT_OK) rc = launch(s, a, c.stream);
  return rc == RT_OK ? c.finish() : rc;
}

int rt_closest_points_device(rt_scene* s, const rt_point_batch* b, const rt_point_hits* h, void* hip_stream) {
  const int rc = check_batch(s != nullptr, b, h, "rt_closest_points_device");
  if (rc != RT_OK || b->n_points == 0) return rc;
  HIP_TRY(hipSetDevice(s->device));
  return launch(s, args_of(b, h), (hipStream_t)hip_stream);
}

int rt_closest_points_model(const rt_scene_desc* d, const rt_point_batch* b, const rt_point_hits* h) {
  const int rc = check_batch(d != nullptr, b, h, "rt_closest_points_model");
  if (rc != RT_OK) return rc;
  const int rd = rt_check_scene_desc(d);
  if (rd != RT_OK) return rd;
  const RtClosestArgs a = args_of(b, h);
  for (size_t i = 0; i < a.n; i++) {
    const float p[3] = {a.point[3 * i], a.point[3 * i + 1], a.point[3 * i + 2]};
    const float max_distance = a.max_distance ? a.max_distance[i] : INFINITY;
    RtClosestHit hit;
    rt_closest_miss(hit);
    if (rt_closest_alive(p, max_distance)) {
      RtClosestBest best;
      best.dist = max_distance, best.id = -1, best.slot = 0u;
      for (uint32_t k = 0; k < d->n_spheres; k++) {
        RtClosestSphere s;
        rt_closest_sphere(d->sphere_center + 3 * (size_t)k, d->sphere_r_sq[k], p, s);
        rt_closest_offer(best, s.dist, (int32_t)k, k);
      }
      for (uint32_t t = 0; t < d->n_triangles; t++) {
        RtClosestTri r;
        rt_closest_tri(d->tri_v1 + 3 * (size_t)t, d->tri_e1 + 3 * (size_t)t, d->tri_e2 + 3 * (size_t)t, p, r);
        rt_closest_offer(best, rt_fsqrt(r.d2), (int32_t)(d->n_spheres + t), t);
      }
      if (best.id >= 0 && (uint32_t)best.id < d->n_spheres) {
        const size_t k = (size_t)best.id;
        rt_closest_hit_sphere(d->sphere_center + 3 * k, d->sphere_r_sq[k], d->sphere_material[k], p, best.id, hit);
      } else if (best.id >= 0) {
        const size_t t = best.slot;
        rt_closest_hit_tri(d->tri_v1 + 3 * t, d->tri_e1 + 3 * t, d->tri_e2 + 3 * t, d->tri_normal + 3 * t, d->tri_material[t], p, best.id, hit);
      }
    }
    rt_closest_store(a, i, hit);
  }
  return RT_OK;
}

}  // extern "C"
