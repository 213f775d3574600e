// rt_query.cpp -- the ray-query entry points of include/rt_hip.h: rt_cast_rays[_device] (Raytracer::cast_ray,
// src/raytracing/raytracer.rs:162-220) and rt_any_intersection[_device] (Raytracer::has_any_intersection, raytracer.rs:24-106).
//
// A query reads only the scene's immutable device arrays (RtDevScene): no frame slot, counter block, parameter table or
// per-stream-key render state is touched, so a query may run on any stream while frames of the same scene render on
// others (rt_render_begin's band thread included).  The _device forms allocate nothing and only enqueue; the host forms
// stage the batch through device memory of their own for the call.
#include <hip/hip_runtime.h>

#include <cstring>

#include "rt_host.h"

namespace {

// validation shared by the four entry points; runs before any HIP call
int check_batch(const rt_scene* s, const rt_ray_batch* b, const void* out, bool any_output, const char* fn) {
  if (!s) return fail(RT_ERR_INVALID_ARG, "%s: null scene", fn);
  if (b && !out)  // (a null batch is reported first, by rt_check_ray_batch)
    return fail(RT_ERR_INVALID_ARG, "%s: null output struct", fn);
  const int rc = rt_check_ray_batch(b, fn);
  if (rc != RT_OK) return rc;
  if (b->flags & ~RT_FLAG_BACKFACE_CULLING)
    return fail(RT_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x (only RT_FLAG_BACKFACE_CULLING)", fn, b->flags & ~RT_FLAG_BACKFACE_CULLING);
  if (!any_output) return fail(RT_ERR_INVALID_ARG, "%s: every output plane is NULL", fn);
  return RT_OK;
}

bool any_plane(const rt_ray_hits* h) { return h && (h->id || h->t || h->point || h->normal || h->material); }
bool any_plane(const rt_ray_occlusion* o) {
  return o && (o->has_intersection || o->completely_occluded || o->combined_opacity || o->color_filter);
}

// the kernel's arguments as the caller gave them: of the nearest-hit query (h) or the any-hit query (o)
RtQueryArgs args_of(const rt_ray_batch* b, const rt_ray_hits* h, const rt_ray_occlusion* o) {
  RtQueryArgs q;
  memset(&q, 0, sizeof(q));
  q.origin = b->origin;
  q.direction = b->direction;
  q.n = b->n_rays;
  q.cull = (b->flags & RT_FLAG_BACKFACE_CULLING) ? 1u : 0u;
  if (h) {
    q.id = h->id, q.t = h->t, q.point = h->point, q.normal = h->normal, q.material = h->material;
  } else {
    q.max_distance = b->max_distance;
    q.has_intersection = o->has_intersection, q.occluded = o->completely_occluded, q.opacity = o->combined_opacity,
    q.filter = o->color_filter;
  }
  return q;
}

int launch(rt_scene* s, const RtQueryArgs& q, bool nearest, hipStream_t stream) {
  const hipError_t e = (hipError_t)(nearest ? rt_launch_query_nearest(s->dev, q, stream) : rt_launch_query_any(s->dev, q, stream));
  if (e != hipSuccess) return fail(RT_ERR_HIP, "query launch failed: %s", hipGetErrorString(e));
  return RT_OK;
}

// device form: enqueues on the caller's stream
int run_device(rt_scene* s, const rt_ray_batch* b, const rt_ray_hits* h, const rt_ray_occlusion* o, void* hip_stream) {
  if (b->n_rays == 0) return RT_OK;
  HIP_TRY(hipSetDevice(s->device));
  return launch(s, args_of(b, h, o), h != nullptr, (hipStream_t)hip_stream);
}

// host form: the batch and every requested plane go through a HostCall
int run_host(rt_scene* s, const rt_ray_batch* b, const rt_ray_hits* h, const rt_ray_occlusion* o) {
  if (b->n_rays == 0) return RT_OK;
  HIP_TRY(hipSetDevice(s->device));
  const size_t n = b->n_rays;
  RtQueryArgs q = args_of(b, h, o);
  HostCall c;
  c.in(&q.origin, n * 12), c.in(&q.direction, n * 12), c.in(&q.max_distance, n * 4);
  c.out(&q.id, n * 4), c.out(&q.t, n * 4), c.out(&q.point, n * 12), c.out(&q.normal, n * 12), c.out(&q.material, n * 4);
  c.out(&q.has_intersection, n), c.out(&q.occluded, n), c.out(&q.opacity, n * 4), c.out(&q.filter, n * 12);
  int rc = c.begin();
  if (rc == RT_OK) rc = launch(s, q, h != nullptr, c.stream);
  return rc == RT_OK ? c.finish() : rc;
}

}  // namespace

extern "C" {

int rt_cast_rays(rt_scene* s, const rt_ray_batch* b, const rt_ray_hits* h) {
  const int rc = check_batch(s, b, h, any_plane(h), "rt_cast_rays");
  return rc == RT_OK ? run_host(s, b, h, nullptr) : rc;
}

int rt_any_intersection(rt_scene* s, const rt_ray_batch* b, const rt_ray_occlusion* o) {
  const int rc = check_batch(s, b, o, any_plane(o), "rt_any_intersection");
  return rc == RT_OK ? run_host(s, b, nullptr, o) : rc;
}

int rt_cast_rays_device(rt_scene* s, const rt_ray_batch* b, const rt_ray_hits* h, void* hip_stream) {
  const int rc = check_batch(s, b, h, any_plane(h), "rt_cast_rays_device");
  return rc == RT_OK ? run_device(s, b, h, nullptr, hip_stream) : rc;
}

int rt_any_intersection_device(rt_scene* s, const rt_ray_batch* b, const rt_ray_occlusion* o, void* hip_stream) {
  const int rc = check_batch(s, b, o, any_plane(o), "rt_any_intersection_device");
  return rc == RT_OK ? run_device(s, b, nullptr, o, hip_stream) : rc;
}

}  // extern "C"
