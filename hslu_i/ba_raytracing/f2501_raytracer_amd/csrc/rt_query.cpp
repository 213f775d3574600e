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
  if (!b) return fail(RT_ERR_INVALID_ARG, "%s: null ray batch", fn);
  if (!out) return fail(RT_ERR_INVALID_ARG, "%s: null output struct", fn);
  if (b->abi_version != RT_ABI_VERSION)
    return fail(RT_ERR_INVALID_ARG, "%s: rt_ray_batch.abi_version %u != %u", fn, b->abi_version, RT_ABI_VERSION);
  if (b->flags & ~RT_FLAG_BACKFACE_CULLING)
    return fail(RT_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x (only RT_FLAG_BACKFACE_CULLING)", fn, b->flags & ~RT_FLAG_BACKFACE_CULLING);
  if (b->n_rays && (!b->origin || !b->direction)) return fail(RT_ERR_INVALID_ARG, "%s: origin / direction missing", fn);
  if (!any_output) return fail(RT_ERR_INVALID_ARG, "%s: every output plane is NULL", fn);
  return RT_OK;
}

bool any_plane(const rt_ray_hits* h) { return h && (h->id || h->t || h->point || h->normal || h->material); }
bool any_plane(const rt_ray_occlusion* o) {
  return o && (o->has_intersection || o->completely_occluded || o->combined_opacity || o->color_filter);
}

RtQueryArgs args_of(const rt_ray_batch* b) {
  RtQueryArgs q;
  memset(&q, 0, sizeof(q));
  q.origin = b->origin;
  q.direction = b->direction;
  q.max_distance = b->max_distance;
  q.n = b->n_rays;
  q.cull = (b->flags & RT_FLAG_BACKFACE_CULLING) ? 1u : 0u;
  return q;
}

// Host form: one device allocation for the call -- inputs, then every requested output plane (256-byte aligned each)
struct Staging {
  DevBuf buf;
  size_t used = 0;
  char* take(size_t bytes) {
    char* p = (char*)buf.p + used;
    used += (bytes + 255u) & ~(size_t)255u;
    return p;
  }
  ~Staging() { buf.release(); }
};

struct Plane {  // a host output plane and its device twin
  void* host;
  void* dev;
  size_t bytes;
};

int run_host(rt_scene* s, const rt_ray_batch* b, bool nearest, const rt_ray_hits* h, const rt_ray_occlusion* o) {
  if (b->n_rays == 0) return RT_OK;
  HIP_TRY(hipSetDevice(s->device));
  const size_t n = b->n_rays;
  Plane planes[5];
  int np = 0;
  if (nearest) {
    if (h->id) planes[np++] = {h->id, nullptr, n * 4};
    if (h->t) planes[np++] = {h->t, nullptr, n * 4};
    if (h->point) planes[np++] = {h->point, nullptr, n * 12};
    if (h->normal) planes[np++] = {h->normal, nullptr, n * 12};
    if (h->material) planes[np++] = {h->material, nullptr, n * 4};
  } else {
    if (o->has_intersection) planes[np++] = {o->has_intersection, nullptr, n};
    if (o->completely_occluded) planes[np++] = {o->completely_occluded, nullptr, n};
    if (o->combined_opacity) planes[np++] = {o->combined_opacity, nullptr, n * 4};
    if (o->color_filter) planes[np++] = {o->color_filter, nullptr, n * 12};
  }
  const bool with_max = !nearest && b->max_distance;
  size_t total = 2 * ((n * 12 + 255u) & ~(size_t)255u) + (with_max ? ((n * 4 + 255u) & ~(size_t)255u) : 0u);
  for (int k = 0; k < np; k++) total += (planes[k].bytes + 255u) & ~(size_t)255u;
  Staging st;
  int rc = st.buf.ensure(total);
  if (rc != RT_OK) return rc;
  RtQueryArgs q = args_of(b);
  float* d_o = (float*)st.take(n * 12);
  float* d_d = (float*)st.take(n * 12);
  float* d_m = with_max ? (float*)st.take(n * 4) : nullptr;
  for (int k = 0; k < np; k++) planes[k].dev = st.take(planes[k].bytes);
  // a private stream: the call neither waits for nor delays work the caller has on the null stream
  hipStream_t stream = nullptr;
  HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  struct StreamGuard {
    hipStream_t s;
    ~StreamGuard() { (void)hipStreamSynchronize(s), (void)hipStreamDestroy(s); }
  } guard{stream};
  HIP_TRY(hipMemcpyAsync(d_o, b->origin, n * 12, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_d, b->direction, n * 12, hipMemcpyHostToDevice, stream));
  if (d_m) HIP_TRY(hipMemcpyAsync(d_m, b->max_distance, n * 4, hipMemcpyHostToDevice, stream));
  q.origin = d_o;
  q.direction = d_d;
  q.max_distance = d_m;
  int k = 0;
  if (nearest) {
    if (h->id) q.id = (int32_t*)planes[k++].dev;
    if (h->t) q.t = (float*)planes[k++].dev;
    if (h->point) q.point = (float*)planes[k++].dev;
    if (h->normal) q.normal = (float*)planes[k++].dev;
    if (h->material) q.material = (uint32_t*)planes[k++].dev;
  } else {
    if (o->has_intersection) q.has_intersection = (uint8_t*)planes[k++].dev;
    if (o->completely_occluded) q.occluded = (uint8_t*)planes[k++].dev;
    if (o->combined_opacity) q.opacity = (float*)planes[k++].dev;
    if (o->color_filter) q.filter = (float*)planes[k++].dev;
  }
  hipError_t e = (hipError_t)(nearest ? rt_launch_query_nearest(s->dev, q, stream) : rt_launch_query_any(s->dev, q, stream));
  if (e != hipSuccess) return fail(RT_ERR_HIP, "query launch failed: %s", hipGetErrorString(e));
  for (int j = 0; j < np; j++) HIP_TRY(hipMemcpyAsync(planes[j].host, planes[j].dev, planes[j].bytes, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_cast_rays(rt_scene* s, const rt_ray_batch* b, const rt_ray_hits* h) {
  int rc = check_batch(s, b, h, any_plane(h), "rt_cast_rays");
  if (rc != RT_OK) return rc;
  return run_host(s, b, true, h, nullptr);
}

int rt_any_intersection(rt_scene* s, const rt_ray_batch* b, const rt_ray_occlusion* o) {
  int rc = check_batch(s, b, o, any_plane(o), "rt_any_intersection");
  if (rc != RT_OK) return rc;
  return run_host(s, b, false, nullptr, o);
}

int rt_cast_rays_device(rt_scene* s, const rt_ray_batch* b, const rt_ray_hits* h, void* hip_stream) {
  int rc = check_batch(s, b, h, any_plane(h), "rt_cast_rays_device");
  if (rc != RT_OK) return rc;
  if (b->n_rays == 0) return RT_OK;
  HIP_TRY(hipSetDevice(s->device));
  RtQueryArgs q = args_of(b);
  q.max_distance = nullptr;
  q.id = h->id, q.t = h->t, q.point = h->point, q.normal = h->normal, q.material = h->material;
  hipError_t e = (hipError_t)rt_launch_query_nearest(s->dev, q, hip_stream);
  if (e != hipSuccess) return fail(RT_ERR_HIP, "query launch failed: %s", hipGetErrorString(e));
  return RT_OK;
}

int rt_any_intersection_device(rt_scene* s, const rt_ray_batch* b, const rt_ray_occlusion* o, void* hip_stream) {
  int rc = check_batch(s, b, o, any_plane(o), "rt_any_intersection_device");
  if (rc != RT_OK) return rc;
  if (b->n_rays == 0) return RT_OK;
  HIP_TRY(hipSetDevice(s->device));
  RtQueryArgs q = args_of(b);
  q.has_intersection = o->has_intersection, q.occluded = o->completely_occluded, q.opacity = o->combined_opacity,
  q.filter = o->color_filter;
  hipError_t e = (hipError_t)rt_launch_query_any(s->dev, q, hip_stream);
  if (e != hipSuccess) return fail(RT_ERR_HIP, "query launch failed: %s", hipGetErrorString(e));
  return RT_OK;
}

}  // extern "C"
