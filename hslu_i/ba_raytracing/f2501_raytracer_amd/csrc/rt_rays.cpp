// rt_rays.cpp -- the radiance-query entry points of include/rt_hip.h: rt_trace_rays[_device], the reference's
// single_raytrace (src/renderer/raytracer_renderer.rs:147-264) for a batch of rays the caller supplies.
//
// Unlike the queries of rt_query.cpp a radiance call IS a render call: it goes through the frame scheduler of rt_api.cpp
// (rt_trace_rays_enqueue) as a frame of n x 1 pixels and uses the scene's parameter tables, frame slots and workspaces.
// What is here: validation (before any HIP call), the parameters of that frame, and the host form's staging.
//
// Also the ray orders (rt_ray_order*, rt_trace_rays_ordered*): the handle, its workspace and its checks.  What an order IS
// is in rt_ray_key.h (the key; host model: rt_ray_order.cpp) and rt_order.hip (the kernels); a trace reads it as
// RtRayArgs::order.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>

#include "rt_host.h"
#include "rt_ray_key.h"

// A permutation of one batch's rays on one device and the workspace that builds it (one allocation: RtOrderWs).
struct rt_ray_order {
  int device = 0;
  uint32_t capacity = 0, origin_bits = 0;
  uint32_t n = 0;         // rays of the batch the order was built or set for
  bool ready = false;     // built or set at least once
  bool has_keys = false;  // built (rt_ray_order_set leaves no keys)
  DevBuf buf;
  RtOrderWs ws{};
  RtPending built;        // behind the kernels of the last build
  double device_ms = 0.0;
};

namespace {

int check_order_batch(const rt_ray_order* o, const rt_ray_batch* b, const char* fn) {
  if (!o) return fail(RT_ERR_INVALID_ARG, "%s: null ray order", fn);
  const int rc = rt_check_ray_batch(b, fn);
  if (rc != RT_OK) return rc;
  if (b->n_rays > o->capacity) return fail(RT_ERR_INVALID_ARG, "%s: %u rays exceed the order's capacity of %u", fn, b->n_rays, o->capacity);
  return RT_OK;
}

// an order a trace of `b` may read: built or set, for as many rays (before any HIP call, before the scene is looked at)
int check_order_use(const rt_ray_order* o, const rt_ray_batch* b, const char* fn) {
  if (!o->ready) return fail(RT_ERR_INVALID_ARG, "%s: the ray order has never been built or set", fn);
  if (o->n != b->n_rays) return fail(RT_ERR_INVALID_ARG, "%s: the ray order holds %u rays, the batch %u", fn, o->n, b->n_rays);
  return RT_OK;
}

int check_order_device(const rt_ray_order* o, const rt_scene* s, const char* fn) {
  if (o->device != s->device) return fail(RT_ERR_INVALID_ARG, "%s: the ray order lives on device %d, the scene on device %d", fn, o->device, s->device);
  return RT_OK;
}

// the kernels of a build on `stream` (DEVICE arrays); n = 0 builds the empty order
int order_enqueue(rt_ray_order* o, const float* origin, const float* direction, uint32_t n, hipStream_t stream) {
  if (n) {
    const hipError_t e = (hipError_t)rt_launch_order_build(o->ws, origin, direction, n, o->origin_bits, stream);
    if (e != hipSuccess) return fail(RT_ERR_HIP, "ray order launch failed: %s", hipGetErrorString(e));
    const int rc = o->built.mark(stream);
    if (rc != RT_OK) return rc;
  }
  o->n = n, o->ready = true, o->has_keys = true, o->device_ms = 0.0;
  return RT_OK;
}

bool any_plane(const rt_ray_radiance* o) { return o && (o->rgb || o->valid || o->id || o->t || o->argb); }

// Validation shared by both entry points; runs before any HIP call and before the scene is looked at.  On success *q is
// the frame the scheduler runs: the caller's shading parameters, its camera members replaced by "n rays, one row".
int check_call(const rt_scene* s, const rt_params* p, const rt_ray_batch* b, const rt_ray_radiance* out, const char* fn, rt_params* q) {
  if (!s) return fail(RT_ERR_INVALID_ARG, "%s: null scene", fn);
  if (!p) return fail(RT_ERR_INVALID_ARG, "%s: null shading parameters", fn);
  // (b &&: a null batch is reported before these, by rt_check_ray_batch)
  if (b && !out) return fail(RT_ERR_INVALID_ARG, "%s: null output struct", fn);
  if (b && p->abi_version != RT_ABI_VERSION)
    return fail(RT_ERR_INVALID_ARG, "%s: rt_params.abi_version %u != %u", fn, p->abi_version, RT_ABI_VERSION);
  int rc = rt_check_ray_batch(b, fn);
  if (rc != RT_OK) return rc;
  if (b->max_distance) return fail(RT_ERR_INVALID_ARG, "%s: rt_ray_batch.max_distance must be NULL (a radiance ray has no length limit)", fn);
  if (b->flags) return fail(RT_ERR_INVALID_ARG, "%s: rt_ray_batch.flags must be 0 (backface culling comes from the shading flags)", fn);
  if (p->flags & RT_FLAG_ANTI_ALIASING)
    return fail(RT_ERR_INVALID_ARG, "%s: RT_FLAG_ANTI_ALIASING in the shading flags (the caller supplies its samples as rays)", fn);
  if (!any_plane(out)) return fail(RT_ERR_INVALID_ARG, "%s: every output plane is NULL", fn);
  *q = *p;
  q->width = b->n_rays ? b->n_rays : 1u, q->height = 1u;
  q->aa_rays = 0, q->aa_offsets = nullptr;
  q->win_x0 = q->win_y0 = q->win_w = q->win_h = 0;
  q->tile_size = 0, q->n_ranks = 0, q->rank = 0;
  // ignored for ray batches: the merged-level and phase kernels and the tile order belong to the camera
  q->tuning.levels = RT_LEVELS_CHAINED, q->tuning.phases = RT_PHASES_FUSED, q->tuning.tile_order = RT_TILE_ORDER_DEFAULT, q->tuning.no_aa_dedup = 0;
  rc = rt_validate_params(q);  // clouds, depths, tuning ranges; "frame too large" = more than 2^31 - 1 rays
  if (rc != RT_OK) return rc;
  if ((q->flags & (RT_FLAG_REFLECTIONS | RT_FLAG_REFRACTIONS)) && q->max_depth_reflection == 0 && q->max_depth_refraction == 0)
    return fail(RT_ERR_INVALID_ARG, "%s: secondary rays enabled with depth 0", fn);
  return RT_OK;
}

RtRayArgs args_of(const rt_ray_batch* b, const rt_ray_radiance* o, const rt_ray_order* order) {
  RtRayArgs r;
  memset(&r, 0, sizeof(r));
  r.origin = b->origin, r.direction = b->direction, r.n = b->n_rays;
  r.order = order ? order->ws.idx_b : nullptr;
  r.rgb = o->rgb, r.valid = o->valid, r.id = o->id, r.t = o->t, r.argb = o->argb;
  return r;
}

// the device memory of an order for `capacity` rays on the current device
int order_alloc(rt_ray_order* o) {
  RtArena lay;
  rt_sort_ws_add(lay, o->capacity, &o->ws);
  lay.add(RT_ORDER_BOUNDS_WGS * sizeof(RtKeyBounds), &o->ws.partial), lay.add(sizeof(RtKeyFrame), &o->ws.frame);
  const int rc = o->buf.ensure(lay.total());
  if (rc != RT_OK) return rc;
  lay.bind(o->buf.p);
  return o->built.create();
}

void order_free(rt_ray_order* o) {
  if (!o) return;
  (void)hipSetDevice(o->device);
  o->built.destroy();
  o->buf.release();
  delete o;
}

// rt_trace_rays and rt_trace_rays_ordered: HOST arrays.  `order`: the order the kernels read the batch through (nullptr:
// none); build_one: no order was given, one is built for this call behind the upload of the rays and freed at its end.
int trace_host(rt_scene* s, const rt_params* p, const rt_ray_batch* b, const rt_ray_order* order, bool build_one, const rt_ray_radiance* out,
               rt_stats* stats, const char* fn) {
  rt_params q;
  int rc = check_call(s, p, b, out, fn, &q);
  if (rc != RT_OK) return rc;
  if (order && (rc = check_order_use(order, b, fn)) != RT_OK) return rc;
  if (stats) memset(stats, 0, sizeof(*stats));
  if (b->n_rays == 0) return RT_OK;
  if (s->progress_active) return fail(RT_ERR_INVALID_ARG, "a progressive render owns this scene until rt_render_end");
  if (order && (rc = check_order_device(order, s, fn)) != RT_OK) return rc;
  HIP_TRY(hipSetDevice(s->device));
  const auto t_begin = std::chrono::steady_clock::now();
  const size_t n = b->n_rays;
  struct OrderGuard {  // the order of this call alone
    rt_ray_order* o = nullptr;
    ~OrderGuard() { order_free(o); }
  } own;
  if (build_one) {
    own.o = new rt_ray_order();
    own.o->device = s->device, own.o->capacity = b->n_rays;
    if ((rc = order_alloc(own.o)) != RT_OK) return rc;
    order = own.o;
  }
  RtRayArgs r = args_of(b, out, order);
  HostCall c;  // (declared behind `own`: the stream drains before the call's order is freed)
  c.in(&r.origin, n * 12), c.in(&r.direction, n * 12);
  c.out(&r.rgb, n * 12), c.out(&r.valid, n), c.out(&r.id, n * 4), c.out(&r.t, n * 4), c.out(&r.argb, n * 4, true);
  Forget forget{s, c};
  EventPair ev;
  if ((rc = ev.create()) != RT_OK || (rc = c.begin()) != RT_OK) return rc;
  // an order another stream is still building: this stream waits for it
  if (order && !build_one && order->built.pending) HIP_TRY(hipStreamWaitEvent(c.stream, order->built.ev, 0));
  HIP_TRY(hipEventRecord(ev.e0, c.stream));
  if (build_one && (rc = order_enqueue(own.o, r.origin, r.direction, b->n_rays, c.stream)) != RT_OK) return rc;
  if ((rc = rt_trace_rays_enqueue(s, &q, r, c.stream)) != RT_OK) return rc;
  HIP_TRY(hipEventRecord(ev.e1, c.stream));
  if ((rc = c.finish()) != RT_OK) return rc;
  if (stats) {
    if ((rc = rt_render_collect_stats(s, stats)) != RT_OK) return rc;
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    stats->kernel_ms = ms;  // (with secondary rays: every attempt of the batch, and the waits for its counters; the build of an order of this call)
    stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  }
  return RT_OK;
}

}  // namespace

int rt_trace_rays_check(const rt_scene* s, const rt_params* p, const rt_ray_batch* b, const rt_ray_radiance* out, const char* fn) {
  rt_params q;
  return check_call(s, p, b, out, fn, &q);
}

size_t rt_ray_order_bytes(const rt_ray_order* o) { return o ? o->buf.cap : 0; }

const uint32_t* rt_ray_order_perm(const rt_ray_order* o) { return o ? o->ws.idx_b : nullptr; }

int rt_trace_rays_perm_device(rt_scene* s, const rt_params* p, const rt_ray_batch* b, const uint32_t* perm, const rt_ray_radiance* out,
                              hipStream_t stream, const char* fn) {
  rt_params q;
  const int rc = check_call(s, p, b, out, fn, &q);
  if (rc != RT_OK) return rc;
  if (b->n_rays == 0) return RT_OK;
  if (s->progress_active) return fail(RT_ERR_INVALID_ARG, "a progressive render owns this scene until rt_render_end");
  RtRayArgs r = args_of(b, out, nullptr);
  r.order = perm;
  return rt_trace_rays_enqueue(s, &q, r, stream);
}

extern "C" {

int rt_trace_rays_device(rt_scene* s, const rt_params* p, const rt_ray_batch* b, const rt_ray_radiance* out, void* hip_stream) {
  rt_params q;
  int rc = check_call(s, p, b, out, "rt_trace_rays_device", &q);
  if (rc != RT_OK) return rc;
  if (b->n_rays == 0) return RT_OK;
  if (s->progress_active) return fail(RT_ERR_INVALID_ARG, "a progressive render owns this scene until rt_render_end");
  return rt_trace_rays_enqueue(s, &q, args_of(b, out, nullptr), (hipStream_t)hip_stream);
}

int rt_trace_rays_ordered_device(rt_scene* s, const rt_params* p, const rt_ray_batch* b, const rt_ray_order* order, const rt_ray_radiance* out,
                                 void* hip_stream) {
  const char* fn = "rt_trace_rays_ordered_device";
  rt_params q;
  int rc = check_call(s, p, b, out, fn, &q);
  if (rc != RT_OK) return rc;
  if (!order) return fail(RT_ERR_INVALID_ARG, "%s: null ray order (the device form allocates nothing: build one with rt_ray_order_build_device)", fn);
  if ((rc = check_order_use(order, b, fn)) != RT_OK) return rc;
  if (b->n_rays == 0) return RT_OK;
  if (s->progress_active) return fail(RT_ERR_INVALID_ARG, "a progressive render owns this scene until rt_render_end");
  if ((rc = check_order_device(order, s, fn)) != RT_OK) return rc;
  return rt_trace_rays_enqueue(s, &q, args_of(b, out, order), (hipStream_t)hip_stream);
}

int rt_trace_rays(rt_scene* s, const rt_params* p, const rt_ray_batch* b, const rt_ray_radiance* out, rt_stats* stats) {
  return trace_host(s, p, b, nullptr, false, out, stats, "rt_trace_rays");
}

int rt_trace_rays_ordered(rt_scene* s, const rt_params* p, const rt_ray_batch* b, const rt_ray_order* order, const rt_ray_radiance* out,
                          rt_stats* stats) {
  return trace_host(s, p, b, order, order == nullptr, out, stats, "rt_trace_rays_ordered");
}

// ---- ray orders ---------------------------------------------------------------------------------------------------------------
int rt_ray_order_create(const rt_ray_order_desc* d, int device, rt_ray_order** out) {
  if (!d || !out) return fail(RT_ERR_INVALID_ARG, "rt_ray_order_create: null argument");
  *out = nullptr;
  if (d->abi_version != RT_ABI_VERSION)
    return fail(RT_ERR_INVALID_ARG, "rt_ray_order_create: rt_ray_order_desc.abi_version %u != %u", d->abi_version, RT_ABI_VERSION);
  if (d->capacity == 0) return fail(RT_ERR_INVALID_ARG, "rt_ray_order_create: capacity 0");
  if (d->capacity > RT_ORDER_MAX_RAYS) return fail(RT_ERR_INVALID_ARG, "rt_ray_order_create: capacity %u exceeds the %u rays an order sorts", d->capacity, RT_ORDER_MAX_RAYS);
  if (d->origin_bits > RT_KEY_AXIS_BITS) return fail(RT_ERR_INVALID_ARG, "rt_ray_order_create: origin_bits %u > %u", d->origin_bits, RT_KEY_AXIS_BITS);
  if (d->reserved) return fail(RT_ERR_INVALID_ARG, "rt_ray_order_create: rt_ray_order_desc.reserved must be 0");
  int rc = rt_open_device(device);
  if (rc != RT_OK) return rc;
  rt_ray_order* o = new rt_ray_order();
  o->device = device, o->capacity = d->capacity, o->origin_bits = d->origin_bits;
  rc = order_alloc(o);
  if (rc != RT_OK) {
    order_free(o);
    return rc;
  }
  *out = o;
  return RT_OK;
}

void rt_ray_order_destroy(rt_ray_order* o) { order_free(o); }

int rt_ray_order_build_device(rt_ray_order* o, const rt_ray_batch* b, void* hip_stream) {
  const int rc = check_order_batch(o, b, "rt_ray_order_build_device");
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(o->device));
  return order_enqueue(o, b->origin, b->direction, b->n_rays, (hipStream_t)hip_stream);
}

int rt_ray_order_build(rt_ray_order* o, const rt_ray_batch* b) {
  int rc = check_order_batch(o, b, "rt_ray_order_build");
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(o->device));
  if ((rc = o->built.wait()) != RT_OK) return rc;
  const size_t n = b->n_rays;
  if (n == 0) return order_enqueue(o, nullptr, nullptr, 0, nullptr);
  const float *d_o = b->origin, *d_d = b->direction;
  HostCall c;
  c.in(&d_o, n * 12), c.in(&d_d, n * 12);
  EventPair ev;
  if ((rc = ev.create()) != RT_OK || (rc = c.begin()) != RT_OK) return rc;
  HIP_TRY(hipEventRecord(ev.e0, c.stream));
  if ((rc = order_enqueue(o, d_o, d_d, b->n_rays, c.stream)) != RT_OK) return rc;
  HIP_TRY(hipEventRecord(ev.e1, c.stream));
  if ((rc = c.finish()) != RT_OK) return rc;
  o->built.clear();
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  o->device_ms = ms;
  return RT_OK;
}

int rt_ray_order_set(rt_ray_order* o, const uint32_t* perm, uint32_t n) {
  if (!o) return fail(RT_ERR_INVALID_ARG, "rt_ray_order_set: null ray order");
  if (n > o->capacity) return fail(RT_ERR_INVALID_ARG, "rt_ray_order_set: %u rays exceed the order's capacity of %u", n, o->capacity);
  int rc = rt_check_permutation(perm, n);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(o->device));
  if ((rc = o->built.wait()) != RT_OK) return rc;
  if (n) HIP_TRY(hipMemcpy(o->ws.idx_b, perm, (size_t)n * 4, hipMemcpyHostToDevice));
  o->n = n, o->ready = true, o->has_keys = false, o->device_ms = 0.0;
  return RT_OK;
}

int rt_ray_order_read(rt_ray_order* o, uint32_t* perm, uint32_t* keys, rt_ray_order_info* info) {
  if (!o) return fail(RT_ERR_INVALID_ARG, "rt_ray_order_read: null ray order");
  if (!o->ready) return fail(RT_ERR_INVALID_ARG, "rt_ray_order_read: the ray order has never been built or set");
  if (keys && !o->has_keys) return fail(RT_ERR_INVALID_ARG, "rt_ray_order_read: an order given by rt_ray_order_set has no keys");
  HIP_TRY(hipSetDevice(o->device));
  const int rc = o->built.wait();
  if (rc != RT_OK) return rc;
  if (perm && o->n) HIP_TRY(hipMemcpy(perm, o->ws.idx_b, (size_t)o->n * 4, hipMemcpyDeviceToHost));
  if (keys && o->n) HIP_TRY(hipMemcpy(keys, o->ws.keys, (size_t)o->n * 4, hipMemcpyDeviceToHost));
  if (info) {
    *info = rt_ray_order_info{};
    info->n_rays = o->n, info->bytes = rt_ray_order_bytes(o), info->device_ms = o->device_ms;
    if (o->has_keys && o->n) {
      RtKeyFrame f;
      HIP_TRY(hipMemcpy(&f, o->ws.frame, sizeof(f), hipMemcpyDeviceToHost));
      info->n_live = f.n_live, info->origin_bits = f.origin_bits, info->direction_bits = f.direction_bits;
      info->n_origin_axes = f.n_origin_axes, info->n_direction_axes = f.n_direction_axes;
    }
  }
  return RT_OK;
}

}  // extern "C"
