// rt_rays.cpp -- the radiance-query entry points of include/rt_hip.h: rt_trace_rays[_device], the reference's
// single_raytrace (src/renderer/raytracer_renderer.rs:147-264) for a batch of rays the caller supplies.
//
// Unlike the queries of rt_query.cpp a radiance call IS a render call: it goes through the frame scheduler of rt_api.cpp
// (rt_trace_rays_enqueue) as a frame of n x 1 pixels and uses the scene's parameter tables, frame slots and workspaces.
// What is here: validation (before any HIP call), the parameters of that frame, and the host form's staging.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>

#include "rt_host.h"

namespace {

bool any_plane(const rt_ray_radiance* o) { return o && (o->rgb || o->valid || o->id || o->t || o->argb); }

// Validation shared by both entry points; runs before any HIP call and before the scene is looked at.  On success *q is
// the frame the scheduler runs: the caller's shading parameters, its camera members replaced by "n rays, one row".
int check_call(const rt_scene* s, const rt_params* p, const rt_ray_batch* b, const rt_ray_radiance* out, const char* fn, rt_params* q) {
  if (!s) return fail(RT_ERR_INVALID_ARG, "%s: null scene", fn);
  if (!p) return fail(RT_ERR_INVALID_ARG, "%s: null shading parameters", fn);
  if (!b) return fail(RT_ERR_INVALID_ARG, "%s: null ray batch", fn);
  if (!out) return fail(RT_ERR_INVALID_ARG, "%s: null output struct", fn);
  if (p->abi_version != RT_ABI_VERSION)
    return fail(RT_ERR_INVALID_ARG, "%s: rt_params.abi_version %u != %u", fn, p->abi_version, RT_ABI_VERSION);
  if (b->abi_version != RT_ABI_VERSION)
    return fail(RT_ERR_INVALID_ARG, "%s: rt_ray_batch.abi_version %u != %u", fn, b->abi_version, RT_ABI_VERSION);
  if (b->max_distance) return fail(RT_ERR_INVALID_ARG, "%s: rt_ray_batch.max_distance must be NULL (a radiance ray has no length limit)", fn);
  if (b->flags) return fail(RT_ERR_INVALID_ARG, "%s: rt_ray_batch.flags must be 0 (backface culling comes from the shading flags)", fn);
  if (p->flags & RT_FLAG_ANTI_ALIASING)
    return fail(RT_ERR_INVALID_ARG, "%s: RT_FLAG_ANTI_ALIASING in the shading flags (the caller supplies its samples as rays)", fn);
  if (b->n_rays && (!b->origin || !b->direction)) return fail(RT_ERR_INVALID_ARG, "%s: origin / direction missing", fn);
  if (!any_plane(out)) return fail(RT_ERR_INVALID_ARG, "%s: every output plane is NULL", fn);
  *q = *p;
  q->width = b->n_rays ? b->n_rays : 1u, q->height = 1u;
  q->aa_rays = 0, q->aa_offsets = nullptr;
  q->win_x0 = q->win_y0 = q->win_w = q->win_h = 0;
  q->tile_size = 0, q->n_ranks = 0, q->rank = 0;
  // ignored for ray batches: the merged-level and phase kernels and the tile order belong to the camera
  q->tuning.levels = RT_LEVELS_CHAINED, q->tuning.phases = RT_PHASES_FUSED, q->tuning.tile_order = RT_TILE_ORDER_DEFAULT, q->tuning.no_aa_dedup = 0;
  const int rc = rt_validate_params(q);  // clouds, depths, tuning ranges; "frame too large" = more than 2^31 - 1 rays
  if (rc != RT_OK) return rc;
  if ((q->flags & (RT_FLAG_REFLECTIONS | RT_FLAG_REFRACTIONS)) && q->max_depth_reflection == 0 && q->max_depth_refraction == 0)
    return fail(RT_ERR_INVALID_ARG, "%s: secondary rays enabled with depth 0", fn);
  return RT_OK;
}

RtRayArgs args_of(const rt_ray_batch* b, const rt_ray_radiance* o) {
  RtRayArgs r;
  memset(&r, 0, sizeof(r));
  r.origin = b->origin, r.direction = b->direction, r.n = b->n_rays;
  r.rgb = o->rgb, r.valid = o->valid, r.id = o->id, r.t = o->t, r.argb = o->argb;
  return r;
}

struct Staging {  // one device allocation for a host call: inputs, then every requested plane (256-byte aligned each)
  DevBuf buf;
  size_t used = 0;
  static size_t pad(size_t bytes) { return (bytes + 255u) & ~(size_t)255u; }
  char* take(size_t bytes) {
    char* p = (char*)buf.p + used;
    used += pad(bytes);
    return p;
  }
  ~Staging() { buf.release(); }
};

struct Plane {  // a host output plane and its device twin
  void* host;
  void** dev;
  size_t bytes;
  bool upload;  // argb: a miss leaves the caller's value, so the caller's plane goes up first
};

}  // namespace

extern "C" {

int rt_trace_rays_device(rt_scene* s, const rt_params* p, const rt_ray_batch* b, const rt_ray_radiance* out, void* hip_stream) {
  rt_params q;
  int rc = check_call(s, p, b, out, "rt_trace_rays_device", &q);
  if (rc != RT_OK) return rc;
  if (b->n_rays == 0) return RT_OK;
  if (s->progress_active) return fail(RT_ERR_INVALID_ARG, "a progressive render owns this scene until rt_render_end");
  return rt_trace_rays_enqueue(s, &q, args_of(b, out), (hipStream_t)hip_stream);
}

int rt_trace_rays(rt_scene* s, const rt_params* p, const rt_ray_batch* b, const rt_ray_radiance* out, rt_stats* stats) {
  rt_params q;
  int rc = check_call(s, p, b, out, "rt_trace_rays", &q);
  if (rc != RT_OK) return rc;
  if (stats) memset(stats, 0, sizeof(*stats));
  if (b->n_rays == 0) return RT_OK;
  if (s->progress_active) return fail(RT_ERR_INVALID_ARG, "a progressive render owns this scene until rt_render_end");
  HIP_TRY(hipSetDevice(s->device));
  const auto t_begin = std::chrono::steady_clock::now();
  const size_t n = b->n_rays;
  RtRayArgs r = args_of(b, out);
  Plane planes[5];
  int np = 0;
  if (out->rgb) planes[np++] = {out->rgb, (void**)&r.rgb, n * 12, false};
  if (out->valid) planes[np++] = {out->valid, (void**)&r.valid, n, false};
  if (out->id) planes[np++] = {out->id, (void**)&r.id, n * 4, false};
  if (out->t) planes[np++] = {out->t, (void**)&r.t, n * 4, false};
  if (out->argb) planes[np++] = {out->argb, (void**)&r.argb, n * 4, true};
  size_t total = 2 * Staging::pad(n * 12);
  for (int k = 0; k < np; k++) total += Staging::pad(planes[k].bytes);
  Staging st;
  if ((rc = st.buf.ensure(total)) != RT_OK) return rc;
  float* d_o = (float*)st.take(n * 12);
  float* d_d = (float*)st.take(n * 12);
  for (int k = 0; k < np; k++) *planes[k].dev = st.take(planes[k].bytes);
  r.origin = d_o, r.direction = d_d;
  // a private stream: the call neither waits for nor delays work the caller has on the null stream
  hipStream_t stream = nullptr;
  HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  struct StreamGuard {  // (the scene remembers streams -- of table uploads, of its frame slots: not this one, once it is gone)
    rt_scene* scene;
    hipStream_t s;
    ~StreamGuard() { (void)hipStreamSynchronize(s), rt_scene_forget_stream(scene, s), (void)hipStreamDestroy(s); }
  } guard{s, stream};
  EventPair ev;
  HIP_TRY(hipEventCreate(&ev.e0));
  HIP_TRY(hipEventCreate(&ev.e1));
  HIP_TRY(hipMemcpyAsync(d_o, b->origin, n * 12, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_d, b->direction, n * 12, hipMemcpyHostToDevice, stream));
  for (int k = 0; k < np; k++)
    if (planes[k].upload) HIP_TRY(hipMemcpyAsync(*planes[k].dev, planes[k].host, planes[k].bytes, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipEventRecord(ev.e0, stream));
  if ((rc = rt_trace_rays_enqueue(s, &q, r, stream)) != RT_OK) return rc;
  HIP_TRY(hipEventRecord(ev.e1, stream));
  for (int k = 0; k < np; k++) HIP_TRY(hipMemcpyAsync(planes[k].host, *planes[k].dev, planes[k].bytes, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  if (stats) {
    if ((rc = rt_render_collect_stats(s, stats)) != RT_OK) return rc;
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    stats->kernel_ms = ms;  // (with secondary rays: every attempt of the batch, and the waits for its counters)
    stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  }
  return RT_OK;
}

}  // extern "C"
