// rt_multihit.cpp -- the multi-hit entry points of include/rt_hip.h: rt_list_intersections[_device] on a scene handle and
// rt_list_intersections_model, the specification: a linear scan of a scene description with the functions of rt_multihit.h.
//
// As the other queries (rt_query.cpp, rt_closest.cpp), a call reads only the scene's device arrays (RtDevScene): no frame slot,
// counter block or parameter table is touched, so it may run on any stream beside renders.  The _device form allocates nothing
// and only enqueues; the host form stages the batch through device memory of its own for the call.
#include <hip/hip_runtime.h>

#include <cstring>

#include "rt_host.h"

namespace {

bool any_plane(const rt_ray_hit_lists* l) { return l->count || l->total || l->id || l->t || l->point || l->normal || l->material; }

// validation shared by the three entry points; runs before any HIP call
int check_call(bool have_scene, const rt_ray_batch* b, const rt_ray_hit_lists* l, const char* fn) {
  if (!have_scene) return fail(RT_ERR_INVALID_ARG, "%s: null scene", fn);
  if (b && !l)  // (a null batch is reported first, by rt_check_ray_batch)
    return fail(RT_ERR_INVALID_ARG, "%s: null output struct", fn);
  const int rc = rt_check_ray_batch(b, fn);
  if (rc != RT_OK) return rc;
  if (b->flags & ~RT_FLAG_BACKFACE_CULLING)
    return fail(RT_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x (only RT_FLAG_BACKFACE_CULLING)", fn, b->flags & ~RT_FLAG_BACKFACE_CULLING);
  if (l->max_hits < 1u || l->max_hits > RT_MAX_HITS_PER_RAY)
    return fail(RT_ERR_INVALID_ARG, "%s: max_hits %u outside 1 .. %u", fn, l->max_hits, RT_MAX_HITS_PER_RAY);
  if ((l->after_t == nullptr) != (l->after_id == nullptr))
    return fail(RT_ERR_INVALID_ARG, "%s: after_t and after_id are given together or not at all", fn);
  if (!any_plane(l)) return fail(RT_ERR_INVALID_ARG, "%s: every output plane is NULL", fn);
  return RT_OK;
}

RtMultiHitArgs args_of(const rt_ray_batch* b, const rt_ray_hit_lists* l) {
  RtMultiHitArgs a;
  memset(&a, 0, sizeof(a));
  a.origin = b->origin, a.direction = b->direction, a.max_distance = b->max_distance, a.n = b->n_rays;
  a.cull = (b->flags & RT_FLAG_BACKFACE_CULLING) ? 1u : 0u;
  a.max_hits = l->max_hits, a.after_t = l->after_t, a.after_id = l->after_id;
  a.count = l->count, a.total = l->total, a.id = l->id, a.t = l->t, a.point = l->point, a.normal = l->normal, a.material = l->material;
  return a;
}

int launch(rt_scene* s, const RtMultiHitArgs& a, hipStream_t stream) {
  const hipError_t e = (hipError_t)rt_launch_multihit(s->dev, a, stream);
  if (e != hipSuccess) return fail(RT_ERR_HIP, "multi-hit launch failed: %s", hipGetErrorString(e));
  return RT_OK;
}

}  // namespace

static_assert(RT_MH_KMAX == RT_MAX_HITS_PER_RAY, "the list of rt_multihit.h holds RT_MAX_HITS_PER_RAY entries");

extern "C" {

int rt_list_intersections(rt_scene* s, const rt_ray_batch* b, const rt_ray_hit_lists* l) {
  const int rc0 = check_call(s != nullptr, b, l, "rt_list_intersections");
  if (rc0 != RT_OK || b->n_rays == 0) return rc0;
  HIP_TRY(hipSetDevice(s->device));
  const size_t n = b->n_rays, nk = n * l->max_hits;
  RtMultiHitArgs a = args_of(b, l);
  HostCall c;
  c.in(&a.origin, n * 12), c.in(&a.direction, n * 12), c.in(&a.max_distance, n * 4), c.in(&a.after_t, n * 4), c.in(&a.after_id, n * 4);
  c.out(&a.count, n * 4), c.out(&a.total, n * 4), c.out(&a.id, nk * 4), c.out(&a.t, nk * 4), c.out(&a.point, nk * 12),
      c.out(&a.normal, nk * 12), c.out(&a.material, nk * 4);
  int rc = c.begin();
  if (rc == RT_OK) rc = launch(s, a, c.stream);
  return rc == RT_OK ? c.finish() : rc;
}

int rt_list_intersections_device(rt_scene* s, const rt_ray_batch* b, const rt_ray_hit_lists* l, void* hip_stream) {
  const int rc = check_call(s != nullptr, b, l, "rt_list_intersections_device");
  if (rc != RT_OK || b->n_rays == 0) return rc;
  HIP_TRY(hipSetDevice(s->device));
  return launch(s, args_of(b, l), (hipStream_t)hip_stream);
}

int rt_list_intersections_model(const rt_scene_desc* d, const rt_ray_batch* b, const rt_ray_hit_lists* l) {
  const int rc = check_call(d != nullptr, b, l, "rt_list_intersections_model");
  if (rc != RT_OK) return rc;
  const int rd = rt_check_scene_desc(d);
  if (rd != RT_OK) return rd;
  const RtMultiHitArgs a = args_of(b, l);
  const RtMhDesc S = {d};
  for (uint32_t i = 0; i < a.n; i++) rt_mh_query<RT_MH_KMAX>(S, RtMhArgsRef{a}, i, true);
  return RT_OK;
}

}  // extern "C"
