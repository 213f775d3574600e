// rt_occlusion.cpp -- the ambient-occlusion entry points of include/rt_hip.h: rt_ambient_occlusion[_device] on a scene handle,
// rt_ambient_occlusion_model, the specification: a linear scan of a scene description with the functions of rt_occlusion.h, and
// rt_occlusion_rays_model, the rays the definition casts.
//
// As the other queries (rt_query.cpp, rt_closest.cpp, rt_multihit.cpp), a call reads only the scene's device arrays
// (RtDevScene): no frame slot, counter block or parameter table is touched, so it may run on any stream beside renders.  The
// _device form allocates nothing, has no workspace and only enqueues ONE launch; the host form stages the batch through device
// memory of its own for the call.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "rt_host.h"

namespace {

// validation shared by the entry points; runs before any HIP call
int check_batch(const rt_occlusion_batch* b, const char* fn) {
  if (!b) return fail(RT_ERR_INVALID_ARG, "%s: null occlusion batch", fn);
  if (b->abi_version != RT_ABI_VERSION)
    return fail(RT_ERR_INVALID_ARG, "%s: rt_occlusion_batch.abi_version %u != %u", fn, b->abi_version, RT_ABI_VERSION);
  if (b->n_points && (!b->point || !b->normal || !b->table)) return fail(RT_ERR_INVALID_ARG, "%s: point / normal / table missing", fn);
  if (b->n_samples < 1u || b->n_samples > RT_MAX_OCCLUSION_SAMPLES)
    return fail(RT_ERR_INVALID_ARG, "%s: n_samples %u outside 1 .. %u", fn, b->n_samples, RT_MAX_OCCLUSION_SAMPLES);
  if (b->n_table == 0u) return fail(RT_ERR_INVALID_ARG, "%s: n_table is 0", fn);
  if (!std::isfinite(b->bias)) return fail(RT_ERR_INVALID_ARG, "%s: bias is not finite", fn);
  if (b->flags & ~RT_OCCLUSION_PASS_TRANSMISSIVE)
    return fail(RT_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x (only RT_OCCLUSION_PASS_TRANSMISSIVE)", fn, b->flags & ~RT_OCCLUSION_PASS_TRANSMISSIVE);
  return RT_OK;
}
int check_call(bool have_scene, const rt_occlusion_batch* b, const rt_occlusion_out* o, const char* fn) {
  if (!have_scene) return fail(RT_ERR_INVALID_ARG, "%s: null scene", fn);
  if (b && !o)  // (a null batch is reported first, by check_batch)
    return fail(RT_ERR_INVALID_ARG, "%s: null output struct", fn);
  const int rc = check_batch(b, fn);
  if (rc != RT_OK) return rc;
  if (!(o->bits || o->clear || o->visibility || o->bent_normal)) return fail(RT_ERR_INVALID_ARG, "%s: every output plane is NULL", fn);
  return RT_OK;
}

RtOcclusionArgs args_of(const rt_occlusion_batch* b, const rt_occlusion_out* o) {
  RtOcclusionArgs a;
  memset(&a, 0, sizeof(a));
  a.point = b->point, a.normal = b->normal, a.table = b->table, a.first = b->first;
  a.bias = b->bias, a.max_distance = b->max_distance;
  a.n = b->n_points, a.n_samples = b->n_samples, a.n_table = b->n_table, a.pass = (b->flags & RT_OCCLUSION_PASS_TRANSMISSIVE) ? 1u : 0u;
  if (o) a.bits = o->bits, a.clear = o->clear, a.visibility = o->visibility, a.bent_normal = o->bent_normal;
  return a;
}

int launch(rt_scene* s, const RtOcclusionArgs& a, hipStream_t stream) {
  const hipError_t e = (hipError_t)rt_launch_occlusion(s->dev, a, stream);
  if (e != hipSuccess) return fail(RT_ERR_HIP, "ambient-occlusion launch failed: %s", hipGetErrorString(e));
  return RT_OK;
}

}  // namespace

static_assert(RT_OCC_SMAX == RT_MAX_OCCLUSION_SAMPLES, "the bit words of rt_occlusion.h hold RT_MAX_OCCLUSION_SAMPLES samples");

extern "C" {

int rt_ambient_occlusion(rt_scene* s, const rt_occlusion_batch* b, const rt_occlusion_out* o) {
  const int rc0 = check_call(s != nullptr, b, o, "rt_ambient_occlusion");
  if (rc0 != RT_OK || b->n_points == 0) return rc0;
  HIP_TRY(hipSetDevice(s->device));
  const size_t n = b->n_points;
  RtOcclusionArgs a = args_of(b, o);
  HostCall c;
  c.in(&a.point, n * 12), c.in(&a.normal, n * 12), c.in(&a.table, (size_t)b->n_table * 12), c.in(&a.first, n * 4);
  c.out(&a.bits, n * rt_occ_words(b->n_samples) * 4), c.out(&a.clear, n * 4), c.out(&a.visibility, n * 4), c.out(&a.bent_normal, n * 12);
  int rc = c.begin();
  if (rc == RT_OK) rc = launch(s, a, c.stream);
  return rc == RT_OK ? c.finish() : rc;
}

int rt_ambient_occlusion_device(rt_scene* s, const rt_occlusion_batch* b, const rt_occlusion_out* o, void* hip_stream) {
  const int rc = check_call(s != nullptr, b, o, "rt_ambient_occlusion_device");
  if (rc != RT_OK || b->n_points == 0) return rc;
  HIP_TRY(hipSetDevice(s->device));
  return launch(s, args_of(b, o), (hipStream_t)hip_stream);
}

int rt_ambient_occlusion_model(const rt_scene_desc* d, const rt_occlusion_batch* b, const rt_occlusion_out* o) {
  const int rc = check_call(d != nullptr, b, o, "rt_ambient_occlusion_model");
  if (rc != RT_OK) return rc;
  const int rd = rt_check_scene_desc(d);
  if (rd != RT_OK) return rd;
  const RtOcclusionArgs a = args_of(b, o);
  const RtMhDesc S = {d};
  for (uint32_t i = 0; i < a.n; i++) rt_occ_query_host(S, RtOccArgsRef{a}, i);
  return RT_OK;
}

int rt_occlusion_rays_model(const rt_occlusion_batch* b, float* origin, float* direction, uint8_t* alive) {
  const int rc = check_batch(b, "rt_occlusion_rays_model");
  if (rc != RT_OK) return rc;
  const RtOcclusionArgs a = args_of(b, nullptr);
  const RtOccArgsRef A{a};
  for (uint32_t i = 0; i < a.n; i++) {
    RtOccPoint P;
    rt_occ_point(A, i, true, P);
    if (alive) alive[i] = P.alive ? 1 : 0;
    if (origin)
      for (int k = 0; k < 3; k++) origin[3u * (size_t)i + k] = P.o[k];
    if (direction)
      for (uint32_t s = 0; s < a.n_samples; s++)
        rt_occ_direction(P, a.table + 3u * (size_t)rt_occ_row(P.row0, s, a.n_table), direction + 3u * ((size_t)i * a.n_samples + s));
  }
  return RT_OK;
}

}  // extern "C"
