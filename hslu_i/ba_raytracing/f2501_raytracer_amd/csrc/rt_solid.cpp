// rt_solid.cpp -- the containment and signed-distance entry points of include/rt_hip.h: rt_contains_points[_device] and
// rt_signed_distance[_device] on a scene handle, and rt_contains_points_model / rt_signed_distance_model, the specification: a
// linear scan of a scene description with the functions of rt_solid.h (and, for the distance, rt_closest_points_model).
//
// As the other queries (rt_query.cpp, rt_closest.cpp, rt_multihit.cpp, rt_occlusion.cpp), a call reads only the scene's device
// arrays (RtDevScene): no frame slot, counter block or parameter table is touched, so it may run on any stream beside renders.
// The _device forms allocate nothing and only enqueue: rt_contains_points_device ONE launch, rt_signed_distance_device the
// closest-point kernel, unchanged, and then the containment kernel on the same stream -- the two walks share nothing, and kept
// apart the bit equality with rt_closest_points is a fact of construction.  The direction table is a host array in every form:
// it is validated here and travels to the kernel by value.  The host forms stage the batch through device memory of their own.
#include <hip/hip_runtime.h>

#include <cstring>

#include "rt_host.h"

namespace {

bool any_solid(const rt_solid_out& o) { return o.inside || o.votes || o.crossings || o.winding; }
bool any_closest(const rt_point_hits& h) { return h.id || h.distance || h.point || h.normal || h.bary || h.material; }

// validation shared by the entry points; runs before any HIP call
int check_batch(bool have_scene, const rt_solid_batch* b, bool have_out, const char* fn) {
  if (!have_scene) return fail(RT_ERR_INVALID_ARG, "%s: null scene", fn);
  if (!b) return fail(RT_ERR_INVALID_ARG, "%s: null solid batch", fn);
  if (!have_out) return fail(RT_ERR_INVALID_ARG, "%s: null output struct", fn);
  if (b->abi_version != RT_ABI_VERSION)
    return fail(RT_ERR_INVALID_ARG, "%s: rt_solid_batch.abi_version %u != %u", fn, b->abi_version, RT_ABI_VERSION);
  if (b->n_points && !b->point) return fail(RT_ERR_INVALID_ARG, "%s: point missing", fn);
  if (b->n_directions < 1u || b->n_directions > RT_MAX_SOLID_DIRECTIONS)
    return fail(RT_ERR_INVALID_ARG, "%s: n_directions %u outside 1 .. %u", fn, b->n_directions, RT_MAX_SOLID_DIRECTIONS);
  if (!b->directions) return fail(RT_ERR_INVALID_ARG, "%s: directions missing", fn);
  if (b->rule != RT_SOLID_RULE_PARITY && b->rule != RT_SOLID_RULE_WINDING)
    return fail(RT_ERR_INVALID_ARG, "%s: unknown rule %u (RT_SOLID_RULE_PARITY or RT_SOLID_RULE_WINDING)", fn, b->rule);
  for (uint32_t r = 0; r < b->n_directions; r++)
    if (!rt_solid_direction_ok(b->directions + 3u * (size_t)r))
      return fail(RT_ERR_INVALID_ARG, "%s: direction %u (%g, %g, %g) does not normalise to finite components", fn, r, (double)b->directions[3u * r],
                  (double)b->directions[3u * r + 1u], (double)b->directions[3u * r + 2u]);
  return RT_OK;
}
int check_contains(bool have_scene, const rt_solid_batch* b, const rt_solid_out* o, const char* fn) {
  const int rc = check_batch(have_scene, b, o != nullptr, fn);
  if (rc != RT_OK) return rc;
  if (!any_solid(*o)) return fail(RT_ERR_INVALID_ARG, "%s: every output plane is NULL", fn);
  return RT_OK;
}
int check_signed(bool have_scene, const rt_solid_batch* b, const rt_signed_distance_out* o, const char* fn) {
  const int rc = check_batch(have_scene, b, o != nullptr, fn);
  if (rc != RT_OK) return rc;
  if (!(o->signed_distance || any_solid(o->solid) || any_closest(o->closest))) return fail(RT_ERR_INVALID_ARG, "%s: every output plane is NULL", fn);
  return RT_OK;
}

RtSolidArgs solid_args(const rt_solid_batch* b, const rt_solid_out& o, float* signed_distance) {
  RtSolidArgs a;
  memset(&a, 0, sizeof(a));
  a.point = b->point, a.n = b->n_points, a.n_dirs = b->n_directions, a.rule = b->rule;
  memcpy(a.dir, b->directions, (size_t)b->n_directions * 12u);
  a.inside = o.inside, a.votes = o.votes, a.crossings = o.crossings, a.winding = o.winding, a.signed_distance = signed_distance;
  return a;
}
RtClosestArgs closest_args(const rt_solid_batch* b, const rt_point_hits& h) {
  RtClosestArgs a;
  memset(&a, 0, sizeof(a));
  a.point = b->point, a.max_distance = b->max_distance, a.n = b->n_points;
  a.id = h.id, a.distance = h.distance, a.out_point = h.point, a.normal = h.normal, a.bary = h.bary, a.material = h.material;
  return a;
}
// The two halves of a signed-distance call share the point plane and the distance plane: without a `distance` plane of the
// caller's the closest-point part writes the unsigned distance into `signed_distance`, where the containment part signs it.
// Called once the pointers are the ones the work will use (the host form: after staging).  -> which halves run
struct Halves {
  bool closest, solid;
};
Halves join(RtClosestArgs& ca, RtSolidArgs& sa) {
  ca.point = sa.point;
  if (!ca.distance) ca.distance = sa.signed_distance;
  sa.distance = sa.signed_distance ? ca.distance : nullptr;
  Halves h;
  h.closest = ca.id || ca.distance || ca.out_point || ca.normal || ca.bary || ca.material;
  h.solid = sa.inside || sa.votes || sa.crossings || sa.winding || sa.signed_distance;
  return h;
}

int launch_solid(rt_scene* s, const RtSolidArgs& a, hipStream_t stream) {
  const hipError_t e = (hipError_t)rt_launch_solid(s->dev, a, stream);
  if (e != hipSuccess) return fail(RT_ERR_HIP, "containment launch failed: %s", hipGetErrorString(e));
  return RT_OK;
}
int launch_signed(rt_scene* s, RtClosestArgs& ca, RtSolidArgs& sa, hipStream_t stream) {
  const Halves h = join(ca, sa);
  if (h.closest) {
    const hipError_t e = (hipError_t)rt_launch_closest(s->dev, ca, stream);
    if (e != hipSuccess) return fail(RT_ERR_HIP, "closest-point launch failed: %s", hipGetErrorString(e));
  }
  return h.solid ? launch_solid(s, sa, stream) : RT_OK;
}

void stage_solid(HostCall& c, RtSolidArgs& a, size_t n) {
  c.in(&a.point, n * 12);
  c.out(&a.inside, n), c.out(&a.votes, n), c.out(&a.crossings, n * a.n_dirs * 4), c.out(&a.winding, n * a.n_dirs * 4), c.out(&a.signed_distance, n * 4);
}

}  // namespace

static_assert(RT_SOLID_RMAX == RT_MAX_SOLID_DIRECTIONS, "the direction table of rt_solid.h holds RT_MAX_SOLID_DIRECTIONS rows");
static_assert(RT_SOLID_PARITY == RT_SOLID_RULE_PARITY && RT_SOLID_WINDING == RT_SOLID_RULE_WINDING, "the rules of rt_solid.h are rt_hip.h's");

extern "C" {

int rt_contains_points(rt_scene* s, const rt_solid_batch* b, const rt_solid_out* o) {
  int rc = check_contains(s != nullptr, b, o, "rt_contains_points");
  if (rc == RT_OK) rc = rt_check_solid(s->dev, "rt_contains_points");
  if (rc != RT_OK || b->n_points == 0) return rc;
  HIP_TRY(hipSetDevice(s->device));
  RtSolidArgs a = solid_args(b, *o, nullptr);
  HostCall c;
  stage_solid(c, a, b->n_points);
  rc = c.begin();
  if (rc == RT_OK) rc = launch_solid(s, a, c.stream);
  return rc == RT_OK ? c.finish() : rc;
}

int rt_contains_points_device(rt_scene* s, const rt_solid_batch* b, const rt_solid_out* o, void* hip_stream) {
  int rc = check_contains(s != nullptr, b, o, "rt_contains_points_device");
  if (rc == RT_OK) rc = rt_check_solid(s->dev, "rt_contains_points_device");
  if (rc != RT_OK || b->n_points == 0) return rc;
  HIP_TRY(hipSetDevice(s->device));
  return launch_solid(s, solid_args(b, *o, nullptr), (hipStream_t)hip_stream);
}

int rt_signed_distance(rt_scene* s, const rt_solid_batch* b, const rt_signed_distance_out* o) {
  int rc = check_signed(s != nullptr, b, o, "rt_signed_distance");
  if (rc == RT_OK) rc = rt_check_solid(s->dev, "rt_signed_distance");
  if (rc != RT_OK || b->n_points == 0) return rc;
  HIP_TRY(hipSetDevice(s->device));
  const size_t n = b->n_points;
  RtSolidArgs sa = solid_args(b, o->solid, o->signed_distance);
  RtClosestArgs ca = closest_args(b, o->closest);
  ca.point = nullptr;  // (staged once, as the containment part's)
  HostCall c;
  stage_solid(c, sa, n);
  c.in(&ca.max_distance, n * 4);
  c.out(&ca.id, n * 4), c.out(&ca.distance, n * 4), c.out(&ca.out_point, n * 12), c.out(&ca.normal, n * 12), c.out(&ca.bary, n * 8),
      c.out(&ca.material, n * 4);
  rc = c.begin();
  if (rc == RT_OK) rc = launch_signed(s, ca, sa, c.stream);
  return rc == RT_OK ? c.finish() : rc;
}

int rt_signed_distance_device(rt_scene* s, const rt_solid_batch* b, const rt_signed_distance_out* o, void* hip_stream) {
  int rc = check_signed(s != nullptr, b, o, "rt_signed_distance_device");
  if (rc == RT_OK) rc = rt_check_solid(s->dev, "rt_signed_distance_device");
  if (rc != RT_OK || b->n_points == 0) return rc;
  HIP_TRY(hipSetDevice(s->device));
  RtSolidArgs sa = solid_args(b, o->solid, o->signed_distance);
  RtClosestArgs ca = closest_args(b, o->closest);
  return launch_signed(s, ca, sa, (hipStream_t)hip_stream);
}

int rt_contains_points_model(const rt_scene_desc* d, const rt_solid_batch* b, const rt_solid_out* o) {
  const int rc = check_contains(d != nullptr, b, o, "rt_contains_points_model");
  if (rc != RT_OK) return rc;
  const int rd = rt_check_scene_desc(d);
  if (rd != RT_OK) return rd;
  const RtSolidArgs a = solid_args(b, *o, nullptr);
  const RtMhDesc S = {d};
  for (uint32_t i = 0; i < a.n; i++) rt_solid_query(S, RtSolidArgsRef{a}, i, true);
  return RT_OK;
}

int rt_signed_distance_model(const rt_scene_desc* d, const rt_solid_batch* b, const rt_signed_distance_out* o) {
  const int rc = check_signed(d != nullptr, b, o, "rt_signed_distance_model");
  if (rc != RT_OK) return rc;
  const int rd = rt_check_scene_desc(d);
  if (rd != RT_OK) return rd;
  if (b->n_points == 0) return RT_OK;
  RtSolidArgs sa = solid_args(b, o->solid, o->signed_distance);
  RtClosestArgs ca = closest_args(b, o->closest);
  const Halves h = join(ca, sa);
  if (h.closest) {
    const rt_point_batch pb = {RT_ABI_VERSION, b->n_points, b->point, b->max_distance};
    const rt_point_hits ph = {ca.id, ca.distance, ca.out_point, ca.normal, ca.bary, ca.material};
    const int rp = rt_closest_points_model(d, &pb, &ph);
    if (rp != RT_OK) return rp;
  }
  if (h.solid) {
    const RtMhDesc S = {d};
    for (uint32_t i = 0; i < sa.n; i++) rt_solid_query(S, RtSolidArgsRef{sa}, i, true);
  }
  return RT_OK;
}

}  // extern "C"
