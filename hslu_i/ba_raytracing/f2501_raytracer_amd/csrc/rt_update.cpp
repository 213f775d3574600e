// rt_update.cpp -- rt_scene_update / rt_scene_update_device: the stateful half of an in-place scene update.  What the
// update computes is in rt_refit.h (host model: rt_refit_packed, kernels: rt_update.hip); here: the device copy of the
// refit plan, the checks, the waits on either side of the kernels, the staging of host arrays, and which of the scene's
// cached tables an update invalidates.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>

#include "rt_host.h"
#include "rt_sah.h"

// the device copy of RtRefitPlan: [height_nodes | thr_src | recv_cell | tri_slot | 8 words: bounds, counter], 256-byte aligned parts
int rt_scene_upload_plan(rt_scene* s, const RtPackedScene& pk) {
  s->plan = pk.plan;
  const std::vector<uint32_t>* parts[4] = {&s->plan.height_nodes, &s->plan.thr_src, &s->plan.recv_cell, &s->plan.tri_slot};
  const size_t part_bytes[4] = {parts[0]->size() * 4, parts[1]->size() * 4, parts[2]->size() * 4, parts[3]->size() * 4};
  int rc = s->plan_dev.ensure(rt_plan_layout(part_bytes, s->plan_off));
  if (rc != RT_OK) return rc;
  for (int k = 0; k < 4; k++)
    if (!parts[k]->empty()) HIP_TRY(hipMemcpy((char*)s->plan_dev.p + s->plan_off[k], parts[k]->data(), parts[k]->size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset((char*)s->plan_dev.p + s->plan_off[4], 0, 256));
  return RT_OK;
}

void rt_scene_release_update(rt_scene* s) {
  s->plan_dev.release();
  s->upd_dev.release();
  s->sah_dev.release();
  if (s->upd_stage) (void)hipHostFree(s->upd_stage);
  if (s->upd_back) (void)hipHostFree(s->upd_back);
  s->upd_stage = nullptr, s->upd_back = nullptr, s->upd_stage_cap = 0;
}

int rt_scene_wait_frames(rt_scene* s) {
  if (s->tables_pending) {
    HIP_TRY(hipStreamSynchronize(s->tables_stream));
    s->tables_pending = false;
  }
  for (int b = 0; b < RT_SLOTS; b++)
    if (s->frame_pending[b]) {
      HIP_TRY(hipEventSynchronize(s->frame_ev[b]));
      s->frame_pending[b] = false;
    }
  return RT_OK;
}

namespace {

// the arrays of a delta as one run of floats: {array, floats} in staging order (sphere_r_inv is not read: not staged)
struct Group {
  const float* rt_scene_delta::*member;
  size_t floats;
};
size_t delta_groups(const rt_scene* s, const rt_scene_delta* d, Group g[8]) {
  const size_t ns = s->dev.n_spheres, nt = d->tri_count, nm = s->plan.mat_class.size(), nl = s->dev.n_lights;
  size_t n = 0;
  if (d->sphere_center) g[n++] = {&rt_scene_delta::sphere_center, 3 * ns}, g[n++] = {&rt_scene_delta::sphere_r_sq, ns};
  if (d->tri_count) {
    g[n++] = {&rt_scene_delta::tri_v1, 3 * nt}, g[n++] = {&rt_scene_delta::tri_e1, 3 * nt};
    g[n++] = {&rt_scene_delta::tri_e2, 3 * nt}, g[n++] = {&rt_scene_delta::tri_normal, 3 * nt};
  }
  if (d->materials) g[n++] = {&rt_scene_delta::materials, nm * RT_MATERIAL_STRIDE};
  if (d->lights) g[n++] = {&rt_scene_delta::lights, nl * RT_LIGHT_STRIDE};
  return n;
}

// `host`: the caller's delta of host arrays to stage first (null: `dev` holds the caller's device arrays already).
int update_impl(rt_scene* s, const rt_scene_delta* host, rt_scene_delta dev, hipStream_t stream, rt_update_info* info) {
  const auto t0 = std::chrono::steady_clock::now();
  HIP_TRY(hipSetDevice(s->device));
  // every frame of this scene still in flight reads the old records
  const int rc_wait = rt_scene_wait_frames(s);
  if (rc_wait != RT_OK) return rc_wait;
  if (!host && dev.materials) {  // the transmissive classes of device rows: read them back to check them
    std::vector<float> rows(s->plan.mat_class.size() * RT_MATERIAL_STRIDE);
    HIP_TRY(hipMemcpyAsync(rows.data(), dev.materials, rows.size() * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const int rc = rt_check_scene_delta(s->dev, s->plan, &dev, rows.data());
    if (rc != RT_OK) return rc;
  }
  if (!s->upd_back) HIP_TRY(hipHostMalloc((void**)&s->upd_back, 32, hipHostMallocDefault));
  EventPair ev;
  const int rc_ev = ev.create();
  if (rc_ev != RT_OK) return rc_ev;
  HIP_TRY(hipEventRecord(ev.e0, stream));
  if (host) {  // one pinned buffer, one copy; the groups follow one another, each on a multiple of 16 bytes
    Group g[8];
    const size_t n = delta_groups(s, host, g);
    size_t bytes = 0;
    for (size_t k = 0; k < n; k++) bytes += (g[k].floats * 4 + 15) / 16 * 16;
    if (bytes > s->upd_stage_cap) {
      if (s->upd_stage) (void)hipHostFree(s->upd_stage);
      s->upd_stage = nullptr, s->upd_stage_cap = 0;
      HIP_TRY(hipHostMalloc(&s->upd_stage, bytes, hipHostMallocDefault));
      s->upd_stage_cap = bytes;
    }
    const int rc = s->upd_dev.ensure(bytes);
    if (rc != RT_OK) return rc;
    size_t off = 0;
    for (size_t k = 0; k < n; k++) {
      memcpy((char*)s->upd_stage + off, host->*(g[k].member), g[k].floats * 4);
      dev.*(g[k].member) = (const float*)((const char*)s->upd_dev.p + off);
      off += (g[k].floats * 4 + 15) / 16 * 16;
    }
    if (dev.sphere_center) dev.sphere_r_inv = dev.sphere_r_sq;  // (present, never read)
    if (bytes) HIP_TRY(hipMemcpyAsync(s->upd_dev.p, s->upd_stage, bytes, hipMemcpyHostToDevice, stream));
  }
  char* plan = (char*)s->plan_dev.p;
  RtUpdateArgs u{};
  u.base = (char*)s->blob.p;
  u.flag_geo = s->n_cells ? (float*)s->flag_geo.p : nullptr;
  u.height_nodes = (const uint32_t*)(plan + s->plan_off[0]);
  u.thr_src = (const uint32_t*)(plan + s->plan_off[1]);
  u.recv_cell = (const uint32_t*)(plan + s->plan_off[2]);
  u.tri_slot = (const uint32_t*)(plan + s->plan_off[3]);
  u.bounds = (float*)(plan + s->plan_off[4]);
  u.height_offset = s->plan.height_offset.data();
  u.n_heights = s->plan.height_offset.empty() ? 0u : (uint32_t)s->plan.height_offset.size() - 1u;
  u.n_materials = (uint32_t)s->plan.mat_class.size();
  uint32_t n_launches = 0;
  const hipError_t e = (hipError_t)rt_launch_update(s->dev, u, dev, stream, &n_launches);
  if (e != hipSuccess) return fail(RT_ERR_HIP, "scene update launch failed: %s", hipGetErrorString(e));
  const bool geometry = dev.sphere_center || dev.tri_count;
  if (geometry) HIP_TRY(hipMemcpyAsync(s->upd_back, u.bounds, 32, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipEventRecord(ev.e1, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  if (geometry) {  // the Morton frame of the next frame and the FAR_ORIGINS test of its receiver cells follow these
    memcpy(s->aabb_lo, s->upd_back, 12), memcpy(s->aabb_hi, s->upd_back + 3, 12);
    memcpy(&s->plan.receivers_disabled, s->upd_back + 6, 4);
  }
  // what the scene has cached about its old contents
  uint32_t inval = RT_UPDATE_INVALIDATES_QUEUE_SIZES;  // (a material alone changes the ray counts)
  s->stream_verified = false, s->est_valid = false, s->key_gen++;
  if (geometry || dev.lights) {
    inval |= RT_UPDATE_INVALIDATES_RECEIVER_TABLES | RT_UPDATE_INVALIDATES_TILE_COSTS;
    s->flags_key[0] = -1.f;  // the next soft-shadow frame reruns rt_flags_kernel (flags and cell lists)
    s->cell_lists_built = false;
    s->cost_valid = false;
  }
  if (info) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    info->device_ms = ms;
    info->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    info->nodes_refitted = dev.tri_count ? s->dev.n_nodes : 0u;
    info->slots_rewritten = dev.tri_count;  // (triangle groups are refused on split-clipped trees: one slot per triangle)
    info->receivers_disabled = s->plan.receivers_disabled;
    info->tables_invalidated = inval;
  }
  return RT_OK;
}

int check_handle(const rt_scene* s, const rt_scene_delta* d) {
  if (!s || !d) return fail(RT_ERR_INVALID_ARG, "null argument");
  if (s->progress_active) return fail(RT_ERR_INVALID_ARG, "a progressive render owns this scene until rt_render_end");
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_scene_update(rt_scene* s, const rt_scene_delta* d, rt_update_info* info) {
  int rc = check_handle(s, d);
  if (rc == RT_OK) rc = rt_check_scene_delta(s->dev, s->plan, d, d->materials);
  if (rc != RT_OK) return rc;
  return update_impl(s, d, *d, nullptr, info);
}

int rt_scene_update_device(rt_scene* s, const rt_scene_delta* d, void* hip_stream, rt_update_info* info) {
  int rc = check_handle(s, d);
  if (rc == RT_OK) rc = rt_check_scene_delta(s->dev, s->plan, d, nullptr);  // (material classes: update_impl, after a read-back)
  if (rc != RT_OK) return rc;
  return update_impl(s, nullptr, *d, (hipStream_t)hip_stream, info);
}

// The SAH report of the tree as it stands.  A stream of its own: the call neither waits for nor delays the caller's frames.
int rt_scene_bvh_quality(rt_scene* s, rt_bvh_quality* out) {
  if (!s || !out) return fail(RT_ERR_INVALID_ARG, "rt_scene_bvh_quality: null argument");
  *out = rt_bvh_quality{};
  if (!s->dev.n_triangles) return RT_OK;
  HIP_TRY(hipSetDevice(s->device));
  struct Stream {  // destroyed on every return path
    hipStream_t st = nullptr;
    ~Stream() {
      if (st) (void)hipStreamSynchronize(st), (void)hipStreamDestroy(st);
    }
  } q;
  HIP_TRY(hipStreamCreateWithFlags(&q.st, hipStreamNonBlocking));
  EventPair ev;
  const int rc = ev.create();
  if (rc != RT_OK) return rc;
  HIP_TRY(hipEventRecord(ev.e0, q.st));
  unsigned long long* dev = (unsigned long long*)s->sah_dev.p;
  const hipError_t e = (hipError_t)rt_launch_sah((const RtNode*)((const char*)s->blob.p + s->dev.off_nodes), s->dev.n_nodes, dev, q.st);
  if (e != hipSuccess) return fail(RT_ERR_HIP, "SAH report launch failed: %s", hipGetErrorString(e));
  HIP_TRY(hipEventRecord(ev.e1, q.st));
  unsigned long long host[3] = {0, 0, 0};
  HIP_TRY(hipMemcpyAsync(host, dev, sizeof(host), hipMemcpyDeviceToHost, q.st));
  HIP_TRY(hipStreamSynchronize(q.st));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  const double cost = (double)s->sah_tri_cost;
  out->inner_q = host[0], out->leaf_q = host[1], out->n_bad = (uint32_t)host[2];
  out->sah_created = ((double)s->sah_created[0] + cost * (double)s->sah_created[1]) / RT_SAH_ONE;
  out->sah_now = ((double)host[0] + cost * (double)host[1]) / RT_SAH_ONE;
  out->device_ms = ms;
  return RT_OK;
}

}  // extern "C"
