// rt_api.cpp -- the C ABI of include/rt_hip.h over the HIP runtime: everything on the host that is stateful.
//
// rt_scene owns the device copies of the flattened Scene (reference src/scene/scene.rs:24-27), the
// BVH, and reusable device workspaces (parameter tables, counters, ray queues, accumulator), so a
// render call performs no allocation when its shape repeats (graph-capture friendly: rt_render_device
// only enqueues async work on the caller's stream).
// What is in this file: scene creation as an upload of what rt_pack_scene laid out (rt_scene_pack.cpp), prepare() -- when
// a frame's parameter tables are rebuilt and when they may be overwritten; their contents come from rt_tables.cpp -- and
// the frame scheduler.  Byte layouts and table arithmetic are NOT here: they make no HIP call and are tested on the CPU.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rt_cell_resolve.h"
#include "rt_cell_through.h"
#include "rt_host.h"

static void trace_point(hipStream_t stream, const char* what, uint32_t a = 0, uint32_t b = 0, uint32_t c = 0);  // RT_TRACE_LAUNCHES
#define RC_TRY(expr) do { const int rc_ = (expr); if (rc_ != RT_OK) return rc_; } while (0)

extern "C" {

#ifndef RT_BUILD_ID
#define RT_BUILD_ID "unknown"
#endif
const char* rt_build_id(void) { return RT_BUILD_ID; }

int rt_selftest_exact_math(int device, const float* in, float* out_sqrt, float* out_rcp, uint32_t n) {
  if (!in || !out_sqrt || !out_rcp) return fail(RT_ERR_INVALID_ARG, "null argument");
  if (device < 0 || device >= rt_device_count()) return fail(RT_ERR_INVALID_ARG, "device %d out of range", device);
  HIP_TRY(hipSetDevice(device));
  DevBuf b;
  int rc = b.ensure((size_t)n * 12 + 12);
  if (rc != RT_OK) return rc;
  float* d = (float*)b.p;
  HIP_TRY(hipMemcpy(d, in, (size_t)n * 4, hipMemcpyHostToDevice));
  hipError_t e = (hipError_t)rt_launch_selftest_math(d, d + n, d + 2 * (size_t)n, n, nullptr);
  if (e != hipSuccess) {
    b.release();
    return fail(RT_ERR_HIP, "selftest launch failed: %s", hipGetErrorString(e));
  }
  hipError_t e1 = hipMemcpy(out_sqrt, d + n, (size_t)n * 4, hipMemcpyDeviceToHost);
  hipError_t e2 = hipMemcpy(out_rcp, d + 2 * (size_t)n, (size_t)n * 4, hipMemcpyDeviceToHost);
  b.release();
  if (e1 != hipSuccess || e2 != hipSuccess) return fail(RT_ERR_HIP, "selftest copy failed");
  return RT_OK;
}

int rt_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

void rt_scene_destroy(rt_scene* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  if (s->tables_ev) (void)hipEventDestroy(s->tables_ev);
  for (hipEvent_t e : s->frame_ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& w : s->ws) {
    if (w.cnt_ev) (void)hipEventDestroy(w.cnt_ev);
    if (w.cnt_host) (void)hipHostFree(w.cnt_host);
    if (w.fork_ev) (void)hipEventDestroy(w.fork_ev);
    w.acc.release();
    for (auto& l : w.lane) {
      if (l.stream) (void)hipStreamSynchronize(l.stream), (void)hipStreamDestroy(l.stream);
      if (l.done_ev) (void)hipEventDestroy(l.done_ev);
      for (int k = 0; k < 2; k++) {
        if (l.shade_stream[k]) (void)hipStreamSynchronize(l.shade_stream[k]), (void)hipStreamDestroy(l.shade_stream[k]);
        if (l.shade_done[k]) (void)hipEventDestroy(l.shade_done[k]);
      }
      for (hipEvent_t e : l.level_ev) (void)hipEventDestroy(e);
      if (l.hit_ev) (void)hipEventDestroy(l.hit_ev);
      for (DevBuf* b : {&l.queues, &l.qcount, &l.trace_ws, &l.hard, &l.hitrec, &l.sets}) b->release();
    }
  }
  for (DevBuf* b : {&s->blob, &s->aa, &s->cloud, &s->counters, &s->suplist, &s->fb, &s->aux_rgb, &s->costmap, &s->aux_id, &s->aux_t, &s->flag_geo, &s->flags, &s->cell_lists, &s->resolve_work, &s->cell_wide, &s->progress_fb, &s->rays_argb})
    b->release();
  rt_scene_release_update(s);
  delete s;
}

static int upload(DevBuf& b, const void* src, size_t bytes) {
  int rc = b.ensure(bytes);
  if (rc != RT_OK) return rc;
  if (bytes) {
    hipError_t e = hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(RT_ERR_HIP, "hipMemcpy H2D failed: %s", hipGetErrorString(e));
  }
  return RT_OK;
}

// what the scene looks like in device memory is decided by rt_pack_scene (rt_scene_pack.cpp); this uploads it
int rt_scene_create(const rt_scene_desc* d, int device, rt_scene** out) {
  if (!d || !out) return fail(RT_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  int rc = rt_check_scene_desc(d);
  if (rc != RT_OK) return rc;
  if ((rc = rt_open_device(device)) != RT_OK) return rc;

  rt_scene* s = new rt_scene();
  s->device = device;
  s->budget = d->device_budget_bytes ? d->device_budget_bytes : RT_SCENE_BUDGET_DEFAULT;
  RtPackedScene pk;
  rc = rt_pack_scene(d, s->budget, &pk);
  if (rc == RT_OK && pk.n_cells) {  // receiver flags: their kernel's input now, the flags when a frame first needs them (prepare())
    rc = upload(s->flag_geo, pk.flag_geo.data(), pk.flag_geo.size() * 4);
    if (rc == RT_OK) rc = s->flags.ensure((size_t)pk.n_cells * 2 + 64);
  }
  if (rc == RT_OK) rc = s->counters.ensure(RT_SLOTS * RT_COUNTER_REPLICAS * 16 * sizeof(unsigned long long));
  if (rc == RT_OK) rc = upload(s->blob, pk.blob.data(), pk.blob.size());
  if (rc == RT_OK) rc = rt_scene_upload_plan(s, pk);  // (in-place updates: rt_update.cpp)
  if (rc == RT_OK) rc = s->sah_dev.ensure(256);
  if (rc == RT_OK) {  // (SAH report: the sums of creation)
    rt_sah_packed(pk, s->sah_created, nullptr);
    s->sah_tri_cost = d->bvh.tri_cost > 0.f ? d->bvh.tri_cost : 2.0f;  // (as rt_build_bvh applies it)
  }
  if (rc != RT_OK) {
    rt_scene_destroy(s);
    return rc;
  }
  s->dev = pk.dev;
  s->dev.base = (const char*)s->blob.p;
  s->info = pk.info;
  s->n_cells = pk.n_cells;
  s->n_tri_cells = pk.n_tri_cells;
  s->bytes_bvh = pk.bytes_bvh;
  s->max_leaf = pk.max_leaf;
  memcpy(s->aabb_lo, pk.aabb_lo, sizeof(s->aabb_lo));
  memcpy(s->aabb_hi, pk.aabb_hi, sizeof(s->aabb_hi));
  *out = s;
  return RT_OK;
}

int rt_scene_bvh_info(const rt_scene* s, rt_bvh_info* out) {
  if (!s || !out) return fail(RT_ERR_INVALID_ARG, "null argument");
  *out = s->info;
  return RT_OK;
}

int rt_scene_memory_info(const rt_scene* s, rt_scene_info* out) {
  if (!s || !out) return fail(RT_ERR_INVALID_ARG, "null argument");
  memset(out, 0, sizeof(*out));
  out->bytes_bvh = s->bytes_bvh;
  out->bytes_geometry = s->blob.cap > s->bytes_bvh ? s->blob.cap - s->bytes_bvh : 0;
  out->bytes_flags = s->flags.cap + s->flag_geo.cap;
  out->bytes_cell_lists = s->cell_lists.cap + s->resolve_work.cap + s->cell_wide.cap;
  out->bytes_tables = s->aa.cap + s->cloud.cap + s->counters.cap + s->suplist.cap + s->costmap.cap;
  for (const auto& w : s->ws) {
    out->bytes_workspace += w.bytes();
    for (const auto& l : w.lane) out->bytes_workspace += l.qcount.cap;
  }
  out->bytes_frames = s->fb.cap + s->aux_rgb.cap + s->aux_id.cap + s->aux_t.cap + s->progress_fb.cap + s->rays_argb.cap;
  out->bytes_total = out->bytes_geometry + out->bytes_bvh + out->bytes_flags + out->bytes_cell_lists + out->bytes_tables + out->bytes_workspace +
                     out->bytes_frames;
  out->budget_bytes = s->budget;
  out->n_receiver_cells = s->n_cells;
  out->cell_lists_built = s->cell_lists_built ? 1u : 0u;
  return RT_OK;
}

}  // extern "C"

int rt_validate_params(const rt_params* p) {
  if (!p) return fail(RT_ERR_INVALID_ARG, "null params");
  if (p->abi_version != RT_ABI_VERSION)
    return fail(RT_ERR_INVALID_ARG, "rt_params.abi_version %u != %u", p->abi_version, RT_ABI_VERSION);
  if (p->width == 0 || p->height == 0) return fail(RT_ERR_INVALID_ARG, "empty frame");
  if ((uint64_t)p->width * p->height > 0x7FFFFFFFull) return fail(RT_ERR_INVALID_ARG, "frame too large");
  if (p->win_w && (p->win_x0 + (uint64_t)p->win_w > p->width || p->win_y0 + (uint64_t)p->win_h > p->height || !p->win_h))
    return fail(RT_ERR_INVALID_ARG, "window outside the frame");
  if ((p->flags & RT_FLAG_ANTI_ALIASING) && p->aa_rays > 0 && !p->aa_offsets)
    return fail(RT_ERR_INVALID_ARG, "aa_offsets missing");
  if (p->light_mult > 1 && (!p->cloud_sets || p->n_cloud_sets == 0))
    return fail(RT_ERR_INVALID_ARG, "cloud_sets missing");
  if (p->n_ranks > 1 && p->rank >= p->n_ranks) return fail(RT_ERR_INVALID_ARG, "rank out of range");
  if (p->n_ranks > 1 && p->tile_size != 0 && p->tile_size < 16) return fail(RT_ERR_UNSUPPORTED, "tile_size < 16");
  if (p->traversal > RT_TRAVERSAL_LINEAR) return fail(RT_ERR_INVALID_ARG, "unknown traversal mode");
  if (p->max_depth_reflection > RT_MAX_DEPTH || p->max_depth_refraction > RT_MAX_DEPTH)
    return fail(RT_ERR_UNSUPPORTED, "recursion depth > %u", RT_MAX_DEPTH);
  if (p->tuning.shadow_candidate_cap > 64u && p->tuning.shadow_candidate_cap != RT_CAND_CAP_NONE)
    return fail(RT_ERR_INVALID_ARG, "tuning.shadow_candidate_cap > 64");
  if (p->tuning.chunk_log2 && (p->tuning.chunk_log2 < 10u || p->tuning.chunk_log2 > 26u))
    return fail(RT_ERR_INVALID_ARG, "tuning.chunk_log2 outside 10..26");
  if (p->tuning.sort_bits && (p->tuning.sort_bits < 12u || p->tuning.sort_bits > 24u))
    return fail(RT_ERR_INVALID_ARG, "tuning.sort_bits outside 12..24");
  if (p->tuning.sub_frames > RT_LANES) return fail(RT_ERR_INVALID_ARG, "tuning.sub_frames > %u", (unsigned)RT_LANES);
  if (p->tuning.levels > RT_LEVELS_PIPELINED) return fail(RT_ERR_INVALID_ARG, "tuning.levels > %u", (unsigned)RT_LEVELS_PIPELINED);
  if (p->tuning.phases > RT_PHASES_FUSED_DEFER) return fail(RT_ERR_INVALID_ARG, "tuning.phases > %u", (unsigned)RT_PHASES_FUSED_DEFER);
  return RT_OK;
}

// ---- prepare: the device parameter block of a frame --------------------------------------------------------------------
// prepare() fills RtDevParams, uploading tables as needed.  What goes INTO a table is arithmetic without a HIP call
// (rt_tables.cpp); what is here is the stateful part: when a table must be rebuilt, when it may be overwritten, on which
// stream.  Its stages, in order: copy_view, prepare_aa_table, prepare_cloud_table, prepare_receiver_flags,
// copy_frame_shape, take_frame_slot, prepare_super_tiles, TableUpload::finish.

// A table may only be overwritten once the frames that read the old one are done, and kernels on another stream may only
// start once the upload has landed.
struct TableUpload {
  rt_scene* s;
  hipStream_t stream;
  bool uploaded = false;
  // before a table (device copy or its host staging vector) is written
  int begin() {
    if (!s->tables_ev) HIP_TRY(hipEventCreateWithFlags(&s->tables_ev, hipEventDisableTiming));
    // (also covers the host staging vectors: the previous asynchronous upload has read them by now)
    if (s->tables_pending) HIP_TRY(hipStreamSynchronize(s->tables_stream));
    for (int b = 0; b < RT_SLOTS; b++)  // every frame still in flight (on whatever stream) reads the old tables
      if (s->frame_pending[b]) HIP_TRY(hipEventSynchronize(s->frame_ev[b]));
    uploaded = true;
    s->tables_version++;
    return RT_OK;
  }
  // once per prepare(): marks this stream's uploads, or makes the stream wait for those of another
  int finish() {
    if (uploaded) {
      HIP_TRY(hipEventRecord(s->tables_ev, stream));
      s->tables_stream = stream;
      s->tables_pending = true;
    } else if (s->tables_pending && s->tables_stream != stream) {
      HIP_TRY(hipStreamWaitEvent(stream, s->tables_ev, 0));
    }
    return RT_OK;
  }
};

static void copy_view(const rt_params* p, RtDevParams* P) {
  memset(P, 0, sizeof(*P));
  P->width = p->width;
  P->height = p->height;
  memcpy(P->focus, p->focus, sizeof(P->focus));
  P->fw = p->fw, P->fh = p->fh, P->fd = p->fd;
  P->eps_distance = p->eps_distance;
  P->air_ior = p->air_ior;
  P->ambient = p->ambient;
  P->flags = p->flags;
  const bool aa = (p->flags & RT_FLAG_ANTI_ALIASING) && p->aa_rays > 0;
  P->aa_rays = aa ? p->aa_rays : 0;
  P->aa_unique = 1;
}

// AA samples: bit-identical repeats of an offset are traced once (rt_build_aa_table)
static int prepare_aa_table(rt_scene* s, const rt_params* p, TableUpload& up, RtDevParams* P) {
  if (!P->aa_rays) return RT_OK;
  const size_t n = p->aa_rays;
  const bool dedup = !p->tuning.no_aa_dedup;
  if (s->aa_host.size() != 2 * n || memcmp(s->aa_host.data(), p->aa_offsets, 2 * n * 4) != 0 || s->aa_dedup != dedup) {
    std::vector<uint32_t> table;
    const uint32_t U = rt_build_aa_table(p->aa_offsets, p->aa_rays, dedup, &table);
    RC_TRY(up.begin());
    s->aa_table.swap(table);
    RC_TRY(s->aa.ensure(s->aa_table.size() * 4));
    HIP_TRY(hipMemcpyAsync(s->aa.p, s->aa_table.data(), s->aa_table.size() * 4, hipMemcpyHostToDevice, up.stream));
    s->aa_host.assign(p->aa_offsets, p->aa_offsets + 2 * n);
    s->aa_unique = U;
    s->aa_dedup = dedup;
  }
  P->aa_unique = s->aa_unique;
  P->weighted = s->aa_unique != p->aa_rays;
  P->aa_offsets = (const float*)s->aa.p;
  P->aa_mult = (const uint32_t*)s->aa.p + 2 * (size_t)s->aa_unique;
  P->aa_src = (const uint32_t*)s->aa.p + 3 * (size_t)s->aa_unique;
  return RT_OK;
}

// light clouds: the scaled table, its bounding ball (cached with the table) and the beam constants that follow from it
static int prepare_cloud_table(rt_scene* s, const rt_params* p, TableUpload& up, RtDevParams* P) {
  P->light_mult = p->light_mult < 1 ? 1 : p->light_mult;
  P->cloud_seed = p->cloud_seed;
  P->n_cloud_sets = p->n_cloud_sets;
  if (P->light_mult <= 1) return RT_OK;
  const size_t n = (size_t)p->n_cloud_sets * P->light_mult * 3;
  const bool new_table = s->cloud_host.size() != n || memcmp(s->cloud_host.data(), p->cloud_sets, n * 4) != 0;
  const bool new_scale = s->cloud_ball_f[0] != p->fw || s->cloud_ball_f[1] != p->fh || s->cloud_ball_f[2] != p->fd;
  if (new_table || new_scale) {
    RC_TRY(up.begin());
    RC_TRY(s->cloud.ensure(n / 3 * 16));
    if (new_table) s->cloud_host.assign(p->cloud_sets, p->cloud_sets + n);
    s->cloud_ball_f[0] = p->fw, s->cloud_ball_f[1] = p->fh, s->cloud_ball_f[2] = p->fd;
    rt_scale_cloud(s->cloud_host.data(), n, s->cloud_ball_f, &s->cloud_scaled, s->cloud_ball);
    HIP_TRY(hipMemcpyAsync(s->cloud.p, s->cloud_scaled.data(), n / 3 * 16, hipMemcpyHostToDevice, up.stream));
  }
  P->cloud_sets = (const float4*)s->cloud.p;
  memcpy(P->cloud_centre, s->cloud_ball, 12);
  P->cloud_delta = s->cloud_ball[3];
  rt_beam_constants(p->eps_distance, P);
  const uint32_t cap = p->tuning.shadow_candidate_cap;
  P->cand_cap = cap == RT_CAND_CAP_NONE ? 0u : (cap ? cap : 64u);
  return RT_OK;
}

// receiver flags: cells no triangle / sphere can shadow for a light skip the candidate walk (rt_flags_kernel); the same
// kernel writes the per-cell candidate lists.  Both are rebuilt when the beam constants change.
static int prepare_receiver_flags(rt_scene* s, const rt_params* p, TableUpload& up, RtDevParams* P) {
  hipStream_t stream = up.stream;
  P->recv_flags = nullptr;
  // (why the flags are off, when they are: rt_stats.notes)
  if (p->tuning.no_receiver_flags || P->cand_cap == 0u) s->notes |= RT_NOTE_RECV_FLAGS_OFF_TUNING;
  if (!s->n_cells || !(P->cloud_delta > 0.0f)) s->notes |= RT_NOTE_RECV_FLAGS_OFF_SCENE;
  if (s->dev.n_lights > 8u) s->notes |= RT_NOTE_RECV_FLAGS_OFF_LIGHTS;
  if (p->traversal != RT_TRAVERSAL_BVH) s->notes |= RT_NOTE_RECV_FLAGS_OFF_TRAVERSAL;
  if (p->flags & RT_FLAG_BACKFACE_CULLING) s->notes |= RT_NOTE_RECV_FLAGS_OFF_CULLING;
  if (!p->tuning.no_receiver_flags && P->cand_cap != 0u && s->n_cells && s->dev.n_lights <= 8u && p->traversal == RT_TRAVERSAL_BVH &&
      !(p->flags & RT_FLAG_BACKFACE_CULLING) && P->cloud_delta > 0.0f) {
    const float key[8] = {P->beam_delta, p->eps_distance, P->cloud_centre[0], P->cloud_centre[1], P->cloud_centre[2], 1.f, 0.f, 0.f};
    if (memcmp(key, s->flags_key, sizeof(key)) != 0) {
      RC_TRY(up.begin());  // (waits for kernels of an earlier frame that read the old flags)
      RtDevParams B = *P;
      B.flag_out = (uint16_t*)s->flags.p;
      B.flag_geo = (const float4*)s->flag_geo.p;
      B.n_cells = s->n_cells;
      B.n_tri_cells = s->n_tri_cells;
      // per-cell candidate lists, written by the same kernel: 16 bytes per cell and light (16-bit leaf slots), when the
      // scene allows it and a quarter of the free memory holds them
      s->cell_lists_built = false;
      s->cell_wide_built = false;
      s->cell_marks_bytes = 0;
      B.cell_list_out = nullptr;
      const size_t list_bytes = (size_t)s->n_cells * s->dev.n_lights * 16u;
      size_t free_b = 0, total_b = 0;
      const size_t flag_bytes = s->flags.cap + s->flag_geo.cap;
      if (s->dev.n_slots <= 65533u && flag_bytes + list_bytes <= s->budget && hipMemGetInfo(&free_b, &total_b) == hipSuccess &&
          list_bytes <= (free_b + s->cell_lists.cap) / 4 && s->cell_lists.ensure(list_bytes + 64) == RT_OK) {
        HIP_TRY(hipMemsetAsync(s->cell_lists.p, 0xFF, list_bytes, stream));
        B.cell_list_out = (uint16_t*)s->cell_lists.p;
        s->cell_lists_built = true;
      }
      if (!s->cell_lists_built) s->cell_lists.release();  // (a table built under an earlier, larger need)
      hipError_t e = (hipError_t)rt_launch_flags(s->dev, B, stream);
      if (e != hipSuccess) return fail(RT_ERR_HIP, "rt_flags_kernel launch failed: %s", hipGetErrorString(e));
      trace_point(stream, "rt_flags_kernel: cells, lights, lists", s->n_cells, s->dev.n_lights, s->cell_lists_built ? 1u : 0u);
      // the lists thinned out by the sharper per-cell rule (rt_cell_prune.h): same stream, same key, so it reruns whenever
      // the flags do.  RT_CELL_PRUNE=0 (read once per process) leaves it out (A/B timing, equality tests).
      static const char* const prune_env = getenv("RT_CELL_PRUNE");
      static const bool prune_off = prune_env && *prune_env == '0';
      // marks of the listed glass panes every shadow ray of a cell crosses (rt_cell_through.h): a fourth stage behind the same key,
      // after the lists have their final form.  One byte per list, in front of the wide records in their allocation, counted
      // against the budget before the later stages' temporary memory and pool are sized; RT_CELL_THROUGH=0 (read once per
      // process) leaves it out.
      static const char* const through_env = getenv("RT_CELL_THROUGH");
      static const bool through_off = through_env && *through_env == '0';
      size_t mark_bytes = s->cell_lists_built && !through_off ? rt_cell_through_bytes(s->n_cells, s->dev.n_lights, s->budget - flag_bytes - list_bytes) : 0;
      if (mark_bytes && !(hipMemGetInfo(&free_b, &total_b) == hipSuccess && mark_bytes <= (free_b + s->cell_wide.cap) / 4)) mark_bytes = 0;
      RtCellPruneArgs a{};
      if (s->cell_lists_built) {
        a.flag_geo = (const float*)s->flag_geo.p;
        a.lists = (uint16_t*)s->cell_lists.p;
        a.flags = (uint16_t*)s->flags.p;
        a.n_cells = s->n_cells, a.n_tri_cells = s->n_tri_cells;
        memcpy(a.cloud_centre, P->cloud_centre, 12);
        a.beam_delta = P->beam_delta, a.beam_eps_o = P->beam_eps_o;
        a.mode = RT_PRUNE_FULL;
      }
      if (s->cell_lists_built && !prune_off) {
        e = (hipError_t)rt_launch_cell_prune(s->dev, a, stream);
        if (e != hipSuccess) return fail(RT_ERR_HIP, "rt_cell_prune_kernel launch failed: %s", hipGetErrorString(e));
        trace_point(stream, "rt_cell_prune_kernel: cells, lights", s->n_cells, s->dev.n_lights, 0u);
        // lists that overflowed under the fat beam, enumerated again under the sharper rule (rt_cell_resolve.h): a third stage
        // behind the same key.  Its work list counts against the budget as the lists do; RT_CELL_RESOLVE=0 (read once per
        // process) leaves it out, and so does RT_CELL_PRUNE=0.
        static const char* const resolve_env = getenv("RT_CELL_RESOLVE");
        static const bool resolve_off = resolve_env && *resolve_env == '0';
        RtCellResolveArgs r{};
        const size_t temp_bytes = resolve_off ? 0 : rt_cell_resolve_temp_bytes(s->n_cells, s->budget - flag_bytes - list_bytes - mark_bytes, &r.chunk_cells);
        if (temp_bytes && s->resolve_work.ensure(temp_bytes) == RT_OK) {
          r.cell = a;
          r.eps_push = P->beam_eps_push, r.eps_ulp = P->beam_eps_ulp;
          r.work = (uint32_t*)s->resolve_work.p;
          // lists with 9 to 32 survivors go to a pool of 64-byte records, sized from what the budget still leaves and counted
          // with the lists; the stage empties it whenever it runs.  RT_CELL_WIDE=0 (read once per process) leaves it out.
          static const char* const wide_env = getenv("RT_CELL_WIDE");
          static const bool wide_off = wide_env && *wide_env == '0';
          const size_t used = flag_bytes + list_bytes + temp_bytes + mark_bytes;
          const size_t wide_bytes = wide_off || used >= s->budget ? 0 : rt_cell_wide_pool_bytes(s->n_cells, s->dev.n_lights, s->budget - used, &r.wide_cap);
          if (wide_bytes && hipMemGetInfo(&free_b, &total_b) == hipSuccess && mark_bytes + wide_bytes <= (free_b + s->cell_wide.cap) / 4 &&
              s->cell_wide.ensure(mark_bytes + wide_bytes) == RT_OK) {
            r.wide = (uint16_t*)((char*)s->cell_wide.p + mark_bytes);  // (the records behind the marks, at 64-byte boundaries)
            r.wide_count = (uint32_t*)((char*)r.wide + (size_t)r.wide_cap * 2u * RT_CELL_WIDE_SLOTS);
            s->cell_wide_built = true;
          } else {
            r.wide_cap = 0u;
          }
          e = (hipError_t)rt_launch_cell_resolve(s->dev, r, stream);
          if (e != hipSuccess) return fail(RT_ERR_HIP, "rt_cell_resolve_kernel launch failed: %s", hipGetErrorString(e));
          trace_point(stream, "rt_cell_resolve_kernel: cells, lights, cells per chunk", s->n_cells, s->dev.n_lights, r.chunk_cells);
        } else {
          s->resolve_work.release();
        }
      }
      if (mark_bytes && (s->cell_wide_built || s->cell_wide.ensure(mark_bytes + 64u) == RT_OK)) {  // (no pool: the marks alone)
        RtCellThroughArgs t{};
        t.cell = a;
        t.marks_end = (uint8_t*)s->cell_wide.p + mark_bytes;
        e = (hipError_t)rt_launch_cell_through(s->dev, t, stream);
        if (e != hipSuccess) return fail(RT_ERR_HIP, "rt_cell_through_kernel launch failed: %s", hipGetErrorString(e));
        trace_point(stream, "rt_cell_through_kernel: cells, lights", s->n_cells, s->dev.n_lights, 0u);
        s->cell_wide_built = true;
        s->cell_marks_bytes = mark_bytes;
      }
      if (!s->cell_lists_built) s->resolve_work.release();
      if (!s->cell_wide_built) s->cell_wide.release();
      memcpy(s->flags_key, key, sizeof(key));
    }
    P->recv_flags = (const uint16_t*)s->flags.p;
    if (s->cell_lists_built && !p->tuning.no_cell_lists) P->cell_lists = (const uint4*)s->cell_lists.p;
    // (bit 0 of the pointer: the marks stand in front of the records; the list kernels, its only readers, take it off)
    if (P->cell_lists && s->cell_wide_built)
      P->cell_wide = (const uint32_t*)((uintptr_t)((char*)s->cell_wide.p + s->cell_marks_bytes) | (s->cell_marks_bytes ? 1u : 0u));
  }
  if (!P->cell_lists) s->notes |= RT_NOTE_CELL_LISTS_OFF;
  return RT_OK;
}

// recursion depths, the scheduler's wishes, window, tiling and outputs
static void copy_frame_shape(rt_scene* s, const rt_params* p, uint32_t* argb_dev, const rt_aux* aux_dev, RtDevParams* P) {
  P->max_depth_reflection = p->max_depth_reflection;
  P->max_depth_refraction = p->max_depth_refraction;
  s->sort_bits_wanted = p->tuning.sort_bits;
  s->lanes_wanted = p->tuning.sub_frames;
  s->phases_wanted = p->tuning.phases;
  s->levels_wanted = p->tuning.levels;
  if (p->win_w) {
    P->win_x0 = p->win_x0, P->win_y0 = p->win_y0, P->win_w = p->win_w, P->win_h = p->win_h;
  } else {
    P->win_x0 = P->win_y0 = 0;
    P->win_w = p->width;
    P->win_h = p->height;
  }
  P->tile_size = p->tile_size ? p->tile_size : 48u;
  P->n_ranks = p->n_ranks;
  P->rank = p->rank;
  P->traversal = p->traversal;
  P->argb = argb_dev;
  if (aux_dev) {
    P->aux_rgb = aux_dev->rgb;
    P->aux_hit_id = aux_dev->hit_id;
    P->aux_hit_t = aux_dev->hit_t;
  }
}

// This frame's slot (counter block + workspace set): one whose last frame has finished if there is one, else the one
// used longest ago -- whose frame this stream then waits for.
// (a slot whose last frame ran on THIS stream is taken first: the stream orders the two frames anyway, and a host that
// runs far ahead of the GPU on two streams then holds two workspace sets, not one per slot)
static int take_frame_slot(rt_scene* s, const rt_params* p, hipStream_t stream, RtDevParams* P) {
  int blk = -1, oldest = 0, same = -1;
  for (int b = 0; b < RT_SLOTS; b++) {
    if (!s->frame_ev[b]) HIP_TRY(hipEventCreateWithFlags(&s->frame_ev[b], hipEventDisableTiming));
    if (s->frame_pending[b] && hipEventQuery(s->frame_ev[b]) == hipSuccess) s->frame_pending[b] = false;
    if (blk < 0 && !s->frame_pending[b]) blk = b;
    if (same < 0 && s->frame_seq[b] && s->frame_stream[b] == stream) same = b;
    if (s->frame_seq[b] < s->frame_seq[oldest]) oldest = b;
  }
  if (same >= 0 && s->frame_pending[same]) blk = same;  // still running: queue up behind it on its stream
  if (blk < 0) blk = oldest;
  if (s->frame_pending[blk] && s->frame_stream[blk] != stream) HIP_TRY(hipStreamWaitEvent(stream, s->frame_ev[blk], 0));
  s->frame_stream[blk] = stream;
  s->frame_seq[blk] = ++s->frame_no;
  s->cur_block = blk;
  unsigned long long* blk_p = (unsigned long long*)s->counters.p + (size_t)blk * RT_COUNTER_REPLICAS * 16;
  P->counters = p->tuning.no_counters ? nullptr : blk_p;
  HIP_TRY(hipMemsetAsync(blk_p, 0, RT_COUNTER_REPLICAS * 16 * sizeof(unsigned long long), stream));
  return RT_OK;
}

// The super-tiles (16x16 pixels) this launch renders, in launch order.  Multi-GPU: only those that hold pixels of this
// rank's tiles.  RT_TILE_ORDER_COST: heaviest first, by the cost map measured on a calibration frame of this shape.
static int prepare_super_tiles(rt_scene* s, const rt_params* p, TableUpload& up, RtDevParams* P) {
  P->sup_list = nullptr;
  P->n_sup = ((P->win_w + 15u) / 16u) * ((P->win_h + 15u) / 16u);
  uint32_t order = p->tuning.tile_order == RT_TILE_ORDER_COST ? RT_TILE_ORDER_COST : RT_TILE_ORDER_ROW_MAJOR;
  if (order == RT_TILE_ORDER_COST && !rt_has_cost_kernel()) order = RT_TILE_ORDER_ROW_MAJOR, s->notes |= RT_NOTE_TILE_ORDER_COST_OFF;
  s->cost_wanted = false;
  if (order == RT_TILE_ORDER_COST) {
    // (the calibration frame times the super-tiles THIS rank owns, and only its primary kernel: secondary levels are not part of the cost)
    const uint32_t ck[13] = {P->win_x0, P->win_y0, P->win_w, P->win_h, P->width, P->height, P->flags, P->aa_rays, P->light_mult,
                             p->max_depth_reflection | (p->max_depth_refraction << 8) | (p->traversal << 16), P->n_ranks, P->rank, P->tile_size};
    if (memcmp(ck, s->cost_key, sizeof(ck)) != 0) s->cost_valid = false, memcpy(s->cost_key, ck, sizeof(ck));
    s->cost_wanted = !s->cost_valid;  // the caller runs the calibration frame (calibrate_costs)
  }
  if (P->n_ranks <= 1 && !(order == RT_TILE_ORDER_COST && s->cost_valid)) return RT_OK;  // all of the window, row-major
  const uint32_t key[8] = {P->win_x0, P->win_y0, P->win_w, P->win_h, P->tile_size, P->n_ranks, P->rank,
                           order == RT_TILE_ORDER_COST && s->cost_valid ? 2u : 1u};
  if (memcmp(key, s->sup_key, sizeof(key)) != 0 || s->sup_host.empty()) {
    RC_TRY(up.begin());
    rt_super_tiles(key, P->tile_size, P->n_ranks, P->rank, key[7] == 2u ? &s->cost_host : nullptr, &s->sup_host);
    memcpy(s->sup_key, key, sizeof(key));
    RC_TRY(s->suplist.ensure(s->sup_host.size() * 4 + 4));
    HIP_TRY(hipMemcpyAsync(s->suplist.p, s->sup_host.data(), s->sup_host.size() * 4, hipMemcpyHostToDevice, up.stream));
  }
  P->sup_list = (const uint32_t*)s->suplist.p;
  P->n_sup = (uint32_t)s->sup_host.size();
  return RT_OK;
}

static int prepare(rt_scene* s, const rt_params* p, uint32_t* argb_dev, const rt_aux* aux_dev, hipStream_t stream, RtDevParams* P) {
  TableUpload up{s, stream};
  s->notes = 0;
  copy_view(p, P);
  RC_TRY(prepare_aa_table(s, p, up, P));
  RC_TRY(prepare_cloud_table(s, p, up, P));
  if (P->light_mult > 1) RC_TRY(prepare_receiver_flags(s, p, up, P));
  copy_frame_shape(s, p, argb_dev, aux_dev, P);
  RC_TRY(take_frame_slot(s, p, stream, P));
  if (P->aa_rays > 256) return fail(RT_ERR_UNSUPPORTED, "aa_rays > 256");
  rt_morton_frame(s->aabb_lo, s->aabb_hi, P->morton_lo, P->morton_scale);
  RC_TRY(prepare_super_tiles(s, p, up, P));
  RC_TRY(up.finish());
  s->last_stream = stream;
  s->rendered = true;
  return RT_OK;
}

extern "C" {


// ---- frame scheduler -------------------------------------------------------------------------------
// Without secondary rays a frame is ONE launch of the primary kernel.  With reflections / refractions every child ray
// becomes an independent work item in HBM ("ray streaming"): the reference's recursion (single_raytrace,
// raytracer_renderer.rs:147-264: a node spawns calculate_reflection :526-729 and calculate_refractions :279-524) is run
// LEVEL BY LEVEL.  Level k reads one of two ray queues and appends its children to the other:
//     primary -> [hard pairs] -> for k = 1 .. depth:  trace(k) -> sort(k) -> shade(k) -> [hard pairs]  -> resolve
// Every launch takes its size from the device (the counter the launch before it wrote) and walks it with a grid-stride
// loop, so the host never waits for a level: a steady-state frame is enqueued without one synchronisation.  What the
// host contributes is a GUESS of each grid -- the counts of the previous frame of the same shape, read back
// asynchronously -- and the queue sizes.  Queues are sized by need: the first frame of a shape runs with a generous
// estimate and is verified (one synchronisation at its end: were children or pairs dropped?); if so the queues grow to
// what the counters say was needed and the frame is rendered again.  A verified shape renders asynchronously from then
// on (the scene is static, so its ray counts repeat exactly).  Pixel sums use a fixed-point accumulator (order
// independent, hence bit-reproducible), resolved to packed pixels by a last kernel.
// render_frame_impl runs these as stages: plan_schedule, take_workspace, match_stream_key, then per attempt size_queues,
// set_up_chains, enqueue_chains (enqueue_primary + enqueue_merged_levels / enqueue_chained_levels per batch) and finish_frame.
static const size_t RT_QUEUE_BUDGET = (size_t)160 << 30;  // hard ceiling; the real limit is half of the free HBM
// phase-split pipeline: bytes of a (wavefront, light) set record (header, 64-dword candidate list, slots in 3 class queues, class)
static const uint32_t RT_SET_RECORD_BYTES = 32u + 256u + 12u + 1u;

// Diagnostics: RT_TRACE_LAUNCHES=1 in the environment makes every launch of a frame wait for its kernel and report it on
// stderr (which launch of which level does not come back, with which sizes); never set in timed runs.
static void trace_point(hipStream_t stream, const char* what, uint32_t a, uint32_t b, uint32_t c) {
  static const char* const v = getenv("RT_TRACE_LAUNCHES");
  static const bool on = v && *v && *v != '0';
  if (!on) return;
  fprintf(stderr, "[rt_hip] %s (%u, %u, %u) launched ...", what, a, b, c);
  fflush(stderr);
  const hipError_t e = hipStreamSynchronize(stream);
  fprintf(stderr, " %s\n", e == hipSuccess ? "done" : hipGetErrorString(e));
  fflush(stderr);
}

// the result of a kernel launch on `stream`: "<what> failed: <HIP error>", or its RT_TRACE_LAUNCHES point (when it has a label)
static int launched(int err, hipStream_t stream, const char* what, const char* label = nullptr, uint32_t a = 0, uint32_t b = 0, uint32_t c = 0) {
  if ((hipError_t)err != hipSuccess) return fail(RT_ERR_HIP, "%s failed: %s", what, hipGetErrorString((hipError_t)err));
  if (label) trace_point(stream, label, a, b, c);
  return RT_OK;
}

static uint32_t grid_for(uint64_t items, uint32_t per_wg, uint32_t cap_wgs) {
  uint64_t w = (items + items / 16u + per_wg - 1u) / per_wg + 8u;  // a little above the guess; the loop covers the rest
  if (w > cap_wgs) w = cap_wgs;
  return w ? (uint32_t)w : 1u;
}
static uint32_t cap32(uint64_t n) { return (uint32_t)std::min<uint64_t>(n, 0xFFFFFF00ull); }  // (16-byte aligned arrays behind a queue)

// how the levels of a ray tree are run (rt_tuning.levels)
// (measured, round 4: MERGED config 4 40.6 ms alone / 39.3 with two frames in flight against 49.8 / 42.6 CHAINED, config 5 120.4 / 118.4
// against 126.4 / 122.3; PIPELINED 47.7 / 42.9 and 129.4 / 123.3: one hit-point order over all levels is worth more than the overlap)
static uint32_t rt_levels_mode(uint32_t wanted) { return wanted == RT_LEVELS_DEFAULT ? RT_LEVELS_MERGED : wanted; }

// which form of the render loop a frame takes (rt_tuning.phases; RT_PHASES_DEFAULT: by frame shape; the calibration frame of
// RT_TILE_ORDER_COST times the fused primary kernel)
static bool rt_use_phases(uint32_t wanted, const RtDevParams& P) { return !P.cost_map && wanted == RT_PHASES_SPLIT; }

// What the stages of one accumulated frame share.  Side chains and shade streams with work in flight drain when it goes out of scope,
// on every error path: their work refers to the workspace set, and only the caller's stream is guarded by the frame event.
struct Frame {
  rt_scene* s;
  RtDevParams& P;
  hipStream_t stream;
  uint32_t forced;  // rt_tuning.chunk_log2: batch size under test (0: sized by need)
  bool blocking;
  // A ray batch (rt_trace_rays*): a frame of n x 1 "pixels" whose camera rays are the caller's (rt_rays.h).  Its ray counts say
  // nothing about the next batch, so it is always verified (blocking) and never marks its shape verified; it runs the chained
  // schedule with fused phases -- the merged-level and phase kernels re-derive the camera ray from the work-item index.
  const RtRayArgs* rays;
  // ---- plan (hard: soft-shadow sets of incoherent wavefronts deferred to rt_hard_kernel; merged: one append-only queue per chain)
  bool secondary, split, defer, hard = false, merged = false, pipelined = false;
  uint32_t total_wgs, levels = 0, levels_mode = RT_LEVELS_CHAINED, lanes = 1, n_cnt = 0;
  uint64_t items = 0;  // primary work items (threads) of the frame
  rt_scene::StreamWs* w = nullptr;
  // ---- sizes of the current attempt; guess: grids from the previous frame's counts (else: whole capacity)
  uint32_t n_buckets = 0, q_sort_cap = 0, set_cap = 0, n_batches = 0, cap_wgs = 0, pairs_per_wg = 0, hard_cap_wgs = 0;
  size_t hitrec_items = 0;
  bool guess = false;
  // ---- the chains: the caller's parameters with the chain's own queues and counters; what is in flight on their streams
  RtDevParams Pl[RT_LANES];
  float4* q[RT_LANES][2];
  uint32_t* counts[RT_LANES];
  bool forked = false, joined = false, shading = false;
  Frame(rt_scene* s_, RtDevParams& P_, hipStream_t stream_, uint32_t forced_, bool blocking_, const RtRayArgs* rays_)
      : s(s_), P(P_), stream(stream_), forced(forced_), blocking(blocking_ || rays_), rays(rays_),
        secondary((P.flags & (RT_FLAG_REFLECTIONS | RT_FLAG_REFRACTIONS)) != 0) {
    total_wgs = rays ? (rays->n + 255u) / 256u : rt_primary_total_wgs(P);
    // The phase-split pipeline (rt_phases.h; rt_tuning.phases): hit -> classify -> one kernel per class of (wavefront, light)
    // set -> resolve, instead of the fused kernels.  Frames without secondary rays then also sum through the accumulator.
    split = rt_use_phases(s->phases_wanted, P);
    // RT_PHASES_FUSED_DEFER: the fused kernels, but a frame without secondary rays also sums through the accumulator, so that its
    // incoherent (wavefront, light) sets can be deferred to rt_hard_kernel like those of a frame with secondary rays
    defer = !secondary && !split && !P.cost_map && s->phases_wanted == RT_PHASES_FUSED_DEFER && P.light_mult > 1;
    if (rays) split = defer = false;
  }
  ~Frame() {
    for (uint32_t j = 1; j < lanes && forked && !joined; j++) (void)hipStreamSynchronize(w->lane[j].stream);
    for (uint32_t j = 0; j < lanes && shading; j++)
      for (hipStream_t ss : w->lane[j].shade_stream)
        if (ss) (void)hipStreamSynchronize(ss);
  }
  // a grid over the rays (or hits) of counter `idx` of chain j in the last frame of this shape
  uint32_t ray_grid(uint32_t j, uint32_t idx) const { return guess ? grid_for(s->est[j][idx], 256u, cap_wgs) : cap_wgs; }
};

// ---- plan: depth, pair deferral, level schedule, chains
static int plan_schedule(Frame& f) {
  rt_scene* s = f.s;
  const RtDevParams& P = f.P;
  f.levels = !f.secondary ? 0u : std::max(P.max_depth_reflection, P.max_depth_refraction);
  if (f.secondary && f.levels == 0) return fail(RT_ERR_INVALID_ARG, "secondary rays enabled with depth 0");
  f.items = (uint64_t)f.total_wgs * 256u;
  f.hard = (f.secondary || f.split || f.defer) && P.light_mult > 1 && P.light_mult <= 64 && P.traversal == RT_TRAVERSAL_BVH &&
           s->dev.n_triangles && P.cand_cap != 0;
  if (!f.hard && P.light_mult > 1) s->notes |= RT_NOTE_HARD_PAIRS_OFF;
  // merged levels (rt_tuning.levels): every level traced first (the trace kernel appends the children), then ONE sort and ONE shade launch
  f.levels_mode = (f.secondary && !f.split && !f.rays) ? rt_levels_mode(s->levels_wanted) : RT_LEVELS_CHAINED;
  if (f.levels_mode == RT_LEVELS_MERGED && s->levels_wanted == RT_LEVELS_DEFAULT) {
    // The merged queue holds every level of the tree at once (config 4: 5.0 GB against the 2.9 GB of two alternating queues).  Where a
    // third of the free memory (plus what this scene's workspaces already hold) does not take about four times the primary work items,
    // the library's choice is the chained schedule rather than a frame cut into batches.
    size_t free_b = 0, total_b = 0, held = 0;
    for (const auto& o : s->ws) held += o.bytes();
    const uint64_t want = (uint64_t)f.total_wgs * 256u * 4u * (64u + 12u);
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || want > (free_b + held) / 3u) f.levels_mode = RT_LEVELS_CHAINED;
  }
  f.pipelined = f.levels_mode == RT_LEVELS_PIPELINED, f.merged = f.levels_mode == RT_LEVELS_MERGED || f.pipelined;
  f.n_cnt = RT_CNT_TOTAL(f.levels);
  // ---- chains.  The ray tree of a frame is a chain of launches, one per level, each with a drain of its own (a launch
  // cannot end before its longest wavefront does).  A frame that has the GPU to itself is therefore split into two
  // interleaved halves of its primary work-group list that run as independent chains -- own queues, own counters, own
  // stream -- and meet in the pixel accumulator: the head of one chain's launch fills the drain of the other's
  // (rt_tuning.sub_frames; a frame alone: config 4 51.8 -> 49.5 ms, at depth 21 102.7 -> 92.2).  When the host keeps
  // frames in flight itself the other FRAME is the better filler (42.3 ms against 43.3 with chains on top): sub_frames = 0
  // uses two chains only while no other frame of the scene is running (and stays with one for 8 frames after the last
  // overlap, so that a pipeline that drains now and then does not flip -- every flip re-verifies the queue sizes).
  f.lanes = s->lanes_wanted ? std::min<uint32_t>(s->lanes_wanted, RT_LANES) : RT_LANES;
  if (!s->lanes_wanted) {
    bool busy = false;
    for (int b = 0; b < RT_SLOTS; b++)
      if (b != s->cur_block && s->frame_pending[b] && hipEventQuery(s->frame_ev[b]) == hipErrorNotReady) busy = true;
    s->calm_frames = busy ? 0u : std::min<uint32_t>(s->calm_frames + 1u, 1u << 30);
    if (s->calm_frames < 8u) f.lanes = 1;
  }
  // (forced batch sizes: the batching itself is under test; tiny frames: nothing to overlap)
  if (f.forced || f.items < (1ull << 16) || (!f.secondary && !s->lanes_wanted)) f.lanes = 1;
  if (f.merged && !s->lanes_wanted) f.lanes = 1;  // (measured: two chains add nothing once the levels share one shade launch)
  return RT_OK;
}

// ---- workspace: this frame's set -- the one of its slot, unless that would mean ALLOCATING a second set on a device that cannot
// spare the memory (a partitioned or shared GPU): then the frame waits for the frame that uses set 0 and takes it.
static int take_workspace(Frame& f) {
  rt_scene* s = f.s;
  int wsi = s->cur_block;
  if (wsi > 0 && !s->ws[wsi].lane[0].queues.p && s->ws[0].lane[0].queues.p) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < 3 * s->ws[0].bytes()) wsi = 0;
  }
  if (s->ws_last_block[wsi] != s->cur_block && s->frame_pending[s->ws_last_block[wsi]])
    HIP_TRY(hipStreamWaitEvent(f.stream, s->frame_ev[s->ws_last_block[wsi]], 0));
  s->ws_last_block[wsi] = s->cur_block;
  s->cur_ws = wsi;
  rt_scene::StreamWs& w = *(f.w = &s->ws[wsi]);
  for (uint32_t j = 0; j < f.lanes; j++) {
    RC_TRY(w.lane[j].qcount.ensure((size_t)f.n_cnt * 4));
    if (j && !w.lane[j].stream) HIP_TRY(hipStreamCreateWithFlags(&w.lane[j].stream, hipStreamNonBlocking));
    if (j && !w.lane[j].done_ev) HIP_TRY(hipEventCreateWithFlags(&w.lane[j].done_ev, hipEventDisableTiming));
  }
  for (rt_scene::Lane* L = w.lane + f.lanes; L < w.lane + RT_LANES; L++)  // memory by need: a set that runs one chain does not keep the other chain's queues
    if (L->queues.p || L->trace_ws.p || L->hard.p || L->hitrec.p || L->sets.p) {
      if (L->stream) HIP_TRY(hipStreamSynchronize(L->stream));
      HIP_TRY(hipStreamSynchronize(f.stream));  // (behind the wait for the set's last frame enqueued above)
      L->queues.release(), L->trace_ws.release(), L->hard.release(), L->hitrec.release(), L->sets.release();
      L->sort_hist_clean = nullptr;
    }
  if (!w.cnt_host) HIP_TRY(hipHostMalloc((void**)&w.cnt_host, RT_LANES * RT_CNT_STRIDE * 4, hipHostMallocDefault));
  if (!w.cnt_ev) HIP_TRY(hipEventCreateWithFlags(&w.cnt_ev, hipEventDisableTiming));
  if (!w.fork_ev) HIP_TRY(hipEventCreateWithFlags(&w.fork_ev, hipEventDisableTiming));
  return RT_OK;
}

// ---- the shape of this frame: what its ray counts depend on.  Same key as the last verified frame = same counts.  Then the counts
// of earlier frames of this shape whose read-back has landed.
static void match_stream_key(Frame& f) {
  rt_scene* s = f.s;
  const RtDevParams& P = f.P;
  StreamKey key;
  memset(&key, 0, sizeof(key));
  key.width = P.width, key.height = P.height, key.flags = P.flags, key.aa_rays = P.aa_rays, key.aa_unique = P.aa_unique;
  key.light_mult = P.light_mult, key.depth_refl = P.max_depth_reflection, key.depth_refr = P.max_depth_refraction;
  key.win[0] = P.win_x0, key.win[1] = P.win_y0, key.win[2] = P.win_w, key.win[3] = P.win_h;
  key.tile_size = P.tile_size, key.n_ranks = P.n_ranks, key.rank = P.rank, key.traversal = P.traversal, key.cand_cap = P.cand_cap;
  key.cloud_seed = P.cloud_seed, key.n_cloud_sets = P.n_cloud_sets, key.forced = f.forced, key.tables = s->tables_version;
  memcpy(key.f, P.focus, 12), key.f[3] = P.fw, key.f[4] = P.fh, key.f[5] = P.fd, key.f[6] = P.eps_distance, key.f[7] = P.air_ior;
  key.staged = P.stage_slot != nullptr, key.flags_on = P.recv_flags != nullptr, key.n_sup = P.n_sup, key.lanes = f.lanes, key.merged = f.levels_mode;
  key.split = (f.split ? 1u : 0u) | (f.defer ? 2u : 0u), key.sort_bits = s->sort_bits_wanted, key.lists_on = P.cell_lists != nullptr;
  key.rays = f.rays ? 1u : 0u;  // (a camera frame behind a ray batch is a new shape: it does not trust sizes the batch left)
  if (memcmp(&key, &s->stream_key, sizeof(key)) != 0) {
    s->stream_key = key, s->key_gen++, s->stream_verified = false, s->est_valid = false;
    s->q_cap = s->hard_cap = s->batch_items = 0;
  }
  for (auto& o : s->ws)
    if (o.cnt_pending && hipEventQuery(o.cnt_ev) == hipSuccess) {
      o.cnt_pending = false;
      if (o.cnt_key_gen != s->key_gen) continue;  // (the counts of another frame shape say nothing about this one)
      // A verified shape renders without waiting for its counters -- but how many pairs a frame defers depends on how its rays
      // were packed into wavefronts (atomic order in the sort), so a later frame can need a little more than the verified one
      // did.  If a frame dropped anything, say so (rt_stats.notes) and verify -- i.e. size and, if needed, render again -- the next.
      bool dropped_any = false;
      for (uint32_t j = 0; j < o.cnt_host_lanes; j++) {
        const uint32_t* c = o.cnt_host + (size_t)j * RT_CNT_STRIDE;
        if (c[RT_CNT_OVERFLOW] || c[RT_CNT_HARD_STAT(o.cnt_host_levels)]) {
          dropped_any = true;
          s->hard_cap = std::max<uint32_t>(s->hard_cap, cap32((uint64_t)c[RT_CNT_HARD_STAT(o.cnt_host_levels) + 1u] * 5u / 4u + 256u));
        }
      }
      if (dropped_any) {
        s->stream_verified = false, s->est_valid = false, s->sticky_notes |= RT_NOTE_FRAME_DROPPED_WORK;
        continue;
      }
      if (o.cnt_host_levels == f.levels && o.cnt_host_lanes == f.lanes && o.cnt_host_valid) memcpy(s->est, o.cnt_host, sizeof(s->est)), s->est_valid = true;
    }
}

// smaller primary batches, queues and pair buffer in proportion (rays per queue no fewer than q_floor)
static void shrink_sizes(rt_scene* s, bool hard, uint32_t q_floor) {
  s->q_cap = std::max<uint32_t>(s->q_cap / 2u, q_floor);
  s->hard_cap = hard ? std::max<uint32_t>(s->hard_cap / 2u, 1u << 16) : 0u;
  s->batch_items = std::max<uint32_t>(s->batch_items / 2u, 1u << 10);
}

// ---- sizes, per chain, and the workspaces that hold them.  Unknown shape: every level fits the chain's primary work items
// (children usually thin out; a scene where they multiply is caught by the verification), pairs = 1/8 of that.  Budget: half
// of the free HBM.  `oom`: an allocation failed, the sizes were halved -- try again.
static int size_queues(Frame& f, int attempt, bool& oom) {
  rt_scene* s = f.s;
  rt_scene::StreamWs& w = *f.w;
  if (!s->q_cap) {
    if (f.forced) {
      s->batch_items = 1u << f.forced;
      s->q_cap = 2u * s->batch_items;
    } else {
      const uint64_t lane_items = ((uint64_t)f.total_wgs + f.lanes - 1u) / f.lanes * 256u;
      s->batch_items = (uint32_t)std::min<uint64_t>(lane_items, 1ull << 28);
      // (merged levels: ONE queue of 2 q_cap rays holds every level of the tree -- three times the primary work items as a first guess)
      s->q_cap = f.merged ? (uint32_t)std::min<uint64_t>((uint64_t)s->batch_items * 3u / 2u, 0x7FFFFF00ull) : s->batch_items;
    }
    if (s->q_cap < (1u << 16)) s->q_cap = 1u << 16;
    s->hard_cap = f.hard ? std::max<uint32_t>(s->q_cap / 8u, 1u << 16) : 0u;
  }
  size_t budget = RT_QUEUE_BUDGET, free_b = 0, total_b = 0;
  const size_t held = w.bytes() - w.acc.cap;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = std::min(budget, (size_t)((double)(free_b + held) * 0.5));
  // (phase-split pipeline: 8 bytes of hit record per primary work item of a batch + the (wavefront, light) set records, dense by set id)
  const uint32_t levels = f.levels;
  auto set_cap_for = [&](uint64_t q, uint64_t batch) { return (uint32_t)(((std::max<uint64_t>(levels ? q : 0u, batch + 64u * 256u) / 64u + 4u) * std::max<uint32_t>(s->dev.n_lights, 1u) + 15u) & ~7ull); };
  auto bytes_for = [&](uint64_t q, uint64_t h) {
    size_t b = levels ? (size_t)(q * (2u * 64u + (f.merged ? 24u : 12u)) + (h ? (h + 64u) * 64u : 0u)) : 0u;
    if (f.split) b += (size_t)(s->batch_items + 64u * 256u) * 8u + (size_t)set_cap_for(q, s->batch_items) * RT_SET_RECORD_BYTES;
    return (size_t)f.lanes * b;
  };
  while (bytes_for(s->q_cap, s->hard_cap) > budget && s->q_cap > (1u << 16))  // does not fit
    shrink_sizes(s, f.hard, 1u << 16), s->stream_verified = false;
  s->batch_items = std::max<uint32_t>((s->batch_items + 255u) / 256u * 256u, 256u);
  s->q_cap = cap32(((uint64_t)s->q_cap + 255u) / 256u * 256u);
  // (more rays per level = more rays per bucket: two more key bits for 4K-sized frames: config 5 136.2 -> 133.4 ms)
  // (merged levels sort the rays of every level at once, three times a level's: config 4 20 / 22 / 23 / 24 bits = 41.3 / 39.9 / 39.3 / 38.9 ms)
  f.P.sort_bits = s->sort_bits_wanted ? s->sort_bits_wanted : ((f.merged || f.items >= (32ull << 20)) ? RT_SORT_BITS_DEFAULT + 2u : RT_SORT_BITS_DEFAULT);
  f.n_buckets = 1u << f.P.sort_bits;
  // (merged levels: the two queues of q_cap rays are ONE queue of 2 q_cap -- same memory -- and the sort workspace covers all of it)
  f.q_sort_cap = f.merged ? 2u * s->q_cap : s->q_cap;
  f.set_cap = f.split ? set_cap_for(s->q_cap, s->batch_items) : 0u;
  f.hitrec_items = (size_t)s->batch_items + 64u * 256u;  // (an interleaved chain's launch is rounded up to whole groups)
  int rc = RT_OK;
  for (uint32_t j = 0; j < f.lanes && rc == RT_OK; j++) {
    rt_scene::Lane& L = w.lane[j];
    if (levels) {
      rc = L.queues.ensure((size_t)2 * s->q_cap * RT_QUEUE_QUADS * sizeof(float4));
      if (rc == RT_OK) rc = L.trace_ws.ensure((size_t)f.q_sort_cap * 12 + (size_t)f.n_buckets * 8 + (f.n_buckets / RT_SORT_TILE) * 4 + 256);
    }
    if (rc == RT_OK && f.hard) rc = L.hard.ensure(((size_t)s->hard_cap + 64u) * 4u * sizeof(float4));
    if (rc == RT_OK && (f.split || f.merged)) rc = L.hitrec.ensure(f.hitrec_items * 8u);
    if (rc == RT_OK && f.split) rc = L.sets.ensure((size_t)f.set_cap * RT_SET_RECORD_BYTES + 256u);
  }
  if (rc == RT_ERR_OOM && s->q_cap > (1u << 16) && attempt < 12) {
    shrink_sizes(s, f.hard, 0u), oom = true;
    return RT_OK;
  }
  if (rc != RT_OK) return rc;
  const size_t npix = (size_t)f.P.width * f.P.height;
  if (w.acc_pixels != npix) {
    RC_TRY(w.acc.ensure(npix * 4 * sizeof(long long)));
    HIP_TRY(hipMemsetAsync(w.acc.p, 0, npix * 4 * sizeof(long long), f.stream));
    w.acc_pixels = npix;
  }
  f.n_batches = (uint32_t)((f.items + s->batch_items - 1) / s->batch_items);
  if (f.n_batches > f.lanes) s->notes |= RT_NOTE_FRAME_BATCHED;
  f.cap_wgs = (f.q_sort_cap + 255u) / 256u;
  f.guess = s->est_valid && f.n_batches == f.lanes && !f.rays;  // (another batch, other counts: whole-capacity grids)
  const uint32_t ppw = 64u / (f.P.light_mult < 2u ? 2u : f.P.light_mult);
  f.pairs_per_wg = 4u * (ppw ? ppw : 1u), f.hard_cap_wgs = f.hard ? (s->hard_cap + f.pairs_per_wg - 1u) / f.pairs_per_wg : 1u;
  return RT_OK;
}

// ---- every chain's view of the frame, its histogram zeroed once and its counters zeroed for this attempt
static int set_up_chains(Frame& f) {
  rt_scene* s = f.s;
  rt_scene::StreamWs& w = *f.w;
  for (uint32_t j = 0; j < f.lanes; j++) {
    rt_scene::Lane& L = w.lane[j];
    RtDevParams& Q = f.Pl[j] = f.P;
    uint32_t* ws = (uint32_t*)L.trace_ws.p;
    Q.sort_slot = (uint2*)ws;  // (8-byte aligned: first)
    Q.sh_idx = ws + (size_t)2 * f.q_sort_cap;
    Q.sort_hist = Q.sh_idx + f.q_sort_cap;
    Q.sort_offs = Q.sort_hist + f.n_buckets, Q.sort_tile = Q.sort_offs + f.n_buckets;
    if (f.split) {
      const uint32_t set_cap = f.set_cap;
      Q.hitrec = (uint2*)L.hitrec.p;
      Q.set_hdr = (uint4*)L.sets.p;                                        // [set_cap][2] uint4
      Q.set_list = (uint32_t*)L.sets.p + (size_t)set_cap * 8u;             // [set_cap][64]
      Q.set_q = (uint32_t*)L.sets.p + (size_t)set_cap * (8u + 64u);        // [3][set_cap]
      Q.set_cls = (uint8_t*)((uint32_t*)L.sets.p + (size_t)set_cap * (8u + 64u + 3u));  // [set_cap] bytes
      Q.set_cap = set_cap, Q.set_lights = s->dev.n_lights;
    }
    if (f.levels && (L.sort_hist_clean != (void*)Q.sort_hist || L.sort_hist_buckets != f.n_buckets)) {
      // a fresh (moved, resized) histogram: zero it once; every use leaves it zero
      HIP_TRY(hipMemsetAsync(Q.sort_hist, 0, (size_t)f.n_buckets * 4, f.stream));
      L.sort_hist_clean = (void*)Q.sort_hist, L.sort_hist_buckets = f.n_buckets;
    }
    uint32_t* cnt = f.counts[j] = (uint32_t*)L.qcount.p;
    HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)f.n_cnt * 4, f.stream));
    Q.acc = (long long*)w.acc.p, Q.q_capacity = s->q_cap, Q.q_overflow = cnt + RT_CNT_OVERFLOW;
    Q.hard_q = f.hard ? (float4*)L.hard.p : nullptr, Q.hard_capacity = s->hard_cap;
    Q.hard_count = cnt + RT_CNT_HARD(f.levels), Q.hard_stat = cnt + RT_CNT_HARD_STAT(f.levels);
    f.q[j][0] = (float4*)L.queues.p, f.q[j][1] = (float4*)L.queues.p + (size_t)s->q_cap * RT_QUEUE_QUADS;
  }
  s->queue_bytes = 0;
  for (auto& o : s->ws) s->queue_bytes += o.bytes();
  return RT_OK;
}

// the pairs chain j deferred so far, traced by rt_hard_kernel
static int run_hard(Frame& f, uint32_t j, hipStream_t st) {
  if (!f.hard) return RT_OK;
  RtDevParams& Q = f.Pl[j];
  const uint32_t g = f.guess ? grid_for(f.s->est[j][RT_CNT_HARD_STAT(f.levels) + 1u], f.pairs_per_wg, f.hard_cap_wgs) : std::min(f.hard_cap_wgs, 16384u);
  RC_TRY(launched(rt_launch_hard(f.s->dev, Q, g, st), st, "hard-pair launch", "rt_hard_kernel: workgroups, pair capacity, chain", g, f.s->hard_cap, j));
  HIP_TRY(hipMemsetAsync(Q.hard_count, 0, 4, st));  // (stream ordered: behind the kernel that read it)
  return RT_OK;
}

// the (wavefront, light) sets K2 queued for level k of chain j, one launch per class (grids: last frame's counts of this shape)
static int run_sets(Frame& f, uint32_t j, hipStream_t st, uint32_t k, uint32_t n_sets_host) {
  rt_scene* s = f.s;
  RtDevParams& Q = f.Pl[j];
  // class bytes -> class queues (level 0: the launch's set ids are known here; deeper levels: from the device-side hit count)
  const uint32_t n_sets_guess = k == 0 ? n_sets_host : (f.guess ? (s->est[j][RT_CNT_HITS(f.levels, k)] / 64u + 2u) * s->dev.n_lights : f.set_cap);
  Q.set_n = k == 0 ? n_sets_host : 0u;
  RC_TRY(launched(rt_launch_compact(Q, std::min<uint32_t>((n_sets_guess + 2047u) / 2048u + 1u, (f.set_cap + 2047u) / 2048u), st), st, "compaction launch"));
  const uint32_t cap_sets = (f.set_cap + 3u) / 4u;
  for (int c = 0; c < 3; c++) {
    if (c == 0 && rt_phases_arrive_inline()) continue;  // (ARRIVE sets are finished by K2 itself in this build)
    const uint32_t g = f.guess ? grid_for(s->est[j][RT_CNT_SETS(f.levels, k, c)], 4u, cap_sets) : cap_sets;
    RC_TRY(launched(rt_launch_sets(s->dev, Q, k == 0, c, g, st), st, "set-kernel launch", "rt_sets kernel: level, class, workgroups", k, (uint32_t)c, g));
  }
  return RT_OK;
}

// ---- the primary launches of one batch of chain j (workgroups w0 .. w0 + nw of the list; `next`: not the chain's first batch)
static int enqueue_primary(Frame& f, uint32_t j, hipStream_t st, uint32_t w0, uint32_t nw, bool next) {
  rt_scene* s = f.s;
  RtDevParams& Q = f.Pl[j];
  if ((f.split || f.merged) && (size_t)nw * 256u > f.hitrec_items)
    return fail(RT_ERR_HIP, "internal: primary batch of %u workgroups exceeds the hit-record buffer", nw);
  if (f.split) {
    if (next) HIP_TRY(hipMemsetAsync(f.counts[j] + RT_CNT_SETS(f.levels, 0, 0), 0, (size_t)3 * (f.levels + 1) * 4, st));  // its set counters
    Q.set_count = f.counts[j] + RT_CNT_SETS(f.levels, 0, 0), Q.set_items = nw * 256u;
    RC_TRY(launched(rt_launch_hit(s->dev, Q, nw, st), st, "kernel launch", "rt_hit_kernel: first workgroup, workgroups", w0, nw));
    RC_TRY(launched(rt_launch_classify(s->dev, Q, true, nw, st), st, "kernel launch", "rt_classify0_kernel: first workgroup, workgroups, set capacity", w0, nw, f.set_cap));
    return run_sets(f, j, st, 0, nw * 4u * s->dev.n_lights);
  }
  if (f.rays)
    return launched(rt_launch_rays(s->dev, Q, *f.rays, nw, st), st, "kernel launch", "rt_rays_stream_kernel: first workgroup, workgroups, queue capacity", w0, nw, s->q_cap);
  if (!f.merged)
    return launched(rt_launch_primary(s->dev, Q, nw, st), st, "kernel launch", "rt_primary_stream_kernel: first workgroup, workgroups, queue capacity", w0, nw, s->q_cap);
  // The camera rays' hits and children first (rt_hit_spawn_kernel: 44 VGPRs, no scratch), so that the levels below can be traced
  // at once -- latency-bound launches -- while the hits are SHADED on a stream of the chain's (rt_primary_pre_kernel: issue bound).
  rt_scene::Lane& L = f.w->lane[j];
  for (int k = 0; k < (f.pipelined ? 2 : 1); k++) {  // (pipelined levels are shaded on two streams alternately)
    if (!L.shade_stream[k]) HIP_TRY(hipStreamCreateWithFlags(&L.shade_stream[k], hipStreamNonBlocking));
    if (!L.shade_done[k]) HIP_TRY(hipEventCreateWithFlags(&L.shade_done[k], hipEventDisableTiming));
  }
  if (!L.hit_ev) HIP_TRY(hipEventCreateWithFlags(&L.hit_ev, hipEventDisableTiming));
  Q.hitrec = (uint2*)L.hitrec.p, Q.hit_spawns = 1u;
  RC_TRY(launched(rt_launch_hit(s->dev, Q, nw, st), st, "kernel launch", "rt_hit_spawn_kernel: first workgroup, workgroups, queue capacity", w0, nw, f.q_sort_cap));
  HIP_TRY(hipEventRecord(L.hit_ev, st));
  HIP_TRY(hipStreamWaitEvent(L.shade_stream[0], L.hit_ev, 0));
  f.shading = true;
  RtDevParams Pp = Q;
  Pp.q_out = nullptr, Pp.q_out_count = nullptr, Pp.hit_spawns = 0u;
  RC_TRY(launched(rt_launch_primary(s->dev, Pp, nw, L.shade_stream[0]), L.shade_stream[0], "kernel launch", "rt_primary_pre_kernel: first workgroup, workgroups", w0, nw));
  Q.hit_spawns = 0u;
  return RT_OK;
}

// ---- merged / pipelined levels of chain j: every level traced first -- rt_trace_spawn_kernel finds the hits of the slice
// [seg[k], seg[k + 1]) of the chain's ONE queue and appends their children behind it; the slice's end is a stream-ordered snapshot
// of the queue's running total.  (No rt_hard_kernel in between: the camera rays are being shaded on the chain's shade stream
// meanwhile and defer pairs of their own; every deferred pair of the frame waits in the pair queue for the one launch behind the join.)
static int enqueue_merged_levels(Frame& f, uint32_t j, hipStream_t st, bool next) {
  rt_scene* s = f.s;
  rt_scene::Lane& L = f.w->lane[j];
  RtDevParams& Q = f.Pl[j];
  const uint32_t levels = f.levels;
  uint32_t *const cnt = f.counts[j], *const total = cnt + RT_CNT_LEVEL(1);
  if (next) HIP_TRY(hipMemsetAsync(cnt + RT_CNT_SEG(levels, 0), 0, (size_t)(levels + 2u) * 4, st));
  while (f.pipelined && L.level_ev.size() < levels) {
    hipEvent_t ev = nullptr;
    HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    L.level_ev.push_back(ev);
  }
  Q.q_in = f.q[j][0], Q.q_in_count = total;
  for (uint32_t k = 1; k <= levels; k++) {
    HIP_TRY(hipMemcpyAsync(cnt + RT_CNT_SEG(levels, k + 1u), total, 4, hipMemcpyDeviceToDevice, st));
    Q.seg_lo = cnt + RT_CNT_SEG(levels, k), Q.seg_hi = cnt + RT_CNT_SEG(levels, k + 1u);
    Q.q_out = f.q[j][0], Q.q_out_count = total;
    const uint32_t n_k = f.guess ? s->est[j][RT_CNT_SEG(levels, k + 1u)] - s->est[j][RT_CNT_SEG(levels, k)] : 0u;
    const uint32_t g_rays = f.guess ? grid_for(n_k, 256u, f.cap_wgs) : f.cap_wgs;
    RC_TRY(launched(rt_launch_trace(s->dev, Q, g_rays, st), st, "trace launch", "rt_trace_spawn_kernel: level, workgroups, chain", k, g_rays, j));
    if (!f.pipelined) continue;
    // the level's own hit-point order (its slice of sh_idx), then its shading on one of the chain's two shade streams: the
    // next levels are traced meanwhile, and the head of level k + 1's shading fills the drain of level k's
    Q.sort_hits = cnt + RT_CNT_HITS(levels, k);
    RC_TRY(launched(rt_launch_sort(Q, g_rays, st), st, "sort launch"));
    HIP_TRY(hipEventRecord(L.level_ev[k - 1u], st));
    hipStream_t ss = L.shade_stream[k & 1u];
    HIP_TRY(hipStreamWaitEvent(ss, L.level_ev[k - 1u], 0));
    f.shading = true;
    RtDevParams S = Q;
    S.q_out = nullptr, S.q_out_count = nullptr;  // (the children exist already)
    const uint32_t g_hits = f.ray_grid(j, RT_CNT_HITS(levels, k));
    RC_TRY(launched(rt_launch_shade(s->dev, S, g_hits, ss), ss, "shade launch", "rt_shade_kernel: level, workgroups, chain (pipelined)", k, g_hits, j));
  }
  Q.seg_lo = Q.seg_hi = nullptr, Q.q_out = nullptr, Q.q_out_count = nullptr;
  if (!f.pipelined) {
    // ---- MERGED: one hit-point order over the rays of all levels, one shade launch (no children: they exist already)
    Q.hitrec = nullptr;
    Q.sort_hits = cnt + RT_CNT_HITS(levels, 1);
    const uint32_t g_all = f.ray_grid(j, RT_CNT_LEVEL(1)), g_hits = f.ray_grid(j, RT_CNT_HITS(levels, 1));
    RC_TRY(launched(rt_launch_sort(Q, g_all, st), st, "sort launch"));
    RC_TRY(launched(rt_launch_shade(s->dev, Q, g_hits, st), st, "shade launch", "rt_shade_kernel (all levels): workgroups, chain", g_hits, j));
  }
  // join: the camera rays' shading (pipelined: and every level's) -- the pairs it deferred, and the resolve, need all of it
  for (int k = 0; k < (f.pipelined ? 2 : 1); k++) {
    HIP_TRY(hipEventRecord(L.shade_done[k], L.shade_stream[k]));
    HIP_TRY(hipStreamWaitEvent(st, L.shade_done[k], 0));
  }
  f.shading = false;  // (joined on the device: the chain's stream now orders everything behind the shade launches)
  return RT_OK;
}

// ---- chained levels of chain j: trace -> sort -> shade (or classify -> sets) per level, the pairs deferred before each level first
static int enqueue_chained_levels(Frame& f, uint32_t j, hipStream_t st) {
  rt_scene* s = f.s;
  RtDevParams& Q = f.Pl[j];
  const uint32_t levels = f.levels;
  uint32_t* const cnt = f.counts[j];
  for (uint32_t k = 1; k <= levels; k++) {
    RC_TRY(run_hard(f, j, st));  // the pairs the launch before deferred
    Q.q_in = f.q[j][(k - 1u) & 1u], Q.q_in_count = cnt + RT_CNT_LEVEL(k), Q.sort_hits = cnt + RT_CNT_HITS(levels, k);
    Q.q_out = k < levels ? f.q[j][k & 1u] : nullptr;  // (rays of the last level have depth 1: no children possible)
    Q.q_out_count = k < levels ? cnt + RT_CNT_LEVEL(k + 1u) : nullptr;
    const uint32_t g_rays = f.ray_grid(j, RT_CNT_LEVEL(k)), g_hits = f.ray_grid(j, RT_CNT_HITS(levels, k));
    RC_TRY(launched(rt_launch_trace(s->dev, Q, g_rays, st), st, "trace launch", "rt_trace_kernel: level, workgroups, chain", k, g_rays, j));
    RC_TRY(launched(rt_launch_sort(Q, g_rays, st), st, "sort launch", "sort kernels: level, buckets, chain", k, f.n_buckets, j));
    if (f.split) {
      Q.set_count = cnt + RT_CNT_SETS(levels, k, 0);
      RC_TRY(launched(rt_launch_classify(s->dev, Q, false, g_hits, st), st, "classify launch", "rt_classify_kernel: level, workgroups, chain", k, g_hits, j));
      RC_TRY(run_sets(f, j, st, k, 0u));
    } else {
      RC_TRY(launched(rt_launch_shade(s->dev, Q, g_hits, st), st, "shade launch", "rt_shade_kernel: level, workgroups, chain", k, g_hits, j));
    }
  }
  return RT_OK;
}

// ---- the batches of every chain.  One batch per chain (the rule): the chains INTERLEAVE, groups of 64 workgroups of the list
// alternately, so that each gets its share of the expensive regions (contiguous halves = sky and text: the sky's chain is done at
// once and the text's runs alone).  Frames batched for memory: contiguous batches, dealt to the chains in turn.
static int enqueue_chains(Frame& f) {
  rt_scene* s = f.s;
  rt_scene::StreamWs& w = *f.w;
  if (f.lanes > 1) {  // fork: the other chains start behind everything enqueued on the caller's stream so far
    HIP_TRY(hipEventRecord(w.fork_ev, f.stream));
    for (uint32_t j = 1; j < f.lanes; j++) HIP_TRY(hipStreamWaitEvent(w.lane[j].stream, w.fork_ev, 0));
    f.forked = true, f.joined = false;
  }
  const uint32_t batch_wgs = s->batch_items / 256u, group_log2 = 6u, n_groups = (f.total_wgs + 63u) >> 6;
  const bool interleave = f.lanes > 1 && f.n_batches == f.lanes;
  uint32_t lane_batches[RT_LANES] = {0};
  for (uint32_t b = 0, w0 = 0; interleave ? b < f.lanes : w0 < f.total_wgs; b++, w0 += batch_wgs) {
    const uint32_t j = b % f.lanes;
    RtDevParams& Q = f.Pl[j];
    hipStream_t st = j ? w.lane[j].stream : f.stream;
    const bool next = lane_batches[j]++ > 0;
    if (next) HIP_TRY(hipMemsetAsync(f.counts[j] + 1, 0, (size_t)(f.levels + 1) * 4, st));  // the chain's next batch: its level counters
    // (interleaved: groups j, j + lanes, ...; workgroups past the end of the list find no pixel and leave)
    const uint32_t nw = interleave ? ((n_groups + f.lanes - 1u - j) / f.lanes) << group_log2 : std::min(f.total_wgs - w0, batch_wgs);
    if (interleave) Q.batch_first_wg = j << group_log2, Q.batch_stride = f.lanes, Q.batch_group_log2 = group_log2;
    else Q.batch_first_wg = w0, Q.batch_stride = 1, Q.batch_group_log2 = 0;
    Q.q_in = nullptr, Q.q_in_count = nullptr, Q.seg_lo = Q.seg_hi = nullptr;
    Q.q_out = f.levels ? f.q[j][0] : nullptr, Q.q_out_count = f.counts[j] + RT_CNT_LEVEL(1);
    Q.q_capacity = f.q_sort_cap;  // (merged levels: the chain's two queues are one, and RT_CNT_LEVEL(1) is its running total)
    RC_TRY(enqueue_primary(f, j, st, w0, nw, next));
    RC_TRY(f.merged ? enqueue_merged_levels(f, j, st, next) : enqueue_chained_levels(f, j, st));
    RC_TRY(run_hard(f, j, st));  // pairs deferred by the last level's shading (merged levels: every pair of the batch)
  }
  return RT_OK;
}

// ---- join, resolve, and the frame's counters: they come back asynchronously (grids of the next frame); an unverified shape (or a
// blocking call) waits for them.  `again`: children or pairs were dropped, the queues grew -- render the frame again.
static int finish_frame(Frame& f, int attempt, bool& again) {
  rt_scene* s = f.s;
  rt_scene::StreamWs& w = *f.w;
  const uint32_t levels = f.levels, lanes = f.lanes;
  for (uint32_t j = 1; j < lanes; j++) {  // join: the resolve needs every chain's sums
    HIP_TRY(hipEventRecord(w.lane[j].done_ev, w.lane[j].stream));
    HIP_TRY(hipStreamWaitEvent(f.stream, w.lane[j].done_ev, 0));
  }
  f.joined = true;
  RC_TRY(launched(rt_launch_resolve(f.Pl[0], f.stream), f.stream, "resolve launch", "rt_resolve_kernel: attempt", (uint32_t)attempt));
  if (w.cnt_pending && (!s->stream_verified || f.blocking)) {  // (an older read-back still owns the pinned buffer)
    HIP_TRY(hipEventSynchronize(w.cnt_ev));
    w.cnt_pending = false;
  }
  if (!w.cnt_pending) {
    for (uint32_t j = 0; j < lanes; j++)
      HIP_TRY(hipMemcpyAsync(w.cnt_host + (size_t)j * RT_CNT_STRIDE, f.counts[j], (size_t)f.n_cnt * 4, hipMemcpyDeviceToHost, f.stream));
    HIP_TRY(hipEventRecord(w.cnt_ev, f.stream));
    w.cnt_pending = true, w.cnt_host_levels = levels, w.cnt_host_lanes = lanes, w.cnt_host_valid = f.n_batches == lanes, w.cnt_key_gen = s->key_gen;
  }
  if (s->stream_verified && !f.blocking) return RT_OK;
  HIP_TRY(hipEventSynchronize(w.cnt_ev));
  w.cnt_pending = false;
  uint32_t dropped = 0, dropped_pairs = 0, need = 0, need_pairs = 0;
  for (uint32_t j = 0; j < lanes; j++) {
    const uint32_t* c = w.cnt_host + (size_t)j * RT_CNT_STRIDE;
    dropped += c[RT_CNT_OVERFLOW], dropped_pairs += c[RT_CNT_HARD_STAT(levels)];
    // (merged levels: RT_CNT_LEVEL(1) is the running total of ONE queue of 2 q_cap rays)
    for (uint32_t k = 1; k <= levels + 1u; k++) need = std::max(need, f.merged ? (c[RT_CNT_LEVEL(k)] + 1u) / 2u : c[RT_CNT_LEVEL(k)]);
    need_pairs = std::max(need_pairs, c[RT_CNT_HARD_STAT(levels) + 1u]);
  }
  if (!dropped && !dropped_pairs) {
    if (f.rays) return RT_OK;  // (verified for THIS batch only: the next one is verified again)
    if (w.cnt_host_valid) memcpy(s->est, w.cnt_host, sizeof(s->est)), s->est_valid = true;
    s->stream_verified = true;
    // headroom for the frames that now run unverified: a quarter more pairs than this frame deferred (takes effect with the next
    // frame's allocation; nothing was dropped, so this frame stands)
    if (f.hard && f.n_batches == lanes && (uint64_t)need_pairs * 5u / 4u > s->hard_cap) s->hard_cap = cap32((uint64_t)need_pairs * 5u / 4u + 256u);
    return RT_OK;
  }
  // children or pairs were dropped: the counters say what the frame needed; render it again with that
  if (attempt >= (f.merged ? 12 : 6)) return fail(RT_ERR_HIP, "%u child rays / %u pair batches were dropped (queues could not be sized)", dropped, dropped_pairs);
  if (f.n_batches == lanes && !f.forced) {
    // (one queue for all levels: the rays that were dropped would have had children of their own, so the count is a lower bound)
    if (f.merged && dropped) need = std::max<uint32_t>(need + need / 4u, s->q_cap + s->q_cap / 2u);
    if (need > s->q_cap) s->q_cap = cap32((uint64_t)need + need / 16u + 256u);
    if (need_pairs > s->hard_cap) s->hard_cap = cap32((uint64_t)need_pairs + need_pairs / 8u + 256u);
  } else {
    // (batched or forced: the counters are those of the last batch only -- grow geometrically)
    if (dropped) s->q_cap = cap32((uint64_t)s->q_cap * 2u);
    if (dropped_pairs) s->hard_cap = cap32((uint64_t)s->hard_cap * 4u);
  }
  s->est_valid = false, w.acc_pixels = 0;  // partial sums: clear the accumulator
  // ... and the ray counters of the abandoned attempt (rt_stats counts what the reference casts, once)
  if (f.P.counters) HIP_TRY(hipMemsetAsync(f.P.counters, 0, RT_COUNTER_REPLICAS * 16 * sizeof(unsigned long long), f.stream));
  again = true;
  return RT_OK;
}

static int render_frame_impl(rt_scene* s, RtDevParams& P, hipStream_t stream, uint32_t forced_chunk_log2, bool blocking, const RtRayArgs* rays) {
  s->queue_bytes = 0;
  Frame f(s, P, stream, forced_chunk_log2, blocking, rays);
  P.resolve_counts_written = f.split ? 1u : 0u;
  if (!f.secondary && !f.split && !f.defer) {  // one launch of the fused primary kernel
    P.acc = nullptr, P.q_out = nullptr;
    P.batch_first_wg = 0, P.batch_stride = 1, P.batch_group_log2 = 0;
    if (rays) return launched(rt_launch_rays(s->dev, P, *rays, f.total_wgs, stream), stream, "kernel launch", "rt_rays_kernel: workgroups", f.total_wgs);
    char label[64];  // (names the kernel that runs: rt_primary_kernel or the one compiled for this configuration)
    snprintf(label, sizeof(label), "%s: workgroups", rt_primary_variant_name(rt_primary_variant_used(s->dev, P)));
    return launched(rt_launch_primary(s->dev, P, f.total_wgs, stream), stream, "kernel launch", label, f.total_wgs);
  }
  if (f.total_wgs == 0) return RT_OK;  // this rank owns no tile inside the window (more ranks than tiles): nothing to trace, nothing to resolve
  RC_TRY(plan_schedule(f));
  RC_TRY(take_workspace(f));
  match_stream_key(f);
  for (int attempt = 0;; attempt++) {
    bool oom = false, again = false;
    RC_TRY(size_queues(f, attempt, oom));
    if (oom) continue;
    RC_TRY(set_up_chains(f));
    RC_TRY(enqueue_chains(f));
    RC_TRY(finish_frame(f, attempt, again));
    if (!again) return RT_OK;
  }
}

// A frame that fails half-way (HIP / launch error, out of memory) leaves partial sums in the pixel accumulator: mark
// the accumulator dirty so that the next frame clears it.
static int render_frame(rt_scene* s, RtDevParams& P, hipStream_t stream, uint32_t forced_chunk_log2, bool blocking = false,
                        const RtRayArgs* rays = nullptr) {
  const int rc = render_frame_impl(s, P, stream, forced_chunk_log2, blocking, rays);
  if (rc != RT_OK) s->ws[s->cur_ws].acc_pixels = 0;
  // marks the end of this frame's use of its counter block (prepare() of a later frame waits for it)
  if (hipEventRecord(s->frame_ev[s->cur_block], stream) == hipSuccess) s->frame_pending[s->cur_block] = true;
  s->last_block = s->cur_block;
  return rc;
}

// prepare() + the calibration frame of RT_TILE_ORDER_COST when this frame shape has no cost map yet: the frame is rendered
// once in row-major order with every wavefront of the primary kernel adding its run time to its super-tile's entry (a
// complete, valid frame into the caller's buffer), the map is read back (one synchronisation, once per scene and frame
// shape -- like the receiver flags) and prepare() runs again, now sorting the list.
static int prepare_ordered(rt_scene* s, const rt_params* p, uint32_t* argb_dev, const rt_aux* aux_dev, hipStream_t stream, RtDevParams* P,
                           const uint32_t* stage_slot, uint32_t stage_tiles_x) {
  int rc = prepare(s, p, argb_dev, aux_dev, stream, P);
  if (rc != RT_OK || !s->cost_wanted) return rc;
  const size_t n_sup_all = (size_t)((P->win_w + 15u) / 16u) * ((P->win_h + 15u) / 16u);
  if ((rc = s->costmap.ensure(n_sup_all * 4 + 4)) != RT_OK) return rc;
  HIP_TRY(hipMemsetAsync(s->costmap.p, 0, n_sup_all * 4, stream));
  P->cost_map = (uint32_t*)s->costmap.p;
  P->stage_slot = stage_slot;
  P->stage_tiles_x = stage_tiles_x;
  if ((rc = render_frame(s, *P, stream, p->tuning.chunk_log2)) != RT_OK) return rc;
  s->cost_host.assign(n_sup_all, 0u);
  HIP_TRY(hipMemcpyAsync(s->cost_host.data(), s->costmap.p, n_sup_all * 4, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  s->cost_valid = true;
  return prepare(s, p, argb_dev, aux_dev, stream, P);
}

int rt_render_device(rt_scene* s, const rt_params* p, uint32_t* argb_dev, const rt_aux* aux_dev, void* hip_stream) {
  if (!s || !argb_dev) return fail(RT_ERR_INVALID_ARG, "null argument");
  int rc = rt_validate_params(p);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(s->device));
  RtDevParams P;
  if ((rc = prepare_ordered(s, p, argb_dev, aux_dev, (hipStream_t)hip_stream, &P, nullptr, 0)) != RT_OK) return rc;
  return render_frame(s, P, (hipStream_t)hip_stream, p->tuning.chunk_log2);
}

int rt_render_collect_stats(rt_scene* s, rt_stats* st) {
  if (!s || !st) return fail(RT_ERR_INVALID_ARG, "null argument");
  return rt_collect_stats_slot(s, s->last_block, st);
}

}  // extern "C"

// the ray counters of the frame that used `slot` last (the caller has waited for that frame)
int rt_collect_stats_slot(rt_scene* s, int slot, rt_stats* st) {
  if (!s || !st || slot < 0 || slot >= RT_SLOTS) return fail(RT_ERR_INVALID_ARG, "bad argument");
  HIP_TRY(hipSetDevice(s->device));
  unsigned long long all[RT_COUNTER_REPLICAS * 16];
  HIP_TRY(hipMemcpy(all, (unsigned long long*)s->counters.p + (size_t)slot * RT_COUNTER_REPLICAS * 16, sizeof(all), hipMemcpyDeviceToHost));
  unsigned long long c[16] = {0};
  for (unsigned r = 0; r < RT_COUNTER_REPLICAS; r++)
    for (unsigned i = 0; i < 16; i++) c[i] += all[r * 16 + i];
  st->rays_primary = c[0];
  st->rays_reflection = c[1];
  st->rays_refraction = c[2];
  st->rays_shadow = c[3];
  st->pixels_written = c[4];
  st->wave_ray_passes = c[5];
  st->wave_ray_lanes = c[6];
  st->wave_nearest_nodes = c[7];
  st->wave_nearest_tris = c[8];
  st->wave_shadow_nodes = c[9];
  st->wave_shadow_tris = c[10];
  st->wave_shadow_passes = c[11];
  st->wave_nearest_tris_exact = c[12];
  st->wave_shadow_tris_exact = c[13];
  st->rays_traced = c[14];
  st->notes = s->notes | s->sticky_notes;
  s->sticky_notes = 0;
  st->queue_bytes = s->queue_bytes;
  rt_scene_info mi;
  if (rt_scene_memory_info(s, &mi) == RT_OK) st->scene_bytes = mi.bytes_total;
  return RT_OK;
}

extern "C" {


int rt_render(rt_scene* s, const rt_params* p, uint32_t* argb, const rt_aux* aux, rt_stats* stats) {
  if (!s || !argb) return fail(RT_ERR_INVALID_ARG, "null argument");
  if (s->progress_active) return fail(RT_ERR_INVALID_ARG, "a progressive render owns this scene until rt_render_end");
  int rc = rt_validate_params(p);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(s->device));
  auto t_begin = std::chrono::steady_clock::now();
  const size_t npix = (size_t)p->width * p->height;
  // Only the window travels (ChunkView, image_buffer.rs:178-251): the caller's fill of its rows goes up so that
  // miss pixels keep it (image_buffer.rs:27-37), the rendered rows come back.  A progressive band of a 1620-wide
  // frame moves 48 rows, not the frame.
  const uint32_t wx = p->win_w ? p->win_x0 : 0u, wy = p->win_w ? p->win_y0 : 0u;
  const uint32_t ww = p->win_w ? p->win_w : p->width, wh = p->win_w ? p->win_h : p->height;
  const size_t first = (size_t)wy * p->width + wx;
  auto copy_window = [&](void* dst, const void* src, size_t bytes_per_px, hipMemcpyKind kind) -> hipError_t {
    if (ww == p->width)  // whole rows: one contiguous block
      return hipMemcpy((char*)dst + first * bytes_per_px, (const char*)src + first * bytes_per_px,
                       (size_t)wh * p->width * bytes_per_px, kind);
    return hipMemcpy2D((char*)dst + first * bytes_per_px, (size_t)p->width * bytes_per_px,
                       (const char*)src + first * bytes_per_px, (size_t)p->width * bytes_per_px, (size_t)ww * bytes_per_px, wh, kind);
  };
  if ((rc = s->fb.ensure(npix * 4)) != RT_OK) return rc;
  HIP_TRY(copy_window(s->fb.p, argb, 4, hipMemcpyHostToDevice));
  rt_aux ad{};
  if (aux) {
    if (aux->rgb) {
      if ((rc = s->aux_rgb.ensure(npix * 12)) != RT_OK) return rc;
      HIP_TRY(copy_window(s->aux_rgb.p, aux->rgb, 12, hipMemcpyHostToDevice));
      ad.rgb = (float*)s->aux_rgb.p;
    }
    if (aux->hit_id) {
      if ((rc = s->aux_id.ensure(npix * 4)) != RT_OK) return rc;
      HIP_TRY(copy_window(s->aux_id.p, aux->hit_id, 4, hipMemcpyHostToDevice));
      ad.hit_id = (int32_t*)s->aux_id.p;
    }
    if (aux->hit_t) {
      if ((rc = s->aux_t.ensure(npix * 4)) != RT_OK) return rc;
      HIP_TRY(copy_window(s->aux_t.p, aux->hit_t, 4, hipMemcpyHostToDevice));
      ad.hit_t = (float*)s->aux_t.p;
    }
  }
  EventPair ev, ev_setup;  // (ev_setup: e0 alone)
  if ((rc = ev.create()) != RT_OK) return rc;
  HIP_TRY(hipEventCreate(&ev_setup.e0));
  HIP_TRY(hipEventRecord(ev_setup.e0, nullptr));  // what prepare enqueues (table uploads, rt_flags_kernel) is timed as setup_ms
  RtDevParams P;
  if ((rc = prepare_ordered(s, p, (uint32_t*)s->fb.p, aux ? &ad : nullptr, nullptr, &P, nullptr, 0)) != RT_OK) return rc;
  HIP_TRY(hipEventRecord(ev.e0, nullptr));
  if ((rc = render_frame(s, P, nullptr, p->tuning.chunk_log2, true)) != RT_OK) return rc;
  HIP_TRY(hipEventRecord(ev.e1, nullptr));
  HIP_TRY(hipEventSynchronize(ev.e1));
  float ms = 0.f, setup_ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  HIP_TRY(hipEventElapsedTime(&setup_ms, ev_setup.e0, ev.e0));
  auto t_copy = std::chrono::steady_clock::now();
  HIP_TRY(copy_window(argb, s->fb.p, 4, hipMemcpyDeviceToHost));
  const double d2h_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_copy).count();
  if (aux) {
    if (aux->rgb) HIP_TRY(copy_window(aux->rgb, s->aux_rgb.p, 12, hipMemcpyDeviceToHost));
    if (aux->hit_id) HIP_TRY(copy_window(aux->hit_id, s->aux_id.p, 4, hipMemcpyDeviceToHost));
    if (aux->hit_t) HIP_TRY(copy_window(aux->hit_t, s->aux_t.p, 4, hipMemcpyDeviceToHost));
  }
  if (stats) {
    memset(stats, 0, sizeof(*stats));
    if ((rc = rt_render_collect_stats(s, stats)) != RT_OK) return rc;
    stats->kernel_ms = ms;
    stats->setup_ms = setup_ms;
    stats->d2h_ms = d2h_ms;
    stats->total_ms =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  }
  return RT_OK;
}

}  // extern "C"

// ---- ray batches (rt_trace_rays*, rt_rays.cpp): a frame of n x 1 "pixels" whose camera rays are the caller's ------------------
// `p` is the caller's shading parameters with the camera members replaced (width n, height 1, no window, no ranks, no
// anti-aliasing) and has been validated; `r` holds DEVICE pointers.  Uses the scene's tables, frame slots and workspaces as a
// frame does.  Without secondary rays: one asynchronous launch.  With them: the chained schedule, resolved by
// rt_resolve_kernel into r.rgb / r.argb (a plane of the library's when the caller has none), and verified at its end -- the
// call waits for the batch's counters and runs it again with larger queues if a ray or a pair was dropped.
int rt_trace_rays_enqueue(rt_scene* s, const rt_params* p, const RtRayArgs& r, hipStream_t stream) {
  HIP_TRY(hipSetDevice(s->device));
  const bool secondary = (p->flags & (RT_FLAG_REFLECTIONS | RT_FLAG_REFRACTIONS)) != 0;
  uint32_t* argb = r.argb;
  if (secondary && !argb) {  // rt_resolve_kernel needs a target
    RC_TRY(s->rays_argb.ensure((size_t)r.n * 4));
    argb = (uint32_t*)s->rays_argb.p;
  }
  rt_aux aux{};
  aux.rgb = r.rgb;
  RtDevParams P;
  RC_TRY(prepare(s, p, argb, &aux, stream, &P));
  P.sup_list = nullptr, P.n_sup = (r.n + 255u) / 256u;  // (the work list: 256 rays per workgroup, in the caller's order)
  // the resolve kernel only writes hits: a miss reads (0, 0, 0)
  if (secondary && r.rgb) HIP_TRY(hipMemsetAsync(r.rgb, 0, (size_t)r.n * 12, stream));
  return render_frame(s, P, stream, p->tuning.chunk_log2, false, &r);
}

void rt_scene_forget_stream(rt_scene* s, hipStream_t stream) {
  if (s->tables_stream == stream) s->tables_stream = nullptr, s->tables_pending = false;
  if (s->last_stream == stream) s->last_stream = nullptr;
  for (int b = 0; b < RT_SLOTS; b++)
    if (s->frame_stream[b] == stream) s->frame_stream[b] = nullptr, s->frame_pending[b] = false;
}

int rt_render_device_staged(rt_scene* s, const rt_params* p, uint32_t* out_dev, const uint32_t* stage_slot,
                            uint32_t tiles_x, hipStream_t stream) {
  if (!s || !out_dev) return fail(RT_ERR_INVALID_ARG, "null argument");
  int rc = rt_validate_params(p);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(s->device));
  RtDevParams P;
  if ((rc = prepare_ordered(s, p, out_dev, nullptr, stream, &P, stage_slot, tiles_x)) != RT_OK) return rc;
  P.stage_slot = stage_slot;
  P.stage_tiles_x = tiles_x;
  return render_frame(s, P, stream, p->tuning.chunk_log2);
}

