// rt_host.h -- host-side internals shared by rt_api.cpp (single-GPU entry points) and rt_multi.cpp (multi-GPU
// gather).  Not part of the public ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "rt_closest.h"     // (RtClosestArgs, rt_launch_closest: the kernel of rt_closest_points*, rt_closest.hip)
#include "rt_multihit.h"    // (RtMultiHitArgs, rt_launch_multihit: the kernel of rt_list_intersections*, rt_multihit.hip)
#include "rt_occlusion.h"   // (RtOcclusionArgs, rt_launch_occlusion: the kernels of rt_ambient_occlusion*, rt_occlusion.hip)
#include "rt_solid.h"       // (RtSolidArgs, rt_launch_solid: the kernel of rt_contains_points* / rt_signed_distance*, rt_solid.hip)
#include "rt_ray_key.h"     // (RtOrderWs)
#include "rt_scene_pack.h"  // (rt_internal.h; rt_fail; the device-free scene packer and table builders)

#define fail rt_fail

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess)                                                                      \
      return fail(e_ == hipErrorOutOfMemory ? RT_ERR_OOM : RT_ERR_HIP, "%s failed: %s", #expr, \
                  hipGetErrorString(e_));                                                      \
  } while (0)

// frames of one scene that can be in flight at once (slots: counter block + workspace set)
#define RT_SLOTS 4
// chains a frame with secondary rays is split into (rt_tuning.sub_frames)
#define RT_LANES 2
// deepest reflection / refraction recursion rt_params may ask for (levels of a frame's ray tree)
#define RT_MAX_DEPTH 64u

// A chain's device-side counter block, in dwords, for a ray tree of `levels` levels: overflow, levels, hard, hits, sets, seg.
#define RT_CNT_OVERFLOW 0u                       // dropped children
#define RT_CNT_LEVEL(k) (k)                      // 1 .. levels + 1: rays appended to level k (dropped ones included)
#define RT_CNT_HARD(levels) ((levels) + 2u)      // hard pairs waiting
#define RT_CNT_HARD_STAT(levels) ((levels) + 3u) // [0] dropped pairs, [1] largest batch of pairs
#define RT_CNT_HITS(levels, k) ((levels) + 5u + (k))  // rays of level k that hit something
#define RT_CNT_SETS(levels, k, c) (2u * (levels) + 8u + 3u * (k) + (c))  // phase-split pipeline: sets of class c at level k = 0 .. levels
#define RT_CNT_SEG(levels, k) (2u * (levels) + 8u + 3u * ((levels) + 1u) + (k))  // merged levels: first queue index of level k = 1 .. levels + 1
#define RT_CNT_TOTAL(levels) (2u * (levels) + 8u + 3u * ((levels) + 1u) + (levels) + 2u)
// one chain's row of the host copies (rt_scene::est, StreamWs::cnt_host): the block of the deepest tree, rounded up to 64 bytes
#define RT_CNT_STRIDE ((RT_CNT_TOTAL(RT_MAX_DEPTH) + 15u) & ~15u)
static_assert(RT_CNT_TOTAL(RT_MAX_DEPTH) <= RT_CNT_STRIDE, "counter rows shorter than the counter block");

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  int ensure(size_t bytes) {
    if (bytes <= cap) return RT_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = bytes < 256 ? 256 : bytes;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {
      p = nullptr;
      return fail(RT_ERR_OOM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
    }
    cap = want;
    return RT_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

struct EventPair {  // destroyed on every return path
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int create() {
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    return RT_OK;
  }
  ~EventPair() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
};

// the alignment of every array inside a device allocation that holds several
inline size_t rt_pad256(size_t bytes) { return (bytes + 255u) & ~(size_t)255u; }

// The layout of one allocation that holds several arrays: list the parts, allocate total() bytes, bind().  Every part
// starts on a multiple of 256 bytes and occupies rt_pad256(bytes), so a part of 0 bytes takes none.  add() returns the
// part's offset; with a `slot` the part is remembered, and bind(base) stores base + offset into every slot -- the slots
// must still be where they were.  bind() may be called again: on a host image first, on its device copy afterwards.
// Arithmetic only: no HIP call, usable before a device is chosen.
struct RtArena {
  struct Part {
    void** slot;
    size_t off;
  };
  std::vector<Part> parts;
  size_t used = 0;
  template <class T = void>
  size_t add(size_t bytes, T** slot = nullptr) {
    const size_t off = used;
    used += rt_pad256(bytes);
    if (slot) parts.push_back({(void**)slot, off});
    return off;
  }
  size_t total() const { return used; }
  void bind(void* base) const {
    for (const Part& p : parts) *p.slot = (char*)base + p.off;
  }
};

// the device copy of a refit plan (rt_scene::plan_dev, RtRebuildOut::plan_dev): height_nodes, thr_src, recv_cell, tri_slot
// of part_bytes[] bytes, then 256 bytes for the 8 words of results; fills off[5], returns the size of the allocation
inline size_t rt_plan_layout(const size_t part_bytes[4], size_t off[5]) {
  RtArena lay;
  for (int k = 0; k < 4; k++) off[k] = lay.add(part_bytes[k]);
  off[4] = lay.add(256);
  return lay.total();
}

// the radix sort's arrays for `n` keys, the head of an RtOrderWs (the orders; the Morton sort of a rebuild): parts of `lay`
inline void rt_sort_ws_add(RtArena& lay, size_t n, RtOrderWs* ws) {
  const size_t n_tiles = (n + RT_ORDER_TILE - 1u) / RT_ORDER_TILE;
  for (uint32_t** per : {&ws->keys, &ws->key_a, &ws->key_b, &ws->idx_a, &ws->idx_b}) lay.add(n * 4, per);
  lay.add(256u * n_tiles * 4, &ws->hist), lay.add(RT_ORDER_SCAN_BLOCKS * 4, &ws->sums);
}

// Work enqueued for a handle that nobody has waited for yet: an event behind the last of it, and whether it was recorded.
struct RtPending {
  hipEvent_t ev = nullptr;
  bool pending = false;
  int create() {
    HIP_TRY(hipEventCreate(&ev));
    return RT_OK;
  }
  int mark(hipStream_t stream) {
    HIP_TRY(hipEventRecord(ev, stream));
    pending = true;
    return RT_OK;
  }
  int wait() {
    if (pending) {
      HIP_TRY(hipEventSynchronize(ev));
      pending = false;
    }
    return RT_OK;
  }
  void clear() { pending = false; }  // the caller knows that the stream has drained
  void destroy() {
    if (pending) (void)hipEventSynchronize(ev);
    if (ev) (void)hipEventDestroy(ev);
    ev = nullptr, pending = false;
  }
};

// what every create function does first with the device it is given
inline int rt_open_device(int device) {
  const int ndev = rt_device_count();
  if (ndev <= 0) return fail(RT_ERR_NO_DEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(RT_ERR_INVALID_ARG, "device %d out of range (%d visible)", device, ndev);
  HIP_TRY(hipSetDevice(device));
  return RT_OK;
}

// The device side of an entry point that takes HOST arrays (rt_cast_rays, rt_any_intersection, rt_trace_rays*,
// rt_ray_order_build): one device allocation for the call, every array 256-byte aligned in it, and a private stream, so
// that the call neither waits for nor delays work the caller has on the null stream.  in() / out() list the arrays: *slot
// is the host array (NULL: not staged) and becomes its device twin in begin(), which allocates, creates the stream and
// enqueues the uploads; the caller enqueues its work on `stream`; finish() enqueues the downloads and waits.  The stream
// drains and is destroyed on every return path, then the memory is freed.
struct HostCall {
  struct Array {
    void* host;
    void** dev;
    size_t bytes;
    bool up, down;
  };
  std::vector<Array> arrays;
  RtArena lay;
  DevBuf buf;
  hipStream_t stream = nullptr;
  template <class T>
  void in(const T** slot, size_t bytes) {
    if (*slot) arrays.push_back({(void*)*slot, (void**)slot, bytes, true, false}), lay.add(bytes, slot);
  }
  // upload_first: a plane the kernels write only in part (argb: a miss leaves the caller's value)
  template <class T>
  void out(T** slot, size_t bytes, bool upload_first = false) {
    if (*slot) arrays.push_back({*slot, (void**)slot, bytes, upload_first, true}), lay.add(bytes, slot);
  }
  int begin() {
    const int rc = buf.ensure(lay.total());
    if (rc != RT_OK) return rc;
    lay.bind(buf.p);
    HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    for (const Array& a : arrays)
      if (a.up) HIP_TRY(hipMemcpyAsync(*a.dev, a.host, a.bytes, hipMemcpyHostToDevice, stream));
    return RT_OK;
  }
  int finish() {
    for (const Array& a : arrays)
      if (a.down) HIP_TRY(hipMemcpyAsync(a.host, *a.dev, a.bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return RT_OK;
  }
  ~HostCall() {
    if (stream) (void)hipStreamSynchronize(stream), (void)hipStreamDestroy(stream);
    buf.release();
  }
};

// `stream` has drained and is about to be destroyed: what the scene enqueued on it is done, and its handle must not be used again
void rt_scene_forget_stream(rt_scene* s, hipStream_t stream);

// A HostCall's stream that carried frames of a scene: the scene remembers streams -- of table uploads, of its frame slots --
// and must not remember this one once it is gone.  Declared behind the HostCall, so that it runs before the stream goes.
struct Forget {
  rt_scene* scene;
  HostCall& c;
  ~Forget() {
    if (c.stream) (void)hipStreamSynchronize(c.stream), rt_scene_forget_stream(scene, c.stream);
  }
};

// the checks of a rt_ray_batch every entry point that takes one makes; before any HIP call
inline int rt_check_ray_batch(const rt_ray_batch* b, const char* fn) {
  if (!b) return fail(RT_ERR_INVALID_ARG, "%s: null ray batch", fn);
  if (b->abi_version != RT_ABI_VERSION)
    return fail(RT_ERR_INVALID_ARG, "%s: rt_ray_batch.abi_version %u != %u", fn, b->abi_version, RT_ABI_VERSION);
  if (b->n_rays && (!b->origin || !b->direction)) return fail(RT_ERR_INVALID_ARG, "%s: origin / direction missing", fn);
  return RT_OK;
}

// what the ray counts of a frame with secondary rays depend on (besides the scene): a frame with the key of the last
// verified frame renders without a synchronisation
struct StreamKey {
  uint32_t width, height, flags, aa_rays, aa_unique, light_mult, depth_refl, depth_refr, win[4], tile_size, n_ranks, rank, traversal,
      cand_cap, cloud_seed, n_cloud_sets, forced, tables, staged, flags_on, n_sup, lanes, split, sort_bits, lists_on, merged,
      rays;  // 1: a ray batch (rt_trace_rays*), 0: a camera frame
  float f[8];
};

struct rt_scene {
  int device = 0;
  RtDevScene dev{};
  rt_bvh_info info{};
  DevBuf blob;  // spheres, triangles, materials, lights, BVH (RtDevScene offsets)
  // per-render workspaces
  DevBuf aa, cloud, counters, fb, aux_rgb, aux_id, aux_t, suplist;
  DevBuf progress_fb;   // rt_render_begin: the device frame its bands are rendered into
  DevBuf rays_argb;     // rt_trace_rays* with secondary rays and no argb plane of the caller's: rt_resolve_kernel's target
  bool progress_active = false;  // a progressive render (rt_render_begin .. rt_render_end) owns the scene
  uint64_t budget = 0;  // rt_scene_desc.device_budget_bytes as applied: bounds flags + per-cell lists
  size_t bytes_bvh = 0; // of `blob`: nodes + octant copies + threaded copy
  // What ONE frame with secondary rays owns while it is in flight: ray queues, sort workspace, hard-pair queue, level
  // counters (+ their pinned read-back), pixel accumulator.  Two sets, so that two such frames can be in flight (the
  // second set is only allocated when a frame is enqueued while the one before it is still running).
  // A frame's ray tree runs as RT_LANES independent CHAINS (halves of its primary work-group list), each with its own
  // queues, sort workspace, pair queue and level counters; chain 0 on the caller's stream, the others on streams of the
  // set (forked / joined with events).  The chains meet in the pixel accumulator.
  struct Lane {
    DevBuf queues, trace_ws, hard, qcount;
    DevBuf hitrec, sets;              // phase-split pipeline: hit records of the primary launch, (wavefront, light) set records
    void* sort_hist_clean = nullptr;  // the histogram (address, size) that is known to be zero
    uint32_t sort_hist_buckets = 0;
    hipStream_t stream = nullptr;     // chains 1..: their own stream
    hipEvent_t done_ev = nullptr;     // ... and the event the caller's stream waits for before the resolve
    // pipelined levels (rt_tuning.levels): the two streams levels are shaded on alternately, their join events, one event per traced level
    hipStream_t shade_stream[2] = {nullptr, nullptr};
    hipEvent_t shade_done[2] = {nullptr, nullptr};
    std::vector<hipEvent_t> level_ev;
    hipEvent_t hit_ev = nullptr;      // merged levels: the camera rays' hits (and children) exist -- their shading may start on shade_stream[0]
  };
  struct StreamWs {
    Lane lane[RT_LANES];
    DevBuf acc;
    size_t acc_pixels = 0;            // pixels the (zeroed) accumulator currently covers; 0 = must be cleared before use
    uint32_t* cnt_host = nullptr;     // pinned, [RT_LANES][RT_CNT_STRIDE]: asynchronous read-back of the chains' counters
    hipEvent_t cnt_ev = nullptr, fork_ev = nullptr;
    bool cnt_pending = false, cnt_host_valid = false;
    uint32_t cnt_host_levels = 0, cnt_host_lanes = 0, cnt_key_gen = 0;
    size_t bytes() const {
      size_t b = acc.cap;
      for (const Lane& l : lane) b += l.queues.cap + l.trace_ws.cap + l.hard.cap + l.hitrec.cap + l.sets.cap;
      return b;
    }
  } ws[RT_SLOTS];
  std::vector<uint32_t> sup_host;
  uint32_t sup_key[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // window, tile size, n_ranks, rank, order the list was built for
  // RT_TILE_ORDER_COST: measured cost per super-tile (window-relative index) for cost_key = frame shape + what a ray costs
  DevBuf costmap;
  std::vector<uint32_t> cost_host;
  uint32_t cost_key[13] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  bool cost_valid = false, cost_wanted = false;
  // ray streaming (frames with secondary rays): sizes shared by both workspace sets, see render_frame_impl
  uint32_t q_cap = 0, hard_cap = 0, batch_items = 0;  // per chain: rays per queue, pairs; primary work items per batch
  StreamKey stream_key{};
  uint32_t key_gen = 0;          // bumped whenever stream_key changes (counter read-backs are stamped with it)
  uint32_t sticky_notes = 0;     // notes about frames already delivered (reported by the next rt_render_collect_stats)
  bool stream_verified = false;  // a frame of this key ran without dropping a ray or a pair
  uint32_t est[RT_LANES][RT_CNT_STRIDE] = {{0}};  // the counters of the last complete frame of this key, per chain (grids of the next one)
  bool est_valid = false;
  uint32_t sort_bits_wanted = 0;    // rt_tuning.sort_bits of the current frame (0 = default)
  uint32_t lanes_wanted = 0;        // rt_tuning.sub_frames of the current frame (0 = default)
  uint32_t phases_wanted = 0;       // rt_tuning.phases of the current frame (0 = default)
  uint32_t levels_wanted = 0;       // rt_tuning.levels of the current frame (0 = default)
  uint32_t calm_frames = 1u << 30;  // frames enqueued in a row while no other frame of the scene was running (sub_frames = 0: auto)
  uint32_t tables_version = 0;      // bumped whenever a parameter table (AA samples, light clouds, flags, tile list) is uploaded
  float aabb_lo[3] = {0.f, 0.f, 0.f}, aabb_hi[3] = {1.f, 1.f, 1.f};  // bounds of all objects (Morton keys)
  // host copies of the parameter tables last uploaded (skip re-upload when unchanged)
  std::vector<float> aa_host, cloud_host, cloud_scaled;
  std::vector<uint32_t> aa_table;  // device image: [2U] offsets (float bits), [U] multiplicities, [n] sample -> thread
  uint32_t aa_unique = 0;
  bool aa_dedup = true;
  // The tables are uploaded on the stream of the call that changed them; a later call on another stream waits for
  // that upload (tables_ev) before its kernels read them.
  hipEvent_t tables_ev = nullptr;
  hipStream_t tables_stream = nullptr, last_stream = nullptr;
  bool tables_pending = false, rendered = false;
  float cloud_ball[4] = {0.f, 0.f, 0.f, -1.f};  // centre offset (scene units) + radius of all cloud offsets
  // receiver flags (rt_flags_kernel): cell tables built with the scene, flags rebuilt when the beam constants change
  DevBuf flag_geo, flags;
  DevBuf cell_lists;     // per (receiver cell, light): 8 x uint16 leaf slots surviving the cell's fat beam (rt_flags_kernel)
  DevBuf resolve_work;   // work list of rt_cell_resolve_kernel (at most 64 MiB, counted with the lists)
  DevBuf cell_wide;      // marks of certain crossings (rt_cell_through.h), then the pool of wide records (rt_cell_resolve.h: 64 bytes each, then the counter); counted with the lists
  bool cell_wide_built = false;
  size_t cell_marks_bytes = 0;  // the marks of rt_cell_through.h in front of the records of cell_wide (0: none); counted with the lists
  bool cell_lists_built = false;
  uint32_t n_cells = 0, n_tri_cells = 0;
  float flags_key[8] = {-1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // beam_delta, eps, cloud centre: what the flags were built for
  float cloud_ball_f[3] = {0.f, 0.f, 0.f};
  // Frames in flight.  Consecutive frames may be enqueued on different streams so that the head of one overlaps the
  // drain of the other (a launch cannot end before its longest wavefront does).  A frame owns one of RT_SLOTS SLOTS -- a
  // counter block and, with secondary rays, a workspace set (ws[]) -- guarded by the event recorded behind the frame that
  // used the slot last.  A frame takes a slot whose last frame has finished if there is one (a host that renders frame by
  // frame only ever uses slot 0), else the one used longest ago.
  hipEvent_t frame_ev[RT_SLOTS] = {};
  bool frame_pending[RT_SLOTS] = {};
  uint32_t frame_seq[RT_SLOTS] = {};
  hipStream_t frame_stream[RT_SLOTS] = {};  // the stream the slot's last frame was enqueued on
  uint32_t frame_no = 0;
  int cur_block = 0, last_block = 0;
  int cur_ws = 0;                  // workspace set of the frame being enqueued (normally its slot)
  int ws_last_block[RT_SLOTS] = {0, 1, 2, 3};  // the slot of the frame that used each workspace set last
  // which fast paths the last frame did NOT take (rt_stats.notes)
  uint32_t notes = 0;
  size_t queue_bytes = 0;  // ray queues + hard-pair queue + sort workspace of the last frame with secondary rays
  // in-place updates (rt_update.cpp): the refit plan and its device copy (parts at plan_off[]: height_nodes, thr_src,
  // recv_cell, tri_slot, 8 words of results), the staging of a host delta (pinned, device) and the pinned read-back
  RtRefitPlan plan;
  DevBuf plan_dev, upd_dev;
  size_t plan_off[5] = {0, 0, 0, 0, 0};
  void* upd_stage = nullptr;
  size_t upd_stage_cap = 0;
  float* upd_back = nullptr;
  // SAH report (rt_scene_bvh_quality): the integer sums of rt_sah.h over the tree as created, the triangle cost the tree
  // was built with, and the three 64-bit words the kernel adds into
  uint64_t sah_created[2] = {0, 0};
  float sah_tri_cost = 2.0f;
  DevBuf sah_dev;
  uint32_t max_leaf = 4;  // rt_bvh_tuning.max_leaf as applied at creation: what rt_scene_rebuild* collapses its tree to
};


// rt_update.cpp: the device copy of pk.plan (rt_scene_create) and the release of everything an update allocated (rt_scene_destroy)
int rt_scene_upload_plan(rt_scene* s, const RtPackedScene& pk);
void rt_scene_release_update(rt_scene* s);

// rt_update.cpp: waits for every frame of the scene still in flight (they read the records an update or a rebuild replaces)
int rt_scene_wait_frames(rt_scene* s);

// rt_rebuild.cpp: the device side of rt_scene_rebuild* without a handle -- from a blob and two plan parts on the device to
// a new blob and a new plan, both allocated here (the layout of rt_scene_upload_plan).  Blocks on `stream`.  On any
// failure nothing is left allocated and `in` is untouched.
struct RtRebuildIn {
  RtDevScene dev;             // the scene as it stands, base set
  const uint32_t* recv_cell;  // device: RtRefitPlan::recv_cell
  const uint32_t* tri_slot;   // device: RtRefitPlan::tri_slot
  uint32_t max_leaf, n_materials;
  uint32_t method, radius;    // RT_REBUILD_LBVH (0; radius unused) or RT_REBUILD_PLOC with the radius as applied (1 .. 32)
};
struct RtRebuildOut {
  DevBuf blob, plan_dev;
  size_t plan_off[5] = {0, 0, 0, 0, 0};
  RtDevScene dev{};           // base set
  RtRebuildShape shape;
  std::vector<uint32_t> height_nodes, thr_src, tri_slot;  // host copies of the new plan parts
  float bounds[6] = {0.f, 0.f, 0.f, 1.f, 1.f, 1.f};
  uint32_t receivers_disabled = 0;
  float device_ms = 0.f;
  uint32_t iterations = 0;    // of the PLOC loop (0: the LBVH, or a single root)
};
int rt_rebuild_device(const RtRebuildIn& in, hipStream_t stream, RtRebuildOut* out);

// rt_api.cpp internals used by the multi-GPU path
// Multi-GPU staging: when `stage_slot` (device, [tiles_x * tiles_y]) is given, packed pixels are stored into the
// rank-compact staging buffer `out_dev` (tile slot * tile_size^2 + offset inside the tile) instead of a W x H frame.
int rt_render_device_staged(rt_scene* s, const rt_params* p, uint32_t* out_dev, const uint32_t* stage_slot,
                            uint32_t tiles_x, hipStream_t stream);
int rt_validate_params(const rt_params* p);
// a ray batch through the frame scheduler (rt_api.cpp; entry points and validation: rt_rays.cpp)
int rt_trace_rays_enqueue(rt_scene* s, const rt_params* p, const RtRayArgs& r, hipStream_t stream);
// what rt_trace_rays* refuse in a call, before any HIP call and without looking at the scene (rt_rays.cpp); `fn` names the caller
int rt_trace_rays_check(const rt_scene* s, const rt_params* p, const rt_ray_batch* b, const rt_ray_radiance* out, const char* fn);
// the device memory an order holds (rt_ray_order_info.bytes), readable before the order was ever built (rt_rays.cpp)
size_t rt_ray_order_bytes(const rt_ray_order* o);
// the permutation a built or set order holds on its device, [n] (rt_rays.cpp)
const uint32_t* rt_ray_order_perm(const rt_ray_order* o);
// rt_trace_rays_ordered_device through a permutation the caller holds on the scene's device instead of an order handle
// (perm == nullptr: rt_trace_rays_device): the partitioned orders of an adaptive view.  Same checks, same enqueue.
int rt_trace_rays_perm_device(rt_scene* s, const rt_params* p, const rt_ray_batch* b, const uint32_t* perm, const rt_ray_radiance* out,
                              hipStream_t stream, const char* fn);
// the ray counters of the frame that used frame slot `slot` of the scene last (rt_scene::cur_block right after a frame
// was enqueued); the caller has waited for that frame
int rt_collect_stats_slot(rt_scene* s, int slot, rt_stats* st);
