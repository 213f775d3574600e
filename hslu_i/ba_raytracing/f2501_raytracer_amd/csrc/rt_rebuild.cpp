// rt_rebuild.cpp -- rt_scene_rebuild[_with][_device]: the stateful half of a device-side BVH rebuild.  What a rebuild
// computes is in rt_lbvh.h, rt_ploc.h and rt_refit.h (host models: rt_rebuild_packed, rt_rebuild_ploc_packed; kernels:
// rt_rebuild.hip, rt_ploc.hip, rt_order.hip, rt_update.hip); here: the scratch, the read-back between the two phases, the
// new blob and plan, the SAH comparison of RT_REBUILD_KEEP_BETTER, and the swap.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>

#include "rt_host.h"
#include "rt_ploc.h"
#include "rt_sah.h"

int rt_rebuild_device(const RtRebuildIn& in, hipStream_t stream, RtRebuildOut* out) {
  const uint32_t n = in.dev.n_triangles, max_leaf = in.max_leaf;
  struct Bufs {  // released on every return path but the last
    DevBuf ws, blob, plan;
    ~Bufs() { ws.release(), blob.release(), plan.release(); }
  } b;
  // ---- scratch
  const size_t per = (size_t)n * 4, sums = RT_ORDER_SCAN_BLOCKS * 4, rank = (size_t)(n + 7u) / 8u * 8u * 4, ids = 2 * (size_t)n - 1u;
  const bool ploc = in.method == RT_REBUILD_PLOC && n > max_leaf;  // (n <= max_leaf: the single root of either method)
  RtRebuildWs w{};
  RtPlocWs pw{};
  RtArena lay;
  rt_sort_ws_add(lay, n, &w.sort);
  lay.add(256, &w.frame), lay.add(RT_LBVH_RES_WORDS * 4, &w.result);
  if (ploc) {
    lay.add(ids * sizeof(RtPlocNode), &pw.node), lay.add(ids * sizeof(RtPlocPlace), &pw.place);
    lay.add(per, &pw.cid[0]), lay.add(per, &pw.cid[1]), lay.add(per, &pw.nn);
    lay.add(rank, &pw.flags), lay.add(sums, &pw.scan_sums), lay.add(256, &pw.state);
  } else {
    lay.add(per, &w.depth), lay.add(per, &w.start), lay.add(sums, &w.scan_sums);
    lay.add((size_t)n * sizeof(RtLbvhNode), &w.kn), lay.add(rank, &w.rank);
  }
  int rc = b.ws.ensure(lay.total());
  if (rc != RT_OK) return rc;
  lay.bind(b.ws.p);
  EventPair ev;
  if ((rc = ev.create()) != RT_OK) return rc;
  HIP_TRY(hipEventRecord(ev.e0, stream));
  // ---- phase 1: the topology, and the few words the new blob is laid out with
  hipError_t e;
  if (ploc) {
    e = (hipError_t)rt_launch_rebuild_order(in.dev, in.dev.base, in.tri_slot, w, stream);
    if (e == hipSuccess) e = (hipError_t)rt_launch_ploc_topology(in.dev, in.dev.base, in.tri_slot, w, pw, max_leaf, in.radius, stream, &out->iterations);
    if (e == hipSuccess && out->iterations > RT_PLOC_MAX_ITERATIONS)
      return fail(RT_ERR_UNSUPPORTED, "rt_scene_rebuild: PLOC did not finish within %u iterations", RT_PLOC_MAX_ITERATIONS);
  } else {
    e = (hipError_t)rt_launch_rebuild_topology(in.dev, in.dev.base, in.tri_slot, w, max_leaf, stream);
  }
  if (e != hipSuccess) return fail(RT_ERR_HIP, "rebuild launch failed: %s", hipGetErrorString(e));
  uint32_t result[RT_LBVH_RES_WORDS];
  HIP_TRY(hipMemcpyAsync(result, w.result, sizeof(result), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  rc = rt_rebuild_shape(n, max_leaf, result, &out->shape);
  if (rc != RT_OK) return rc;
  const RtRebuildShape& sh = out->shape;
  RtDevScene sc{};
  const RtBlobCounts counts{in.dev.n_spheres, n, n, sh.n_nodes, sh.n_thr, in.n_materials, in.dev.n_lights};
  const size_t bytes = rt_blob_layout(counts, &sc);
  if (!bytes) return fail(RT_ERR_UNSUPPORTED, "scene data exceeds 4 GiB");
  rc = b.blob.ensure(bytes);
  if (rc != RT_OK) return rc;
  sc.base = (const char*)b.blob.p;
  const size_t part[4] = {(size_t)sh.n_nodes * 4, (size_t)sh.n_thr * 4, (size_t)n * 8, (size_t)n * 4};
  const size_t plan_bytes = rt_plan_layout(part, out->plan_off);
  rc = b.plan.ensure(plan_bytes);
  if (rc != RT_OK) return rc;
  // ---- phase 2: the new blob
  char* base = (char*)b.blob.p;
  char* plan = (char*)b.plan.p;
  HIP_TRY(hipMemsetAsync(base, 0, bytes, stream));
  HIP_TRY(hipMemsetAsync(plan, 0, plan_bytes, stream));
  RtBlobSection sec[RT_BLOB_CANONICAL_SECTIONS];
  rt_blob_canonical_sections(in.dev, sc, in.n_materials, sec);
  for (const RtBlobSection& c : sec)
    if (c.bytes) HIP_TRY(hipMemcpyAsync(base + c.to, in.dev.base + c.from, c.bytes, hipMemcpyDeviceToDevice, stream));
  HIP_TRY(hipMemcpyAsync(plan + out->plan_off[2], in.recv_cell, part[2], hipMemcpyDeviceToDevice, stream));
  uint32_t cursor[RT_LBVH_DEPTH_BINS + 1u] = {0};  // depth k + 1 at k: the first index of its group
  if (n > max_leaf)  // (the single root has no kept node to place: its group is written as it is)
    for (uint32_t g = 0; g + 1u < sh.group_offset.size(); g++) cursor[sh.max_depth - 2u - g] = sh.group_offset[g];
  HIP_TRY(hipMemcpyAsync(w.result + RT_LBVH_RES_CURSOR, cursor, sizeof(cursor), hipMemcpyHostToDevice, stream));
  uint32_t* group_nodes = (uint32_t*)(plan + out->plan_off[0]);
  uint32_t* thr_src = (uint32_t*)(plan + out->plan_off[1]);
  uint32_t* tri_slot = (uint32_t*)(plan + out->plan_off[3]);
  if (ploc)
    e = (hipError_t)rt_launch_ploc_fill(in.dev, in.dev.base, in.tri_slot, sc, base, group_nodes, thr_src, tri_slot, w, pw, max_leaf, stream);
  else
    e = (hipError_t)rt_launch_rebuild_fill(in.dev, in.dev.base, in.tri_slot, sc, base, group_nodes, thr_src, tri_slot, w, max_leaf, stream);
  if (e != hipSuccess) return fail(RT_ERR_HIP, "rebuild launch failed: %s", hipGetErrorString(e));
  // ---- the boxes: the refit of this topology
  RtUpdateArgs u{};
  u.base = base;
  u.height_nodes = group_nodes, u.thr_src = thr_src, u.tri_slot = tri_slot;
  u.recv_cell = (const uint32_t*)(plan + out->plan_off[2]);
  u.bounds = (float*)(plan + out->plan_off[4]);
  u.height_offset = sh.group_offset.data();
  u.n_heights = (uint32_t)sh.group_offset.size() - 1u;
  u.n_materials = in.n_materials;
  e = (hipError_t)rt_launch_refit(sc, u, stream);
  if (e != hipSuccess) return fail(RT_ERR_HIP, "rebuild refit launch failed: %s", hipGetErrorString(e));
  HIP_TRY(hipEventRecord(ev.e1, stream));
  float back[8];
  out->height_nodes.resize(sh.n_nodes), out->thr_src.resize(sh.n_thr), out->tri_slot.resize(n);
  HIP_TRY(hipMemcpyAsync(back, u.bounds, 32, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(out->height_nodes.data(), group_nodes, part[0], hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(out->thr_src.data(), thr_src, part[1], hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(out->tri_slot.data(), tri_slot, part[3], hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipEventElapsedTime(&out->device_ms, ev.e0, ev.e1));
  memcpy(out->bounds, back, 24), memcpy(&out->receivers_disabled, back + 6, 4);
  out->dev = sc;
  out->blob = b.blob, out->plan_dev = b.plan;
  b.blob = DevBuf(), b.plan = DevBuf();  // (theirs now)
  return RT_OK;
}

namespace {

// what rt_scene_rebuild_with* refuse of a descriptor, before the scene is looked at and before any HIP call; *radius: as applied
int check_desc(const rt_rebuild_desc* d, uint32_t* radius) {
  if (!d) return fail(RT_ERR_INVALID_ARG, "rt_scene_rebuild_with: null rt_rebuild_desc");
  if (d->method != RT_REBUILD_LBVH && d->method != RT_REBUILD_PLOC) return fail(RT_ERR_INVALID_ARG, "rt_rebuild_desc.method = %u: unknown method", d->method);
  if (d->method == RT_REBUILD_LBVH && d->radius) return fail(RT_ERR_INVALID_ARG, "rt_rebuild_desc.radius = %u: the LBVH takes no radius", d->radius);
  *radius = 0u;
  if (d->method == RT_REBUILD_PLOC) {
    const int rc = rt_check_ploc_radius(d->radius, radius);
    if (rc != RT_OK) return rc;
  }
  if (d->flags & ~RT_REBUILD_KEEP_BETTER) return fail(RT_ERR_INVALID_ARG, "rt_rebuild_desc.flags = 0x%x: unknown bits", d->flags);
  if (d->reserved) return fail(RT_ERR_INVALID_ARG, "rt_rebuild_desc.reserved must be 0");
  return RT_OK;
}

// desc == nullptr: rt_scene_rebuild[_device], the LBVH and no SAH report
int rebuild_impl(rt_scene* s, const rt_rebuild_desc* desc, uint32_t radius, hipStream_t stream, bool own_stream, rt_rebuild_info* info,
                 rt_rebuild_report* report) {
  const auto t0 = std::chrono::steady_clock::now();
  if (!s) return fail(RT_ERR_INVALID_ARG, "rt_scene_rebuild: null scene");
  if (s->progress_active) return fail(RT_ERR_INVALID_ARG, "a progressive render owns this scene until rt_render_end");
  int rc = rt_check_rebuild(s->dev);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(s->device));
  rc = rt_scene_wait_frames(s);  // every frame of this scene still in flight reads the old blob
  if (rc != RT_OK) return rc;
  struct Stream {  // destroyed on every return path
    hipStream_t st = nullptr;
    ~Stream() {
      if (st) (void)hipStreamSynchronize(st), (void)hipStreamDestroy(st);
    }
  } q;
  if (own_stream) {
    HIP_TRY(hipStreamCreateWithFlags(&q.st, hipStreamNonBlocking));
    stream = q.st;
  }
  RtRebuildIn in{};
  in.dev = s->dev;
  in.recv_cell = (const uint32_t*)((const char*)s->plan_dev.p + s->plan_off[2]);
  in.tri_slot = (const uint32_t*)((const char*)s->plan_dev.p + s->plan_off[3]);
  in.max_leaf = s->max_leaf, in.n_materials = (uint32_t)s->plan.mat_class.size();
  in.method = desc ? desc->method : RT_REBUILD_LBVH, in.radius = radius;
  RtRebuildOut o;
  rc = rt_rebuild_device(in, stream, &o);
  if (rc != RT_OK) return rc;  // (the handle is as it was)
  struct Candidate {  // freed on every return path before the swap
    RtRebuildOut* o;
    ~Candidate() {
      if (o) o->blob.release(), o->plan_dev.release();
    }
  } cand{&o};
  bool swap = true;
  if (desc) {  // ---- the SAH sums of the tree in place and of the candidate, from the kernel of rt_scene_bvh_quality
    unsigned long long* dev = (unsigned long long*)s->sah_dev.p;  // (256 bytes: two reports of three words)
    hipError_t e = (hipError_t)rt_launch_sah((const RtNode*)((const char*)s->blob.p + s->dev.off_nodes), s->dev.n_nodes, dev, stream);
    if (e == hipSuccess) e = (hipError_t)rt_launch_sah((const RtNode*)((const char*)o.blob.p + o.dev.off_nodes), o.dev.n_nodes, dev + 4, stream);
    if (e != hipSuccess) return fail(RT_ERR_HIP, "SAH report launch failed: %s", hipGetErrorString(e));
    unsigned long long host[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(host, dev, sizeof(host), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const double cost = (double)s->sah_tri_cost;
    const double before = ((double)host[0] + cost * (double)host[1]) / RT_SAH_ONE, after = ((double)host[4] + cost * (double)host[5]) / RT_SAH_ONE;
    swap = !(desc->flags & RT_REBUILD_KEEP_BETTER) || after < before;
    if (report) {
      report->inner_q_before = host[0], report->leaf_q_before = host[1], report->inner_q_after = host[4], report->leaf_q_after = host[5];
      report->sah_before = before, report->sah_after = after;
      report->swapped = swap ? 1u : 0u, report->iterations = o.iterations;
    }
  }
  if (swap) {  // ---- nothing below can fail
    cand.o = nullptr;
    s->blob.release(), s->plan_dev.release();
    s->blob = o.blob, s->plan_dev = o.plan_dev;
    memcpy(s->plan_off, o.plan_off, sizeof(s->plan_off));
    s->dev = o.dev;
    s->plan.height_nodes.swap(o.height_nodes), s->plan.thr_src.swap(o.thr_src), s->plan.tri_slot.swap(o.tri_slot);
    s->plan.height_offset = o.shape.group_offset;
    s->plan.receivers_disabled = o.receivers_disabled;
    rt_rebuild_info_of(o.shape, s->dev.n_triangles, &s->info, &s->bytes_bvh);
    memcpy(s->aabb_lo, o.bounds, 12), memcpy(s->aabb_hi, o.bounds + 3, 12);
    // what the scene has cached about its old tree: as a geometry update (the cell lists hold leaf slots)
    s->stream_verified = false, s->est_valid = false, s->key_gen++;
    s->flags_key[0] = -1.f, s->cell_lists_built = false, s->cost_valid = false;
  }
  if (info) {
    info->device_ms = o.device_ms;
    info->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    info->n_nodes = s->info.n_nodes, info->n_leaves = s->info.n_leaves, info->max_depth = s->info.max_depth, info->max_leaf_size = s->info.max_leaf_size;
    info->tables_invalidated = swap ? RT_UPDATE_INVALIDATES_RECEIVER_TABLES | RT_UPDATE_INVALIDATES_TILE_COSTS | RT_UPDATE_INVALIDATES_QUEUE_SIZES : 0u;
    info->reserved = 0;
  }
  return RT_OK;
}

int rebuild_with(rt_scene* s, const rt_rebuild_desc* d, hipStream_t stream, bool own_stream, rt_rebuild_report* report) {
  uint32_t radius = 0u;
  const int rc = check_desc(d, &radius);
  if (rc != RT_OK) return rc;
  if (report) *report = rt_rebuild_report{};
  return rebuild_impl(s, d, radius, stream, own_stream, report ? &report->info : nullptr, report);
}

}  // namespace

extern "C" {

int rt_scene_rebuild(rt_scene* s, rt_rebuild_info* info) { return rebuild_impl(s, nullptr, 0u, nullptr, true, info, nullptr); }

int rt_scene_rebuild_device(rt_scene* s, void* hip_stream, rt_rebuild_info* info) {
  return rebuild_impl(s, nullptr, 0u, (hipStream_t)hip_stream, false, info, nullptr);
}

int rt_scene_rebuild_with(rt_scene* s, const rt_rebuild_desc* d, rt_rebuild_report* report) { return rebuild_with(s, d, nullptr, true, report); }

int rt_scene_rebuild_with_device(rt_scene* s, const rt_rebuild_desc* d, void* hip_stream, rt_rebuild_report* report) {
  return rebuild_with(s, d, (hipStream_t)hip_stream, false, report);
}

}  // extern "C"
