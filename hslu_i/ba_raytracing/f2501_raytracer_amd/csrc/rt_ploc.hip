// rt_ploc.hip -- the kernels of a PLOC rebuild (rt_scene_rebuild_with*, RT_REBUILD_PLOC): each kernel is one function of
// rt_ploc.h with a thread index, so what they compute is what rt_rebuild_ploc_packed computes on the host.
//
// After the order of rt_rebuild.hip (frame, keys, sort): the leaves; then per iteration the neighbour search (one thread
// per cluster, a workgroup's boxes and a halo of RT_PLOC_MAX_RADIUS on either side in LDS), the "survives" flags, their
// exclusive scan (rt_order.hip) and the compaction, which also writes the new nodes; then the climb, which places every
// kept node and every triangle and counts what the host lays the new blob out with.  Phase 2 gathers the slot records and
// emits the nodes, as rt_rebuild.hip does for the LBVH.
//
// The loop's state -- m clusters, `next` merges so far, the iterations run -- lives in device memory: every kernel of an
// iteration reads it and does nothing once m is 1, the compaction writes the next state into the other of two copies.  The
// host enqueues RT_PLOC_BATCH iterations, reads the state back and sizes the next batch's grids from the m it read (m never
// grows).  A launch boundary is the only ordering used: no kernel ever waits for another workgroup.  The only atomics are
// the counts the LBVH path also counts (leaves, the depth histogram, the cursors of the plan's groups).
#include <hip/hip_runtime.h>

#include "rt_ploc.h"

#define RT_PLOC_WG 256u
#define RT_PLOC_WINDOW (RT_PLOC_WG + 2u * RT_PLOC_MAX_RADIUS)

// node x < 2 n - 1: the leaf of sorted position x, or an inner node not made yet (cleared); position x starts as leaf x.
// The first threads also clear the result words and write the first state.
__global__ __launch_bounds__(RT_PLOC_WG) void rt_ploc_leaves_kernel(RtDevScene sc, const char* base, const uint32_t* tri_slot, const uint32_t* sorted,
                                                                    RtPlocNode* node, uint32_t* cid, RtPlocState* state, uint32_t* result) {
  const uint32_t x = blockIdx.x * RT_PLOC_WG + threadIdx.x, n = sc.n_triangles;
  if (x < RT_LBVH_RES_WORDS) result[x] = 0u;
  if (x == 0u) state[0].m = n, state[0].next = 0u, state[0].iterations = 0u, state[0].pad = 0u;
  if (x >= 2u * n - 1u) return;
  if (x >= n) {
    node[x].parent = RT_LBVH_NONE;
    return;
  }
  const uint32_t t = sorted[x];
  if (t >= n) return;  // (never: a permutation)
  rt_ploc_leaf(sc, base, tri_slot[t], &node[x]);
  cid[x] = x;
}

__global__ __launch_bounds__(RT_PLOC_WG) void rt_ploc_nearest_kernel(const RtPlocNode* node, uint32_t n_ids, const uint32_t* cid, const RtPlocState* state,
                                                                     uint32_t radius, uint32_t* nn) {
  __shared__ float box[6u * RT_PLOC_WINDOW];
  const uint32_t m = state->m, first = blockIdx.x * RT_PLOC_WG;
  if (m <= 1u || first >= m) return;  // (uniform)
  const uint32_t shift = RT_PLOC_MAX_RADIUS - first;  // position p at p + shift: the window starts RT_PLOC_MAX_RADIUS before `first`
  for (uint32_t k = threadIdx.x; k < RT_PLOC_WINDOW; k += RT_PLOC_WG) {
    const uint32_t p = k - shift;  // (wraps below position 0: not < m)
    if (p >= m) continue;
    const uint32_t id = cid[p];
    if (id >= n_ids) continue;  // (never)
    for (int a = 0; a < 3; a++) box[a * RT_PLOC_WINDOW + k] = node[id].lo[a], box[(3 + a) * RT_PLOC_WINDOW + k] = node[id].hi[a];
  }
  __syncthreads();
  const uint32_t i = first + threadIdx.x;
  if (i < m) nn[i] = rt_ploc_nearest(box, RT_PLOC_WINDOW, shift, m, radius, i);
}

// `total` flags in all (zero behind the last cluster)
__global__ __launch_bounds__(RT_PLOC_WG) void rt_ploc_flags_kernel(const uint32_t* nn, const RtPlocState* state, uint32_t total, uint32_t* flags) {
  const uint32_t i = blockIdx.x * RT_PLOC_WG + threadIdx.x, m = state->m;
  if (m <= 1u || i >= total) return;
  flags[i] = i < m && rt_ploc_survives(nn, m, i) ? 1u : 0u;
}

__global__ __launch_bounds__(RT_PLOC_WG) void rt_ploc_merge_kernel(RtPlocNode* node, uint32_t n, const uint32_t* cid, const uint32_t* nn, const uint32_t* scan,
                                                                   const RtPlocState* state, uint32_t max_leaf, uint32_t* cid_out, RtPlocState* state_out) {
  const uint32_t i = blockIdx.x * RT_PLOC_WG + threadIdx.x;
  const RtPlocState st = *state;
  if (st.m <= 1u) {
    if (i == 0u) *state_out = st;
    return;
  }
  if (i < st.m) rt_ploc_merge(node, n, cid, nn, scan, st, max_leaf, i, cid_out, state_out);
}

// node x: a kept node's place and the counts the host lays the new blob out with; a triangle's slot
__global__ __launch_bounds__(RT_PLOC_WG) void rt_ploc_climb_kernel(const RtPlocNode* node, uint32_t n, uint32_t max_leaf, RtPlocPlace* place, uint32_t* result) {
  const uint32_t x = blockIdx.x * RT_PLOC_WG + threadIdx.x;
  if (x >= 2u * n - 1u) return;
  if (x == 2u * n - 2u) result[RT_LBVH_RES_NODES] = node[x].kept;  // (the root: the last merge)
  const bool kept = rt_ploc_keeps(node[x], max_leaf);
  if (!kept && x >= n) return;
  RtPlocPlace p;
  rt_ploc_climb(node, x, kept ? RT_PLOC_CLIMB_KEPT : RT_PLOC_CLIMB_LEAF, &p);
  place[x] = p;
  if (!kept) return;
  atomicMax(&result[RT_LBVH_RES_DEPTH], p.depth);
  atomicAdd(&result[RT_LBVH_RES_HIST + (p.depth - 1u)], 1u);  // (depth <= RT_LBVH_DEPTH_BINS + 1)
  for (int k = 0; k < 2; k++) {
    const RtLbvhChild ch = rt_ploc_child(node, max_leaf, x, p, k);
    if (ch.n) atomicAdd(&result[RT_LBVH_RES_LEAVES], 1u), atomicMax(&result[RT_LBVH_RES_LARGEST], ch.n);
  }
}

__global__ __launch_bounds__(RT_PLOC_WG) void rt_ploc_gather_kernel(RtDevScene old_sc, const char* old_base, const uint32_t* old_tri_slot, RtDevScene sc,
                                                                    char* base, uint32_t* tri_slot, const uint32_t* sorted, const RtPlocPlace* place) {
  const uint32_t x = blockIdx.x * RT_PLOC_WG + threadIdx.x;
  if (x >= sc.n_triangles) return;
  const uint32_t t = sorted[x], s = place[x].first;
  if (t < sc.n_triangles && s < sc.n_slots) rt_lbvh_gather(old_sc, old_base, old_tri_slot, sc, base, tri_slot, s, t);  // (always: two permutations)
}

__global__ __launch_bounds__(RT_PLOC_WG) void rt_ploc_emit_kernel(RtDevScene sc, char* base, const RtPlocNode* node, const RtPlocPlace* place, uint32_t n,
                                                                  uint32_t max_leaf, uint32_t* cursor, uint32_t* group_nodes, uint32_t* thr_src) {
  const uint32_t x = n + blockIdx.x * RT_PLOC_WG + threadIdx.x;
  if (x >= 2u * n - 1u || !rt_ploc_keeps(node[x], max_leaf)) return;
  const RtPlocPlace p = place[x];
  if (p.number >= sc.n_nodes || p.start + 1u >= sc.n_thr || p.depth > RT_LBVH_DEPTH_BINS) return;  // (never: the host sized the blob from these counts)
  const RtLbvhChild c0 = rt_ploc_child(node, max_leaf, x, p, 0), c1 = rt_ploc_child(node, max_leaf, x, p, 1);
  if (p.start + 2u + 2u * c0.kept > sc.n_thr) return;  // (never)
  rt_lbvh_emit_pair(c0, c1, p.number, p.start, (RtNode*)(base + sc.off_nodes), (RtThrNode*)(base + sc.off_nodes_thr), thr_src);
  const uint32_t at = atomicAdd(&cursor[p.depth - 1u], 1u);
  if (at < sc.n_nodes) group_nodes[at] = p.number;
}

static inline uint32_t wgs(uint32_t n) { return (n + RT_PLOC_WG - 1u) / RT_PLOC_WG; }

#define RT_PLOC_LAUNCH(kernel, grid, block, ...)                                \
  do {                                                                          \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, __VA_ARGS__); \
    const hipError_t e_ = hipGetLastError();                                    \
    if (e_ != hipSuccess) return (int)e_;                                       \
  } while (0)

int rt_launch_ploc_topology(const RtDevScene& sc, const char* base, const uint32_t* tri_slot, const RtRebuildWs& w, const RtPlocWs& pw, uint32_t max_leaf,
                            uint32_t radius, void* stream_, uint32_t* iterations) {
  hipStream_t stream = (hipStream_t)stream_;
  const uint32_t n = sc.n_triangles, n_ids = 2u * n - 1u;
  RT_PLOC_LAUNCH(rt_ploc_leaves_kernel, wgs(n_ids > RT_LBVH_RES_WORDS ? n_ids : RT_LBVH_RES_WORDS), RT_PLOC_WG, sc, base, tri_slot,
                 (const uint32_t*)w.sort.idx_b, pw.node, pw.cid[0], pw.state, w.result);
  RtPlocState st = {n, 0u, 0u, 0u};
  uint32_t it = 0u;  // iterations enqueued: iteration `it` reads state and cid copy it & 1 and writes the other
  while (st.m > 1u && it < RT_PLOC_MAX_ITERATIONS) {
    const uint32_t m = st.m, total = (m + 7u) / 8u * 8u;
    for (uint32_t b = 0; b < RT_PLOC_BATCH; b++, it++) {
      const uint32_t in = it & 1u, out = in ^ 1u;
      RT_PLOC_LAUNCH(rt_ploc_nearest_kernel, wgs(m), RT_PLOC_WG, (const RtPlocNode*)pw.node, n_ids, (const uint32_t*)pw.cid[in],
                     (const RtPlocState*)(pw.state + in), radius, pw.nn);
      RT_PLOC_LAUNCH(rt_ploc_flags_kernel, wgs(total), RT_PLOC_WG, (const uint32_t*)pw.nn, (const RtPlocState*)(pw.state + in), total, pw.flags);
      const int e = rt_launch_exclusive_scan(pw.flags, total, pw.scan_sums, stream_);
      if (e != (int)hipSuccess) return e;
      RT_PLOC_LAUNCH(rt_ploc_merge_kernel, wgs(m), RT_PLOC_WG, pw.node, n, (const uint32_t*)pw.cid[in], (const uint32_t*)pw.nn, (const uint32_t*)pw.flags,
                     (const RtPlocState*)(pw.state + in), max_leaf, pw.cid[out], pw.state + out);
    }
    hipError_t e = hipMemcpyAsync(&st, pw.state + (it & 1u), sizeof(st), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return (int)e;
  }
  *iterations = st.m > 1u ? RT_PLOC_MAX_ITERATIONS + 1u : st.iterations;
  if (st.m > 1u) return (int)hipSuccess;  // (cut off: the caller refuses)
  RT_PLOC_LAUNCH(rt_ploc_climb_kernel, wgs(n_ids), RT_PLOC_WG, (const RtPlocNode*)pw.node, n, max_leaf, pw.place, w.result);
  return (int)hipSuccess;
}

int rt_launch_ploc_fill(const RtDevScene& old_sc, const char* old_base, const uint32_t* old_tri_slot, const RtDevScene& sc, char* base, uint32_t* group_nodes,
                        uint32_t* thr_src, uint32_t* tri_slot, const RtRebuildWs& w, const RtPlocWs& pw, uint32_t max_leaf, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const uint32_t n = sc.n_triangles;
  RT_PLOC_LAUNCH(rt_ploc_gather_kernel, wgs(n), RT_PLOC_WG, old_sc, old_base, old_tri_slot, sc, base, tri_slot, (const uint32_t*)w.sort.idx_b,
                 (const RtPlocPlace*)pw.place);
  RT_PLOC_LAUNCH(rt_ploc_emit_kernel, wgs(n - 1u), RT_PLOC_WG, sc, base, (const RtPlocNode*)pw.node, (const RtPlocPlace*)pw.place, n, max_leaf,
                 w.result + RT_LBVH_RES_CURSOR, group_nodes, thr_src);
  return (int)hipSuccess;
}
#undef RT_PLOC_LAUNCH
