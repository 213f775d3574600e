// rt_rebuild.hip -- the kernels of a device-side BVH rebuild (rt_scene_rebuild*): one thread per record, each kernel one
// function of rt_lbvh.h with a thread index, so what they compute is what rt_rebuild_packed computes on the host.
//
// Two phases around one read-back (rt_rebuild.cpp): the topology into scratch buffers -- frame, keys, sort (rt_order.hip),
// radix tree, keep flags and their scan (rt_order.hip), depths -- then, once the host has laid out the new blob, its slot
// records, nodes, threaded entries and plan parts.  The boxes come from the refit kernels of rt_update.hip afterwards.
// A launch boundary is the only ordering used: no kernel ever waits for another workgroup.  The only atomics are counts
// (leaves, the depth histogram, the cursors of the plan's groups): integer sums, so their order changes nothing but the
// order of the nodes inside a group, which a refit does not depend on.
#include <hip/hip_runtime.h>

#include "rt_lbvh.h"

#define RT_RB_WG 256u
#define RT_RB_FRAME_WG 1024u

// the frame of all finite centres: ONE workgroup strides over the triangles, then reduces in LDS (as rt_upd_bounds_kernel)
__global__ __launch_bounds__(RT_RB_FRAME_WG) void rt_lbvh_frame_kernel(RtDevScene sc, const char* base, const uint32_t* tri_slot, float* out) {
  __shared__ float red[6][RT_RB_FRAME_WG];
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t t = threadIdx.x; t < sc.n_triangles; t += RT_RB_FRAME_WG) {
    float c[3];
    rt_lbvh_centre((const float*)(base + sc.off_tri_isect) + 12 * (size_t)tri_slot[t], c);
    rt_bounds_grow(lo, hi, c[0], c[1], c[2]);
  }
  for (int a = 0; a < 3; a++) red[a][threadIdx.x] = lo[a], red[3 + a][threadIdx.x] = hi[a];
  __syncthreads();
  for (uint32_t w = RT_RB_FRAME_WG / 2u; w > 0u; w >>= 1) {
    if (threadIdx.x < w)
      for (int a = 0; a < 3; a++) {
        red[a][threadIdx.x] = fminf(red[a][threadIdx.x], red[a][threadIdx.x + w]);
        red[3 + a][threadIdx.x] = fmaxf(red[3 + a][threadIdx.x], red[3 + a][threadIdx.x + w]);
      }
    __syncthreads();
  }
  if (threadIdx.x < 6u) out[threadIdx.x] = red[threadIdx.x][0];
}

__global__ __launch_bounds__(RT_RB_WG) void rt_lbvh_keys_kernel(RtDevScene sc, const char* base, const uint32_t* tri_slot, const float* frame,
                                                                 uint32_t* keys) {
  const uint32_t t = blockIdx.x * RT_RB_WG + threadIdx.x;
  if (t >= sc.n_triangles) return;
  const float lo[3] = {frame[0], frame[1], frame[2]}, hi[3] = {frame[3], frame[4], frame[5]};
  float c[3];
  rt_lbvh_centre((const float*)(base + sc.off_tri_isect) + 12 * (size_t)tri_slot[t], c);
  keys[t] = rt_lbvh_key(lo, hi, c);
}

// inner node i: its range, its split, the parent link of its inner children, its keep flag; `total` flags in all (zero
// behind the last inner node).  The first RT_LBVH_RES_WORDS threads also clear the result words.
__global__ __launch_bounds__(RT_RB_WG) void rt_lbvh_karras_kernel(const uint32_t* key, const uint32_t* idx, uint32_t n, uint32_t max_leaf, uint32_t total,
                                                                  RtLbvhNode* kn, uint32_t* flags, uint32_t* result) {
  const uint32_t i = blockIdx.x * RT_RB_WG + threadIdx.x;
  if (i < RT_LBVH_RES_WORDS) result[i] = 0u;
  if (i >= total) return;
  if (i + 1u >= n) {
    flags[i] = 0u;
    return;
  }
  RtLbvhNode nd;
  rt_lbvh_karras(key, idx, n, i, &nd);
  kn[i].f = nd.f, kn[i].l = nd.l, kn[i].split = nd.split;
  if (i == 0u) kn[0].parent = RT_LBVH_NONE;
  if (nd.split > nd.f) kn[nd.split].parent = i;
  if (nd.split + 1u < nd.l) kn[nd.split + 1u].parent = i;
  flags[i] = rt_lbvh_keeps(nd, max_leaf) ? 1u : 0u;
}

// kept node i: its depth and first threaded entry; the counts the host lays the new blob out with
__global__ __launch_bounds__(RT_RB_WG) void rt_lbvh_depth_kernel(const RtLbvhNode* kn, const uint32_t* rank, uint32_t n, uint32_t max_leaf,
                                                                 uint32_t* depth, uint32_t* start, uint32_t* result) {
  const uint32_t i = blockIdx.x * RT_RB_WG + threadIdx.x;
  if (i + 1u >= n) return;
  if (i == 0u) result[RT_LBVH_RES_NODES] = rank[n - 1u];
  const RtLbvhNode nd = kn[i];
  if (!rt_lbvh_keeps(nd, max_leaf)) return;
  uint32_t d, s;
  rt_lbvh_climb(kn, rank, max_leaf, i, &d, &s);
  depth[i] = d, start[i] = s;
  atomicMax(&result[RT_LBVH_RES_DEPTH], d);
  atomicAdd(&result[RT_LBVH_RES_HIST + (d - 1u)], 1u);  // (d <= RT_LBVH_DEPTH_BINS + 1)
  for (int k = 0; k < 2; k++) {
    const RtLbvhChild ch = rt_lbvh_child(rank, max_leaf, nd, k);
    if (ch.n) atomicAdd(&result[RT_LBVH_RES_LEAVES], 1u), atomicMax(&result[RT_LBVH_RES_LARGEST], ch.n);
  }
}

__global__ __launch_bounds__(RT_RB_WG) void rt_lbvh_gather_kernel(RtDevScene old_sc, const char* old_base, const uint32_t* old_tri_slot, RtDevScene sc,
                                                                  char* base, uint32_t* tri_slot, const uint32_t* sorted) {
  const uint32_t s = blockIdx.x * RT_RB_WG + threadIdx.x;
  if (s >= sc.n_slots) return;
  const uint32_t t = sorted[s];
  if (t < sc.n_triangles) rt_lbvh_gather(old_sc, old_base, old_tri_slot, sc, base, tri_slot, s, t);  // (always: a permutation)
}

__global__ __launch_bounds__(RT_RB_WG) void rt_lbvh_emit_kernel(RtDevScene sc, char* base, const RtLbvhNode* kn, const uint32_t* rank, uint32_t n,
                                                                uint32_t max_leaf, const uint32_t* depth, const uint32_t* start, uint32_t* cursor,
                                                                uint32_t* group_nodes, uint32_t* thr_src) {
  const uint32_t i = blockIdx.x * RT_RB_WG + threadIdx.x;
  if (i + 1u >= n) return;
  const RtLbvhNode nd = kn[i];
  if (!rt_lbvh_keeps(nd, max_leaf)) return;
  const uint32_t r = rank[i], s = start[i], d = depth[i];
  if (r >= sc.n_nodes || s + 1u >= sc.n_thr || d > RT_LBVH_DEPTH_BINS) return;  // (never: the host sized the blob from these counts)
  rt_lbvh_emit(rank, max_leaf, nd, r, s, (RtNode*)(base + sc.off_nodes), (RtThrNode*)(base + sc.off_nodes_thr), thr_src);
  const uint32_t at = atomicAdd(&cursor[d - 1u], 1u);
  if (at < sc.n_nodes) group_nodes[at] = r;
}

__global__ void rt_lbvh_single_kernel(RtDevScene sc, char* base, uint32_t* group_nodes, uint32_t* thr_src) {
  if (blockIdx.x == 0u && threadIdx.x == 0u)
    rt_lbvh_single_root(sc.n_triangles, (RtNode*)(base + sc.off_nodes), (RtThrNode*)(base + sc.off_nodes_thr), thr_src, group_nodes);
}

static inline uint32_t wgs(uint32_t n) { return (n + RT_RB_WG - 1u) / RT_RB_WG; }

#define RT_RB_LAUNCH(kernel, grid, block, ...)                                  \
  do {                                                                          \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, __VA_ARGS__); \
    const hipError_t e_ = hipGetLastError();                                    \
    if (e_ != hipSuccess) return (int)e_;                                       \
  } while (0)

int rt_launch_rebuild_order(const RtDevScene& sc, const char* base, const uint32_t* tri_slot, const RtRebuildWs& w, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const uint32_t n = sc.n_triangles;
  RT_RB_LAUNCH(rt_lbvh_frame_kernel, 1u, RT_RB_FRAME_WG, sc, base, tri_slot, w.frame);
  RT_RB_LAUNCH(rt_lbvh_keys_kernel, wgs(n), RT_RB_WG, sc, base, tri_slot, (const float*)w.frame, w.sort.keys);
  return rt_launch_sort_keys(w.sort, n, stream_);
}

int rt_launch_rebuild_topology(const RtDevScene& sc, const char* base, const uint32_t* tri_slot, const RtRebuildWs& w, uint32_t max_leaf, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const uint32_t n = sc.n_triangles, total = (n + 7u) / 8u * 8u;
  int e = rt_launch_rebuild_order(sc, base, tri_slot, w, stream_);
  if (e != (int)hipSuccess) return e;
  // (the grid covers the flags and the result words, whichever are more)
  RT_RB_LAUNCH(rt_lbvh_karras_kernel, wgs(total > RT_LBVH_RES_WORDS ? total : RT_LBVH_RES_WORDS), RT_RB_WG, (const uint32_t*)w.sort.key_b,
               (const uint32_t*)w.sort.idx_b, n, max_leaf, total, w.kn, w.rank, w.result);
  e = rt_launch_exclusive_scan(w.rank, total, w.scan_sums, stream_);
  if (e != (int)hipSuccess) return e;
  if (n > 1u)
    RT_RB_LAUNCH(rt_lbvh_depth_kernel, wgs(n - 1u), RT_RB_WG, (const RtLbvhNode*)w.kn, (const uint32_t*)w.rank, n, max_leaf, w.depth, w.start, w.result);
  return (int)hipSuccess;
}

int rt_launch_rebuild_fill(const RtDevScene& old_sc, const char* old_base, const uint32_t* old_tri_slot, const RtDevScene& sc, char* base,
                           uint32_t* group_nodes, uint32_t* thr_src, uint32_t* tri_slot, const RtRebuildWs& w, uint32_t max_leaf, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const uint32_t n = sc.n_triangles;
  RT_RB_LAUNCH(rt_lbvh_gather_kernel, wgs(n), RT_RB_WG, old_sc, old_base, old_tri_slot, sc, base, tri_slot, (const uint32_t*)w.sort.idx_b);
  if (n <= max_leaf)
    RT_RB_LAUNCH(rt_lbvh_single_kernel, 1u, 64u, sc, base, group_nodes, thr_src);
  else
    RT_RB_LAUNCH(rt_lbvh_emit_kernel, wgs(n - 1u), RT_RB_WG, sc, base, (const RtLbvhNode*)w.kn, (const uint32_t*)w.rank, n, max_leaf,
                 (const uint32_t*)w.depth, (const uint32_t*)w.start, w.result + RT_LBVH_RES_CURSOR, group_nodes, thr_src);
  return (int)hipSuccess;
}
#undef RT_RB_LAUNCH
