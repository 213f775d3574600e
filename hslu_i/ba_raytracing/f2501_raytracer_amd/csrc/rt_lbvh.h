// rt_lbvh.h -- the tree of a device-side rebuild (rt_scene_rebuild*): a Morton-order LBVH over the triangles a scene holds
// right now, its small subtrees collapsed into leaves.
//
// Compiled twice, as rt_refit.h is: rt_rebuild_packed (rt_scene_pack.cpp) calls these functions in loops on the host, the
// kernels of rt_rebuild.hip are these functions with a thread index.  Every float operation is one rt_fmul / rt_fadd /
// rt_fdiv of rt_refit.h, never fused, so the host model is the specification of the device tree, bit for bit.
//
//   key        canonical triangle t: per axis the centre 0.5 * (min + max) of p0, p0 + e1, p0 + e2 of its intersection
//              record, quantised to 10 bits inside the min / max of all finite centres and interleaved to 30 bits
//              (rt_key_cell / rt_key_morton of rt_ray_key.h).  A degenerate frame axis (hi == lo, or no finite centre)
//              gives cell 0; on any other axis a centre that is not finite takes the top cell.
//   order      a stable sort by key = the total order (key, canonical index); sorted position = new leaf slot.
//   hierarchy  Karras' radix tree over the n sorted 62-bit values key << 32 | index (all distinct).  Inner node i covers
//              the sorted range [f, l] with i == f or i == l, and splits it behind `split`: its children are the ranges
//              [f, split] (inner node `split` when it holds more than one value) and [split + 1, l] (inner node split + 1).
//   collapse   a range of at most max_leaf values is a LEAF CHILD (c = f, n = l - f + 1) of its parent; every other
//              inner node is KEPT and becomes an RtNode.  Kept nodes are numbered by ascending Karras index (an
//              exclusive scan of the keep flags: `rank`), so the root is node 0.  A child's number is NOT larger than its
//              parent's here.  1 <= n <= max_leaf keeps nothing: the tree is rt_build_bvh's single root, child 0 the
//              leaf (0, n), child 1 absent (rt_lbvh_single_root).
//
// Nothing bottom-up needs a pass of its own.  The inner nodes below (and including) node x of range [f, l] are the Karras
// indices f .. l - 1 when x == f and f + 1 .. l when x == l, so the kept nodes of a subtree are a difference of two
// entries of `rank` (rt_lbvh_kept_below); the depth of a kept node and the position of its two entries in the threaded
// (pre-order) copy come from climbing its parent links (rt_lbvh_climb), and "nodes by descending depth" is an order in
// which every child comes before its parent, which is all RtRefitPlan asks of its groups.  Every loop here has a
// compile-time trip bound of at most 64 next to its data-dependent exit, and no index depends on a float that could be a
// NaN.  The boxes are not computed here: they are what the refit of rt_refit.h makes of this topology.
// Not part of the public ABI.
#pragma once

#include "rt_ray_key.h"

#define RT_LBVH_NONE 0xFFFFFFFFu
#define RT_LBVH_DEPTH_BINS 64u  // depths of kept nodes a rebuild can count (the root has depth 1); deeper trees are refused anyway
// most triangles of a rebuild: the one-workgroup step of the keep-flag scan takes RT_ORDER_SCAN_BLOCKS block sums of 2048 flags
#define RT_LBVH_MAX_TRIANGLES (RT_ORDER_SCAN_BLOCKS * 2048u - 8u)

// rt_bvh_tuning.max_leaf as rt_build_bvh applies it
RT_HD static inline uint32_t rt_lbvh_max_leaf(uint32_t max_leaf) { return max_leaf ? (max_leaf > 64u ? 64u : max_leaf) : 4u; }

// ---- keys ---------------------------------------------------------------------------------------------------------------------
// the centre of the triangle of intersection record q = {v1, e1, e2, X}
RT_HD static inline void rt_lbvh_centre(const float* q, float c[3]) {
  for (int a = 0; a < 3; a++) {
    const float p0 = q[a], p1 = rt_fadd(p0, q[3 + a]), p2 = rt_fadd(p0, q[6 + a]);
    float l = INFINITY, h = -INFINITY;
    l = rt_min_keep(l, p0), h = rt_max_keep(h, p0);
    l = rt_min_keep(l, p1), h = rt_max_keep(h, p1);
    l = rt_min_keep(l, p2), h = rt_max_keep(h, p2);
    c[a] = rt_fmul(0.5f, rt_fadd(l, h));
  }
}

// the key of centre c inside the frame (lo, hi) of all finite centres (grown with rt_bounds_grow: order-free)
RT_HD static inline uint32_t rt_lbvh_key(const float lo[3], const float hi[3], const float c[3]) {
  RtKeyFrame f = {};
  uint32_t q[3];
  for (int a = 0; a < 3; a++) {
    const bool active = hi[a] > lo[a];  // (false for the cleared frame +inf, -inf)
    f.bits[a] = RT_KEY_AXIS_BITS;
    f.lo[a] = active ? lo[a] : 0.0f;
    f.extent[a] = active ? rt_fadd(hi[a], -lo[a]) : 1.0f;  // (inf for bounds more than FLT_MAX apart: every cell is cell 0)
    f.scale[a] = (float)(1u << RT_KEY_AXIS_BITS);
    q[a] = !active ? 0u : (!rt_finite(c[a]) ? (1u << RT_KEY_AXIS_BITS) - 1u : rt_key_cell(f, a, c[a]));
  }
  return rt_key_morton(f, 0, 3u, q);
}

// ---- hierarchy ------------------------------------------------------------------------------------------------------------------
struct RtLbvhNode {
  uint32_t f, l, split, parent;  // `parent` is written by the parent (RT_LBVH_NONE: the root)
};

// common leading bits of sorted values i and j; -1 when j is outside [0, n)
RT_HD static inline int rt_lbvh_delta(const uint32_t* key, const uint32_t* idx, uint32_t n, uint32_t i, long long j) {
  if (j < 0 || j >= (long long)n) return -1;
  const unsigned long long a = ((unsigned long long)key[i] << 32) | idx[i], b = ((unsigned long long)key[j] << 32) | idx[j];
  return a == b ? 64 : (int)__builtin_clzll(a ^ b);
}

// inner node i of the radix tree over n >= 2 sorted values (Karras 2012): its range and its split
RT_HD static inline void rt_lbvh_karras(const uint32_t* key, const uint32_t* idx, uint32_t n, uint32_t i, RtLbvhNode* out) {
  const long long d = rt_lbvh_delta(key, idx, n, i, (long long)i + 1) > rt_lbvh_delta(key, idx, n, i, (long long)i - 1) ? 1 : -1;
  const int dmin = rt_lbvh_delta(key, idx, n, i, (long long)i - d);
  long long lmax = 2;
  for (int it = 0; it < 32 && rt_lbvh_delta(key, idx, n, i, (long long)i + lmax * d) > dmin; it++) lmax *= 2;
  long long len = 0, t = lmax >> 1;
  for (int it = 0; it < 34 && t >= 1; it++, t >>= 1)
    if (rt_lbvh_delta(key, idx, n, i, (long long)i + (len + t) * d) > dmin) len += t;
  const long long j = (long long)i + len * d;
  const int dn = rt_lbvh_delta(key, idx, n, i, j);
  long long s = 0;
  t = len;
  for (int it = 0; it < 34; it++) {
    t = (t + 1) >> 1;
    if (rt_lbvh_delta(key, idx, n, i, (long long)i + (s + t) * d) > dn) s += t;
    if (t <= 1) break;
  }
  const long long split = (long long)i + s * d + (d < 0 ? -1 : 0);
  out->f = (uint32_t)(d > 0 ? (long long)i : j), out->l = (uint32_t)(d > 0 ? j : (long long)i), out->split = (uint32_t)split;
}

RT_HD static inline bool rt_lbvh_keeps(const RtLbvhNode& nd, uint32_t max_leaf) { return nd.l - nd.f + 1u > max_leaf; }

// kept nodes among the inner nodes below and including x, whose range is [f, l]; rank = the exclusive scan of the keep
// flags over Karras indices 0 .. n - 1 (index n - 1 is no node: rank[n - 1] = all kept nodes)
RT_HD static inline uint32_t rt_lbvh_kept_below(const uint32_t* rank, uint32_t x, uint32_t f, uint32_t l) {
  return x == f ? rank[l] - rank[f] : rank[l + 1u] - rank[f + 1u];
}

// how kept node `nd` refers to its child k: a leaf (c = first slot, n = count) or a kept node (c = its number, n = 0,
// `kept` = the kept nodes of its subtree)
struct RtLbvhChild {
  uint32_t c, n, kept;
};
RT_HD static inline RtLbvhChild rt_lbvh_child(const uint32_t* rank, uint32_t max_leaf, const RtLbvhNode& nd, int k) {
  const uint32_t f = k ? nd.split + 1u : nd.f, l = k ? nd.l : nd.split;
  RtLbvhChild ch;
  if (l - f + 1u <= max_leaf) {
    ch.c = f, ch.n = l - f + 1u, ch.kept = 0u;
  } else {
    const uint32_t x = k ? nd.split + 1u : nd.split;
    ch.c = rank[x], ch.n = 0u, ch.kept = rt_lbvh_kept_below(rank, x, f, l);
  }
  return ch;
}

// Kept node x: its depth (the root has 1) and the position of its first entry in the threaded copy -- entry, subtree of
// child 0, entry, subtree of child 1, two entries per kept node.  False when the root is more than 64 links away.
RT_HD static inline bool rt_lbvh_climb(const RtLbvhNode* kn, const uint32_t* rank, uint32_t max_leaf, uint32_t x, uint32_t* depth, uint32_t* start) {
  uint32_t d = 1u, s = 0u;
  for (int it = 0; it < 64; it++) {
    const uint32_t p = kn[x].parent;
    if (p == RT_LBVH_NONE) {
      *depth = d, *start = s;
      return true;
    }
    const RtLbvhNode nd = kn[p];
    const bool second = x == nd.split + 1u;
    s += second ? 2u + 2u * rt_lbvh_child(rank, max_leaf, nd, 0).kept : 1u;
    d++, x = p;
  }
  *depth = RT_LBVH_DEPTH_BINS + 1u, *start = 0u;
  return false;
}

// the topology of kept node nd, number r, first threaded entry `start`: the node (NaN boxes until the refit), its two
// threaded entries (skip, leaf) and the children they mirror
RT_HD static inline void rt_lbvh_emit_pair(const RtLbvhChild& c0, const RtLbvhChild& c1, uint32_t r, uint32_t start, RtNode* nodes, RtThrNode* thr,
                                           uint32_t* thr_src) {
  RtNode o;
  for (int a = 0; a < 3; a++) o.lo0[a] = o.hi0[a] = o.lo1[a] = o.hi1[a] = NAN;
  o.c0 = c0.c, o.n0 = c0.n, o.c1 = c1.c, o.n1 = c1.n;
  nodes[r] = o;
  const uint32_t second = start + 1u + 2u * c0.kept;
  RtThrNode t;
  for (int a = 0; a < 3; a++) t.lo[a] = t.hi[a] = NAN;
  t.skip = second, t.leaf = c0.n ? ((c0.n << 24) | c0.c) : 0u;
  thr[start] = t, thr_src[start] = 2u * r;
  t.skip = second + 1u + 2u * c1.kept, t.leaf = c1.n ? ((c1.n << 24) | c1.c) : 0u;
  thr[second] = t, thr_src[second] = 2u * r + 1u;
}
RT_HD static inline void rt_lbvh_emit(const uint32_t* rank, uint32_t max_leaf, const RtLbvhNode& nd, uint32_t r, uint32_t start, RtNode* nodes,
                                      RtThrNode* thr, uint32_t* thr_src) {
  rt_lbvh_emit_pair(rt_lbvh_child(rank, max_leaf, nd, 0), rt_lbvh_child(rank, max_leaf, nd, 1), r, start, nodes, thr, thr_src);
}

// 1 <= n <= max_leaf: one root, child 0 the leaf (0, n), child 1 absent
RT_HD static inline void rt_lbvh_single_root(uint32_t n, RtNode* nodes, RtThrNode* thr, uint32_t* thr_src, uint32_t* group_nodes) {
  RtNode o;
  for (int a = 0; a < 3; a++) o.lo0[a] = o.hi0[a] = o.lo1[a] = o.hi1[a] = NAN;
  o.c0 = 0u, o.n0 = n, o.c1 = RT_NODE_EMPTY, o.n1 = 0u;
  nodes[0] = o;
  RtThrNode t;
  for (int a = 0; a < 3; a++) t.lo[a] = t.hi[a] = NAN;
  t.skip = 1u, t.leaf = (n << 24) | 0u;
  thr[0] = t, thr_src[0] = 0u, group_nodes[0] = 0u;
}

// new leaf slot s takes canonical triangle t from its old slot: intersection record, slot shading record, id (the
// transmissive flag carried, never RT_TRI_DUPLICATE: one slot per triangle), and the plan's tri_slot
RT_HD static inline void rt_lbvh_gather(const RtDevScene& old_sc, const char* old_base, const uint32_t* old_tri_slot, const RtDevScene& sc, char* base,
                                        uint32_t* tri_slot, uint32_t s, uint32_t t) {
  const uint32_t from = old_tri_slot[t];
  const float* qi = (const float*)(old_base + old_sc.off_tri_isect) + 12 * (size_t)from;
  float* qo = rt_blob_f(base, sc.off_tri_isect) + 12 * (size_t)s;
  for (int k = 0; k < 12; k++) qo[k] = qi[k];
  const uint32_t* si = (const uint32_t*)(old_base + old_sc.off_tri_shade) + 4 * (size_t)from;
  uint32_t* so = rt_blob_u(base, sc.off_tri_shade) + 4 * (size_t)s;
  for (int k = 0; k < 4; k++) so[k] = si[k];
  rt_blob_u(base, sc.off_tri_id)[s] = t | (((const uint32_t*)(old_base + old_sc.off_tri_id))[from] & RT_TRI_TRANSMISSIVE);
  tri_slot[t] = s;
}

// ---- the device half (rt_rebuild.hip, rt_rebuild.cpp) ---------------------------------------------------------------------------
// words of RtRebuildWs::result
#define RT_LBVH_RES_NODES 0u      // kept nodes
#define RT_LBVH_RES_LEAVES 1u
#define RT_LBVH_RES_LARGEST 2u    // triangles of the largest leaf
#define RT_LBVH_RES_DEPTH 3u      // deepest kept node (RT_LBVH_DEPTH_BINS + 1: deeper than a climb goes)
#define RT_LBVH_RES_HIST 4u       // [RT_LBVH_DEPTH_BINS + 1]: kept nodes of depth k + 1
#define RT_LBVH_RES_CURSOR 72u    // [RT_LBVH_DEPTH_BINS + 1]: phase 2, where the next node of depth k + 1 goes in the plan's groups
#define RT_LBVH_RES_WORDS 144u
// the device scratch of one rebuild of n triangles
struct RtRebuildWs {
  RtOrderWs sort;    // keys [n], key_a/b, idx_a/b [n], hist, sums (partial and frame stay null); sorted: key_b, idx_b
  float* frame;      // 8 words: lo, hi of the finite centres
  RtLbvhNode* kn;    // [n]
  uint32_t* rank;    // [(n + 7) / 8 * 8]: keep flags, scanned in place
  uint32_t* scan_sums;  // [RT_ORDER_SCAN_BLOCKS]
  uint32_t* depth;   // [n] of kept nodes, by Karras index
  uint32_t* start;   // [n]
  uint32_t* result;  // [RT_LBVH_RES_WORDS]
};
// (rt_order.hip) four stable 8-bit passes over w.keys[0 .. n) with the identity as the first index: w.key_b / w.idx_b
int rt_launch_sort_keys(const RtOrderWs& w, uint32_t n, void* stream);
// (rt_order.hip) exclusive prefix over `total` counts (a multiple of 8, at most RT_ORDER_SCAN_BLOCKS * 2048), in place
int rt_launch_exclusive_scan(uint32_t* counts, uint32_t total, uint32_t* sums, void* stream);
// The first half of phase 1: frame, keys and the sort (w.sort.key_b / w.sort.idx_b).  rt_launch_rebuild_topology runs it itself.
int rt_launch_rebuild_order(const RtDevScene& sc, const char* base, const uint32_t* tri_slot, const RtRebuildWs& w, void* stream);
// Phase 1: keys, order, hierarchy, and w.result up to the histogram.  sc / base / tri_slot: the scene as it stands.
int rt_launch_rebuild_topology(const RtDevScene& sc, const char* base, const uint32_t* tri_slot, const RtRebuildWs& w, uint32_t max_leaf, void* stream);
// Phase 2: the slot records, ids, nodes, threaded entries and plan parts of the new blob (zeroed, its canonical sections
// copied by the caller); w.result's cursors hold the first index of every depth's group.
int rt_launch_rebuild_fill(const RtDevScene& old_sc, const char* old_base, const uint32_t* old_tri_slot, const RtDevScene& sc, char* base,
                           uint32_t* group_nodes, uint32_t* thr_src, uint32_t* tri_slot, const RtRebuildWs& w, uint32_t max_leaf, void* stream);
