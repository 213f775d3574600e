// rt_ploc.h -- the second tree a device-side rebuild can make (rt_scene_rebuild_with*, RT_REBUILD_PLOC): parallel locally-
// ordered clustering (Meister & Bittner 2018) over the Morton order of rt_lbvh.h.  Where the LBVH splits at Morton cells,
// PLOC merges, bottom-up, the two clusters whose common box has the smallest surface area, looking only at the clusters
// within `radius` positions of each other in the Morton order.
//
// Compiled twice, as rt_lbvh.h is: rt_rebuild_ploc_packed (rt_scene_pack.cpp) calls these functions in loops on the host,
// the kernels of rt_ploc.hip are these functions with a thread index.  Every float operation is one rt_fmul / rt_fadd of
// rt_refit.h, never fused, and every decision is a comparison of such floats as 32-bit patterns, so the host model is the
// specification of the device tree, bit for bit.
//
//   order      the LBVH's: rt_lbvh_centre, rt_lbvh_key, the stable sort.  Cluster position s starts as the leaf of
//              triangle idx[s] (node id s); its box is rt_grow_slot_box of the triangle's slot record, grown from the
//              cleared box -- the box the refit will give it.
//   distance   d(a, b) = the half area ex ey + ey ez + ez ex of the union box (min / max per axis, then e = hi - lo; an e
//              that is negative or not a number counts as 0, an area that is not finite as +inf), compared as the 32 bits
//              of a non-negative float.  The cluster at the LOWER position is always the first argument: both members of a
//              pair then see the same bits even where a box holds a NaN (rt_min_keep is not symmetric there).
//   nearest    among m clusters nn(i) is the j != i, |i - j| <= radius, 0 <= j < m, that minimises the pair (d, i xor j).
//              The second component is symmetric and differs for different j, so the closest pair of all is always
//              mutual -- every iteration merges at least one pair -- and n identical triangles halve per iteration
//              (nn(i) = i xor 1) where a tie broken by j or by |i - j| would merge ONE pair per iteration.
//   merge      i and j = nn(i) merge iff nn(j) == i.  The new cluster sits at the lower position, child 0 the lower
//              cluster, child 1 the upper one, box = the union as computed.  Compaction keeps the order: one exclusive scan
//              of the "survives" flags (the upper member of a pair does not), and the pair of upper position j becomes
//              node n + next + (j - scan[j]).  Internal numbering is free: nothing below depends on it.
//   end        m == 1; more than RT_PLOC_MAX_ITERATIONS iterations is refused.
//   collapse   the LBVH's rule: a subtree of at most max_leaf triangles is a LEAF CHILD (c = first slot, n = size), every
//              other inner node is KEPT.  `size` and `kept` (kept nodes below and including) are summed at merge time.
//   numbers    the leaf slot of a triangle is its rank in the depth-first order of the tree (child 0 first), kept nodes are
//              numbered in pre-order (root 0), the threaded copy and the depth are laid out as rt_lbvh_climb /
//              rt_lbvh_emit lay them out, groups run by descending depth -- all from climbing parent links with the sums
//              taken on the way up (rt_ploc_climb).  PLOC has no depth guarantee: a kept node more than 64 links below
//              the root is the refusal of rt_rebuild_shape.  n <= max_leaf keeps nothing: rt_lbvh_single_root.
//
// Every loop has a compile-time trip bound next to its data-dependent exit, and no index depends on a float that could be
// a NaN.  The boxes of the final tree are not these: they are what the refit of rt_refit.h makes of this topology.
// Not part of the public ABI.
#pragma once

#include "rt_lbvh.h"

#define RT_PLOC_MAX_RADIUS 32u
#define RT_PLOC_DEFAULT_RADIUS 8u
// A guard, not a tuning knob.  Every iteration merges at least one pair, so n - 1 iterations always suffice.  Measured on
// the host model (radius 8): 15 iterations for the 87 triangles of test_scene, 31 for a mesh of 1687, 30 for a heightfield
// of 8192, 44 to 55 for a mesh of 14 569 under 0 to 20 % jitter -- geometry with any irregularity pairs up a constant
// fraction of its clusters per iteration, and 2^23 triangles at that rate stay below 100.  The other extreme exists: on a
// perfectly regular strip of equal triangles the distance to the next cluster grows monotonically along the order (the pad
// of a box grows with the magnitude of its coordinates), every cluster prefers its lower neighbour, only the pair at the
// low end is mutual, and the loop needs about n / 2 iterations: 25 for 40 triangles, 108 for 200.  No batch size makes
// that usable, so such a scene is refused here (at 256: 32 read-back batches, a few milliseconds) and keeps the LBVH.
#define RT_PLOC_MAX_ITERATIONS 256u
#define RT_PLOC_BATCH 8u  // iterations enqueued per read-back of m
#define RT_PLOC_CLIMB_KEPT 64  // links a kept node climbs at most (rt_lbvh_climb's bound)
#define RT_PLOC_CLIMB_LEAF 128  // ... a triangle: at most max_leaf - 1 <= 63 collapsed links more

// node id x: a leaf (x < n: the triangle at sorted position x) or the pair n + k made by the k-th merge
struct RtPlocNode {
  float lo[3], hi[3];
  uint32_t c0, c1, parent;  // RT_LBVH_NONE: none (a leaf's children, the root's parent)
  uint32_t size, kept;      // triangles below; nodes below and including with size > max_leaf
  uint32_t pad;
};
// what the climb of node x gives: kept nodes use all four, leaves only `first` (their slot)
struct RtPlocPlace {
  uint32_t depth, start, number, first;
};
// the loop's state, read by every kernel of an iteration and rewritten by its last one (two copies, used alternately)
struct RtPlocState {
  uint32_t m, next, iterations, pad;
};

RT_HD static inline uint32_t rt_ploc_bits(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return u;
}

// the leaf of sorted position s: triangle t in old slot `slot`
RT_HD static inline void rt_ploc_leaf(const RtDevScene& old_sc, const char* old_base, uint32_t slot, RtPlocNode* out) {
  RtPlocNode nd;
  for (int a = 0; a < 3; a++) nd.lo[a] = INFINITY, nd.hi[a] = -INFINITY;
  rt_grow_slot_box(old_sc, old_base, slot, nd.lo, nd.hi);
  nd.c0 = nd.c1 = nd.parent = RT_LBVH_NONE, nd.size = 1u, nd.kept = 0u, nd.pad = 0u;
  *out = nd;
}

// the union of box a (the cluster at the lower position) and box b, and its distance
RT_HD static inline uint32_t rt_ploc_union(const float alo[3], const float ahi[3], const float blo[3], const float bhi[3], float lo[3], float hi[3]) {
  float e[3];
  for (int a = 0; a < 3; a++) {
    lo[a] = rt_min_keep(alo[a], blo[a]), hi[a] = rt_max_keep(ahi[a], bhi[a]);
    const float d = rt_fadd(hi[a], -lo[a]);
    e[a] = d > 0.0f ? d : 0.0f;  // (a NaN counts as 0)
  }
  const float area = rt_fadd(rt_fadd(rt_fmul(e[0], e[1]), rt_fmul(e[1], e[2])), rt_fmul(e[2], e[0]));
  return rt_finite(area) ? rt_ploc_bits(area) : 0x7F800000u;  // (inf * 0: not a number, counts as +inf)
}

// Boxes of cluster positions as six planes of `stride` floats: component c of position p is box[c * stride + (p + shift)]
// (unsigned wrap-around: a workgroup's LDS window starts before its first position).  lower < upper.
RT_HD static inline uint32_t rt_ploc_distance(const float* box, uint32_t stride, uint32_t shift, uint32_t lower, uint32_t upper) {
  const uint32_t a = lower + shift, b = upper + shift;
  const float alo[3] = {box[a], box[stride + a], box[2u * stride + a]}, ahi[3] = {box[3u * stride + a], box[4u * stride + a], box[5u * stride + a]};
  const float blo[3] = {box[b], box[stride + b], box[2u * stride + b]}, bhi[3] = {box[3u * stride + b], box[4u * stride + b], box[5u * stride + b]};
  float lo[3], hi[3];
  return rt_ploc_union(alo, ahi, blo, bhi, lo, hi);
}

// nn(i) among m >= 2 clusters
RT_HD static inline uint32_t rt_ploc_nearest(const float* box, uint32_t stride, uint32_t shift, uint32_t m, uint32_t radius, uint32_t i) {
  uint32_t best_d = 0xFFFFFFFFu, best_x = 0xFFFFFFFFu, best_j = i;
  for (uint32_t k = 1u; k <= RT_PLOC_MAX_RADIUS && k <= radius; k++) {
    if (i >= k) {
      const uint32_t j = i - k, d = rt_ploc_distance(box, stride, shift, j, i), x = i ^ j;
      if (d < best_d || (d == best_d && x < best_x)) best_d = d, best_x = x, best_j = j;
    }
    if (i + k < m) {
      const uint32_t j = i + k, d = rt_ploc_distance(box, stride, shift, i, j), x = i ^ j;
      if (d < best_d || (d == best_d && x < best_x)) best_d = d, best_x = x, best_j = j;
    }
  }
  return best_j;
}

// whether position i is still a cluster after this iteration: the upper member of a mutual pair is not
RT_HD static inline bool rt_ploc_survives(const uint32_t* nn, uint32_t m, uint32_t i) {
  const uint32_t j = nn[i];
  return !(j < i && nn[j] == i);  // (j < m: nn holds positions)
}

// Position i of m in iteration's compaction: a survivor moves to scan[i]; the lower member of a mutual pair becomes the new
// node first.  n_ids = 2 n - 1.  The thread of the last position also writes the next state.
RT_HD static inline void rt_ploc_merge(RtPlocNode* node, uint32_t n, const uint32_t* cid, const uint32_t* nn, const uint32_t* scan, const RtPlocState& st,
                                       uint32_t max_leaf, uint32_t i, uint32_t* cid_out, RtPlocState* st_out) {
  const uint32_t m = st.m, j = nn[i];
  const bool survives = rt_ploc_survives(nn, m, i);
  if (i + 1u == m) {
    const uint32_t m_new = scan[i] + (survives ? 1u : 0u);
    st_out->m = m_new, st_out->next = st.next + (m - m_new), st_out->iterations = st.iterations + 1u, st_out->pad = 0u;
  }
  if (!survives) return;
  uint32_t id = cid[i];
  if (j > i && j < m && nn[j] == i) {
    const uint32_t a = id, b = cid[j];
    id = n + st.next + (j - scan[j]);
    if (id >= 2u * n - 1u || a >= id || b >= id) return;  // (never: n - 1 merges in all, each of older nodes)
    RtPlocNode nd;
    (void)rt_ploc_union(node[a].lo, node[a].hi, node[b].lo, node[b].hi, nd.lo, nd.hi);
    nd.c0 = a, nd.c1 = b, nd.parent = RT_LBVH_NONE;
    nd.size = node[a].size + node[b].size;
    nd.kept = node[a].kept + node[b].kept + (nd.size > max_leaf ? 1u : 0u);
    nd.pad = 0u;
    node[id] = nd;
    node[a].parent = id, node[b].parent = id;
  }
  if (scan[i] < m) cid_out[scan[i]] = id;
}

// Node x climbs to the root: depth (the root has 1), the first entry of its pair in the threaded copy, its pre-order number
// among the kept nodes (all three as rt_lbvh_climb counts them: they mean something for a kept node only) and the first
// leaf slot of its subtree.  False when the root is more than `trips` links away.
RT_HD static inline bool rt_ploc_climb(const RtPlocNode* node, uint32_t x, int trips, RtPlocPlace* out) {
  RtPlocPlace p = {1u, 0u, 0u, 0u};
  for (int it = 0; it < RT_PLOC_CLIMB_LEAF && it < trips; it++) {
    const uint32_t up = node[x].parent;
    if (up == RT_LBVH_NONE) {
      *out = p;
      return true;
    }
    const uint32_t c0 = node[up].c0;
    const bool second = x != c0;
    p.start += second ? 2u + 2u * node[c0].kept : 1u;
    p.number += second ? 1u + node[c0].kept : 1u;
    p.first += second ? node[c0].size : 0u;
    p.depth++, x = up;
  }
  out->depth = RT_LBVH_DEPTH_BINS + 1u, out->start = 0u, out->number = 0u, out->first = RT_LBVH_NONE;
  return false;
}

RT_HD static inline bool rt_ploc_keeps(const RtPlocNode& nd, uint32_t max_leaf) { return nd.size > max_leaf; }

// how kept node x (placed at p) refers to its child k
RT_HD static inline RtLbvhChild rt_ploc_child(const RtPlocNode* node, uint32_t max_leaf, uint32_t x, const RtPlocPlace& p, int k) {
  const RtPlocNode& c0 = node[node[x].c0];
  const RtPlocNode& ch = k ? node[node[x].c1] : c0;
  RtLbvhChild o;
  if (!rt_ploc_keeps(ch, max_leaf))
    o.c = p.first + (k ? c0.size : 0u), o.n = ch.size, o.kept = 0u;
  else
    o.c = p.number + 1u + (k ? c0.kept : 0u), o.n = 0u, o.kept = ch.kept;
  return o;
}

// ---- the device half (rt_ploc.hip, rt_rebuild.cpp) ------------------------------------------------------------------------------
// the device scratch of one PLOC rebuild of n triangles, next to the sort's, the frame and the result words of RtRebuildWs
struct RtPlocWs {
  RtPlocNode* node;      // [2 n - 1]
  RtPlocPlace* place;    // [2 n - 1]
  uint32_t* cid[2];      // [n] each: the node id of every cluster position, used alternately
  uint32_t* nn;          // [n]
  uint32_t* flags;       // [(n + 7) / 8 * 8]: "survives", scanned in place
  uint32_t* scan_sums;   // [RT_ORDER_SCAN_BLOCKS]
  RtPlocState* state;    // [2]
};
// Phase 1 after the order (w.sort.idx_b): leaves, the loop, the climb and w.result up to the histogram.  BLOCKS on `stream`
// once per RT_PLOC_BATCH iterations.  hipError_t as int; *iterations = RT_PLOC_MAX_ITERATIONS + 1 when the loop was cut off.
int rt_launch_ploc_topology(const RtDevScene& sc, const char* base, const uint32_t* tri_slot, const RtRebuildWs& w, const RtPlocWs& pw, uint32_t max_leaf,
                            uint32_t radius, void* stream, uint32_t* iterations);
// Phase 2, as rt_launch_rebuild_fill (n > max_leaf)
int rt_launch_ploc_fill(const RtDevScene& old_sc, const char* old_base, const uint32_t* old_tri_slot, const RtDevScene& sc, char* base, uint32_t* group_nodes,
                        uint32_t* thr_src, uint32_t* tri_slot, const RtRebuildWs& w, const RtPlocWs& pw, uint32_t max_leaf, void* stream);
