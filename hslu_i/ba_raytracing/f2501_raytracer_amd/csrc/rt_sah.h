// rt_sah.h -- the arithmetic of the SAH report (rt_scene_bvh_quality): the surface-area-heuristic cost of the tree as it
// stands, in fp64 with contraction off, summed as 64-bit INTEGERS so that any summation order gives the same two numbers.
//
// Compiled twice, as rt_refit.h is: rt_sah_packed (rt_scene_pack.cpp) loops over the nodes on the host, rt_sah_kernel
// (rt_sah.hip) runs one thread per node.
//   half_area(lo, hi) = dx dy + dy dz + dz dx,  dx = (double)hi[0] - (double)lo[0], dy and dz likewise; left to right
//   A_root            = half_area of the union (rt_min_keep / rt_max_keep) of the root's present child boxes
//   for every node and every present child (c != RT_NODE_EMPTY):
//     ratio = half_area(child box) / A_root; a ratio that is NaN, negative or above 1 counts in n_bad and adds nothing
//     q = (uint64_t)(ratio 2^30), truncated;  inner_q += q for an inner child (n == 0),  leaf_q += q n for a leaf of n slots
//   sah = (inner_q + tri_cost leaf_q) / 2^30 as doubles on the host
// Bound: q <= 2^30, n < 2^8 per leaf, fewer than 2^24 nodes and slots: both sums stay below 2^30 2^8 2^24 < 2^63.
// Not part of the public ABI.
#pragma once

#include "rt_refit.h"

#define RT_SAH_WG 256u
#define RT_SAH_ONE 1073741824.0  // 2^30

RT_HD static inline double rt_sah_half_area(const float lo[3], const float hi[3]) {
#pragma clang fp contract(off)
  const double dx = (double)hi[0] - (double)lo[0], dy = (double)hi[1] - (double)lo[1], dz = (double)hi[2] - (double)lo[2];
  return dx * dy + dy * dz + dz * dx;
}

RT_HD static inline double rt_sah_root_area(const RtNode& root) {
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int a = 0; a < 3; a++) {
    if (root.c0 != RT_NODE_EMPTY) lo[a] = rt_min_keep(lo[a], root.lo0[a]), hi[a] = rt_max_keep(hi[a], root.hi0[a]);
    if (root.c1 != RT_NODE_EMPTY) lo[a] = rt_min_keep(lo[a], root.lo1[a]), hi[a] = rt_max_keep(hi[a], root.hi1[a]);
  }
  return rt_sah_half_area(lo, hi);
}

// what node `nd` adds: sums[0] += inner_q, sums[1] += leaf_q, *n_bad += refused ratios
RT_HD static inline void rt_sah_node(const RtNode& nd, double a_root, uint64_t sums[2], uint32_t* n_bad) {
#pragma clang fp contract(off)
  for (int k = 0; k < 2; k++) {
    const uint32_t c = k ? nd.c1 : nd.c0, n = k ? nd.n1 : nd.n0;
    if (c == RT_NODE_EMPTY) continue;
    const double ratio = rt_sah_half_area(k ? nd.lo1 : nd.lo0, k ? nd.hi1 : nd.hi0) / a_root;
    if (!(ratio >= 0.0 && ratio <= 1.0)) {  // (NaN fails both)
      *n_bad += 1u;
      continue;
    }
    const uint64_t q = (uint64_t)(ratio * RT_SAH_ONE);
    if (n) sums[1] += q * n;
    else sums[0] += q;
  }
}

// rt_sah.hip: clears out[0..3) = {inner_q, leaf_q, n_bad} (device, 64-bit words) and enqueues rt_sah_kernel; hipError_t as int
int rt_launch_sah(const RtNode* nodes_dev, uint32_t n_nodes, unsigned long long* out_dev, void* stream);
