// rt_solid.h -- containment and signed-distance queries (rt_contains_points*, rt_signed_distance*): whether a point lies inside
// the closed surfaces of the scene, and how deep.  trimesh's contains / signed_distance, Open3D's occupancy and SDF grids.
//
// Everything here is compiled three times from this one text, as rt_closest.h, rt_multihit.h and rt_occlusion.h are and with
// the primitives of rt_multihit.h: into rt_contains_points_model / rt_signed_distance_model (rt_solid.cpp: a linear scan of a
// scene description, the specification), into rt_solid_packed (rt_scene_pack.cpp: the kernel's walk over a packed blob, on the
// host) and into rt_solid_kernel (rt_solid.hip).  Every float result is ONE correctly rounded operation (rt_fmul, rt_fadd,
// rt_fdiv, rt_fsqrt of rt_refit.h) or an fmaf where written, so the three agree bit for bit.
//
// ---- the definition ----------------------------------------------------------------------------------------------------------
// A batch: n points p, a table of R directions (1 <= R <= RT_SOLID_RMAX, any length; a row that rt_mh_ray cannot normalise to
// finite components is refused before the query runs) and a rule, RT_SOLID_PARITY or RT_SOLID_WINDING.
// Per point p and direction r the ray is rt_mh_ray(p, dir_r): no bias, no max_distance.  A CROSSING is a triangle whose literal
// test rt_mh_tri accepts that ray (t > eps, u >= 0, v >= 0, u + v < 1, |det| > eps): the hits of rt_list_intersections, without
// culling, transmissive objects included.
//   crossings[i][r]  the number of distinct triangles crossed
//   winding[i][r]    the sum over the crossings of the sign of rt_mh_dot(d, stored normal): positive = the ray LEAVES through
//                    the triangle, +1; negative = it ENTERS, -1; zero or NaN counts 0.  The orientation is the stored normal's,
//                    as the reference's culling uses it, never the vertex order's (the built-in slabs are not consistently wound)
//   spheres          are decided analytically, not by rays: sphere k contains p when rt_mh_sphere_cc(v, r_sq) < 0 with v = p - c
//                    as rt_mh_sphere forms it -- the condition under which that test takes the origin for inside.  A NaN or
//                    negative r_sq never contains.  k_s = the number of containing spheres
//   the vote of r    parity: (crossings + k_s) & 1;  winding: winding + k_s > 0
// Per point: votes[i] = the directions voting inside; inside[i] = 2 votes > R (R odd is recommended, a tie at an even R is
// outside).  votes not in {0, R} means the directions DISAGREE: the point lies on or near a surface (a ray through an edge or a
// vertex of a closed mesh may count it twice or not at all), or the surface is open or inconsistently oriented there.  That
// disagreement is the diagnostic an open mesh gets instead of a refusal: the letters of the built-in text scenes are open
// surfaces, and the points whose rays pass through a missing face show up as non-unanimous.
// The two rules differ where solids OVERLAP: in the intersection of two slabs every ray leaves two surfaces, so parity says
// outside and winding says inside (winding = 2).
// Dead points: a point with a non-finite coordinate gets inside 0, votes 0, crossings 0, winding 0.
// The result is a function of the scene description and the batch alone -- not of the tree, the slot order or the order a walk
// meets crossings in: a count and an integer sum have no order.
//
// Signed distance: rt_closest_points' result for the point, unchanged bit for bit (the kernel of rt_closest.hip runs first, this
// one reads its `distance` plane), and signed_distance = inside ? -distance : distance, so a miss is +inf or -inf.  The
// max_distance plane applies to the closest-point search only.
//
// ---- split-clipped trees -------------------------------------------------------------------------------------------------------
// Every reference of a split-clipped triangle evaluates the WHOLE triangle, so a counting walk would count a crossing once per
// reference it reaches, and a box-pruned walk cannot know which reference is the only one.  Such trees (rt_bvh_tuning.split_depth
// > 0; off by default) are refused with RT_ERR_UNSUPPORTED (rt_check_solid, rt_scene_pack.cpp), as rt_scene_update and
// rt_scene_rebuild refuse them.  There is no dedup rule.
//
// ---- the walk --------------------------------------------------------------------------------------------------------------------
// The stackless walk of RtMhBlob::triangles -- two loops in one, wave votes, links that must lead forward, no index read from
// memory used unchecked -- that COUNTS instead of keeping a list or stopping.  The box test is rt_mh_box_enter with the constant
// limit +inf; its argument (rt_multihit.h, "pruning") needs nothing of a list: a box is skipped only when no triangle under it can
// be hit at t <= limit, so every crossing is met, and without duplicate references it is met once.
//
// Out of scope: generalized winding numbers, a watertight triangle test (the crossings are deliberately rt_list_intersections'
// hits), split-clipped trees, per-object containment ids, a skip-transmissive flag, wave-cooperative walks.
// Not part of the public ABI.
#pragma once

#include "rt_multihit.h"

#define RT_SOLID_RMAX 8u     // RT_MAX_SOLID_DIRECTIONS of rt_hip.h
#define RT_SOLID_PARITY 0u   // RT_SOLID_RULE_PARITY
#define RT_SOLID_WINDING 1u  // RT_SOLID_RULE_WINDING

// Kernel argument besides RtDevScene: the caller's batch and output planes (device pointers, nullptr = absent), and the
// direction table BY VALUE: it is small and wave-uniform, so it travels in the kernel-argument segment.
struct RtSolidArgs {
  const float* point;      // [n][3]
  const float* distance;   // [n] rt_closest_points' distance plane (the signed-distance calls), nullptr = none
  uint8_t* inside;         // [n]
  uint8_t* votes;          // [n]
  uint32_t* crossings;     // [n][R]
  int32_t* winding;        // [n][R]
  float* signed_distance;  // [n]; may be `distance` itself: a lane reads its element before it writes it
  float dir[RT_SOLID_RMAX][3];
  uint32_t n, n_dirs, rule;
};

// How the query reads that struct, as RtMhArgsRef / RtMhKernArgs of the multi-hit queries: the host reads the struct, the kernel
// reads each POINTER and each direction from the kernel-argument segment where it is used (RtSolidKernArgs, rt_solid.hip).
#define RT_SOLID_POINTERS(X)                                                                                                         \
  X(const float*, point) X(const float*, distance) X(uint8_t*, inside) X(uint8_t*, votes) X(uint32_t*, crossings) X(int32_t*, winding) \
  X(float*, signed_distance)
struct RtSolidArgsRef {
  const RtSolidArgs& a;
#define RT_SOLID_X(type, name) \
  RT_HD type name() const { return a.name; }
  RT_SOLID_POINTERS(RT_SOLID_X)
#undef RT_SOLID_X
  RT_HD float dir(uint32_t r, int k) const { return a.dir[r][k]; }
  RT_HD uint32_t n_dirs() const { return a.n_dirs; }
  RT_HD uint32_t rule() const { return a.rule; }
};

// a table row the query accepts: rt_mh_ray normalises it to finite components (the origin plays no part in that) that are not
// all zero (a row whose squared length overflows normalises to (0, 0, 0))
RT_HD static inline bool rt_solid_direction_ok(const float d_raw[3]) {
  const float o[3] = {0.0f, 0.0f, 0.0f};
  RtMhRay r;
  return rt_mh_ray(o, d_raw, r) && rt_finite(r.d[0]) && rt_finite(r.d[1]) && rt_finite(r.d[2]) && (r.d[0] != 0.0f || r.d[1] != 0.0f || r.d[2] != 0.0f);
}

// ---- the crossings of one ray -------------------------------------------------------------------------------------------------------
struct RtSolidCount {
  uint32_t crossings;
  int32_t winding;
};
// a crossed triangle's share of the winding sum
RT_HD static inline int32_t rt_solid_sign(const RtMhRay& r, const float normal[3]) {
  const float s = rt_mh_dot(r.d, normal);
  return s > 0.0f ? 1 : (s < 0.0f ? -1 : 0);
}
// a description's triangles, one after the other.  `walk`: this lane asks; `wind`: the winding sum is wanted
RT_HD static inline void rt_solid_triangles(const RtMhDesc& S, const RtMhRay& r, bool walk, bool wind, RtSolidCount& c) {
  const rt_scene_desc* d = S.d;
  if (!walk) return;
  for (uint32_t t = 0; t < d->n_triangles; t++) {
    const size_t k = 3 * (size_t)t;
    float tt = 0.0f;
    if (!rt_mh_tri(d->tri_v1 + k, d->tri_e1 + k, d->tri_e2 + k, r, &tt)) continue;
    c.crossings++;
    if (wind) c.winding += rt_solid_sign(r, d->tri_normal + k);
  }
}
// a leaf slot of a blob
RT_HD static inline void rt_solid_slot(const RtMhBlob& S, const RtMhRay& r, bool wind, uint32_t slot, RtSolidCount& c) {
  const float* q = S.at<float>(S.sc.off_tri_isect + 48u * slot);
  const float v1[3] = {q[0], q[1], q[2]}, e1[3] = {q[3], q[4], q[5]}, e2[3] = {q[6], q[7], q[8]};
  float tt = 0.0f;
  if (!rt_mh_tri(v1, e1, e2, r, &tt)) return;
  c.crossings++;
  if (wind) {
    const float* sh = S.at<float>(S.sc.off_tri_shade + 16u * slot);
    const float nrm[3] = {sh[0], sh[1], sh[2]};
    c.winding += rt_solid_sign(r, nrm);
  }
}
// RtMhBlob::triangles with a count in place of the list, at the constant limit +inf
RT_HD static inline void rt_solid_triangles(const RtMhBlob& S, const RtMhRay& r, bool walk, bool wind, RtSolidCount& c) {
  const RtDevScene& sc = S.sc;
  if (!(sc.n_triangles && sc.n_slots)) return;
  uint32_t node = walk ? 0u : sc.n_thr, first = 0u, k = 0u, n = 0u;  // slots first + k .. first + n - 1 of the lane's leaf are still to be evaluated
  for (;;) {
    while (RT_MH_ANY(k >= n && node < sc.n_thr)) {
      if (k >= n && node < sc.n_thr) {
        const RtThrNode t = *S.at<RtThrNode>(sc.off_nodes_thr + 32u * node);
        uint32_t next = t.skip;
        if (rt_mh_box_enter(t.lo, t.hi, r, INFINITY)) {
          if ((t.leaf >> 24) == 0u) next = node + 1u;
          else first = t.leaf & 0xFFFFFFu, n = t.leaf >> 24, k = 0u;
        }
        node = next > node ? next : sc.n_thr;
      }
    }
    const bool todo = k < n;
    if (!RT_MH_ANY(todo)) break;
    if (todo) {
      const uint32_t slot = first + k;
      k++;
      if (slot < sc.n_slots) rt_solid_slot(S, r, wind, slot, c);
    }
  }
}

// ---- one point ---------------------------------------------------------------------------------------------------------------------
// Point i of the batch.  `have`: this lane has one (the host: true).  The spheres once, then the directions in a loop that is
// uniform over the wavefront; the rows of crossings and winding are written as their direction finishes, the point's record
// at the end.
template <class Scene, class Args>
RT_HD static inline void rt_solid_query(const Scene& S, const Args& a, uint32_t i, bool have) {
  float p[3] = {0.0f, 0.0f, 0.0f};
  if (have) {
    const float* point = a.point();
    for (int k = 0; k < 3; k++) p[k] = point[3u * (size_t)i + k];
  }
  const bool alive = have && rt_finite(p[0]) && rt_finite(p[1]) && rt_finite(p[2]);
  uint32_t k_s = 0u;
  if (RT_MH_ANY(alive)) {
    for (uint32_t k = 0; k < S.n_spheres(); k++) {
      float c[3], r_sq, v[3];
      uint32_t material;
      S.sphere(k, c, &r_sq, &material);
      rt_mh_sphere_v(c, p, v);
      if (alive && rt_mh_sphere_cc(v, r_sq) < 0.0f) k_s++;
    }
  }
  const uint32_t n_dirs = a.n_dirs();
  const bool by_winding = a.rule() == RT_SOLID_WINDING;
  const bool wind = by_winding || a.winding() != nullptr;
  uint32_t votes = 0u;
  for (uint32_t r = 0; r < n_dirs; r++) {
    const float d_raw[3] = {a.dir(r, 0), a.dir(r, 1), a.dir(r, 2)};
    RtMhRay ray;
    const bool walk = rt_mh_ray(p, d_raw, ray) && alive;
    RtSolidCount c = {0u, 0};
    rt_solid_triangles(S, ray, walk, wind, c);
    const bool vote = by_winding ? ((int64_t)c.winding + (int64_t)k_s > 0) : (((c.crossings + k_s) & 1u) != 0u);
    if (vote) votes++;
    if (have) {
      if (uint32_t* out = a.crossings()) out[(size_t)i * n_dirs + r] = c.crossings;
      if (int32_t* out = a.winding()) out[(size_t)i * n_dirs + r] = c.winding;
    }
  }
  if (!have) return;
  const bool inside = 2u * votes > n_dirs;
  if (uint8_t* out = a.inside()) out[i] = inside ? 1 : 0;
  if (uint8_t* out = a.votes()) out[i] = (uint8_t)votes;
  if (float* out = a.signed_distance()) {
    const float dist = a.distance()[i];
    out[i] = inside ? -dist : dist;
  }
}

// the kernel (rt_solid.hip); returns hipError_t as int.  The host model of its walk is rt_solid_packed (rt_scene_pack.h).
int rt_launch_solid(const RtDevScene& sc, const RtSolidArgs& a, void* stream);
