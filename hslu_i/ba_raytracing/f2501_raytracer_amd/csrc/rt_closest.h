// rt_closest.h -- closest-point queries (rt_closest_points*): for a point p, the point of the scene's SURFACE that is nearest
// to it, and how far away it is.  Embree's rtcPointQuery, Open3D's compute_closest_points.
//
// Everything here is compiled three times from this one text: into rt_closest_points_model (rt_closest.cpp: a linear scan
// of a scene description, the specification), into rt_closest_packed (rt_scene_pack.cpp: the kernel's walk over a packed
// blob, on the host) and into rt_closest_kernel (rt_closest.hip).  Every float result is ONE correctly rounded multiply, add,
// division or square root (rt_fmul, rt_fadd, rt_fdiv, rt_fsqrt of rt_refit.h; the library is built with -ffp-contract=off), so
// the three agree bit for bit.
//
// ---- the definition -----------------------------------------------------------------------------------------------------------
// Triangle {v1, e1, e2} (vertices v1, v1 + e1, v1 + e2), point p.  A = v1 - p comes first, so every later rounding is relative to
// distances from p, not to absolute coordinates.  Candidates, each a point of the triangle given as r = q - p:
//   the three edges   t = clamp(-(S.e) / (e.e), 0, 1), r = S + t e, for (S, e) = (A, e1), (A, e2), (A + e1, e2 - e1);
//                     e.e == 0 (two equal vertices) gives t = 0: the edge is its start point
//   the face          only when n.n is positive and finite, n = e1 x e2: u = ((e2 x A).n) / (n.n), v = ((A x e1).n) / (n.n), and
//                     only when u >= 0, v >= 0, u + v <= 1 as computed: r = A + u e1 + v e2
// The candidate of smallest r.r wins, in the order edge 1, edge 2, edge 3, face, a later one only when strictly smaller.  Every
// candidate IS a point of the triangle whatever the rounding of t, u, v did, so the result is never farther than the nearest
// edge point, a wrong inside test of a sliver's projection cannot lose the triangle, and no division has a zero denominator.
// A zero-area triangle (n.n == 0) is the union of its edges, that is its longest segment; three equal vertices are that point.
// q = p + r, barycentric weights (u, v) of e1 and e2: (t, 0), (0, t), (1 - t, t) on the edges.  distance = sqrt(r.r).
// This is a surface, not a solid: there is no sign.
// Inputs that give no finite distance: coordinates so far from p that A, or r.r, overflows fp32 (|v - p| above 1.8e19), and
// non-finite vertices.  The distance is then inf or NaN, and such a candidate never wins (rt_closest_offer).
//
// Sphere {c, r_sq}: r = sqrt(r_sq), w = p - c, l = sqrt(w.w); distance = | l - r |; q = c + w (r / l), normal = w / l; when l == 0
// (p == c, or closer than fp32 can square) the direction is (1, 0, 0).  Inside and outside are alike.  r_sq < 0: NaN, never wins.
//
// Key and tie rule.  One fp32 distance per object; the smaller wins, on EQUAL distance the LARGER canonical id (spheres first,
// then triangles in insertion order): the "later object wins" of rt_cast_rays.  A candidate counts only when distance <=
// max_distance (NaN or negative: nothing counts; absent: +inf) and is finite.  So the result is a function of the scene
// description and the point alone -- not of the tree, the slot order, or the order a walk meets candidates in.
// Dead queries: a point with a non-finite coordinate is a miss.  A miss: id -1, distance +inf, point, normal, bary 0, material
// 0xFFFFFFFF (as rt_ray_hits).
//
// ---- pruning ------------------------------------------------------------------------------------------------------------------
// rt_closest_box_d2 is the squared distance from p to a box, sum of squares of max(lo - p, 0, p - hi): three non-negative terms,
// each difference rounded once, so it is within 4 ulp (relative 5e-7) of the true D_box^2.  rt_closest_may_skip(box_d2, best) is
// true only when NO triangle under the box can win or tie against the distance `best`:
//   Every padded leaf box contains its triangle grown by a ball of pad >= 2e-5 + 1e-4 extent (rt_bvh.cpp; rt_grow_slot_box of
//   rt_refit.h term for term), and every box above contains its leaves' boxes.  So for a triangle T under the box with true
//   distance D_T from p: D_box <= max(0, D_T - pad).
//   The computed distance d_T differs from D_T by at most c eps (D_T + extent), eps = 2^-24, c < 40: A is off by eps |A| <=
//   eps (D_T + extent) per component, and the some twenty operations behind r.r and its root each add a relative eps of
//   quantities bounded by D_T + extent.  Hence d_T >= D_T (1 - c eps) - c eps extent >= (D_box + pad)(1 - c eps) - c eps extent
//   >= D_box (1 - c eps), because pad (1 - c eps) >= 1e-4 extent (1 - c eps) > c eps extent as long as c < 800.
//   The absolute part of the error is thus covered by the pad; what remains is relative: d_T^2 >= box_d2 (1 - 2 c eps - 5e-7)
//   > box_d2 / 1.0001.  The rule skips when box_d2 > 1.0001 best^2 (two rounded multiplies, relative 1.2e-7, inside the slack):
//   then d_T > best for every T below, which can neither win nor tie.  best = +inf, a NaN box or a NaN best never skip.
//   best^2 underflowing to 0 needs best < 1e-22, box_d2 > 0 then means D_box > 3e-23 > best.
// Split clipping needs no special case: the clipped references cover the triangle, so the reference whose (padded) box holds
// the closest point is never skipped, every reference evaluates the WHOLE triangle, and duplicates give equal results.
//
// Signed distance and inside tests are rt_solid.h (the meshes need not be closed: it says what an open one gets).  Out of scope:
// k nearest, a wave-cooperative walk for coherent point sets such as grids, an ordered variant.
// Not part of the public ABI.
#pragma once

#include "rt_refit.h"

// A loop of the walk goes on while ANY lane of the wavefront wants another turn (a wave vote, as walk_tris_lane's loops); the
// host runs one query at a time.
#if defined(__HIP_DEVICE_COMPILE__)
#define RT_CLOSEST_ANY(x) (__builtin_amdgcn_ballot_w64(x) != 0ull)
#else
#define RT_CLOSEST_ANY(x) (x)
#endif

// Kernel argument besides RtDevScene: the caller's batch and the output planes (device pointers, nullptr = not written).
struct RtClosestArgs {
  const float* point;         // [n][3]
  const float* max_distance;  // [n], nullptr = +inf
  int32_t* id;
  float* distance;
  float* out_point;           // [n][3]
  float* normal;              // [n][3]
  float* bary;                // [n][2]
  uint32_t* material;
  uint32_t n;
};

RT_HD static inline float rt_closest_dot(const float a[3], const float b[3]) {
  return rt_fadd(rt_fadd(rt_fmul(a[0], b[0]), rt_fmul(a[1], b[1])), rt_fmul(a[2], b[2]));
}
RT_HD static inline void rt_closest_cross(const float a[3], const float b[3], float c[3]) {
  c[0] = rt_fadd(rt_fmul(a[1], b[2]), -rt_fmul(a[2], b[1]));
  c[1] = rt_fadd(rt_fmul(a[2], b[0]), -rt_fmul(a[0], b[2]));
  c[2] = rt_fadd(rt_fmul(a[0], b[1]), -rt_fmul(a[1], b[0]));
}

// ---- one triangle ---------------------------------------------------------------------------------------------------------------
struct RtClosestTri {
  float r[3];  // q - p
  float u, v;  // weights of e1, e2
  float d2;    // r.r
};
// the nearest point of the segment S + t e, t in [0, 1], to the origin
RT_HD static inline float rt_closest_seg(const float S[3], const float e[3], float r[3], float* t_out) {
  const float ee = rt_closest_dot(e, e);
  float t = 0.0f;
  if (ee > 0.0f) t = rt_fdiv(-rt_closest_dot(S, e), ee);
  if (!(t > 0.0f)) t = 0.0f;  // (NaN included)
  if (t > 1.0f) t = 1.0f;
  for (int a = 0; a < 3; a++) r[a] = rt_fadd(S[a], rt_fmul(t, e[a]));
  *t_out = t;
  return rt_closest_dot(r, r);
}
RT_HD static inline void rt_closest_tri(const float v1[3], const float e1[3], const float e2[3], const float p[3], RtClosestTri& o) {
  float A[3], B[3], e3[3], r[3], t;
  for (int a = 0; a < 3; a++) A[a] = rt_fadd(v1[a], -p[a]), B[a] = rt_fadd(A[a], e1[a]), e3[a] = rt_fadd(e2[a], -e1[a]);
  o.d2 = rt_closest_seg(A, e1, o.r, &t);
  o.u = t, o.v = 0.0f;
  float d2 = rt_closest_seg(A, e2, r, &t);
  if (d2 < o.d2) {
    o.d2 = d2, o.u = 0.0f, o.v = t;
    for (int a = 0; a < 3; a++) o.r[a] = r[a];
  }
  d2 = rt_closest_seg(B, e3, r, &t);
  if (d2 < o.d2) {
    o.d2 = d2, o.u = rt_fadd(1.0f, -t), o.v = t;
    for (int a = 0; a < 3; a++) o.r[a] = r[a];
  }
  float n[3], x[3];
  rt_closest_cross(e1, e2, n);
  const float nn = rt_closest_dot(n, n);
  if (nn > 0.0f && nn < INFINITY) {
    rt_closest_cross(e2, A, x);
    const float u = rt_fdiv(rt_closest_dot(x, n), nn);
    rt_closest_cross(A, e1, x);
    const float v = rt_fdiv(rt_closest_dot(x, n), nn);
    if (u >= 0.0f && v >= 0.0f && rt_fadd(u, v) <= 1.0f) {
      for (int a = 0; a < 3; a++) r[a] = rt_fadd(rt_fadd(A[a], rt_fmul(u, e1[a])), rt_fmul(v, e2[a]));
      d2 = rt_closest_dot(r, r);
      if (d2 < o.d2) {
        o.d2 = d2, o.u = u, o.v = v;
        for (int a = 0; a < 3; a++) o.r[a] = r[a];
      }
    }
  }
}

// ---- one sphere -----------------------------------------------------------------------------------------------------------------
struct RtClosestSphere {
  float q[3], n[3], dist;
};
RT_HD static inline void rt_closest_sphere(const float c[3], float r_sq, const float p[3], RtClosestSphere& o) {
  float w[3];
  for (int a = 0; a < 3; a++) w[a] = rt_fadd(p[a], -c[a]);
  const float l = rt_fsqrt(rt_closest_dot(w, w)), r = rt_fsqrt(r_sq);
  o.dist = fabsf(rt_fadd(l, -r));
  if (l > 0.0f) {
    const float s = rt_fdiv(r, l);
    for (int a = 0; a < 3; a++) o.q[a] = rt_fadd(c[a], rt_fmul(w[a], s)), o.n[a] = rt_fdiv(w[a], l);
  } else {
    o.q[0] = rt_fadd(c[0], r), o.q[1] = c[1], o.q[2] = c[2];
    o.n[0] = 1.0f, o.n[1] = 0.0f, o.n[2] = 0.0f;
  }
}

// ---- the comparison ---------------------------------------------------------------------------------------------------------------
// the best candidate so far: starts as {max_distance, -1}, so that "counts" and "wins" are one comparison (a candidate AT
// max_distance ties with id -1 and wins)
struct RtClosestBest {
  float dist;
  int32_t id;
  uint32_t slot;  // a triangle's leaf slot (the model: its canonical index)
};
RT_HD static inline void rt_closest_offer(RtClosestBest& b, float dist, int32_t id, uint32_t slot) {
  if (rt_finite(dist) && (dist < b.dist || (dist == b.dist && id > b.id))) b.dist = dist, b.id = id, b.slot = slot;
}
// whether a query is looked up at all: finite coordinates, and a radius that can admit something
RT_HD static inline bool rt_closest_alive(const float p[3], float max_distance) {
  return rt_finite(p[0]) && rt_finite(p[1]) && rt_finite(p[2]) && max_distance >= 0.0f;
}

// ---- boxes ------------------------------------------------------------------------------------------------------------------------
// NaN for a box that is not lo <= hi on every axis (an absent child, the single root of rt_lbvh_single_root before its refit)
RT_HD static inline float rt_closest_box_d2(const float lo[3], const float hi[3], const float p[3]) {
  if (!(lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2])) return NAN;
  float s = 0.0f;
  for (int a = 0; a < 3; a++) {
    const float d = fmaxf(fmaxf(rt_fadd(lo[a], -p[a]), rt_fadd(p[a], -hi[a])), 0.0f);
    s = rt_fadd(s, rt_fmul(d, d));
  }
  return s;
}
RT_HD static inline bool rt_closest_may_skip(float box_d2, float best_distance) {
  return box_d2 > rt_fmul(rt_fmul(best_distance, best_distance), 1.0001f);
}

// ---- one result -------------------------------------------------------------------------------------------------------------------
struct RtClosestHit {
  int32_t id;
  float distance, point[3], normal[3], bary[2];
  uint32_t material;
};
RT_HD static inline void rt_closest_miss(RtClosestHit& h) {
  h.id = -1, h.distance = INFINITY, h.material = 0xFFFFFFFFu;
  for (int a = 0; a < 3; a++) h.point[a] = 0.0f, h.normal[a] = 0.0f;
  h.bary[0] = h.bary[1] = 0.0f;
}
RT_HD static inline void rt_closest_hit_sphere(const float c[3], float r_sq, uint32_t material, const float p[3], int32_t id, RtClosestHit& h) {
  RtClosestSphere s;
  rt_closest_sphere(c, r_sq, p, s);
  h.id = id, h.distance = s.dist, h.material = material;
  for (int a = 0; a < 3; a++) h.point[a] = s.q[a], h.normal[a] = s.n[a];
  h.bary[0] = h.bary[1] = 0.0f;
}
RT_HD static inline void rt_closest_hit_tri(const float v1[3], const float e1[3], const float e2[3], const float normal[3], uint32_t material,
                                            const float p[3], int32_t id, RtClosestHit& h) {
  RtClosestTri t;
  rt_closest_tri(v1, e1, e2, p, t);
  h.id = id, h.distance = rt_fsqrt(t.d2), h.material = material;
  for (int a = 0; a < 3; a++) h.point[a] = rt_fadd(p[a], t.r[a]), h.normal[a] = normal[a];
  h.bary[0] = t.u, h.bary[1] = t.v;
}

// ---- the walk over a packed scene: the kernel's, and rt_closest_packed's ------------------------------------------------------------
RT_HD static inline void rt_closest_offer_slot(const RtDevScene& sc, const char* base, uint32_t slot, const float p[3], RtClosestBest& best) {
  const float* q = (const float*)(base + sc.off_tri_isect) + 12u * (size_t)slot;
  const float v1[3] = {q[0], q[1], q[2]}, e1[3] = {q[3], q[4], q[5]}, e2[3] = {q[6], q[7], q[8]};
  RtClosestTri t;
  rt_closest_tri(v1, e1, e2, p, t);
  const uint32_t tri = ((const uint32_t*)(base + sc.off_tri_id))[slot] & RT_TRI_INDEX_MASK;
  rt_closest_offer(best, rt_fsqrt(t.d2), (int32_t)(sc.n_spheres + tri), slot);
}

// One query.  `have`: this lane has one (the host: true).  Three parts: the spheres; a seed, ONE root-to-leaf descent of the
// BVH2 into the nearer child box (child 0 on a tie; an absent child or a NaN box is never entered), which gives the fixed-order
// walk a near-final bound before it starts (at most 64 steps, no stack; measured against the walk alone it is 1.4 to 2 times
// faster on the text meshes, profiles/point_query.md); the stackless walk of the threaded tree, two loops in one as rt_resolve_walk: the
// inner one steps from box to box until the lane stands in a leaf it may not skip, the outer one evaluates ONE slot per turn,
// so that the lanes of a wavefront run the triangle routine side by side.  The walk needs its links to lead forward and ends
// early where one does not; no index read from memory is used unchecked.
RT_HD static inline void rt_closest_query(const RtDevScene& sc, const char* base, const float p[3], float max_distance, bool have, RtClosestHit& h) {
  const bool alive = have && rt_closest_alive(p, max_distance);
  RtClosestBest best;
  best.dist = max_distance, best.id = -1, best.slot = 0u;
  if (RT_CLOSEST_ANY(alive)) {
    const float* sph = (const float*)(base + sc.off_spheres);
    for (uint32_t k = 0; k < sc.n_spheres; k++) {
      RtClosestSphere s;
      rt_closest_sphere(sph + 4u * (size_t)k, sph[4u * (size_t)k + 3u], p, s);
      if (alive) rt_closest_offer(best, s.dist, (int32_t)k, k);
    }
  }
  if (sc.n_triangles && sc.n_slots) {
    if (sc.n_nodes) {
      const RtNode* nodes = (const RtNode*)(base + sc.off_nodes);
      uint32_t node = 0u, first = 0u, count = 0u;
      bool go = alive;
      for (int step = 0; step < 64 && RT_CLOSEST_ANY(go); step++) {
        if (go) {
          const RtNode nd = nodes[node];
          const float d0 = nd.c0 != RT_NODE_EMPTY ? rt_closest_box_d2(nd.lo0, nd.hi0, p) : NAN;
          const float d1 = nd.c1 != RT_NODE_EMPTY ? rt_closest_box_d2(nd.lo1, nd.hi1, p) : NAN;
          const bool h0 = d0 == d0, h1 = d1 == d1;  // (a NaN reads as absent)
          const bool second = !h0 || (h1 && d1 < d0);
          const uint32_t c = second ? nd.c1 : nd.c0, n = second ? nd.n1 : nd.n0;
          if (!h0 && !h1) go = false;
          else if (n) first = c, count = n, go = false;
          else if (c < sc.n_nodes) node = c;
          else go = false;
        }
      }
      for (uint32_t k = 0; RT_CLOSEST_ANY(k < count); k++)
        if (k < count && first + k < sc.n_slots) rt_closest_offer_slot(sc, base, first + k, p, best);
    }
    const RtThrNode* thr = (const RtThrNode*)(base + sc.off_nodes_thr);
    uint32_t node = alive ? 0u : sc.n_thr, first = 0u, k = 0u, n = 0u;  // slots first + k .. first + n - 1 of the lane's leaf are still to be evaluated
    for (;;) {
      while (RT_CLOSEST_ANY(k >= n && node < sc.n_thr)) {
        if (k >= n && node < sc.n_thr) {
          const RtThrNode t = thr[node];
          uint32_t next = t.skip;
          if (!rt_closest_may_skip(rt_closest_box_d2(t.lo, t.hi, p), best.dist)) {
            if ((t.leaf >> 24) == 0u) next = node + 1u;
            else first = t.leaf & 0xFFFFFFu, n = t.leaf >> 24, k = 0u;
          }
          node = next > node ? next : sc.n_thr;
        }
      }
      const bool todo = k < n;
      if (!RT_CLOSEST_ANY(todo)) break;
      if (todo) {
        const uint32_t slot = first + k;
        k++;
        if (slot < sc.n_slots) rt_closest_offer_slot(sc, base, slot, p, best);
      }
    }
  }
  rt_closest_miss(h);
  if (!alive || best.id < 0) return;
  if ((uint32_t)best.id < sc.n_spheres) {
    const float* s = (const float*)(base + sc.off_spheres) + 4u * (size_t)best.id;
    rt_closest_hit_sphere(s, s[3], ((const uint32_t*)(base + sc.off_sphere_mat))[best.id], p, best.id, h);
  } else {
    const float* q = (const float*)(base + sc.off_tri_isect) + 12u * (size_t)best.slot;
    const float* sh = (const float*)(base + sc.off_tri_shade) + 4u * (size_t)best.slot;
    const float v1[3] = {q[0], q[1], q[2]}, e1[3] = {q[3], q[4], q[5]}, e2[3] = {q[6], q[7], q[8]};
    uint32_t material;
    memcpy(&material, sh + 3, 4);
    rt_closest_hit_tri(v1, e1, e2, sh, material, p, best.id, h);
  }
}

// one result into the planes that were asked for
RT_HD static inline void rt_closest_store(const RtClosestArgs& a, size_t i, const RtClosestHit& h) {
  if (a.id) a.id[i] = h.id;
  if (a.distance) a.distance[i] = h.distance;
  if (a.out_point) a.out_point[3u * i] = h.point[0], a.out_point[3u * i + 1u] = h.point[1], a.out_point[3u * i + 2u] = h.point[2];
  if (a.normal) a.normal[3u * i] = h.normal[0], a.normal[3u * i + 1u] = h.normal[1], a.normal[3u * i + 2u] = h.normal[2];
  if (a.bary) a.bary[2u * i] = h.bary[0], a.bary[2u * i + 1u] = h.bary[1];
  if (a.material) a.material[i] = h.material;
}

// the kernel (rt_closest.hip); returns hipError_t as int.  The host model of its walk is rt_closest_packed (rt_scene_pack.h).
int rt_launch_closest(const RtDevScene& sc, const RtClosestArgs& a, void* stream);
