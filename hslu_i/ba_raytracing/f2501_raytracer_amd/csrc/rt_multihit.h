// rt_multihit.h -- multi-hit ray queries (rt_list_intersections*): for a ray, the first K objects it passes through, in order, and
// how many it passes through in all.  Open3D's list_intersections / count_intersections, Embree's multi-hit, trimesh's
// multiple_hits.
//
// Everything here is compiled three times from this one text: into rt_list_intersections_model (rt_multihit.cpp: a linear scan of
// a scene description, the specification), into rt_multihit_packed (rt_scene_pack.cpp: the kernel's walk over a packed blob, on
// the host) and into rt_multihit_kernel (rt_multihit.hip).  Every float result is ONE correctly rounded multiply, add, division
// or square root (rt_fmul, rt_fadd, rt_fdiv, rt_fsqrt of rt_refit.h), or an fmaf where the reference writes mul_add: in every dot
// product (ultraviolet's Vec3::dot), in the sphere's discriminant and in Ray::at.  So the three agree bit for bit, and with
// oracle/rt_oracle.c, whose sphere_intersect and triangle_intersect are restated here operation for operation.
//
// ---- the definition ----------------------------------------------------------------------------------------------------------
// A ray is an origin, a direction of any length (normalised as Ray::new_with_mask does: d * (1 / |d|)) and a max_distance
// (absent: +inf).  A HIT is what the reference's `intersect` returns for ONE object, so there is at most one per object:
//   sphere    the root SphereData::intersect picks (sphere.rs:78-162): the smaller non-negative one -- a ray from outside gets the
//             entry point only, a ray from inside the exit point
//   triangle  the literal matrix-inverse test (triangle.rs:149-212) with its t > eps, u >= 0, v >= 0, u + v < 1 and |det| > eps
// With culling, sphere.rs:137-151 / triangle.rs:154-168 apply as in rt_cast_rays: a hit on a material that is not transmissive
// counts only where dot(d, normal) < 0.75.
// A hit is ADMITTED when t <= max_distance as computed (a NaN t never is; a NaN or negative max_distance admits nothing) and
// when it lies strictly after the cursor, if there is one.
// The KEY of a hit is (t, id): t ascending, on equal t the LARGER canonical id first -- the "later object wins" of rt_cast_rays,
// so entry 0 of a list without a cursor is rt_cast_rays' answer.  A cursor (after_t, after_id) admits only keys strictly after
// it: t > after_t, or t == after_t and id < after_id; a NaN after_t admits nothing.  Feeding the last returned key back pages
// through all hits without an epsilon and without losing or repeating coincident hits.
// Output for max_hits = K: the first `count` <= K admitted hits in key order; `total` = the number of distinct objects with an
// admitted hit (count == min(total, K)).  Entries from `count` on hold the miss values of rt_ray_hits.  Dead rays (a direction
// that normalises to NaN, a non-finite origin: deviation D2) give count 0, total 0.
// The result is a function of the scene description and the ray alone -- not of the tree, the slot order, the duplicate
// references of split clipping or the order a walk meets hits in.
//
// ---- the list ------------------------------------------------------------------------------------------------------------------
// RtMhLane holds the K smallest admitted keys met so far, sorted.  rt_mh_offer ignores a key whose id the list holds: every
// reference of a split-clipped triangle evaluates the WHOLE triangle and gives the same t, so a duplicate is the same key.  (A
// duplicate of a key that was pushed out of a full list lies after the list's last key and is not inserted either.)  The insert
// is a compare-exchange chain over statically indexed entries, without a branch: on the device the list stays in registers.
// `total` by paging inside the call: while a pass ends with a full list, the lane sets its cursor to the list's last key, walks
// again and adds what it finds.  Each pass strictly advances the key, so there are at most n_objects / K + 1 passes; a ray with
// fewer than K hits costs one walk, and without `total` there is one pass.  The planes are written after the first pass.
//
// ---- pruning -------------------------------------------------------------------------------------------------------------------
// rt_mh_box_enter is the slab test of the per-lane walks (walk_tris_lane): entry tn = max over the axes of the nearer plane
// distance, exit tm = min of the farther one; the box is entered when tn <= min(S(tm), S(limit)) and S(tm) >= 0, with the slack
// S(x) = x + 1e-5 + 4e-6 |x|.  `limit` is max_distance until the list is full, then the t of its K-th entry.  A box is skipped
// only when NO triangle under it can yield an admitted key at t <= limit; a hit AT the limit is never cut, which is what keeps
// ties (which the id decides) independent of the walk:
//   Space.  The literal triangle test accepts a ray at computed t only where the exact point o + t d lies within its own
//   rounding of the triangle.  For origins in or near the scene that overreach is inside the pad of every leaf box, 2e-5 + 1e-4
//   of the triangle's extent + 4 ulp of its coordinates (rt_bvh.cpp; rt_grow_slot_box of rt_refit.h term for term), and every
//   box above contains its leaves' boxes.  The overreach grows with |v1 - o| (a few ulp of it, over the cosine of incidence), so
//   every box is widened here by far_pad = 8e-6 (|ox| + |oy| + |oz|) on every side, about 70 ulp of the origin's magnitude, as
//   rt_query.h does for rt_cast_rays (rays from 100 extents away are part of the tests).  Hence for an accepted hit the exact
//   point lies in the widened box of its leaf and of every ancestor, and the exact slab distances satisfy Tn <= t <= Tm.
//   The test's own rounding.  A plane distance is ((plane -+ far_pad) - o) * inv: two rounded differences, absolute error below
//   2^-23 (|plane| + |o|), less than 1/16 of the 4 ulp + 70 ulp the pads hold for it; inv = 1 / d is correctly rounded and the
//   product rounds once, relative 2^-23 together.  So tn <= Tn (1 + 2^-22) + tiny and tm >= Tm (1 - 2^-22) - tiny, far inside
//   S: 4e-6 relative is 16 times 2^-22, and 1e-5 absolute covers distances near zero (t > eps for triangles).  With Tn <= t <= Tm
//   and t <= limit that gives tn <= S(tm), tn <= S(limit) and S(tm) >= 0: the box is entered.
//   Zero direction components: inv is clamped to +-1e30 (no inf, so no 0 * inf), a plane difference of exactly 0 gives distance 0
//   and every other one +-huge with the right sign, which is the slab's "inside or not" for that axis.  A box that is not
//   lo <= hi on every axis (an absent child's NaN box) is never entered.
// The reciprocals are correctly rounded so that the host twin takes the kernel's decisions; the results would be equal without.
// Split clipping needs no special case: the clipped references cover the triangle, the reference whose widened box holds the
// hit point is reached, and it evaluates the whole triangle.
//
// Inside / occupancy tests and signed distance are rt_solid.h (a sphere gives ONE hit, so crossing parity has a definition of
// its own there).  Out of scope: both roots of a sphere; K above RT_MAX_HITS_PER_RAY; an ordered or wave-cooperative variant for
// coherent rays; a phase-1 prefilter like tri_hit's.
// Not part of the public ABI.
#pragma once

#include "rt_refit.h"

// A loop of the walk goes on while ANY lane of the wavefront wants another turn (a wave vote, as walk_tris_lane's loops and
// rt_closest.h's); the host runs one ray at a time.
#if defined(__HIP_DEVICE_COMPILE__)
#define RT_MH_ANY(x) (__builtin_amdgcn_ballot_w64(x) != 0ull)
#else
#define RT_MH_ANY(x) (x)
#endif

#define RT_MH_KMAX 16  // RT_MAX_HITS_PER_RAY of rt_hip.h
#define RT_MH_EPS 1.1920929e-7f  // f32::EPSILON (float_ext.rs:44-45)

// Kernel argument besides RtDevScene: the caller's batch, request and output planes (device pointers, nullptr = absent).
struct RtMultiHitArgs {
  const float* origin;        // [n][3]
  const float* direction;     // [n][3]
  const float* max_distance;  // [n], nullptr = +inf
  const float* after_t;       // [n] cursor, nullptr (both) = none
  const int32_t* after_id;    // [n]
  uint32_t* count;            // [n]
  uint32_t* total;            // [n]
  int32_t* id;                // [n][max_hits]
  float* t;                   // [n][max_hits]
  float* point;               // [n][max_hits][3]
  float* normal;              // [n][max_hits][3]
  uint32_t* material;         // [n][max_hits]
  uint32_t n, max_hits, cull;
};

// How the query reads that struct: A.origin(), A.count(), ...  The host reads the struct (RtMhArgsRef).  The kernel has an
// accessor of its own (RtMhKernArgs, rt_multihit.hip) that reads each POINTER from the kernel-argument segment where it is
// used: twelve pointers and the flags "is it null" would otherwise sit in scalar registers across the whole walk, on top of
// the scene's, and the kernel would spill them.
#define RT_MH_POINTERS(X)                                                                                                      \
  X(const float*, origin) X(const float*, direction) X(const float*, max_distance) X(const float*, after_t) X(const int32_t*, after_id) \
  X(uint32_t*, count) X(uint32_t*, total) X(int32_t*, id) X(float*, t) X(float*, point) X(float*, normal) X(uint32_t*, material)
struct RtMhArgsRef {
  const RtMultiHitArgs& a;
#define RT_MH_X(type, name) \
  RT_HD type name() const { return a.name; }
  RT_MH_POINTERS(RT_MH_X)
#undef RT_MH_X
  RT_HD uint32_t max_hits() const { return a.max_hits; }
  RT_HD bool cull() const { return a.cull != 0u; }
};

// ---- vectors: ultraviolet's, as oracle/rt_oracle.c restates them -------------------------------------------------------------------
RT_HD static inline float rt_mh_dot(const float a[3], const float b[3]) { return fmaf(a[0], b[0], fmaf(a[1], b[1], rt_fmul(a[2], b[2]))); }
RT_HD static inline void rt_mh_cross(const float a[3], const float b[3], float c[3]) {
  c[0] = rt_fadd(rt_fmul(a[1], b[2]), rt_fmul(-a[2], b[1]));
  c[1] = rt_fadd(rt_fmul(a[2], b[0]), rt_fmul(-a[0], b[2]));
  c[2] = rt_fadd(rt_fmul(a[0], b[1]), rt_fmul(-a[1], b[0]));
}
RT_HD static inline void rt_mh_normalize(const float a[3], float n[3]) {
  const float r = rt_fdiv(1.0f, rt_fsqrt(rt_mh_dot(a, a)));
  for (int k = 0; k < 3; k++) n[k] = rt_fmul(a[k], r);
}
// Ray::at (ray.rs:60-66)
RT_HD static inline void rt_mh_at(const float o[3], const float d[3], float t, float p[3]) {
  for (int k = 0; k < 3; k++) p[k] = fmaf(d[k], t, o[k]);
}
// TransmissionProperties::mask (material.rs:44-50) of a row that holds has_opacity and opacity
RT_HD static inline bool rt_mh_transmissive(float has_opacity, float opacity) { return has_opacity != 0.0f && !(fabsf(opacity) <= RT_MH_EPS); }

// ---- the ray ---------------------------------------------------------------------------------------------------------------------
struct RtMhRay {
  float o[3], d[3];  // d normalised
  float inv[3], pad; // slab test: clamped reciprocals, far_pad
};
// false for a dead ray
RT_HD static inline bool rt_mh_ray(const float o[3], const float d_raw[3], RtMhRay& r) {
  rt_mh_normalize(d_raw, r.d);
  for (int k = 0; k < 3; k++) {
    r.o[k] = o[k];
    r.inv[k] = fminf(fmaxf(rt_fdiv(1.0f, r.d[k]), -1e30f), 1e30f);
  }
  r.pad = rt_fmul(8e-6f, rt_fadd(rt_fadd(fabsf(o[0]), fabsf(o[1])), fabsf(o[2])));
  return rt_finite(o[0]) && rt_finite(o[1]) && rt_finite(o[2]) && r.d[0] == r.d[0] && r.d[1] == r.d[1] && r.d[2] == r.d[2];
}

// ---- the intersection tests --------------------------------------------------------------------------------------------------------
// The two quantities of SphereData::intersect that do not depend on the direction: v = o - c and cc = v.v - r_sq.  cc < 0 exactly
// where the test sees the origin INSIDE the sphere (its one hit is then the exit point): rt_solid.h decides containment with it.
RT_HD static inline void rt_mh_sphere_v(const float c[3], const float o[3], float v[3]) {
  for (int k = 0; k < 3; k++) v[k] = rt_fadd(o[k], -c[k]);
}
RT_HD static inline float rt_mh_sphere_cc(const float v[3], float r_sq) { return rt_fadd(rt_mh_dot(v, v), -r_sq); }
// SphereData::intersect (sphere.rs:78-162) up to the choice of the root
RT_HD static inline bool rt_mh_sphere(const float c[3], float r_sq, const RtMhRay& r, float* t_out) {
  float v[3];
  rt_mh_sphere_v(c, r.o, v);
  const float b = rt_fmul(2.0f, rt_mh_dot(r.d, v));
  const float cc = rt_mh_sphere_cc(v, r_sq);
  const float disc = fmaf(b, b, rt_fmul(-4.0f, cc));
  const float sq = rt_fsqrt(disc);
  const float mba = rt_fmul(-b, 0.5f), sa = rt_fmul(sq, 0.5f);
  const float t0 = rt_fadd(mba, -sa), t1 = rt_fadd(mba, sa);
  const bool t0v = t0 >= 0.0f, t1v = t1 >= 0.0f;
  const bool use0 = t0v && (!t1v || t0 < t1);
  const bool use1 = t1v && !use0;
  *t_out = use0 ? t0 : t1;
  return disc >= 0.0f && (use0 || use1);
}
// sphere.rs:137-151: whether a hit at t on a material that is not transmissive faces the ray enough to count
RT_HD static inline bool rt_mh_sphere_faces(const float c[3], const RtMhRay& r, float t) {
  float p[3], n[3];
  rt_mh_at(r.o, r.d, t, p);
  for (int k = 0; k < 3; k++) p[k] = rt_fadd(p[k], -c[k]);
  rt_mh_normalize(p, n);
  return rt_mh_dot(r.d, n) < 0.75f;
}
// TriangleData::intersect (triangle.rs:169-212; ultraviolet Mat3::inversed / determinant) without the culling
RT_HD static inline bool rt_mh_tri(const float v1[3], const float e1[3], const float e2[3], const RtMhRay& r, float* t_out) {
  float b[3], c1[3], c2[3], x[3], y[3], z[3];
  for (int k = 0; k < 3; k++) b[k] = rt_fadd(v1[k], -r.o[k]), c1[k] = -e1[k], c2[k] = -e2[k];
  const float* c0 = r.d;
  rt_mh_cross(c1, c2, x);
  rt_mh_cross(c2, c0, y);
  rt_mh_cross(c0, c1, z);
  const float inv_det = rt_fdiv(1.0f, rt_mh_dot(c0, x));
  float t = 0.0f, u = 0.0f, v = 0.0f;
  {
    const float r0[3] = {rt_fmul(x[0], inv_det), rt_fmul(x[1], inv_det), rt_fmul(x[2], inv_det)};
    const float r1[3] = {rt_fmul(y[0], inv_det), rt_fmul(y[1], inv_det), rt_fmul(y[2], inv_det)};
    const float r2[3] = {rt_fmul(z[0], inv_det), rt_fmul(z[1], inv_det), rt_fmul(z[2], inv_det)};
    t = rt_fadd(rt_fadd(rt_fmul(r0[0], b[0]), rt_fmul(r0[1], b[1])), rt_fmul(r0[2], b[2]));
    u = rt_fadd(rt_fadd(rt_fmul(r1[0], b[0]), rt_fmul(r1[1], b[1])), rt_fmul(r1[2], b[2]));
    v = rt_fadd(rt_fadd(rt_fmul(r2[0], b[0]), rt_fmul(r2[1], b[1])), rt_fmul(r2[2], b[2]));
  }
  const float m0 = rt_fadd(rt_fmul(c1[1], c2[2]), -rt_fmul(c2[1], c1[2]));
  const float m1 = rt_fadd(rt_fmul(c0[1], c2[2]), -rt_fmul(c2[1], c0[2]));
  const float m2 = rt_fadd(rt_fmul(c0[1], c1[2]), -rt_fmul(c1[1], c0[2]));
  const float det = rt_fadd(rt_fadd(rt_fmul(c0[0], m0), -rt_fmul(c1[0], m1)), rt_fmul(c2[0], m2));
  const bool t_invalid = t <= RT_MH_EPS;
  const bool uv_invalid = (u < 0.0f) || (v < 0.0f) || (rt_fadd(u, v) >= 1.0f);
  *t_out = t;
  return !(t_invalid || uv_invalid) && !(fabsf(det) <= RT_MH_EPS);
}

// ---- one lane: the ray, the request and the list -----------------------------------------------------------------------------------
// The list always holds KMAX keys in ascending order, so that every entry is indexed statically and the insert needs no case
// for a short list: the first KMAX - k entries are FRONT keys (-inf, INT32_MAX), before which no hit ever sorts (t is never
// -inf: t >= 0 for spheres, t > eps for triangles), the other k start as EMPTY keys (+inf, -1), behind which every hit sorts (a
// hit at t = +inf has an id > -1).  A new key is carried through the entries and exchanged wherever it sorts first; what falls
// off the end was the largest.  So the last entry is the k-th smallest key met, or EMPTY while fewer than k were met.
template <int KMAX>
struct RtMhLane {
  RtMhRay r;
  float max_d;
  bool cur_on;  // a cursor applies
  float cur_t;
  int32_t cur_id;
  uint32_t k;  // max_hits, 1 .. KMAX
  bool cull;
  bool walk;  // this lane takes part in the pass
  float t[KMAX];
  int32_t id[KMAX];
  uint32_t n;  // hits held, <= k
};
template <int KMAX>
RT_HD static inline void rt_mh_reset(RtMhLane<KMAX>& L) {
#pragma unroll
  for (int j = 0; j < KMAX; j++) L.t[j] = INFINITY, L.id[j] = -1;
#pragma nounroll
  for (uint32_t s = L.k; s < (uint32_t)KMAX; s++) {  // KMAX - k front keys, shifted in (no entry is indexed by a variable)
#pragma unroll
    for (int e = KMAX - 1; e > 0; e--) L.t[e] = L.t[e - 1], L.id[e] = L.id[e - 1];
    L.t[0] = -INFINITY, L.id[0] = 0x7FFFFFFF;
  }
  L.n = 0u;
}
// what the walk prunes with: max_distance until the list is full, then its last t (an EMPTY last entry is +inf)
template <int KMAX>
RT_HD static inline float rt_mh_limit(const RtMhLane<KMAX>& L) {
  return fminf(L.max_d, L.t[KMAX - 1]);
}
// the cursor test
RT_HD static inline bool rt_mh_after(bool cur_on, float cur_t, int32_t cur_id, float t, int32_t id) {
  return !cur_on | (t > cur_t) | ((t == cur_t) & (id < cur_id));
}
// The sorted insert of an object's hit (`hit`: the test accepted it).  Straight-line code over statically indexed entries (the
// bool operators are the bitwise ones, so that nothing short-circuits into a branch); skipped as a whole, by a vote, where no
// lane of the wavefront has a key to insert.
template <int KMAX>
RT_HD static inline void rt_mh_offer(RtMhLane<KMAX>& L, float t, int32_t id, bool hit) {
  bool ins = hit & (t <= L.max_d) & rt_mh_after(L.cur_on, L.cur_t, L.cur_id, t, id);
  if (!RT_MH_ANY(ins)) return;
#pragma unroll
  for (int j = 0; j < KMAX; j++) ins = ins & (L.id[j] != id);
  float ct = t;
  int32_t cid = id;
#pragma unroll
  for (int j = 0; j < KMAX; j++) {
    const float st = L.t[j];
    const int32_t sid = L.id[j];
    const bool place = ins & ((ct < st) | ((ct == st) & (cid > sid)));
    L.t[j] = place ? ct : st, L.id[j] = place ? cid : sid;
    ct = place ? st : ct, cid = place ? sid : cid;
  }
  L.n += (ins & (L.n < L.k)) ? 1u : 0u;
}

// ---- boxes ---------------------------------------------------------------------------------------------------------------------------
RT_HD static inline float rt_mh_slack(float x) { return rt_fadd(rt_fadd(x, 1e-5f), rt_fmul(fabsf(x), 4e-6f)); }
RT_HD static inline bool rt_mh_box_enter(const float lo[3], const float hi[3], const RtMhRay& r, float limit) {
  if (!(lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2])) return false;
  float tn = -INFINITY, tm = INFINITY;
  for (int a = 0; a < 3; a++) {
    const float t1 = rt_fmul(rt_fadd(rt_fadd(lo[a], -r.pad), -r.o[a]), r.inv[a]);
    const float t2 = rt_fmul(rt_fadd(rt_fadd(hi[a], r.pad), -r.o[a]), r.inv[a]);
    tn = fmaxf(tn, fminf(t1, t2)), tm = fminf(tm, fmaxf(t1, t2));
  }
  const float s = rt_mh_slack(tm);
  return tn <= fminf(s, rt_mh_slack(limit)) && s >= 0.0f;
}

// ---- where the objects come from -------------------------------------------------------------------------------------------------------
// A scene as the query sees it: sphere(k), material_transmissive(row), tri_record(tri) for the planes, objects(), and
// triangles(L): every triangle hit of a pass into the list.  RtMhDesc scans a description (the model); RtMhBlob walks a packed
// blob (the kernel and its host twin).
template <int KMAX>
RT_HD static inline void rt_mh_offer_tri(RtMhLane<KMAX>& L, const float v1[3], const float e1[3], const float e2[3], bool faces_or_passes, int32_t id,
                                         bool on) {
  float t = 0.0f;
  const bool h = rt_mh_tri(v1, e1, e2, L.r, &t);
  rt_mh_offer(L, t, id, on && h && faces_or_passes);
}

struct RtMhDesc {
  const rt_scene_desc* d;
  RT_HD uint32_t n_spheres() const { return d->n_spheres; }
  RT_HD uint64_t objects() const { return (uint64_t)d->n_spheres + d->n_triangles; }
  RT_HD bool bounded() const { return false; }  // the model pages without a limit
  RT_HD void sphere(uint32_t k, float c[3], float* r_sq, uint32_t* material) const {
    for (int a = 0; a < 3; a++) c[a] = d->sphere_center[3 * (size_t)k + a];
    *r_sq = d->sphere_r_sq[k], *material = d->sphere_material[k];
  }
  RT_HD bool transmissive(uint32_t material) const {
    const float* row = d->materials + (size_t)material * RT_MATERIAL_STRIDE;
    return rt_mh_transmissive(row[RT_MAT_HAS_OPACITY], row[RT_MAT_OPACITY]);
  }
  RT_HD void tri_record(uint32_t tri, float normal[3], uint32_t* material) const {
    for (int a = 0; a < 3; a++) normal[a] = d->tri_normal[3 * (size_t)tri + a];
    *material = d->tri_material[tri];
  }
  template <int KMAX>
  RT_HD void triangles(RtMhLane<KMAX>& L) const {
    if (!L.walk) return;
    for (uint32_t t = 0; t < d->n_triangles; t++) {
      const size_t k = 3 * (size_t)t;
      bool ok = true;
      if (L.cull) ok = rt_mh_dot(L.r.d, d->tri_normal + k) < 0.75f || transmissive(d->tri_material[t]);  // triangle.rs:154-168
      rt_mh_offer_tri(L, d->tri_v1 + k, d->tri_e1 + k, d->tri_e2 + k, ok, (int32_t)(d->n_spheres + t), true);
    }
  }
};

struct RtMhBlob {
  const RtDevScene& sc;
  const char* base;
  // a record at a 32-bit byte offset into the blob (which stays below 4 GiB, rt_blob_layout), as the kernels of rt_kernels.hip
  // address it: one 64-bit base for every section
  template <class T>
  RT_HD const T* at(uint32_t byte_offset) const {
    return (const T*)(base + byte_offset);
  }
  RT_HD uint32_t n_spheres() const { return sc.n_spheres; }
  RT_HD uint64_t objects() const { return (uint64_t)sc.n_spheres + sc.n_triangles; }
  RT_HD bool bounded() const { return true; }
  RT_HD void sphere(uint32_t k, float c[3], float* r_sq, uint32_t* material) const {
    const float* s = at<float>(sc.off_spheres + 16u * k);
    c[0] = s[0], c[1] = s[1], c[2] = s[2], *r_sq = s[3];
    *material = *at<uint32_t>(sc.off_sphere_mat + 4u * k);
  }
  RT_HD bool transmissive(uint32_t material) const {
    const float* row = at<float>(sc.off_materials + 48u * material);
    return rt_mh_transmissive(row[8], row[6]);
  }
  // the canonical shading record of a triangle (behind the n_slots records in leaf order)
  RT_HD void tri_record(uint32_t tri, float normal[3], uint32_t* material) const {
    const float* sh = at<float>(sc.off_tri_shade + 16u * (sc.n_slots + tri));
    normal[0] = sh[0], normal[1] = sh[1], normal[2] = sh[2];
    memcpy(material, sh + 3, 4);
  }
  template <int KMAX>
  RT_HD void offer_slot(RtMhLane<KMAX>& L, uint32_t slot) const {
    const float* q = at<float>(sc.off_tri_isect + 48u * slot);
    const float v1[3] = {q[0], q[1], q[2]}, e1[3] = {q[3], q[4], q[5]}, e2[3] = {q[6], q[7], q[8]};
    bool ok = true;
    if (L.cull) {  // triangle.rs:154-168
      const float* sh = at<float>(sc.off_tri_shade + 16u * slot);
      const float nrm[3] = {sh[0], sh[1], sh[2]};
      uint32_t material;
      memcpy(&material, sh + 3, 4);
      ok = rt_mh_dot(L.r.d, nrm) < 0.75f || transmissive(material);
    }
    const uint32_t tri = *at<uint32_t>(sc.off_tri_id + 4u * slot) & RT_TRI_INDEX_MASK;
    rt_mh_offer_tri(L, v1, e1, e2, ok, (int32_t)(sc.n_spheres + tri), true);
  }
  // The stackless walk of the threaded tree, two loops in one as rt_closest_query's: the inner one steps from box to box until
  // the lane stands in a leaf it may not skip, the outer one evaluates ONE slot per turn, so that the lanes of a wavefront run the
  // triangle test side by side.  The walk needs its links to lead forward and ends early where one does not; no index read from
  // memory is used unchecked.
  template <int KMAX>
  RT_HD void triangles(RtMhLane<KMAX>& L) const {
    if (!(sc.n_triangles && sc.n_slots)) return;
    uint32_t node = L.walk ? 0u : sc.n_thr, first = 0u, k = 0u, n = 0u;  // slots first + k .. first + n - 1 of the lane's leaf are still to be evaluated
    for (;;) {
      while (RT_MH_ANY(k >= n && node < sc.n_thr)) {
        if (k >= n && node < sc.n_thr) {
          const RtThrNode t = *at<RtThrNode>(sc.off_nodes_thr + 32u * node);
          uint32_t next = t.skip;
          if (rt_mh_box_enter(t.lo, t.hi, L.r, rt_mh_limit(L))) {
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
        if (slot < sc.n_slots) offer_slot(L, slot);
      }
    }
  }
};

// ---- one ray ---------------------------------------------------------------------------------------------------------------------------
// the planes of ray i after the first pass: `count` entries in key order, then the miss values.  The loop is uniform (max_hits);
// the list is read at entry 0 and shifted down, so that no entry is indexed by a variable.  The list is used up by this.
template <int KMAX, class Scene, class Args>
RT_HD static inline void rt_mh_store(const Scene& S, const Args& a, uint32_t i, RtMhLane<KMAX>& L, bool have) {
  if (!have) return;
  const uint32_t count = L.n, k = a.max_hits();
  if (uint32_t* out = a.count()) out[i] = count;
  int32_t* out_id = a.id();
  float *out_t = a.t(), *out_point = a.point(), *out_normal = a.normal();
  uint32_t* out_material = a.material();
  if (!(out_id || out_t || out_point || out_normal || out_material)) return;
  const bool records = out_normal || out_material;
#pragma nounroll
  for (uint32_t s = k; s < (uint32_t)KMAX; s++) {  // the front keys go first
#pragma unroll
    for (int e = 0; e + 1 < KMAX; e++) L.t[e] = L.t[e + 1], L.id[e] = L.id[e + 1];
  }
#pragma nounroll
  for (uint32_t j = 0; j < k; j++) {
    const bool valid = j < count;
    const int32_t id = valid ? L.id[0] : -1;
    const float t = valid ? L.t[0] : INFINITY;
    float p[3] = {0.0f, 0.0f, 0.0f}, nrm[3] = {0.0f, 0.0f, 0.0f};
    uint32_t material = 0xFFFFFFFFu;
    if (valid) {
      rt_mh_at(L.r.o, L.r.d, t, p);
      if (records) {
        if ((uint32_t)id < S.n_spheres()) {
          float c[3], r_sq, w[3];
          S.sphere((uint32_t)id, c, &r_sq, &material);
          for (int x = 0; x < 3; x++) w[x] = rt_fadd(p[x], -c[x]);
          rt_mh_normalize(w, nrm);
        } else {
          S.tri_record((uint32_t)id - S.n_spheres(), nrm, &material);
        }
      }
    }
    const size_t at = (size_t)i * k + j;
    if (out_id) out_id[at] = id;
    if (out_t) out_t[at] = t;
    if (out_point) out_point[3u * at] = p[0], out_point[3u * at + 1u] = p[1], out_point[3u * at + 2u] = p[2];
    if (out_normal) out_normal[3u * at] = nrm[0], out_normal[3u * at + 1u] = nrm[1], out_normal[3u * at + 2u] = nrm[2];
    if (out_material) out_material[at] = material;
#pragma unroll
    for (int e = 0; e + 1 < KMAX; e++) L.t[e] = L.t[e + 1], L.id[e] = L.id[e + 1];
  }
}

// Ray i of the batch.  `have`: this lane has one (the host: true).  A pass: the spheres in index order, then the scene's
// triangles; the planes after the first pass; further passes, each behind the last key of the one before, only while `total` is
// asked for and some lane's list came back full.
template <int KMAX, class Scene, class Args>
RT_HD static inline void rt_mh_query(const Scene& S, const Args& a, uint32_t i, bool have) {
  RtMhLane<KMAX> L;
  float o[3] = {0.0f, 0.0f, 0.0f}, d_raw[3] = {0.0f, 0.0f, 0.0f};
  L.max_d = INFINITY, L.cur_on = false, L.cur_t = 0.0f, L.cur_id = 0;
  L.k = a.max_hits(), L.cull = a.cull();
  if (have) {
    const float *origin = a.origin(), *direction = a.direction();
    for (int k = 0; k < 3; k++) o[k] = origin[3u * (size_t)i + k], d_raw[k] = direction[3u * (size_t)i + k];
    if (const float* m = a.max_distance()) L.max_d = m[i];
    if (const float* at = a.after_t()) L.cur_on = true, L.cur_t = at[i], L.cur_id = a.after_id()[i];
  }
  const bool alive = rt_mh_ray(o, d_raw, L.r);
  // (a NaN or negative max_distance and a NaN cursor admit nothing: such a ray does not walk)
  L.walk = have && alive && L.max_d >= 0.0f && !(L.cur_on && L.cur_t != L.cur_t);
  uint32_t total = 0u;
  const bool want_total = a.total() != nullptr;
  const uint32_t pass_bound = S.bounded() ? (uint32_t)S.objects() / L.k + 1u : 0u;  // (bounded: a blob holds fewer than 2^32 objects)
  for (uint32_t pass = 0;; pass++) {
    rt_mh_reset(L);
    if (RT_MH_ANY(L.walk)) {
      for (uint32_t k = 0; k < S.n_spheres(); k++) {
        float c[3], r_sq, t = 0.0f;
        uint32_t material;
        S.sphere(k, c, &r_sq, &material);
        bool h = rt_mh_sphere(c, r_sq, L.r, &t);
        if (L.cull) h = h && (rt_mh_sphere_faces(c, L.r, t) || S.transmissive(material));  // sphere.rs:137-151
        rt_mh_offer(L, t, (int32_t)k, L.walk && h);
      }
      S.triangles(L);
    }
    total += L.n;
    // the next pass starts behind this one's last key
    L.walk = L.walk && want_total && L.n == L.k && (!S.bounded() || pass + 1u < pass_bound);
    L.cur_on = L.cur_on || L.walk;
    if (L.walk) L.cur_t = L.t[KMAX - 1], L.cur_id = L.id[KMAX - 1];
    if (pass == 0) rt_mh_store(S, a, i, L, have);
    if (!RT_MH_ANY(L.walk)) break;
  }
  if (have && want_total) a.total()[i] = total;
}

// the kernel (rt_multihit.hip); returns hipError_t as int.  The host model of its walk is rt_multihit_packed (rt_scene_pack.h).
int rt_launch_multihit(const RtDevScene& sc, const RtMultiHitArgs& a, void* stream);
