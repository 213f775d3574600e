// rt_occlusion.h -- ambient-occlusion queries (rt_ambient_occlusion*): for a surface point and its normal, which of S directions
// of the hemisphere above it are blocked within max_distance, how many are open, and the mean open direction (the bent normal).
// Embree's rtcOccluded over a hemisphere, Open3D's and trimesh's per-vertex occlusion bakes.
//
// Everything here is compiled three times from this one text, as rt_multihit.h is and with its primitives: into
// rt_ambient_occlusion_model (rt_occlusion.cpp: a linear scan of a scene description, the specification), into
// rt_occlusion_packed (rt_scene_pack.cpp: the kernel's walk over a packed blob, on the host) and into the kernels
// (rt_occlusion.hip).  Every float result is ONE correctly rounded operation (rt_fmul, rt_fadd, rt_fdiv, rt_fsqrt of rt_refit.h)
// or an fmaf where written, so the three agree bit for bit.
//
// ---- the definition ----------------------------------------------------------------------------------------------------------
// A batch: n points p with normals nrm_raw of any length, a table of n_table >= 1 directions in the LOCAL frame (z along the
// normal, any length), n_samples = S in 1 .. RT_OCC_SMAX, an optional plane first[n], and the scalars bias, max_distance, flags.
// Per point i:
//   normal   n = rt_mh_normalize(nrm_raw).  The point is DEAD if a coordinate of p is non-finite or n has a NaN.
//   frame    the branchless orthonormal basis of Duff et al. 2017 ("Building an Orthonormal Basis, Revisited"), in this order:
//              sg = copysignf(1, n.z)   a = rt_fdiv(-1, rt_fadd(sg, n.z))   b = rt_fmul(rt_fmul(n.x, n.y), a)
//              tx = (fmaf(rt_fmul(sg, rt_fmul(n.x, n.x)), a, 1), rt_fmul(sg, b), rt_fmul(-sg, n.x))
//              ty = (b, fmaf(rt_fmul(n.y, n.y), a, sg), -n.y)
//   origin   o[k] = fmaf(n[k], bias, p[k])
//   sample s takes table row ((uint64)first[i] + s) % n_table (first absent: 0) = l; the world direction is
//              w[k] = fmaf(l.x, tx[k], fmaf(l.y, ty[k], rt_fmul(l.z, n[k])))
//            and the ray is rt_mh_ray(o, w), which normalises as Ray::new_with_mask does and gives u, the unit direction.
//   OCCLUDED a sample is occluded if some object has a hit (rt_multihit.h: at most one per object) with t <= max_distance.  A NaN
//            or negative max_distance admits nothing, +inf is allowed.  With RT_OCCLUSION_PASS_TRANSMISSIVE objects whose
//            material is rt_mh_transmissive do not count.  No back-face culling.  A sample whose ray is dead (the row
//            normalises to NaN, o overflowed) counts as occluded: a ray that cannot be cast shows no open sky.
//   outputs  bits[i][(S + 31) / 32]: bit s % 32 of word s / 32 is set when sample s is occluded, unused high bits 0;
//            clear[i]: the samples that are not occluded; visibility[i] = rt_fdiv((float)clear, (float)S);
//            bent_normal[i]: over the clear samples the int32 sums of (int32)rintf(rt_fmul(u[k], 1048576.0f)) -- 2^-20 fixed
//            point, 256 samples stay below 2^29, and an integer sum does not depend on its order, as the opacity sums of
//            rt_any_intersection do not -- converted to float and normalised by rt_mh_normalize, or (0, 0, 0) when all three are 0.
//   A dead point: bits all set, clear 0, visibility 0, bent_normal 0 -- every one of its samples counts as occluded.
// The result is a function of the scene description and the batch alone -- not of the tree, the slot order, the duplicate
// references of split clipping, the lane mapping or the order a walk meets hits in: "some object has an admitted hit" has no order.
//
// ---- the walk --------------------------------------------------------------------------------------------------------------------
// An any-hit walk: spheres first, then the triangles -- RtMhDesc scans them, RtMhBlob walks the threaded tree as
// RtMhBlob::triangles does (two loops in one, wave votes, links that must lead forward, no index used unchecked), but a lane ends
// its walk at its FIRST admitted hit (node = n_thr, as a finished lane does elsewhere).  The box test is rt_mh_box_enter with the
// constant limit max_distance; its argument (rt_multihit.h, "pruning") needs nothing of the list: a box is skipped only when no
// triangle under it can be hit at t <= limit, so every admitted hit is met unless the walk has ended at another one.
//
// Not part of the public ABI.
#pragma once

#include "rt_multihit.h"

#define RT_OCC_SMAX 256u          // RT_MAX_OCCLUSION_SAMPLES of rt_hip.h
#define RT_OCC_FIXED 1048576.0f   // 2^20: the fixed point of the bent normal's sums

// Kernel argument besides RtDevScene: the caller's batch and output planes (device pointers, nullptr = absent).
struct RtOcclusionArgs {
  const float* point;       // [n][3]
  const float* normal;      // [n][3]
  const float* table;       // [n_table][3]
  const uint32_t* first;    // [n], nullptr = 0
  uint32_t* bits;           // [n][(S + 31) / 32]
  uint32_t* clear;          // [n]
  float* visibility;        // [n]
  float* bent_normal;       // [n][3]
  float bias, max_distance;
  uint32_t n, n_samples, n_table, pass;  // pass: RT_OCCLUSION_PASS_TRANSMISSIVE is set
};

// How the query reads that struct, as RtMhArgsRef / RtMhKernArgs of the multi-hit queries: the host reads the struct, the kernel
// reads each POINTER from the kernel-argument segment where it is used (RtOccKernArgs, rt_occlusion.hip).
#define RT_OCC_POINTERS(X)                                                                                                   \
  X(const float*, point) X(const float*, normal) X(const float*, table) X(const uint32_t*, first) X(uint32_t*, bits) X(uint32_t*, clear) \
  X(float*, visibility) X(float*, bent_normal)
struct RtOccArgsRef {
  const RtOcclusionArgs& a;
#define RT_OCC_X(type, name) \
  RT_HD type name() const { return a.name; }
  RT_OCC_POINTERS(RT_OCC_X)
#undef RT_OCC_X
  RT_HD float bias() const { return a.bias; }
  RT_HD float max_distance() const { return a.max_distance; }
  RT_HD uint32_t n_samples() const { return a.n_samples; }
  RT_HD uint32_t n_table() const { return a.n_table; }
  RT_HD bool pass() const { return a.pass != 0u; }
};

RT_HD static inline uint32_t rt_occ_words(uint32_t n_samples) { return (n_samples + 31u) / 32u; }

// ---- the point: normal, frame, origin ----------------------------------------------------------------------------------------------
struct RtOccPoint {
  float n[3], tx[3], ty[3], o[3];
  uint32_t row0;  // first[i] % n_table
  bool alive;
};
template <class Args>
RT_HD static inline void rt_occ_point(const Args& a, uint32_t i, bool have, RtOccPoint& P) {
  float p[3] = {0.0f, 0.0f, 0.0f}, nrm_raw[3] = {0.0f, 0.0f, 0.0f};
  uint32_t first = 0u;
  if (have) {
    const float *point = a.point(), *normal = a.normal();
    for (int k = 0; k < 3; k++) p[k] = point[3u * (size_t)i + k], nrm_raw[k] = normal[3u * (size_t)i + k];
    if (const uint32_t* f = a.first()) first = f[i];
  }
  rt_mh_normalize(nrm_raw, P.n);
  const float sg = copysignf(1.0f, P.n[2]);
  const float aa = rt_fdiv(-1.0f, rt_fadd(sg, P.n[2]));
  const float b = rt_fmul(rt_fmul(P.n[0], P.n[1]), aa);
  P.tx[0] = fmaf(rt_fmul(sg, rt_fmul(P.n[0], P.n[0])), aa, 1.0f), P.tx[1] = rt_fmul(sg, b), P.tx[2] = rt_fmul(-sg, P.n[0]);
  P.ty[0] = b, P.ty[1] = fmaf(rt_fmul(P.n[1], P.n[1]), aa, sg), P.ty[2] = -P.n[1];
  const float bias = a.bias();
  for (int k = 0; k < 3; k++) P.o[k] = fmaf(P.n[k], bias, p[k]);
  P.row0 = first % a.n_table();
  P.alive = have && rt_finite(p[0]) && rt_finite(p[1]) && rt_finite(p[2]) && P.n[0] == P.n[0] && P.n[1] == P.n[1] && P.n[2] == P.n[2];
}
// ((uint64)first + s) % n_table in 32 bits: row0 = first % n_table and s % n_table both lie below n_table, so their sum lies
// below 2 n_table and one subtraction reduces it; where the 32-bit sum wrapped (c < row0) the subtraction wraps back.
RT_HD static inline uint32_t rt_occ_row(uint32_t row0, uint32_t s, uint32_t n_table) {
  uint32_t c = row0 + s % n_table;
  if (c < row0 || c >= n_table) c -= n_table;
  return c;
}
// sample s of the point: its world direction (any length; rt_mh_ray normalises it)
RT_HD static inline void rt_occ_direction(const RtOccPoint& P, const float l[3], float w[3]) {
  for (int k = 0; k < 3; k++) w[k] = fmaf(l[0], P.tx[k], fmaf(l[1], P.ty[k], rt_fmul(l[2], P.n[k])));
}

// ---- any hit -------------------------------------------------------------------------------------------------------------------------
// a triangle of a description / a leaf slot of a blob: an admitted hit that counts
RT_HD static inline bool rt_occ_tri(const float v1[3], const float e1[3], const float e2[3], const RtMhRay& r, float max_d) {
  float t = 0.0f;
  return rt_mh_tri(v1, e1, e2, r, &t) && t <= max_d;
}
RT_HD static inline bool rt_occ_triangles(const RtMhDesc& S, const RtMhRay& r, float max_d, bool pass, bool walk) {
  const rt_scene_desc* d = S.d;
  if (!walk) return false;
  for (uint32_t t = 0; t < d->n_triangles; t++) {
    const size_t k = 3 * (size_t)t;
    if (rt_occ_tri(d->tri_v1 + k, d->tri_e1 + k, d->tri_e2 + k, r, max_d) && !(pass && S.transmissive(d->tri_material[t]))) return true;
  }
  return false;
}
RT_HD static inline bool rt_occ_slot(const RtMhBlob& S, const RtMhRay& r, float max_d, bool pass, uint32_t slot) {
  const float* q = S.at<float>(S.sc.off_tri_isect + 48u * slot);
  const float v1[3] = {q[0], q[1], q[2]}, e1[3] = {q[3], q[4], q[5]}, e2[3] = {q[6], q[7], q[8]};
  bool h = rt_occ_tri(v1, e1, e2, r, max_d);
  if (pass && h) {
    uint32_t material;
    memcpy(&material, S.at<float>(S.sc.off_tri_shade + 16u * slot) + 3, 4);
    h = !S.transmissive(material);
  }
  return h;
}
// RtMhBlob::triangles with an end at the first hit
RT_HD static inline bool rt_occ_triangles(const RtMhBlob& S, const RtMhRay& r, float max_d, bool pass, bool walk) {
  const RtDevScene& sc = S.sc;
  if (!(sc.n_triangles && sc.n_slots)) return false;
  bool hit = false;
  uint32_t node = walk ? 0u : sc.n_thr, first = 0u, k = 0u, n = 0u;  // slots first + k .. first + n - 1 of the lane's leaf are still to be evaluated
  for (;;) {
    while (RT_MH_ANY(k >= n && node < sc.n_thr)) {
      if (k >= n && node < sc.n_thr) {
        const RtThrNode t = *S.at<RtThrNode>(sc.off_nodes_thr + 32u * node);
        uint32_t next = t.skip;
        if (rt_mh_box_enter(t.lo, t.hi, r, max_d)) {
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
      if (slot < sc.n_slots && rt_occ_slot(S, r, max_d, pass, slot)) hit = true, node = sc.n_thr, k = 0u, n = 0u;  // the first hit settles it
    }
  }
  return hit;
}
// whether some object of the scene has an admitted hit that counts; `walk`: this lane asks
template <class Scene>
RT_HD static inline bool rt_occ_any(const Scene& S, const RtMhRay& r, float max_d, bool pass, bool walk) {
  bool hit = false;
  for (uint32_t k = 0; k < S.n_spheres(); k++) {
    if (!RT_MH_ANY(walk && !hit)) break;
    float c[3], r_sq, t = 0.0f;
    uint32_t material;
    S.sphere(k, c, &r_sq, &material);
    const bool h = rt_mh_sphere(c, r_sq, r, &t) && t <= max_d;
    if (walk && h && !(pass && S.transmissive(material))) hit = true;
  }
  return rt_occ_triangles(S, r, max_d, pass, walk && !hit) || hit;
}

// ---- one sample ------------------------------------------------------------------------------------------------------------------------
// Sample s of point P.  `have`: this lane has one (the host: true).  -> occluded; q: the sample's share of the bent normal's
// sums, 0 where it is occluded.
template <class Scene, class Args>
RT_HD static inline bool rt_occ_sample(const Scene& S, const Args& a, const RtOccPoint& P, uint32_t s, bool have, int32_t q[3]) {
  float l[3] = {0.0f, 0.0f, 0.0f}, w[3];
  if (have) {
    const float* row = a.table() + 3u * (size_t)rt_occ_row(P.row0, s, a.n_table());
    l[0] = row[0], l[1] = row[1], l[2] = row[2];
  }
  rt_occ_direction(P, l, w);
  RtMhRay r;
  const bool alive = rt_mh_ray(P.o, w, r) && P.alive;
  const float max_d = a.max_distance();
  // (a NaN or negative max_distance admits nothing: such a ray does not walk)
  const bool hit = rt_occ_any(S, r, max_d, a.pass(), have && alive && max_d >= 0.0f);
  const bool occluded = !alive || hit;
  for (int k = 0; k < 3; k++) q[k] = 0;
  if (have && !occluded)
    for (int k = 0; k < 3; k++) q[k] = (int32_t)rintf(rt_fmul(r.d[k], RT_OCC_FIXED));
  return occluded;
}

// ---- one point's planes ------------------------------------------------------------------------------------------------------------------
// what follows from the reductions (the bit words are written where they are made)
template <class Args>
RT_HD static inline void rt_occ_store(const Args& a, uint32_t i, uint32_t clear, const int32_t sum[3]) {
  if (uint32_t* out = a.clear()) out[i] = clear;
  if (float* out = a.visibility()) out[i] = rt_fdiv((float)clear, (float)a.n_samples());
  if (float* out = a.bent_normal()) {
    float b[3] = {0.0f, 0.0f, 0.0f};
    if (sum[0] | sum[1] | sum[2]) {
      const float f[3] = {(float)sum[0], (float)sum[1], (float)sum[2]};
      rt_mh_normalize(f, b);
    }
    out[3u * (size_t)i] = b[0], out[3u * (size_t)i + 1u] = b[1], out[3u * (size_t)i + 2u] = b[2];
  }
}
// Point i, one sample after the other: the model and the kernel's host twin.  (The kernel puts samples into lanes and reduces
// them by ballot, popcount and cross-lane adds: rt_occlusion.hip.)
template <class Scene, class Args>
static inline void rt_occ_query_host(const Scene& S, const Args& a, uint32_t i) {
  RtOccPoint P;
  rt_occ_point(a, i, true, P);
  const uint32_t n_samples = a.n_samples(), words = rt_occ_words(n_samples);
  uint32_t word[RT_OCC_SMAX / 32u] = {0u}, clear = 0u;
  int32_t sum[3] = {0, 0, 0};
  for (uint32_t s = 0; s < n_samples; s++) {
    int32_t q[3];
    if (rt_occ_sample(S, a, P, s, true, q)) word[s / 32u] |= 1u << (s % 32u);
    else clear++;
    for (int k = 0; k < 3; k++) sum[k] += q[k];
  }
  if (uint32_t* out = a.bits())
    for (uint32_t w = 0; w < words; w++) out[(size_t)i * words + w] = word[w];
  rt_occ_store(a, i, clear, sum);
}

// the kernels (rt_occlusion.hip); returns hipError_t as int.  The host model of their walk is rt_occlusion_packed (rt_scene_pack.h).
int rt_launch_occlusion(const RtDevScene& sc, const RtOcclusionArgs& a, void* stream);
