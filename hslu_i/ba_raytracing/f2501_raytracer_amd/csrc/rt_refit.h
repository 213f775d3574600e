// rt_refit.h -- the arithmetic of an in-place scene update (rt_scene_update*), one function per record kind.
//
// Every function here rewrites ONE record of a packed scene (the blob of rt_scene_pack.cpp) from new object values.  They
// are compiled twice: rt_refit_packed (rt_scene_pack.cpp) calls them in loops on the host, and each kernel of rt_update.hip
// is one of them with a thread index.  So the host model IS the kernels' code, and what it is checked against on the CPU
// -- a fresh rt_pack_scene of the updated description -- holds for the device up to the exactness of its float operations:
// single multiplies, adds, divisions and square roots are the correctly rounded intrinsics there, never fused.
// Not part of the public ABI.
#pragma once

#include <math.h>
#include <string.h>

#include "rt_internal.h"

#if defined(__HIPCC__)
#define RT_HD __host__ __device__
#else
#define RT_HD
#endif

// ---- single operations: one rounding each, on either side ---------------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
RT_HD static inline float rt_fmul(float a, float b) { return __fmul_rn(a, b); }
RT_HD static inline float rt_fadd(float a, float b) { return __fadd_rn(a, b); }
RT_HD static inline float rt_fdiv(float a, float b) { return __fdiv_rn(a, b); }
RT_HD static inline float rt_fsqrt(float a) { return __builtin_sqrtf(a); }  // (hipcc lowers this to its correctly rounded sequence; __fsqrt_rn is the 1-ulp v_sqrt_f32)
#else
// volatile: no host-side contraction into an fma, whatever the flags (as in rt_scene_pack.cpp)
static inline float rt_fmul(float a, float b) { volatile float r = a * b; return r; }
static inline float rt_fadd(float a, float b) { volatile float r = a + b; return r; }
static inline float rt_fdiv(float a, float b) { volatile float r = a / b; return r; }
static inline float rt_fsqrt(float a) { return sqrtf(a); }
#endif
// std::min(a, b) / std::max(a, b) of rt_bvh.cpp, NaN behaviour included: a NaN `b` never replaces `a`
RT_HD static inline float rt_min_keep(float a, float b) { return b < a ? b : a; }
RT_HD static inline float rt_max_keep(float a, float b) { return a < b ? b : a; }
RT_HD static inline bool rt_finite(float x) { return fabsf(x) < INFINITY; }  // false for NaN

// the triangle range of a delta: canonical triangles [first, first + count) take element t - first of each array
struct RtTriDelta {
  uint32_t first, count;
  const float *v1, *e1, *e2, *normal;
};

RT_HD static inline float* rt_blob_f(char* base, uint32_t off) { return (float*)(base + off); }
RT_HD static inline uint32_t* rt_blob_u(char* base, uint32_t off) { return (uint32_t*)(base + off); }

// ---- geometry records ------------------------------------------------------------------------------------------------------
// leaf slot: {v1, e1, e2, X} (pack_isect_records: X from six separately rounded products) and the normal of its shading record
RT_HD static inline bool rt_upd_slot(const RtDevScene& sc, char* base, uint32_t slot, const RtTriDelta& d) {
  const uint32_t t = rt_blob_u(base, sc.off_tri_id)[slot] & RT_TRI_INDEX_MASK;
  if (t < d.first || t - d.first >= d.count) return false;
  const size_t k = 3 * (size_t)(t - d.first);
  const float v1[3] = {d.v1[k], d.v1[k + 1], d.v1[k + 2]}, e1[3] = {d.e1[k], d.e1[k + 1], d.e1[k + 2]};
  const float e2[3] = {d.e2[k], d.e2[k + 1], d.e2[k + 2]};
  const float a0 = rt_fmul(e1[1], e2[2]), b0 = rt_fmul(e1[2], e2[1]);
  const float a1 = rt_fmul(e1[2], e2[0]), b1 = rt_fmul(e1[0], e2[2]);
  const float a2 = rt_fmul(e1[0], e2[1]), b2 = rt_fmul(e1[1], e2[0]);
  float* q = rt_blob_f(base, sc.off_tri_isect) + 12 * (size_t)slot;
  q[0] = v1[0], q[1] = v1[1], q[2] = v1[2], q[3] = e1[0];
  q[4] = e1[1], q[5] = e1[2], q[6] = e2[0], q[7] = e2[1];
  q[8] = e2[2], q[9] = rt_fadd(a0, -b0), q[10] = rt_fadd(a1, -b1), q[11] = rt_fadd(a2, -b2);
  float* sh = rt_blob_f(base, sc.off_tri_shade) + 4 * (size_t)slot;  // (word 3, the material row, stays)
  sh[0] = d.normal[k], sh[1] = d.normal[k + 1], sh[2] = d.normal[k + 2];
  return true;
}

// canonical triangle d.first + k: the normal of its canonical shading record and the input of rt_flags_kernel (`geo`, null
// when the scene has no receiver cells; its R and first-cell words stay)
RT_HD static inline void rt_upd_tri(const RtDevScene& sc, char* base, float* geo, uint32_t k, const RtTriDelta& d) {
  const size_t t = (size_t)d.first + k, s = 3 * (size_t)k;
  float* sh = rt_blob_f(base, sc.off_tri_shade) + 4 * ((size_t)sc.n_slots + t);
  sh[0] = d.normal[s], sh[1] = d.normal[s + 1], sh[2] = d.normal[s + 2];
  if (!geo) return;
  float* g = geo + 12 * t;
  g[0] = d.v1[s], g[1] = d.v1[s + 1], g[2] = d.v1[s + 2];
  g[4] = d.e1[s], g[5] = d.e1[s + 1], g[6] = d.e1[s + 2];
  g[8] = d.e2[s], g[9] = d.e2[s + 1], g[10] = d.e2[s + 2];
}

// ---- boxes -----------------------------------------------------------------------------------------------------------------
// the padded box of the triangle in leaf slot `slot`, grown into (lo, hi): rt_build_bvh's box and pad, term for term
RT_HD static inline void rt_grow_slot_box(const RtDevScene& sc, const char* base, uint32_t slot, float lo[3], float hi[3]) {
  const float* q = (const float*)(base + sc.off_tri_isect) + 12 * (size_t)slot;
  float blo[3], bhi[3], ext = 0.f, mag = 0.f;
  for (int a = 0; a < 3; a++) {
    const float p0 = q[a], p1 = rt_fadd(p0, q[3 + a]), p2 = rt_fadd(p0, q[6 + a]);
    float l = INFINITY, h = -INFINITY;
    l = rt_min_keep(l, p0), h = rt_max_keep(h, p0);
    l = rt_min_keep(l, p1), h = rt_max_keep(h, p1);
    l = rt_min_keep(l, p2), h = rt_max_keep(h, p2);
    blo[a] = l, bhi[a] = h;
    ext = rt_max_keep(ext, rt_fadd(h, -l));
    mag = rt_max_keep(mag, rt_max_keep(fabsf(l), fabsf(h)));
  }
  const float pad = rt_fadd(rt_fadd(2e-5f, rt_fmul(1e-4f, ext)), rt_fmul(4.0f * 1.1920929e-7f, mag));
  for (int a = 0; a < 3; a++) {
    lo[a] = rt_min_keep(lo[a], rt_fadd(blo[a], -pad));
    hi[a] = rt_max_keep(hi[a], rt_fadd(bhi[a], pad));
  }
}

// Both child boxes of node `i`: a leaf's is the union of its slots' padded triangle boxes, an inner child's the union of
// that node's child boxes -- which are final when the nodes are visited by height (RtRefitPlan).  Absent children keep
// their NaN boxes.
RT_HD static inline void rt_upd_node(const RtDevScene& sc, char* base, uint32_t i) {
  RtNode* nodes = (RtNode*)(base + sc.off_nodes);
  RtNode& nd = nodes[i];
  for (int k = 0; k < 2; k++) {
    const uint32_t c = k ? nd.c1 : nd.c0, n = k ? nd.n1 : nd.n0;
    if (c == RT_NODE_EMPTY) continue;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (n) {
      for (uint32_t s = c; s < c + n; s++) rt_grow_slot_box(sc, base, s, lo, hi);
    } else {
      const RtNode& ch = nodes[c];
      for (int a = 0; a < 3; a++) {
        if (ch.c0 != RT_NODE_EMPTY) lo[a] = rt_min_keep(lo[a], ch.lo0[a]), hi[a] = rt_max_keep(hi[a], ch.hi0[a]);
        if (ch.c1 != RT_NODE_EMPTY) lo[a] = rt_min_keep(lo[a], ch.lo1[a]), hi[a] = rt_max_keep(hi[a], ch.hi1[a]);
      }
    }
    float* dlo = k ? nd.lo1 : nd.lo0;
    float* dhi = k ? nd.hi1 : nd.hi0;
    for (int a = 0; a < 3; a++) dlo[a] = lo[a], dhi[a] = hi[a];
  }
}

// the copy of node `src` for direction octant `oc` (pack_octant_nodes): planes selected, the child entered first stored first
RT_HD static inline RtNode rt_octant_node(const RtNode& src, uint32_t oc) {
  RtNode d0 = src;
  float key[2] = {0.f, 0.f};
  for (int a = 0; a < 3; a++) {
    const bool neg = (oc >> a) & 1u;
    if (src.c0 != RT_NODE_EMPTY) {
      d0.lo0[a] = neg ? src.hi0[a] : src.lo0[a];
      d0.hi0[a] = neg ? src.lo0[a] : src.hi0[a];
      key[0] = rt_fadd(key[0], neg ? -src.hi0[a] : src.lo0[a]);
    }
    if (src.c1 != RT_NODE_EMPTY) {
      d0.lo1[a] = neg ? src.hi1[a] : src.lo1[a];
      d0.hi1[a] = neg ? src.lo1[a] : src.hi1[a];
      key[1] = rt_fadd(key[1], neg ? -src.hi1[a] : src.lo1[a]);
    }
  }
  if (src.c0 != RT_NODE_EMPTY && src.c1 != RT_NODE_EMPTY && key[1] < key[0]) {
    RtNode sw = d0;
    for (int a = 0; a < 3; a++) {
      sw.lo0[a] = d0.lo1[a], sw.hi0[a] = d0.hi1[a];
      sw.lo1[a] = d0.lo0[a], sw.hi1[a] = d0.hi0[a];
    }
    sw.c0 = d0.c1, sw.n0 = d0.n1, sw.c1 = d0.c0, sw.n1 = d0.n0;
    d0 = sw;
  }
  return d0;
}
RT_HD static inline void rt_upd_octant(const RtDevScene& sc, char* base, uint32_t oc, uint32_t i) {
  const RtNode* nodes = (const RtNode*)(base + sc.off_nodes);
  ((RtNode*)(base + sc.off_nodes_oct))[(size_t)oc * sc.n_nodes + i] = rt_octant_node(nodes[i], oc);
}

// threaded entry i mirrors child (thr_src[i] & 1) of node thr_src[i] >> 1: its box is copied, skip and leaf stay
RT_HD static inline void rt_upd_thr(const RtDevScene& sc, char* base, const uint32_t* thr_src, uint32_t i) {
  const RtNode& nd = ((const RtNode*)(base + sc.off_nodes))[thr_src[i] >> 1];
  const bool second = thr_src[i] & 1u;
  const float* lo = second ? nd.lo1 : nd.lo0;
  const float* hi = second ? nd.hi1 : nd.hi0;
  RtThrNode& t = ((RtThrNode*)(base + sc.off_nodes_thr))[i];
  for (int a = 0; a < 3; a++) t.lo[a] = lo[a], t.hi[a] = hi[a];
}

// ---- scene bounds (scene_bounds of rt_scene_pack.cpp): minima and maxima of finite coordinates, so any order gives the
// same six floats ----------------------------------------------------------------------------------------------------------
RT_HD static inline void rt_bounds_grow(float lo[3], float hi[3], float x, float y, float z) {
  const float v[3] = {x, y, z};
  for (int a = 0; a < 3; a++)
    if (rt_finite(v[a])) lo[a] = fminf(lo[a], v[a]), hi[a] = fmaxf(hi[a], v[a]);
}
RT_HD static inline void rt_bounds_sphere(const RtDevScene& sc, const char* base, uint32_t i, float lo[3], float hi[3]) {
  const float* s = (const float*)(base + sc.off_spheres) + 4 * (size_t)i;
  const float r = rt_fsqrt(fabsf(s[3]));
  rt_bounds_grow(lo, hi, rt_fadd(s[0], -r), rt_fadd(s[1], -r), rt_fadd(s[2], -r));
  rt_bounds_grow(lo, hi, rt_fadd(s[0], r), rt_fadd(s[1], r), rt_fadd(s[2], r));
}
// (a triangle referenced by several slots is grown several times: the same bounds)
RT_HD static inline void rt_bounds_slot(const RtDevScene& sc, const char* base, uint32_t slot, float lo[3], float hi[3]) {
  const float* q = (const float*)(base + sc.off_tri_isect) + 12 * (size_t)slot;
  rt_bounds_grow(lo, hi, q[0], q[1], q[2]);
  rt_bounds_grow(lo, hi, rt_fadd(q[0], q[3]), rt_fadd(q[1], q[4]), rt_fadd(q[2], q[5]));
  rt_bounds_grow(lo, hi, rt_fadd(q[0], q[6]), rt_fadd(q[1], q[7]), rt_fadd(q[2], q[8]));
}
RT_HD static inline void rt_bounds_finish(const float lo[3], const float hi[3], float out[6]) {
  for (int a = 0; a < 3; a++) {
    const bool ok = lo[a] <= hi[a];
    out[a] = ok ? lo[a] : 0.f, out[3 + a] = ok ? hi[a] : 1.f;
  }
}

// ---- receiver record of canonical triangle t (triangle_cells): the (u, v) maps in fp64 from the triangle's intersection
// record.  The cell ALLOCATION is the one of creation: recv_cell[2 t] = R, recv_cell[2 t + 1] = first cell.  The record gets
// that R, or 0 ("no cells: walk", the shade side's rr.x != 0u test) while the maps are not finite or fail the conditioning
// bound err * R <= 0.04 against the CURRENT scene bounds.  Returns true when R went to 0 that way.
RT_HD static inline bool rt_upd_recv(const RtDevScene& sc, char* base, const uint32_t* recv_cell, const uint32_t* tri_slot,
                                     const float bounds[6], uint32_t t) {
#pragma clang fp contract(off)
  const float* s = (const float*)(base + sc.off_tri_isect) + 12 * (size_t)tri_slot[t];
  const float v1[3] = {s[0], s[1], s[2]}, e1[3] = {s[3], s[4], s[5]}, e2[3] = {s[6], s[7], s[8]};
  double pmax = 0.0;
  for (int a = 0; a < 3; a++) pmax = fmax(pmax, fmax(fabs((double)bounds[a]), fabs((double)bounds[3 + a])));
  const double n[3] = {(double)e1[1] * e2[2] - (double)e1[2] * e2[1], (double)e1[2] * e2[0] - (double)e1[0] * e2[2],
                       (double)e1[0] * e2[1] - (double)e1[1] * e2[0]};
  const double nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
  const uint32_t R0 = recv_cell[2 * (size_t)t];
  uint32_t Rr = 0;
  float q[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (nn > 0.0 && fabs(nn) < (double)INFINITY) {
    Rr = R0;
    const double au[3] = {(e2[1] * n[2] - e2[2] * n[1]) / nn, (e2[2] * n[0] - e2[0] * n[2]) / nn, (e2[0] * n[1] - e2[1] * n[0]) / nn};
    const double av[3] = {(n[1] * e1[2] - n[2] * e1[1]) / nn, (n[2] * e1[0] - n[0] * e1[2]) / nn, (n[0] * e1[1] - n[1] * e1[0]) / nn};
    const double au0 = -(v1[0] * au[0] + v1[1] * au[1] + v1[2] * au[2]), av0 = -(v1[0] * av[0] + v1[1] * av[1] + v1[2] * av[2]);
    q[0] = (float)au[0], q[1] = (float)au[1], q[2] = (float)au[2], q[3] = (float)au0;
    q[4] = (float)av[0], q[5] = (float)av[1], q[6] = (float)av[2], q[7] = (float)av0;
    for (int k = 0; k < 8; k++)
      if (!rt_finite(q[k])) Rr = 0;
    const double err = 4e-7 * fmax((fabs(au[0]) + fabs(au[1]) + fabs(au[2])) * pmax + fabs(au0),
                                   (fabs(av[0]) + fabs(av[1]) + fabs(av[2])) * pmax + fabs(av0));
    if (Rr > 1u && err * Rr > 0.04) Rr = 0;
  }
  float* r = rt_blob_f(base, sc.off_recv) + 12 * (size_t)t;
  for (int k = 0; k < 8; k++) r[k] = q[k];
  ((uint32_t*)r)[8] = Rr;  // (word 9, the first cell, stays)
  return R0 != 0u && Rr == 0u;
}

// ---- spheres, materials, lights (pack_spheres, pack_materials, pack_lights) -------------------------------------------------
RT_HD static inline void rt_upd_sphere(const RtDevScene& sc, char* base, uint32_t i, const float* centre, const float* r_sq) {
  float* s = rt_blob_f(base, sc.off_spheres) + 4 * (size_t)i;
  s[0] = centre[3 * (size_t)i], s[1] = centre[3 * (size_t)i + 1], s[2] = centre[3 * (size_t)i + 2], s[3] = r_sq[i];
  rt_blob_f(base, sc.off_sphere_rad)[i] = rt_fmul(rt_fsqrt(fabsf(r_sq[i])), 1.0f + 4e-7f);
}
RT_HD static inline void rt_upd_material(const RtDevScene& sc, char* base, uint32_t i, const float* rows) {
  const float* r = rows + (size_t)i * RT_MATERIAL_STRIDE;
  float* q = rt_blob_f(base, sc.off_materials) + 12 * (size_t)i;
  q[0] = r[RT_MAT_R], q[1] = r[RT_MAT_G], q[2] = r[RT_MAT_B], q[3] = r[RT_MAT_METALLIC];
  q[4] = r[RT_MAT_SHININESS], q[5] = r[RT_MAT_IOR], q[6] = r[RT_MAT_OPACITY], q[7] = r[RT_MAT_BOOST];
  q[8] = r[RT_MAT_HAS_OPACITY];
  const float ior = r[RT_MAT_IOR];
  const float k = rt_fdiv(rt_fadd(1.0f, -ior), rt_fadd(1.0f, ior));
  q[9] = rt_fdiv(1.0f, ior), q[10] = rt_fmul(k, k), q[11] = 0.f;
}
RT_HD static inline void rt_upd_light(const RtDevScene& sc, char* base, uint32_t i, const float* rows) {
  const float* r = rows + (size_t)i * RT_LIGHT_STRIDE;
  float* q = rt_blob_f(base, sc.off_lights) + 8 * (size_t)i;
  q[0] = r[0], q[1] = r[1], q[2] = r[2], q[3] = r[6];
  q[4] = r[3], q[5] = r[4], q[6] = r[5], q[7] = 0.f;
}
// the class the tree was built for (build_bvh's no_split): light passes through triangles of this material
RT_HD static inline bool rt_material_transmissive(const float* row) {
  return row[RT_MAT_HAS_OPACITY] != 0.0f && !(fabsf(row[RT_MAT_OPACITY]) <= 1.1920929e-7f);
}
