// rt_cell_prune.h -- the rule that thins out the per-cell shadow candidate lists (RtDevParams::cell_lists).
//
// rt_flags_kernel lists, per (receiver cell, light), the leaf slots that survive the cell's fat beam.  Its barycentric test
// bounds the beam with products of 1-norms and a cylinder, and it has no test for "behind the light", so a list carries
// candidates that no sample ray of any hit point of the cell can be accepted for.  Every such candidate is then beam-tested
// once per (wavefront, light) and triangle-tested once per sample by the render kernels, for nothing.  The rule below
// removes them from the lists, once per scene and light-cloud size, right after rt_flags_kernel.
//
// Compiled twice, as rt_refit.h is: rt_cell_prune_packed (rt_cell_prune.cpp) calls rt_cell_prune_cell in a loop on the host,
// rt_cell_prune_kernel (rt_cell_prune.hip) is the same function with a thread index.  Every float operation is a single
// correctly rounded one (rt_fmul, rt_fadd, rt_fdiv, rt_fsqrt), so the device writes what the host model writes, word for word.
// Not part of the public ABI.
//
// ---- the geometry ------------------------------------------------------------------------------------------------------------
// A shadow ray of the render starts at so = fl(h + ld * eps) for a hit point h of the cell and the unit direction
// ld = normalize(lp - h) towards a light sample lp = fl(light + cloud offset); it is accepted by a triangle when the literal
// test (tri_hit) finds u >= 0, v >= 0, u + v < 1 and EPS < t <= tmax = |lp - so|.
//
//   o  = so, the ray's ORIGIN:     o = p + do,   |do|_2 <= rho    p = the cell's centre
//   lp' = o + tmax * ld:           lp' = c + dl, |dl|_2 <= delta  c = fl(light + cloud_centre)
//
// rho = the Euclidean radius of the cell's 8-point hull about p (the hull rt_flags_kernel builds: 5 % larger than the cell on
// every side) + the rounding of a hit point off that hull and of this file's own construction of it + beam_eps_o (>= |so - h|).
// delta = beam_delta (cloud radius + 2 eps) + the distance of lp' from lp: ld and so are rounded, so the ray passes lp within
// a few ulp of the coordinates involved.  By construction D = lp' - o is parallel to ld EXACTLY, |D| = tmax, and (o, D)
// ranges over a subset of ball(p, rho) x ball(c, delta): what holds for every pair of the two balls holds for every ray.
//
// With dseg = c - p, b = v1 - p, b_c = v1 - c, c1 = -e1, c2 = -e2, X = e1 x e2, D = dseg + dl - do, v1 - o = b - do:
//
//   u det = D . ((v1 - o) x c2)          [tri_hit: y = c2 x d, u det = y . (v1 - o) = d . ((v1 - o) x c2)]
//         = (dseg + dl - do) . (w - do x c2)                                     w = b x c2
//         = dseg.w + dl.w - do.w - dseg.(do x c2) - (dl - do).(do x c2)
//     and do.w + dseg.(do x c2) = do.(b x c2) - do.(dseg x c2) = do.((b - dseg) x c2) = do.w_c,   w_c = b_c x c2, so
//         = dseg.w + dl.w - do.w_c - (dl - do).(do x c2)
//   |u det - dseg.w| <= delta |w| + rho |w_c| + (delta + rho) rho |c2|                                          (U)
//   v det = D . (c1 x (v1 - o)): the same with w' = c1 x b, w'_c = c1 x b_c and |c1|                            (V)
//   det   = D . X = dseg.X + (dl - do).X:         |det - dseg.X| <= (delta + rho) |X|                           (D)
//   t det = X . (v1 - o) = X.b - X.do:            |X.(v1 - o) - X.b| <= rho |X|      (d = D: t in units of |D|) (T)
//
// Rounding.  The literal test evaluates these sums in fp32; its own pre-filter (tri_hit phase 1) takes G = 2e-6 times the sum
// of the absolute products as the bound of that error, and so does beam_rejects_all.  Here every sum of absolute products
// is bounded by a product of norms (|y.b'| terms <= |D| |c2| |b'|, ...) with |D| <= Lp = |dseg| + delta + rho and
// |v1 - o| <= |b| + rho, and the margin is taken four times as large (RT_PRUNE_G), which also covers this file's own fp32
// evaluation of dseg.w, dseg.X and X.b (three roundings per product chain, < 1e-6 of the same products).  Norms are rounded
// up (rt_prune_norm).  Every comparison is written so that a NaN keeps the candidate.
#pragma once

#include "rt_refit.h"

#define RT_PRUNE_LIST_SLOTS 8u       // RT_CELL_LIST_SLOTS, RT_CELL_LIST_END, RT_CELL_LIST_OVERFLOW of rt_kernels.hip
#define RT_PRUNE_LIST_END 0xFFFFu
#define RT_PRUNE_LIST_OVERFLOW 0xFFFEu
#define RT_PRUNE_G 8e-6f

// what the rule consists of.  The render uses RT_PRUNE_FULL; the other values exist for the host-side checks: the weaker
// rule (no far side, products of 1-norms) must prune a subset, and a rule without one of its rho terms must be caught.
#define RT_PRUNE_FAR 1u            // the far-side inequality
#define RT_PRUNE_EUCLID 2u         // Euclidean slacks (else: products of 1-norms)
#define RT_PRUNE_NO_RHO_WC 4u      // ABLATION (unsound): without rho |w_c|
#define RT_PRUNE_NO_RHO_FAR 8u     // ABLATION (unsound): without rho |X| in the far-side inequality
#define RT_PRUNE_FULL (RT_PRUNE_FAR | RT_PRUNE_EUCLID)

// kernel argument besides RtDevScene
struct RtCellPruneArgs {
  const float* flag_geo;  // canonical triangles, 12 floats: {v1, bits(R)} {e1, bits(first cell)} {e2, 0}
  uint16_t* lists;        // [n_cells][n_lights][8], in place
  uint16_t* flags;        // [n_cells], in place: bit l is set when the list of light l becomes empty
  uint32_t n_cells, n_tri_cells;
  float cloud_centre[3];
  float beam_delta, beam_eps_o;
  uint32_t mode;          // RT_PRUNE_*
};

// one (cell, light) beam
struct RtPruneBeam {
  float p[3], c[3], dseg[3];
  float rho, delta, lenp;  // lenp >= |D| for every ray of the beam
};

RT_HD static inline float rt_prune_dot(const float a[3], const float b[3]) {
  return rt_fadd(rt_fadd(rt_fmul(a[0], b[0]), rt_fmul(a[1], b[1])), rt_fmul(a[2], b[2]));
}
RT_HD static inline void rt_prune_cross(const float a[3], const float b[3], float out[3]) {
  out[0] = rt_fadd(rt_fmul(a[1], b[2]), -rt_fmul(a[2], b[1]));
  out[1] = rt_fadd(rt_fmul(a[2], b[0]), -rt_fmul(a[0], b[2]));
  out[2] = rt_fadd(rt_fmul(a[0], b[1]), -rt_fmul(a[1], b[0]));
}
RT_HD static inline void rt_prune_sub(const float a[3], const float b[3], float out[3]) {
  out[0] = rt_fadd(a[0], -b[0]), out[1] = rt_fadd(a[1], -b[1]), out[2] = rt_fadd(a[2], -b[2]);
}
RT_HD static inline float rt_prune_norm1(const float a[3]) { return rt_fadd(rt_fadd(fabsf(a[0]), fabsf(a[1])), fabsf(a[2])); }
// an upper bound of |a|_2: the rounded root of the rounded sum of squares is low by < 3e-7 of it; where the squares would
// underflow the 1-norm stands in (>= the 2-norm)
RT_HD static inline float rt_prune_norm(const float a[3]) {
  const float q = rt_prune_dot(a, a);
  return q > 1e-30f ? rt_fmul(rt_fsqrt(q), 1.00001f) : rt_prune_norm1(a);
}
// |a x b| from above: the Euclidean norm of the computed product plus its rounding (each component: two products and a
// difference, < 2e-7 (|a||b|) in all), or the product of the 1-norms
RT_HD static inline float rt_prune_cross_norm(const float axb[3], float na, float nb, bool euclid) {
  if (!euclid) return rt_fmul(rt_fmul(na, nb), 1.0001f);
  return rt_fadd(rt_prune_norm(axb), rt_fmul(4e-7f, rt_fmul(na, nb)));
}

// ---- the rule: true = no ray of the beam can be accepted by the triangle in q = {v1, e1, e2, X} (a leaf slot's record) -----------
RT_HD static inline bool rt_prune_rule(const RtPruneBeam& B, const float* q, uint32_t mode) {
  const bool euclid = (mode & RT_PRUNE_EUCLID) != 0u;
  const float v1[3] = {q[0], q[1], q[2]}, c1[3] = {-q[3], -q[4], -q[5]}, c2[3] = {-q[6], -q[7], -q[8]}, X[3] = {q[9], q[10], q[11]};
  float b[3], bc[3];
  rt_prune_sub(v1, B.p, b);
  rt_prune_sub(v1, B.c, bc);
  const float dr = rt_fadd(B.delta, B.rho);
  const float nX = euclid ? rt_prune_norm(X) : rt_fmul(rt_prune_norm1(X), 1.0001f);
  const float nb = euclid ? rt_prune_norm(b) : rt_fmul(rt_prune_norm1(b), 1.0001f);
  const float nbc = euclid ? rt_prune_norm(bc) : rt_fmul(rt_prune_norm1(bc), 1.0001f);
  const float nbo = rt_fadd(nb, B.rho);  // >= |v1 - o|
  // (D) the sign of det is the sign of dseg.X over the whole beam: |det - dseg.X| <= (delta + rho)|X|, and the literal det
  // (d.X with the rounded unit d; in units of |D| <= Lp) is off by its rounding, < G Lp |X|
  const float det0 = rt_prune_dot(B.dseg, X);
  const float ad = fabsf(det0);
  const float dslack = rt_fadd(rt_fmul(dr, nX), rt_fmul(RT_PRUNE_G, rt_fmul(B.lenp, nX)));
  if (!(ad > rt_fmul(dslack, 1.001f))) return false;
  const float sg = det0 < 0.0f ? -1.0f : 1.0f;
  const float det_hi = rt_fmul(rt_fadd(ad, dslack), 1.00001f);  // >= |det| (Lp units), rounding of this line included
  // (T) far side: the literal accepts only t <= tmax = |D|, that is (t det) sgn <= |det| in units of |D|.  Over the beam
  // (t det) sgn >= X.b sgn - rho |X| and |det| <= |dseg.X| + (delta + rho)|X|; the literal t is a sum of three products
  // (x_i / det)(v1 - o)_i, off by < G |X| |v1 - o| / |det|, and tmax by < 1e-6 of itself (the 1.00001 of det_hi).
  if (mode & RT_PRUNE_FAR) {
    const float xb = rt_fmul(rt_prune_dot(X, b), sg);
    const float rho_x = (mode & RT_PRUNE_NO_RHO_FAR) ? 0.0f : rt_fmul(B.rho, nX);
    const float lo = rt_fadd(rt_fadd(xb, -rho_x), -rt_fmul(RT_PRUNE_G, rt_fmul(nX, nbo)));
    if (lo > det_hi) return true;
  }
  // (U) u < 0 for every ray: (u det) sgn <= dseg.w sgn + delta |w| + rho |w_c| + (delta + rho) rho |c2| < 0 by more than the
  // rounding of the literal u (y.(v1 - o) / det: < G Lp |c2| |v1 - o| in units of |D|)
  const float n2 = euclid ? rt_prune_norm(c2) : rt_fmul(rt_prune_norm1(c2), 1.0001f);
  float w[3], wc[3];
  rt_prune_cross(b, c2, w);
  rt_prune_cross(bc, c2, wc);
  const float u0 = rt_fmul(rt_prune_dot(B.dseg, w), sg);
  const float rho_wc = (mode & RT_PRUNE_NO_RHO_WC) ? 0.0f : rt_fmul(B.rho, rt_prune_cross_norm(wc, nbc, n2, euclid));
  const float su = rt_fmul(rt_fadd(rt_fadd(rt_fadd(rt_fmul(B.delta, rt_prune_cross_norm(w, nb, n2, euclid)), rho_wc), rt_fmul(rt_fmul(dr, B.rho), n2)),
                                   rt_fmul(RT_PRUNE_G, rt_fmul(B.lenp, rt_fmul(n2, nbo)))), 1.00001f);
  if (rt_fadd(u0, su) < 0.0f) return true;
  // (V) v < 0 for every ray: the same with w' = c1 x b, w'_c = c1 x b_c, |c1|
  const float n1 = euclid ? rt_prune_norm(c1) : rt_fmul(rt_prune_norm1(c1), 1.0001f);
  rt_prune_cross(c1, b, w);
  rt_prune_cross(c1, bc, wc);
  const float v0 = rt_fmul(rt_prune_dot(B.dseg, w), sg);
  const float rho_wc1 = (mode & RT_PRUNE_NO_RHO_WC) ? 0.0f : rt_fmul(B.rho, rt_prune_cross_norm(wc, nbc, n1, euclid));
  const float sv = rt_fmul(rt_fadd(rt_fadd(rt_fadd(rt_fmul(B.delta, rt_prune_cross_norm(w, nb, n1, euclid)), rho_wc1), rt_fmul(rt_fmul(dr, B.rho), n1)),
                                   rt_fmul(RT_PRUNE_G, rt_fmul(B.lenp, rt_fmul(n1, nbo)))), 1.00001f);
  if (rt_fadd(v0, sv) < 0.0f) return true;
  // u + v >= 1 for every ray: ((u + v) det) sgn >= (dseg.w + dseg.w') sgn - su - sv, |det| <= det_hi (the literal adds two
  // rounded quotients and compares with 1: the margins of su, sv and det_hi cover it)
  if (rt_fadd(rt_fadd(u0, v0), -rt_fmul(rt_fadd(su, sv), 1.00001f)) > det_hi) return true;
  return false;
}

// ---- the cell: centre p, hull points pt[8] (as rt_flags_kernel builds them), false = the cell is never looked up ----------------
RT_HD static inline bool rt_prune_cell_hull(const RtDevScene& sc, const char* base, const RtCellPruneArgs& a, uint32_t c, float pm[3], float pt[8][3],
                                            float* extra_scale) {
  *extra_scale = 0.0f;
  auto axpy2 = [](const float v1[3], const float e1[3], float s, const float e2[3], float t, float out[3]) {
    for (int k = 0; k < 3; k++) out[k] = rt_fadd(rt_fadd(v1[k], rt_fmul(e1[k], s)), rt_fmul(e2[k], t));
  };
  if (c < a.n_tri_cells) {
    // the triangle that owns cell c: the last one whose first cell is <= c (triangles without cells share their successor's)
    uint32_t lo = 0u, hi = sc.n_triangles;
    while (hi - lo > 1u) {
      const uint32_t mid = (lo + hi) >> 1;
      uint32_t first_mid;
      memcpy(&first_mid, a.flag_geo + 12u * (size_t)mid + 7u, 4);
      if (first_mid <= c) lo = mid; else hi = mid;
    }
    const float* g = a.flag_geo + 12u * (size_t)lo;
    uint32_t R, first;
    memcpy(&R, g + 3, 4), memcpy(&first, g + 7, 4);
    if (R == 0u || c < first) return false;
    const uint32_t local = c - first, j = local / R, i = local - j * R;
    if (i + j >= R) return false;  // (cells beyond the hypotenuse are never looked up)
    const float v1[3] = {g[0], g[1], g[2]}, e1[3] = {g[4], g[5], g[6]}, e2[3] = {g[8], g[9], g[10]};
    const float inv_r = rt_fdiv(1.0f, (float)R);
    const float u0 = rt_fmul(rt_fadd((float)i, -0.05f), inv_r), u1 = rt_fmul(rt_fadd((float)i, 1.05f), inv_r);
    const float w0 = rt_fmul(rt_fadd((float)j, -0.05f), inv_r), w1 = rt_fmul(rt_fadd((float)j, 1.05f), inv_r);
    axpy2(v1, e1, u0, e2, w0, pt[0]);
    axpy2(v1, e1, u1, e2, w0, pt[1]);
    axpy2(v1, e1, u0, e2, w1, pt[2]);
    axpy2(v1, e1, u1, e2, w1, pt[3]);
    for (int k = 0; k < 4; k++) pt[4 + k][0] = pt[k][0], pt[4 + k][1] = pt[k][1], pt[4 + k][2] = pt[k][2];
    axpy2(v1, e1, rt_fmul(rt_fadd((float)i, 0.5f), inv_r), e2, rt_fmul(rt_fadd((float)j, 0.5f), inv_r), pm);
    return true;
  }
  // a cell of a sphere: a patch of its cube map of directions between the tangent plane at the patch centre (outer corners)
  // and the parallel plane through its lowest corner (inner corners)
  uint32_t k = 0u, Rs = 0u, first = 0u;
  for (uint32_t s = 0; s < sc.n_spheres; s++) {
    const uint32_t* sr = (const uint32_t*)(base + sc.off_srecv) + 2u * (size_t)s;
    const uint64_t end = (uint64_t)sr[1] + 6ull * sr[0] * sr[0];
    if (sr[0] != 0u && c >= sr[1] && (uint64_t)c < end) k = s, Rs = sr[0], first = sr[1];
  }
  if (Rs == 0u) return false;
  const float* sp = (const float*)(base + sc.off_spheres) + 4u * (size_t)k;
  const float rad = ((const float*)(base + sc.off_sphere_rad))[k];  // (upper bound of the radius)
  const uint32_t local = c - first, face = local / (Rs * Rs), rem = local - face * Rs * Rs, j = rem / Rs, i = rem - j * Rs;
  const float inv_r = rt_fdiv(2.0f, (float)Rs);
  const float a0 = fmaxf(rt_fadd(rt_fmul(rt_fadd((float)i, -0.05f), inv_r), -1.0f), -1.1f), a1 = fminf(rt_fadd(rt_fmul(rt_fadd((float)i, 1.05f), inv_r), -1.0f), 1.1f);
  const float b0 = fmaxf(rt_fadd(rt_fmul(rt_fadd((float)j, -0.05f), inv_r), -1.0f), -1.1f), b1 = fminf(rt_fadd(rt_fmul(rt_fadd((float)j, 1.05f), inv_r), -1.0f), 1.1f);
  const uint32_t m = face >> 1;
  const float sgn = (face & 1u) ? -1.0f : 1.0f;
  auto dir = [&](float x, float y, float out[3]) {  // component m = sign, (m + 1) % 3 = x, (m + 2) % 3 = y; normalised
    float d[3];
    if (m == 0u) d[0] = sgn, d[1] = x, d[2] = y;
    else if (m == 1u) d[0] = y, d[1] = sgn, d[2] = x;
    else d[0] = x, d[1] = y, d[2] = sgn;
    const float n = rt_fsqrt(rt_prune_dot(d, d));
    out[0] = rt_fdiv(d[0], n), out[1] = rt_fdiv(d[1], n), out[2] = rt_fdiv(d[2], n);
  };
  float uc[3], uk[4][3];
  dir(rt_fmul(0.5f, rt_fadd(a0, a1)), rt_fmul(0.5f, rt_fadd(b0, b1)), uc);
  dir(a0, b0, uk[0]), dir(a1, b0, uk[1]), dir(a0, b1, uk[2]), dir(a1, b1, uk[3]);
  float cmin = 1.0f;
  for (int s = 0; s < 4; s++) cmin = fminf(cmin, rt_prune_dot(uk[s], uc));
  cmin = fmaxf(rt_fmul(cmin, 0.9999f), 0.1f);
  for (int s = 0; s < 4; s++) {
    const float cq = fmaxf(rt_prune_dot(uk[s], uc), 0.1f);
    const float ri = rt_fdiv(rt_fmul(rt_fmul(rad, cmin), 0.9999f), cq), ro = rt_fdiv(rt_fmul(rad, 1.0001f), cq);
    for (int x = 0; x < 3; x++) pt[s][x] = rt_fadd(sp[x], rt_fmul(uk[s][x], ri)), pt[4 + s][x] = rt_fadd(sp[x], rt_fmul(uk[s][x], ro));
  }
  for (int x = 0; x < 3; x++) pm[x] = rt_fadd(sp[x], rt_fmul(uc[x], rad));
  *extra_scale = rt_fadd(rt_prune_norm1(sp), rad);
  return true;
}

// ---- one cell: its n_lights lists (list, 8 words each) and its flags word, in place ---------------------------------------------
RT_HD static inline void rt_cell_prune_cell(const RtDevScene& sc, const char* base, const RtCellPruneArgs& a, uint32_t c, uint16_t* list, uint16_t* flag) {
  float pm[3], pt[8][3], extra;
  if (!rt_prune_cell_hull(sc, base, a, c, pm, pt, &extra)) return;
  // rho: Euclidean radius of the hull about pm (1.0001: its rounding) + 2e-6 of the coordinates that go into a hit point and
  // into the hull (a hit point lies off its triangle's plane by the rounding of o + t d; this file and rt_flags_kernel round
  // the hull differently) + the push of the shadow ray's origin
  float r = 0.0f, scale = rt_fadd(rt_prune_norm1(pm), extra);
  for (int k = 0; k < 8; k++) {
    float dk[3];
    rt_prune_sub(pt[k], pm, dk);
    r = fmaxf(r, rt_prune_norm(dk));
    scale = fmaxf(scale, rt_fadd(rt_prune_norm1(pt[k]), extra));
  }
  RtPruneBeam B;
  B.p[0] = pm[0], B.p[1] = pm[1], B.p[2] = pm[2];
  B.rho = rt_fadd(rt_fadd(rt_fmul(r, 1.0001f), rt_fmul(2e-6f, scale)), a.beam_eps_o);
  const float* lights = (const float*)(base + sc.off_lights);
  const float* isect = (const float*)(base + sc.off_tri_isect);
  uint32_t fl = *flag;
  bool fl_changed = false;
  for (uint32_t l = 0; l < sc.n_lights && l < 8u; l++) {
    uint16_t* w = list + (size_t)l * RT_PRUNE_LIST_SLOTS;
    uint16_t in[RT_PRUNE_LIST_SLOTS];
    memcpy(in, __builtin_assume_aligned(w, 16), 16);  // (one 16-byte load: a list is one uint4 of RtDevParams::cell_lists)
    if (in[0] >= RT_PRUNE_LIST_OVERFLOW) continue;  // empty, or more than 8 candidates: the render walks the tree for such a cell
    for (int x = 0; x < 3; x++) B.c[x] = rt_fadd(lights[8u * l + x], a.cloud_centre[x]);
    rt_prune_sub(B.c, B.p, B.dseg);
    // delta: the cloud's ball + 2 eps (beam_delta) + how far the ray passes from its light sample (rounding of ld and so)
    B.delta = rt_fadd(a.beam_delta, rt_fmul(2e-6f, rt_fadd(scale, rt_prune_norm1(B.c))));
    B.lenp = rt_fadd(rt_fadd(rt_prune_norm(B.dseg), B.delta), B.rho);
    uint32_t n = 0, n_in = 0;
    uint16_t out[RT_PRUNE_LIST_SLOTS];
    for (uint32_t k = 0; k < RT_PRUNE_LIST_SLOTS; k++) {
      const uint32_t slot = in[k];
      if (slot >= RT_PRUNE_LIST_OVERFLOW) break;
      n_in++;
      if (slot < sc.n_slots && rt_prune_rule(B, isect + 12u * (size_t)slot, a.mode)) continue;
      out[n++] = (uint16_t)slot;
    }
    if (n == n_in) continue;
    for (uint32_t k = n; k < RT_PRUNE_LIST_SLOTS; k++) out[k] = (uint16_t)RT_PRUNE_LIST_END;
    memcpy(__builtin_assume_aligned(w, 16), out, 16);
    if (n == 0u) fl |= 1u << l, fl_changed = true;  // no triangle can shadow this cell for light l
  }
  if (fl_changed) *flag = (uint16_t)fl;
}

// host model (rt_cell_prune.cpp): every cell of a packed scene, on arrays laid out as the device's.  a.flag_geo is taken from pk.
struct RtPackedScene;
void rt_cell_prune_packed(const RtPackedScene& pk, RtCellPruneArgs a);
// the kernel (rt_cell_prune.hip); returns hipError_t as int
int rt_launch_cell_prune(const RtDevScene& sc, const RtCellPruneArgs& a, void* stream);
