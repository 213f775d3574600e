// rt_cell_through.h -- the fourth once-per-scene stage of the per-cell shadow candidate lists: marks for the transmissive
// triangles that EVERY shadow ray of a (receiver cell, light) crosses.
//
// A wall-sized pane of glass between a receiver and a light passes every stage of tri_hit's pre-filter for every lane, so each
// sample ray pays the whole literal test (the pre-filter, an IEEE reciprocal, three 16-byte record loads) for the answer "yes,
// these lanes", and only the accumulation of the pane's filter behind it changes the pixel.  The answer is fixed per receiver
// cell: the beam of a cell is thin against a pane.  This stage, right after rt_cell_resolve on the same stream, decides it once
// per (cell, light, listed entry) with the mirror image of the bounds of rt_cell_prune.h -- "every ray of the beam is accepted"
// instead of "no ray of the beam is accepted" -- and writes one byte per (cell, light): bit k set = entry k of the final 16-byte
// list is crossed for certain.  The list kernels (rt_primary_soft*_kernel) then skip the literal test of an entry that every
// lane in use lists as marked, and accumulate the occluder for the lanes the test would have returned.  The shadow sums are
// integers, so leaving out a test that would have accepted gives the same bits.
//
// Only entries of lists that are neither empty nor overflowed are marked (a list that stands for a wide record stays
// unmarked), and only leaf slots that carry RT_TRI_TRANSMISSIVE: an opaque triangle that every ray crosses is the umbra rule's
// business (collect_light_candidates), spheres have no entries.
//
// The table is addressed BACKWARDS from its end: the byte of (cell c, light l) is marks_end[-1 - (c n_lights + l)].  The render
// keeps the table in front of the wide records of RtDevParams::cell_wide, in the same allocation, and so needs neither a
// pointer nor a size of its own in the kernel arguments.
//
// Compiled twice, as rt_cell_prune.h is: rt_cell_through_packed (rt_cell_through.cpp) calls rt_cell_through_cell in a loop on the
// host, rt_cell_through_kernel (rt_cell_through.hip) is the same function with a thread index.  Every float operation is a
// single correctly rounded one, so the device writes what the host model writes, word for word.  Not part of the public ABI.
//
// The geometry and the names (p, rho, c, delta, dseg, Lp = lenp, X, b, b_c, w, w_c, G) are those of rt_cell_prune.h.
#pragma once

#include "rt_cell_resolve.h"

// mode bits of this stage (the render passes 0)
#define RT_THROUGH_NO_RHO_WC 1u  // ABLATION (unsound): without rho |w_c|
#define RT_THROUGH_NO_NEAR 2u    // ABLATION (unsound): without the near-side inequality

#define RT_THROUGH_EPS 1.1920929e-7f  // RT_EPS of rt_kernels.hip: the literal test wants t > EPS and |det| > EPS

struct RtCellThroughArgs {
  RtCellPruneArgs cell;  // as the prune stage got it; lists and flags are only read, mode is not used
  uint8_t* marks_end;    // one past the table's last byte: [n_cells][n_lights] bytes, backwards
  uint32_t mode;         // RT_THROUGH_*
};

// ---- the rule: true = every ray of the beam is accepted by the literal test of the triangle q = {v1, e1, e2, X} ------------------
// The literal test (tri_hit phase 2, then t <= tmax) accepts a ray (o, unit d) when |det| > EPS, u >= 0, v >= 0, u + v < 1,
// t > EPS and t <= tmax; its pre-filter (phase 1) may drop a lane only where one of these fails by more than the rounding of
// the literal sequence, so a ray that passes all of them by the margins below passes the pre-filter too.
RT_HD static inline bool rt_through_rule(const RtPruneBeam& B, const float* q, uint32_t mode) {
  const float v1[3] = {q[0], q[1], q[2]}, c1[3] = {-q[3], -q[4], -q[5]}, c2[3] = {-q[6], -q[7], -q[8]}, X[3] = {q[9], q[10], q[11]};
  float b[3], bc[3];
  rt_prune_sub(v1, B.p, b);
  rt_prune_sub(v1, B.c, bc);
  const float dr = rt_fadd(B.delta, B.rho);
  const float nX = rt_prune_norm(X), nb = rt_prune_norm(b), nbc = rt_prune_norm(bc);
  const float nbo = rt_fadd(nb, B.rho);  // >= |v1 - o|
  // (D) as in rt_prune_rule: the sign of det is the sign of dseg.X over the whole beam, |det - dseg.X| <= (delta + rho)|X| and
  // the literal's rounding < G Lp |X| (units of |D| <= Lp)
  const float det0 = rt_prune_dot(B.dseg, X);
  const float ad = fabsf(det0);
  const float dslack = rt_fadd(rt_fmul(dr, nX), rt_fmul(RT_PRUNE_G, rt_fmul(B.lenp, nX)));
  if (!(ad > rt_fmul(dslack, 1.001f))) return false;
  const float sg = det0 < 0.0f ? -1.0f : 1.0f;
  const float det_hi = rt_fmul(rt_fadd(ad, dslack), 1.00001f);   // >= |det| for every ray (units of |D|)
  const float det_lo = rt_fmul(rt_fadd(ad, -dslack), 0.99999f);  // <= |det| for every ray
  // |det| > EPS: the literal takes det with the UNIT direction, |d.X| = |D.X| / |D| >= det_lo / Lp (its rounding, in both of the
  // forms the literal evaluates, is the G Lp |X| of dslack); 1.01 for the roundings of this line and of the unit vector
  if (!(rt_fdiv(det_lo, B.lenp) > rt_fmul(1.01f, RT_THROUGH_EPS))) return false;
  // (U) u > 0 for every ray: (u det) sgn >= dseg.w sgn - delta |w| - rho |w_c| - (delta + rho) rho |c2|, and that exceeds the
  // rounding of the literal u (< G Lp |c2| |v1 - o| in units of |D|): su is the slack of rt_prune_rule, rounding included
  const float n2 = rt_prune_norm(c2);
  float w[3], wc[3];
  rt_prune_cross(b, c2, w);
  rt_prune_cross(bc, c2, wc);
  const float u0 = rt_fmul(rt_prune_dot(B.dseg, w), sg);
  const float rho_wc = (mode & RT_THROUGH_NO_RHO_WC) ? 0.0f : rt_fmul(B.rho, rt_prune_cross_norm(wc, nbc, n2, true));
  const float su = rt_fmul(rt_fadd(rt_fadd(rt_fadd(rt_fmul(B.delta, rt_prune_cross_norm(w, nb, n2, true)), rho_wc), rt_fmul(rt_fmul(dr, B.rho), n2)),
                                   rt_fmul(RT_PRUNE_G, rt_fmul(B.lenp, rt_fmul(n2, nbo)))), 1.00001f);
  if (!(rt_fadd(u0, -su) > 0.0f)) return false;
  // (V) v > 0 for every ray: the same with w' = c1 x b, w'_c = c1 x b_c, |c1|
  const float n1 = rt_prune_norm(c1);
  rt_prune_cross(c1, b, w);
  rt_prune_cross(c1, bc, wc);
  const float v0 = rt_fmul(rt_prune_dot(B.dseg, w), sg);
  const float rho_wc1 = (mode & RT_THROUGH_NO_RHO_WC) ? 0.0f : rt_fmul(B.rho, rt_prune_cross_norm(wc, nbc, n1, true));
  const float sv = rt_fmul(rt_fadd(rt_fadd(rt_fadd(rt_fmul(B.delta, rt_prune_cross_norm(w, nb, n1, true)), rho_wc1), rt_fmul(rt_fmul(dr, B.rho), n1)),
                                   rt_fmul(RT_PRUNE_G, rt_fmul(B.lenp, rt_fmul(n1, nbo)))), 1.00001f);
  if (!(rt_fadd(v0, -sv) > 0.0f)) return false;
  // u + v < 1 for every ray: ((u + v) det) sgn <= (dseg.w + dseg.w') sgn + su + sv < det_lo <= |det|; the literal adds two
  // rounded quotients and compares with 1 (one more rounding, 6e-8: the 0.99999 of det_lo and the margins of su, sv cover it)
  if (!(rt_fadd(rt_fadd(u0, v0), rt_fmul(rt_fadd(su, sv), 1.00001f)) < det_lo)) return false;
  // (T) t det = X.(v1 - o) = X.b - X.do: (t det) sgn lies within rho |X| of X.b sgn, and the literal t (a sum of three products
  // (x_i / det)(v1 - o)_i) is off by < G |X| |v1 - o| / |det|
  const float xb = rt_fmul(rt_prune_dot(X, b), sg);
  const float tslack = rt_fmul(rt_fadd(rt_fmul(B.rho, nX), rt_fmul(RT_PRUNE_G, rt_fmul(nX, nbo))), 1.00001f);
  // near side, t > EPS: the literal t is a true length (unit d), t = (X.(v1 - o)) sgn / |d.X| with |d.X| = |D.X| / |D| <= det_hi /
  // |D|, and |D| >= |dseg| - delta - rho =: dmin (|dseg| rounded down).  So t >= (X.b sgn - tslack) dmin / det_hi, which must
  // exceed EPS (1.01: the roundings of this line).  A receiver cell that lies on the pane has X.b ~ 0 and fails here.
  if (!(mode & RT_THROUGH_NO_NEAR)) {
    const float t_num = rt_fadd(xb, -tslack);
    const float dmin = rt_fadd(rt_fadd(rt_fmul(rt_fsqrt(rt_prune_dot(B.dseg, B.dseg)), 0.99999f), -B.delta), -B.rho);
    if (!(t_num > 0.0f && dmin > 0.0f)) return false;
    if (!(rt_fmul(rt_fdiv(t_num, det_hi), rt_fmul(dmin, 0.9999f)) > rt_fmul(1.01f, RT_THROUGH_EPS))) return false;
  }
  // far side, t <= tmax = |D|: in units of |D| that is (t det) sgn <= |det|.  (t det) sgn <= X.b sgn + tslack < det_lo (1 - 1e-5):
  // tmax and the product t |D| are off by < 1e-6 of themselves, the margin tmax carries
  if (!(rt_fadd(xb, tslack) < rt_fmul(det_lo, 0.99999f))) return false;
  return true;
}

// whether any list of the cell has a transmissive entry the rule could mark (the hull is built only then)
RT_HD static inline bool rt_cell_through_wanted(const RtDevScene& sc, const char* base, const uint16_t* list) {
  const uint32_t* tri_id = (const uint32_t*)(base + sc.off_tri_id);
  for (uint32_t l = 0; l < sc.n_lights && l < 8u; l++) {
    const uint16_t* w = list + (size_t)l * RT_PRUNE_LIST_SLOTS;
    if (w[0] >= RT_PRUNE_LIST_OVERFLOW) continue;
    for (uint32_t k = 0; k < RT_PRUNE_LIST_SLOTS && w[k] < RT_PRUNE_LIST_OVERFLOW; k++)
      if (w[k] < sc.n_slots && (tri_id[w[k]] & RT_TRI_TRANSMISSIVE)) return true;
  }
  return false;
}

// ---- one cell: its n_lights lists (list, 8 words each, read only) -> its n_lights mark bytes, every one of them written -----------
RT_HD static inline void rt_cell_through_cell(const RtDevScene& sc, const char* base, const RtCellThroughArgs& a, uint32_t c, const uint16_t* list) {
  const uint32_t nl = sc.n_lights < 8u ? sc.n_lights : 8u;
  uint8_t* out = a.marks_end - 1 - (size_t)c * sc.n_lights;  // light l: out[-l]
  RtResolveCell K;
  const bool on = rt_cell_through_wanted(sc, base, list) && rt_resolve_cell_setup(sc, base, a.cell, c, K);
  const uint32_t* tri_id = (const uint32_t*)(base + sc.off_tri_id);
  const float* isect = (const float*)(base + sc.off_tri_isect);
  for (uint32_t l = 0; l < nl; l++) {
    uint32_t m = 0u;
    const uint16_t* w = list + (size_t)l * RT_PRUNE_LIST_SLOTS;
    if (on && w[0] < RT_PRUNE_LIST_OVERFLOW) {
      RtPruneBeam B;
      rt_resolve_beam(sc, base, a.cell, K, l, B);
      for (uint32_t k = 0; k < RT_PRUNE_LIST_SLOTS; k++) {
        const uint32_t slot = w[k];
        if (slot >= RT_PRUNE_LIST_OVERFLOW) break;
        if (slot < sc.n_slots && (tri_id[slot] & RT_TRI_TRANSMISSIVE) && rt_through_rule(B, isect + 12u * (size_t)slot, a.mode)) m |= 1u << k;
      }
    }
    out[-(ptrdiff_t)l] = (uint8_t)m;
  }
}

// host model (rt_cell_through.cpp): every cell of a packed scene, on arrays laid out as the device's.  a.cell.flag_geo is taken
// from pk.
struct RtPackedScene;
void rt_cell_through_packed(const RtPackedScene& pk, RtCellThroughArgs a);
// the table's bytes (a multiple of 64: the wide records behind it stay at 64-byte boundaries), 0 = does not fit what the
// budget leaves
size_t rt_cell_through_bytes(uint32_t n_cells, uint32_t n_lights, size_t budget_left);
// the kernel (rt_cell_through.hip); returns hipError_t as int
int rt_launch_cell_through(const RtDevScene& sc, const RtCellThroughArgs& a, void* stream);
