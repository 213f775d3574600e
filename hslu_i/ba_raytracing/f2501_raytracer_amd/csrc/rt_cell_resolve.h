// rt_cell_resolve.h -- the third once-per-scene stage of the per-cell shadow candidate lists: lists that rt_flags_kernel gave
// up on (more than 8 candidates under its fat beam: RT_CELL_LIST_OVERFLOW) are enumerated again under the sharper rule.
//
// A (wavefront, light) set in which any lane in use sits in a cell with an overflowed list takes no list at all: it walks the
// BVH, and what it collects is never seen by the rule of rt_cell_prune.h.  rt_cell_prune_cell leaves such lists alone (it
// can only thin out what is listed).  This stage, right after it, walks the threaded tree once per overflowed (cell, light)
// with the beam of rt_cell_prune_cell, offers every leaf slot it reaches to the near-side rule below and to rt_prune_rule,
// and writes the survivors as a normal list when there are at most 8 of them (none: an empty list and the cell's
// triangle-clear bit).  More than 8: the marker stays, the render keeps walking for that cell -- unless a pool of WIDE RECORDS
// is given (RtCellResolveArgs::wide): then a list with 9 .. RT_CELL_WIDE_SLOTS survivors gets a record of the pool, 64 bytes
// at a 64-byte boundary: RT_CELL_WIDE_SLOTS 16-bit slots, distinct, padded with RT_PRUNE_LIST_END.  Entry 0 of the 16-byte
// list stays RT_PRUNE_LIST_OVERFLOW -- what follows the marker is read by nobody who does not know of the records, so every
// such reader keeps walking, which gives what the record gives -- entry 1 becomes RT_CELL_WIDE_MARK (0xFFFD: no leaf slot, they
// end at 65532, and neither of the two markers), entries 2 and 3 the record's index in two 15-bit digits, the rest
// RT_PRUNE_LIST_END.  More than RT_CELL_WIDE_SLOTS survivors, or no record left in the pool: the list stays as it was.  Which
// record a list gets depends on the order of the device's atomics; nothing that is rendered does.
//
// Compiled twice, as rt_cell_prune.h is: rt_cell_resolve_packed (rt_cell_resolve.cpp) calls rt_cell_resolve_cell in a loop on the
// host, rt_cell_resolve_kernel (rt_cell_resolve.hip) is the same function with a thread index.  Every float operation is a
// single correctly rounded one, so the device writes what the host model writes, word for word.  Not part of the public ABI.
//
// The geometry and the names (p, rho, c, delta, dseg, Lp = lenp, X, b, G) are those of rt_cell_prune.h.
#pragma once

#include "rt_cell_prune.h"

// mode bits of this stage, beside RT_PRUNE_* (the render uses RT_PRUNE_FULL alone)
#define RT_RESOLVE_NEAR_CENTRE 0x100u  // ABLATION (unsound): the near-side bound taken at the cell's centre, not at its 8 hull points
#define RT_RESOLVE_NO_INFLATE 0x200u   // ABLATION (unsound): boxes are not inflated by max(rho, delta)
#define RT_RESOLVE_NO_NEAR 0x400u      // counting only (sound, weaker): without the near-side rule

// wide records: slots per record (64 bytes: one 64-byte scalar load in the render), the mark in entry 1 of the 16-byte list
#define RT_CELL_WIDE_SLOTS 32u
#define RT_CELL_WIDE_MARK 0xFFFDu
#define RT_CELL_WIDE_MAX_RECORDS (1u << 30)  // two 15-bit digits

// what the stage needs besides RtDevScene
struct RtCellResolveArgs {
  RtCellPruneArgs cell;    // as the prune stage got it (flag_geo, lists, flags, cells, cloud centre, beam constants); mode: RT_PRUNE_* | RT_RESOLVE_*
  float eps_push, eps_ulp; // RtDevParams::beam_eps_push, beam_eps_ulp (0.998 eps and the rounding of eps-sized terms)
  uint32_t* work;          // device only, temporary: 1024 chunk counters, then chunk_cells cell indices (rt_cell_resolve_temp_bytes)
  uint32_t chunk_cells;
  uint8_t* counts;         // optional, [n_cells][n_lights]: survivors of every formerly overflowed list, capped at 255 (the
                           // walk then does not stop at the ninth); nullptr in the render
  // the pool of wide records; all zero: off, and the stage writes what it wrote before there were any
  uint16_t* wide;          // [wide_cap][RT_CELL_WIDE_SLOTS], 64-byte aligned
  uint32_t wide_cap;       // records in the pool, at most RT_CELL_WIDE_MAX_RECORDS
  uint32_t* wide_count;    // records asked for so far (it runs past wide_cap when the pool is full); zero before the stage
};

// the index of the record the 16-byte list w points to, or ~0u: not a wide list
RT_HD static inline uint32_t rt_cell_wide_index(const uint16_t* w) {
  if (w[0] != RT_PRUNE_LIST_OVERFLOW || w[1] != RT_CELL_WIDE_MARK) return ~0u;
  return (uint32_t)(w[2] & 0x7FFFu) | ((uint32_t)(w[3] & 0x7FFFu) << 15);
}
// the next free record of the pool, or ~0u: the pool is full (or off)
RT_HD static inline uint32_t rt_cell_wide_take(const RtCellResolveArgs& a) {
  if (!a.wide || !a.wide_count || a.wide_cap == 0u) return ~0u;
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t at = __hip_atomic_fetch_add(a.wide_count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (a builtin: no device header needed)
#else
  const uint32_t at = (*a.wide_count)++;
#endif
  return at < a.wide_cap && at < RT_CELL_WIDE_MAX_RECORDS ? at : ~0u;
}

// one cell as the stage sees it: hull, centre, and what does not depend on the light
struct RtResolveCell {
  float pm[3], pt[8][3];
  float rho, scale;
};

// rho and scale exactly as rt_cell_prune_cell takes them
RT_HD static inline bool rt_resolve_cell_setup(const RtDevScene& sc, const char* base, const RtCellPruneArgs& a, uint32_t c, RtResolveCell& K) {
  float extra;
  if (!rt_prune_cell_hull(sc, base, a, c, K.pm, K.pt, &extra)) return false;
  float r = 0.0f, scale = rt_fadd(rt_prune_norm1(K.pm), extra);
  for (int k = 0; k < 8; k++) {
    float dk[3];
    rt_prune_sub(K.pt[k], K.pm, dk);
    r = fmaxf(r, rt_prune_norm(dk));
    scale = fmaxf(scale, rt_fadd(rt_prune_norm1(K.pt[k]), extra));
  }
  K.rho = rt_fadd(rt_fadd(rt_fmul(r, 1.0001f), rt_fmul(2e-6f, scale)), a.beam_eps_o);
  K.scale = scale;
  return true;
}
// ... and the beam of light l
RT_HD static inline void rt_resolve_beam(const RtDevScene& sc, const char* base, const RtCellPruneArgs& a, const RtResolveCell& K, uint32_t l, RtPruneBeam& B) {
  const float* lights = (const float*)(base + sc.off_lights);
  B.p[0] = K.pm[0], B.p[1] = K.pm[1], B.p[2] = K.pm[2];
  B.rho = K.rho;
  for (int x = 0; x < 3; x++) B.c[x] = rt_fadd(lights[8u * l + x], a.cloud_centre[x]);
  rt_prune_sub(B.c, B.p, B.dseg);
  B.delta = rt_fadd(a.beam_delta, rt_fmul(2e-6f, rt_fadd(K.scale, rt_prune_norm1(B.c))));
  B.lenp = rt_fadd(rt_fadd(rt_prune_norm(B.dseg), B.delta), B.rho);
}

// ---- near side: true = every ray of the beam finds the triangle q at t <= 0 ("the surface the point lies on, and everything
// behind it": the t-rejection of rt_flags_kernel, collect_light_candidates, restated with this file's beam) -------------------------
// The ray of hit point h and light sample lp starts at so = fl(h + fl(ld eps)), ld the rounded unit vector towards lp, and the
// literal test accepts only t > EPS, t = sum_i fl(fl(x_i / det) (v1 - so)_i).  With sgn = the sign of det -- the sign of
// dseg.X for the whole beam once |dseg.X| > dslack, (D) of rt_cell_prune.h --
//   (X.(v1 - so)) sgn = (X.(v1 - h)) sgn - eps (X.ld) sgn - (X.r) sgn,   r = so - h - eps ld (rounding)
// * ld is parallel to the ray's D, and (o, D) lies in the beam: (X.ld) sgn = |D.X| / |D| >= (|dseg.X| - dslack) / Lp.  The push
//   is taken along ld as rounded (off the unit vector by < 3e-7): 0.998 eps (eps_push) stands for eps.
// * (X.(v1 - h)) sgn is affine in h, and h lies in the hull of the cell's 8 points up to the rounding of a hit point
//   (o + t d evaluated in fp32) and of the hull's construction: it is at most its largest value at the 8 points plus
//   |X| 2.7e-7 scale; |X.r| <= |X| 1.3e-7 (scale + eps).  Together |X| (4e-7 scale + eps_ulp): the allowance rt_flags_kernel makes.
// * the literal t has the sign of (X.(v1 - so)) sgn unless that is within the rounding of its three products,
//   < G |X| |v1 - so| (Cauchy-Schwarz on sum |x_i b_i|, |v1 - so| <= |b| + rho, G four times the pre-filter's, which also
//   covers this file's own three roundings of X.(v1 - pt_k)).
// So when  max_k (X.(v1 - pt_k)) sgn + G |X| (|b| + rho) + |X| (4e-7 scale + eps_ulp)  <  0.998 eps (|dseg.X| - dslack) / Lp
// every ray of the beam has (X.(v1 - so)) sgn < -G |X| |v1 - so|: its literal t is negative, and it is not accepted.  The right
// side is rounded down (0.99999).  A NaN keeps the candidate.
RT_HD static inline bool rt_resolve_near_rule(const RtPruneBeam& B, const RtResolveCell& K, const RtCellResolveArgs& a, const float* q) {
  const float v1[3] = {q[0], q[1], q[2]}, X[3] = {q[9], q[10], q[11]};
  float b[3];
  rt_prune_sub(v1, B.p, b);
  const float nX = rt_prune_norm(X), nbo = rt_fadd(rt_prune_norm(b), B.rho);
  const float det0 = rt_prune_dot(B.dseg, X);
  const float ad = fabsf(det0);
  const float dslack = rt_fadd(rt_fmul(rt_fadd(B.delta, B.rho), nX), rt_fmul(RT_PRUNE_G, rt_fmul(B.lenp, nX)));
  if (!(ad > rt_fmul(dslack, 1.001f))) return false;
  const float sg = det0 < 0.0f ? -1.0f : 1.0f;
  const float rhs = rt_fmul(rt_fdiv(rt_fmul(a.eps_push, rt_fadd(ad, -dslack)), B.lenp), 0.99999f);
  const float round = rt_fadd(rt_fmul(RT_PRUNE_G, rt_fmul(nX, nbo)), rt_fmul(nX, rt_fadd(rt_fmul(4e-7f, K.scale), a.eps_ulp)));
  if (a.cell.mode & RT_RESOLVE_NEAR_CENTRE) return rt_fadd(rt_fmul(rt_prune_dot(X, b), sg), round) < rhs;
  for (int k = 0; k < 8; k++) {
    float bk[3];
    rt_prune_sub(v1, K.pt[k], bk);
    if (!(rt_fadd(rt_fmul(rt_prune_dot(X, bk), sg), round) < rhs)) return false;
  }
  return true;
}

// ---- enumeration: the segment p -> c against a box of the threaded tree, inflated -------------------------------------------------
// Every point of every ray of the beam, o + s D with o in ball(p, rho) and o + D in ball(c, delta), lies within
// (1 - s) rho + s delta <= max(rho, delta) of the point p + s dseg of the segment.  A ray the literal test accepts for a
// triangle meets the padded box of the triangle's leaf, and of every node above it, to within the slack of the slab test
// (1e-5 + 4e-6 t in units of its unit direction, t <= Lp: what every walk of the render rests on, rt_bvh.cpp), that is, it has a
// point within 2e-5 + 8e-6 Lp of the box.  So the segment has a point within
//   infl = max(rho, delta) + 2e-5 + 8e-6 Lp + 1e-6 (|p|_1 + |c|_1)
// of the box in the max-norm (<= the 2-norm), the last term for p + dseg != c (dseg is rounded) and for the rounding of the
// segment's centre m = p + dseg / 2 computed here.  Segment against box by separating axes, with a = m - box centre,
// h = dseg / 2, e = the box's half extent + infl + 1e-6 |box centre| (the rounding of a: it moves the box by < 2e-7 of the
// coordinates involved): a miss is |a_i| > e_i + |h_i| on an axis, or |a_j h_k - a_k h_j| > e_j |h_k| + e_k |h_j| on a cross axis.
// The cross axes are evaluated with three roundings each, < 4e-7 (|a_j h_k| + |a_k h_j|): 1e-6 of that sum is added, and the
// right sides are rounded up (1.00001).  A miss is declared only when a comparison says so: a NaN on the beam's side enters
// the box.  A box that is not lo <= hi on every axis (NaN: an absent child) is empty.
struct RtResolveSeg {
  float m[3], h[3], ah[3], infl;
};
RT_HD static inline void rt_resolve_seg(const RtPruneBeam& B, uint32_t mode, RtResolveSeg& S) {
  for (int x = 0; x < 3; x++) {
    S.h[x] = rt_fmul(0.5f, B.dseg[x]);
    S.m[x] = rt_fadd(B.p[x], S.h[x]);
    S.ah[x] = fabsf(S.h[x]);
  }
  const float r = (mode & RT_RESOLVE_NO_INFLATE) ? 0.0f : fmaxf(B.rho, B.delta);
  S.infl = rt_fadd(rt_fadd(r, rt_fadd(2e-5f, rt_fmul(8e-6f, B.lenp))), rt_fmul(1e-6f, rt_fadd(rt_prune_norm1(B.p), rt_prune_norm1(B.c))));
}
RT_HD static inline bool rt_resolve_box_hit(const RtResolveSeg& S, const float lo[3], const float hi[3]) {
  if (!(lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2])) return false;
  float a[3], e[3];
  for (int x = 0; x < 3; x++) {
    const float bc = rt_fmul(0.5f, rt_fadd(lo[x], hi[x]));
    a[x] = rt_fadd(S.m[x], -bc);
    e[x] = rt_fmul(rt_fadd(rt_fadd(rt_fmul(0.5f, rt_fadd(hi[x], -lo[x])), S.infl), rt_fmul(1e-6f, fabsf(bc))), 1.00001f);
    if (fabsf(a[x]) > rt_fmul(rt_fadd(e[x], S.ah[x]), 1.00001f)) return false;
  }
  for (int x = 0; x < 3; x++) {
    const int j = (x + 1) % 3, k = (x + 2) % 3;
    const float ajk = rt_fmul(a[j], S.h[k]), akj = rt_fmul(a[k], S.h[j]);
    const float lhs = fabsf(rt_fadd(ajk, -akj));
    const float rhs = rt_fadd(rt_fadd(rt_fmul(e[j], S.ah[k]), rt_fmul(e[k], S.ah[j])), rt_fmul(1e-6f, rt_fadd(fabsf(ajk), fabsf(akj))));
    if (lhs > rt_fmul(rhs, 1.00001f)) return false;
  }
  return true;
}

// The walk: every leaf slot whose boxes the inflated segment meets and neither rule rejects goes to keep(slot); keep returns
// false to end the walk.  Stackless over RtThrNode (a missed box or a leaf continues at its skip link, a hit inner box at the
// next entry).  Two loops in one: the inner one steps from box to box until it stands in a leaf the segment meets, the outer
// one offers ONE slot of that leaf to the rules per turn.  On the device the lanes of a wavefront are different cells: this
// way they run the rules (some 500 instructions) side by side, each on its own next slot, instead of every lane waiting
// through the rules whenever any lane has reached a leaf; the slots come in the same order either way.  Returns false when
// the tree is not what it must be (a link that does not lead forward, a slot outside the scene or the 16-bit list format):
// the caller then leaves the list as it is.
template <class Keep>
RT_HD static inline bool rt_resolve_walk(const RtDevScene& sc, const char* base, const RtCellResolveArgs& a, const RtResolveCell& K, const RtPruneBeam& B,
                                         Keep&& keep) {
  const RtThrNode* thr = (const RtThrNode*)(base + sc.off_nodes_thr);
  const float* isect = (const float*)(base + sc.off_tri_isect);
  const uint32_t mode = a.cell.mode;
  RtResolveSeg S;
  rt_resolve_seg(B, mode, S);
  uint32_t node = 0, first = 0, k = 0, n = 0;  // slots first + k .. first + n - 1 of the current leaf are still to be offered
  for (;;) {
    while (k >= n && node < sc.n_thr) {
      const RtThrNode t = thr[node];
      uint32_t next = t.skip;
      if (rt_resolve_box_hit(S, t.lo, t.hi)) {
        if ((t.leaf >> 24) == 0u) next = node + 1u;
        else first = t.leaf & 0xFFFFFFu, n = t.leaf >> 24, k = 0u;
      }
      if (next <= node) return false;
      node = next;
    }
    if (k >= n) return true;  // the tree is exhausted
    const uint32_t slot = first + k;
    k++;
    if (slot >= sc.n_slots || slot >= RT_PRUNE_LIST_OVERFLOW) return false;
    const float* q = isect + 12u * (size_t)slot;
    if (rt_prune_rule(B, q, mode & 0xFFu)) continue;
    if (!(mode & RT_RESOLVE_NO_NEAR) && rt_resolve_near_rule(B, K, a, q)) continue;
    if (!keep(slot)) return true;
  }
}

// whether the stage has anything to do for the cell whose n_lights lists start at `list`
RT_HD static inline bool rt_cell_resolve_wanted(const uint16_t* list, uint32_t n_lights) {
  bool any = false;
  for (uint32_t l = 0; l < n_lights && l < 8u; l++) any = any || list[(size_t)l * RT_PRUNE_LIST_SLOTS] == RT_PRUNE_LIST_OVERFLOW;
  return any;
}

// ---- one cell: its n_lights lists (list, 8 words each) and its flags word, in place; counts: this cell's n_lights bytes or nullptr ----
RT_HD static inline void rt_cell_resolve_cell(const RtDevScene& sc, const char* base, const RtCellResolveArgs& a, uint32_t c, uint16_t* list, uint16_t* flag,
                                              uint8_t* counts) {
  if (!rt_cell_resolve_wanted(list, sc.n_lights)) return;
  RtResolveCell K;
  if (!rt_resolve_cell_setup(sc, base, a.cell, c, K)) return;  // (never looked up)
  uint32_t fl = *flag;
  bool fl_changed = false;
  for (uint32_t l = 0; l < sc.n_lights && l < 8u; l++) {
    uint16_t* w = list + (size_t)l * RT_PRUNE_LIST_SLOTS;
    if (w[0] != RT_PRUNE_LIST_OVERFLOW) continue;
    RtPruneBeam B;
    rt_resolve_beam(sc, base, a.cell, K, l, B);
    uint32_t n = 0;
    uint16_t out[RT_CELL_WIDE_SLOTS];
    const bool count_all = counts != nullptr;
    const uint32_t room = a.wide ? RT_CELL_WIDE_SLOTS : RT_PRUNE_LIST_SLOTS;
    const bool ok = rt_resolve_walk(sc, base, a, K, B, [&](uint32_t slot) {
      if (n < room) out[n] = (uint16_t)slot;
      n++;
      return n <= room || count_all;  // one survivor more than there is room for: the list stays overflowed
    });
    if (!ok) continue;
    if (counts) counts[l] = (uint8_t)(n < 255u ? n : 255u);
    if (n > room) continue;
    if (n > RT_PRUNE_LIST_SLOTS) {  // 9 .. RT_CELL_WIDE_SLOTS: a wide record, if the pool has one left
      const uint32_t at = rt_cell_wide_take(a);
      if (at == ~0u) continue;
      for (uint32_t k = n; k < RT_CELL_WIDE_SLOTS; k++) out[k] = (uint16_t)RT_PRUNE_LIST_END;
      memcpy(__builtin_assume_aligned(a.wide + (size_t)at * RT_CELL_WIDE_SLOTS, 64), out, 2u * RT_CELL_WIDE_SLOTS);
      const uint16_t mark[RT_PRUNE_LIST_SLOTS] = {(uint16_t)RT_PRUNE_LIST_OVERFLOW, (uint16_t)RT_CELL_WIDE_MARK, (uint16_t)(at & 0x7FFFu), (uint16_t)((at >> 15) & 0x7FFFu),
                                                  (uint16_t)RT_PRUNE_LIST_END, (uint16_t)RT_PRUNE_LIST_END, (uint16_t)RT_PRUNE_LIST_END, (uint16_t)RT_PRUNE_LIST_END};
      memcpy(__builtin_assume_aligned(w, 16), mark, 16);
      continue;
    }
    for (uint32_t k = n; k < RT_PRUNE_LIST_SLOTS; k++) out[k] = (uint16_t)RT_PRUNE_LIST_END;
    memcpy(__builtin_assume_aligned(w, 16), out, 16);
    if (n == 0u) fl |= 1u << l, fl_changed = true;  // no triangle can shadow this cell for light l
  }
  if (fl_changed) *flag = (uint16_t)fl;
}

// host model (rt_cell_resolve.cpp): every cell of a packed scene, on arrays laid out as the device's.  a.cell.flag_geo is taken
// from pk; a.work is not used.
struct RtPackedScene;
void rt_cell_resolve_packed(const RtPackedScene& pk, RtCellResolveArgs a);
// the temporary memory of the device stage: bytes for a.work and (out) a.chunk_cells, given what the scene's budget leaves;
// never more than 64 MiB.  0 = nothing useful fits, the stage is left out.
size_t rt_cell_resolve_temp_bytes(uint32_t n_cells, size_t budget_left, uint32_t* chunk_cells);
// the pool of wide records: bytes (the records, then 64 bytes that hold the counter) and (out) its capacity in records, given
// what the budget leaves after flags, lists and work list: one record per eight lists at the most (half the lists' own
// bytes).  0 = no pool.
size_t rt_cell_wide_pool_bytes(uint32_t n_cells, uint32_t n_lights, size_t budget_left, uint32_t* wide_cap);
// the kernels (rt_cell_resolve.hip); returns hipError_t as int
int rt_launch_cell_resolve(const RtDevScene& sc, const RtCellResolveArgs& a, void* stream);
