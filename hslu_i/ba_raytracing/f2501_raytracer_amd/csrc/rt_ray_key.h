// rt_ray_key.h -- the sort key of a ray order (rt_ray_order*): which rays of a batch should share a wavefront.
//
// The key is a Morton code of the ray's origin and normalised direction, quantised inside the bounds of the batch's live
// rays; origins are its major part.  A camera whose origins differ per pixel gives its bits to the image plane, a pinhole
// (one origin) gives all of them to the direction.  The major part is coded in row-major blocks of about 4096 rays with
// the Morton code inside (rt_key_frame says why).  Nothing of the scene takes part: an order belongs to a batch.
//
// Compiled twice, as rt_refit.h is: rt_ray_order_model (rt_ray_order.cpp) calls these functions in loops on the host, the
// kernels of rt_order.hip are these functions with a thread index.  Every float operation is one correctly rounded
// multiply, add, division or square root on either side (rt_refit.h: rt_fmul / rt_fadd / rt_fdiv / rt_fsqrt), so the host
// model is the specification of the device keys, bit for bit.  Not part of the public ABI.
#pragma once

#include "rt_refit.h"

#define RT_KEY_DEAD 0xFFFFFFFFu  // a dead ray: sorts behind every live one (a live key has at most 30 bits)
#define RT_KEY_BITS 30u          // bits of a live key
#define RT_KEY_AXIS_BITS 10u     // most bits one axis gets
#define RT_KEY_BLOCK_RAYS_LOG2 12u // rays a row-major block of the key aims to hold: 4096 (64 x 64 pixels measured best, 16 x 16 .. 128 x 128)
#define RT_KEY_ORIGIN_BITS_3D 5u // default per origin axis when three origin axes share the key with directions

// min / max of the six key coordinates {o.x, o.y, o.z, n.x, n.y, n.z} over the live rays, and their number
struct RtKeyBounds {
  float lo[6], hi[6];
  uint32_t n_live;
};

// What a key is quantised with: per coordinate its lower bound, its extent and 2^bits (bits = 0: the axis takes no part),
// origins in [0, 3), directions in [3, 6).
struct RtKeyFrame {
  float lo[6], extent[6], scale[6];
  uint32_t bits[6];
  uint32_t n_live, origin_bits, direction_bits, n_origin_axes, n_direction_axes;
  uint32_t low_bits;  // of each axis of the major group (origins, or directions when no origin axis is active): see rt_key_frame
};

RT_HD static inline void rt_key_bounds_clear(RtKeyBounds& b) {
  for (int a = 0; a < 6; a++) b.lo[a] = INFINITY, b.hi[a] = -INFINITY;
  b.n_live = 0u;
}

// The six coordinates of ray (o, d): n = d * (1 / sqrt(d.d)).  False for a dead ray -- the rule of the queries: a
// direction that normalises to a non-finite vector (zero length, a NaN or inf component) or a non-finite origin.
RT_HD static inline bool rt_key_coords(const float* o, const float* d, float c[6]) {
  const float dd = rt_fadd(rt_fadd(rt_fmul(d[0], d[0]), rt_fmul(d[1], d[1])), rt_fmul(d[2], d[2]));
  const float inv = rt_fdiv(1.0f, rt_fsqrt(dd));
  c[0] = o[0], c[1] = o[1], c[2] = o[2];
  c[3] = rt_fmul(d[0], inv), c[4] = rt_fmul(d[1], inv), c[5] = rt_fmul(d[2], inv);
  bool live = true;
  for (int a = 0; a < 6; a++) live = live && rt_finite(c[a]);
  return live;
}

RT_HD static inline void rt_key_bounds_add(RtKeyBounds& b, const float c[6]) {
  for (int a = 0; a < 6; a++) b.lo[a] = rt_min_keep(b.lo[a], c[a]), b.hi[a] = rt_max_keep(b.hi[a], c[a]);
  b.n_live++;
}

RT_HD static inline void rt_key_bounds_merge(RtKeyBounds& b, const RtKeyBounds& x) {
  for (int a = 0; a < 6; a++) b.lo[a] = rt_min_keep(b.lo[a], x.lo[a]), b.hi[a] = rt_max_keep(b.hi[a], x.hi[a]);
  b.n_live += x.n_live;
}

// The bit split.  An axis is active when max > min.  Each active origin axis gets ob = origin_bits, or by default
// min(10, 30 / n_origin_axes) -- 5 when all three origin axes and some direction axis are active; each active direction axis db = min(10, (30 - ob n_origin_axes) / n_direction_axes).
RT_HD static inline void rt_key_frame(const RtKeyBounds& b, uint32_t origin_bits, RtKeyFrame& f) {
  uint32_t no = 0, nd = 0;
  bool active[6];
  for (int a = 0; a < 6; a++) {
    active[a] = b.n_live > 0u && b.hi[a] > b.lo[a];
    if (active[a]) (a < 3 ? no : nd)++;
  }
  uint32_t ob = 0, db = 0;
  if (no) {
    ob = origin_bits ? origin_bits : RT_KEY_BITS / no;
    if (ob > RT_KEY_AXIS_BITS) ob = RT_KEY_AXIS_BITS;
    // three origin axes would take all 30 bits and leave the direction unused: measured on 2^22 random rays, 5 + 5 traces
    // 2 % faster than 10 + 0 and 7 + 3 (profiles/ray_order.md), so the directions get the other half
    if (!origin_bits && no == 3u && nd) ob = RT_KEY_ORIGIN_BITS_3D;
  }
  if (nd) {
    db = (RT_KEY_BITS - ob * no) / nd;
    if (db > RT_KEY_AXIS_BITS) db = RT_KEY_AXIS_BITS;
  }
  for (int a = 0; a < 6; a++) {
    const uint32_t bits = active[a] ? (a < 3 ? ob : db) : 0u;
    f.bits[a] = bits;
    f.lo[a] = active[a] ? b.lo[a] : 0.0f;
    f.extent[a] = active[a] ? rt_fadd(b.hi[a], -b.lo[a]) : 1.0f;  // (inf for bounds more than FLT_MAX apart: every cell is cell 0)
    f.scale[a] = (float)(1u << bits);
  }
  f.n_live = b.n_live, f.origin_bits = ob, f.direction_bits = db, f.n_origin_axes = no, f.n_direction_axes = nd;
  // Blocks.  A Morton code all the way up walks the batch in nested squares, and a camera batch traced in that order ran
  // SLOWER than in row-major strips with direct light, whatever the lanes inside a wavefront were; blocks of rays in
  // row-major order with the Morton code inside them ran faster than either (profiles/ray_order.md).  So the major group's
  // cells split into a high part, which orders the blocks row-major (last axis first), and `low_bits` per axis, the Morton
  // code inside a block -- as many as make a block hold about 2^RT_KEY_BLOCK_RAYS_LOG2 rays if the live rays filled the
  // group's cells evenly.
  const uint32_t m = no ? no : nd, gb = no ? ob : db;
  uint32_t low = gb;
  if (m) {
    uint32_t rays_log2 = 0u;
    while (rays_log2 < 31u && (1u << rays_log2) < b.n_live) rays_log2++;
    const uint32_t cells_log2 = gb * m;
    const uint32_t block_log2 = cells_log2 + RT_KEY_BLOCK_RAYS_LOG2 > rays_log2 ? cells_log2 + RT_KEY_BLOCK_RAYS_LOG2 - rays_log2 : 0u;
    low = (block_log2 + m - 1u) / m;
    if (low > gb) low = gb;
  }
  f.low_bits = low;
}

// q(x) = min(2^b - 1, floor((x - lo) / (hi - lo) 2^b)); 0 where the quotient is not a number (inf / inf)
RT_HD static inline uint32_t rt_key_cell(const RtKeyFrame& f, int a, float x) {
  const float v = rt_fmul(rt_fdiv(rt_fadd(x, -f.lo[a]), f.extent[a]), f.scale[a]);
  if (v >= f.scale[a]) return (1u << f.bits[a]) - 1u;
  return v >= 0.0f ? (uint32_t)v : 0u;
}

// Morton code of the cells of axes first .. first + 2, of which `m` are active (the others have cell 0): most significant
// bit first, x y z round robin -- bit l of the j-th active axis lands at position l m + (m - 1 - j)
RT_HD static inline uint32_t rt_key_morton(const RtKeyFrame& f, int first, uint32_t m, const uint32_t q[3]) {
  uint32_t key = 0u, j = 0u;
  for (int a = 0; a < 3; a++) {
    if (!f.bits[first + a]) continue;
    uint32_t spread = 0u;
    for (uint32_t l = 0; l < RT_KEY_AXIS_BITS; l++) spread |= ((q[a] >> l) & 1u) << (l * m);
    key |= spread << (m - 1u - j);
    j++;
  }
  return key;
}

// the major group's code: its blocks row-major (the last active axis is the slowest), the Morton code of the low bits inside
RT_HD static inline uint32_t rt_key_blocks(const RtKeyFrame& f, int first, uint32_t m, uint32_t bits, const uint32_t q[3]) {
  const uint32_t low = f.low_bits, mask = (1u << low) - 1u;
  uint32_t hi = 0u, lo[3];
  for (int a = 2; a >= 0; a--) {
    lo[a] = q[a] & mask;
    if (f.bits[first + a]) hi = (hi << (bits - low)) | (q[a] >> low);
  }
  return (hi << (low * m)) | rt_key_morton(f, first, m, lo);
}

RT_HD static inline uint32_t rt_key_of(const RtKeyFrame& f, const float* o, const float* d) {
  float c[6];
  if (!rt_key_coords(o, d, c)) return RT_KEY_DEAD;
  uint32_t q[6];
  for (int a = 0; a < 6; a++) q[a] = f.bits[a] ? rt_key_cell(f, a, c[a]) : 0u;
  if (!f.n_origin_axes) return rt_key_blocks(f, 3, f.n_direction_axes, f.direction_bits, q + 3);
  return (rt_key_blocks(f, 0, f.n_origin_axes, f.origin_bits, q) << (f.direction_bits * f.n_direction_axes)) |
         rt_key_morton(f, 3, f.n_direction_axes, q + 3);
}

// ---- the device-free half (rt_ray_order.cpp) --------------------------------------------------------------------------------
// RT_OK, or RT_ERR_INVALID_ARG with a message: `perm` is not a permutation of [0, n) (rt_ray_order_set)
int rt_check_permutation(const uint32_t* perm, uint32_t n);
// The host model of rt_ray_order_build: keys[i] = the key of ray i, perm = the rays sorted by key, STABLY (as the device's
// sort: each of its passes is stable, so rays of equal key stay in index order there too).  Every output nullable.
int rt_ray_order_model(const float* origin, const float* direction, uint32_t n, uint32_t origin_bits, uint32_t* keys, uint32_t* perm,
                       rt_ray_order_info* info);

// ---- the device half (rt_order.hip) --------------------------------------------------------------------------------------------
#define RT_ORDER_TILE 4096u         // keys per workgroup of a sort pass
#define RT_ORDER_BOUNDS_WGS 1024u   // most workgroups of the bounds reduction
#define RT_ORDER_SCAN_BLOCKS 4096u  // most block sums the one-workgroup step of the histogram scan takes
// most rays of an order: 256 counts per tile, 2048 counts per scan block, RT_ORDER_SCAN_BLOCKS blocks = 2^27
#define RT_ORDER_MAX_RAYS (RT_ORDER_SCAN_BLOCKS * 2048u / 256u * RT_ORDER_TILE)
// the device arrays of one order, each for `capacity` rays: the key of ray i, two (key, index) pairs the passes alternate
// between, the per-(digit, workgroup) histogram of a pass and its block sums, the partial bounds and the frame the keys are
// quantised with
struct RtOrderWs {
  uint32_t *keys, *key_a, *key_b, *idx_a, *idx_b, *hist, *sums;
  RtKeyBounds* partial;
  RtKeyFrame* frame;
};
// Enqueues bounds -> frame -> keys -> four stable 8-bit radix passes; the sorted indices end in w.idx_b.  n > 0.  Returns
// hipError_t as int; allocates nothing, reads nothing back.
int rt_launch_order_build(const RtOrderWs& w, const float* origin, const float* direction, uint32_t n, uint32_t origin_bits, void* stream);
