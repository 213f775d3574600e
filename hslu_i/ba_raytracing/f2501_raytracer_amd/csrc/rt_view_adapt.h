// rt_view_adapt.h -- the arithmetic of adaptive camera views (rt_render_view_adaptive*): which pixels of a frame are refined
// with all their samples, and what a pixel is that is not.
//
// An adaptive frame traces sample 0 of every pixel (plane 0 of the view's sample-major layout) and the other distinct
// samples only of the pixels the refine rule picks from plane 0.  A refined pixel is the full view's pixel: the same rays
// with the same indices, hence the same light-cloud keys, resolved by the same formula.  An unrefined pixel is that
// formula with every sample reading plane 0: the brightness the full resolve gives a pixel whose samples all agree.
//
// Compiled twice, as rt_view.h is: rt_view_refine_model / rt_view_resolve_adaptive_model (rt_view_adapt.cpp) call these
// functions in loops on the host, the kernels of rt_view_adapt.hip are these functions with a thread index.  Every float
// operation is one correctly rounded add or multiply (rt_refit.h), so the host model is the specification of the device's
// mask and pixels, bit for bit.  Not part of the public ABI.
#pragma once

#include "rt_view.h"

#define RT_REFINE_KNOWN (RT_REFINE_ID | RT_REFINE_DEPTH | RT_REFINE_COLOUR | RT_REFINE_EVERY)
#define RT_PARTITION_WG 256u  // entries per workgroup of the partition: one count per workgroup

// Does the edge between pixel p and its neighbour q refine?  (symmetric in p and q; comparisons negated: a NaN refines)
RT_HD static inline bool rt_view_refine_edge(uint32_t p, uint32_t q, uint32_t criteria, float colour_tol, float depth_tol, const float* rgb0,
                                             const uint8_t* valid0, const int32_t* id0, const float* t0) {
  const bool vp = valid0[p] != 0u, vq = valid0[q] != 0u;
  bool r = vp != vq;
  if ((criteria & RT_REFINE_ID) && id0[p] != id0[q]) r = true;
  if (vp && vq) {
    if (criteria & RT_REFINE_DEPTH) {
      const float tp = t0[p], tq = t0[q];
      if (!(fabsf(rt_fadd(tp, -tq)) <= rt_fmul(depth_tol, fminf(tp, tq)))) r = true;
    }
    if (criteria & RT_REFINE_COLOUR)
      for (int k = 0; k < 3; k++)
        if (!(fabsf(rt_fadd(rgb0[3u * (size_t)p + k], -rgb0[3u * (size_t)q + k])) <= colour_tol)) r = true;
  }
  return r;
}

// Is pixel (x, y) of a W x H frame refined?  Reads plane 0 (sample 0 of every pixel) at the pixel and at its up to 8
// neighbours inside the frame.  RT_REFINE_EVERY: always; no criterion: never.  No early exit: the trip counts are constants.
RT_HD static inline bool rt_view_refine_pixel(uint32_t x, uint32_t y, uint32_t W, uint32_t H, uint32_t criteria, float colour_tol, float depth_tol,
                                              const float* rgb0, const uint8_t* valid0, const int32_t* id0, const float* t0) {
  if (criteria & RT_REFINE_EVERY) return true;
  if (!(criteria & (RT_REFINE_ID | RT_REFINE_DEPTH | RT_REFINE_COLOUR))) return false;
  const uint32_t p = y * W + x;
  bool r = false;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int dy = -1; dy <= 1; dy++) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int dx = -1; dx <= 1; dx++) {
      if (dx == 0 && dy == 0) continue;
      const uint32_t qx = x + (uint32_t)dx, qy = y + (uint32_t)dy;  // (x - 1 at x == 0 wraps to a value >= W)
      if (qx < W && qy < H && rt_view_refine_edge(p, qy * W + qx, criteria, colour_tol, depth_tol, rgb0, valid0, id0, t0)) r = true;
    }
  }
  return r;
}

// Sample u of pixel p: plane 0 lives in the base planes (pass 1), the others in the per-ray planes (pass 2)
RT_HD static inline void rt_view_take_adaptive(bool first, uint32_t u, uint32_t p, uint32_t n_pixels, float scale, const float* rgb0,
                                               const uint8_t* valid0, const float* rgb, const uint8_t* valid, float acc[3], bool& any) {
  if (u == 0u)
    rt_view_take(first, p, scale, rgb0, valid0, acc, any);
  else
    rt_view_take(first, u * n_pixels + p, scale, rgb, valid, acc, any);
}

// rt_view_resolve_pixel for an adaptive frame: a refined pixel reads its samples through plane_of, an unrefined one reads
// plane 0 for every sample (n_samples and scale unchanged).  id and t are those of plane 0.
RT_HD static inline void rt_view_resolve_adaptive_pixel(uint32_t p, uint32_t n_pixels, uint32_t n_samples, float scale, const uint8_t* plane_of,
                                                        bool refined, const float* rgb0, const uint8_t* valid0, const int32_t* id0, const float* t0,
                                                        const float* rgb, const uint8_t* valid, float* o_rgb, uint8_t* o_valid, int32_t* o_id,
                                                        float* o_t, uint32_t* o_argb) {
  float colour[3] = {0.0f, 0.0f, 0.0f};
  bool any = false;
  if (n_samples == 1u) {
    if (valid0[p]) {
      any = true;
      for (int k = 0; k < 3; k++) colour[k] = rgb0[3u * (size_t)p + k];
    }
  } else {
    float first[8][3], rest[8][3];
    for (int l = 0; l < 8; l++)
      for (int k = 0; k < 3; k++) first[l][k] = rest[l][k] = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t l = 0; l < 8u; l++)
      if (l < n_samples) rt_view_take_adaptive(true, refined ? (uint32_t)plane_of[l] : 0u, p, n_pixels, scale, rgb0, valid0, rgb, valid, first[l], any);
    for (uint32_t base = 8u; base < n_samples; base += 8u) {  // (uniform: the trip count is an argument)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (uint32_t l = 0; l < 8u; l++)
        if (base + l < n_samples)
          rt_view_take_adaptive(false, refined ? (uint32_t)plane_of[base + l] : 0u, p, n_pixels, scale, rgb0, valid0, rgb, valid, rest[l], any);
    }
    float lane[8][3];
    for (int l = 0; l < 8; l++)
      for (int k = 0; k < 3; k++) lane[l][k] = rt_fadd(rest[l][k], first[l][k]);
    for (int k = 0; k < 3; k++)
      colour[k] = rt_fadd(rt_fadd(rt_fadd(lane[0][k], lane[4][k]), rt_fadd(lane[2][k], lane[6][k])),
                          rt_fadd(rt_fadd(lane[1][k], lane[5][k]), rt_fadd(lane[3][k], lane[7][k])));
  }
  if (o_rgb)
    for (int k = 0; k < 3; k++) o_rgb[3u * (size_t)p + k] = any ? colour[k] : 0.0f;
  if (o_valid) o_valid[p] = any ? 1u : 0u;
  if (o_id) o_id[p] = id0[p];
  if (o_t) o_t[p] = t0[p];
  if (o_argb && any) o_argb[p] = rt_view_pack(colour);
}

// Is ray i = u n_pixels + p of the pass-2 batch live?  (the predicate the order is partitioned by)
RT_HD static inline bool rt_view_ray_live(uint32_t i, uint32_t n_pixels, const uint8_t* mask) { return i >= n_pixels && mask[i % n_pixels] != 0u; }

// ---- the workspace of an adaptive view (rt_view_enable_adaptive) ---------------------------------------------------------------
// base planes: what pass 1 writes (21 bytes per pixel); mask; perm2: the view's order partitioned by liveness; order0: the
// first n_pixels entries of the view's order partitioned by "ray < n_pixels" (the order of pass 1); flags: the predicate per
// entry of the order being partitioned; counts: set flags per RT_PARTITION_WG entries, one more for the total, rounded up to
// the scan's multiple of 8; sums: the scan's block sums; n_refined: one word
struct RtViewAdaptWs {
  float *rgb0, *t0;
  int32_t* id0;
  uint8_t *valid0, *mask, *flags;
  uint32_t *perm2, *order0, *counts, *sums, *n_refined;
};
static inline size_t rt_partition_counts(size_t n) { return ((n + RT_PARTITION_WG - 1u) / RT_PARTITION_WG + 1u + 7u) & ~(size_t)7u; }
// the parts of `lay` (an RtArena, rt_host.h); scan_blocks: RT_ORDER_SCAN_BLOCKS (rt_ray_key.h), the scan's block sums
template <class Arena>
static inline void rt_view_adapt_ws_add(Arena& lay, size_t n_pixels, size_t n_rays, size_t scan_blocks, RtViewAdaptWs* ws) {
  lay.add(n_pixels * 12, &ws->rgb0), lay.add(n_pixels * 4, &ws->id0), lay.add(n_pixels * 4, &ws->t0), lay.add(n_pixels, &ws->valid0);
  lay.add(n_pixels, &ws->mask), lay.add(n_rays * 4, &ws->perm2), lay.add(n_pixels * 4, &ws->order0), lay.add(n_rays, &ws->flags);
  lay.add(rt_partition_counts(n_rays) * 4, &ws->counts), lay.add(scan_blocks * 4, &ws->sums), lay.add(4, &ws->n_refined);
}

// The host model of the partition: out = the entries of perm_in (nullptr: the identity) whose flag is set, in their order,
// then the others in theirs; only the first n_out entries are written.  flags[k] belongs to ENTRY k, not to ray perm_in[k].
static inline uint32_t rt_partition_model(const uint32_t* perm_in, const uint8_t* flags, uint32_t n, uint32_t n_out, uint32_t* perm_out) {
  uint32_t n_set = 0, at = 0;
  for (uint32_t k = 0; k < n; k++) n_set += flags[k] ? 1u : 0u;
  uint32_t rest = n_set;
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t pos = flags[k] ? at++ : rest++;
    if (pos < n_out) perm_out[pos] = perm_in ? perm_in[k] : k;
  }
  return n_set;
}

// ---- the device-free half (rt_view_adapt.cpp) ---------------------------------------------------------------------------------------
// RT_OK, or RT_ERR_INVALID_ARG with a message naming `fn`; before any HIP call
int rt_view_check_refine(const rt_view_refine* r, const char* fn);

// ---- the device half (rt_view_adapt.hip) --------------------------------------------------------------------------------------------
// Each returns hipError_t as int; allocates nothing, reads nothing back.
// mask[p] = refined (also into mask_out when given); *n_refined += the number of set entries (the caller cleared it)
int rt_launch_view_classify(uint32_t width, uint32_t height, uint32_t criteria, float colour_tol, float depth_tol, const RtViewAdaptWs& w,
                            uint8_t* mask_out, void* stream);
// the generator of pass 2: rt_view_ray for ray (u, p) with u >= 1 and mask[p] set, every other ray dead (origin and direction 0)
int rt_launch_view_sparse_rays(const RtViewCam& cam, const float* distinct, uint32_t n_distinct, const uint8_t* mask, float* origin,
                               float* direction, void* stream);
// flags[k] for entry k of perm_in (nullptr: the identity): mask given: rt_view_ray_live(ray); mask == nullptr: ray < n_pixels
int rt_launch_view_flags(const uint32_t* perm_in, uint32_t n, uint32_t n_pixels, const uint8_t* mask, uint8_t* flags, void* stream);
// rt_partition_model on the device: counts [rt_partition_counts(n)], sums [RT_ORDER_SCAN_BLOCKS], perm_out [n_out]; n > 0
int rt_launch_partition(const uint32_t* perm_in, const uint8_t* flags, uint32_t n, uint32_t n_out, uint32_t* counts, uint32_t* sums,
                        uint32_t* perm_out, void* stream);
int rt_launch_view_resolve_adaptive(uint32_t n_pixels, uint32_t n_samples, const uint8_t* plane_of, const RtViewAdaptWs& w, const float* rgb,
                                    const uint8_t* valid, const rt_ray_radiance& out, void* stream);
