// rt_view_lens.h -- the arithmetic of thin-lens camera views (rt_view_create_lens, rt_view_set_lens): the ray of a (pixel, pixel
// offset, lens offset), and the defocus criterion that adds the out-of-focus pixels of plane 0 to the mask of an adaptive frame.
//
// A lens sample is four floats: the pixel offset (sx, sy) of rt_view.h and a lens offset (lx, ly) in unit-disk coordinates.
// With aperture radius A and focus distance F (along `forward`), a, b and d0 as the pinhole camera of rt_view_ray makes them:
//   off[k] = (A lx) right[k] + (A ly) up[k],   o[k] = eye[k] + off[k],   d[k] = F d0[k] - off[k]
// so every lens sample of a pixel offset passes eye + F d0: the plane at distance F along `forward` is in focus.
//
// The defocus criterion reads plane 0 (sample 0 of every pixel; its lens offset should be (0, 0), the view through the lens
// centre).  The circle of confusion of pixel p, in pixels:
//   len = sqrt((dx dx + dy dy) + dz dz) of d0 through plane 0's pixel offset,   z = t0[p] / len   (depth along `forward`)
//   coc[p] = ((A |z - F|) / (z F)) (H / (2 tan_half)),   0 where plane 0 missed
// and pixel p joins the mask iff some pixel q of the frame with max(|dx|, |dy|) <= spread has
//   NOT coc[q] <= coc_tol   and   NOT coc[q] < max(|dx|, |dy|)          (q = p included; negated: a NaN refines)
// -- q is out of focus and its blur reaches p.  A miss has coc 0, which no tolerance >= 0 lets through, so the rule reads the
// coc plane alone.  Blur wider than `spread` pixels is cut off: the method's limit.
//
// Compiled twice, as rt_view.h is: rt_view_lens_rays_model / rt_view_defocus_model (rt_view_lens.cpp) call these functions in
// loops on the host, the kernels of rt_view_lens.hip are these functions with a thread index.  Every float operation is one
// correctly rounded multiply, add, division or square root (rt_refit.h), evaluated as written, left to right, so the host
// model is the specification of the device's rays, coc plane and mask, bit for bit.  Not part of the public ABI.
#pragma once

#include "rt_view_adapt.h"

#define RT_VIEW_LENS_MAX_SPREAD 16u
#define RT_VIEW_LENS_TILE 16u  // the spread kernel's workgroup: TILE x TILE pixels, a halo of `spread` around them in LDS

// a and b of rt_view_ray's RT_VIEW_PINHOLE for pixel (x, y) through pixel offset (sx, sy): d0 = forward + a right + b up
RT_HD static inline void rt_view_lens_ab(const RtViewCam& c, uint32_t x, uint32_t y, float sx, float sy, float& a, float& b) {
  const float w = (float)c.width, h = (float)c.height;
  const float px = rt_fadd(rt_fadd((float)x, 0.5f), sx), py = rt_fadd(rt_fadd((float)y, 0.5f), sy);
  a = rt_fmul(rt_fdiv(rt_fadd(rt_fmul(2.0f, px), -w), h), c.tan_half);
  b = rt_fmul(rt_fdiv(rt_fadd(h, -rt_fmul(2.0f, py)), h), c.tan_half);
}

// The ray of pixel (x, y) through pixel offset (sx, sy) and lens offset (lx, ly); c.kind is RT_VIEW_PINHOLE
RT_HD static inline void rt_view_lens_ray(const RtViewCam& c, uint32_t x, uint32_t y, float sx, float sy, float lx, float ly, float aperture,
                                          float focus_distance, float o[3], float d[3]) {
  float a, b;
  rt_view_lens_ab(c, x, y, sx, sy, a, b);
  const float ax = rt_fmul(aperture, lx), ay = rt_fmul(aperture, ly);
  for (int k = 0; k < 3; k++) {
    const float d0 = rt_fadd(rt_fadd(c.forward[k], rt_fmul(a, c.right[k])), rt_fmul(b, c.up[k]));
    const float off = rt_fadd(rt_fmul(ax, c.right[k]), rt_fmul(ay, c.up[k]));
    o[k] = rt_fadd(c.eye[k], off);
    d[k] = rt_fadd(rt_fmul(focus_distance, d0), -off);
  }
}

// H / (2 tan_half): pixels per unit of image-plane height at distance 1.  Computed on the host on either side.
static inline float rt_view_coc_scale(const RtViewCam& c) { return rt_fdiv((float)c.height, rt_fmul(2.0f, c.tan_half)); }

// The circle of confusion, in pixels, of what pixel (x, y) saw at distance t along plane 0's ray; 0 on a miss
RT_HD static inline float rt_view_coc_pixel(const RtViewCam& c, uint32_t x, uint32_t y, float sx, float sy, float aperture, float focus_distance,
                                            float coc_scale, bool valid, float t) {
  if (!valid) return 0.0f;
  float a, b, d0[3];
  rt_view_lens_ab(c, x, y, sx, sy, a, b);
  for (int k = 0; k < 3; k++) d0[k] = rt_fadd(rt_fadd(c.forward[k], rt_fmul(a, c.right[k])), rt_fmul(b, c.up[k]));
  const float len = rt_fsqrt(rt_fadd(rt_fadd(rt_fmul(d0[0], d0[0]), rt_fmul(d0[1], d0[1])), rt_fmul(d0[2], d0[2])));
  const float z = rt_fdiv(t, len);
  return rt_fmul(rt_fdiv(rt_fmul(aperture, fabsf(rt_fadd(z, -focus_distance))), rt_fmul(z, focus_distance)), coc_scale);
}

// Does a pixel with circle of confusion `coc` refine the pixel `dist` = max(|dx|, |dy|) away?  (dist is an integer as a float)
RT_HD static inline bool rt_view_defocus_reaches(float coc, float coc_tol, float dist) { return !(coc <= coc_tol) && !(coc < dist); }

// Is pixel (x, y) of a W x H frame picked by the defocus criterion?  No early exit: the trip counts are arguments.
RT_HD static inline bool rt_view_defocus_pixel(uint32_t x, uint32_t y, uint32_t W, uint32_t H, uint32_t spread, float coc_tol, const float* coc) {
  bool r = false;
  const int s = (int)spread;
  for (int dy = -s; dy <= s; dy++)
    for (int dx = -s; dx <= s; dx++) {
      const uint32_t qx = x + (uint32_t)dx, qy = y + (uint32_t)dy;  // (x - 1 at x == 0 wraps to a value >= W)
      const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
      if (qx < W && qy < H && rt_view_defocus_reaches(coc[(size_t)qy * W + qx], coc_tol, (float)(ax > ay ? ax : ay))) r = true;
    }
  return r;
}

// The bit-distinct (sx, sy, lx, ly) in first-occurrence order: px[2 u] / lens[2 u] = the pixel / lens offset of plane u,
// plane_of[k] = the plane of sample k.  (rt_view_dedup on 4-tuples; two planes may share a pixel offset.)
static inline uint32_t rt_view_lens_dedup(const float* samples, const float* lens_samples, uint32_t n, float px[2 * RT_VIEW_MAX_SAMPLES],
                                          float lens[2 * RT_VIEW_MAX_SAMPLES], uint8_t plane_of[RT_VIEW_MAX_SAMPLES]) {
  uint32_t nd = 0;
  for (uint32_t k = 0; k < n; k++) {
    uint32_t u = 0;
    while (u < nd && (memcmp(px + 2 * u, samples + 2 * k, 8) != 0 || memcmp(lens + 2 * u, lens_samples + 2 * k, 8) != 0)) u++;
    if (u == nd) {
      memcpy(px + 2 * nd, samples + 2 * k, 8), memcpy(lens + 2 * nd, lens_samples + 2 * k, 8);
      nd++;
    }
    plane_of[k] = (uint8_t)u;
  }
  return nd;
}

// ---- the device-free half (rt_view_lens.cpp) -----------------------------------------------------------------------------------
// RT_OK, or RT_ERR_INVALID_ARG with a message naming `fn`; before any HIP call
int rt_view_lens_check_desc(const rt_view_desc* d, const float* lens_samples, const char* fn);  // rt_view_check_desc + the lens table
int rt_view_check_lens(const rt_view_lens* l, const char* fn);
// is the defocus criterion on?  (A > 0 and a finite tolerance)
static inline bool rt_view_defocus_active(float aperture, float coc_tol) { return aperture > 0.0f && rt_finite(coc_tol); }

// ---- the device half (rt_view_lens.hip) ----------------------------------------------------------------------------------------
// Each returns hipError_t as int; allocates nothing, reads nothing back.  px / lens: DEVICE tables of n_distinct offset pairs.
int rt_launch_view_lens_rays(const RtViewCam& cam, const float* px, const float* lens, uint32_t n_distinct, float aperture, float focus_distance,
                             float* origin, float* direction, void* stream);
// the generator of pass 2: rt_view_lens_ray for ray (u, p) with u >= 1 and mask[p] set, every other ray dead
int rt_launch_view_lens_sparse_rays(const RtViewCam& cam, const float* px, const float* lens, uint32_t n_distinct, float aperture,
                                    float focus_distance, const uint8_t* mask, float* origin, float* direction, void* stream);
// coc[p] of plane 0 (px: its pixel offset is the table's first pair); then mask[p] = 1 (also in mask_out when given) for the
// pixels the criterion picks, *n_refined += the number of pixels it ADDED (those not set before)
int rt_launch_view_coc(const RtViewCam& cam, const float* px, float aperture, float focus_distance, const uint8_t* valid0, const float* t0,
                       float* coc, void* stream);
int rt_launch_view_defocus_spread(uint32_t width, uint32_t height, uint32_t spread, float coc_tol, const float* coc, uint8_t* mask,
                                  uint8_t* mask_out, uint32_t* n_refined, void* stream);
