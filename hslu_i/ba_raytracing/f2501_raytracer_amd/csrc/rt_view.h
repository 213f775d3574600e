// rt_view.h -- the arithmetic of device-side camera views (rt_view*, rt_render_view*): the ray of a (pixel, sample) and the
// resolve of a pixel's sample colours into the pixel.
//
// Compiled twice, as rt_refit.h and rt_ray_key.h are: rt_view_rays_model / rt_view_resolve_model (rt_view.cpp) call these
// functions in loops on the host, the kernels of rt_view.hip are these functions with a thread index.  Every float
// operation is one correctly rounded multiply, add or division on either side (rt_refit.h: rt_fmul / rt_fadd / rt_fdiv), so
// the host model is the specification of the device's rays and pixels, bit for bit.  Not part of the public ABI.
#pragma once

#include "rt_refit.h"

#define RT_VIEW_MAX_SAMPLES 64u
#define RT_VIEW_WG 256u

// What the generator reads: rt_view_camera and the frame of the view, by value (a kernel argument)
struct RtViewCam {
  uint32_t kind, width, height, n_pixels;
  float eye[3], right[3], up[3], forward[3], tan_half;
  float focus[3], fw, fh;
};

// The ray of pixel (x, y) through sample offset (sx, sy).
// RT_VIEW_PINHOLE: origin = eye, direction = forward + a right + b up with
//   a = (2 (x + 0.5 + sx) - W) / H tan_half,  b = (H - 2 (y + 0.5 + sy)) / H tan_half        (offsets in pixels, row 0 on top)
// RT_VIEW_REFERENCE: coords = (float(x) fw, float(y) fh, 0), origin = coords + (sx, sy, 0), direction = coords - focus
//   (offsets in the units of rt_params.aa_offsets; the oracle's render_pixel)
RT_HD static inline void rt_view_ray(const RtViewCam& c, uint32_t x, uint32_t y, float sx, float sy, float o[3], float d[3]) {
  if (c.kind == RT_VIEW_PINHOLE) {
    const float w = (float)c.width, h = (float)c.height;
    const float px = rt_fadd(rt_fadd((float)x, 0.5f), sx), py = rt_fadd(rt_fadd((float)y, 0.5f), sy);
    const float a = rt_fmul(rt_fdiv(rt_fadd(rt_fmul(2.0f, px), -w), h), c.tan_half);
    const float b = rt_fmul(rt_fdiv(rt_fadd(h, -rt_fmul(2.0f, py)), h), c.tan_half);
    for (int k = 0; k < 3; k++) {
      o[k] = c.eye[k];
      d[k] = rt_fadd(rt_fadd(c.forward[k], rt_fmul(a, c.right[k])), rt_fmul(b, c.up[k]));
    }
  } else {
    const float cx = rt_fmul((float)x, c.fw), cy = rt_fmul((float)y, c.fh);
    o[0] = rt_fadd(cx, sx), o[1] = rt_fadd(cy, sy), o[2] = 0.0f;
    d[0] = rt_fadd(cx, -c.focus[0]), d[1] = rt_fadd(cy, -c.focus[1]), d[2] = rt_fadd(0.0f, -c.focus[2]);
  }
}

// palette Rgb<f32> -> 0xFFRRGGBB: clamp to [0, 1] (NaN -> 0), x 255, round half to even (OutputColorEncoder::to_output)
RT_HD static inline uint32_t rt_view_u8(float x) {
  float c = x > 0.0f ? x : 0.0f;
  c = c < 1.0f ? c : 1.0f;
  return (uint32_t)rintf(rt_fmul(c, 255.0f));
}
RT_HD static inline uint32_t rt_view_pack(const float c[3]) {
  return 0xFF000000u | (rt_view_u8(c[0]) << 16) | (rt_view_u8(c[1]) << 8) | rt_view_u8(c[2]);
}

// 1 / (8 ceil(n / 8)): the weight of one sample (raytracer_renderer.rs:936-937).  Computed on the host on either side.
static inline float rt_view_scale(uint32_t n_samples) { return 1.0f / (float)(((n_samples + 7u) / 8u) * 8u); }

// One sample of packet lane `l`: `acc` takes it when it is valid.  first: packet 0 (stored), else summed `cs + acc`.
RT_HD static inline void rt_view_take(bool first, uint32_t i, float scale, const float* rgb, const uint8_t* valid, float acc[3], bool& any) {
  if (!valid[i]) return;
  any = true;
  for (int k = 0; k < 3; k++) {
    const float cs = rt_fmul(rgb[3u * (size_t)i + k], scale);
    acc[k] = first ? cs : rt_fadd(cs, acc[k]);
  }
}

// The pixel p of a frame of n_pixels from the per-ray planes of its n_distinct sample planes (ray u n_pixels + p), the
// reference's antialiased_raytrace accumulation over all n_samples, repeats read through plane_of:
//   valid sample k: cs = c scale; k < 8: first[k] = cs, else rest[k & 7] = cs + rest[k & 7]
//   lane[l] = rest[l] + first[l];  colour = ((l0 + l4) + (l2 + l6)) + ((l1 + l5) + (l3 + l7))
// n_samples == 1: the sample's colour, unscaled.  Every output nullable; argb is left alone when no sample is valid.
RT_HD static inline void rt_view_resolve_pixel(uint32_t p, uint32_t n_pixels, uint32_t n_samples, float scale, const uint8_t* plane_of,
                                               const float* rgb, const uint8_t* valid, const int32_t* id, const float* t, float* o_rgb,
                                               uint8_t* o_valid, int32_t* o_id, float* o_t, uint32_t* o_argb) {
  float colour[3] = {0.0f, 0.0f, 0.0f};
  bool any = false;
  if (n_samples == 1u) {
    if (valid[p]) {
      any = true;
      for (int k = 0; k < 3; k++) colour[k] = rgb[3u * (size_t)p + k];
    }
  } else {
    float first[8][3], rest[8][3];
    for (int l = 0; l < 8; l++)
      for (int k = 0; k < 3; k++) first[l][k] = rest[l][k] = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t l = 0; l < 8u; l++)
      if (l < n_samples) rt_view_take(true, (uint32_t)plane_of[l] * n_pixels + p, scale, rgb, valid, first[l], any);
    for (uint32_t base = 8u; base < n_samples; base += 8u) {  // (uniform: the trip count is an argument)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (uint32_t l = 0; l < 8u; l++)
        if (base + l < n_samples) rt_view_take(false, (uint32_t)plane_of[base + l] * n_pixels + p, scale, rgb, valid, rest[l], any);
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
  if (o_id) o_id[p] = id[p];  // sample 0 is distinct sample 0: -1 / +inf on its miss, as the trace wrote them
  if (o_t) o_t[p] = t[p];
  if (o_argb && any) o_argb[p] = rt_view_pack(colour);
}

// ---- the device-free half (rt_view.cpp) --------------------------------------------------------------------------------------
// the bit-distinct sample offsets in first-occurrence order: distinct[2 u], plane_of[k] = the distinct sample of sample k
static inline uint32_t rt_view_dedup(const float* samples, uint32_t n, float distinct[2 * RT_VIEW_MAX_SAMPLES], uint8_t plane_of[RT_VIEW_MAX_SAMPLES]) {
  uint32_t nd = 0;
  for (uint32_t k = 0; k < n; k++) {
    uint32_t u = 0;
    while (u < nd && memcmp(distinct + 2 * u, samples + 2 * k, 8) != 0) u++;
    if (u == nd) memcpy(distinct + 2 * nd++, samples + 2 * k, 8);
    plane_of[k] = (uint8_t)u;
  }
  return nd;
}
// RT_OK, or RT_ERR_INVALID_ARG with a message naming `fn`; before any HIP call
int rt_view_check_desc(const rt_view_desc* d, const char* fn);
int rt_view_check_camera(const rt_view_camera* c, const char* fn);
RtViewCam rt_view_cam_of(const rt_view_desc& d, const rt_view_camera& c);

// ---- the device half (rt_view.hip) ---------------------------------------------------------------------------------------------
// Enqueue the generator (n_distinct planes of cam.n_pixels rays; `distinct` is a DEVICE table of n_distinct offset pairs)
// and the resolve (plane_of: DEVICE, n_samples bytes).  Return hipError_t as int; allocate nothing, read nothing back.
int rt_launch_view_rays(const RtViewCam& cam, const float* distinct, uint32_t n_distinct, float* origin, float* direction, void* stream);
int rt_launch_view_resolve(uint32_t n_pixels, uint32_t n_samples, const uint8_t* plane_of, const float* rgb, const uint8_t* valid,
                           const int32_t* id, const float* t, const rt_ray_radiance& out, void* stream);
