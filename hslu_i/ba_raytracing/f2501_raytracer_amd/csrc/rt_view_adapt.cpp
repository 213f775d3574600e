// rt_view_adapt.cpp -- the device-free half of adaptive camera views: the check of an rt_view_refine and the host models of
// the refine rule and of the adaptive resolve (the functions of rt_view_adapt.h in loops).  No HIP call: links without a
// device.  The handle and the launch sequence are in rt_view.cpp.
#include <hip/hip_runtime_api.h>  // (types only: rt_internal.h names float4 / uint4)

#include "rt_scene_pack.h"  // rt_fail
#include "rt_view_adapt.h"

int rt_view_check_refine(const rt_view_refine* r, const char* fn) {
  if (!r) return rt_fail(RT_ERR_INVALID_ARG, "%s: null refine rule", fn);
  if (r->abi_version != RT_ABI_VERSION) return rt_fail(RT_ERR_INVALID_ARG, "%s: rt_view_refine.abi_version %u != %u", fn, r->abi_version, RT_ABI_VERSION);
  if (r->criteria & ~RT_REFINE_KNOWN) return rt_fail(RT_ERR_INVALID_ARG, "%s: unknown criteria bits 0x%x", fn, r->criteria & ~RT_REFINE_KNOWN);
  if (!(r->colour_tol >= 0.0f)) return rt_fail(RT_ERR_INVALID_ARG, "%s: colour_tol %g is negative or not a number", fn, (double)r->colour_tol);
  if (!(r->depth_tol >= 0.0f)) return rt_fail(RT_ERR_INVALID_ARG, "%s: depth_tol %g is negative or not a number", fn, (double)r->depth_tol);
  return RT_OK;
}

extern "C" {

int rt_view_refine_model(uint32_t width, uint32_t height, const rt_view_refine* refine, const rt_ray_radiance* plane0, uint8_t* mask_out,
                         uint32_t* n_refined_out) {
  const char* fn = "rt_view_refine_model";
  const int rc = rt_view_check_refine(refine, fn);
  if (rc != RT_OK) return rc;
  if (width == 0 || height == 0 || (uint64_t)width * height > ((uint64_t)1 << 27)) return rt_fail(RT_ERR_INVALID_ARG, "%s: a frame of %u x %u", fn, width, height);
  if (!plane0 || !plane0->rgb || !plane0->valid || !plane0->id || !plane0->t)
    return rt_fail(RT_ERR_INVALID_ARG, "%s: the rgb, valid, id and t planes of sample 0 are all required", fn);
  uint32_t n = 0;
  for (uint32_t y = 0; y < height; y++)
    for (uint32_t x = 0; x < width; x++) {
      const bool r = rt_view_refine_pixel(x, y, width, height, refine->criteria, refine->colour_tol, refine->depth_tol, plane0->rgb, plane0->valid,
                                          plane0->id, plane0->t);
      if (mask_out) mask_out[y * width + x] = r ? 1u : 0u;
      n += r ? 1u : 0u;
    }
  if (n_refined_out) *n_refined_out = n;
  return RT_OK;
}

int rt_view_resolve_adaptive_model(uint32_t n_pixels, uint32_t n_samples, const uint8_t* plane_of, const uint8_t* mask, const rt_ray_radiance* base,
                                   const rt_ray_radiance* rays, const rt_ray_radiance* pixels) {
  const char* fn = "rt_view_resolve_adaptive_model";
  if (!plane_of || !mask || !base || !pixels) return rt_fail(RT_ERR_INVALID_ARG, "%s: null argument", fn);
  if (n_samples == 0 || n_samples > RT_VIEW_MAX_SAMPLES) return rt_fail(RT_ERR_INVALID_ARG, "%s: n_samples %u outside 1 .. %u", fn, n_samples, RT_VIEW_MAX_SAMPLES);
  if (!base->rgb || !base->valid || !base->id || !base->t) return rt_fail(RT_ERR_INVALID_ARG, "%s: the rgb, valid, id and t planes of sample 0 are all required", fn);
  if (plane_of[0] != 0) return rt_fail(RT_ERR_INVALID_ARG, "%s: plane_of[0] must be 0", fn);
  bool others = false;
  for (uint32_t k = 0; k < n_samples; k++) {
    if (plane_of[k] > k) return rt_fail(RT_ERR_INVALID_ARG, "%s: plane_of[%u] = %u is not a first-occurrence index", fn, k, plane_of[k]);
    others = others || plane_of[k] != 0;
  }
  if (others && (!rays || !rays->rgb || !rays->valid)) return rt_fail(RT_ERR_INVALID_ARG, "%s: the per-ray rgb and valid planes are required", fn);
  const float scale = rt_view_scale(n_samples);
  for (uint32_t p = 0; p < n_pixels; p++)
    rt_view_resolve_adaptive_pixel(p, n_pixels, n_samples, scale, plane_of, mask[p] != 0u, base->rgb, base->valid, base->id, base->t,
                                   others ? rays->rgb : nullptr, others ? rays->valid : nullptr, pixels->rgb, pixels->valid, pixels->id, pixels->t,
                                   pixels->argb);
  return RT_OK;
}

}  // extern "C"
