// rt_view_lens.cpp -- the device-free half of thin-lens camera views: the checks of a lens table and of an rt_view_lens, and
// the host models of the lens generator and of the defocus criterion (the functions of rt_view_lens.h in loops).  No HIP
// call: links without a device.  The handle and the launch sequence are in rt_view.cpp.
#include <hip/hip_runtime_api.h>  // (types only: rt_internal.h names float4 / uint4)

#include <vector>

#include "rt_scene_pack.h"  // rt_fail
#include "rt_view_lens.h"

int rt_view_lens_check_desc(const rt_view_desc* d, const float* lens_samples, const char* fn) {
  const int rc = rt_view_check_desc(d, fn);
  if (rc != RT_OK) return rc;
  if (!lens_samples) return rt_fail(RT_ERR_INVALID_ARG, "%s: null lens sample table", fn);
  for (uint32_t k = 0; k < 2u * d->n_samples; k++)
    if (!rt_finite(lens_samples[k])) return rt_fail(RT_ERR_INVALID_ARG, "%s: sample %u has a non-finite lens offset", fn, k / 2u);
  float px[2 * RT_VIEW_MAX_SAMPLES], lens[2 * RT_VIEW_MAX_SAMPLES];
  uint8_t plane_of[RT_VIEW_MAX_SAMPLES];
  const uint64_t n_rays = (uint64_t)rt_view_lens_dedup(d->samples, lens_samples, d->n_samples, px, lens, plane_of) * d->width * d->height;
  if (n_rays > ((uint64_t)1 << 27))
    return rt_fail(RT_ERR_INVALID_ARG, "%s: %u x %u pixels of distinct lens samples exceed the 2^27 rays a ray order sorts", fn, d->width, d->height);
  return RT_OK;
}

int rt_view_check_lens(const rt_view_lens* l, const char* fn) {
  if (!l) return rt_fail(RT_ERR_INVALID_ARG, "%s: null lens", fn);
  if (l->abi_version != RT_ABI_VERSION) return rt_fail(RT_ERR_INVALID_ARG, "%s: rt_view_lens.abi_version %u != %u", fn, l->abi_version, RT_ABI_VERSION);
  if (!(l->aperture >= 0.0f) || !rt_finite(l->aperture))
    return rt_fail(RT_ERR_INVALID_ARG, "%s: aperture %g is negative or not finite", fn, (double)l->aperture);
  if (!(l->focus_distance > 0.0f) || !rt_finite(l->focus_distance))
    return rt_fail(RT_ERR_INVALID_ARG, "%s: focus_distance %g is not finite and positive", fn, (double)l->focus_distance);
  if (!(l->coc_tol >= 0.0f)) return rt_fail(RT_ERR_INVALID_ARG, "%s: coc_tol %g is negative or not a number", fn, (double)l->coc_tol);
  if (l->spread > RT_VIEW_LENS_MAX_SPREAD) return rt_fail(RT_ERR_INVALID_ARG, "%s: spread %u above %u", fn, l->spread, RT_VIEW_LENS_MAX_SPREAD);
  if (l->reserved != 0u) return rt_fail(RT_ERR_INVALID_ARG, "%s: rt_view_lens.reserved must be 0", fn);
  return RT_OK;
}

extern "C" {

int rt_view_lens_rays_model(const rt_view_desc* d, const float* lens_samples, const rt_view_camera* c, const rt_view_lens* l, float* origin,
                            float* direction, uint8_t* plane_of, uint32_t* n_distinct) {
  const char* fn = "rt_view_lens_rays_model";
  int rc = rt_view_lens_check_desc(d, lens_samples, fn);
  if (rc != RT_OK) return rc;
  if ((rc = rt_view_check_camera(c, fn)) != RT_OK) return rc;
  if ((rc = rt_view_check_lens(l, fn)) != RT_OK) return rc;
  if (l->aperture > 0.0f && c->kind != RT_VIEW_PINHOLE) return rt_fail(RT_ERR_INVALID_ARG, "%s: an RT_VIEW_REFERENCE camera has no lens (aperture %g)", fn, (double)l->aperture);
  float px[2 * RT_VIEW_MAX_SAMPLES], lens[2 * RT_VIEW_MAX_SAMPLES];
  uint8_t po[RT_VIEW_MAX_SAMPLES];
  const uint32_t nd = rt_view_lens_dedup(d->samples, lens_samples, d->n_samples, px, lens, po);
  if (plane_of) memcpy(plane_of, po, d->n_samples);
  if (n_distinct) *n_distinct = nd;
  if (!origin && !direction) return RT_OK;
  const RtViewCam cam = rt_view_cam_of(*d, *c);
  for (uint32_t u = 0; u < nd; u++)
    for (uint32_t p = 0; p < cam.n_pixels; p++) {
      float o[3], dir[3];
      if (l->aperture > 0.0f)
        rt_view_lens_ray(cam, p % cam.width, p / cam.width, px[2 * u], px[2 * u + 1], lens[2 * u], lens[2 * u + 1], l->aperture, l->focus_distance, o, dir);
      else
        rt_view_ray(cam, p % cam.width, p / cam.width, px[2 * u], px[2 * u + 1], o, dir);
      const size_t k = 3u * ((size_t)u * cam.n_pixels + p);
      if (origin) memcpy(origin + k, o, 12);
      if (direction) memcpy(direction + k, dir, 12);
    }
  return RT_OK;
}

int rt_view_defocus_model(const rt_view_desc* d, const rt_view_camera* c, const rt_view_lens* l, const uint8_t* valid0, const float* t0,
                          float* coc_out, uint8_t* mask_inout, uint32_t* n_added_out) {
  const char* fn = "rt_view_defocus_model";
  int rc = rt_view_check_desc(d, fn);
  if (rc != RT_OK) return rc;
  if ((rc = rt_view_check_camera(c, fn)) != RT_OK) return rc;
  if ((rc = rt_view_check_lens(l, fn)) != RT_OK) return rc;
  if (!valid0 || !t0) return rt_fail(RT_ERR_INVALID_ARG, "%s: the valid and t planes of sample 0 are both required", fn);
  const RtViewCam cam = rt_view_cam_of(*d, *c);
  if (n_added_out) *n_added_out = 0;
  if (!rt_view_defocus_active(l->aperture, l->coc_tol)) {
    if (coc_out) memset(coc_out, 0, (size_t)cam.n_pixels * 4);
    return RT_OK;
  }
  if (c->kind != RT_VIEW_PINHOLE) return rt_fail(RT_ERR_INVALID_ARG, "%s: an RT_VIEW_REFERENCE camera has no lens (aperture %g)", fn, (double)l->aperture);
  std::vector<float> coc(cam.n_pixels);
  const float scale = rt_view_coc_scale(cam);
  for (uint32_t p = 0; p < cam.n_pixels; p++)
    coc[p] = rt_view_coc_pixel(cam, p % cam.width, p / cam.width, d->samples[0], d->samples[1], l->aperture, l->focus_distance, scale, valid0[p] != 0u, t0[p]);
  if (coc_out) memcpy(coc_out, coc.data(), (size_t)cam.n_pixels * 4);
  uint32_t n = 0;
  for (uint32_t y = 0; y < cam.height; y++)
    for (uint32_t x = 0; x < cam.width; x++)
      if (rt_view_defocus_pixel(x, y, cam.width, cam.height, l->spread, l->coc_tol, coc.data())) {
        const uint32_t p = y * cam.width + x;
        if (mask_inout) {
          n += mask_inout[p] ? 0u : 1u;
          mask_inout[p] = 1u;
        } else {
          n++;
        }
      }
  if (n_added_out) *n_added_out = n;
  return RT_OK;
}

}  // extern "C"
