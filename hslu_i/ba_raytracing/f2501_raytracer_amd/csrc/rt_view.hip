// rt_view.hip -- the kernels of device-side camera views: the functions of rt_view.h (the host model's) with a thread index.
//
//   rt_view_rays_kernel     one thread per ray; workgroup (bx, u) makes rays u n_pixels + 256 bx .. of sample plane u, so the
//                           sample offset is uniform in a workgroup (two scalar loads) and every store is contiguous
//   rt_view_resolve_kernel  one thread per pixel; reads the pixel's entry of every sample plane -- lanes take consecutive
//                           pixels, every plane read and every write is contiguous -- and writes the pixel planes
// Streaming kernels: no LDS, no atomics, nothing is read back, no kernel waits for another workgroup.  The sizes are kernel
// arguments; every index is below n_distinct n_pixels <= 2^27.
#include <hip/hip_runtime.h>

#include "rt_view.h"

namespace {

__global__ __launch_bounds__(RT_VIEW_WG) void rt_view_rays_kernel(RtViewCam cam, const float* __restrict__ distinct, float* __restrict__ origin,
                                                                  float* __restrict__ direction) {
  const uint32_t p = blockIdx.x * RT_VIEW_WG + threadIdx.x, u = blockIdx.y;
  if (p >= cam.n_pixels) return;
  const float sx = distinct[2u * u], sy = distinct[2u * u + 1u];
  float o[3], d[3];
  rt_view_ray(cam, p % cam.width, p / cam.width, sx, sy, o, d);
  const size_t k = 3u * ((size_t)u * cam.n_pixels + p);
  origin[k] = o[0], origin[k + 1] = o[1], origin[k + 2] = o[2];
  direction[k] = d[0], direction[k + 1] = d[1], direction[k + 2] = d[2];
}

__global__ __launch_bounds__(RT_VIEW_WG) void rt_view_resolve_kernel(uint32_t n_pixels, uint32_t n_samples, float scale,
                                                                     const uint8_t* __restrict__ plane_of, const float* __restrict__ rgb,
                                                                     const uint8_t* __restrict__ valid, const int32_t* __restrict__ id,
                                                                     const float* __restrict__ t, float* __restrict__ o_rgb,
                                                                     uint8_t* __restrict__ o_valid, int32_t* __restrict__ o_id,
                                                                     float* __restrict__ o_t, uint32_t* __restrict__ o_argb) {
  const uint32_t p = blockIdx.x * RT_VIEW_WG + threadIdx.x;
  if (p >= n_pixels) return;
  rt_view_resolve_pixel(p, n_pixels, n_samples, scale, plane_of, rgb, valid, id, t, o_rgb, o_valid, o_id, o_t, o_argb);
}

}  // namespace

int rt_launch_view_rays(const RtViewCam& cam, const float* distinct, uint32_t n_distinct, float* origin, float* direction, void* stream) {
  const uint32_t n_wgs = (cam.n_pixels + RT_VIEW_WG - 1u) / RT_VIEW_WG;
  hipLaunchKernelGGL(rt_view_rays_kernel, dim3(n_wgs, n_distinct), dim3(RT_VIEW_WG), 0, (hipStream_t)stream, cam, distinct, origin, direction);
  return (int)hipGetLastError();
}

int rt_launch_view_resolve(uint32_t n_pixels, uint32_t n_samples, const uint8_t* plane_of, const float* rgb, const uint8_t* valid,
                           const int32_t* id, const float* t, const rt_ray_radiance& out, void* stream) {
  const uint32_t n_wgs = (n_pixels + RT_VIEW_WG - 1u) / RT_VIEW_WG;
  hipLaunchKernelGGL(rt_view_resolve_kernel, dim3(n_wgs), dim3(RT_VIEW_WG), 0, (hipStream_t)stream, n_pixels, n_samples, rt_view_scale(n_samples),
                     plane_of, rgb, valid, id, t, out.rgb, out.valid, out.id, out.t, out.argb);
  return (int)hipGetLastError();
}
