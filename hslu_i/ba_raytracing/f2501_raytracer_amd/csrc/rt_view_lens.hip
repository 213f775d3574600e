// rt_view_lens.hip -- the kernels of thin-lens camera views: the functions of rt_view_lens.h (the host model's) with a thread index.
//
//   rt_view_lens_rays_kernel         one thread per ray, laid out as rt_view_rays_kernel: workgroup (bx, u) makes rays
//                                    u n_pixels + 256 bx .. of plane u, so the plane's four offsets are uniform (scalar loads)
//   rt_view_lens_sparse_rays_kernel  the generator of pass 2 of an adaptive frame, as rt_view_sparse_rays_kernel
//   rt_view_coc_kernel               one thread per pixel: the circle of confusion of plane 0 -> the view's coc plane
//   rt_view_defocus_spread_kernel    one workgroup per 16 x 16 pixels: their coc and a halo of `spread` pixels go to LDS
//                                    (cells outside the frame hold 0, which reaches nothing), then every thread walks its
//                                    (2 spread + 1)^2 window there.  A tile without an out-of-focus cell is skipped: the vote is
//                                    taken with the barrier.  A workgroup adds the pixels it ADDED to one word with one atomic
//                                    (out of focus, most wavefronts add some: one atomic each to one address costs more
//                                    than the window walk).
//                                    profiles/view_lens.md: why LDS and not cached global reads (RT_LENS_SPREAD_GLOBAL=1 builds
//                                    that form, for the A/B).
// The sizes are kernel arguments; no kernel waits for another workgroup; every loop's trip count is uniform.  Every index
// is below n_distinct n_pixels <= 2^27; a tile index is below (16 + 2 * 16)^2.
#include <hip/hip_runtime.h>

#include "rt_view_lens.h"

#ifndef RT_LENS_SPREAD_GLOBAL
#define RT_LENS_SPREAD_GLOBAL 0
#endif

namespace {

constexpr uint32_t TILE = RT_VIEW_LENS_TILE;
#if !RT_LENS_SPREAD_GLOBAL
constexpr uint32_t SIDE = RT_VIEW_LENS_TILE + 2u * RT_VIEW_LENS_MAX_SPREAD;
#endif

__global__ __launch_bounds__(RT_VIEW_WG) void rt_view_lens_rays_kernel(RtViewCam cam, const float* __restrict__ px, const float* __restrict__ lens,
                                                                       float aperture, float focus_distance, float* __restrict__ origin,
                                                                       float* __restrict__ direction) {
  const uint32_t p = blockIdx.x * RT_VIEW_WG + threadIdx.x, u = blockIdx.y;
  if (p >= cam.n_pixels) return;
  float o[3], d[3];
  rt_view_lens_ray(cam, p % cam.width, p / cam.width, px[2u * u], px[2u * u + 1u], lens[2u * u], lens[2u * u + 1u], aperture, focus_distance, o, d);
  const size_t k = 3u * ((size_t)u * cam.n_pixels + p);
  origin[k] = o[0], origin[k + 1] = o[1], origin[k + 2] = o[2];
  direction[k] = d[0], direction[k + 1] = d[1], direction[k + 2] = d[2];
}

__global__ __launch_bounds__(RT_VIEW_WG) void rt_view_lens_sparse_rays_kernel(RtViewCam cam, const float* __restrict__ px,
                                                                              const float* __restrict__ lens, float aperture, float focus_distance,
                                                                              const uint8_t* __restrict__ mask, float* __restrict__ origin,
                                                                              float* __restrict__ direction) {
  const uint32_t p = blockIdx.x * RT_VIEW_WG + threadIdx.x, u = blockIdx.y;
  if (p >= cam.n_pixels) return;
  float o[3] = {0.0f, 0.0f, 0.0f}, d[3] = {0.0f, 0.0f, 0.0f};
  if (u >= 1u && mask[p])
    rt_view_lens_ray(cam, p % cam.width, p / cam.width, px[2u * u], px[2u * u + 1u], lens[2u * u], lens[2u * u + 1u], aperture, focus_distance, o, d);
  const size_t k = 3u * ((size_t)u * cam.n_pixels + p);
  origin[k] = o[0], origin[k + 1] = o[1], origin[k + 2] = o[2];
  direction[k] = d[0], direction[k + 1] = d[1], direction[k + 2] = d[2];
}

__global__ __launch_bounds__(RT_VIEW_WG) void rt_view_coc_kernel(RtViewCam cam, const float* __restrict__ px, float aperture, float focus_distance,
                                                                 float coc_scale, const uint8_t* __restrict__ valid0, const float* __restrict__ t0,
                                                                 float* __restrict__ coc) {
  const uint32_t p = blockIdx.x * RT_VIEW_WG + threadIdx.x;
  if (p >= cam.n_pixels) return;
  coc[p] = rt_view_coc_pixel(cam, p % cam.width, p / cam.width, px[0], px[1], aperture, focus_distance, coc_scale, valid0[p] != 0u, t0[p]);
}

__global__ __launch_bounds__(TILE* TILE) void rt_view_defocus_spread_kernel(uint32_t width, uint32_t height, uint32_t spread, float coc_tol,
                                                                            const float* __restrict__ coc, uint8_t* __restrict__ mask,
                                                                            uint8_t* __restrict__ mask_out, uint32_t* __restrict__ n_refined) {
  const uint32_t tx = threadIdx.x % TILE, ty = threadIdx.x / TILE;
  const uint32_t x = blockIdx.x * TILE + tx, y = blockIdx.y * TILE + ty;
  bool found = false;
#if RT_LENS_SPREAD_GLOBAL
  if (x < width && y < height) found = rt_view_defocus_pixel(x, y, width, height, spread, coc_tol, coc);
#else
  __shared__ float tile[SIDE * SIDE];
  const uint32_t side = TILE + 2u * spread;  // (spread <= RT_VIEW_LENS_MAX_SPREAD, checked on the host: side <= SIDE)
  bool blurred = false;
  for (uint32_t ry = 0; ry < side; ry += TILE)
    for (uint32_t rx = 0; rx < side; rx += TILE) {
      const uint32_t cx = rx + tx, cy = ry + ty;
      if (cx < side && cy < side) {
        const uint32_t gx = blockIdx.x * TILE + cx - spread, gy = blockIdx.y * TILE + cy - spread;  // (left of / above the frame: wraps to >= W / H)
        const float c = gx < width && gy < height ? coc[(size_t)gy * width + gx] : 0.0f;
        tile[cy * SIDE + cx] = c;
        if (!(c <= coc_tol)) blurred = true;
      }
    }
  if (__syncthreads_or(blurred ? 1 : 0)) {
    const int s = (int)spread;
    for (int dy = -s; dy <= s; dy++)
      for (int dx = -s; dx <= s; dx++) {
        const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
        const float c = tile[(ty + (uint32_t)(dy + s)) * SIDE + tx + (uint32_t)(dx + s)];
        if (rt_view_defocus_reaches(c, coc_tol, (float)(ax > ay ? ax : ay))) found = true;
      }
  }
#endif
  bool added = false;
  if (found && x < width && y < height) {
    const uint32_t p = y * width + x;
    added = mask[p] == 0u;
    mask[p] = 1u;
    if (mask_out) mask_out[p] = 1u;
  }
  const uint32_t n_added = (uint32_t)__syncthreads_count(added ? 1 : 0);  // (every thread of the workgroup is here: nothing returned early)
  if (threadIdx.x == 0u && n_added) atomicAdd(n_refined, n_added);
}

}  // namespace

#define RT_LENS_LAUNCH(kernel, grid, block, ...)                                              \
  do {                                                                                        \
    hipLaunchKernelGGL(kernel, dim3 grid, dim3(block), 0, (hipStream_t)stream, __VA_ARGS__);  \
    return (int)hipGetLastError();                                                            \
  } while (0)

int rt_launch_view_lens_rays(const RtViewCam& cam, const float* px, const float* lens, uint32_t n_distinct, float aperture, float focus_distance,
                             float* origin, float* direction, void* stream) {
  const uint32_t n_wgs = (cam.n_pixels + RT_VIEW_WG - 1u) / RT_VIEW_WG;
  RT_LENS_LAUNCH(rt_view_lens_rays_kernel, (n_wgs, n_distinct), RT_VIEW_WG, cam, px, lens, aperture, focus_distance, origin, direction);
}

int rt_launch_view_lens_sparse_rays(const RtViewCam& cam, const float* px, const float* lens, uint32_t n_distinct, float aperture,
                                    float focus_distance, const uint8_t* mask, float* origin, float* direction, void* stream) {
  const uint32_t n_wgs = (cam.n_pixels + RT_VIEW_WG - 1u) / RT_VIEW_WG;
  RT_LENS_LAUNCH(rt_view_lens_sparse_rays_kernel, (n_wgs, n_distinct), RT_VIEW_WG, cam, px, lens, aperture, focus_distance, mask, origin, direction);
}

int rt_launch_view_coc(const RtViewCam& cam, const float* px, float aperture, float focus_distance, const uint8_t* valid0, const float* t0,
                       float* coc, void* stream) {
  const uint32_t n_wgs = (cam.n_pixels + RT_VIEW_WG - 1u) / RT_VIEW_WG;
  RT_LENS_LAUNCH(rt_view_coc_kernel, (n_wgs), RT_VIEW_WG, cam, px, aperture, focus_distance, rt_view_coc_scale(cam), valid0, t0, coc);
}

int rt_launch_view_defocus_spread(uint32_t width, uint32_t height, uint32_t spread, float coc_tol, const float* coc, uint8_t* mask,
                                  uint8_t* mask_out, uint32_t* n_refined, void* stream) {
  if (spread > RT_VIEW_LENS_MAX_SPREAD) return (int)hipErrorInvalidValue;  // (the tile holds a halo of 16 at most)
  RT_LENS_LAUNCH(rt_view_defocus_spread_kernel, ((width + TILE - 1u) / TILE, (height + TILE - 1u) / TILE), TILE * TILE, width, height, spread, coc_tol,
                 coc, mask, mask_out, n_refined);
}
#undef RT_LENS_LAUNCH
