// rt_view_adapt.hip -- the kernels of adaptive camera views: the functions of rt_view_adapt.h (the host model's) with a thread
// index, and the stable partition of a permutation by a flag per entry.
//
//   rt_view_classify_kernel          one thread per pixel: the refine rule on plane 0 -> mask; a wavefront adds its number of
//                                    refined pixels to one word with ONE atomic (the lowest active lane, a vector instruction)
//   rt_view_sparse_rays_kernel       the generator of pass 2, laid out as rt_view_rays_kernel: workgroup (bx, u)
//   rt_view_flags_kernel             the predicate of every entry of a permutation -> one byte
//   rt_partition_count_kernel        set flags per RT_PARTITION_WG entries -> counts (zero behind the last workgroup)
//   rt_partition_scatter_kernel      after the exclusive scan of counts (rt_launch_exclusive_scan): a set entry goes to
//                                    counts[wg] + its rank among the workgroup's set entries, an unset one behind all set ones,
//                                    in entry order as well -- ranks from ballots and mbcnt, across wavefronts from LDS
//   rt_view_resolve_adaptive_kernel  one thread per pixel, as rt_view_resolve_kernel
// The sizes are kernel arguments; nothing is read back; no kernel waits for another workgroup.  Every index is below
// n_distinct n_pixels <= 2^27; a scatter position is checked against the size of its target before the store.
#include <hip/hip_runtime.h>

#include "rt_lbvh.h"  // (rt_launch_exclusive_scan)
#include "rt_view_adapt.h"

namespace {

__device__ __forceinline__ uint32_t lanes_below(unsigned long long m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__global__ __launch_bounds__(RT_VIEW_WG) void rt_view_classify_kernel(uint32_t width, uint32_t height, uint32_t criteria, float colour_tol,
                                                                      float depth_tol, const float* __restrict__ rgb0,
                                                                      const uint8_t* __restrict__ valid0, const int32_t* __restrict__ id0,
                                                                      const float* __restrict__ t0, uint8_t* __restrict__ mask,
                                                                      uint8_t* __restrict__ mask_out, uint32_t* __restrict__ n_refined) {
  const uint32_t p = blockIdx.x * RT_VIEW_WG + threadIdx.x;
  const bool on = p < width * height;
  bool refined = false;
  if (on) {
    refined = rt_view_refine_pixel(p % width, p / width, width, height, criteria, colour_tol, depth_tol, rgb0, valid0, id0, t0);
    mask[p] = refined ? 1u : 0u;
    if (mask_out) mask_out[p] = refined ? 1u : 0u;
  }
  const unsigned long long m = __ballot(refined);
  if (refined && lanes_below(m) == 0u) atomicAdd(n_refined, (uint32_t)__popcll(m));
}

__global__ __launch_bounds__(RT_VIEW_WG) void rt_view_sparse_rays_kernel(RtViewCam cam, const float* __restrict__ distinct,
                                                                         const uint8_t* __restrict__ mask, float* __restrict__ origin,
                                                                         float* __restrict__ direction) {
  const uint32_t p = blockIdx.x * RT_VIEW_WG + threadIdx.x, u = blockIdx.y;
  if (p >= cam.n_pixels) return;
  float o[3] = {0.0f, 0.0f, 0.0f}, d[3] = {0.0f, 0.0f, 0.0f};
  if (u >= 1u && mask[p]) rt_view_ray(cam, p % cam.width, p / cam.width, distinct[2u * u], distinct[2u * u + 1u], o, d);
  const size_t k = 3u * ((size_t)u * cam.n_pixels + p);
  origin[k] = o[0], origin[k + 1] = o[1], origin[k + 2] = o[2];
  direction[k] = d[0], direction[k + 1] = d[1], direction[k + 2] = d[2];
}

__global__ __launch_bounds__(RT_PARTITION_WG) void rt_view_flags_kernel(const uint32_t* __restrict__ perm_in, uint32_t n, uint32_t n_pixels,
                                                                        const uint8_t* __restrict__ mask, uint8_t* __restrict__ flags) {
  const uint32_t k = blockIdx.x * RT_PARTITION_WG + threadIdx.x;
  if (k >= n) return;
  const uint32_t i = perm_in ? perm_in[k] : k;
  bool f = i < n_pixels;
  if (mask) f = i < n ? rt_view_ray_live(i, n_pixels, mask) : false;  // (i < n always: perm_in is a permutation)
  flags[k] = f ? 1u : 0u;
}

// the number of set flags among the workgroup's threads below this one, and in the whole workgroup
__device__ __forceinline__ uint32_t block_rank(bool f, uint32_t* lds /* [RT_PARTITION_WG / 64] */, uint32_t* total) {
  const unsigned long long m = __ballot(f);
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u) lds[wave] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t before = 0u, all = 0u;
#pragma unroll
  for (uint32_t w = 0; w < RT_PARTITION_WG / 64u; w++) {
    const uint32_t c = lds[w];
    if (w < wave) before += c;
    all += c;
  }
  *total = all;
  return before + lanes_below(m);
}

__global__ __launch_bounds__(RT_PARTITION_WG) void rt_partition_count_kernel(const uint8_t* __restrict__ flags, uint32_t n, uint32_t n_wgs,
                                                                             uint32_t* __restrict__ counts) {
  __shared__ uint32_t lds[RT_PARTITION_WG / 64u];
  const uint32_t e = blockIdx.x * RT_PARTITION_WG + threadIdx.x;
  const bool f = blockIdx.x < n_wgs && e < n && flags[e] != 0u;
  uint32_t all;
  block_rank(f, lds, &all);
  if (threadIdx.x == 0u) counts[blockIdx.x] = all;
}

__global__ __launch_bounds__(RT_PARTITION_WG) void rt_partition_scatter_kernel(const uint32_t* __restrict__ perm_in,
                                                                               const uint8_t* __restrict__ flags, uint32_t n, uint32_t n_out,
                                                                               uint32_t n_wgs, const uint32_t* __restrict__ counts,
                                                                               uint32_t* __restrict__ perm_out) {
  __shared__ uint32_t lds[RT_PARTITION_WG / 64u];
  const uint32_t e = blockIdx.x * RT_PARTITION_WG + threadIdx.x;
  const bool on = e < n;
  const bool f = on && flags[e] != 0u;
  uint32_t all;
  const uint32_t set_before = counts[blockIdx.x] + block_rank(f, lds, &all);
  const uint32_t n_set = counts[n_wgs];  // (the scan is exclusive: the entry behind the last workgroup holds the total)
  const uint32_t pos = f ? set_before : n_set + (e - set_before);
  if (on && pos < n_out) perm_out[pos] = perm_in ? perm_in[e] : e;
}

__global__ __launch_bounds__(RT_VIEW_WG) void rt_view_resolve_adaptive_kernel(uint32_t n_pixels, uint32_t n_samples, float scale,
                                                                              const uint8_t* __restrict__ plane_of, const uint8_t* __restrict__ mask,
                                                                              const float* __restrict__ rgb0, const uint8_t* __restrict__ valid0,
                                                                              const int32_t* __restrict__ id0, const float* __restrict__ t0,
                                                                              const float* __restrict__ rgb, const uint8_t* __restrict__ valid,
                                                                              float* __restrict__ o_rgb, uint8_t* __restrict__ o_valid,
                                                                              int32_t* __restrict__ o_id, float* __restrict__ o_t,
                                                                              uint32_t* __restrict__ o_argb) {
  const uint32_t p = blockIdx.x * RT_VIEW_WG + threadIdx.x;
  if (p >= n_pixels) return;
  rt_view_resolve_adaptive_pixel(p, n_pixels, n_samples, scale, plane_of, mask[p] != 0u, rgb0, valid0, id0, t0, rgb, valid, o_rgb, o_valid, o_id, o_t,
                                 o_argb);
}

}  // namespace

#define RT_ADAPT_LAUNCH(kernel, grid, block, ...)                                             \
  do {                                                                                        \
    hipLaunchKernelGGL(kernel, dim3 grid, dim3(block), 0, (hipStream_t)stream, __VA_ARGS__);  \
    const hipError_t e_ = hipGetLastError();                                                  \
    if (e_ != hipSuccess) return (int)e_;                                                     \
  } while (0)

int rt_launch_view_classify(uint32_t width, uint32_t height, uint32_t criteria, float colour_tol, float depth_tol, const RtViewAdaptWs& w,
                            uint8_t* mask_out, void* stream) {
  const uint32_t n_wgs = (width * height + RT_VIEW_WG - 1u) / RT_VIEW_WG;
  RT_ADAPT_LAUNCH(rt_view_classify_kernel, (n_wgs), RT_VIEW_WG, width, height, criteria, colour_tol, depth_tol, (const float*)w.rgb0,
                  (const uint8_t*)w.valid0, (const int32_t*)w.id0, (const float*)w.t0, w.mask, mask_out, w.n_refined);
  return (int)hipSuccess;
}

int rt_launch_view_sparse_rays(const RtViewCam& cam, const float* distinct, uint32_t n_distinct, const uint8_t* mask, float* origin,
                               float* direction, void* stream) {
  const uint32_t n_wgs = (cam.n_pixels + RT_VIEW_WG - 1u) / RT_VIEW_WG;
  RT_ADAPT_LAUNCH(rt_view_sparse_rays_kernel, (n_wgs, n_distinct), RT_VIEW_WG, cam, distinct, mask, origin, direction);
  return (int)hipSuccess;
}

int rt_launch_view_flags(const uint32_t* perm_in, uint32_t n, uint32_t n_pixels, const uint8_t* mask, uint8_t* flags, void* stream) {
  const uint32_t n_wgs = (n + RT_PARTITION_WG - 1u) / RT_PARTITION_WG;
  RT_ADAPT_LAUNCH(rt_view_flags_kernel, (n_wgs), RT_PARTITION_WG, perm_in, n, n_pixels, mask, flags);
  return (int)hipSuccess;
}

int rt_launch_partition(const uint32_t* perm_in, const uint8_t* flags, uint32_t n, uint32_t n_out, uint32_t* counts, uint32_t* sums,
                        uint32_t* perm_out, void* stream) {
  const uint32_t n_wgs = (n + RT_PARTITION_WG - 1u) / RT_PARTITION_WG, n_counts = (uint32_t)rt_partition_counts(n);
  RT_ADAPT_LAUNCH(rt_partition_count_kernel, (n_counts), RT_PARTITION_WG, flags, n, n_wgs, counts);
  const int e = rt_launch_exclusive_scan(counts, n_counts, sums, stream);  // (n <= 2^27: n_counts <= 2^19 + 8, 257 scan blocks)
  if (e != (int)hipSuccess) return e;
  RT_ADAPT_LAUNCH(rt_partition_scatter_kernel, (n_wgs), RT_PARTITION_WG, perm_in, flags, n, n_out, n_wgs, (const uint32_t*)counts, perm_out);
  return (int)hipSuccess;
}

int rt_launch_view_resolve_adaptive(uint32_t n_pixels, uint32_t n_samples, const uint8_t* plane_of, const RtViewAdaptWs& w, const float* rgb,
                                    const uint8_t* valid, const rt_ray_radiance& out, void* stream) {
  const uint32_t n_wgs = (n_pixels + RT_VIEW_WG - 1u) / RT_VIEW_WG;
  RT_ADAPT_LAUNCH(rt_view_resolve_adaptive_kernel, (n_wgs), RT_VIEW_WG, n_pixels, n_samples, rt_view_scale(n_samples), plane_of,
                  (const uint8_t*)w.mask, (const float*)w.rgb0, (const uint8_t*)w.valid0, (const int32_t*)w.id0, (const float*)w.t0, rgb, valid,
                  out.rgb, out.valid, out.id, out.t, out.argb);
  return (int)hipSuccess;
}
#undef RT_ADAPT_LAUNCH
