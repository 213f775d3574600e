// rt_ray_order.cpp -- the device-free half of ray orders (rt_ray_order*): the host model of the order a build produces, and
// the check of a caller's permutation.  The model calls the functions of rt_ray_key.h in loops -- the functions the kernels
// of rt_order.hip are made of -- so it is the specification of the device's keys.  No HIP call: links without a device.
#include <hip/hip_runtime_api.h>  // (types only: rt_internal.h names float4 / uint4)

#include <algorithm>
#include <numeric>
#include <vector>

#include "rt_ray_key.h"
#include "rt_scene_pack.h"  // rt_fail

int rt_check_permutation(const uint32_t* perm, uint32_t n) {
  if (n && !perm) return rt_fail(RT_ERR_INVALID_ARG, "rt_ray_order_set: null permutation");
  std::vector<bool> seen(n, false);
  for (uint32_t k = 0; k < n; k++) {
    if (perm[k] >= n) return rt_fail(RT_ERR_INVALID_ARG, "rt_ray_order_set: not a permutation: entry %u is %u, out of range for %u rays", k, perm[k], n);
    if (seen[perm[k]]) return rt_fail(RT_ERR_INVALID_ARG, "rt_ray_order_set: not a permutation: ray %u appears twice (entry %u)", perm[k], k);
    seen[perm[k]] = true;
  }
  return RT_OK;
}

int rt_ray_order_model(const float* origin, const float* direction, uint32_t n, uint32_t origin_bits, uint32_t* keys, uint32_t* perm,
                       rt_ray_order_info* info) {
  if (n && (!origin || !direction)) return rt_fail(RT_ERR_INVALID_ARG, "rt_ray_order_model: origin / direction missing");
  if (origin_bits > RT_KEY_AXIS_BITS) return rt_fail(RT_ERR_INVALID_ARG, "rt_ray_order_model: origin_bits %u > %u", origin_bits, RT_KEY_AXIS_BITS);
  RtKeyBounds b;
  rt_key_bounds_clear(b);
  for (uint32_t i = 0; i < n; i++) {
    float c[6];
    if (rt_key_coords(origin + 3 * (size_t)i, direction + 3 * (size_t)i, c)) rt_key_bounds_add(b, c);
  }
  RtKeyFrame f;
  rt_key_frame(b, origin_bits, f);
  std::vector<uint32_t> k(n);
  for (uint32_t i = 0; i < n; i++) k[i] = rt_key_of(f, origin + 3 * (size_t)i, direction + 3 * (size_t)i);
  if (keys) std::copy(k.begin(), k.end(), keys);
  if (perm) {
    std::iota(perm, perm + n, 0u);
    std::stable_sort(perm, perm + n, [&](uint32_t x, uint32_t y) { return k[x] < k[y]; });
  }
  if (info) {
    *info = rt_ray_order_info{};
    info->n_rays = n, info->n_live = f.n_live;
    info->origin_bits = f.origin_bits, info->direction_bits = f.direction_bits;
    info->n_origin_axes = f.n_origin_axes, info->n_direction_axes = f.n_direction_axes;
  }
  return RT_OK;
}
