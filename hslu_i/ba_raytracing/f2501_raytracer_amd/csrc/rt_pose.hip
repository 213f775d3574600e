// rt_pose.hip -- the kernel of device-side part poses: the functions of rt_pose.h (the host model's) with a thread index.
//
//   rt_pose_kernel   one thread per triangle of the pose's covering range, then one per sphere.  A thread whose object
//                    belongs to no part returns at once (its posed record keeps the rest values written at creation);
//                    the others read their part's transform and write the object's posed record.
// A streaming kernel over at most a few hundred kilobytes: plain loads and stores, no LDS, no atomics, nothing is read
// back, no kernel waits for another workgroup.  It costs a launch, not bandwidth.
#include <hip/hip_runtime.h>

#include "rt_pose.h"

__global__ __launch_bounds__(RT_POSE_WG) void rt_pose_kernel(RtPoseArrays p, const rt_transform* __restrict__ transforms) {
  const uint32_t i = blockIdx.x * RT_POSE_WG + threadIdx.x;
  if (i < p.n_cover) {
    const uint32_t part = p.tri_part[i];
    if (part == RT_POSE_NONE) return;
    rt_pose_tri(p, i, (const float*)(transforms + part));
  } else if (i - p.n_cover < p.n_spheres) {
    const uint32_t k = i - p.n_cover, part = p.sphere_part[k];
    if (part == RT_POSE_NONE) return;
    rt_pose_sphere(p, k, (const float*)(transforms + part));
  }
}

int rt_launch_pose(const RtPoseArrays& p, const rt_transform* transforms_dev, void* stream) {
  const uint32_t n = p.n_cover + p.n_spheres;  // (both below 2^30: the scene's limits)
  if (!n) return (int)hipSuccess;
  hipLaunchKernelGGL(rt_pose_kernel, dim3((n + RT_POSE_WG - 1u) / RT_POSE_WG), dim3(RT_POSE_WG), 0, (hipStream_t)stream, p, transforms_dev);
  return (int)hipGetLastError();
}
