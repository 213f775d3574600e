// rt_sah.hip -- the kernel of the SAH report (rt_scene_bvh_quality): rt_sah_node of rt_sah.h with a thread index.
//
//   rt_sah_kernel   one thread per node.  Every thread reads the root's two child boxes from node 0 (uniform: scalar loads)
//                   for A_root, adds its node's terms, and the workgroup reduces its three integer sums -- across a
//                   wavefront with __shfl_down, across the wavefronts through LDS -- into ONE 64-bit atomicAdd per sum
//                   and workgroup.  Integer sums: the result does not depend on the order of arrival.
// It only reads the node array, as a query does.
#include <hip/hip_runtime.h>

#include "rt_sah.h"

#define RT_SAH_WAVES (RT_SAH_WG / 64u)

__global__ __launch_bounds__(RT_SAH_WG) void rt_sah_kernel(const RtNode* __restrict__ nodes, uint32_t n_nodes, unsigned long long* __restrict__ out) {
  __shared__ unsigned long long red[3][RT_SAH_WAVES];
  const uint32_t i = blockIdx.x * RT_SAH_WG + threadIdx.x;
  uint64_t sums[2] = {0u, 0u};
  uint32_t bad = 0u;
  if (i < n_nodes) rt_sah_node(nodes[i], rt_sah_root_area(nodes[0]), sums, &bad);
  unsigned long long v[3] = {sums[0], sums[1], bad};
#pragma unroll
  for (int k = 0; k < 3; k++) {
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) v[k] += __shfl_down(v[k], w, 64);
  }
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0u)
    for (int k = 0; k < 3; k++) red[k][wave] = v[k];
  __syncthreads();
  if (threadIdx.x < 3u) {
    unsigned long long t = 0u;
    for (uint32_t w = 0; w < RT_SAH_WAVES; w++) t += red[threadIdx.x][w];
    if (t) atomicAdd(out + threadIdx.x, t);
  }
}

int rt_launch_sah(const RtNode* nodes_dev, uint32_t n_nodes, unsigned long long* out_dev, void* stream) {
  hipError_t e = hipMemsetAsync(out_dev, 0, 3 * sizeof(unsigned long long), (hipStream_t)stream);
  if (e != hipSuccess || !n_nodes) return (int)e;
  hipLaunchKernelGGL(rt_sah_kernel, dim3((n_nodes + RT_SAH_WG - 1u) / RT_SAH_WG), dim3(RT_SAH_WG), 0, (hipStream_t)stream, nodes_dev, n_nodes, out_dev);
  return (int)hipGetLastError();
}
