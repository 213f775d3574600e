// rt_closest.hip -- the kernel of the closest-point queries (rt_closest_points*): rt_closest_query of rt_closest.h with a thread index.
//
// One lane per point, 256 threads per workgroup, a grid-stride loop over the batch (the stride is wave-uniform; the tail
// wavefront runs with `have` false in its idle lanes).  The points of a batch are unrelated, so every lane walks for itself
// with vector loads, as walk_tris_lane of the ray queries does: no LDS, no scratch, nothing shared between lanes but the votes
// that control the loops.  The kernel reads only the scene's blob and the caller's batch.
#include <hip/hip_runtime.h>

#include "rt_closest.h"

__global__ __launch_bounds__(256) void rt_closest_kernel(RtDevScene sc, RtClosestArgs a) {
  for (size_t base = (size_t)blockIdx.x * 256u; base < a.n; base += (size_t)gridDim.x * 256u) {
    const size_t i = base + threadIdx.x;
    const bool have = i < a.n;
    float p[3] = {0.0f, 0.0f, 0.0f}, max_distance = INFINITY;
    if (have) {
      p[0] = a.point[3u * i], p[1] = a.point[3u * i + 1u], p[2] = a.point[3u * i + 2u];
      if (a.max_distance) max_distance = a.max_distance[i];
    }
    RtClosestHit h;
    rt_closest_query(sc, sc.base, p, max_distance, have, h);
    if (!have) continue;
    rt_closest_store(a, i, h);
  }
}

// a grid-stride kernel, at most 32 workgroups per CU in flight (as the ray queries)
int rt_launch_closest(const RtDevScene& sc, const RtClosestArgs& a, void* stream) {
  if (a.n == 0) return 0;
  const uint32_t w = (uint32_t)(((uint64_t)a.n + 255u) / 256u);
  hipLaunchKernelGGL(rt_closest_kernel, dim3(w < 8192u ? w : 8192u), dim3(256), 0, (hipStream_t)stream, sc, a);
  return (int)hipGetLastError();
}
