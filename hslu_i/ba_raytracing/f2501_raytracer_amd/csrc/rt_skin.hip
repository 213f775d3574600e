// rt_skin.hip -- the kernels of device-side skinned meshes: the functions of rt_skin.h (the host model's) with a thread index.
//
//   rt_skin_vertex_kernel     one thread per vertex: rest position and normal, four bone indices (one 8-byte load), four
//                             weights (one 16-byte load), up to four bones of 32 bytes; writes V[i] and N[i].  The
//                             influence loop is unrolled.  Bones are read with plain loads: the table is at most 2 MiB and
//                             usually a few KiB, it stays in cache.
//   rt_skin_triangle_kernel   one thread per triangle of a mesh WITH vertex normals: three indices, gathers V and N,
//                             writes v1, e1, e2 and the lerped normal.
//   rt_skin_face_kernel       the same for a mesh WITHOUT vertex normals: the normal is the normalised cross product of
//                             the skinned edges.  A kernel of its own, so that the two fused steps of that normal (and the
//                             compiler's division and square root) are the only fused instructions of the file.
// Streaming kernels over a few hundred kilobytes: no LDS, no atomics, nothing is read back, no kernel waits for another
// workgroup.  The vertex kernel and the triangle kernel go on one stream back to back: stream order is the dependency.
#include <hip/hip_runtime.h>

#include "rt_skin.h"

__global__ __launch_bounds__(RT_SKIN_WG) void rt_skin_vertex_kernel(RtSkinArrays a, const rt_transform* __restrict__ bones) {
  const uint32_t i = blockIdx.x * RT_SKIN_WG + threadIdx.x;
  if (i < a.n_vertices) rt_skin_vertex(a, i, (const float*)bones);
}

__global__ __launch_bounds__(RT_SKIN_WG) void rt_skin_triangle_kernel(RtSkinArrays a) {
  const uint32_t t = blockIdx.x * RT_SKIN_WG + threadIdx.x;
  if (t < a.n_tris) rt_skin_tri(a, t);
}

__global__ __launch_bounds__(RT_SKIN_WG) void rt_skin_face_kernel(RtSkinArrays a) {
  const uint32_t t = blockIdx.x * RT_SKIN_WG + threadIdx.x;
  if (t < a.n_tris) rt_skin_face(a, t);
}

int rt_launch_skin(const RtSkinArrays& a, const rt_transform* bones_dev, void* stream) {
  const hipStream_t s = (hipStream_t)stream;  // (both counts below 2^31: the checks of rt_skin_create)
  hipLaunchKernelGGL(rt_skin_vertex_kernel, dim3((a.n_vertices + RT_SKIN_WG - 1u) / RT_SKIN_WG), dim3(RT_SKIN_WG), 0, s, a, bones_dev);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  const dim3 grid((a.n_tris + RT_SKIN_WG - 1u) / RT_SKIN_WG);
  if (a.normal)
    hipLaunchKernelGGL(rt_skin_triangle_kernel, grid, dim3(RT_SKIN_WG), 0, s, a);
  else
    hipLaunchKernelGGL(rt_skin_face_kernel, grid, dim3(RT_SKIN_WG), 0, s, a);
  return (int)hipGetLastError();
}
