// rt_solid.hip -- the kernel of the containment and signed-distance queries (rt_contains_points*, rt_signed_distance*):
// rt_solid_query of rt_solid.h with a thread index.
//
// One lane per point, 256 threads per workgroup, a grid-stride loop over the batch (the stride is wave-uniform; the tail
// wavefront runs with `have` false in its idle lanes).  The R directions are a loop that is uniform over the wavefront: the
// lanes of a wave cast PARALLEL rays, so the neighbouring points of a grid go through the same boxes side by side.  Every lane
// walks the threaded tree for itself with vector loads, as rt_multihit_kernel does, and counts: no list, no early end.  Nothing
// is shared between lanes but the votes that control the loops.  The spheres are decided once per point before the loop.  The
// stores are plain vector stores: the rows of crossings and winding as their direction finishes, one record per point at the
// end.  No LDS, no atomics, no scratch.  The kernel reads only the scene's blob and the batch; for a signed distance it also reads
// the `distance` plane rt_closest_kernel wrote before it on the same stream.
#include <hip/hip_runtime.h>

#include "rt_solid.h"

// RtSolidArgs as the kernel reads it (the accessor rt_solid_query asks for): the scalars from the argument, every pointer and
// every direction by a load from the kernel-argument segment at the place of its use, as RtMhKernArgs (rt_multihit.hip) and for
// its reason -- seven pointers and a table of 24 floats would otherwise sit in scalar registers across the walk.  The row index
// is uniform and checked against RT_SOLID_RMAX by the launch.  The struct is the kernel's second argument, behind RtDevScene.
#define RT_SOLID_ARGS_AT ((sizeof(RtDevScene) + 7u) & ~(size_t)7u)
struct RtSolidKernArgs {
  uint32_t n, n_dirs_, rule_;
  template <class T>
  __device__ static T ld(size_t field) {
    typedef const char __attribute__((address_space(4))) * KernArg;
    return *(const volatile T __attribute__((address_space(4)))*)((KernArg)__builtin_amdgcn_kernarg_segment_ptr() + RT_SOLID_ARGS_AT + field);
  }
#define RT_SOLID_X(type, name) \
  __device__ type name() const { return ld<type>(offsetof(RtSolidArgs, name)); }
  RT_SOLID_POINTERS(RT_SOLID_X)
#undef RT_SOLID_X
  __device__ float dir(uint32_t r, int k) const { return ld<float>(offsetof(RtSolidArgs, dir) + 12u * (size_t)r + 4u * (size_t)k); }
  __device__ uint32_t n_dirs() const { return n_dirs_; }
  __device__ uint32_t rule() const { return rule_; }
};

__global__ __launch_bounds__(256) void rt_solid_kernel(RtDevScene sc, RtSolidArgs a) {
  const RtMhBlob S = {sc, sc.base};
  const RtSolidKernArgs A = {a.n, a.n_dirs < RT_SOLID_RMAX ? a.n_dirs : RT_SOLID_RMAX, a.rule};
  for (size_t base = (size_t)blockIdx.x * 256u; base < A.n; base += (size_t)gridDim.x * 256u) {
    const size_t i = base + threadIdx.x;
    rt_solid_query(S, A, (uint32_t)i, i < A.n);
  }
}

// a grid-stride kernel, at most 32 workgroups per CU in flight (as the ray queries)
int rt_launch_solid(const RtDevScene& sc, const RtSolidArgs& a, void* stream) {
  if (a.n == 0) return 0;
  if (a.n_dirs < 1u || a.n_dirs > RT_SOLID_RMAX) return (int)hipErrorInvalidValue;
  const uint32_t w = (uint32_t)(((uint64_t)a.n + 255u) / 256u);
  hipLaunchKernelGGL(rt_solid_kernel, dim3(w < 8192u ? w : 8192u), dim3(256), 0, (hipStream_t)stream, sc, a);
  return (int)hipGetLastError();
}
