// rt_multihit.hip -- the kernel of the multi-hit ray queries (rt_list_intersections*): rt_mh_query of rt_multihit.h with a thread index.
//
// One lane per ray, 256 threads per workgroup, a grid-stride loop over the batch (the stride is wave-uniform; the tail
// wavefront runs with `have` false in its idle lanes).  The rays of a batch are unrelated, so every lane walks for itself with
// vector loads, as walk_tris_lane of the ray queries and rt_closest_kernel do: nothing is shared between lanes but the votes
// that control the loops.  The K-entry list lives in REGISTERS: its entries are indexed statically only (the insert is an
// unrolled compare-exchange chain, the planes are written from entry 0 of a list that shifts down), so the compiler never
// needs scratch for it.  Two classes are compiled, for max_hits <= 4 and <= 16: a list of 4 keys costs 8 VGPRs and a chain of
// 4 steps per hit, one of 16 costs 32 and 16 (profiles/multi_hit.md has the register counts and the occupancy of each).  No
// LDS, no atomics.  The kernel reads only the scene's blob and the caller's batch.
#include <hip/hip_runtime.h>

#include "rt_multihit.h"

// RtMultiHitArgs as the kernel reads it (the accessor rt_mh_query asks for, rt_multihit.h): the scalars from the argument, every
// pointer by a load from the kernel-argument segment at the place of its use.  The loads are volatile so that the compiler
// does not gather them in front of the walk again; they hit the scalar or vector cache, a dozen per ray.  The struct is the
// kernel's second argument, behind RtDevScene.
#define RT_MH_ARGS_AT ((sizeof(RtDevScene) + 7u) & ~(size_t)7u)
struct RtMhKernArgs {
  uint32_t n, max_hits_, cull_;
  template <class T>
  __device__ static T ld(size_t field) {
    typedef const char __attribute__((address_space(4))) * KernArg;
    return *(const volatile T __attribute__((address_space(4)))*)((KernArg)__builtin_amdgcn_kernarg_segment_ptr() + RT_MH_ARGS_AT + field);
  }
#define RT_MH_X(type, name) \
  __device__ type name() const { return ld<type>(offsetof(RtMultiHitArgs, name)); }
  RT_MH_POINTERS(RT_MH_X)
#undef RT_MH_X
  __device__ uint32_t max_hits() const { return max_hits_; }
  __device__ bool cull() const { return cull_ != 0u; }
};

template <int KMAX>
__device__ __forceinline__ void multihit_body(const RtDevScene& sc, const RtMultiHitArgs& a) {
  const RtMhBlob S = {sc, sc.base};
  const RtMhKernArgs A = {a.n, a.max_hits, a.cull};
  for (size_t base = (size_t)blockIdx.x * 256u; base < A.n; base += (size_t)gridDim.x * 256u) {
    const size_t i = base + threadIdx.x;
    rt_mh_query<KMAX>(S, A, (uint32_t)i, i < A.n);
  }
}
// rt_multihit_kernel, one per list class (the same arguments in the same places: RtMhKernArgs reads them)
__global__ __launch_bounds__(256) void rt_multihit_kernel_k4(RtDevScene sc, RtMultiHitArgs a) { multihit_body<4>(sc, a); }
__global__ __launch_bounds__(256) void rt_multihit_kernel_k16(RtDevScene sc, RtMultiHitArgs a) { multihit_body<RT_MH_KMAX>(sc, a); }

// a grid-stride kernel, at most 32 workgroups per CU in flight (as the ray queries)
int rt_launch_multihit(const RtDevScene& sc, const RtMultiHitArgs& a, void* stream) {
  if (a.n == 0) return 0;
  const uint32_t w = (uint32_t)(((uint64_t)a.n + 255u) / 256u);
  const dim3 grid(w < 8192u ? w : 8192u);
  if (a.max_hits <= 4u)
    hipLaunchKernelGGL(rt_multihit_kernel_k4, grid, dim3(256), 0, (hipStream_t)stream, sc, a);
  else
    hipLaunchKernelGGL(rt_multihit_kernel_k16, grid, dim3(256), 0, (hipStream_t)stream, sc, a);
  return (int)hipGetLastError();
}
