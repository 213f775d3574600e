// rt_occlusion.hip -- the kernels of the ambient-occlusion queries (rt_ambient_occlusion*): rt_occ_sample of rt_occlusion.h with a
// lane index, and the reductions of a point's samples inside the wavefront.
//
// Lanes are SAMPLES, and a wavefront owns whole points, so that no reduction leaves the wave: for S <= 64 a point takes a
// segment of seg = the next power of two >= S lanes and a wave holds 64 / seg points; for S > 64 a wave takes one point in
// ceil(S / 64) rounds.  256 threads per workgroup, a grid-stride loop over groups of points whose stride and bound are
// wave-uniform; idle lanes (the tail of a segment, of the batch, of the last round) run with `have` false.  Every lane makes its
// own ray from the point's frame and walks the threaded tree for itself with vector loads, as rt_multihit_kernel does; the
// lanes of a segment start at one point, so they share the top of the tree in cache.  Nothing is shared between lanes but the
// votes that control the loops, until the end: the occlusion bits are a ballot, shifted and masked per segment, `clear` is a
// popcount of it, and the three int32 sums of the bent normal go through a butterfly of cross-lane adds that stays inside the
// segment.  One lane per point stores.  No atomics, no LDS, no scratch.  The kernels read only the scene's blob and the batch.
#include <hip/hip_runtime.h>

#include "rt_occlusion.h"

// RtOcclusionArgs as the kernels read it (the accessor rt_occ_sample asks for): the scalars from the argument, every pointer by a
// load from the kernel-argument segment at the place of its use, as RtMhKernArgs (rt_multihit.hip) and for its reason.  The
// struct is the kernels' second argument, behind RtDevScene.
#define RT_OCC_ARGS_AT ((sizeof(RtDevScene) + 7u) & ~(size_t)7u)
struct RtOccKernArgs {
  float bias_, max_distance_;
  uint32_t n, n_samples_, n_table_, pass_;
  template <class T>
  __device__ static T ld(size_t field) {
    typedef const char __attribute__((address_space(4))) * KernArg;
    return *(const volatile T __attribute__((address_space(4)))*)((KernArg)__builtin_amdgcn_kernarg_segment_ptr() + RT_OCC_ARGS_AT + field);
  }
#define RT_OCC_X(type, name) \
  __device__ type name() const { return ld<type>(offsetof(RtOcclusionArgs, name)); }
  RT_OCC_POINTERS(RT_OCC_X)
#undef RT_OCC_X
  __device__ float bias() const { return bias_; }
  __device__ float max_distance() const { return max_distance_; }
  __device__ uint32_t n_samples() const { return n_samples_; }
  __device__ uint32_t n_table() const { return n_table_; }
  __device__ bool pass() const { return pass_ != 0u; }
};

// the sum of v over the lanes of a segment of `seg` lanes (a power of two), in every lane of it: an xor butterfly, whose steps
// below seg never leave the segment
__device__ __forceinline__ int32_t segment_sum(int32_t v, uint32_t seg) {
#pragma unroll
  for (uint32_t m = 32u; m >= 1u; m >>= 1)
    if (m < seg) v += __shfl_xor(v, (int)m, 64);
  return v;
}

// WIDE: S > 64, one point per wave in rounds of 64 samples; else S <= 64, 64 / seg points per wave in one round
template <bool WIDE>
__device__ __forceinline__ void occlusion_body(const RtDevScene& sc, const RtOcclusionArgs& a) {
  const RtMhBlob S = {sc, sc.base};
  const RtOccKernArgs A = {a.bias, a.max_distance, a.n, a.n_samples, a.n_table, a.pass};
  const uint32_t n_samples = A.n_samples(), words = rt_occ_words(n_samples);
  uint32_t seg = 64u;
  if (!WIDE)
    while ((seg >> 1) >= n_samples) seg >>= 1;
  const uint32_t per_wave = 64u / seg;  // points of a wave
  const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t sub = lane / seg, s0 = lane & (seg - 1u);  // the lane's point within the wave, its sample within the round
  const uint32_t n_groups = (uint32_t)(((uint64_t)A.n + per_wave - 1u) / per_wave);
  for (uint32_t g = blockIdx.x * 4u + wave; g < n_groups; g += gridDim.x * 4u) {
    const uint64_t at = (uint64_t)g * per_wave + sub;
    const uint32_t i = (uint32_t)at;
    const bool point = at < A.n;
    RtOccPoint P;
    rt_occ_point(A, i, point, P);
    int32_t sum[3] = {0, 0, 0};
    uint32_t clear = 0u;
    const uint32_t rounds = WIDE ? (n_samples + 63u) / 64u : 1u;
    for (uint32_t round = 0; round < rounds; round++) {
      const uint32_t s = round * 64u + s0;
      const bool have = point && s < n_samples;
      int32_t q[3];
      const bool occluded = rt_occ_sample(S, A, P, s, have, q);
      for (int k = 0; k < 3; k++) sum[k] += q[k];
      const uint64_t blocked = __builtin_amdgcn_ballot_w64(have && occluded), open = __builtin_amdgcn_ballot_w64(have && !occluded);
      if (WIDE) {
        clear += (uint32_t)__builtin_popcountll(open);
        uint32_t* bits = A.bits();
        if (bits && lane < 2u && 2u * round + lane < words)
          bits[(size_t)i * words + 2u * round + lane] = lane ? (uint32_t)(blocked >> 32) : (uint32_t)blocked;
      } else {
        const uint64_t mask = seg == 64u ? ~0ull : (1ull << seg) - 1ull;
        const uint64_t mine = (blocked >> (sub * seg)) & mask;
        clear = (uint32_t)__builtin_popcountll((open >> (sub * seg)) & mask);
        uint32_t* bits = A.bits();
        if (bits && point && s0 == 0u) {
          bits[(size_t)i * words] = (uint32_t)mine;
          if (words > 1u) bits[(size_t)i * words + 1u] = (uint32_t)(mine >> 32);
        }
      }
    }
    for (int k = 0; k < 3; k++) sum[k] = segment_sum(sum[k], seg);
    if (point && s0 == 0u) rt_occ_store(A, i, clear, sum);
  }
}
// rt_occlusion_kernel, one per class (the same arguments in the same places: RtOccKernArgs reads them)
__global__ __launch_bounds__(256) void rt_occlusion_kernel_s64(RtDevScene sc, RtOcclusionArgs a) { occlusion_body<false>(sc, a); }
__global__ __launch_bounds__(256) void rt_occlusion_kernel_wide(RtDevScene sc, RtOcclusionArgs a) { occlusion_body<true>(sc, a); }

// a grid-stride kernel, at most 32 workgroups per CU in flight (as the ray queries): a workgroup's four waves take a group of
// points each
int rt_launch_occlusion(const RtDevScene& sc, const RtOcclusionArgs& a, void* stream) {
  if (a.n == 0) return 0;
  uint32_t seg = 64u;
  if (a.n_samples <= 64u)
    while ((seg >> 1) >= a.n_samples) seg >>= 1;
  const uint64_t groups = ((uint64_t)a.n * seg + 63u) / 64u, w = (groups + 3u) / 4u;
  const dim3 grid((uint32_t)(w < 8192u ? w : 8192u));
  if (a.n_samples <= 64u)
    hipLaunchKernelGGL(rt_occlusion_kernel_s64, grid, dim3(256), 0, (hipStream_t)stream, sc, a);
  else
    hipLaunchKernelGGL(rt_occlusion_kernel_wide, grid, dim3(256), 0, (hipStream_t)stream, sc, a);
  return (int)hipGetLastError();
}
