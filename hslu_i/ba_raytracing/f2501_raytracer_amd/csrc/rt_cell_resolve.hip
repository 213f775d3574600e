// rt_cell_resolve.hip -- the kernels that enumerate overflowed per-cell shadow candidate lists again under the sharper rule:
// rt_cell_resolve_cell of rt_cell_resolve.h with a thread index.
//
//   rt_cell_resolve_find_kernel   one thread per receiver cell of a chunk: a cell with at least one overflowed list appends its
//                                 index to the chunk's work list (one atomic per wavefront).  About a quarter of the cells of a
//                                 dense scene have one, an eighth of the lists.
//   rt_cell_resolve_kernel        one thread per listed CELL, a loop over its overflowed lights: the thread owns the cell's
//                                 flags word, as in rt_cell_prune_kernel, so no atomic is needed, and what is written does not
//                                 depend on the order of the work list.  Every lane of a wavefront has a tree walk to do (without
//                                 the work list three lanes in four would idle through their neighbours' walks).  The launch
//                                 covers the chunk; threads beyond the count the find kernel left on the device return at
//                                 once, so the host never waits for the count.
// They run once per scene and light-cloud size, right after rt_cell_prune_kernel on the same stream, and touch only the lists,
// the flags, the temporary work list (at most 64 MiB, rt_cell_resolve_temp_bytes; larger scenes go chunk by chunk) and, when
// there is one, the pool of wide records (one atomic on its counter per record).
#include <hip/hip_runtime.h>

#include "rt_cell_resolve.h"

#define RT_CELL_RESOLVE_WG 256u
#define RT_CELL_RESOLVE_COUNTERS 1024u

__global__ __launch_bounds__(RT_CELL_RESOLVE_WG) void rt_cell_resolve_find_kernel(const uint16_t* lists, uint32_t n_lights, uint32_t cell0, uint32_t cell1,
                                                                                  uint32_t* counter, uint32_t* work) {
  const uint32_t c = cell0 + blockIdx.x * RT_CELL_RESOLVE_WG + threadIdx.x;
  const bool has = c < cell1 && rt_cell_resolve_wanted(lists + (size_t)c * n_lights * RT_PRUNE_LIST_SLOTS, n_lights);
  const unsigned long long m = __ballot(has);
  if (!m) return;
  const uint32_t lane = threadIdx.x & 63u, leader = (uint32_t)__ffsll((long long)m) - 1u;
  uint32_t at = 0u;
  if (lane == leader) at = atomicAdd(counter, (uint32_t)__popcll(m));
  at = (uint32_t)__shfl((int)at, (int)leader);
  // (every cell of the chunk is appended at most once: at + rank < cell1 - cell0 <= the work list's size)
  if (has) work[at + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = c;
}

__global__ __launch_bounds__(RT_CELL_RESOLVE_WG) void rt_cell_resolve_kernel(RtDevScene sc, RtCellResolveArgs a, const uint32_t* counter, const uint32_t* work) {
  const uint32_t i = blockIdx.x * RT_CELL_RESOLVE_WG + threadIdx.x;
  if (i >= *counter || i >= a.chunk_cells) return;
  const uint32_t c = work[i];
  if (c >= a.cell.n_cells) return;
  rt_cell_resolve_cell(sc, sc.base, a, c, a.cell.lists + (size_t)c * sc.n_lights * RT_PRUNE_LIST_SLOTS, a.cell.flags + c,
                       a.counts ? a.counts + (size_t)c * sc.n_lights : nullptr);
}

int rt_launch_cell_resolve(const RtDevScene& sc, const RtCellResolveArgs& a, void* stream) {
  const uint32_t n = a.cell.n_cells, chunk = a.chunk_cells;
  if (n == 0u || sc.n_lights == 0u || sc.n_lights > 8u || sc.n_thr == 0u) return 0;
  if (!a.work || chunk == 0u || ((size_t)n + chunk - 1u) / chunk > RT_CELL_RESOLVE_COUNTERS) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(a.work, 0, RT_CELL_RESOLVE_COUNTERS * 4u, st);
  if (e != hipSuccess) return (int)e;
  if (a.wide && a.wide_count && (e = hipMemsetAsync(a.wide_count, 0, 4u, st)) != hipSuccess) return (int)e;  // the pool starts empty
  uint32_t* list = a.work + RT_CELL_RESOLVE_COUNTERS;
  uint32_t k = 0;
  for (uint32_t c0 = 0; c0 < n; k++) {
    const uint32_t c1 = n - c0 > chunk ? c0 + chunk : n;
    const dim3 grid((c1 - c0 + RT_CELL_RESOLVE_WG - 1u) / RT_CELL_RESOLVE_WG);
    hipLaunchKernelGGL(rt_cell_resolve_find_kernel, grid, dim3(RT_CELL_RESOLVE_WG), 0, st, a.cell.lists, sc.n_lights, c0, c1, a.work + k, list);
    hipLaunchKernelGGL(rt_cell_resolve_kernel, grid, dim3(RT_CELL_RESOLVE_WG), 0, st, sc, a, a.work + k, list);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    c0 = c1;
  }
  return 0;
}
