// rt_cell_prune.hip -- the kernel that thins out the per-cell shadow candidate lists: rt_cell_prune_cell of rt_cell_prune.h
// with a thread index.
//
//   rt_cell_prune_kernel   one thread per receiver cell, a loop over the lights: the threads of a cell would share its flags
//                          word, so one thread owns the cell and no atomic is needed.  Neighbouring threads are neighbouring
//                          cells of one triangle: their lists name the same few leaf slots, whose 48-byte records then come
//                          from the cache.  A list is read with one 16-byte load and, when it changed, written with one store.
// It runs once per scene and light-cloud size, right after rt_flags_kernel on the same stream, and touches only the lists
// and the flags.
#include <hip/hip_runtime.h>

#include "rt_cell_prune.h"

#define RT_CELL_PRUNE_WG 256u

__global__ __launch_bounds__(RT_CELL_PRUNE_WG) void rt_cell_prune_kernel(RtDevScene sc, RtCellPruneArgs a) {
  const uint32_t c = blockIdx.x * RT_CELL_PRUNE_WG + threadIdx.x;
  if (c >= a.n_cells) return;
  rt_cell_prune_cell(sc, sc.base, a, c, a.lists + (size_t)c * sc.n_lights * RT_PRUNE_LIST_SLOTS, a.flags + c);
}

int rt_launch_cell_prune(const RtDevScene& sc, const RtCellPruneArgs& a, void* stream) {
  if (a.n_cells == 0u || sc.n_lights == 0u || sc.n_lights > 8u) return 0;
  hipLaunchKernelGGL(rt_cell_prune_kernel, dim3((a.n_cells + RT_CELL_PRUNE_WG - 1u) / RT_CELL_PRUNE_WG), dim3(RT_CELL_PRUNE_WG), 0, (hipStream_t)stream, sc, a);
  return (int)hipGetLastError();
}
