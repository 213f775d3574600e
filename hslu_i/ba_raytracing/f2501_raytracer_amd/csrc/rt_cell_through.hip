// rt_cell_through.hip -- the kernel that marks the listed glass panes every shadow ray of a receiver cell crosses:
// rt_cell_through_cell of rt_cell_through.h with a thread index.
//
//   rt_cell_through_kernel   one thread per receiver cell, a loop over the lights, as rt_cell_prune_kernel: the cell's hull is
//                            built once for all its lights, and only when one of its lists names a transmissive leaf slot at
//                            all.  Every thread writes its cell's n_lights bytes, marked or not, so the table needs no clearing.
// It runs once per scene and light-cloud size, right after rt_cell_resolve_kernel on the same stream; it reads the final lists
// and writes only the marks.
#include <hip/hip_runtime.h>

#include "rt_cell_through.h"

#define RT_CELL_THROUGH_WG 256u

__global__ __launch_bounds__(RT_CELL_THROUGH_WG) void rt_cell_through_kernel(RtDevScene sc, RtCellThroughArgs a) {
  const uint32_t c = blockIdx.x * RT_CELL_THROUGH_WG + threadIdx.x;
  if (c >= a.cell.n_cells) return;
  rt_cell_through_cell(sc, sc.base, a, c, a.cell.lists + (size_t)c * sc.n_lights * RT_PRUNE_LIST_SLOTS);
}

int rt_launch_cell_through(const RtDevScene& sc, const RtCellThroughArgs& a, void* stream) {
  if (a.cell.n_cells == 0u || sc.n_lights == 0u || sc.n_lights > 8u) return 0;
  if (!a.marks_end || !a.cell.lists) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(rt_cell_through_kernel, dim3((a.cell.n_cells + RT_CELL_THROUGH_WG - 1u) / RT_CELL_THROUGH_WG), dim3(RT_CELL_THROUGH_WG), 0,
                     (hipStream_t)stream, sc, a);
  return (int)hipGetLastError();
}
