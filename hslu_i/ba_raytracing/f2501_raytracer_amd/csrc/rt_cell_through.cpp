// rt_cell_through.cpp -- the host model of rt_cell_through_kernel: rt_cell_through_cell (rt_cell_through.h) in a loop over the
// cells of a packed scene, and the sizing of the marks table.  No HIP call: compiled host-only and checked on the CPU, as
// rt_cell_prune.cpp is.
#include <hip/hip_runtime_api.h>

#include "rt_cell_through.h"
#include "rt_scene_pack.h"

void rt_cell_through_packed(const RtPackedScene& pk, RtCellThroughArgs a) {
  if (pk.dev.n_lights == 0u || pk.dev.n_lights > 8u || pk.flag_geo.empty() || !a.marks_end) return;
  a.cell.flag_geo = pk.flag_geo.data();
  a.cell.n_cells = a.cell.n_cells < pk.n_cells ? a.cell.n_cells : pk.n_cells;
  a.cell.n_tri_cells = pk.n_tri_cells;
  const char* base = (const char*)pk.blob.data();
  for (uint32_t c = 0; c < a.cell.n_cells; c++)
    rt_cell_through_cell(pk.dev, base, a, c, a.cell.lists + (size_t)c * pk.dev.n_lights * RT_PRUNE_LIST_SLOTS);
}

// one byte per (cell, light), rounded up to the 64 bytes of a wide record
size_t rt_cell_through_bytes(uint32_t n_cells, uint32_t n_lights, size_t budget_left) {
  const size_t n = ((size_t)n_cells * n_lights + 63u) & ~(size_t)63u;
  return n != 0u && n <= budget_left ? n : 0u;
}
