// rt_cell_prune.cpp -- the host model of rt_cell_prune_kernel: rt_cell_prune_cell (rt_cell_prune.h) in a loop over the cells
// of a packed scene.  No HIP call (the header only brings the vector types of rt_internal.h): compiled host-only and checked
// on the CPU, as rt_scene_pack.cpp is.
#include <hip/hip_runtime_api.h>

#include "rt_cell_prune.h"
#include "rt_scene_pack.h"

void rt_cell_prune_packed(const RtPackedScene& pk, RtCellPruneArgs a) {
  if (pk.dev.n_lights == 0u || pk.dev.n_lights > 8u || pk.flag_geo.empty()) return;
  a.flag_geo = pk.flag_geo.data();
  a.n_cells = a.n_cells < pk.n_cells ? a.n_cells : pk.n_cells;
  a.n_tri_cells = pk.n_tri_cells;
  const char* base = (const char*)pk.blob.data();
  for (uint32_t c = 0; c < a.n_cells; c++)
    rt_cell_prune_cell(pk.dev, base, a, c, a.lists + (size_t)c * pk.dev.n_lights * RT_PRUNE_LIST_SLOTS, a.flags + c);
}
