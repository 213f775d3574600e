// rt_cell_resolve.cpp -- the host model of rt_cell_resolve_kernel: rt_cell_resolve_cell (rt_cell_resolve.h) in a loop over the
// cells of a packed scene, and the sizing of the device stage's temporary memory.  No HIP call: compiled host-only and checked
// on the CPU, as rt_cell_prune.cpp is.
#include <hip/hip_runtime_api.h>

#include "rt_cell_resolve.h"
#include "rt_scene_pack.h"

void rt_cell_resolve_packed(const RtPackedScene& pk, RtCellResolveArgs a) {
  if (pk.dev.n_lights == 0u || pk.dev.n_lights > 8u || pk.flag_geo.empty()) return;
  a.cell.flag_geo = pk.flag_geo.data();
  a.cell.n_cells = a.cell.n_cells < pk.n_cells ? a.cell.n_cells : pk.n_cells;
  a.cell.n_tri_cells = pk.n_tri_cells;
  const char* base = (const char*)pk.blob.data();
  const uint32_t nl = pk.dev.n_lights;
  for (uint32_t c = 0; c < a.cell.n_cells; c++)
    rt_cell_resolve_cell(pk.dev, base, a, c, a.cell.lists + (size_t)c * nl * RT_PRUNE_LIST_SLOTS, a.cell.flags + c, a.counts ? a.counts + (size_t)c * nl : nullptr);
}

// 4096 bytes of chunk counters (one per chunk, at most 1024 chunks), then one cell index per cell of a chunk
size_t rt_cell_resolve_temp_bytes(uint32_t n_cells, size_t budget_left, uint32_t* chunk_cells) {
  *chunk_cells = 0u;
  const size_t cap = budget_left < ((size_t)64u << 20) ? budget_left : ((size_t)64u << 20);
  if (n_cells == 0u || cap < 4096u + 4u * 256u) return 0;
  size_t chunk = (cap - 4096u) / 4u;
  if (chunk > n_cells) chunk = n_cells;
  if (((size_t)n_cells + chunk - 1u) / chunk > 1024u) return 0;
  *chunk_cells = (uint32_t)chunk;
  return 4096u + 4u * chunk;
}

// the records at 64 bytes each, then 64 bytes for the counter
size_t rt_cell_wide_pool_bytes(uint32_t n_cells, uint32_t n_lights, size_t budget_left, uint32_t* wide_cap) {
  *wide_cap = 0u;
  const size_t rec = 2u * RT_CELL_WIDE_SLOTS;
  if (n_cells == 0u || n_lights == 0u || budget_left < 2u * rec) return 0;
  size_t cap = (budget_left - rec) / rec;
  const size_t lists = (size_t)n_cells * n_lights;
  if (cap > (lists + 7u) / 8u) cap = (lists + 7u) / 8u;
  if (cap > RT_CELL_WIDE_MAX_RECORDS) cap = RT_CELL_WIDE_MAX_RECORDS;
  *wide_cap = (uint32_t)cap;
  return cap * rec + rec;
}
