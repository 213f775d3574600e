// cell_resolve_check.cpp -- a stand-alone program around the host model of the stage that resolves overflowed per-cell shadow
// candidate lists (csrc/rt_cell_resolve.h, rt_cell_resolve.cpp) and the scene packer, meant to be compiled host-only under
// -fsanitize=address,undefined: the walk indexes the threaded tree, the leaf records and the lists by values read from memory.
//
//   cell_resolve_check SCENE.bin BUDGET_BYTES STRIDE [POOL_RECORDS]
//
// SCENE.bin (tests/test_cell_resolve_sanitize.py writes it): uint32 {n_spheres, n_triangles, n_materials, n_lights, n_cloud_floats},
// then sphere centres, r^2, 1/r (float), sphere materials (uint32), triangle v1, e1, e2, normals (float), triangle materials
// (uint32), materials, lights, the light-cloud table, {fw, fh, fd, eps} (float).  Every STRIDE-th cell gets all its lists set to the
// overflow marker and resolved; the program prints how many lists it resolved, emptied and left overflowed.  With POOL_RECORDS the
// stage gets a pool of that many wide records (64 bytes each, at a 64-byte boundary, exactly that long: a write past the last
// record is a write past the allocation), and every list that carries the mark is followed to its record.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_cell_resolve.h"
#include "rt_scene_pack.h"

template <class T>
static bool take(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 4 && argc != 5) return fprintf(stderr, "usage: %s SCENE.bin BUDGET_BYTES STRIDE [POOL_RECORDS]\n", argv[0]), 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return perror(argv[1]), 2;
  const uint64_t budget = strtoull(argv[2], nullptr, 10);
  const uint32_t stride = (uint32_t)strtoul(argv[3], nullptr, 10);
  uint32_t h[5];
  if (fread(h, 4, 5, f) != 5 || stride == 0u) return fprintf(stderr, "bad header\n"), 2;
  std::vector<float> sc, sr, si, v1, e1, e2, nr, mats, lights, cloud, tail;
  std::vector<uint32_t> sm, tm;
  bool ok = take(f, sc, 3u * h[0]) && take(f, sr, h[0]) && take(f, si, h[0]) && take(f, sm, h[0]);
  ok = ok && take(f, v1, 3u * (size_t)h[1]) && take(f, e1, 3u * (size_t)h[1]) && take(f, e2, 3u * (size_t)h[1]) && take(f, nr, 3u * (size_t)h[1]) && take(f, tm, h[1]);
  ok = ok && take(f, mats, (size_t)RT_MATERIAL_STRIDE * h[2]) && take(f, lights, (size_t)RT_LIGHT_STRIDE * h[3]) && take(f, cloud, h[4]) && take(f, tail, 4);
  fclose(f);
  if (!ok) return fprintf(stderr, "short file\n"), 2;
  rt_scene_desc d{};
  d.abi_version = RT_ABI_VERSION;
  d.n_spheres = h[0], d.sphere_center = sc.data(), d.sphere_r_sq = sr.data(), d.sphere_r_inv = si.data(), d.sphere_material = sm.data();
  d.n_triangles = h[1], d.tri_v1 = v1.data(), d.tri_e1 = e1.data(), d.tri_e2 = e2.data(), d.tri_normal = nr.data(), d.tri_material = tm.data();
  d.n_materials = h[2], d.materials = mats.data();
  d.n_lights = h[3], d.lights = lights.data();
  d.device_budget_bytes = budget;
  RtPackedScene pk;
  if (rt_pack_scene(&d, budget, &pk) != 0) return fprintf(stderr, "rt_pack_scene: %s\n", rt_last_error()), 1;
  std::vector<float> scaled;
  float ball[4];
  rt_scale_cloud(cloud.data(), cloud.size(), tail.data(), &scaled, ball);
  RtDevParams P{};
  P.cloud_delta = ball[3];
  rt_beam_constants(tail[3], &P);
  RtCellResolveArgs a{};
  a.cell.flag_geo = pk.flag_geo.data();
  a.cell.n_cells = pk.n_cells, a.cell.n_tri_cells = pk.n_tri_cells;
  memcpy(a.cell.cloud_centre, ball, 12);
  a.cell.beam_delta = P.beam_delta, a.cell.beam_eps_o = P.beam_eps_o;
  a.cell.mode = RT_PRUNE_FULL;
  a.eps_push = P.beam_eps_push, a.eps_ulp = P.beam_eps_ulp;
  const uint32_t nl = pk.dev.n_lights;
  if (nl == 0u || nl > 8u || pk.n_cells == 0u) return fprintf(stderr, "no receiver cells or lights\n"), 1;
  const uint32_t pool_records = argc == 5 ? (uint32_t)strtoul(argv[4], nullptr, 10) : 0u;
  uint16_t* pool = nullptr;
  uint32_t asked = 0;
  if (pool_records) {
    pool = (uint16_t*)aligned_alloc(64, (size_t)pool_records * 2u * RT_CELL_WIDE_SLOTS);
    if (!pool) return fprintf(stderr, "no memory for the pool\n"), 2;
    a.wide = pool, a.wide_cap = pool_records, a.wide_count = &asked;
  }
  unsigned long long cells = 0, resolved = 0, emptied = 0, left = 0, slots = 0, wide = 0, wide_slots = 0;
  for (uint32_t c = 0; c < pk.n_cells; c += stride, cells++) {
    alignas(16) uint16_t list[8 * RT_PRUNE_LIST_SLOTS];
    for (uint32_t k = 0; k < 8 * RT_PRUNE_LIST_SLOTS; k++) list[k] = (k % RT_PRUNE_LIST_SLOTS) ? (uint16_t)RT_PRUNE_LIST_END : (uint16_t)RT_PRUNE_LIST_OVERFLOW;
    uint16_t flag = 0;
    uint8_t counts[8] = {0};
    rt_cell_resolve_cell(pk.dev, (const char*)pk.blob.data(), a, c, list, &flag, (c / stride) & 1u ? counts : nullptr);
    for (uint32_t l = 0; l < nl; l++) {
      const uint16_t* w = list + l * RT_PRUNE_LIST_SLOTS;
      const uint32_t at = rt_cell_wide_index(w);
      if (at != ~0u) {  // a wide list: its record lies inside the pool and holds 9 .. 32 slots of the scene, then padding
        if (!pool || at >= pool_records) return fprintf(stderr, "cell %u light %u: record %u outside the pool\n", c, l, at), 1;
        const uint16_t* rec = pool + (size_t)at * RT_CELL_WIDE_SLOTS;
        uint32_t n = 0;
        while (n < RT_CELL_WIDE_SLOTS && rec[n] != RT_PRUNE_LIST_END) n++;
        for (uint32_t k = 0; k < RT_CELL_WIDE_SLOTS; k++)
          if (k < n ? rec[k] >= pk.dev.n_slots : rec[k] != RT_PRUNE_LIST_END) return fprintf(stderr, "cell %u light %u: record %u is malformed at %u\n", c, l, at, k), 1;
        if (n <= RT_PRUNE_LIST_SLOTS) return fprintf(stderr, "cell %u light %u: a record of %u slots\n", c, l, n), 1;
        wide++, wide_slots += n;
      }
      if (w[0] == RT_PRUNE_LIST_OVERFLOW) { left++; continue; }
      resolved++, emptied += w[0] == RT_PRUNE_LIST_END;
      for (uint32_t k = 0; k < RT_PRUNE_LIST_SLOTS && w[k] < RT_PRUNE_LIST_OVERFLOW; k++) {
        if (w[k] >= pk.dev.n_slots) return fprintf(stderr, "cell %u light %u: slot %u out of range\n", c, l, w[k]), 1;
        slots++;
      }
    }
  }
  printf("cells %llu lists_resolved %llu emptied %llu left_overflowed %llu slots_listed %llu n_cells %u n_slots %u", cells, resolved, emptied, left, slots,
         pk.n_cells, pk.dev.n_slots);
  if (pool_records) printf(" wide_lists %llu wide_slots %llu records_asked %u", wide, wide_slots, asked);
  printf("\n");
  free(pool);
  return 0;
}
