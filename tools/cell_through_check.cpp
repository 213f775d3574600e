// cell_through_check.cpp -- a stand-alone program around the host model of the stage that marks the listed glass panes every
// shadow ray of a receiver cell crosses (csrc/rt_cell_through.h, rt_cell_through.cpp) and the scene packer, meant to be compiled
// host-only under -fsanitize=address,undefined: the stage indexes the leaf records and the slot flags by values read from the
// lists, and writes its table backwards from the table's end.
//
//   cell_through_check SCENE.bin BUDGET_BYTES STRIDE
//
// SCENE.bin as tools/cell_resolve_check.cpp reads it (tests/test_cell_through_sanitize.py writes it).  Every STRIDE-th cell gets
// the lists the resolve stage's walk gives it (at most 8 survivors: a list; more: the overflow marker) and then its marks, in a
// table that is allocated exactly as long as its bytes, one per (cell, light): a write before its first or past its last byte is
// a write outside the allocation.  The program prints what it listed and marked.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_cell_through.h"
#include "rt_scene_pack.h"

template <class T>
static bool take(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 4) return fprintf(stderr, "usage: %s SCENE.bin BUDGET_BYTES STRIDE\n", argv[0]), 2;
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
  RtCellResolveArgs r{};
  r.cell.flag_geo = pk.flag_geo.data();
  r.cell.n_cells = pk.n_cells, r.cell.n_tri_cells = pk.n_tri_cells;
  memcpy(r.cell.cloud_centre, ball, 12);
  r.cell.beam_delta = P.beam_delta, r.cell.beam_eps_o = P.beam_eps_o;
  r.cell.mode = RT_PRUNE_FULL;
  r.eps_push = P.beam_eps_push, r.eps_ulp = P.beam_eps_ulp;
  const uint32_t nl = pk.dev.n_lights;
  if (nl == 0u || nl > 8u || pk.n_cells == 0u) return fprintf(stderr, "no receiver cells or lights\n"), 1;
  const size_t n_marks = (size_t)pk.n_cells * nl;
  uint8_t* marks = (uint8_t*)malloc(n_marks);  // (exactly the table: the first and the last cell's bytes touch its two ends)
  if (!marks) return fprintf(stderr, "no memory for the marks\n"), 2;
  memset(marks, 0xAB, n_marks);
  RtCellThroughArgs t{};
  t.cell = r.cell;
  t.marks_end = marks + n_marks;
  const char* base = (const char*)pk.blob.data();
  const uint32_t* tri_id = (const uint32_t*)(base + pk.dev.off_tri_id);
  unsigned long long cells = 0, lists = 0, overflowed = 0, listed = 0, transmissive = 0, marked = 0;
  auto one = [&](uint32_t c) -> int {
    alignas(16) uint16_t list[8 * RT_PRUNE_LIST_SLOTS];
    for (auto& x : list) x = (uint16_t)RT_PRUNE_LIST_END;
    RtResolveCell K;
    if (rt_resolve_cell_setup(pk.dev, base, r.cell, c, K))
      for (uint32_t l = 0; l < nl; l++) {
        RtPruneBeam B;
        rt_resolve_beam(pk.dev, base, r.cell, K, l, B);
        uint32_t n = 0;
        uint16_t* w = list + l * RT_PRUNE_LIST_SLOTS;
        const bool ok = rt_resolve_walk(pk.dev, base, r, K, B, [&](uint32_t slot) { if (n < RT_PRUNE_LIST_SLOTS) w[n] = (uint16_t)slot; n++; return n <= RT_PRUNE_LIST_SLOTS; });
        if (!ok || n > RT_PRUNE_LIST_SLOTS) w[0] = (uint16_t)RT_PRUNE_LIST_OVERFLOW;
      }
    rt_cell_through_cell(pk.dev, base, t, c, list);
    cells++;
    for (uint32_t l = 0; l < nl; l++) {
      const uint16_t* w = list + l * RT_PRUNE_LIST_SLOTS;
      const uint32_t m = marks[n_marks - 1u - ((size_t)c * nl + l)];
      if (w[0] == RT_PRUNE_LIST_OVERFLOW) overflowed++;
      if (w[0] >= RT_PRUNE_LIST_OVERFLOW) {
        if (m) return fprintf(stderr, "cell %u light %u: marks %#x on an empty or overflowed list\n", c, l, m), 1;
        continue;
      }
      lists++;
      for (uint32_t k = 0; k < RT_PRUNE_LIST_SLOTS; k++) {
        const bool on = (m >> k) & 1u;
        if (w[k] >= RT_PRUNE_LIST_OVERFLOW) {
          if (m >> k) return fprintf(stderr, "cell %u light %u: marks %#x beyond the list's end\n", c, l, m), 1;
          break;
        }
        if (w[k] >= pk.dev.n_slots) return fprintf(stderr, "cell %u light %u: slot %u out of range\n", c, l, w[k]), 1;
        const bool tr = (tri_id[w[k]] & RT_TRI_TRANSMISSIVE) != 0u;
        if (on && !tr) return fprintf(stderr, "cell %u light %u: an opaque slot is marked\n", c, l), 1;
        listed++, transmissive += tr, marked += on;
      }
    }
    return 0;
  };
  for (uint32_t c = 0; c < pk.n_cells; c += stride)
    if (one(c)) return 1;
  if ((pk.n_cells - 1u) % stride != 0u && one(pk.n_cells - 1u)) return 1;  // (the last cell writes the table's first bytes)
  printf("cells %llu lists %llu overflowed %llu listed %llu transmissive %llu marked %llu n_cells %u n_slots %u\n", cells, lists, overflowed, listed, transmissive, marked,
         pk.n_cells, pk.dev.n_slots);
  free(marks);
  return 0;
}
