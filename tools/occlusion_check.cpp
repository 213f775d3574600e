// occlusion_check.cpp -- a stand-alone program around the host twin of the ambient-occlusion kernels' walk (rt_occlusion_packed:
// csrc/rt_occlusion.h over the blob of csrc/rt_scene_pack.cpp), meant to be compiled host-only under -fsanitize=address,undefined:
// the walk indexes the threaded tree, the leaf records, the shading records and the material rows by values read from memory,
// reads table rows at (first + s) % n_table and writes (S + 31) / 32 bit words per point.
//
//   occlusion_check SCENE.bin N_POINTS SPLIT_DEPTH N_SAMPLES
//
// SCENE.bin (tests/test_occlusion_sanitize.py writes it): uint32 {n_spheres, n_triangles, n_materials, n_lights, n_points,
// n_table}, then sphere centres, r^2, 1/r (float), sphere materials (uint32), triangle v1, e1, e2, normals (float), triangle
// materials (uint32), materials, lights, the points and normals [n_points][3], the table [n_table][3] (float), the start rows
// [n_points] (uint32) and {bias, max_distance} (float).  The scene is packed (with split clipping of SPLIT_DEPTH), queried,
// rebuilt where that is allowed (LBVH, then PLOC) and queried again; the program prints what it found.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_occlusion.h"
#include "rt_scene_pack.h"

template <class T>
static bool take(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 5) return fprintf(stderr, "usage: %s SCENE.bin N_POINTS SPLIT_DEPTH N_SAMPLES\n", argv[0]), 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return perror(argv[1]), 2;
  uint32_t h[6];
  if (fread(h, 4, 6, f) != 6) return fprintf(stderr, "bad header\n"), 2;
  std::vector<float> sc, sr, si, v1, e1, e2, nr, mats, lights, pts, nrm, table, scalars;
  std::vector<uint32_t> sm, tm, first;
  bool ok = take(f, sc, 3u * h[0]) && take(f, sr, h[0]) && take(f, si, h[0]) && take(f, sm, h[0]);
  ok = ok && take(f, v1, 3u * (size_t)h[1]) && take(f, e1, 3u * (size_t)h[1]) && take(f, e2, 3u * (size_t)h[1]) && take(f, nr, 3u * (size_t)h[1]) && take(f, tm, h[1]);
  ok = ok && take(f, mats, (size_t)RT_MATERIAL_STRIDE * h[2]) && take(f, lights, (size_t)RT_LIGHT_STRIDE * h[3]);
  ok = ok && take(f, pts, 3u * (size_t)h[4]) && take(f, nrm, 3u * (size_t)h[4]) && take(f, table, 3u * (size_t)h[5]) && take(f, first, h[4]) && take(f, scalars, 2);
  fclose(f);
  if (!ok || h[5] == 0) return fprintf(stderr, "short file\n"), 2;
  const uint32_t n = (uint32_t)strtoul(argv[2], nullptr, 10) < h[4] ? (uint32_t)strtoul(argv[2], nullptr, 10) : h[4];
  const uint32_t S = (uint32_t)strtoul(argv[4], nullptr, 10);
  if (S < 1 || S > RT_OCC_SMAX) return fprintf(stderr, "N_SAMPLES outside 1 .. %u\n", RT_OCC_SMAX), 2;
  rt_scene_desc d{};
  d.abi_version = RT_ABI_VERSION;
  d.n_spheres = h[0], d.sphere_center = sc.data(), d.sphere_r_sq = sr.data(), d.sphere_r_inv = si.data(), d.sphere_material = sm.data();
  d.n_triangles = h[1], d.tri_v1 = v1.data(), d.tri_e1 = e1.data(), d.tri_e2 = e2.data(), d.tri_normal = nr.data(), d.tri_material = tm.data();
  d.n_materials = h[2], d.materials = mats.data();
  d.n_lights = h[3], d.lights = lights.data();
  d.bvh.split_depth = (uint32_t)strtoul(argv[3], nullptr, 10);
  RtPackedScene pk;
  if (rt_pack_scene(&d, RT_SCENE_BUDGET_DEFAULT, &pk) != 0) return fprintf(stderr, "rt_pack_scene: %s\n", rt_last_error()), 1;
  // exactly n * words entries in the bit plane and n in the others: a row written past its end is an access outside the array
  const uint32_t words = rt_occ_words(S);
  std::vector<uint32_t> bits((size_t)n * words), bits0, clear(n), clear0;
  std::vector<float> vis(n), bent(3u * (size_t)n);
  unsigned long long occluded = 0, open = 0, mixed = 0, passed = 0, limited = 0, same_lbvh = 0, same_ploc = 0;
  for (int pass = 0; pass < 5; pass++) {
    if (pass >= 3) {
      if (rt_check_rebuild(pk.dev) != 0) break;  // (a split-clipped tree is not rebuilt)
      if (pass == 3 && rt_rebuild_packed(&pk, 0) != 0) return fprintf(stderr, "rt_rebuild_packed: %s\n", rt_last_error()), 1;
      if (pass == 4 && rt_rebuild_ploc_packed(&pk, 0, 0) != 0) return fprintf(stderr, "rt_rebuild_ploc_packed: %s\n", rt_last_error()), 1;
    }
    // pass 0: every plane, start rows, max_distance +inf; pass 1: transmissive objects pass, bits and clear only, no start rows;
    // pass 2: the file's max_distance; passes 3 and 4: after the rebuilds, as pass 0
    RtOcclusionArgs a;
    memset(&a, 0, sizeof(a));
    a.point = pts.data(), a.normal = nrm.data(), a.table = table.data(), a.n = n, a.n_samples = S, a.n_table = h[5];
    a.bias = scalars[0], a.max_distance = pass == 2 ? scalars[1] : INFINITY;
    a.bits = bits.data(), a.clear = clear.data();
    if (pass != 1) a.first = first.data(), a.visibility = vis.data(), a.bent_normal = bent.data();
    if (pass == 1) a.pass = 1u;
    rt_occlusion_packed(pk, a);
    for (uint32_t i = 0; i < n; i++) {
      unsigned long long set = 0;
      for (uint32_t w = 0; w < words; w++) set += (unsigned long long)__builtin_popcount(bits[(size_t)i * words + w]);
      if (set + clear[i] != S) return fprintf(stderr, "point %u: %llu bits set, clear %u of %u\n", i, set, clear[i], S), 1;
      if (S % 32u && (bits[(size_t)i * words + words - 1u] >> (S % 32u))) return fprintf(stderr, "point %u: high bits set\n", i), 1;
      if (pass != 1) {
        if (vis[i] != (float)clear[i] / (float)S) return fprintf(stderr, "point %u: visibility %g\n", i, vis[i]), 1;
        const float len = bent[3u * i] * bent[3u * i] + bent[3u * i + 1u] * bent[3u * i + 1u] + bent[3u * i + 2u] * bent[3u * i + 2u];
        if (!(len == 0.0f || fabsf(len - 1.0f) < 1e-5f) || (clear[i] == 0 && len != 0.0f)) return fprintf(stderr, "point %u: bent normal of length^2 %g\n", i, len), 1;
      }
      if (pass == 0) occluded += set, open += clear[i], mixed += set != 0 && clear[i] != 0;
      if (pass == 1) passed += clear[i];
      if (pass == 2) limited += clear[i];
    }
    if (pass == 0) bits0 = bits, clear0 = clear;
    if (pass == 3) same_lbvh = bits == bits0 && clear == clear0 ? n : 0;
    if (pass == 4) same_ploc = bits == bits0 && clear == clear0 ? n : 0;
  }
  printf("points %u samples %u occluded %llu clear %llu mixed %llu passed %llu limited %llu slots %u nodes %u same_after_lbvh %llu same_after_ploc %llu\n", n, S,
         occluded, open, mixed, passed, limited, pk.dev.n_slots, pk.dev.n_nodes, same_lbvh, same_ploc);
  return 0;
}
