// closest_check.cpp -- a stand-alone program around the host model of the closest-point kernel's walk (rt_closest_packed:
// csrc/rt_closest.h over the blob of csrc/rt_scene_pack.cpp), meant to be compiled host-only under -fsanitize=address,undefined:
// the walk indexes the BVH2, the threaded tree and the leaf records by values read from memory.
//
//   closest_check SCENE.bin N_POINTS SPLIT_DEPTH
//
// SCENE.bin (tests/test_closest_sanitize.py writes it): uint32 {n_spheres, n_triangles, n_materials, n_lights, n_points}, then
// sphere centres, r^2, 1/r (float), sphere materials (uint32), triangle v1, e1, e2, normals (float), triangle materials (uint32),
// materials, lights, the points [n_points][3] and their radii [n_points] (float).  The scene is packed (with split clipping of
// SPLIT_DEPTH), queried, refitted to itself, rebuilt where that is allowed and queried again; the program prints what it found.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_closest.h"
#include "rt_scene_pack.h"

template <class T>
static bool take(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 4) return fprintf(stderr, "usage: %s SCENE.bin N_POINTS SPLIT_DEPTH\n", argv[0]), 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return perror(argv[1]), 2;
  uint32_t h[5];
  if (fread(h, 4, 5, f) != 5) return fprintf(stderr, "bad header\n"), 2;
  std::vector<float> sc, sr, si, v1, e1, e2, nr, mats, lights, pts, radii;
  std::vector<uint32_t> sm, tm;
  bool ok = take(f, sc, 3u * h[0]) && take(f, sr, h[0]) && take(f, si, h[0]) && take(f, sm, h[0]);
  ok = ok && take(f, v1, 3u * (size_t)h[1]) && take(f, e1, 3u * (size_t)h[1]) && take(f, e2, 3u * (size_t)h[1]) && take(f, nr, 3u * (size_t)h[1]) && take(f, tm, h[1]);
  ok = ok && take(f, mats, (size_t)RT_MATERIAL_STRIDE * h[2]) && take(f, lights, (size_t)RT_LIGHT_STRIDE * h[3]);
  ok = ok && take(f, pts, 3u * (size_t)h[4]) && take(f, radii, h[4]);
  fclose(f);
  if (!ok) return fprintf(stderr, "short file\n"), 2;
  const uint32_t n = (uint32_t)strtoul(argv[2], nullptr, 10) < h[4] ? (uint32_t)strtoul(argv[2], nullptr, 10) : h[4];
  rt_scene_desc d{};
  d.abi_version = RT_ABI_VERSION;
  d.n_spheres = h[0], d.sphere_center = sc.data(), d.sphere_r_sq = sr.data(), d.sphere_r_inv = si.data(), d.sphere_material = sm.data();
  d.n_triangles = h[1], d.tri_v1 = v1.data(), d.tri_e1 = e1.data(), d.tri_e2 = e2.data(), d.tri_normal = nr.data(), d.tri_material = tm.data();
  d.n_materials = h[2], d.materials = mats.data();
  d.n_lights = h[3], d.lights = lights.data();
  d.bvh.split_depth = (uint32_t)strtoul(argv[3], nullptr, 10);
  RtPackedScene pk;
  if (rt_pack_scene(&d, RT_SCENE_BUDGET_DEFAULT, &pk) != 0) return fprintf(stderr, "rt_pack_scene: %s\n", rt_last_error()), 1;
  std::vector<int32_t> id(n), id2(n);
  std::vector<float> dist(n), q(3u * (size_t)n), nrm(3u * (size_t)n), bary(2u * (size_t)n);
  std::vector<uint32_t> mat(n);
  unsigned long long hits = 0, misses = 0, same = 0;
  for (int pass = 0; pass < 3; pass++) {
    if (pass == 2) {
      if (rt_check_rebuild(pk.dev) != 0) break;  // (a split-clipped tree is not rebuilt)
      if (rt_rebuild_packed(&pk, 0) != 0) return fprintf(stderr, "rt_rebuild_packed: %s\n", rt_last_error()), 1;
    }
    // pass 0: every plane, no radii; pass 1: two planes, with radii; pass 2: after the rebuild, as pass 0
    const RtClosestArgs a = {pts.data(), pass == 1 ? radii.data() : nullptr, pass == 2 ? id2.data() : id.data(), dist.data(), pass == 1 ? nullptr : q.data(),
                             pass == 1 ? nullptr : nrm.data(), pass == 1 ? nullptr : bary.data(), pass == 1 ? nullptr : mat.data(), n};
    rt_closest_packed(pk, a);
    for (uint32_t i = 0; i < n; i++) {
      const int32_t got = pass == 2 ? id2[i] : id[i];
      if (got >= (int32_t)(h[0] + h[1])) return fprintf(stderr, "point %u: id %d out of range\n", i, got), 1;
      if (got >= 0 && !(dist[i] >= 0.0f && std::isfinite(dist[i]))) return fprintf(stderr, "point %u: distance %g\n", i, dist[i]), 1;
      if (pass == 0) hits += got >= 0, misses += got < 0;
      if (pass == 2) same += id2[i] == id[i];
    }
    if (pass == 1)  // (ids of pass 0 again for the comparison of pass 2)
      rt_closest_packed(pk, RtClosestArgs{pts.data(), nullptr, id.data(), nullptr, nullptr, nullptr, nullptr, nullptr, n});
  }
  printf("points %u hits %llu misses %llu slots %u nodes %u same_after_rebuild %llu\n", n, hits, misses, pk.dev.n_slots, pk.dev.n_nodes, same);
  return 0;
}
