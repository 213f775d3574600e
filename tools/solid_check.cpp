// solid_check.cpp -- a stand-alone program around the host twin of the containment kernel's walk (rt_solid_packed:
// csrc/rt_solid.h over the blob of csrc/rt_scene_pack.cpp) and of the closest-point walk it follows in a signed-distance call,
// meant to be compiled host-only under -fsanitize=address,undefined: the walk indexes the threaded tree, the leaf records and
// the shading records by values read from memory and writes rows of R entries per point.
//
//   solid_check SCENE.bin N_POINTS RULE
//
// SCENE.bin (tests/test_solid_sanitize.py writes it): uint32 {n_spheres, n_triangles, n_materials, n_lights, n_points,
// n_directions}, then sphere centres, r^2, 1/r (float), sphere materials (uint32), triangle v1, e1, e2, normals (float), triangle
// materials (uint32), materials, lights, the points [n_points][3] and the directions [n_directions][3] (float).  The scene is
// packed, queried, rebuilt (LBVH, then PLOC) and queried again; a split-clipped pack of it must be refused; the program prints
// what it found.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_closest.h"
#include "rt_scene_pack.h"
#include "rt_solid.h"

template <class T>
static bool take(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 4) return fprintf(stderr, "usage: %s SCENE.bin N_POINTS RULE\n", argv[0]), 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return perror(argv[1]), 2;
  uint32_t h[6];
  if (fread(h, 4, 6, f) != 6) return fprintf(stderr, "bad header\n"), 2;
  std::vector<float> sc, sr, si, v1, e1, e2, nr, mats, lights, pts, dirs;
  std::vector<uint32_t> sm, tm;
  bool ok = take(f, sc, 3u * h[0]) && take(f, sr, h[0]) && take(f, si, h[0]) && take(f, sm, h[0]);
  ok = ok && take(f, v1, 3u * (size_t)h[1]) && take(f, e1, 3u * (size_t)h[1]) && take(f, e2, 3u * (size_t)h[1]) && take(f, nr, 3u * (size_t)h[1]) && take(f, tm, h[1]);
  ok = ok && take(f, mats, (size_t)RT_MATERIAL_STRIDE * h[2]) && take(f, lights, (size_t)RT_LIGHT_STRIDE * h[3]);
  ok = ok && take(f, pts, 3u * (size_t)h[4]) && take(f, dirs, 3u * (size_t)h[5]);
  fclose(f);
  const uint32_t R = h[5];
  if (!ok || R < 1 || R > RT_SOLID_RMAX) return fprintf(stderr, "short file, or n_directions outside 1 .. %u\n", RT_SOLID_RMAX), 2;
  for (uint32_t r = 0; r < R; r++)
    if (!rt_solid_direction_ok(dirs.data() + 3u * r)) return fprintf(stderr, "direction %u is refused\n", r), 2;
  const uint32_t n = (uint32_t)strtoul(argv[2], nullptr, 10) < h[4] ? (uint32_t)strtoul(argv[2], nullptr, 10) : h[4];
  const uint32_t rule = (uint32_t)strtoul(argv[3], nullptr, 10);
  rt_scene_desc d{};
  d.abi_version = RT_ABI_VERSION;
  d.n_spheres = h[0], d.sphere_center = sc.data(), d.sphere_r_sq = sr.data(), d.sphere_r_inv = si.data(), d.sphere_material = sm.data();
  d.n_triangles = h[1], d.tri_v1 = v1.data(), d.tri_e1 = e1.data(), d.tri_e2 = e2.data(), d.tri_normal = nr.data(), d.tri_material = tm.data();
  d.n_materials = h[2], d.materials = mats.data();
  d.n_lights = h[3], d.lights = lights.data();
  RtPackedScene pk;
  // a split-clipped pack is refused, and nothing is written for it
  unsigned refused = 0;
  if (h[1]) {
    d.bvh.split_depth = 3;
    if (rt_pack_scene(&d, RT_SCENE_BUDGET_DEFAULT, &pk) != 0) return fprintf(stderr, "rt_pack_scene: %s\n", rt_last_error()), 1;
    if (pk.dev.n_slots > pk.dev.n_triangles) {
      RtSolidArgs a;
      memset(&a, 0, sizeof(a));  // (no plane: a write would be a null dereference)
      a.point = pts.data(), a.n = n, a.n_dirs = R, a.rule = rule;
      memcpy(a.dir, dirs.data(), (size_t)R * 12u);
      if (rt_solid_packed(pk, a) != RT_ERR_UNSUPPORTED) return fprintf(stderr, "a split-clipped tree was not refused\n"), 1;
      refused = 1;
    }
    d.bvh.split_depth = 0;
  }
  if (rt_pack_scene(&d, RT_SCENE_BUDGET_DEFAULT, &pk) != 0) return fprintf(stderr, "rt_pack_scene: %s\n", rt_last_error()), 1;
  // exactly n * R entries in the row planes and n in the others: a row written past its end is an access outside the array
  std::vector<uint8_t> inside(n), votes(n), inside0, votes0;
  std::vector<uint32_t> crossings((size_t)n * R), crossings0;
  std::vector<int32_t> winding((size_t)n * R), winding0;
  std::vector<float> sd(n), sd0, dist(n);
  unsigned long long n_inside = 0, mixed = 0, crossed = 0, negative = 0, same_lbvh = 0, same_ploc = 0;
  long long wound = 0;
  for (int pass = 0; pass < 4; pass++) {
    if (pass >= 2) {
      if (rt_check_rebuild(pk.dev) != 0) break;  // (a scene without triangles is not rebuilt)
      if (pass == 2 && rt_rebuild_packed(&pk, 0) != 0) return fprintf(stderr, "rt_rebuild_packed: %s\n", rt_last_error()), 1;
      if (pass == 3 && rt_rebuild_ploc_packed(&pk, 0, 0) != 0) return fprintf(stderr, "rt_rebuild_ploc_packed: %s\n", rt_last_error()), 1;
    }
    // pass 1: the distance travels in the signed-distance plane, as in a call without a distance plane; else through one of its own
    RtClosestArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.point = pts.data(), ca.n = n, ca.distance = pass == 1 ? sd.data() : dist.data();
    rt_closest_packed(pk, ca);
    RtSolidArgs a;
    memset(&a, 0, sizeof(a));
    a.point = pts.data(), a.n = n, a.n_dirs = R, a.rule = rule;
    memcpy(a.dir, dirs.data(), (size_t)R * 12u);
    a.inside = inside.data(), a.votes = votes.data(), a.crossings = crossings.data(), a.winding = winding.data();
    a.distance = ca.distance, a.signed_distance = sd.data();
    if (rt_solid_packed(pk, a) != 0) return fprintf(stderr, "rt_solid_packed: %s\n", rt_last_error()), 1;
    for (uint32_t i = 0; i < n; i++) {
      if (votes[i] > R || inside[i] != (2u * votes[i] > R ? 1 : 0)) return fprintf(stderr, "point %u: votes %u of %u, inside %u\n", i, votes[i], R, inside[i]), 1;
      if ((std::signbit(sd[i]) ? 1 : 0) != inside[i]) return fprintf(stderr, "point %u: signed distance %g, inside %u\n", i, sd[i], inside[i]), 1;
      if (pass == 0) {
        n_inside += inside[i], mixed += votes[i] != 0 && votes[i] != R, negative += sd[i] < 0.0f;
        for (uint32_t r = 0; r < R; r++) crossed += crossings[(size_t)i * R + r], wound += winding[(size_t)i * R + r];
      }
    }
    const bool same = inside == inside0 && votes == votes0 && crossings == crossings0 && winding == winding0 &&
                      memcmp(sd.data(), sd0.data(), (size_t)n * 4u) == 0;
    if (pass == 0) inside0 = inside, votes0 = votes, crossings0 = crossings, winding0 = winding, sd0 = sd;
    if (pass == 1 && !same) return fprintf(stderr, "the distance plane changed the result\n"), 1;
    if (pass == 2) same_lbvh = same ? n : 0;
    if (pass == 3) same_ploc = same ? n : 0;
  }
  printf("points %u directions %u inside %llu mixed %llu crossings %llu winding %lld negative %llu refused %u slots %u nodes %u same_after_lbvh %llu "
         "same_after_ploc %llu\n", n, R, n_inside, mixed, crossed, wound, negative, refused, pk.dev.n_slots, pk.dev.n_nodes, same_lbvh, same_ploc);
  return 0;
}
