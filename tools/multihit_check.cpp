// multihit_check.cpp -- a stand-alone program around the host twin of the multi-hit kernel's walk (rt_multihit_packed:
// csrc/rt_multihit.h over the blob of csrc/rt_scene_pack.cpp), meant to be compiled host-only under -fsanitize=address,undefined:
// the walk indexes the threaded tree, the leaf records, the material rows and the canonical shading records by values read
// from memory, and writes rows of max_hits entries per ray.
//
//   multihit_check SCENE.bin N_RAYS SPLIT_DEPTH MAX_HITS
//
// SCENE.bin (tests/test_multihit_sanitize.py writes it): uint32 {n_spheres, n_triangles, n_materials, n_lights, n_rays}, then
// sphere centres, r^2, 1/r (float), sphere materials (uint32), triangle v1, e1, e2, normals (float), triangle materials (uint32),
// materials, lights, the ray origins and directions [n_rays][3] and their max_distance [n_rays] (float).  The scene is packed
// (with split clipping of SPLIT_DEPTH), queried, rebuilt where that is allowed and queried again; the program prints what it found.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_multihit.h"
#include "rt_scene_pack.h"

template <class T>
static bool take(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 5) return fprintf(stderr, "usage: %s SCENE.bin N_RAYS SPLIT_DEPTH MAX_HITS\n", argv[0]), 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return perror(argv[1]), 2;
  uint32_t h[5];
  if (fread(h, 4, 5, f) != 5) return fprintf(stderr, "bad header\n"), 2;
  std::vector<float> sc, sr, si, v1, e1, e2, nr, mats, lights, org, dir, maxd;
  std::vector<uint32_t> sm, tm;
  bool ok = take(f, sc, 3u * h[0]) && take(f, sr, h[0]) && take(f, si, h[0]) && take(f, sm, h[0]);
  ok = ok && take(f, v1, 3u * (size_t)h[1]) && take(f, e1, 3u * (size_t)h[1]) && take(f, e2, 3u * (size_t)h[1]) && take(f, nr, 3u * (size_t)h[1]) && take(f, tm, h[1]);
  ok = ok && take(f, mats, (size_t)RT_MATERIAL_STRIDE * h[2]) && take(f, lights, (size_t)RT_LIGHT_STRIDE * h[3]);
  ok = ok && take(f, org, 3u * (size_t)h[4]) && take(f, dir, 3u * (size_t)h[4]) && take(f, maxd, h[4]);
  fclose(f);
  if (!ok) return fprintf(stderr, "short file\n"), 2;
  const uint32_t n = (uint32_t)strtoul(argv[2], nullptr, 10) < h[4] ? (uint32_t)strtoul(argv[2], nullptr, 10) : h[4];
  const uint32_t K = (uint32_t)strtoul(argv[4], nullptr, 10);
  if (K < 1 || K > RT_MH_KMAX) return fprintf(stderr, "MAX_HITS outside 1 .. %d\n", RT_MH_KMAX), 2;
  rt_scene_desc d{};
  d.abi_version = RT_ABI_VERSION;
  d.n_spheres = h[0], d.sphere_center = sc.data(), d.sphere_r_sq = sr.data(), d.sphere_r_inv = si.data(), d.sphere_material = sm.data();
  d.n_triangles = h[1], d.tri_v1 = v1.data(), d.tri_e1 = e1.data(), d.tri_e2 = e2.data(), d.tri_normal = nr.data(), d.tri_material = tm.data();
  d.n_materials = h[2], d.materials = mats.data();
  d.n_lights = h[3], d.lights = lights.data();
  d.bvh.split_depth = (uint32_t)strtoul(argv[3], nullptr, 10);
  RtPackedScene pk;
  if (rt_pack_scene(&d, RT_SCENE_BUDGET_DEFAULT, &pk) != 0) return fprintf(stderr, "rt_pack_scene: %s\n", rt_last_error()), 1;
  // exactly n * K entries per plane: a row written past its end is an access outside the array
  const size_t nk = (size_t)n * K;
  std::vector<uint32_t> count(n), total(n), total0(n), mat(nk);
  std::vector<int32_t> id(nk), cur_id(n);
  std::vector<float> t(nk), p(3u * nk), nrm(3u * nk), cur_t(n);
  unsigned long long hits = 0, objects = 0, full = 0, paged = 0, same = 0;
  for (int pass = 0; pass < 4; pass++) {
    if (pass == 3) {
      if (rt_check_rebuild(pk.dev) != 0) break;  // (a split-clipped tree is not rebuilt)
      if (rt_rebuild_packed(&pk, 0) != 0) return fprintf(stderr, "rt_rebuild_packed: %s\n", rt_last_error()), 1;
    }
    // pass 0: every plane, total, no max_distance; pass 1: culling, max_distance, count and id only; pass 2: behind the cursor
    // of pass 0's last keys; pass 3: after the rebuild, as pass 0
    RtMultiHitArgs a;
    memset(&a, 0, sizeof(a));
    a.origin = org.data(), a.direction = dir.data(), a.n = n, a.max_hits = K;
    a.count = count.data(), a.id = id.data();
    if (pass == 1) a.max_distance = maxd.data(), a.cull = 1u;
    if (pass != 1) a.total = total.data(), a.t = t.data(), a.point = p.data(), a.normal = nrm.data(), a.material = mat.data();
    if (pass == 2) a.after_t = cur_t.data(), a.after_id = cur_id.data();
    rt_multihit_packed(pk, a);
    for (uint32_t i = 0; i < n; i++) {
      if (count[i] > K) return fprintf(stderr, "ray %u: count %u\n", i, count[i]), 1;
      for (uint32_t j = 0; j < K; j++) {
        const int32_t got = id[(size_t)i * K + j];
        if (j < count[i] ? (got < 0 || got >= (int32_t)(h[0] + h[1])) : got != -1) return fprintf(stderr, "ray %u entry %u: id %d\n", i, j, got), 1;
        if (pass != 1 && j + 1 < count[i] && !(t[(size_t)i * K + j] <= t[(size_t)i * K + j + 1])) return fprintf(stderr, "ray %u: order\n", i), 1;
      }
      if (pass != 1 && (total[i] < count[i] || (count[i] < K && total[i] != count[i]))) return fprintf(stderr, "ray %u: total %u count %u\n", i, total[i], count[i]), 1;
      if (pass == 0) {
        hits += count[i], objects += total[i], full += count[i] == K, total0[i] = total[i];
        cur_t[i] = count[i] ? t[(size_t)i * K + count[i] - 1] : INFINITY, cur_id[i] = count[i] ? id[(size_t)i * K + count[i] - 1] : -1;
      }
      if (pass == 2) {
        if (total[i] + (total0[i] < K ? total0[i] : K) != total0[i]) return fprintf(stderr, "ray %u: %u behind the cursor of %u\n", i, total[i], total0[i]), 1;
        paged += count[i];
      }
      if (pass == 3) same += total[i] == total0[i];
    }
  }
  printf("rays %u hits %llu objects %llu full %llu paged %llu slots %u nodes %u same_after_rebuild %llu\n", n, hits, objects, full, paged,
         pk.dev.n_slots, pk.dev.n_nodes, same);
  return 0;
}
