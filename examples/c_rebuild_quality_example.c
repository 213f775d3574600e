/*
 * c_rebuild_quality_example.c -- a tree repaired from plain C, by surface area and only if it pays.  A small heightfield is
 * created, then shuffled in place with rt_scene_update: the cells of the field trade places, so the tree of creation groups
 * strangers.  rt_scene_rebuild_with builds a PLOC tree (RT_REBUILD_PLOC) on the device from the geometry the handle holds
 * and, with RT_REBUILD_KEEP_BETTER, swaps it in only if its SAH cost is lower than the cost of the tree in place; the report
 * says what was compared.  The same call again builds the same candidate, which is not better than itself: the tree in
 * place stays, and nothing the handle has cached is invalidated.  Without a GPU it says so and exits 0.
 *
 *   gcc -I include examples/c_rebuild_quality_example.c -L hslu_i/ba_raytracing/f2501_raytracer_amd -lrt_hip \
 *       -Wl,-rpath,$PWD/hslu_i/ba_raytracing/f2501_raytracer_amd -lm -o /tmp/c_rebuild_quality_example
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rt_hip.h"

#define M 24 /* cells per side */
#define N_TRI (2 * M * M)

static float height(float x, float z) { return 0.25f + 0.08f * sinf(9.0f * x) * cosf(7.0f * z); }

/* the two triangles of cell (i, j) of the field, written as triangles 2 t and 2 t + 1 */
static void cell(int i, int j, int t, float* v1, float* e1, float* e2, float* normal) {
  const float x0 = 0.1f + 0.8f * i / M, x1 = 0.1f + 0.8f * (i + 1) / M, z0 = 0.2f + 0.6f * j / M, z1 = 0.2f + 0.6f * (j + 1) / M;
  const float p[4][3] = {{x0, height(x0, z0), z0}, {x1, height(x1, z0), z0}, {x0, height(x0, z1), z1}, {x1, height(x1, z1), z1}};
  const int corner[2][3] = {{0, 2, 1}, {3, 1, 2}};
  for (int h = 0; h < 2; h++) {
    float* a = v1 + 3 * (2 * t + h);
    float* b = e1 + 3 * (2 * t + h);
    float* c = e2 + 3 * (2 * t + h);
    float* n = normal + 3 * (2 * t + h);
    for (int k = 0; k < 3; k++) a[k] = p[corner[h][0]][k], b[k] = p[corner[h][1]][k] - a[k], c[k] = p[corner[h][2]][k] - a[k];
    n[0] = b[1] * c[2] - b[2] * c[1], n[1] = b[2] * c[0] - b[0] * c[2], n[2] = b[0] * c[1] - b[1] * c[0];
    const float len = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    for (int k = 0; k < 3; k++) n[k] /= len;
  }
}

int main(void) {
  float* v1 = (float*)malloc(4 * 3 * N_TRI * sizeof(float));
  float *e1 = v1 + 3 * N_TRI, *e2 = e1 + 3 * N_TRI, *normal = e2 + 3 * N_TRI;
  uint32_t* tri_material = (uint32_t*)calloc(N_TRI, 4);
  for (int t = 0; t < M * M; t++) cell(t / M, t % M, t, v1, e1, e2, normal);
  const float materials[RT_MATERIAL_STRIDE] = {0.9f, 0.6f, 0.2f, 0.1f, 0.4f, 1.0f, 0.0f, 0.0f, 0.0f};
  const float lights[RT_LIGHT_STRIDE] = {0.8f, 0.9f, 0.0f, 1.0f, 1.0f, 1.0f, 0.9f};

  rt_scene_desc d;
  memset(&d, 0, sizeof(d));
  d.abi_version = RT_ABI_VERSION;
  d.n_triangles = N_TRI;
  d.tri_v1 = v1, d.tri_e1 = e1, d.tri_e2 = e2, d.tri_normal = normal, d.tri_material = tri_material;
  d.n_materials = 1;
  d.materials = materials;
  d.n_lights = 1;
  d.lights = lights;

  if (rt_device_count() <= 0) {
    printf("no HIP device: ABI links, nothing rendered\n");
    return 0;
  }
  rt_scene* scene = NULL;
  if (rt_scene_create(&d, 0, &scene) != RT_OK) {
    fprintf(stderr, "rt_scene_create: %s\n", rt_last_error());
    return 1;
  }
  /* the deformation: cell t takes the place of cell (t * 245) mod M^2 (245 and M^2 = 576 share no factor) -- the same
   * field, every triangle somewhere else */
  for (int t = 0; t < M * M; t++) {
    const int from = (int)(((long)t * 245) % (M * M));
    cell(from / M, from % M, t, v1, e1, e2, normal);
  }
  rt_scene_delta u;
  memset(&u, 0, sizeof(u));
  u.abi_version = RT_ABI_VERSION;
  u.tri_first = 0, u.tri_count = N_TRI;
  u.tri_v1 = v1, u.tri_e1 = e1, u.tri_e2 = e2, u.tri_normal = normal;
  int rc = 1;
  rt_rebuild_desc desc;
  memset(&desc, 0, sizeof(desc));
  desc.method = RT_REBUILD_PLOC; /* radius 0: the default, 8 */
  desc.flags = RT_REBUILD_KEEP_BETTER;
  rt_rebuild_report r;
  do {
    if (rt_scene_update(scene, &u, NULL) != RT_OK) break;
    for (int call = 0; call < 2; call++) {
      if (rt_scene_rebuild_with(scene, &desc, &r) != RT_OK) break;
      printf("call %d: sah in place %.2f, candidate %.2f (%u PLOC iterations): swapped %u\n", call, r.sah_before, r.sah_after, r.iterations, r.swapped);
      printf("        tree in place: %u nodes, %u leaves, depth %u; tables invalidated 0x%x; %.3f ms, %.3f ms on the device\n", r.info.n_nodes,
             r.info.n_leaves, r.info.max_depth, r.info.tables_invalidated, r.info.total_ms, r.info.device_ms);
      if (!r.swapped) printf("        kept the tree in place\n");
      rc = call == 0 ? !(r.swapped == 1 && r.sah_after < r.sah_before) : !(r.swapped == 0 && r.info.tables_invalidated == 0);
      if (rc) break;
    }
  } while (0);
  if (rc) fprintf(stderr, "failed: %s\n", rt_last_error());
  free(v1), free(tri_material);
  rt_scene_destroy(scene);
  return rc;
}
