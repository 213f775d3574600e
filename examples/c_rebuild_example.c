/*
 * c_rebuild_example.c -- a tree repaired from plain C.  A small heightfield is created, then deformed in place with
 * rt_scene_update until its refitted tree has decayed: the cells of the field trade places, so the tree of creation groups
 * strangers.  rt_scene_bvh_quality reports the SAH cost; rt_scene_rebuild builds a new tree on the device from the geometry
 * the handle holds; the cost is reported again and a frame is rendered before and after -- the same hit ids, the same
 * picture.  Without a GPU it says so and exits 0.
 *
 *   gcc -I include examples/c_rebuild_example.c -L hslu_i/ba_raytracing/f2501_raytracer_amd -lrt_hip \
 *       -Wl,-rpath,$PWD/hslu_i/ba_raytracing/f2501_raytracer_amd -lm -o /tmp/c_rebuild_example
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rt_hip.h"

#define W 96
#define H 80
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

static uint32_t checksum(const uint32_t* argb) {
  uint32_t sum = 2166136261u; /* FNV-1a over the packed pixels */
  for (int i = 0; i < W * H; i++) sum = (sum ^ argb[i]) * 16777619u;
  return sum;
}

int main(void) {
  const float sh = (float)H / W, sd = (1.0f + sh) / 2.0f;
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
  rt_params p;
  memset(&p, 0, sizeof(p));
  p.abi_version = RT_ABI_VERSION;
  p.width = W, p.height = H;
  p.focus[0] = 0.5f, p.focus[1] = sh / 2.0f, p.focus[2] = -1.9f * sd;
  p.fw = 1.0f / W, p.fh = sh / H, p.fd = sd;
  p.eps_distance = 1e-4f, p.air_ior = 1.0f, p.ambient = 0.1f;
  p.light_mult = 1;
  p.tile_size = 48;

  /* the deformation: cell t takes the place of cell (t * 577) mod M^2 -- the same field, every triangle somewhere else */
  for (int t = 0; t < M * M; t++) {
    const int from = (int)(((long)t * 577) % (M * M));
    cell(from / M, from % M, t, v1, e1, e2, normal);
  }
  rt_scene_delta u;
  memset(&u, 0, sizeof(u));
  u.abi_version = RT_ABI_VERSION;
  u.tri_first = 0, u.tri_count = N_TRI;
  u.tri_v1 = v1, u.tri_e1 = e1, u.tri_e2 = e2, u.tri_normal = normal;
  int rc = 1;
  uint32_t* argb = (uint32_t*)calloc(2 * W * H, 4);
  int32_t* ids = (int32_t*)calloc(2 * W * H, 4);
  rt_bvh_quality q;
  rt_rebuild_info info;
  rt_aux aux;
  rt_stats st;
  memset(&aux, 0, sizeof(aux));
  do {
    if (rt_scene_update(scene, &u, NULL) != RT_OK || rt_scene_bvh_quality(scene, &q) != RT_OK) break;
    printf("refitted: sah %.2f (created: %.2f)\n", q.sah_now, q.sah_created);
    aux.hit_id = ids;
    if (rt_render(scene, &p, argb, &aux, &st) != RT_OK) break;
    printf("refitted: checksum %08x\n", checksum(argb));
    if (rt_scene_rebuild(scene, &info) != RT_OK || rt_scene_bvh_quality(scene, &q) != RT_OK) break;
    printf("rebuilt:  sah %.2f (created: %.2f); %u nodes, %u leaves, depth %u, %.3f ms\n", q.sah_now, q.sah_created, info.n_nodes, info.n_leaves,
           info.max_depth, info.total_ms);
    aux.hit_id = ids + W * H;
    if (rt_render(scene, &p, argb + W * H, &aux, &st) != RT_OK) break;
    printf("rebuilt:  checksum %08x\n", checksum(argb + W * H));
    rc = memcmp(ids, ids + W * H, W * H * 4) != 0;
    printf(rc ? "hit ids DIFFER\n" : "hit ids equal before and after the rebuild\n");
  } while (0);
  if (rc) fprintf(stderr, "failed: %s\n", rt_last_error());
  free(argb), free(ids), free(v1), free(tri_material);
  rt_scene_destroy(scene);
  return rc;
}
