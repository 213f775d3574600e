/*
 * c_ambient_occlusion_example.c -- the ambient-occlusion query from plain C: a ball on a floor beside a wall, a 24 x 24 grid of
 * rays looking down at it, and at every hit point the share of 32 hemisphere directions that reach 2 units without a hit.  The
 * hit points and normals of the nearest-hit query go into the occlusion query as they are.  The chain runs through the
 * specifications on the host (rt_list_intersections_model at K = 1, whose entry 0 is rt_cast_rays' answer, then
 * rt_ambient_occlusion_model) and, when there is a GPU, through rt_cast_rays and rt_ambient_occlusion, and the two checksums
 * are compared.  Without a GPU it runs the models alone, says so and exits 0.
 *
 *   gcc -I include examples/c_ambient_occlusion_example.c -L hslu_i/ba_raytracing/f2501_raytracer_amd -lrt_hip \
 *       -Wl,-rpath,$PWD/hslu_i/ba_raytracing/f2501_raytracer_amd -lm -o /tmp/c_ambient_occlusion_example
 */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "rt_hip.h"

#define GRID 24
#define N (GRID * GRID)
#define S 32

typedef struct {
  int32_t id[N];
  float point[N][3], normal[N][3];
  uint32_t bits[N], clear[N];
  float visibility[N], bent[N][3];
} result;

/* FNV-1a over the words of a plane */
static uint64_t fnv(uint64_t h, const void* data, size_t bytes) {
  const unsigned char* p = (const unsigned char*)data;
  for (size_t k = 0; k < bytes; k++) h = (h ^ p[k]) * 1099511628211ull;
  return h;
}
static uint64_t checksum(const result* r) {
  uint64_t h = 14695981039346656037ull;
  h = fnv(h, r->id, sizeof(r->id)), h = fnv(h, r->point, sizeof(r->point)), h = fnv(h, r->normal, sizeof(r->normal));
  h = fnv(h, r->bits, sizeof(r->bits)), h = fnv(h, r->clear, sizeof(r->clear));
  return fnv(fnv(h, r->visibility, sizeof(r->visibility)), r->bent, sizeof(r->bent));
}

/* nearest hits, then occlusion at them; scene NULL: the models */
static int chain(rt_scene* scene, const rt_scene_desc* d, const rt_ray_batch* rays, const float* table, result* r) {
  int rc;
  if (scene) {
    rt_ray_hits h;
    memset(&h, 0, sizeof(h));
    h.id = r->id, h.point = &r->point[0][0], h.normal = &r->normal[0][0];
    rc = rt_cast_rays(scene, rays, &h);
  } else {
    rt_ray_hit_lists l;
    memset(&l, 0, sizeof(l));
    l.max_hits = 1;
    l.id = r->id, l.point = &r->point[0][0], l.normal = &r->normal[0][0];
    rc = rt_list_intersections_model(d, rays, &l);
  }
  if (rc != RT_OK) return rc;
  /* (a ray that missed has the point and normal 0: a zero normal makes a dead point, which counts as fully occluded) */
  rt_occlusion_batch b;
  memset(&b, 0, sizeof(b));
  b.abi_version = RT_ABI_VERSION;
  b.n_points = N, b.point = &r->point[0][0], b.normal = &r->normal[0][0];
  b.n_samples = S, b.n_table = S, b.table = table;
  b.bias = 1e-4f, b.max_distance = 2.0f;
  rt_occlusion_out o;
  memset(&o, 0, sizeof(o));
  o.bits = r->bits, o.clear = r->clear, o.visibility = r->visibility, o.bent_normal = &r->bent[0][0];
  return scene ? rt_ambient_occlusion(scene, &b, &o) : rt_ambient_occlusion_model(d, &b, &o);
}

int main(void) {
  /* the floor z = 0 (two triangles, normal +z), a wall x = 2 (two triangles, normal -x) and a ball of radius 0.5 on the floor */
  const float sphere_center[1][3] = {{0.0f, 0.0f, 0.5f}};
  const float sphere_r_sq[1] = {0.25f}, sphere_r_inv[1] = {2.0f};
  const uint32_t sphere_material[1] = {0};
  const float tri_v1[4][3] = {{-4, -4, 0}, {4, 4, 0}, {2, -4, 0}, {2, 4, 4}};
  const float tri_e1[4][3] = {{8, 0, 0}, {-8, 0, 0}, {0, 8, 0}, {0, -8, 0}};
  const float tri_e2[4][3] = {{0, 8, 0}, {0, -8, 0}, {0, 0, 4}, {0, 0, -4}};
  const float tri_normal[4][3] = {{0, 0, 1}, {0, 0, 1}, {-1, 0, 0}, {-1, 0, 0}};
  const uint32_t tri_material[4] = {1, 1, 1, 1};
  const float materials[2 * RT_MATERIAL_STRIDE] = {
      1.0f, 0.2f, 0.2f, 0.0f, 0.3f, 1.0f, 0.0f, 0.0f, 0.0f, /* red, shiny */
      0.5f, 0.75f, 0.75f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f /* floor and wall */
  };
  const float lights[RT_LIGHT_STRIDE] = {0.3f, 0.1f, 5.0f, 1.0f, 1.0f, 1.0f, 0.8f};

  rt_scene_desc d;
  memset(&d, 0, sizeof(d));
  d.abi_version = RT_ABI_VERSION;
  d.n_spheres = 1;
  d.sphere_center = &sphere_center[0][0];
  d.sphere_r_sq = sphere_r_sq;
  d.sphere_r_inv = sphere_r_inv;
  d.sphere_material = sphere_material;
  d.n_triangles = 4;
  d.tri_v1 = &tri_v1[0][0];
  d.tri_e1 = &tri_e1[0][0];
  d.tri_e2 = &tri_e2[0][0];
  d.tri_normal = &tri_normal[0][0];
  d.tri_material = tri_material;
  d.n_materials = 2;
  d.materials = materials;
  d.n_lights = 1;
  d.lights = lights;

  /* rays straight down from z = 3 over [-1.5, 2.5]^2: onto the ball, the floor around it and the floor behind the wall; the
   * twelve rays above the floor's diagonal fall between its two triangles (the test's u + v < 1 is strict) and miss */
  static float origin[N][3], direction[N][3];
  for (int y = 0; y < GRID; y++)
    for (int x = 0; x < GRID; x++) {
      float* o = origin[y * GRID + x];
      o[0] = -1.5f + 4.0f * ((float)x + 0.5f) / GRID, o[1] = -1.5f + 4.0f * ((float)y + 0.5f) / GRID, o[2] = 3.0f;
      direction[y * GRID + x][2] = -1.0f;
    }
  rt_ray_batch rays;
  memset(&rays, 0, sizeof(rays));
  rays.abi_version = RT_ABI_VERSION;
  rays.n_rays = N;
  rays.origin = &origin[0][0];
  rays.direction = &direction[0][0];

  /* S cosine-weighted directions about +z: a golden-angle spiral over the disc, lifted to the hemisphere */
  static float table[S][3];
  for (int k = 0; k < S; k++) {
    const double r2 = (k + 0.5) / S, phi = k * 3.14159265358979323846 * (3.0 - sqrt(5.0));
    table[k][0] = (float)(sqrt(r2) * cos(phi)), table[k][1] = (float)(sqrt(r2) * sin(phi)), table[k][2] = (float)sqrt(1.0 - r2);
  }

  static result model, device;
  if (chain(NULL, &d, &rays, &table[0][0], &model) != RT_OK) {
    fprintf(stderr, "model: %s\n", rt_last_error());
    return 1;
  }
  unsigned hits = 0, open = 0;
  double floor_far, floor_near;
  for (int i = 0; i < N; i++) hits += model.id[i] >= 0, open += model.clear[i];
  /* the floor far from everything (x = -1.4) and right beside the ball (x = 0.6), on a row through the ball */
  floor_far = model.visibility[(GRID / 2 - 3) * GRID + 0];
  floor_near = model.visibility[(GRID / 2 - 3) * GRID + GRID / 2 + 0];
  printf("hits %u of %d rays, clear samples %u of %u\n", hits, N, open, hits * S);
  printf("visibility of the open floor %.3f, of the floor beside the ball %.3f\n", floor_far, floor_near);
  printf("model checksum %016llx\n", (unsigned long long)checksum(&model));
  if (!(floor_far > floor_near)) return 1;

  if (rt_device_count() <= 0) {
    printf("no HIP device: the model alone\n");
    return 0;
  }
  rt_scene* scene = NULL;
  if (rt_scene_create(&d, 0, &scene) != RT_OK) {
    fprintf(stderr, "rt_scene_create: %s\n", rt_last_error());
    return 1;
  }
  int rc = 0;
  if (chain(scene, &d, &rays, &table[0][0], &device) != RT_OK) {
    fprintf(stderr, "device: %s\n", rt_last_error());
    rc = 1;
  } else {
    printf("device checksum %016llx\n", (unsigned long long)checksum(&device));
    const int same = !memcmp(&model, &device, sizeof(model));
    printf("device equals model: %s\n", same ? "yes" : "NO");
    rc = same ? 0 : 1;
  }
  rt_scene_destroy(scene);
  return rc;
}
