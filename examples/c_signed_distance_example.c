/*
 * c_signed_distance_example.c -- the containment and signed-distance queries from plain C: a closed box of 12 triangles with a
 * ball sticking out of its top, and a 24 x 24 grid of points on the plane y = 0.1 through both.  For every point: is it inside
 * something, how far is the nearest surface, which object is that.  The query runs through the specification on the host
 * (rt_signed_distance_model) and, when there is a GPU, through rt_signed_distance, and the two checksums are compared.  Without a
 * GPU it runs the model alone, says so and exits 0.
 *
 *   gcc -I include examples/c_signed_distance_example.c -L hslu_i/ba_raytracing/f2501_raytracer_amd -lrt_hip \
 *       -Wl,-rpath,$PWD/hslu_i/ba_raytracing/f2501_raytracer_amd -lm -o /tmp/c_signed_distance_example
 */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "rt_hip.h"

#define GRID 24
#define N (GRID * GRID)
#define R 3

typedef struct {
  float signed_distance[N];
  uint8_t inside[N], votes[N];
  uint32_t crossings[N][R];
  int32_t winding[N][R];
  int32_t id[N];
  float point[N][3];
} result;

/* FNV-1a over the words of a plane */
static uint64_t fnv(uint64_t h, const void* data, size_t bytes) {
  const unsigned char* p = (const unsigned char*)data;
  for (size_t k = 0; k < bytes; k++) h = (h ^ p[k]) * 1099511628211ull;
  return h;
}
static uint64_t checksum(const result* r) {
  uint64_t h = 14695981039346656037ull;
  h = fnv(h, r->signed_distance, sizeof(r->signed_distance)), h = fnv(h, r->inside, sizeof(r->inside)), h = fnv(h, r->votes, sizeof(r->votes));
  h = fnv(h, r->crossings, sizeof(r->crossings)), h = fnv(h, r->winding, sizeof(r->winding));
  return fnv(fnv(h, r->id, sizeof(r->id)), r->point, sizeof(r->point));
}

/* scene NULL: the model */
static int query(rt_scene* scene, const rt_scene_desc* d, const float* points, uint32_t rule, result* r) {
  /* the default table of the Python side: pairwise near-orthogonal, none parallel to an axis or a face diagonal */
  static const float directions[R][3] = {{1, 2, 3}, {2, -3, 1}, {-3, -1, 2}};
  rt_solid_batch b;
  memset(&b, 0, sizeof(b));
  b.abi_version = RT_ABI_VERSION;
  b.n_points = N, b.point = points;
  b.n_directions = R, b.directions = &directions[0][0], b.rule = rule;
  rt_signed_distance_out o;
  memset(&o, 0, sizeof(o));
  memset(r, 0, sizeof(*r));
  o.signed_distance = r->signed_distance;
  o.solid.inside = r->inside, o.solid.votes = r->votes, o.solid.crossings = &r->crossings[0][0], o.solid.winding = &r->winding[0][0];
  o.closest.id = r->id, o.closest.point = &r->point[0][0];
  return scene ? rt_signed_distance(scene, &b, &o) : rt_signed_distance_model(d, &b, &o);
}

int main(void) {
  /* the box [-1, 1]^3: per face two triangles and the outward normal (the vertex order is not what orients them) */
  static float tri_v1[12][3], tri_e1[12][3], tri_e2[12][3], tri_normal[12][3];
  static uint32_t tri_material[12];
  for (int face = 0; face < 6; face++) {
    const int axis = face / 2, u = (axis + 1) % 3, v = (axis + 2) % 3;
    const float side = face % 2 ? 1.0f : -1.0f;
    for (int half = 0; half < 2; half++) {
      const int t = 2 * face + half;
      const float corner = half ? 1.0f : -1.0f;
      tri_v1[t][axis] = side, tri_v1[t][u] = corner, tri_v1[t][v] = corner;
      tri_e1[t][u] = -2.0f * corner, tri_e2[t][v] = -2.0f * corner;
      tri_normal[t][axis] = side;
      tri_material[t] = 1;
    }
  }
  /* a ball of radius 0.75 around (0, 0, 1.25): half in the box, half above it */
  const float sphere_center[1][3] = {{0.0f, 0.0f, 1.25f}};
  const float sphere_r_sq[1] = {0.5625f}, sphere_r_inv[1] = {1.0f / 0.75f};
  const uint32_t sphere_material[1] = {0};
  const float materials[2 * RT_MATERIAL_STRIDE] = {
      1.0f, 0.2f, 0.2f, 0.0f, 0.3f, 1.0f, 0.0f, 0.0f, 0.0f, /* red, shiny */
      0.5f, 0.75f, 0.75f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f /* the box */
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
  d.n_triangles = 12;
  d.tri_v1 = &tri_v1[0][0];
  d.tri_e1 = &tri_e1[0][0];
  d.tri_e2 = &tri_e2[0][0];
  d.tri_normal = &tri_normal[0][0];
  d.tri_material = tri_material;
  d.n_materials = 2;
  d.materials = materials;
  d.n_lights = 1;
  d.lights = lights;

  /* the slice y = 0.1, x in [-2, 2], z in [-2, 3] */
  static float points[N][3];
  for (int k = 0; k < GRID; k++)
    for (int j = 0; j < GRID; j++) {
      float* p = points[k * GRID + j];
      p[0] = -2.0f + 4.0f * ((float)j + 0.5f) / GRID, p[1] = 0.1f, p[2] = -2.0f + 5.0f * ((float)k + 0.5f) / GRID;
    }

  static result parity, winding, device;
  if (query(NULL, &d, &points[0][0], RT_SOLID_RULE_PARITY, &parity) != RT_OK || query(NULL, &d, &points[0][0], RT_SOLID_RULE_WINDING, &winding) != RT_OK) {
    fprintf(stderr, "model: %s\n", rt_last_error());
    return 1;
  }
  unsigned in_parity = 0, in_winding = 0, mixed = 0;
  float deepest = 0.0f;
  for (int i = 0; i < N; i++) {
    in_parity += parity.inside[i], in_winding += winding.inside[i], mixed += parity.votes[i] != 0 && parity.votes[i] != R;
    if (winding.signed_distance[i] < deepest) deepest = winding.signed_distance[i];
  }
  for (int k = GRID - 1; k >= 0; k -= 2) { /* the slice, z upwards: '#' inside by both rules, '+' by winding only (box and ball overlap) */
    for (int j = 0; j < GRID; j++) putchar(parity.inside[k * GRID + j] ? '#' : (winding.inside[k * GRID + j] ? '+' : '.'));
    putchar('\n');
  }
  printf("inside by parity %u, by winding %u of %d points; %u with disagreeing directions; deepest %.4f\n", in_parity, in_winding, N, mixed, deepest);
  printf("model checksum %016llx\n", (unsigned long long)checksum(&winding));
  if (!(in_winding > in_parity && in_parity > 0 && deepest < -0.5f)) return 1;

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
  if (query(scene, &d, &points[0][0], RT_SOLID_RULE_WINDING, &device) != RT_OK) {
    fprintf(stderr, "device: %s\n", rt_last_error());
    rc = 1;
  } else {
    printf("device checksum %016llx\n", (unsigned long long)checksum(&device));
    const int same = !memcmp(&winding, &device, sizeof(winding));
    printf("device equals model: %s\n", same ? "yes" : "NO");
    rc = same ? 0 : 1;
  }
  rt_scene_destroy(scene);
  return rc;
}
