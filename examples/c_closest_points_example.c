/*
 * c_closest_points_example.c -- the closest-point query from plain C: builds a two-object scene (a sphere in front of a big
 * triangle), asks rt_closest_points for the nearest surface point of a small grid of probes, compares every plane with
 * rt_closest_points_model (the specification: a linear scan on the host, the same bits) and prints a checksum.  Without a
 * GPU it runs the model alone, says so and exits 0.
 *
 *   gcc -I include examples/c_closest_points_example.c -L hslu_i/ba_raytracing/f2501_raytracer_amd -lrt_hip \
 *       -Wl,-rpath,$PWD/hslu_i/ba_raytracing/f2501_raytracer_amd -lm -o /tmp/c_closest_points_example
 */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "rt_hip.h"

#define G 6
#define N (G * G * G)

int main(void) {
  const float sphere_center[3] = {0.5f, 0.4f, 0.5f};
  const float r = 0.2f;
  const float sphere_r_sq[1] = {r * r}, sphere_r_inv[1] = {1.0f / r};
  const uint32_t sphere_material[1] = {0};
  const float tri_v1[3] = {-1.0f, -1.0f, 0.9f}, tri_e1[3] = {3.0f, 0.0f, 0.0f}, tri_e2[3] = {0.0f, 3.0f, 0.0f};
  const float tri_normal[3] = {0.0f, 0.0f, -1.0f};
  const uint32_t tri_material[1] = {1};
  const float materials[2 * RT_MATERIAL_STRIDE] = {
      1.0f, 0.2f, 0.2f, 0.0f, 0.3f, 1.0f, 0.0f, 0.0f, 0.0f, /* red, shiny */
      0.5f, 0.75f, 0.75f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f /* wall */
  };
  const float lights[RT_LIGHT_STRIDE] = {0.3f, 0.1f, 0.0f, 1.0f, 1.0f, 1.0f, 0.8f};

  rt_scene_desc d;
  memset(&d, 0, sizeof(d));
  d.abi_version = RT_ABI_VERSION;
  d.n_spheres = 1;
  d.sphere_center = sphere_center;
  d.sphere_r_sq = sphere_r_sq;
  d.sphere_r_inv = sphere_r_inv;
  d.sphere_material = sphere_material;
  d.n_triangles = 1;
  d.tri_v1 = tri_v1;
  d.tri_e1 = tri_e1;
  d.tri_e2 = tri_e2;
  d.tri_normal = tri_normal;
  d.tri_material = tri_material;
  d.n_materials = 2;
  d.materials = materials;
  d.n_lights = 1;
  d.lights = lights;

  /* probes: a G x G x G grid over [0, 1]^3, and a search radius of 0.45 for every second one */
  static float point[N][3], radius[N];
  for (int i = 0; i < N; i++) {
    point[i][0] = (float)(i % G) / (G - 1), point[i][1] = (float)(i / G % G) / (G - 1), point[i][2] = (float)(i / (G * G)) / (G - 1);
    radius[i] = (i & 1) ? 0.45f : INFINITY;
  }
  rt_point_batch b;
  memset(&b, 0, sizeof(b));
  b.abi_version = RT_ABI_VERSION;
  b.n_points = N;
  b.point = &point[0][0];
  b.max_distance = radius;

  static int32_t id[2][N];
  static float dist[2][N], q[2][N][3], nrm[2][N][3], bary[2][N][2];
  static uint32_t mat[2][N];
  const rt_point_hits model = {id[0], dist[0], &q[0][0][0], &nrm[0][0][0], &bary[0][0][0], mat[0]};
  const rt_point_hits device = {id[1], dist[1], &q[1][0][0], &nrm[1][0][0], &bary[1][0][0], mat[1]};
  if (rt_closest_points_model(&d, &b, &model) != RT_OK) {
    fprintf(stderr, "rt_closest_points_model: %s\n", rt_last_error());
    return 1;
  }
  int on_sphere = 0, on_triangle = 0, missed = 0;
  double sum = 0.0;
  for (int i = 0; i < N; i++) {
    on_sphere += id[0][i] == 0, on_triangle += id[0][i] == 1, missed += id[0][i] < 0;
    if (id[0][i] >= 0) sum += dist[0][i];
  }
  printf("%d probes: %d nearest to the sphere, %d to the triangle, %d with nothing inside their radius\n", N, on_sphere, on_triangle, missed);
  printf("probe 0 (%.2f, %.2f, %.2f): object %d at distance %.6f, point (%.4f, %.4f, %.4f)\n", point[0][0], point[0][1], point[0][2], id[0][0],
         dist[0][0], q[0][0][0], q[0][0][1], q[0][0][2]);

  if (rt_device_count() <= 0) {
    printf("no HIP device: the model alone, checksum %.6f\n", sum);
    return 0;
  }
  rt_scene* scene = NULL;
  if (rt_scene_create(&d, 0, &scene) != RT_OK) {
    fprintf(stderr, "rt_scene_create: %s\n", rt_last_error());
    return 1;
  }
  int rc = 0;
  if (rt_closest_points(scene, &b, &device) != RT_OK) {
    fprintf(stderr, "rt_closest_points: %s\n", rt_last_error());
    rc = 1;
  } else {
    const int same = !memcmp(id[0], id[1], sizeof(id[0])) && !memcmp(dist[0], dist[1], sizeof(dist[0])) && !memcmp(q[0], q[1], sizeof(q[0])) &&
                     !memcmp(nrm[0], nrm[1], sizeof(nrm[0])) && !memcmp(bary[0], bary[1], sizeof(bary[0])) && !memcmp(mat[0], mat[1], sizeof(mat[0]));
    printf("device equals model: %s, checksum %.6f\n", same ? "yes" : "NO", sum);
    rc = same ? 0 : 1;
  }
  rt_scene_destroy(scene);
  return rc;
}
