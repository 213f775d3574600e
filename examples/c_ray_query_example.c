/*
 * c_ray_query_example.c -- the ray queries from plain C: builds a two-object scene, picks the object under the image
 * centre (rt_cast_rays, the reference's Raytracer::cast_ray) and tests one shadow segment from that point to the light
 * (rt_any_intersection, Raytracer::has_any_intersection).  Without a GPU it says so and exits 0.
 *
 *   gcc -I include examples/c_ray_query_example.c -L hslu_i/ba_raytracing/f2501_raytracer_amd -lrt_hip \
 *       -Wl,-rpath,$PWD/hslu_i/ba_raytracing/f2501_raytracer_amd -lm -o /tmp/c_ray_query_example
 */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "rt_hip.h"

int main(void) {
  /* one diffuse sphere in front of one big triangle, one light */
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

  if (rt_device_count() <= 0) {
    printf("no HIP device: nothing to query\n");
    return 0;
  }
  rt_scene* scene = NULL;
  if (rt_scene_create(&d, 0, &scene) != RT_OK) {
    fprintf(stderr, "rt_scene_create: %s\n", rt_last_error());
    return 1;
  }

  /* the camera ray through the centre of a 96x80 window (origin (x fw, y fh, 0), direction origin - focus) */
  const float sh = 80.0f / 96.0f, sd = (1.0f + sh) / 2.0f;
  const float focus[3] = {0.5f, sh / 2.0f, -1.9f * sd};
  const float origin[3] = {48.0f * (1.0f / 96.0f), 40.0f * (sh / 80.0f), 0.0f};
  const float dir[3] = {origin[0] - focus[0], origin[1] - focus[1], origin[2] - focus[2]};
  rt_ray_batch b;
  memset(&b, 0, sizeof(b));
  b.abi_version = RT_ABI_VERSION;
  b.n_rays = 1;
  b.origin = origin;
  b.direction = dir;
  int32_t id = 0;
  float t = 0.0f, point[3], normal[3];
  uint32_t material = 0;
  rt_ray_hits hits = {&id, &t, point, normal, &material};
  if (rt_cast_rays(scene, &b, &hits) != RT_OK) {
    fprintf(stderr, "rt_cast_rays: %s\n", rt_last_error());
    rt_scene_destroy(scene);
    return 1;
  }
  printf("picked object %d at t = %.6f, point (%.4f, %.4f, %.4f), material %u\n", id, t, point[0], point[1], point[2], material);

  /* the shadow segment from that point to the light, pushed off the surface as the render does */
  int rc = 0;
  if (id >= 0) {
    float ld[3] = {lights[0] - point[0], lights[1] - point[1], lights[2] - point[2]};
    const float len = sqrtf(ld[0] * ld[0] + ld[1] * ld[1] + ld[2] * ld[2]);
    const float eps = 1e-4f;
    float so[3], maxd;
    for (int k = 0; k < 3; k++) so[k] = point[k] + ld[k] / len * eps;
    maxd = len - eps;
    b.origin = so;
    b.direction = ld;
    b.max_distance = &maxd;
    uint8_t has = 0, occ = 0;
    float opacity = 0.0f, filter[3];
    rt_ray_occlusion out = {&has, &occ, &opacity, filter};
    if (rt_any_intersection(scene, &b, &out) != RT_OK) {
      fprintf(stderr, "rt_any_intersection: %s\n", rt_last_error());
      rc = 1;
    } else {
      printf("shadow segment to the light: has_intersection %u, completely_occluded %u, opacity %.4f\n", has, occ, opacity);
    }
  }
  rt_scene_destroy(scene);
  return rc;
}
