/*
 * c_trace_rays_example.c -- radiance queries from plain C: builds a two-object scene and asks for the colour of a small
 * fan of rays from a viewpoint of the caller's choosing (rt_trace_rays, the reference's single_raytrace for arbitrary
 * rays), first with direct light only, then with reflections.  Without a GPU it says so and exits 0.
 *
 *   gcc -I include examples/c_trace_rays_example.c -L hslu_i/ba_raytracing/f2501_raytracer_amd -lrt_hip \
 *       -Wl,-rpath,$PWD/hslu_i/ba_raytracing/f2501_raytracer_amd -lm -o /tmp/c_trace_rays_example
 */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "rt_hip.h"

#define N_RAYS 9

int main(void) {
  /* one mirror-like sphere in front of one big matte triangle, one light */
  const float sphere_center[3] = {0.5f, 0.4f, 0.5f};
  const float r = 0.2f;
  const float sphere_r_sq[1] = {r * r}, sphere_r_inv[1] = {1.0f / r};
  const uint32_t sphere_material[1] = {0};
  const float tri_v1[3] = {-1.0f, -1.0f, 0.9f}, tri_e1[3] = {3.0f, 0.0f, 0.0f}, tri_e2[3] = {0.0f, 3.0f, 0.0f};
  const float tri_normal[3] = {0.0f, 0.0f, -1.0f};
  const uint32_t tri_material[1] = {1};
  const float materials[2 * RT_MATERIAL_STRIDE] = {
      1.0f, 0.2f, 0.2f, 0.6f, 0.3f, 1.0f, 0.0f, 0.0f, 0.0f, /* red, metallic 0.6 */
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
    printf("no HIP device: nothing to trace\n");
    return 0;
  }
  rt_scene* scene = NULL;
  if (rt_scene_create(&d, 0, &scene) != RT_OK) {
    fprintf(stderr, "rt_scene_create: %s\n", rt_last_error());
    return 1;
  }

  /* shading parameters: the scene units of a 96x80 frame; the camera members stay 0 -- the rays below are the camera */
  const float sh = 80.0f / 96.0f, sd = (1.0f + sh) / 2.0f;
  rt_params p;
  memset(&p, 0, sizeof(p));
  p.abi_version = RT_ABI_VERSION;
  p.fw = 1.0f / 96.0f, p.fh = sh / 80.0f, p.fd = sd / 88.0f;
  p.eps_distance = 1.1920929e-7f * 100.0f * (1.0f + sh + sd) / 3.0f;
  p.air_ior = 1.000293f;
  p.ambient = 0.08f;
  p.light_mult = 1;

  /* a fan of rays from a viewpoint to the left of the reference's, towards the sphere */
  const float eye[3] = {-0.6f, 0.4f, -0.8f};
  float origin[N_RAYS][3], dir[N_RAYS][3];
  for (int i = 0; i < N_RAYS; i++) {
    const float a = ((float)i - (N_RAYS - 1) / 2.0f) * 0.06f;
    const float tx = sphere_center[0] + a, ty = sphere_center[1], tz = sphere_center[2];
    for (int k = 0; k < 3; k++) origin[i][k] = eye[k];
    dir[i][0] = tx - eye[0], dir[i][1] = ty - eye[1], dir[i][2] = tz - eye[2];
  }
  rt_ray_batch b;
  memset(&b, 0, sizeof(b));
  b.abi_version = RT_ABI_VERSION;
  b.n_rays = N_RAYS;
  b.origin = &origin[0][0];
  b.direction = &dir[0][0];
  float rgb[N_RAYS][3], t[N_RAYS];
  uint8_t valid[N_RAYS];
  int32_t id[N_RAYS];
  uint32_t argb[N_RAYS];
  rt_ray_radiance out = {&rgb[0][0], valid, id, t, argb};
  int rc = 0;
  for (int pass = 0; pass < 2 && rc == 0; pass++) {
    p.flags = pass ? RT_FLAG_REFLECTIONS : 0u;
    p.max_depth_reflection = pass ? 4u : 0u;
    for (int i = 0; i < N_RAYS; i++) argb[i] = 0xFF000000u; /* a miss keeps this */
    rt_stats st;
    if (rt_trace_rays(scene, &p, &b, &out, &st) != RT_OK) {
      fprintf(stderr, "rt_trace_rays: %s\n", rt_last_error());
      rc = 1;
      break;
    }
    printf("%s: %llu rays, %llu valid, %llu reflection rays, %llu shadow rays\n", pass ? "with reflections" : "direct light",
           (unsigned long long)st.rays_primary, (unsigned long long)st.pixels_written, (unsigned long long)st.rays_reflection,
           (unsigned long long)st.rays_shadow);
    for (int i = 0; i < N_RAYS; i++)
      printf("  ray %d: object %d at t = %.4f, rgb (%.4f, %.4f, %.4f), pixel 0x%08X\n", i, id[i], valid[i] ? t[i] : INFINITY, rgb[i][0],
             rgb[i][1], rgb[i][2], argb[i]);
  }
  rt_scene_destroy(scene);
  return rc;
}
