/*
 * c_view_example.c -- camera views from plain C: an anti-aliased frame from a pinhole camera the reference cannot take, its
 * rays made, traced and resolved on the device (rt_view_create, rt_view_set_camera, rt_render_view), then the camera moves and
 * the next frame reuses the ray order of the first.  The frame is checked against the host models of the two formulas:
 * rt_view_resolve_model(rt_trace_rays(rt_view_rays_model)) gives the same bits.  Without a GPU it says so and exits 0.
 *
 *   gcc -I include examples/c_view_example.c -L hslu_i/ba_raytracing/f2501_raytracer_amd -lrt_hip \
 *       -Wl,-rpath,$PWD/hslu_i/ba_raytracing/f2501_raytracer_amd -lm -o /tmp/c_view_example
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rt_hip.h"

#define W 160
#define H 120
#define N (W * H)
#define SAMPLES 9

int main(void) {
  /* one sphere in front of one big matte triangle, one light */
  const float sphere_center[3] = {0.5f, 0.4f, 0.5f};
  const float r = 0.2f;
  const float sphere_r_sq[1] = {r * r}, sphere_r_inv[1] = {1.0f / r};
  const uint32_t sphere_material[1] = {0};
  const float tri_v1[3] = {-1.0f, -1.0f, 0.9f}, tri_e1[3] = {3.0f, 0.0f, 0.0f}, tri_e2[3] = {0.0f, 3.0f, 0.0f};
  const float tri_normal[3] = {0.0f, 0.0f, -1.0f};
  const uint32_t tri_material[1] = {1};
  const float materials[2 * RT_MATERIAL_STRIDE] = {1.0f, 0.2f, 0.2f, 0.6f, 0.3f, 1.0f, 0.0f, 0.0f, 0.0f,
                                                   0.5f, 0.75f, 0.75f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f};
  const float lights[RT_LIGHT_STRIDE] = {0.3f, 0.1f, 0.0f, 1.0f, 1.0f, 1.0f, 0.8f};
  rt_scene_desc d;
  memset(&d, 0, sizeof(d));
  d.abi_version = RT_ABI_VERSION;
  d.n_spheres = 1, d.sphere_center = sphere_center, d.sphere_r_sq = sphere_r_sq, d.sphere_r_inv = sphere_r_inv, d.sphere_material = sphere_material;
  d.n_triangles = 1, d.tri_v1 = tri_v1, d.tri_e1 = tri_e1, d.tri_e2 = tri_e2, d.tri_normal = tri_normal, d.tri_material = tri_material;
  d.n_materials = 2, d.materials = materials;
  d.n_lights = 1, d.lights = lights;

  /* a 3 x 3 grid of sample offsets in pixels; the last one repeats the centre, so 8 of the 9 samples become rays */
  float samples[SAMPLES][2];
  for (int k = 0; k < SAMPLES; k++) samples[k][0] = (float)(k % 3 - 1) / 3.0f, samples[k][1] = (float)(k / 3 - 1) / 3.0f;
  samples[8][0] = samples[4][0], samples[8][1] = samples[4][1];
  const rt_view_desc vd = {RT_ABI_VERSION, W, H, SAMPLES, &samples[0][0], RT_VIEW_ORDER_ONCE};
  /* looking down +z with the image's y axis pointing down, as in the reference's scenes: up = (0, -1, 0) */
  rt_view_camera cam;
  memset(&cam, 0, sizeof(cam));
  cam.abi_version = RT_ABI_VERSION, cam.kind = RT_VIEW_PINHOLE;
  cam.eye[0] = 0.5f, cam.eye[1] = 0.4f, cam.eye[2] = -1.2f;
  cam.right[0] = 1.0f, cam.up[1] = -1.0f, cam.forward[2] = 1.0f;
  cam.tan_half_fov_y = 0.45f;

  /* the host model needs no device: the rays a view of this description makes */
  uint8_t plane_of[SAMPLES];
  uint32_t n_distinct = 0;
  if (rt_view_rays_model(&vd, &cam, NULL, NULL, plane_of, &n_distinct) != RT_OK) {
    fprintf(stderr, "rt_view_rays_model: %s\n", rt_last_error());
    return 1;
  }
  const size_t n_rays = (size_t)n_distinct * N;
  printf("view: %d x %d pixels, %d samples, %u distinct -> %zu rays\n", W, H, SAMPLES, n_distinct, n_rays);
  if (rt_device_count() <= 0) {
    printf("no HIP device: nothing to render\n");
    return 0;
  }

  const float sh = (float)H / (float)W, sd = (1.0f + sh) / 2.0f;
  rt_params p; /* shading only: the camera members of rt_params are not read */
  memset(&p, 0, sizeof(p));
  p.abi_version = RT_ABI_VERSION;
  p.fw = 1.0f / W, p.fh = sh / H, p.fd = sd / ((W + H) / 2.0f);
  p.eps_distance = 1.1920929e-7f * 100.0f * (1.0f + sh + sd) / 3.0f;
  p.air_ior = 1.000293f, p.ambient = 0.08f, p.light_mult = 1;

  int rc = 1;
  rt_scene* scene = NULL;
  rt_view* view = NULL;
  float *rgb = (float*)malloc(sizeof(float) * 3 * N), *want_rgb = (float*)malloc(sizeof(float) * 3 * N);
  uint32_t *argb = (uint32_t*)malloc(sizeof(uint32_t) * N), *want_argb = (uint32_t*)malloc(sizeof(uint32_t) * N);
  float *origin = (float*)malloc(sizeof(float) * 3 * n_rays), *dir = (float*)malloc(sizeof(float) * 3 * n_rays);
  float *ray_rgb = (float*)malloc(sizeof(float) * 3 * n_rays), *ray_t = (float*)malloc(sizeof(float) * n_rays);
  uint8_t* ray_valid = (uint8_t*)malloc(n_rays);
  int32_t* ray_id = (int32_t*)malloc(sizeof(int32_t) * n_rays);
  for (int i = 0; i < N; i++) argb[i] = want_argb[i] = 0xFF101010u; /* pixels no sample hits keep this */
  const rt_ray_radiance pixels = {rgb, NULL, NULL, NULL, argb}, want = {want_rgb, NULL, NULL, NULL, want_argb};
  const rt_ray_radiance rays = {ray_rgb, ray_valid, ray_id, ray_t, NULL};
  rt_ray_batch b;
  memset(&b, 0, sizeof(b));
  b.abi_version = RT_ABI_VERSION, b.n_rays = (uint32_t)n_rays, b.origin = origin, b.direction = dir;
  rt_stats st[2];
  rt_view_info info[2];
  if (rt_scene_create(&d, 0, &scene) != RT_OK || rt_view_create(&vd, 0, &view) != RT_OK || rt_view_set_camera(view, &cam) != RT_OK) {
    fprintf(stderr, "create: %s\n", rt_last_error());
  } else if (rt_render_view(scene, view, &p, &pixels, &st[0]) != RT_OK || rt_view_read(view, NULL, &info[0]) != RT_OK) {
    fprintf(stderr, "rt_render_view: %s\n", rt_last_error());
  } else if (rt_view_rays_model(&vd, &cam, origin, dir, NULL, NULL) != RT_OK || rt_trace_rays(scene, &p, &b, &rays, NULL) != RT_OK ||
             rt_view_resolve_model(N, SAMPLES, plane_of, &rays, &want) != RT_OK) {
    fprintf(stderr, "model: %s\n", rt_last_error());
  } else {
    const int same = memcmp(rgb, want_rgb, sizeof(float) * 3 * N) == 0 && memcmp(argb, want_argb, sizeof(uint32_t) * N) == 0;
    printf("frame 1: %llu rays, %llu valid; generator %.3f ms, order %.3f ms, resolve %.3f ms, all %.3f ms; view holds %llu bytes\n",
           (unsigned long long)st[0].rays_primary, (unsigned long long)st[0].pixels_written, info[0].rays_ms, info[0].order_ms, info[0].resolve_ms,
           st[0].kernel_ms, (unsigned long long)info[0].bytes);
    printf("%s\n", same ? "the frame equals the host models' frame" : "THE FRAME DIFFERS FROM THE HOST MODELS'");
    /* the camera moves; the pixel-to-ray pattern stays, and with it the order */
    cam.eye[0] = 0.8f, cam.eye[1] = 0.3f;
    if (rt_view_set_camera(view, &cam) != RT_OK || rt_render_view(scene, view, &p, &pixels, &st[1]) != RT_OK || rt_view_read(view, NULL, &info[1]) != RT_OK) {
      fprintf(stderr, "frame 2: %s\n", rt_last_error());
    } else {
      printf("frame 2 (moved camera): %llu valid; order %.3f ms (reused), all %.3f ms\n", (unsigned long long)st[1].pixels_written, info[1].order_ms,
             st[1].kernel_ms);
      rc = same && info[1].order_ms == 0.0 ? 0 : 1;
    }
  }
  rt_view_destroy(view);
  rt_scene_destroy(scene);
  free(rgb), free(want_rgb), free(argb), free(want_argb), free(origin), free(dir), free(ray_rgb), free(ray_t), free(ray_valid), free(ray_id);
  return rc;
}
