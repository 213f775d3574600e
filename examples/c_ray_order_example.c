/*
 * c_ray_order_example.c -- ray orders from plain C: a camera batch in row-major order is traced as given and through an
 * order built on the device (rt_ray_order_build, rt_trace_rays_ordered).  The order only changes which 64 rays share a
 * wavefront, so both calls return the same bits: the checksums printed are equal.  Without a GPU it says so and exits 0.
 *
 *   gcc -I include examples/c_ray_order_example.c -L hslu_i/ba_raytracing/f2501_raytracer_amd -lrt_hip \
 *       -Wl,-rpath,$PWD/hslu_i/ba_raytracing/f2501_raytracer_amd -lm -o /tmp/c_ray_order_example
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rt_hip.h"

#define W 320
#define H 240
#define N (W * H)

static uint64_t checksum(const void* p, size_t bytes) { /* FNV-1a */
  const unsigned char* c = (const unsigned char*)p;
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < bytes; i++) h = (h ^ c[i]) * 1099511628211ull;
  return h;
}

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

  if (rt_device_count() <= 0) {
    printf("no HIP device: nothing to order\n");
    return 0;
  }
  rt_scene* scene = NULL;
  if (rt_scene_create(&d, 0, &scene) != RT_OK) {
    fprintf(stderr, "rt_scene_create: %s\n", rt_last_error());
    return 1;
  }
  const float sh = (float)H / (float)W, sd = (1.0f + sh) / 2.0f;
  rt_params p;
  memset(&p, 0, sizeof(p));
  p.abi_version = RT_ABI_VERSION;
  p.fw = 1.0f / W, p.fh = sh / H, p.fd = sd / ((W + H) / 2.0f);
  p.eps_distance = 1.1920929e-7f * 100.0f * (1.0f + sh + sd) / 3.0f;
  p.air_ior = 1.000293f, p.ambient = 0.08f, p.light_mult = 1;

  /* a pinhole camera's rays, row-major: 64 consecutive rays are a strip of one row */
  const float eye[3] = {0.5f, 0.4f, -1.2f};
  float* origin = (float*)malloc(sizeof(float) * 3 * N);
  float* dir = (float*)malloc(sizeof(float) * 3 * N);
  float* rgb[2] = {(float*)malloc(sizeof(float) * 3 * N), (float*)malloc(sizeof(float) * 3 * N)};
  int32_t* id[2] = {(int32_t*)malloc(sizeof(int32_t) * N), (int32_t*)malloc(sizeof(int32_t) * N)};
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++) {
      const int i = y * W + x;
      for (int k = 0; k < 3; k++) origin[3 * i + k] = eye[k];
      dir[3 * i] = ((x + 0.5f) / W - 0.5f) * 1.2f, dir[3 * i + 1] = ((y + 0.5f) / H - 0.5f) * 1.2f * sh, dir[3 * i + 2] = 1.0f;
    }
  rt_ray_batch b;
  memset(&b, 0, sizeof(b));
  b.abi_version = RT_ABI_VERSION, b.n_rays = N, b.origin = origin, b.direction = dir;

  int rc = 1;
  rt_ray_order* order = NULL;
  const rt_ray_order_desc od = {RT_ABI_VERSION, N, 0, 0};
  rt_ray_order_info info;
  rt_stats st[2];
  rt_ray_radiance out0 = {rgb[0], NULL, id[0], NULL, NULL}, out1 = {rgb[1], NULL, id[1], NULL, NULL};
  if (rt_ray_order_create(&od, 0, &order) != RT_OK || rt_ray_order_build(order, &b) != RT_OK ||
      rt_ray_order_read(order, NULL, NULL, &info) != RT_OK) {
    fprintf(stderr, "rt_ray_order: %s\n", rt_last_error());
  } else if (rt_trace_rays(scene, &p, &b, &out0, &st[0]) != RT_OK || rt_trace_rays_ordered(scene, &p, &b, order, &out1, &st[1]) != RT_OK) {
    fprintf(stderr, "rt_trace_rays: %s\n", rt_last_error());
  } else {
    const uint64_t c0 = checksum(rgb[0], sizeof(float) * 3 * N) ^ checksum(id[0], sizeof(int32_t) * N);
    const uint64_t c1 = checksum(rgb[1], sizeof(float) * 3 * N) ^ checksum(id[1], sizeof(int32_t) * N);
    printf("order: %u rays (%u live), %u origin axes x %u bits, %u direction axes x %u bits, %llu bytes, built in %.3f ms\n", info.n_rays,
           info.n_live, info.n_origin_axes, info.origin_bits, info.n_direction_axes, info.direction_bits, (unsigned long long)info.bytes,
           info.device_ms);
    printf("as given: %.3f ms, checksum %016llx\n", st[0].kernel_ms, (unsigned long long)c0);
    printf("ordered:  %.3f ms, checksum %016llx\n", st[1].kernel_ms, (unsigned long long)c1);
    printf("%s\n", c0 == c1 && st[0].rays_shadow == st[1].rays_shadow ? "same results" : "RESULTS DIFFER");
    rc = c0 == c1 ? 0 : 1;
  }
  rt_ray_order_destroy(order);
  rt_scene_destroy(scene);
  free(origin), free(dir), free(rgb[0]), free(rgb[1]), free(id[0]), free(id[1]);
  return rc;
}
