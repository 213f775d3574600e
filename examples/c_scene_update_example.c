/*
 * c_scene_update_example.c -- an animation from plain C: one scene handle, eight frames.  A light orbits the scene and a
 * small mesh (an octahedron) turns about its axis; every step is one rt_scene_update -- the BVH is refitted on the device,
 * nothing is rebuilt -- followed by one rt_render.  Prints a checksum per frame.  Without a GPU it says so and exits 0.
 *
 *   gcc -I include examples/c_scene_update_example.c -L hslu_i/ba_raytracing/f2501_raytracer_amd -lrt_hip \
 *       -Wl,-rpath,$PWD/hslu_i/ba_raytracing/f2501_raytracer_amd -lm -o /tmp/c_scene_update_example
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rt_hip.h"

#define W 96
#define H 80
#define N_TRI 9 /* 8 faces of the octahedron + the wall behind it */

static const float corner[6][3] = {{0.18f, 0, 0}, {-0.18f, 0, 0}, {0, 0.25f, 0}, {0, -0.25f, 0}, {0, 0, 0.18f}, {0, 0, -0.18f}};
static const int face[8][3] = {{0, 2, 4}, {2, 1, 4}, {1, 3, 4}, {3, 0, 4}, {2, 0, 5}, {1, 2, 5}, {3, 1, 5}, {0, 3, 5}};

/* the octahedron turned by `angle` about the vertical axis through `centre`: triangles 0..7 as v1, e1, e2, normal */
static void octahedron(float angle, const float centre[3], float* v1, float* e1, float* e2, float* normal) {
  const float c = cosf(angle), s = sinf(angle);
  float p[6][3];
  for (int k = 0; k < 6; k++) {
    p[k][0] = centre[0] + c * corner[k][0] + s * corner[k][2];
    p[k][1] = centre[1] + corner[k][1];
    p[k][2] = centre[2] - s * corner[k][0] + c * corner[k][2];
  }
  for (int f = 0; f < 8; f++) {
    const float *a = p[face[f][0]], *b = p[face[f][1]], *q = p[face[f][2]];
    float n[3], len;
    for (int k = 0; k < 3; k++) v1[3 * f + k] = a[k], e1[3 * f + k] = b[k] - a[k], e2[3 * f + k] = q[k] - a[k];
    n[0] = e1[3 * f + 1] * e2[3 * f + 2] - e1[3 * f + 2] * e2[3 * f + 1];
    n[1] = e1[3 * f + 2] * e2[3 * f + 0] - e1[3 * f + 0] * e2[3 * f + 2];
    n[2] = e1[3 * f + 0] * e2[3 * f + 1] - e1[3 * f + 1] * e2[3 * f + 0];
    len = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    for (int k = 0; k < 3; k++) normal[3 * f + k] = n[k] / len;
  }
}

int main(void) {
  const float sh = (float)H / W, sd = (1.0f + sh) / 2.0f;
  const float centre[3] = {0.5f, sh / 2.0f, 0.45f};
  float v1[3 * N_TRI], e1[3 * N_TRI], e2[3 * N_TRI], normal[3 * N_TRI];
  uint32_t tri_material[N_TRI];
  octahedron(0.0f, centre, v1, e1, e2, normal);
  /* the wall: triangle 8, never updated */
  const float wall[12] = {-1.0f, -1.0f, 0.9f, 3.0f, 0.0f, 0.0f, 0.0f, 3.0f, 0.0f, 0.0f, 0.0f, -1.0f};
  memcpy(v1 + 24, wall, 12), memcpy(e1 + 24, wall + 3, 12), memcpy(e2 + 24, wall + 6, 12), memcpy(normal + 24, wall + 9, 12);
  for (int f = 0; f < N_TRI; f++) tri_material[f] = f < 8 ? 0u : 1u;
  const float materials[2 * RT_MATERIAL_STRIDE] = {
      0.9f, 0.6f, 0.2f, 0.1f, 0.4f, 1.0f, 0.0f, 0.0f, 0.0f, /* the mesh */
      0.5f, 0.75f, 0.75f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f /* the wall */
  };
  float lights[RT_LIGHT_STRIDE] = {0.8f, 0.1f, 0.0f, 1.0f, 1.0f, 1.0f, 0.9f};

  rt_scene_desc d;
  memset(&d, 0, sizeof(d));
  d.abi_version = RT_ABI_VERSION;
  d.n_triangles = N_TRI;
  d.tri_v1 = v1, d.tri_e1 = e1, d.tri_e2 = e2, d.tri_normal = normal, d.tri_material = tri_material;
  d.n_materials = 2;
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

  uint32_t* argb = (uint32_t*)calloc(W * H, 4);
  int rc = 0;
  for (int frame = 0; frame < 8 && !rc; frame++) {
    if (frame) { /* the light a step further on its orbit, the mesh (triangles 0..7 of 9) a step further in its turn */
      const float a = 6.2831853f * frame / 8.0f;
      lights[0] = 0.5f + 0.3f * cosf(a), lights[2] = 0.3f * sinf(a) - 0.1f;
      octahedron(0.5f * a, centre, v1, e1, e2, normal);
      rt_scene_delta u;
      memset(&u, 0, sizeof(u));
      u.abi_version = RT_ABI_VERSION;
      u.tri_first = 0, u.tri_count = 8;
      u.tri_v1 = v1, u.tri_e1 = e1, u.tri_e2 = e2, u.tri_normal = normal;
      u.lights = lights;
      rt_update_info info;
      if (rt_scene_update(scene, &u, &info) != RT_OK) {
        fprintf(stderr, "rt_scene_update: %s\n", rt_last_error());
        rc = 1;
        break;
      }
      printf("update %d: %u nodes refitted, %u slots rewritten, %.3f ms\n", frame, info.nodes_refitted, info.slots_rewritten, info.total_ms);
    }
    memset(argb, 0, W * H * 4);
    rt_stats st;
    if (rt_render(scene, &p, argb, NULL, &st) != RT_OK) {
      fprintf(stderr, "rt_render: %s\n", rt_last_error());
      rc = 1;
      break;
    }
    uint32_t sum = 2166136261u; /* FNV-1a over the packed pixels */
    for (int i = 0; i < W * H; i++) sum = (sum ^ argb[i]) * 16777619u;
    printf("frame %d: checksum %08x, %llu pixels written\n", frame, sum, (unsigned long long)st.pixels_written);
  }
  free(argb);
  rt_scene_destroy(scene);
  return rc;
}
