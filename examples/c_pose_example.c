/*
 * c_pose_example.c -- part poses from plain C: a scene of an octahedron, a sphere and a wall; one rt_pose holds the rest
 * pose of the octahedron and the sphere as ONE part, and three rt_pose_apply calls place it with 32 bytes of transform each
 * -- the posed arrays are made on the device and handed to the BVH refit, nothing is computed on the host.  After every
 * step one rt_render and the SAH report of the refitted tree.  The third step applies the first transform again: its
 * checksum must be the first step's, or the program exits non-zero.  Without a GPU it says so and exits 0.
 *
 *   gcc -I include examples/c_pose_example.c -L hslu_i/ba_raytracing/f2501_raytracer_amd -lrt_hip \
 *       -Wl,-rpath,$PWD/hslu_i/ba_raytracing/f2501_raytracer_amd -lm -o /tmp/c_pose_example
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

/* a turn by `angle` about the vertical axis through `centre`, a scale about it, as an rt_transform: the rotor of the xz
 * plane is {cos(angle / 2), 0, -sin(angle / 2), 0}, and T(v) = rotate(v) scale + translation keeps `centre` in place when
 * translation = centre - rotate(centre) scale */
static rt_transform turn_about(const float centre[3], float angle, float scale) {
  rt_transform t;
  const float c = cosf(angle), s = sinf(angle);
  t.rotor[0] = cosf(0.5f * angle), t.rotor[1] = 0.0f, t.rotor[2] = -sinf(0.5f * angle), t.rotor[3] = 0.0f;
  t.scale = scale;
  /* rotate(centre) for this rotor: x' = c x - s z, z' = s x + c z */
  t.translation[0] = centre[0] - scale * (c * centre[0] - s * centre[2]);
  t.translation[1] = centre[1] - scale * centre[1];
  t.translation[2] = centre[2] - scale * (s * centre[0] + c * centre[2]);
  return t;
}

int main(void) {
  const float sh = (float)H / W, sd = (1.0f + sh) / 2.0f;
  const float centre[3] = {0.5f, sh / 2.0f, 0.45f};
  /* the rest pose: VERTICES v1, v2, v3 (the scene description takes v1 and the edges v2 - v1, v3 - v1) */
  float v1[3 * N_TRI], v2[3 * N_TRI], v3[3 * N_TRI], e1[3 * N_TRI], e2[3 * N_TRI], normal[3 * N_TRI];
  uint32_t tri_material[N_TRI];
  for (int f = 0; f < 8; f++) {
    float n[3], len;
    for (int k = 0; k < 3; k++) {
      v1[3 * f + k] = centre[k] + corner[face[f][0]][k];
      v2[3 * f + k] = centre[k] + corner[face[f][1]][k];
      v3[3 * f + k] = centre[k] + corner[face[f][2]][k];
      e1[3 * f + k] = v2[3 * f + k] - v1[3 * f + k], e2[3 * f + k] = v3[3 * f + k] - v1[3 * f + k];
    }
    n[0] = e1[3 * f + 1] * e2[3 * f + 2] - e1[3 * f + 2] * e2[3 * f + 1];
    n[1] = e1[3 * f + 2] * e2[3 * f + 0] - e1[3 * f + 0] * e2[3 * f + 2];
    n[2] = e1[3 * f + 0] * e2[3 * f + 1] - e1[3 * f + 1] * e2[3 * f + 0];
    len = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    for (int k = 0; k < 3; k++) normal[3 * f + k] = n[k] / len;
  }
  /* the wall: triangle 8, of no part */
  const float wall[12] = {-1.0f, -1.0f, 0.9f, 3.0f, 0.0f, 0.0f, 0.0f, 3.0f, 0.0f, 0.0f, 0.0f, -1.0f};
  memcpy(v1 + 24, wall, 12), memcpy(e1 + 24, wall + 3, 12), memcpy(e2 + 24, wall + 6, 12), memcpy(normal + 24, wall + 9, 12);
  for (int k = 0; k < 3; k++) v2[24 + k] = v1[24 + k] + e1[24 + k], v3[24 + k] = v1[24 + k] + e2[24 + k];
  for (int f = 0; f < N_TRI; f++) tri_material[f] = f < 8 ? 0u : 1u;
  /* a sphere beside the octahedron, part of the same rigid body */
  const float radius = 0.06f;
  const float sphere_center[3] = {centre[0] + 0.27f, centre[1], centre[2]};
  const float sphere_r_sq = radius * radius, sphere_r_inv = 1.0f / radius;
  const uint32_t sphere_material = 0u;
  const float materials[2 * RT_MATERIAL_STRIDE] = {
      0.9f, 0.6f, 0.2f, 0.1f, 0.4f, 1.0f, 0.0f, 0.0f, 0.0f, /* the body */
      0.5f, 0.75f, 0.75f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f /* the wall */
  };
  const float lights[RT_LIGHT_STRIDE] = {0.8f, 0.1f, 0.0f, 1.0f, 1.0f, 1.0f, 0.9f};

  rt_scene_desc d;
  memset(&d, 0, sizeof(d));
  d.abi_version = RT_ABI_VERSION;
  d.n_spheres = 1;
  d.sphere_center = sphere_center, d.sphere_r_sq = &sphere_r_sq, d.sphere_r_inv = &sphere_r_inv, d.sphere_material = &sphere_material;
  d.n_triangles = N_TRI;
  d.tri_v1 = v1, d.tri_e1 = e1, d.tri_e2 = e2, d.tri_normal = normal, d.tri_material = tri_material;
  d.n_materials = 2;
  d.materials = materials;
  d.n_lights = 1;
  d.lights = lights;

  /* one part: triangles 0..7 and sphere 0 */
  const rt_pose_part part = {0, 8, 0, 1};
  rt_pose_desc pd;
  memset(&pd, 0, sizeof(pd));
  pd.abi_version = RT_ABI_VERSION;
  pd.n_parts = 1, pd.parts = &part;
  pd.n_triangles = N_TRI, pd.n_spheres = 1;
  pd.tri_v1 = v1, pd.tri_v2 = v2, pd.tri_v3 = v3, pd.tri_normal = normal;
  pd.sphere_center = sphere_center, pd.sphere_radius = &radius;

  if (rt_device_count() <= 0) {
    printf("no HIP device: ABI links, nothing rendered\n");
    return 0;
  }
  rt_scene* scene = NULL;
  rt_pose* pose = NULL;
  if (rt_scene_create(&d, 0, &scene) != RT_OK || rt_pose_create(&pd, 0, &pose) != RT_OK) {
    fprintf(stderr, "create: %s\n", rt_last_error());
    rt_scene_destroy(scene);
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

  /* step 1: a turn; step 2: further, and smaller; step 3: the transform of step 1 again */
  const rt_transform steps[3] = {turn_about(centre, 0.6f, 1.0f), turn_about(centre, 1.7f, 0.8f), turn_about(centre, 0.6f, 1.0f)};
  uint32_t* argb = (uint32_t*)calloc(W * H, 4);
  uint32_t sums[3] = {0, 0, 0};
  int rc = 0;
  for (int step = 0; step < 3 && !rc; step++) {
    rt_update_info info;
    if (rt_pose_apply(scene, pose, &steps[step], &info) != RT_OK) {
      fprintf(stderr, "rt_pose_apply: %s\n", rt_last_error());
      rc = 1;
      break;
    }
    rt_bvh_quality q;
    if (rt_scene_bvh_quality(scene, &q) != RT_OK) {
      fprintf(stderr, "rt_scene_bvh_quality: %s\n", rt_last_error());
      rc = 1;
      break;
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
    sums[step] = sum;
    printf("step %d: %u nodes refitted in %.3f ms, sah %.4f (created %.4f), checksum %08x, %llu pixels written\n", step + 1, info.nodes_refitted,
           info.total_ms, q.sah_now, q.sah_created, sum, (unsigned long long)st.pixels_written);
  }
  if (!rc) {
    if (sums[2] == sums[0] && sums[1] != sums[0]) {
      printf("step 3 restores the checksum of step 1\n");
    } else {
      fprintf(stderr, "step 3 gives %08x, step 1 gave %08x, step 2 %08x\n", sums[2], sums[0], sums[1]);
      rc = 1;
    }
  }
  free(argb);
  rt_pose_destroy(pose);
  rt_scene_destroy(scene);
  return rc;
}
