/*
 * c_skin_example.c -- a skinned mesh from plain C: a strip of 32 triangles in front of a wall, held by TWO bones whose
 * weights ramp along the strip.  One rt_skin holds the indexed rest mesh on the device; every rt_skin_apply takes 64 bytes
 * (two rt_transform), skins the shared vertices, rebuilds the triangles and their face normals from them and refits the
 * BVH -- nothing is computed on the host.  The scene itself is created from rt_skin_model, the host model of the same
 * formulas.  Frame 1 is the rest pose, frames 2 and 3 bend the strip, frame 4 bends it back: its checksum must be frame
 * 1's, or the program exits non-zero.  Then the SAH report of the tree refitted to a strong bend, a rebuild, and the
 * report again.  Without a GPU it says so and exits 0.
 *
 *   gcc -I include examples/c_skin_example.c -L hslu_i/ba_raytracing/f2501_raytracer_amd -lrt_hip \
 *       -Wl,-rpath,$PWD/hslu_i/ba_raytracing/f2501_raytracer_amd -lm -o /tmp/c_skin_example
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rt_hip.h"

#define W 96
#define H 80
#define N_QUADS 16
#define N_VERT (2 * (N_QUADS + 1))
#define N_MESH (2 * N_QUADS)
#define N_TRI (N_MESH + 1) /* the strip + the wall behind it */

static const rt_transform identity = {{0.0f, 0.0f, 0.0f}, {1.0f, 0.0f, 0.0f, 0.0f}, 1.0f};

/* a turn by `angle` about the vertical axis through `centre`, as an rt_transform: the rotor of the xz plane is
 * {cos(angle / 2), 0, -sin(angle / 2), 0}, and T(v) = rotate(v) + translation keeps `centre` in place when
 * translation = centre - rotate(centre) */
static rt_transform turn_about(const float centre[3], float angle) {
  rt_transform t = identity;
  const float c = cosf(angle), s = sinf(angle);
  t.rotor[0] = cosf(0.5f * angle), t.rotor[2] = -sinf(0.5f * angle);
  /* rotate(centre) for this rotor: x' = c x - s z, z' = s x + c z */
  t.translation[0] = centre[0] - (c * centre[0] - s * centre[2]);
  t.translation[2] = centre[2] - (s * centre[0] + c * centre[2]);
  return t;
}

int main(void) {
  const float sh = (float)H / W, sd = (1.0f + sh) / 2.0f;
  const float centre[3] = {0.5f, sh / 2.0f, 0.45f};
  const float x0 = 0.2f, length = 0.6f, y0 = centre[1] - 0.1f, y1 = centre[1] + 0.1f;
  /* the indexed rest mesh: vertex 2 k at (x_k, y0), vertex 2 k + 1 at (x_k, y1); bone 0 holds the left end, bone 1 the
   * right end, the weights ramp linearly in between; no vertex normals: the skin makes face normals from the skinned edges */
  float position[3 * N_VERT], weight[4 * N_VERT];
  uint16_t bone[4 * N_VERT];
  uint32_t indices[3 * N_MESH];
  for (int k = 0; k <= N_QUADS; k++) {
    const float u = (float)k / N_QUADS;
    for (int j = 0; j < 2; j++) {
      const int v = 2 * k + j;
      position[3 * v] = x0 + u * length, position[3 * v + 1] = j ? y1 : y0, position[3 * v + 2] = centre[2];
      bone[4 * v] = 0, bone[4 * v + 1] = 1, bone[4 * v + 2] = 0, bone[4 * v + 3] = 0;
      weight[4 * v] = 1.0f - u, weight[4 * v + 1] = u, weight[4 * v + 2] = 0.0f, weight[4 * v + 3] = 0.0f;
    }
  }
  for (int k = 0; k < N_QUADS; k++) { /* both triangles face the camera (normal towards -z) */
    const uint32_t a = 2 * k, b = 2 * k + 1, c = 2 * k + 2, e = 2 * k + 3;
    const uint32_t two[6] = {a, b, c, c, b, e};
    memcpy(indices + 6 * k, two, sizeof(two));
  }
  rt_skin_desc sk;
  memset(&sk, 0, sizeof(sk));
  sk.abi_version = RT_ABI_VERSION;
  sk.n_vertices = N_VERT, sk.n_bones = 2;
  sk.tri_first = 0, sk.tri_count = N_MESH, sk.n_triangles = N_TRI;
  sk.position = position, sk.normal = NULL, sk.indices = indices, sk.bone = bone, sk.weight = weight;

  /* the scene: the strip as the host model gives it at rest, and the wall (triangle N_MESH, not part of the skin) */
  float v1[3 * N_TRI], e1[3 * N_TRI], e2[3 * N_TRI], normal[3 * N_TRI];
  uint32_t tri_material[N_TRI];
  const rt_transform rest[2] = {identity, identity};
  if (rt_skin_model(&sk, rest, NULL, NULL, v1, e1, e2, normal) != RT_OK) {
    fprintf(stderr, "rt_skin_model: %s\n", rt_last_error());
    return 1;
  }
  const float wall[12] = {-1.0f, -1.0f, 0.9f, 3.0f, 0.0f, 0.0f, 0.0f, 3.0f, 0.0f, 0.0f, 0.0f, -1.0f};
  memcpy(v1 + 3 * N_MESH, wall, 12), memcpy(e1 + 3 * N_MESH, wall + 3, 12), memcpy(e2 + 3 * N_MESH, wall + 6, 12);
  memcpy(normal + 3 * N_MESH, wall + 9, 12);
  for (int f = 0; f < N_TRI; f++) tri_material[f] = f < N_MESH ? 0u : 1u;
  const float materials[2 * RT_MATERIAL_STRIDE] = {
      0.9f, 0.6f, 0.2f, 0.1f, 0.4f, 1.0f, 0.0f, 0.0f, 0.0f, /* the strip */
      0.5f, 0.75f, 0.75f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f /* the wall */
  };
  const float lights[RT_LIGHT_STRIDE] = {0.8f, 0.1f, 0.0f, 1.0f, 1.0f, 1.0f, 0.9f};
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
    printf("no HIP device: ABI links, the host model ran, nothing rendered\n");
    return 0;
  }
  rt_scene* scene = NULL;
  rt_skin* skin = NULL;
  if (rt_scene_create(&d, 0, &scene) != RT_OK || rt_skin_create(&sk, 0, &skin) != RT_OK) {
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

  /* bone 0 stays; bone 1 turns about the vertical axis through the strip's centre: rest, a bend, a stronger bend, rest */
  const float angle[4] = {0.0f, 0.5f, 1.1f, 0.0f};
  uint32_t* argb = (uint32_t*)calloc(W * H, 4);
  uint32_t sums[4] = {0, 0, 0, 0};
  int rc = 0;
  for (int step = 0; step < 4 && !rc; step++) {
    const rt_transform bones[2] = {identity, angle[step] != 0.0f ? turn_about(centre, angle[step]) : identity};
    rt_update_info info;
    if (rt_skin_apply(scene, skin, bones, &info) != RT_OK) {
      fprintf(stderr, "rt_skin_apply: %s\n", rt_last_error());
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
    printf("frame %d: bone 1 turned by %.1f rad, %u slots rewritten in %.3f ms, checksum %08x, %llu pixels written\n", step + 1, angle[step],
           info.slots_rewritten, info.total_ms, sum, (unsigned long long)st.pixels_written);
  }
  if (!rc) {
    if (sums[3] == sums[0] && sums[1] != sums[0] && sums[2] != sums[0]) {
      printf("frame 4 restores the checksum of the rest frame\n");
    } else {
      fprintf(stderr, "frame 4 gives %08x, the rest frame gave %08x, the bends %08x and %08x\n", sums[3], sums[0], sums[1], sums[2]);
      rc = 1;
    }
  }
  if (!rc) { /* how far has the refitted tree decayed under a strong bend, and what does a rebuild make of it? */
    const rt_transform bones[2] = {identity, turn_about(centre, 2.4f)};
    rt_bvh_quality before, after;
    rt_rebuild_info rb;
    if (rt_skin_apply(scene, skin, bones, NULL) != RT_OK || rt_scene_bvh_quality(scene, &before) != RT_OK || rt_scene_rebuild(scene, &rb) != RT_OK ||
        rt_scene_bvh_quality(scene, &after) != RT_OK) {
      fprintf(stderr, "bend / report / rebuild: %s\n", rt_last_error());
      rc = 1;
    } else {
      printf("bent by 2.4 rad: sah %.4f refitted (created %.4f); rebuilt in %.3f ms to %u nodes: sah %.4f\n", before.sah_now, before.sah_created,
             rb.total_ms, rb.n_nodes, after.sah_now);
    }
  }
  free(argb);
  rt_skin_destroy(skin);
  rt_scene_destroy(scene);
  return rc;
}
