/*
 * c_view_lens_example.c -- depth of field from plain C: the scene of c_view_example.c through a thin lens
 * (rt_view_create_lens, rt_view_set_lens) focused on the wall behind the sphere, rendered in full (rt_render_view) and
 * adaptively (rt_render_view_adaptive) with the defocus criterion: the sphere is out of focus, so it and the pixels its blur
 * reaches take all their samples although sample 0 shows no edge inside it.  The mask is checked against the host models of
 * the refine rule and of the criterion on the frame of a one-sample lens view (rt_view_refine_model, rt_view_defocus_model),
 * and the frame against the full one: a refined pixel is the full lens frame's pixel, bit for bit.  Without a GPU it runs the
 * host model of the lens rays on one pixel, says so and exits 0.
 *
 *   gcc -I include examples/c_view_lens_example.c -L hslu_i/ba_raytracing/f2501_raytracer_amd -lrt_hip \
 *       -Wl,-rpath,$PWD/hslu_i/ba_raytracing/f2501_raytracer_amd -lm -o /tmp/c_view_lens_example
 */
#include <math.h>
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

  /* a 3 x 3 grid of pixel offsets, the centre first, and a lens offset for each: sample 0 through the lens centre, the others
   * on a circle of radius 0.8 */
  float samples[SAMPLES][2], lens_samples[SAMPLES][2];
  const int grid[SAMPLES] = {4, 0, 1, 2, 3, 5, 6, 7, 8};
  for (int k = 0; k < SAMPLES; k++) {
    samples[k][0] = (float)(grid[k] % 3 - 1) / 3.0f, samples[k][1] = (float)(grid[k] / 3 - 1) / 3.0f;
    lens_samples[k][0] = k ? 0.8f * cosf(0.785398f * (float)k) : 0.0f, lens_samples[k][1] = k ? 0.8f * sinf(0.785398f * (float)k) : 0.0f;
  }
  const rt_view_desc vd = {RT_ABI_VERSION, W, H, SAMPLES, &samples[0][0], RT_VIEW_ORDER_ONCE};
  const rt_view_desc vd1 = {RT_ABI_VERSION, W, H, 1, &samples[0][0], RT_VIEW_ORDER_ONCE};
  rt_view_camera cam;
  memset(&cam, 0, sizeof(cam));
  cam.abi_version = RT_ABI_VERSION, cam.kind = RT_VIEW_PINHOLE;
  cam.eye[0] = 0.5f, cam.eye[1] = 0.4f, cam.eye[2] = -1.2f;
  cam.right[0] = 1.0f, cam.up[1] = -1.0f, cam.forward[2] = 1.0f;
  cam.tan_half_fov_y = 0.45f;
  /* a lens of radius 0.1 focused on the wall, 2.1 in front of the eye; the sphere, 1.5 to 1.7 away, is blurred by 1.5 to 2.5
   * pixels.  Adaptive frames refine what is blurred by more than half a pixel and what that blur reaches, up to 4 pixels away. */
  const rt_view_lens lens = {RT_ABI_VERSION, 4, 0.1f, 2.1f, 0.5f, 0};
  const rt_view_refine refine = {RT_ABI_VERSION, RT_REFINE_DEPTH | RT_REFINE_COLOUR, 0.05f, 0.05f};

  /* the host model of the lens rays needs no device: the 9 rays of the centre pixel of a 1 x 1 frame meet 2.1 in front of the eye */
  {
    const rt_view_desc one_pixel = {RT_ABI_VERSION, 1, 1, SAMPLES, &samples[0][0], RT_VIEW_ORDER_ONCE};
    float o[SAMPLES * 3], dir[SAMPLES * 3];
    uint8_t plane_of[SAMPLES];
    uint32_t nd = 0;
    if (rt_view_lens_rays_model(&one_pixel, &lens_samples[0][0], &cam, &lens, o, dir, plane_of, &nd) != RT_OK) {
      fprintf(stderr, "rt_view_lens_rays_model: %s\n", rt_last_error());
      return 1;
    }
    float zmin = 1e30f, zmax = -1e30f;
    for (uint32_t u = 0; u < nd; u++) {
      const float z = o[3 * u + 2] + dir[3 * u + 2] - cam.eye[2]; /* the point at parameter 1 of every ray */
      zmin = z < zmin ? z : zmin, zmax = z > zmax ? z : zmax;
    }
    printf("lens model: %u planes; every ray passes the focus plane at parameter 1: depth %.4f .. %.4f\n", nd, zmin, zmax);
    if (nd != SAMPLES || fabsf(zmin - 2.1f) > 1e-5f || fabsf(zmax - 2.1f) > 1e-5f) return 1;
  }
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
  rt_view *view = NULL, *view1 = NULL;
  float *full_rgb = (float*)malloc(sizeof(float) * 3 * N), *rgb = (float*)malloc(sizeof(float) * 3 * N), *one_rgb = (float*)malloc(sizeof(float) * 3 * N);
  float *one_t = (float*)malloc(sizeof(float) * N), *coc = (float*)malloc(sizeof(float) * N);
  int32_t* one_id = (int32_t*)malloc(sizeof(int32_t) * N);
  uint8_t *one_valid = (uint8_t*)malloc(N), *mask = (uint8_t*)malloc(N), *want_mask = (uint8_t*)malloc(N);
  const rt_ray_radiance full = {full_rgb, NULL, NULL, NULL, NULL}, pixels = {rgb, NULL, NULL, NULL, NULL};
  const rt_ray_radiance one = {one_rgb, one_valid, one_id, one_t, NULL};
  rt_stats st_full, st;
  rt_view_adaptive_info info;
  rt_view_info vinfo;
  uint32_t n_edges = 0, n_defocus = 0;
  if (rt_scene_create(&d, 0, &scene) != RT_OK || rt_view_create_lens(&vd, &lens_samples[0][0], 0, &view) != RT_OK ||
      rt_view_set_camera(view, &cam) != RT_OK || rt_view_set_lens(view, &lens) != RT_OK ||
      rt_view_create_lens(&vd1, &lens_samples[0][0], 0, &view1) != RT_OK || rt_view_set_camera(view1, &cam) != RT_OK ||
      rt_view_set_lens(view1, &lens) != RT_OK || rt_view_enable_adaptive(view) != RT_OK) {
    fprintf(stderr, "create: %s\n", rt_last_error());
  } else if (rt_render_view(scene, view, &p, &full, &st_full) != RT_OK || rt_render_view(scene, view1, &p, &one, NULL) != RT_OK) {
    fprintf(stderr, "rt_render_view: %s\n", rt_last_error());
  } else if (rt_render_view_adaptive(scene, view, &p, &refine, &pixels, mask, &st) != RT_OK || rt_view_adaptive_read(view, &info) != RT_OK ||
             rt_view_read(view, NULL, &vinfo) != RT_OK) {
    fprintf(stderr, "rt_render_view_adaptive: %s\n", rt_last_error());
  } else if (rt_view_refine_model(W, H, &refine, &one, want_mask, &n_edges) != RT_OK ||
             rt_view_defocus_model(&vd1, &cam, &lens, one_valid, one_t, coc, want_mask, &n_defocus) != RT_OK) {
    fprintf(stderr, "host models: %s\n", rt_last_error());
  } else {
    int refined_same = 1, flat_differ = 0;
    float coc_max = 0.0f;
    for (int i = 0; i < N; i++) {
      const int same = memcmp(rgb + 3 * i, full_rgb + 3 * i, 12) == 0;
      if (mask[i] && !same) refined_same = 0;
      if (!mask[i] && !same) flat_differ++;
      coc_max = coc[i] > coc_max ? coc[i] : coc_max;
    }
    const int mask_same = memcmp(mask, want_mask, N) == 0 && info.n_refined == n_edges + n_defocus;
    printf("full lens frame: %llu rays, %.3f ms; adaptive lens frame: %llu rays, %.3f ms (classify with coc and spread %.3f ms)\n",
           (unsigned long long)st_full.rays_primary, st_full.kernel_ms, (unsigned long long)st.rays_primary, st.kernel_ms, info.classify_ms);
    printf("%u of %d pixels refined (%.1f %%): %u by the edges of sample 0, %u more by the defocus criterion (largest circle of confusion %.2f pixels)\n",
           info.n_refined, N, 100.0 * info.n_refined / N, n_edges, n_defocus, coc_max);
    printf("view memory %llu bytes, the coc plane among them\n", (unsigned long long)vinfo.bytes);
    printf("%s\n", mask_same ? "the mask equals the host models' mask" : "THE MASK DIFFERS FROM THE HOST MODELS'");
    printf("%s; %d unrefined pixels differ from the full frame\n",
           refined_same ? "every refined pixel equals the full lens frame's pixel" : "A REFINED PIXEL DIFFERS FROM THE FULL FRAME'S", flat_differ);
    rc = mask_same && refined_same && n_defocus > 0 && info.n_refined < N && st.rays_primary == (unsigned long long)N + info.n_live_rays ? 0 : 1;
  }
  rt_view_destroy(view);
  rt_view_destroy(view1);
  rt_scene_destroy(scene);
  free(full_rgb), free(rgb), free(one_rgb), free(one_t), free(coc), free(one_id), free(one_valid), free(mask), free(want_mask);
  return rc;
}
