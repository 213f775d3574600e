/*
 * c_list_intersections_example.c -- the multi-hit ray query from plain C: builds a stack of 40 panes (two of them coincident)
 * between two spheres, lists the layers under one picking ray eight at a time -- feeding the last key of each page back as
 * the cursor, so that the coincident pair is neither lost nor repeated -- and counts them with `total`.  It runs the pages
 * through rt_list_intersections_model (the specification: a linear scan on the host) and, when there is a GPU, through
 * rt_list_intersections, and compares the two bit for bit.  Without a GPU it runs the model alone, says so and exits 0.
 *
 *   gcc -I include examples/c_list_intersections_example.c -L hslu_i/ba_raytracing/f2501_raytracer_amd -lrt_hip \
 *       -Wl,-rpath,$PWD/hslu_i/ba_raytracing/f2501_raytracer_amd -lm -o /tmp/c_list_intersections_example
 */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "rt_hip.h"

#define PANES 40
#define K 8
#define MAX_PAGES 16

typedef struct {
  uint32_t count, total;
  int32_t id[K];
  float t[K], point[K][3], normal[K][3];
  uint32_t material[K];
} page;

/* one page of the ray's layers behind the cursor (NULL: from the start); scene NULL: the model */
static int list_page(rt_scene* scene, const rt_scene_desc* d, const rt_ray_batch* ray, const float* after_t, const int32_t* after_id, page* p) {
  rt_ray_hit_lists l;
  memset(&l, 0, sizeof(l));
  l.max_hits = K;
  l.after_t = after_t, l.after_id = after_id;
  l.count = &p->count, l.total = &p->total;
  l.id = p->id, l.t = p->t, l.point = &p->point[0][0], l.normal = &p->normal[0][0], l.material = p->material;
  return scene ? rt_list_intersections(scene, ray, &l) : rt_list_intersections_model(d, ray, &l);
}

/* all pages of the ray: each starts behind the last key of the one before; -> number of pages, or -1 */
static int list_all(rt_scene* scene, const rt_scene_desc* d, const rt_ray_batch* ray, page* pages) {
  int n = 0;
  const float* after_t = NULL;
  const int32_t* after_id = NULL;
  for (;;) {
    if (n == MAX_PAGES || list_page(scene, d, ray, after_t, after_id, &pages[n]) != RT_OK) return -1;
    const page* p = &pages[n++];
    if (p->count < K) return n; /* a page that is not full is the last one */
    after_t = &p->t[K - 1], after_id = &p->id[K - 1];
  }
}

int main(void) {
  /* the ray starts at the centre of sphere 0 and runs along +z through the panes z = 1 .. 40 (pane 10 lies at z = 10 as pane 9
   * does) into sphere 1 */
  const float sphere_center[2][3] = {{0.25f, 0.25f, 0.0f}, {0.25f, 0.25f, 50.0f}};
  const float sphere_r_sq[2] = {0.25f, 4.0f}, sphere_r_inv[2] = {2.0f, 0.5f};
  const uint32_t sphere_material[2] = {0, 0};
  static float tri_v1[PANES][3], tri_e1[PANES][3], tri_e2[PANES][3], tri_normal[PANES][3];
  static uint32_t tri_material[PANES];
  for (int k = 0; k < PANES; k++) {
    tri_v1[k][2] = (k == 10) ? 10.0f : (float)(k + 1);
    tri_e1[k][0] = 1.0f, tri_e2[k][1] = 1.0f, tri_normal[k][2] = 1.0f;
    tri_material[k] = 1;
  }
  const float materials[2 * RT_MATERIAL_STRIDE] = {
      1.0f, 0.2f, 0.2f, 0.0f, 0.3f, 1.0f, 0.0f, 0.0f, 0.0f, /* red, shiny */
      0.5f, 0.75f, 0.75f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f /* pane */
  };
  const float lights[RT_LIGHT_STRIDE] = {0.3f, 0.1f, 0.0f, 1.0f, 1.0f, 1.0f, 0.8f};

  rt_scene_desc d;
  memset(&d, 0, sizeof(d));
  d.abi_version = RT_ABI_VERSION;
  d.n_spheres = 2;
  d.sphere_center = &sphere_center[0][0];
  d.sphere_r_sq = sphere_r_sq;
  d.sphere_r_inv = sphere_r_inv;
  d.sphere_material = sphere_material;
  d.n_triangles = PANES;
  d.tri_v1 = &tri_v1[0][0];
  d.tri_e1 = &tri_e1[0][0];
  d.tri_e2 = &tri_e2[0][0];
  d.tri_normal = &tri_normal[0][0];
  d.tri_material = tri_material;
  d.n_materials = 2;
  d.materials = materials;
  d.n_lights = 1;
  d.lights = lights;

  const float origin[3] = {0.25f, 0.25f, 0.0f}, direction[3] = {0.0f, 0.0f, 2.0f}; /* (any length) */
  rt_ray_batch ray;
  memset(&ray, 0, sizeof(ray));
  ray.abi_version = RT_ABI_VERSION;
  ray.n_rays = 1;
  ray.origin = origin;
  ray.direction = direction;

  static page model[MAX_PAGES], device[MAX_PAGES];
  const int n_model = list_all(NULL, &d, &ray, model);
  if (n_model < 0) {
    fprintf(stderr, "rt_list_intersections_model: %s\n", rt_last_error());
    return 1;
  }
  uint32_t layers = 0;
  for (int p = 0; p < n_model; p++) {
    printf("page %d (%u of the %u layers behind its cursor):", p, model[p].count, model[p].total);
    for (uint32_t j = 0; j < model[p].count; j++) printf(" %d@%g", model[p].id[j], model[p].t[j]);
    printf("\n");
    layers += model[p].count;
  }
  printf("layers under the ray: %u (total of the first call: %u)\n", layers, model[0].total);
  if (layers != model[0].total) return 1;

  if (rt_device_count() <= 0) {
    printf("no HIP device: the model alone\n");
    return 0;
  }
  rt_scene* scene = NULL;
  if (rt_scene_create(&d, 0, &scene) != RT_OK) {
    fprintf(stderr, "rt_scene_create: %s\n", rt_last_error());
    return 1;
  }
  const int n_device = list_all(scene, &d, &ray, device);
  int rc = 0;
  if (n_device < 0) {
    fprintf(stderr, "rt_list_intersections: %s\n", rt_last_error());
    rc = 1;
  } else {
    const int same = n_device == n_model && !memcmp(model, device, sizeof(page) * (size_t)n_model);
    printf("device equals model: %s\n", same ? "yes" : "NO");
    rc = same ? 0 : 1;
  }
  rt_scene_destroy(scene);
  return rc;
}
