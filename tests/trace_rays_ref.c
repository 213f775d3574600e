/* Test-side reference of the radiance queries (rt_trace_rays*): a batch wrapper around the oracle's own restatement of
 * single_raytrace (`trace`, raytracer_renderer.rs:147-264).  Ray i is pixel i: build_lights(&c, i) picks its light
 * clouds (`index`, when given, names the pixel of each ray: a sample of a larger batch keeps its rays' own clouds).  The tests compile this file with the oracle's flags; the oracle itself is included as it is. */
#include <float.h>

#include "../oracle/rt_oracle.c"

typedef struct {
  const rt_scene_desc* s;
  const rt_params* p;
  uint32_t n;
  const float *org, *dir;
  const uint32_t* index;
  float* rgb;
  uint8_t* valid;
  int32_t* id;
  float* t;
  uint32_t* argb;
  volatile uint32_t* next;
  uint64_t rays[3], shadow, written;
} tr_job;

static void* tr_worker(void* arg) {
  tr_job* j = (tr_job*)arg;
  ctx_t c;
  memset(&c, 0, sizeof(c));
  c.s = j->s;
  c.p = j->p;
  c.cull = (j->p->flags & RT_FLAG_BACKFACE_CULLING) != 0;
  uint32_t N = j->p->light_mult < 1 ? 1 : j->p->light_mult;
  size_t nl = (size_t)j->s->n_lights * N;
  c.lpos = (float*)malloc(sizeof(float) * 3 * (nl + 1));
  c.lcol = (float*)malloc(sizeof(float) * 3 * (nl + 1));
  c.lint = (float*)malloc(sizeof(float) * (nl + 1));
  for (;;) {
    uint32_t first = __atomic_fetch_add(j->next, 64u, __ATOMIC_RELAXED);
    if (first >= j->n) break;
    uint32_t last = first + 64u < j->n ? first + 64u : j->n;
    for (uint32_t i = first; i < last; i++) {
      v3 o = V(j->org[3 * i], j->org[3 * i + 1], j->org[3 * i + 2]);
      v3 d_raw = V(j->dir[3 * i], j->dir[3 * i + 1], j->dir[3 * i + 2]);
      trace_t r;
      r.hit = 0;
      /* a dead ray (the query rule): the direction normalises to NaN, or the origin is not finite -- a miss, not counted */
      int dead = has_nan3(vnormalize(d_raw)) || !(fabsf(o.x) <= FLT_MAX && fabsf(o.y) <= FLT_MAX && fabsf(o.z) <= FLT_MAX);
      if (!dead) {
        build_lights(&c, j->index ? j->index[i] : i);
        r = trace(&c, o, d_raw, j->p->air_ior, -1, KIND_PRIMARY);
      }
      if (r.hit) {
        j->rgb[3 * i] = r.color.x, j->rgb[3 * i + 1] = r.color.y, j->rgb[3 * i + 2] = r.color.z;
        j->valid[i] = 1, j->id[i] = r.id, j->t[i] = r.t;
        j->argb[i] = pack_pixel(r.color);
        j->written++;
      } else {
        j->rgb[3 * i] = j->rgb[3 * i + 1] = j->rgb[3 * i + 2] = 0.0f;
        j->valid[i] = 0, j->id[i] = -1, j->t[i] = INFINITY; /* argb: untouched */
      }
    }
  }
  for (int k = 0; k < 3; k++) j->rays[k] = c.rays[k];
  j->shadow = c.shadow;
  free(c.lpos);
  free(c.lcol);
  free(c.lint);
  return NULL;
}

/* counters: rays_primary, rays_reflection, rays_refraction, rays_shadow, valid rays */
int tr_trace(const rt_scene_desc* s, const rt_params* p, uint32_t n, const float* org, const float* dir, const uint32_t* index, float* rgb, uint8_t* valid,
             int32_t* id, float* t, uint32_t* argb, uint64_t counters[5], int n_threads) {
  if (p->light_mult > 1 && (p->n_cloud_sets == 0 || !p->cloud_sets)) return RT_ERR_INVALID_ARG;
  if (n_threads < 1) n_threads = 1;
  if (n_threads > 64) n_threads = 64;
  tr_job jobs[64];
  pthread_t th[64];
  volatile uint32_t next = 0;
  for (int k = 0; k < n_threads; k++) {
    tr_job* j = &jobs[k];
    memset(j, 0, sizeof(*j));
    j->s = s, j->p = p, j->n = n, j->org = org, j->dir = dir, j->index = index;
    j->rgb = rgb, j->valid = valid, j->id = id, j->t = t, j->argb = argb, j->next = &next;
  }
  if (n_threads == 1) {
    tr_worker(&jobs[0]);
  } else {
    for (int k = 0; k < n_threads; k++) pthread_create(&th[k], NULL, tr_worker, &jobs[k]);
    for (int k = 0; k < n_threads; k++) pthread_join(th[k], NULL);
  }
  memset(counters, 0, 5 * sizeof(uint64_t));
  for (int k = 0; k < n_threads; k++) {
    counters[0] += jobs[k].rays[0], counters[1] += jobs[k].rays[1], counters[2] += jobs[k].rays[2];
    counters[3] += jobs[k].shadow, counters[4] += jobs[k].written;
  }
  return RT_OK;
}
