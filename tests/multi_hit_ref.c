/* Test-side reference of the multi-hit ray queries (rt_list_intersections*): every object of the description through the
 * oracle's OWN sphere_intersect / triangle_intersect, the admitted hits sorted by the key (t ascending, on equal t the larger id
 * first), the cursor applied, the first K written and all of them counted.  No tree, no list of bounded size, no paging: what
 * rt_list_intersections_model must equal bit for bit.  The tests compile this file with the oracle's flags; the oracle itself is
 * included as it is. */
#include <float.h>

#include "../oracle/rt_oracle.c"

static int mh_dead(v3 o, v3 d) {
  return has_nan3(d) || !(fabsf(o.x) <= FLT_MAX && fabsf(o.y) <= FLT_MAX && fabsf(o.z) <= FLT_MAX);
}

static int mh_before(const void* a, const void* b) {
  const hit_t *x = (const hit_t*)a, *y = (const hit_t*)b;
  if (x->t < y->t) return -1;
  if (x->t > y->t) return 1;
  return (x->id > y->id) ? -1 : (x->id < y->id) ? 1 : 0;
}

/* max_d, after_t / after_id, total: NULL = absent.  Planes [n][K]. */
void mh_list(const rt_scene_desc* s, int cull, uint32_t n, uint32_t K, const float* org, const float* dir, const float* max_d,
             const float* after_t, const int32_t* after_id, uint32_t* count, uint32_t* total, int32_t* id, float* t, float* p, float* nrm,
             uint32_t* mat) {
  const uint32_t n_obj = s->n_spheres + s->n_triangles;
  hit_t* hits = (hit_t*)malloc(sizeof(hit_t) * (n_obj ? n_obj : 1));
  for (uint32_t i = 0; i < n; i++) {
    v3 o = V(org[3 * i], org[3 * i + 1], org[3 * i + 2]);
    v3 d = vnormalize(V(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2])); /* Ray::new_with_mask, ray.rs:52-57 */
    const float tmax = max_d ? max_d[i] : INFINITY;
    uint32_t m = 0;
    if (!mh_dead(o, d)) {
      for (uint32_t k = 0; k < n_obj; k++) {
        hit_t h;
        h.valid = 0;
        int ok = (k < s->n_spheres) ? sphere_intersect(s, k, o, d, cull, &h) : triangle_intersect(s, k - s->n_spheres, o, d, cull, &h);
        if (!ok || !(h.t <= tmax)) continue;
        if (after_t && !(h.t > after_t[i] || (h.t == after_t[i] && h.id < after_id[i]))) continue;
        hits[m++] = h;
      }
    }
    qsort(hits, m, sizeof(hit_t), mh_before);
    count[i] = m < K ? m : K;
    if (total) total[i] = m;
    for (uint32_t j = 0; j < K; j++) {
      const size_t at = (size_t)i * K + j;
      if (j < m) {
        const hit_t* h = &hits[j];
        id[at] = h->id, t[at] = h->t, mat[at] = h->mat;
        p[3 * at] = h->p.x, p[3 * at + 1] = h->p.y, p[3 * at + 2] = h->p.z;
        nrm[3 * at] = h->n.x, nrm[3 * at + 1] = h->n.y, nrm[3 * at + 2] = h->n.z;
      } else {
        id[at] = -1, t[at] = INFINITY, mat[at] = 0xFFFFFFFFu;
        for (int k = 0; k < 3; k++) p[3 * at + k] = 0.0f, nrm[3 * at + k] = 0.0f;
      }
    }
  }
  free(hits);
}
