/* Test-side reference of the ray queries (rt_cast_rays*, rt_any_intersection*): batch wrappers around the oracle's own
 * restatements of Raytracer::cast_ray (`nearest`) and Raytracer::has_any_intersection (`shadow_test`).  The tests
 * compile this file with the oracle's flags; the oracle itself is included as it is. */
#include <float.h>

#include "../oracle/rt_oracle.c"

/* a dead ray: the direction normalises to NaN (deviation D2) or the origin is not finite */
static int rq_dead(v3 o, v3 d) {
  return has_nan3(d) || !(fabsf(o.x) <= FLT_MAX && fabsf(o.y) <= FLT_MAX && fabsf(o.z) <= FLT_MAX);
}

void rq_nearest(const rt_scene_desc* s, int cull, uint32_t n, const float* org, const float* dir, int32_t* id, float* t,
                float* p, float* nrm, uint32_t* mat) {
  ctx_t c;
  memset(&c, 0, sizeof(c));
  c.s = s;
  c.cull = cull;
  for (uint32_t i = 0; i < n; i++) {
    v3 o = V(org[3 * i], org[3 * i + 1], org[3 * i + 2]);
    v3 d = vnormalize(V(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2])); /* Ray::new_with_mask, ray.rs:52-57 */
    hit_t h;
    h.valid = 0;
    if (!rq_dead(o, d)) h = nearest(&c, o, d);
    if (h.valid) {
      id[i] = h.id, t[i] = h.t, mat[i] = h.mat;
      p[3 * i] = h.p.x, p[3 * i + 1] = h.p.y, p[3 * i + 2] = h.p.z;
      nrm[3 * i] = h.n.x, nrm[3 * i + 1] = h.n.y, nrm[3 * i + 2] = h.n.z;
    } else {
      id[i] = -1, t[i] = INFINITY, mat[i] = 0xFFFFFFFFu;
      for (int k = 0; k < 3; k++) p[3 * i + k] = 0.0f, nrm[3 * i + k] = 0.0f;
    }
  }
}

/* max_d NULL = +inf */
void rq_any(const rt_scene_desc* s, int cull, uint32_t n, const float* org, const float* dir, const float* max_d, uint8_t* has,
            uint8_t* occ, float* opacity, float* filter) {
  ctx_t c;
  memset(&c, 0, sizeof(c));
  c.s = s;
  c.cull = cull;
  for (uint32_t i = 0; i < n; i++) {
    v3 o = V(org[3 * i], org[3 * i + 1], org[3 * i + 2]);
    v3 dr = V(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]);
    v3 d = vnormalize(dr);
    float tmax = max_d ? max_d[i] : INFINITY;
    has[i] = 0, occ[i] = 0, opacity[i] = 1.0f;
    filter[3 * i] = filter[3 * i + 1] = filter[3 * i + 2] = 1.0f;
    if (rq_dead(o, d)) continue;
    shadow_t r = shadow_test(&c, o, dr, tmax);
    occ[i] = (uint8_t)r.occluded;
    opacity[i] = r.opacity;
    filter[3 * i] = r.filter.x, filter[3 * i + 1] = r.filter.y, filter[3 * i + 2] = r.filter.z;
    /* has_intersection (raytracer.rs:53-55): some valid hit at t <= tmax, in object order */
    for (uint32_t k = 0; k < s->n_spheres + s->n_triangles && !has[i]; k++) {
      hit_t h;
      h.valid = 0;
      int ok = (k < s->n_spheres) ? sphere_intersect(s, k, o, d, cull, &h) : triangle_intersect(s, k - s->n_spheres, o, d, cull, &h);
      if (ok && h.t <= tmax) has[i] = 1;
    }
  }
}
