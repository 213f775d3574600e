// rt_query.h -- ray queries on a scene that is already on the device: the reference's two other public functions on a
// scene besides the render, Raytracer::cast_ray (nearest hit, src/raytracing/raytracer.rs:162-220) and
// Raytracer::has_any_intersection (visibility and transmittance of a segment, raytracer.rs:24-106).
//
// Included at the end of rt_kernels.hip INSIDE its anonymous namespace (as rt_phases.h is), so that the kernels share the
// exact intersection helpers (sphere_hit, tri_hit, exact_sqrt / exact_rcp, normalize, surface_of) and the fixed-point
// transmittance state (Shadow, shadow_accumulate*) with the render without moving them.  Nothing here reads the kernel
// arguments through kernarg_scene() / kernarg_params(): those assume the argument layout of the render kernels.
//
// One lane per ray.  A query batch can be arbitrary (picking rays, probes, segments between unrelated points), and the
// render's wave-cooperative walk (nearest_hit) visits the union of the wavefront's nodes -- thousands for 64 unrelated
// rays, against ~50 for one lane alone (rt_hard_kernel).  So every lane walks the threaded copy of the tree (RtThrNode:
// depth first, skip links, no stack) for its own ray with per-lane vector loads -- walk_tris_lane, the walk rt_hard_kernel
// runs; spheres are few and are tested by the whole wavefront one after the other (a loop that is uniform across the wavefront).
//
// Far origins.  The BVH boxes are padded for the rounding of rays that start in or near the scene (rt_bvh.cpp): 2e-5 +
// 1e-4 of the triangle's extent + 4 ulp of its coordinates.  The literal triangle test's own rounding reaches past the
// triangle by an amount that grows with the distance |v1 - o| (a few ulp of it, divided by the cosine of the angle of
// incidence), so a query that starts far away widens every box by 8e-6 |o|_1 on every side (`far_pad`): ~70 ulp of the
// origin's magnitude.  That covers the overreach for every ray not within a few degrees of grazing the triangle's plane;
// rays from 100x the scene's extent are part of the parity tests (tests/test_ray_query_gpu.py).  The widening only adds
// node visits -- every triangle that is reached still goes through the literal test.
//
// Degenerate input (deviation D2 of the render): a direction that normalises to NaN (zero length, NaN or
// inf components) or a non-finite origin makes a dead ray -- a miss, and for the any-hit query "no intersection,
// opacity 1, filter 1".  The reference's triangle arithmetic would accept NaN / inf "hits" for such rays.

// ray `i` of a caller's batch as it lies in memory (zeros in a lane without one: 12 bytes per lane and array, contiguous
// across the wavefront), and the test of its origin: a non-finite origin makes a dead ray
__device__ __forceinline__ void load_ray(const float* origin, const float* direction, uint32_t i, bool have, V3& o, V3& d_raw) {
  o = mk(0.0f, 0.0f, 0.0f);
  d_raw = mk(0.0f, 0.0f, 0.0f);
  if (have) {
    const size_t k = 3u * (size_t)i;
    o = mk(origin[k], origin[k + 1], origin[k + 2]);
    d_raw = mk(direction[k], direction[k + 1], direction[k + 2]);
  }
}
__device__ __forceinline__ bool finite_origin(V3 o) {
  return fabsf(o.x) <= 3.4028235e38f && fabsf(o.y) <= 3.4028235e38f && fabsf(o.z) <= 3.4028235e38f;
}

// the ray of lane `i`: origin and the direction as Ray::new_with_mask normalises it (ray.rs:52-57)
__device__ __forceinline__ bool query_ray(const RtQueryArgs& q, uint32_t i, bool have, V3& o, V3& d) {
  V3 dr;
  load_ray(q.origin, q.direction, i, have, o, dr);
  d = normalize(dr);
  const bool finite_o = finite_origin(o);
  return have && finite_o && !has_nan(d);
}

__device__ __forceinline__ float far_pad(V3 o) { return 8e-6f * ((fabsf(o.x) + fabsf(o.y)) + fabsf(o.z)); }

// ---- nearest hit (cast_ray) --------------------------------------------------------------------------------------
// The triangles of the lane's own walk.  A box whose entry lies beyond the lane's best t (plus the slab slack) is
// skipped, so a hit at EQUAL t in another box is never cut, and such a tie goes to the larger canonical id, as the
// reference's scan in object order decides it (simd_le, raytracer.rs:194).  Split clipping puts several references of a
// triangle into the leaves: each gives the same t and id, and the tie rule keeps the first.
template <bool CULL>
__device__ __forceinline__ void nearest_tris_lane(const RtDevScene& sc, lanemask grp, V3 o, V3 d, float pad, Hit& best) {
  const int tri_base = (int)sc.n_spheres;
  walk_tris_lane<true>(
      sc, grp, o, d, pad, [&]() __attribute__((always_inline)) { return best.t; }, []() __attribute__((always_inline)) { return (lanemask)0; },
      [&](uint32_t slot, float t, lanemask h) __attribute__((always_inline)) {
        if (!h) return;
        if (CULL) {  // triangle.rs:154-168
          const float4 sh = vload<float4>(sc, sc.off_tri_shade + slot * 16u);
          const Mat m = load_mat(sc, lane_of(h) ? __float_as_uint(sh.w) : 0u);
          h &= wave_ballot(m.transmissive || dot(d, mk(sh.x, sh.y, sh.z)) < 0.75f);
        }
        if (!h) return;
        const int id = tri_base + (int)(vload<uint32_t>(sc, sc.off_tri_id + slot * 4u) & RT_TRI_INDEX_MASK);
        if (lane_of(h) && (t < best.t || (t == best.t && id > best.id))) {
          best.t = t;
          best.id = id;
        }
      });
}

template <bool CULL>
__device__ __forceinline__ void query_nearest_body(const RtDevScene& sc, const RtQueryArgs& q, uint32_t i, bool have) {
  V3 o, d;
  const bool alive = query_ray(q, i, have, o, d);
  const lanemask grp = wave_ballot(alive);
  Hit best;
  best.t = INFINITY;
  best.id = -1;
  if (grp) {
    // spheres in index order: a later sphere at equal t wins (raytracer.rs:193-213)
    for (uint32_t k = 0; k < sc.n_spheres; k++) {
      const float4 s = sload<float4>(sc, sc.off_spheres + k * 16u);
      float t = 0.0f;
      bool h = alive && sphere_hit(s, o, d, t);
      if (CULL && h) {  // sphere.rs:137-151
        const V3 n = normalize(fma_s(d, t, o) - mk(s.x, s.y, s.z));
        const Mat m = load_mat_u(sc, sload<uint32_t>(sc, sc.off_sphere_mat + k * 4u));
        h = (dot(d, n) < 0.75f) || m.transmissive;
      }
      if (h && t <= best.t) {
        best.t = t;
        best.id = (int)k;
      }
    }
    if (sc.n_triangles) nearest_tris_lane<CULL>(sc, grp, o, d, far_pad(o), best);
  }
  if (!have) return;
  const bool hit = best.id >= 0;
  Surf sf;
  sf.p = mk(0.0f, 0.0f, 0.0f);
  sf.n = sf.p;
  sf.mat = 0xFFFFFFFFu;
  if (hit) sf = surface_of(sc, best, o, d);  // SurfaceInteraction, surface_interaction.rs:13-30
  if (q.id) q.id[i] = best.id;
  if (q.t) q.t[i] = best.t;
  const size_t k = 3u * (size_t)i;
  if (q.point) q.point[k] = sf.p.x, q.point[k + 1] = sf.p.y, q.point[k + 2] = sf.p.z;
  if (q.normal) q.normal[k] = sf.n.x, q.normal[k + 1] = sf.n.y, q.normal[k + 2] = sf.n.z;
  if (q.material) q.material[i] = sf.mat;
}

// ---- any hit (has_any_intersection) ------------------------------------------------------------------------------
// Every hit at t <= max_distance counts (raytracer.rs:53-55) into the render's order-independent fixed-point state
// (Shadow): the value a lane ends with does not depend on the order its walk meets the hits in.  `any` = lanes with some
// hit.  A lane stops once it is completely occluded: its opacity is 0 whatever follows, and its colour filter is
// unspecified from then on (the reference stops at its first opaque hit in object order).  Split clipping duplicates
// only opaque triangles (rt_api.cpp: transmissive ones are never split), and an opaque hit is idempotent here.
template <bool CULL>
__device__ __forceinline__ void query_any_body(const RtDevScene& sc, const RtQueryArgs& q, uint32_t i, bool have) {
  V3 o, d;
  bool alive = query_ray(q, i, have, o, d);
  const float tmax = (have && q.max_distance) ? q.max_distance[i] : INFINITY;
  alive = alive && tmax >= 0.0f;  // NaN or negative: no hit can count (t >= 0 for spheres, t > eps for triangles)
  const lanemask grp = wave_ballot(alive);
  Shadow S;
  shadow_init(S);
  lanemask any = 0ull;
  if (grp) {
    for (uint32_t k = 0; k < sc.n_spheres; k++) {
      const float4 s = sload<float4>(sc, sc.off_spheres + k * 16u);
      float t = 0.0f;
      lanemask h = grp & ~S.occ & wave_ballot(sphere_hit(s, o, d, t));
      h &= wave_ballot(t <= tmax);
      if (h) {
        // (the exact normal: it is the oracle's and the reference's, and it feeds the Fresnel factor of the opacity)
        const V3 n = normalize(fma_s(d, t, o) - mk(s.x, s.y, s.z));
        const Mat m = load_mat_u(sc, sload<uint32_t>(sc, sc.off_sphere_mat + k * 4u));
        if (CULL && !m.transmissive) h &= wave_ballot(dot(d, n) < 0.75f);  // sphere.rs:137-151
        any |= h;
        shadow_accumulate(S, m, n, d, h);
      }
    }
    if (sc.n_triangles) shadow_tris_lane<CULL, true>(sc, grp, o, d, tmax, far_pad(o), S, any);
  }
  if (!have) return;
  const bool occ = lane_of(S.occ);
  if (q.has_intersection) q.has_intersection[i] = lane_of(any) ? 1u : 0u;
  if (q.occluded) q.occluded[i] = occ ? 1u : 0u;
  if (q.opacity) q.opacity[i] = occ ? 0.0f : shadow_opacity(S);
  if (q.filter) {
    const V3 f = shadow_filter(S);
    const size_t k = 3u * (size_t)i;
    q.filter[k] = f.x, q.filter[k + 1] = f.y, q.filter[k + 2] = f.z;
  }
}

// One lane per ray, a grid-stride loop over the batch (the stride is wave-uniform; the tail wavefront runs with `have`
// false in its idle lanes).
__global__ __launch_bounds__(256) void rt_query_nearest_kernel(RtDevScene sc, RtQueryArgs q) {
  for (size_t base = (size_t)blockIdx.x * 256u; base < q.n; base += (size_t)gridDim.x * 256u) {
    const size_t i = base + threadIdx.x;
    const bool have = i < q.n;
    if (q.cull)
      query_nearest_body<true>(sc, q, (uint32_t)i, have);
    else
      query_nearest_body<false>(sc, q, (uint32_t)i, have);
  }
}

__global__ __launch_bounds__(256) void rt_query_any_kernel(RtDevScene sc, RtQueryArgs q) {
  for (size_t base = (size_t)blockIdx.x * 256u; base < q.n; base += (size_t)gridDim.x * 256u) {
    const size_t i = base + threadIdx.x;
    const bool have = i < q.n;
    if (q.cull)
      query_any_body<true>(sc, q, (uint32_t)i, have);
    else
      query_any_body<false>(sc, q, (uint32_t)i, have);
  }
}
