// rt_rays.h -- radiance queries (rt_trace_rays*): the render's per-ray function, single_raytrace
// (src/renderer/raytracer_renderer.rs:147-264), for rays the CALLER supplies instead of the camera rays primary_body derives
// from a pixel index.
//
// Included at the end of rt_kernels.hip INSIDE its anonymous namespace (as rt_phases.h and rt_query.h are): the kernels run
// process_ray itself, so everything below the ray source -- nearest hit, the lights' shadow and transmittance rays, the
// soft-shadow clouds, attenuation, the children of the reflection / refraction trees -- is the code the frame runs.
//
// One ray per lane, ray i = "pixel" i of a frame of n x 1 pixels: the light-cloud set of ray i is the one pixel i would
// take, its children carry i as their pixel, and (STREAM) its sums meet in accumulator entry i.  The mapping is linear
// (workgroup w of the frame's list holds positions 256 w .. 256 w + 255), not the super-tile order of a frame.  Position k
// holds ray k, or ray order[k] when the call came with a ray order (rt_trace_rays_ordered*; built by rt_order.hip): the
// walks inside process_ray are wave-cooperative, so a wavefront of unrelated rays is correct but visits the union of their
// nodes, and an order packs neighbours in space into one wavefront.  The results do not depend on the packing.
//
// Kernel arguments: process_ray and its callees read sc and P again from the kernarg segment at offsets 0 and 88
// (kernarg_scene / kernarg_params), so the kernels take (RtDevScene, RtDevParams) first and the batch as a THIRD argument,
// read again behind process_ray the same way (kernarg_rays).
//
// Dead rays (the query rule, rt_query.h): a direction that normalises to NaN or a non-finite origin is a miss and is not
// counted as a ray.

#define RT_KERNARG_OFF_R ((RT_KERNARG_OFF_P + sizeof(RtDevParams) + alignof(RtRayArgs) - 1) / alignof(RtRayArgs) * alignof(RtRayArgs))
__device__ __forceinline__ const RtRayArgs& kernarg_rays() { return *(const RtRayArgs*)((const char*)kernarg_fresh() + RT_KERNARG_OFF_R); }

// the position of this thread in the frame's work list (the chains of a batch with secondary rays interleave: rt_batch_wg)
__device__ __forceinline__ uint32_t ray_slot(const RtDevParams& P, uint32_t tid) { return rt_batch_wg(P, blockIdx.x) * 256u + tid; }
// ... and the ray at that position: the caller's order, or through a ray order (rt_ray_order: a permutation of [0, n)).  Past
// the end of the list: the position itself (>= n, never a ray).  Ray i stays ray i whatever its position: its cloud set,
// its accumulator entry and its outputs are indexed by i.
__device__ __forceinline__ uint32_t ray_index(const RtRayArgs& R, uint32_t slot) { return R.order && slot < R.n ? R.order[slot] : slot; }

// STREAM: children are queued and the ray's own terms are added to accumulator entry i (rt_resolve_kernel then writes rgb
// and argb); otherwise the colour is complete here and every plane is written directly.
template <bool CULL, bool STREAM>
__device__ __forceinline__ void rays_body(const RtDevScene& sc, const RtDevParams& P, const RtRayArgs& R, float* lds_stash,
                                          unsigned long long* lds_cnt) {
  Wave wv;
  wave_init(wv);
  wave_flush_init(P, lds_cnt);
  const uint32_t i = ray_index(R, ray_slot(P, threadIdx.x));
  const bool have = i < R.n;
  RayIn r;
  load_ray(R.origin, R.direction, i, have, r.o, r.d_raw);
  const bool finite_o = finite_origin(r.o);
  r.n_start = P.air_ior;
  r.Wt = mk(1.0f, 1.0f, 1.0f);
  r.depth = -1;
  r.kind = KIND_PRIMARY;
  r.pix = i;
  r.mult = 1u;
  Hit none;
  none.t = INFINITY;
  none.id = -1;
  RayOut out = process_ray<CULL, false, STREAM, CfgRays>(sc, P, wv, have && finite_o, r, lds_stash, none);
  // the kernel arguments again, from the kernarg segment: nothing of them is held through process_ray
  const RtDevParams& P1 = kernarg_params();
  const RtRayArgs& R1 = kernarg_rays();
  uint32_t tid2 = threadIdx.x;
  RT_OPAQUE(tid2);  // keeps hipcc from carrying the first index through process_ray
  const uint32_t i2 = ray_index(R1, ray_slot(P1, tid2));
  const bool on = i2 < R1.n, hit = on && out.hit;
  if (on) {
    if (R1.valid) R1.valid[i2] = hit ? 1u : 0u;
    if (R1.id) R1.id[i2] = hit ? out.id : -1;
    if (R1.t) R1.t[i2] = hit ? out.t : INFINITY;
  }
  if (STREAM) {
    if (hit) {
      const long long* fx = stash_fix(lds_stash) + tid2;  // this lane's own terms, already integers (process_ray)
      acc_add_fixed(P1, i2, fx[0], fx[256], fx[512], 1u);
      P1.acc[4 * (size_t)i2 + 3] = 1;
    }
  } else if (on) {
    const V3 c = out.contrib;  // (0, 0, 0) on a miss
    if (R1.rgb) {
      const size_t k = 3u * (size_t)i2;
      R1.rgb[k] = c.x, R1.rgb[k + 1] = c.y, R1.rgb[k + 2] = c.z;
    }
    if (R1.argb && hit) R1.argb[i2] = pack_argb(c);
  }
  wave_flush(wv, P1, (uint32_t)__popcll(wave_ballot(hit)), lds_cnt);
}

// without secondary rays: one launch, every plane written here
__global__ __launch_bounds__(256, RT_MIN_WAVES) void rt_rays_kernel(RtDevScene sc, RtDevParams P, RtRayArgs R) {
  __shared__ __attribute__((aligned(16))) float lds_stash[RT_STASH_FIX * 256];  // (no fixed-point sums without secondary rays)
  __shared__ unsigned long long lds_cnt[20];
  if (P.flags & RT_FLAG_BACKFACE_CULLING)
    rays_body<true, false>(sc, P, R, lds_stash, lds_cnt);
  else
    rays_body<false, false>(sc, P, R, lds_stash, lds_cnt);
}

// with reflections / refractions: level 0 of the chained schedule (rt_primary_stream_kernel's place)
__global__ __launch_bounds__(256, RT_MIN_WAVES) void rt_rays_stream_kernel(RtDevScene sc, RtDevParams P, RtRayArgs R) {
  __shared__ __attribute__((aligned(16))) float lds_stash[RT_STASH_FIELDS * 256];
  __shared__ unsigned long long lds_cnt[20];
  if (P.flags & RT_FLAG_BACKFACE_CULLING)
    rays_body<true, true>(sc, P, R, lds_stash, lds_cnt);
  else
    rays_body<false, true>(sc, P, R, lds_stash, lds_cnt);
}
