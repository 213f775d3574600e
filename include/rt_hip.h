/*
 * rt_hip.h -- C ABI of the MI355X-native render loop (drop-in for the reference's
 * `Renderer::render` path).
 *
 * This is the boundary a Rust `impl Renderer<W,H,C> for HipRenderer` (or any other FFI host)
 * binds.  Plain pointers and sizes only; no C++/torch types cross it.
 *
 * What each entry point replaces in the reference (paths relative to the reference repo):
 *
 *   rt_scene_create   <- Scene<Vec3>{scene_objects, scene_lights}      src/scene/scene.rs:24-27
 *                        (flattened: spheres src/geometry/basic/sphere.rs:20-30,
 *                         triangles src/geometry/basic/triangle.rs:22-48,
 *                         materials src/raytracing/material.rs:15-19,78-89,
 *                         point lights src/scene/lighting/light.rs:162-169)
 *   rt_render         <- <RaytracerRenderer<C> as Renderer<W,H,C>>::render
 *                        src/renderer/raytracer_renderer.rs:1360-1378, driver
 *                        src/renderer/mod.rs:146-209; output layout = ImageBuffer<W,H>
 *                        src/image_buffer.rs:8-15 packed by OutputColorEncoder::to_output
 *                        src/output/window.rs:105-109
 *   rt_render_device  <- same, but the packed pixels stay in a caller-provided DEVICE buffer
 *                        (used by the multi-GPU gather and by bench.py, HBM-resident I/O)
 *   rt_params         <- the compile-time feature/const table: src/lib.rs:30-92,
 *                        src/renderer/raytracer_renderer.rs:55-127
 *   rt_scene_destroy  <- Drop of Scene
 *   rt_cast_rays      <- Raytracer::cast_ray, src/raytracing/raytracer.rs:162-220 (nearest hit as a
 *                        SurfaceInteraction, src/raytracing/surface_interaction.rs:13-30), for a batch of
 *                        HOST rays; blocks
 *   rt_cast_rays_device          <- same, DEVICE arrays, enqueued on the caller's stream
 *   rt_any_intersection          <- Raytracer::has_any_intersection, raytracer.rs:24-106 (IntersectionTest,
 *                                   raytracer.rs:17-22), for a batch of HOST segments; blocks
 *   rt_any_intersection_device   <- same, DEVICE arrays, enqueued on the caller's stream
 *   rt_list_intersections[_device] <- none (has_any_intersection visits every hit at t <= max_distance; this returns them):
 *                                   the first K hits per ray in order and their number; rt_list_intersections_model is
 *                                   its specification
 *   rt_ambient_occlusion[_device] <- none (the reference shades with point lights only): which of S hemisphere directions
 *                                   above a surface point are blocked, their number and the bent normal;
 *                                   rt_ambient_occlusion_model is its specification
 *   rt_closest_points[_device]   <- none (the reference has no point query): the nearest surface point per query
 *                                   point, Embree's rtcPointQuery; rt_closest_points_model is its specification
 *   rt_contains_points[_device], rt_signed_distance[_device] <- none: whether a point lies inside the closed surfaces of
 *                                   the scene, by crossing parity or winding along up to 8 directions, and the signed
 *                                   distance to the surface; the two _model functions are their specification
 *   rt_trace_rays     <- RaytracerRenderer::single_raytrace, src/renderer/raytracer_renderer.rs:147-264 (the colour of
 *                        a ray: nearest hit, the lights' shadow and transmittance rays, soft-shadow clouds, attenuation,
 *                        reflection and refraction trees), for a batch of HOST rays; blocks
 *   rt_trace_rays_device         <- same, DEVICE arrays, enqueued on the caller's stream
 *   rt_ray_order_*, rt_trace_rays_ordered[_device]  <- none (the reference recurses per ray): the same colours, the
 *                        rays packed into wavefronts by a permutation sorted on the device
 *   rt_last_error     <- (reference panics: `unwrap()/expect()`); here: error codes + message
 *
 * All arithmetic on the path is fp32.  Hit ids are canonical object indices: spheres first
 * (insertion order), then triangles (insertion order); -1 = miss.
 */
#ifndef RT_HIP_H
#define RT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 4u

/* ---- error codes -------------------------------------------------------------------------- */
#define RT_OK 0
#define RT_ERR_INVALID_ARG (-1)
#define RT_ERR_NO_DEVICE (-2)
#define RT_ERR_HIP (-3)
#define RT_ERR_OOM (-4)
#define RT_ERR_UNSUPPORTED (-5)

/* ---- feature flags (reference: Cargo features read through cfg!()) ------------------------ */
#define RT_FLAG_REFLECTIONS 0x1u      /* feature "reflections"      raytracer_renderer.rs:216 */
#define RT_FLAG_REFRACTIONS 0x2u      /* feature "refractions"      raytracer_renderer.rs:232 */
#define RT_FLAG_BACKFACE_CULLING 0x4u /* feature "backface_culling" sphere.rs:137, triangle.rs:154 */
#define RT_FLAG_ANTI_ALIASING 0x8u    /* feature "anti_aliasing"    raytracer_renderer.rs:1199 */

/* ---- traversal selector (no reference counterpart: the reference scans linearly) ---------- */
#define RT_TRAVERSAL_BVH 0u    /* BVH over the triangles (result-preserving w.r.t. the scan) */
#define RT_TRAVERSAL_LINEAR 1u /* literal linear scan of all objects, raytracer.rs:48,180 */

/* material row layout inside rt_scene_desc.materials (stride RT_MATERIAL_STRIDE floats).
 * Domain: colour channels and opacity in [0, 1].  No value is validated; outside the domain a result is finite or not as
 * the arithmetic gives (an opacity above 1 never raises a shadow ray's opacity again: each hit's decrement is clamped to
 * [0, 1] before it is summed).  Inside it a shadow ray's colour filter 1 - sum(absorption) can reach 0 only together with
 * combined opacity 0, and a light sample that arrives with combined opacity 0 contributes nothing (the reference's
 * colour / filter * opacity would be inf * 0 there); the ray queries still report the filter as it sums, 0 or below included.
 * Capacity: the absorption a shadow ray collects must stay below 256 per channel (2^-24 fixed point in 32 bits; 255 white
 * panes of opacity 1e-3 fit); beyond it the filter sum wraps. */
#define RT_MATERIAL_STRIDE 9u
#define RT_MAT_R 0
#define RT_MAT_G 1
#define RT_MAT_B 2
#define RT_MAT_METALLIC 3
#define RT_MAT_SHININESS 4
#define RT_MAT_IOR 5         /* TransmissionProperties.refraction_index (raw field) */
#define RT_MAT_OPACITY 6     /* TransmissionProperties.opacity value */
#define RT_MAT_BOOST 7       /* TransmissionProperties.boost */
#define RT_MAT_HAS_OPACITY 8 /* SimdOption mask of opacity: 1.0f = Some, 0.0f = None */

/* light row layout inside rt_scene_desc.lights (stride RT_LIGHT_STRIDE floats).  The colour is
 * the one PointLight::new stores, i.e. ALREADY passed through maximize_value (light.rs:175-181). */
#define RT_LIGHT_STRIDE 7u

/* BVH builder knobs (no reference counterpart: the reference has no acceleration structure).  0 = default. */
typedef struct rt_bvh_tuning {
  uint32_t max_leaf;    /* triangles per leaf, default 4 */
  float tri_cost;       /* SAH cost of one triangle test relative to one node visit, default 2 */
  uint32_t split_depth; /* early split clipping: at most 2^depth references per triangle, default 0 = off */
  float split_gain;     /* split only if area(left) + area(right) < gain * area(whole), default 0.8 */
} rt_bvh_tuning;

typedef struct rt_scene_desc {
  uint32_t abi_version; /* RT_ABI_VERSION */

  uint32_t n_spheres;
  const float* sphere_center;      /* [n_spheres][3] */
  const float* sphere_r_sq;        /* [n_spheres]  radius*radius   sphere.rs:43 */
  const float* sphere_r_inv;       /* [n_spheres]  1/radius        sphere.rs:44 (unused by intersect) */
  const uint32_t* sphere_material; /* [n_spheres]  row in materials */

  uint32_t n_triangles;
  const float* tri_v1;          /* [n_triangles][3] vertex1           triangle.rs:35 */
  const float* tri_e1;          /* [n_triangles][3] vertex2 - vertex1 triangle.rs:65,89 */
  const float* tri_e2;          /* [n_triangles][3] vertex3 - vertex1 triangle.rs:66,90 */
  const float* tri_normal;      /* [n_triangles][3] stored face normal (may be non-unit) */
  const uint32_t* tri_material; /* [n_triangles] */

  uint32_t n_materials;
  const float* materials; /* [n_materials][RT_MATERIAL_STRIDE] */

  uint32_t n_lights;
  const float* lights; /* [n_lights][RT_LIGHT_STRIDE]: x,y,z, r,g,b, intensity */

  rt_bvh_tuning bvh; /* all 0 = defaults */

  /* Device memory the scene may spend on OPTIONAL acceleration tables on top of the scene proper (geometry + BVH, a few MB):
   * the receiver flags (2 bytes per receiver cell) and the per-cell candidate lists (16 bytes per cell and light).  The
   * reference's whole scene is < 1 MB (src/scene/scene.rs:24-27); a drop-in that shares a device should not quietly take a
   * gigabyte for a few percent.  0 = RT_SCENE_BUDGET_DEFAULT (128 MiB).  Tables that do not fit are coarsened (flags) or not
   * built (lists; rt_stats.notes says so) -- the image is the same either way.  rt_scene_memory_info reports what is held. */
  uint64_t device_budget_bytes;
} rt_scene_desc;
#define RT_SCENE_BUDGET_DEFAULT ((uint64_t)128 << 20)

/* Execution knobs that never change the image (no reference counterpart).  All 0 = defaults. */
#define RT_CAND_CAP_NONE 0xFFFFFFFFu
typedef struct rt_tuning {
  /* Soft shadows share one BVH walk per (wavefront, light): the walk collects at most this many candidate
   * triangles (1..64; 0 = default 64).  RT_CAND_CAP_NONE: no sharing, one BVH walk per shadow sample. */
  uint32_t shadow_candidate_cap;
  uint32_t chunk_log2;  /* log2 of the rays per secondary launch / primary batch; 0 = sized from free HBM */
  uint32_t no_aa_dedup; /* 1: trace every AA sample, also the bit-identical repeats of the sample table */
  uint32_t no_counters; /* 1: skip the ray counters of rt_stats (timing experiments) */
  /* rt_render_multi, testing only: use the RCCL calls even when several ranks share one GPU (real RCCL refuses such a
   * communicator; tests/mock_rccl checks the call sequence on a one-GPU box) */
  uint32_t multi_force_rccl;
  /* 1: no receiver flags.  Default 0: with soft shadows every triangle carries a grid of receiver cells, flagged per light
   * when no triangle / sphere can touch a shadow ray that starts in the cell (computed once per scene and light-cloud
   * size by rt_flags_kernel); wavefronts whose hit points all lie in clear cells skip the candidate walk -- same image */
  uint32_t no_receiver_flags;
  /* Launch order of the 16x16-pixel super-tiles of a frame (RT_TILE_ORDER_*).  The reference hands its tiles to a
   * work-stealing pool in shuffled order (src/image_buffer.rs:48-97); a GPU launch runs its workgroups in list order, and
   * cannot end before its longest wavefront does.  COST: the cost of every super-tile is measured once per scene and
   * frame shape (one calibration frame, shader-clock sums per super-tile) and the list is launched heaviest first. */
  uint32_t tile_order;
  /* Secondary rays are shaded in the order of their hit points: a counting sort on the top `sort_bits` bits of the 30-bit
   * Morton key of the hit point (12..24; 0 = default: 22, 24 for frames of more than 32 Mi primary work items).  More bits = neighbouring rays in a wavefront lie closer together
   * (their soft-shadow candidate walks are shared), at 8 bytes of device memory per bucket. */
  uint32_t sort_bits;
  /* 1: no per-cell candidate lists.  Default 0: rt_flags_kernel also LISTS, per receiver cell and light, the (up to 8)
   * triangles that survive the cell's fat beam; a wavefront whose hit points all lie in cells with complete lists takes
   * the union of those lists instead of walking the BVH for its soft-shadow candidates -- same candidates after the
   * lanes' own beam tests, same image.  16 bytes per cell and light of device memory. */
  uint32_t no_cell_lists;
  /* Chains a frame with secondary rays is split into (1..2; 0 = default 2).  The ray tree of a frame is a chain of launches,
   * one per level, and a launch cannot end before its longest wavefront does; two halves of the frame's primary work list
   * run as independent chains on two streams (the caller's and one of the library's, forked and joined with events) so that
   * the head of one chain's launch fills the drain of the other's.  Twice the queues of half the size -- same memory, same
   * image.  A host that keeps several frames in flight itself may prefer 1. */
  uint32_t sub_frames;
  /* Form of the render loop (RT_PHASES_*).  FUSED: one kernel per ray-tree level runs nearest hit, the five lights' shadow
   * classification and N-sample loops, shading and child spawning.  SPLIT: the same work as phase kernels -- hit -> per-hit
   * classification into queues of (wavefront, light) sets -> one kernel per class of set -> resolve (csrc/rt_phases.h); the
   * work item of the dominant kernels is a (wavefront, light) set, a fifth of a fused wavefront's.  Same integers in the pixel
   * accumulator, hence the same frame.  0 = the library's choice for the frame shape. */
  uint32_t phases;
  /* How the levels of a frame's ray tree are run (RT_LEVELS_*; fused kernels only).  CHAINED: per level trace -> sort -> shade,
   * the shade kernel appending the next level's rays.  MERGED: the kernel that finds a ray's hit also appends its children, so the
   * levels are traced back to back (level k+1 does not wait for level k to be shaded) and ALL levels are then shaded by ONE launch in
   * ONE hit-point order: one drain instead of one per level, and rays of every depth that hit neighbouring points share a wavefront.
   * PIPELINED: the levels are traced back to back as in MERGED, each sorted on its own, and level k is shaded -- on one of two streams
   * of the library's, alternately -- as soon as it has been traced and sorted: the trace launches (latency bound) run under the shade
   * launches (issue bound), and the head of level k+1's shading fills the compute units the drain of level k's leaves idle.
   * Same integer pixel sums, same frame.  0 = the library's choice. */
  uint32_t levels;
} rt_tuning;
#define RT_LEVELS_DEFAULT 0u
#define RT_LEVELS_CHAINED 1u
#define RT_LEVELS_MERGED 2u
#define RT_LEVELS_PIPELINED 3u
#define RT_PHASES_DEFAULT 0u
#define RT_PHASES_FUSED 1u
#define RT_PHASES_SPLIT 2u
#define RT_PHASES_FUSED_DEFER 3u /* fused kernels; frames without secondary rays also sum through the accumulator and defer incoherent soft-shadow sets to rt_hard_kernel */
#define RT_TILE_ORDER_DEFAULT 0u
#define RT_TILE_ORDER_ROW_MAJOR 1u
#define RT_TILE_ORDER_COST 2u

typedef struct rt_params {
  uint32_t abi_version; /* RT_ABI_VERSION */
  uint32_t width;       /* WINDOW_WIDTH  lib.rs:50 */
  uint32_t height;      /* WINDOW_HEIGHT lib.rs:61 */

  float focus[3];     /* RENDER_RAY_FOCUS lib.rs:88-89 */
  float fw;           /* WINDOW_TO_SCENE_WIDTH_FACTOR  lib.rs:81 */
  float fh;           /* WINDOW_TO_SCENE_HEIGHT_FACTOR lib.rs:82 */
  float fd;           /* WINDOW_TO_SCENE_DEPTH_FACTOR  lib.rs:83 */
  float eps_distance; /* Vector3DOperations::default_epsilon_distance vector.rs:697-700 */
  float air_ior;      /* DEFAULT_REFRACTION_INDEX lib.rs:92 */
  float ambient;      /* ambient intensity 0.08, raytracer_renderer.rs:754 */

  uint32_t flags; /* RT_FLAG_* */

  /* anti-aliasing sample table, already scaled and direction-multiplied
   * (bundle_rays_for_simd_antialiased_raytracing, raytracer_renderer.rs:1021-1138):
   * sample k origin = (x + aa_offsets[2k], y + aa_offsets[2k+1], 0).  Ignored (one centre ray)
   * unless RT_FLAG_ANTI_ALIASING is set. */
  uint32_t aa_rays;
  const float* aa_offsets; /* [aa_rays][2] */

  /* soft-shadow light cloud (PointLight::to_point_light_cloud<N>, light.rs:183-225).
   * light_mult = N.  N == 1: the light itself.  N > 1: light j of the cloud of light l at pixel
   * p sits at  pos_l + cloud_sets[set][j] * (fw, fh, fd)  with intensity (1/N)*I_l, where
   * set = rt_cloud_hash(cloud_seed, p, l) % n_cloud_sets  -- the seeded, reproducible stand-in
   * for the reference's unseeded per-pixel Poisson3D set. */
  uint32_t light_mult;
  uint32_t cloud_seed;
  uint32_t n_cloud_sets;
  const float* cloud_sets; /* [n_cloud_sets][light_mult][3], in "pixel units" */

  uint32_t max_depth_reflection; /* RAYTRACE_REFLECTION_MAX_DEPTH raytracer_renderer.rs:55 */
  uint32_t max_depth_refraction; /* RAYTRACE_REFRACTION_MAX_DEPTH raytracer_renderer.rs:65 */

  /* sub-rectangle to render (ChunkView, image_buffer.rs:178-251).  win_w == 0 -> full frame. */
  uint32_t win_x0, win_y0, win_w, win_h;

  /* tile ownership for multi-GPU: RENDER_STRIDE x RENDER_STRIDE tiles (renderer/mod.rs:84-90,
   * image_buffer.rs:48-97); this call renders the tiles with rt_tile_owner(tx, ty, n_ranks) == rank.
   * n_ranks <= 1 -> all tiles. */
  uint32_t tile_size; /* 0 -> 48 */
  uint32_t n_ranks;
  uint32_t rank;

  uint32_t traversal; /* RT_TRAVERSAL_* */

  rt_tuning tuning; /* all 0 = defaults */
} rt_params;

/* optional per-pixel debug planes for parity checks (all nullable, caller-owned, W*H each) */
typedef struct rt_aux {
  float* rgb;      /* [H*W][3] un-quantised linear RGB of written pixels (else untouched) */
  int32_t* hit_id; /* [H*W] canonical object index hit by the first sample's primary ray, -1 miss */
  float* hit_t;    /* [H*W] its distance (untouched on miss) */
} rt_aux;

typedef struct rt_stats {
  uint64_t rays_primary;    /* lanes entering cast_ray as camera rays  raytracer.rs:162 */
  uint64_t rays_reflection; /* ... as reflection children (raytracer_renderer.rs:698) */
  uint64_t rays_refraction; /* ... as refraction children (raytracer_renderer.rs:493) */
  uint64_t rays_shadow;     /* has_any_intersection calls, raytracer.rs:24 */
  uint64_t pixels_written;
  /* Rays actually traced on the GPU (nearest-hit searches).  rays_primary/reflection/refraction/shadow count what
   * the reference casts; AA samples whose origin offsets are bit-identical repeats of another sample (7 of 16 with
   * the deterministic table, 15 of 24 with extreme_quality: raytracer_renderer.rs:107-122,1111-1116) are traced once
   * and weighted by their multiplicity, so rays_traced <= the sum of the three.  CPU oracle: equal to the sum. */
  uint64_t rays_traced;
  double kernel_ms; /* device time of the render kernel(s) (CPU oracle: wall time) */
  double total_ms;  /* wall time of the call incl. copies */
  double d2h_ms;    /* rt_render / rt_render_multi: wall time of the device -> host copy of the packed pixels */
  double gather_ms; /* rt_render_multi: device time of the tile gather on the root (RCCL recv + scatter kernel) */
  /* The wave_* work statistics below are filled only by the statistics build of the library
   * (`make STATS=1` -> librt_hip_stats.so, used by tools/perf_ab.py); the shipped kernels leave them 0.
   * GPU only (0 from the CPU oracle): SIMD efficiency of the ray loop.  wave_ray_passes = number of
   * wavefront-level trips through cast_ray + shading; wave_ray_lanes = live lanes summed over those
   * trips.  lanes / (64 * passes) = fraction of the 64-wide machine doing useful ray work. */
  uint64_t wave_ray_passes;
  uint64_t wave_ray_lanes;
  /* GPU only: wavefront-level BVH work (one count per wave, not per lane) */
  uint64_t wave_nearest_nodes; /* BVH nodes fetched by nearest-hit traversals */
  uint64_t wave_nearest_tris;  /* triangle records tested by nearest-hit traversals */
  uint64_t wave_shadow_nodes;  /* same for shadow rays */
  uint64_t wave_shadow_tris;
  uint64_t wave_shadow_passes; /* wavefront-level shadow-ray traversals */
  uint64_t wave_nearest_tris_exact; /* triangle tests that passed the conservative pre-filter */
  uint64_t wave_shadow_tris_exact;
  /* RT_NOTE_* bits: fast paths this frame did NOT take, and why (the image is the same either way) */
  uint32_t notes;
  uint32_t reserved0;
  uint64_t queue_bytes; /* device memory the frame's ray queues, hard-pair queue and sort workspace hold (0 without secondary rays) */
  /* rt_render: device time between the start of the call's device work and its first render kernel -- sample-table uploads and, on
   * the first frame that needs them, rt_flags_kernel (receiver flags + per-cell lists).  NOT part of kernel_ms. */
  double setup_ms;
  uint64_t scene_bytes; /* device memory the scene handle holds in total right now (rt_scene_memory_info.bytes_total) */
} rt_stats;
#define RT_NOTE_RECV_FLAGS_OFF_LIGHTS 0x1u    /* receiver flags need n_lights <= 8 */
#define RT_NOTE_RECV_FLAGS_OFF_CULLING 0x2u   /* ... and no backface culling */
#define RT_NOTE_RECV_FLAGS_OFF_TRAVERSAL 0x4u /* ... and RT_TRAVERSAL_BVH */
#define RT_NOTE_RECV_FLAGS_OFF_TUNING 0x8u    /* switched off by rt_tuning (no_receiver_flags / shadow_candidate_cap) */
#define RT_NOTE_RECV_FLAGS_OFF_SCENE 0x10u    /* no receiver cells (no triangles / degenerate scene) or no light cloud */
#define RT_NOTE_HARD_PAIRS_OFF 0x20u          /* incoherent soft-shadow sets are traced inline (light_mult > 64, linear, cap) */
#define RT_NOTE_FRAME_BATCHED 0x40u           /* the ray queues did not fit: the frame ran in several primary batches */
#define RT_NOTE_CELL_LISTS_OFF 0x80u          /* no per-cell candidate lists (receiver flags off, > 65 533 leaf slots, over the scene's budget, tuning) */
#define RT_NOTE_TILE_ORDER_COST_OFF 0x100u    /* RT_TILE_ORDER_COST asked for, library built without the calibration kernel (make COST=1): row-major */
#define RT_NOTE_FRAME_DROPPED_WORK 0x200u     /* an asynchronously rendered frame of this shape overflowed a ray / pair queue (its counters came back
                                                 later): some of its secondary terms are missing; the queues have grown and the next frame is verified */

typedef struct rt_scene rt_scene; /* opaque: device copies + BVH */

/* the two ABI-spec hashes below are also called from the HIP kernels */
#if defined(__HIPCC__)
#define RT_HOSTDEV __host__ __device__
#else
#define RT_HOSTDEV
#endif

/* deterministic hash that selects the per-(pixel, light) cloud set; part of the ABI spec */
RT_HOSTDEV static inline uint32_t rt_cloud_hash(uint32_t seed, uint32_t pixel, uint32_t light) {
  uint32_t h = seed * 0x9E3779B1u;
  h ^= (pixel + 0x7F4A7C15u) * 0x85EBCA6Bu;
  h ^= (light + 0x165667B1u) * 0xC2B2AE35u;
  h ^= h >> 16;
  h *= 0x7FEB352Du;
  h ^= h >> 15;
  h *= 0x846CA68Bu;
  h ^= h >> 16;
  return h;
}

/* tile -> owning rank for multi-GPU interleaving; part of the ABI spec.  A lattice interleave
 * (tx + S*ty) mod n with S the smallest odd number >= 3 coprime to n: neighbouring tiles always
 * belong to different ranks, so spatial cost hot-spots (glass sphere vs background) spread evenly,
 * and every rank owns the same number of tiles +-1 per row. */
RT_HOSTDEV static inline uint32_t rt_tile_owner(uint32_t tile_x, uint32_t tile_y, uint32_t n_ranks) {
  if (n_ranks <= 1u) return 0u;
  uint32_t s = 3u;
  for (;;) {
    uint32_t a = s, b = n_ranks;
    while (b) {
      uint32_t t = a % b;
      a = b;
      b = t;
    }
    if (a == 1u) break;
    s += 2u;
  }
  return (tile_x + s * tile_y) % n_ranks;
}

/* ---- entry points --------------------------------------------------------------------------- */

/* number of HIP devices visible (0 if none); never fails */
int rt_device_count(void);

/* Uploads the scene to `device`, builds the triangle BVH.  Caller keeps ownership of all host
 * arrays (they may be freed after the call returns). */
int rt_scene_create(const rt_scene_desc* desc, int device, rt_scene** out);

/* Renders into a HOST buffer of width*height packed 0xFFRRGGBB pixels.  Only pixels whose ray
 * hit something are written (miss pixels keep the caller's fill, image_buffer.rs:27-37).
 * Blocks until the buffer is complete.  aux/stats may be NULL; aux pointers are HOST pointers. */
int rt_render(rt_scene* scene, const rt_params* params, uint32_t* argb, const rt_aux* aux,
              rt_stats* stats);

/* Same, but `argb_dev` (and aux pointers) are DEVICE pointers on the scene's device and all work
 * is enqueued on `hip_stream` (a hipStream_t, NULL = default stream).  Without reflections /
 * refractions this is one asynchronous kernel launch; with them the call enqueues the launches of
 * every ray-streaming level and returns: a frame of a verified shape is a burst of launches that
 * does not wait for the GPU.  The call blocks until earlier work has finished only
 *  - on the first frame of a shape (its counters are read back to verify the queue sizes), and while
 *    it renders that frame again after its queues grew;
 *  - on the frame after one that dropped work (the shape is verified again);
 *  - when a parameter table (AA offsets, light clouds, receiver flags, tile list) is uploaded while
 *    frames that read the old one are in flight;
 *  - when a scene switches from two chains to one (rt_tuning.sub_frames) and frees the second's queues;
 *  - on the calibration frame of RT_TILE_ORDER_COST (once per frame shape).
 * Ray counters: after the caller has synchronised, rt_render_collect_stats (those of the frame
 * enqueued last).
 * Consecutive frames of one scene may be enqueued on DIFFERENT streams: the library orders what they share (four
 * frame slots, each a counter block and, with secondary rays, a workspace set; a frame waits on the device for the
 * frame that used its slot last), so two frames overlap -- the head of one fills the compute units the drain of the
 * other leaves idle. */
int rt_render_device(rt_scene* scene, const rt_params* params, uint32_t* argb_dev,
                     const rt_aux* aux_dev, void* hip_stream);
int rt_render_collect_stats(rt_scene* scene, rt_stats* stats);

void rt_scene_destroy(rt_scene* scene);

/* ---- progressive read-back: the frame lands in the caller's buffer band by band WHILE it is being rendered ----------------
 *
 * Reference: main() spawns a thread that calls render(&buffer, &scene) and meanwhile blits the same buffer in its window loop
 * (src/main.rs:327-347); the buffer is [AtomicU32], written tile by tile with relaxed stores and read with relaxed loads
 * (src/image_buffer.rs:39-44,243-250).  Here `begin` starts the library's own render thread: the frame (or params' window) is
 * rendered in bands of `band_rows` rows (0 = tile_size, one row of RENDER_STRIDE tiles: renderer/mod.rs:84-90) on a stream of
 * its own, every finished band is copied to pinned host memory, and a counter says how many rows have landed.  `poll` -- the
 * UI thread's side; it never blocks -- copies the rows that are new since the last poll into `argb` and reports the count; rows
 * [win_y0, win_y0 + rows_done) of `argb` are then final, the rows below still hold the caller's fill.  `end` waits for the
 * rest, hands it over and frees the handle; its stats are summed over the bands.  `argb` (HOST, W*H, pre-filled by the caller)
 * must stay valid until `end`; params and its tables are copied by `begin`.  One progressive render per scene at a time, and no
 * other render call on that scene until `end`.  The final buffer equals rt_render's. */
typedef struct rt_progress rt_progress;
int rt_render_begin(rt_scene* scene, const rt_params* params, uint32_t* argb, uint32_t band_rows, rt_progress** out);
int rt_render_poll(rt_progress* progress, uint32_t* rows_done, int* finished);
int rt_render_end(rt_progress* progress, rt_stats* stats);

/* ---- ray queries on a scene already on the device ------------------------------------------------------------------------
 *
 * One ray per element; the reference's Ray::new_with_mask normalises the direction (ray.rs:52-57), and so do these calls:
 * `direction` may have any length, `t` is the distance along the normalised direction.  Hit ids are canonical object
 * indices as everywhere in this ABI (spheres, then triangles, each in insertion order).
 *
 * cast_ray's `start_refraction_index` and IS_ANTIALIASING_RAY do not take part in which object is hit (they only travel
 * with the ray for the shading after it), so they have no counterpart here.
 *
 * Dead rays (deviation D2 of the render): a direction that normalises to NaN (zero length, a NaN or inf component) or a
 * non-finite origin is a miss, and for rt_any_intersection* "has_intersection 0, completely_occluded 0, combined_opacity
 * 1.0, color_filter (1, 1, 1)".  A NaN or negative max_distance admits no hit.
 *
 * Validation (RT_ERR_INVALID_ARG + rt_last_error, before any HIP call): NULL scene, batch or output struct; wrong
 * abi_version; a flag bit other than RT_FLAG_BACKFACE_CULLING; NULL origin / direction with n_rays > 0; every output
 * plane NULL.
 *
 * A query reads only the scene's data, which no render writes: it may run on any stream while frames of the same scene
 * render on others (rt_render_begin's included), and it leaves every render state alone.  (rt_scene_update* is the one
 * call that rewrites that data: a query still in flight must have finished before it.) */
typedef struct rt_ray_batch {
  uint32_t abi_version;       /* RT_ABI_VERSION */
  uint32_t n_rays;            /* 0 is a valid no-op */
  const float* origin;        /* [n_rays][3] */
  const float* direction;     /* [n_rays][3], any length (normalised as Ray::new_with_mask does, ray.rs:52-57) */
  const float* max_distance;  /* [n_rays], rt_any_intersection* and rt_list_intersections* (raytracer.rs:28); NULL = +inf;
                                 rt_cast_rays* ignores it */
  uint32_t flags;             /* RT_FLAG_BACKFACE_CULLING or 0 (sphere.rs:137-151, triangle.rs:154-168) */
} rt_ray_batch;

/* nearest hit per ray (cast_ray).  Every member nullable: a NULL plane is not written. */
typedef struct rt_ray_hits {
  int32_t* id;        /* canonical object index of the nearest valid hit, -1 on a miss; on equal t the LATER object wins
                         (the simd_le of raytracer.rs:194) */
  float* t;           /* distance along the normalised direction; +inf on a miss */
  float* point;       /* [n][3] fma(d, t, o) (Ray::at, ray.rs:60-66); 0 on a miss */
  float* normal;      /* [n][3] sphere: normalize(p - centre); triangle: its stored face normal; 0 on a miss */
  uint32_t* material; /* material row; 0xFFFFFFFF on a miss */
} rt_ray_hits;

/* visibility / transmittance per segment (has_any_intersection).  Every member nullable. */
typedef struct rt_ray_occlusion {
  uint8_t* has_intersection;    /* some valid hit at t <= max_distance (raytracer.rs:53-55) */
  uint8_t* completely_occluded; /* one of those hits is on a material without opacity (raytracer.rs:75-80) */
  float* combined_opacity;      /* 0 if occluded, else max(0, 1 - sum(1 - io)) over the hits, summed in 2^-28 fixed point
                                   (independent of the order the hits are found in) */
  float* color_filter;          /* [n][3] 1 - sum(absorption) over the hits (2^-24 fixed point) for a ray that is NOT
                                   occluded.  UNSPECIFIED for an occluded ray: the reference stops at its first opaque hit in
                                   object order, and nothing reads the filter after that */
} rt_ray_occlusion;

/* HOST arrays: the batch is copied through device memory allocated for the call (and freed); returns when the results
 * are in host memory. */
int rt_cast_rays(rt_scene* scene, const rt_ray_batch* batch, const rt_ray_hits* hits);
int rt_any_intersection(rt_scene* scene, const rt_ray_batch* batch, const rt_ray_occlusion* out);
/* DEVICE arrays on the scene's device: enqueued on `hip_stream` (a hipStream_t, NULL = default stream); allocates
 * nothing and returns once the work is enqueued. */
int rt_cast_rays_device(rt_scene* scene, const rt_ray_batch* batch, const rt_ray_hits* hits, void* hip_stream);
int rt_any_intersection_device(rt_scene* scene, const rt_ray_batch* batch, const rt_ray_occlusion* out, void* hip_stream);

/* ---- closest-point queries: the nearest point of the scene's surface per query point -----------------------------------------
 *
 * The third query on a scene that is already on the device (Embree's rtcPointQuery, Open3D's compute_closest_points): for each
 * point p, the object whose SURFACE comes nearest, the nearest point q on it and the distance |q - p|.  It works on whatever
 * the handle holds after rt_scene_update*, rt_pose_apply*, rt_skin_apply* and rt_scene_rebuild*.
 *
 * Definition (csrc/rt_closest.h holds the formulas; every float operation is a single correctly rounded one):
 *   triangle  the nearest of four candidates relative to p (v1 - p is formed first): the clamped projections onto its three
 *             edges and, where it falls inside, the projection onto its plane.  Finite for every triangle with finite vertices:
 *             a zero-area triangle is its longest segment, three equal vertices are that point, and no candidate divides by
 *             zero.  A triangle farther than 1.8e19 from p overflows its squared distance and never wins.
 *   sphere    r = sqrt(r_sq); distance | |p - c| - r |, point c + (p - c) (r / |p - c|); for p == c the direction is (1, 0, 0).
 *   Both are surfaces, not solids: inside and outside are treated alike, and there is no sign.
 * One fp32 distance per object.  The smaller distance wins; on EQUAL distance the LARGER canonical id wins (spheres, then
 * triangles, each in insertion order: the "later object wins" of rt_cast_rays).  The result is therefore a function of the
 * scene description and the point alone, not of the tree or of the order a walk meets candidates in.  An object counts only
 * when its distance <= max_distance (the test is <=; a NaN or negative max_distance admits nothing; NULL = +inf).
 *
 * Dead queries: a point with a non-finite coordinate is a miss.  A miss returns id -1, distance +inf, point, normal and bary 0,
 * material 0xFFFFFFFF, as rt_ray_hits does.
 *
 * Validation (RT_ERR_INVALID_ARG + rt_last_error, before any HIP call): NULL scene (or description), batch or output struct;
 * wrong abi_version; NULL point with n_points > 0; every output plane NULL.
 *
 * A query reads only the scene's data: it may run on any stream beside renders and ray queries of the same scene, and must
 * have finished before rt_scene_update* / rt_scene_rebuild* (and the pose and skin calls, which update), exactly as the ray
 * queries.
 *
 * Signed distance and inside tests: rt_signed_distance* and rt_contains_points* below.  Not offered: the k nearest objects, a
 * walk shared by the wavefront for coherent point sets such as grids, and an ordered variant. */
typedef struct rt_point_batch {
  uint32_t abi_version;      /* RT_ABI_VERSION */
  uint32_t n_points;         /* 0 is a valid no-op */
  const float* point;        /* [n_points][3] */
  const float* max_distance; /* [n_points] search radius; NULL = +inf */
} rt_point_batch;

/* nearest surface point per query point.  Every member nullable, at least one non-NULL: a NULL plane is not written. */
typedef struct rt_point_hits {
  int32_t* id;        /* canonical object index, -1 on a miss */
  float* distance;    /* |q - p| as defined above; +inf on a miss */
  float* point;       /* [n][3] q; 0 on a miss */
  float* normal;      /* [n][3] sphere: normalize(q - c), computed as (p - c) / |p - c|; triangle: its stored face normal; 0 on a miss */
  float* bary;        /* [n][2] weights of e1 and e2 at q (q = v1 + bary0 e1 + bary1 e2 up to rounding); 0 for spheres and misses */
  uint32_t* material; /* material row; 0xFFFFFFFF on a miss */
} rt_point_hits;

/* HOST arrays: staged through device memory allocated for the call; returns when the results are in host memory. */
int rt_closest_points(rt_scene* scene, const rt_point_batch* batch, const rt_point_hits* hits);
/* DEVICE arrays on the scene's device: enqueued on `hip_stream` (NULL = default stream); allocates nothing. */
int rt_closest_points_device(rt_scene* scene, const rt_point_batch* batch, const rt_point_hits* hits, void* hip_stream);
/* The specification, without a device or a tree: a LINEAR scan of `desc` with the same arithmetic.  HOST arrays; no HIP call.
 * The two calls above return the same bits. */
int rt_closest_points_model(const rt_scene_desc* desc, const rt_point_batch* batch, const rt_point_hits* hits);

/* ---- multi-hit ray queries: the first K hits of each ray, and how many there are ------------------------------------------------
 *
 * Everything a ray passes through (Open3D's list_intersections / count_intersections, Embree's multi-hit, trimesh's
 * multiple_hits): thickness and x-ray probes, layered picking, transparency ordering, crossing counts.  The call works on
 * whatever the handle holds after rt_scene_update*, rt_pose_apply*, rt_skin_apply* and rt_scene_rebuild*.
 *
 * Definition (csrc/rt_multihit.h holds the formulas).  `batch` is an rt_ray_batch as above, max_distance honoured.  A HIT is
 * what the reference's `intersect` returns for one object, so at most one per object: for a sphere the root
 * SphereData::intersect picks (a ray from outside gets the entry point only), for a triangle the literal matrix-inverse test;
 * RT_FLAG_BACKFACE_CULLING applies sphere.rs:137-151 / triangle.rs:154-168 exactly as rt_cast_rays does.  A hit counts when
 * t <= max_distance as computed (NULL = +inf; a NaN or negative max_distance admits nothing; a NaN t never counts).
 *
 * Order and cursor.  Hits are ordered by the key (t ascending; on equal t the LARGER canonical id first): the "later object
 * wins" of rt_cast_rays, so entry 0 of every list is rt_cast_rays' answer bit for bit.  The optional cursor (after_t[i],
 * after_id[i]) admits only keys strictly after it: t > after_t, or t == after_t and id < after_id; a NaN after_t admits
 * nothing.  Feeding the last returned key back pages through all hits with no epsilon and without losing or repeating
 * coincident hits.
 *
 * Output per ray for max_hits = K: `count` entries (0 .. K) in row i of each plane [n][K]; entries from `count` on hold the
 * miss values of rt_ray_hits (id -1, t +inf, point and normal 0, material 0xFFFFFFFF).  `total` is the number of distinct
 * objects with an admitted hit, which may exceed K: count == min(total, K).  Asking for `total` makes a ray whose list came
 * back full walk again behind its last key until it has counted everything; a ray with fewer than K hits costs one walk either
 * way.  Dead rays (see above) give count 0 and total 0.
 *
 * The result is a function of the scene description and the ray alone: it does not depend on the tree, on slot order, on
 * split-clipped duplicate references or on the order a walk meets hits in.
 *
 * Validation (RT_ERR_INVALID_ARG + rt_last_error, before any HIP call; nothing is written): as the ray queries, and max_hits
 * outside 1 .. RT_MAX_HITS_PER_RAY; exactly one of after_t / after_id NULL; every output NULL.
 *
 * Streams and concurrency: as the ray queries above.
 *
 * Inside / occupancy tests and signed distance: rt_contains_points* and rt_signed_distance* below (a sphere gives one hit, so
 * crossing parity has a definition of its own).  Not offered: both roots of a sphere, K above RT_MAX_HITS_PER_RAY, an ordered
 * or wave-cooperative variant. */
#define RT_MAX_HITS_PER_RAY 16u

/* request and output of rt_list_intersections*.  Every output member nullable, at least one non-NULL: a NULL plane is not written. */
typedef struct rt_ray_hit_lists {
  uint32_t max_hits;       /* K: 1 .. RT_MAX_HITS_PER_RAY entries per ray */
  const float* after_t;    /* [n] cursor: only keys strictly after (after_t, after_id) are admitted; both NULL = from the start */
  const int32_t* after_id; /* [n] */
  uint32_t* count;         /* [n] entries written for the ray, 0 .. K */
  uint32_t* total;         /* [n] distinct objects with an admitted hit (>= count) */
  int32_t* id;             /* [n][K] canonical object index; -1 from `count` on */
  float* t;                /* [n][K] distance along the normalised direction; +inf from `count` on */
  float* point;            /* [n][K][3] fma(d, t, o); 0 from `count` on */
  float* normal;           /* [n][K][3] sphere: normalize(p - centre); triangle: its stored face normal; 0 from `count` on */
  uint32_t* material;      /* [n][K] material row; 0xFFFFFFFF from `count` on */
} rt_ray_hit_lists;

/* HOST arrays: staged through device memory allocated for the call; returns when the results are in host memory. */
int rt_list_intersections(rt_scene* scene, const rt_ray_batch* batch, const rt_ray_hit_lists* lists);
/* DEVICE arrays on the scene's device: enqueued on `hip_stream` (NULL = default stream); allocates nothing. */
int rt_list_intersections_device(rt_scene* scene, const rt_ray_batch* batch, const rt_ray_hit_lists* lists, void* hip_stream);
/* The specification, without a device or a tree: a LINEAR scan of `desc` with the same arithmetic.  HOST arrays; no HIP call.
 * The two calls above return the same bits. */
int rt_list_intersections_model(const rt_scene_desc* desc, const rt_ray_batch* batch, const rt_ray_hit_lists* lists);

/* ---- ambient-occlusion queries: hemisphere visibility per surface point ----------------------------------------------------------
 *
 * How open the surface is at a point: ambient occlusion, sky visibility and bent normals, for baking per vertex or texel,
 * contact shading, accessibility of a point on a part (Embree's rtcOccluded over a hemisphere; Open3D's and trimesh's
 * occlusion bakes).  The points and normals that rt_cast_rays* and rt_closest_points* return plug in directly.  The rays are
 * made on the device, each stops at its first hit, a point's samples are reduced inside a wavefront and one record per point
 * is written.  The call works on whatever the handle holds after rt_scene_update*, rt_pose_apply*, rt_skin_apply* and
 * rt_scene_rebuild*.
 *
 * Definition (csrc/rt_occlusion.h holds the formulas; every float result is one correctly rounded operation or an fmaf).
 * Per point: n = normalize(normal); the point is DEAD if a coordinate of it is non-finite or n has a NaN.  The frame is the
 * branchless orthonormal basis of Duff et al. 2017 (tx, ty, n); the origin is fma(n, bias, point).  Sample s takes table row
 * ((uint64)first[i] + s) % n_table (first NULL: 0), a direction l in the LOCAL frame (z along the normal, any length); the
 * world direction is l.x tx + l.y ty + l.z n and is normalised as every ray's is (u).  A sample is OCCLUDED if some object has
 * a hit -- what rt_list_intersections defines, at most one per object, no back-face culling -- with t <= max_distance (a NaN
 * or negative max_distance admits nothing; +inf is allowed).  With RT_OCCLUSION_PASS_TRANSMISSIVE objects whose material is
 * transmissive (TransmissionProperties::mask) do not count.  A sample whose ray is dead (its row normalises to NaN, the
 * origin overflowed) counts as occluded: a ray that cannot be cast shows no open sky.
 *
 * Output per point, for n_samples = S: bits[(S + 31) / 32] -- bit s % 32 of word s / 32 is set when sample s is occluded, the
 * unused high bits are 0; clear = the samples that are not occluded; visibility = clear / S; bent_normal = the normalised sum
 * of the unit directions u of the clear samples, summed in 2^-20 fixed point (int32, so the sum has no order), or (0, 0, 0)
 * when the three sums are 0.  A dead point: bits all set, clear 0, visibility 0, bent_normal 0.
 *
 * The result is a function of the scene description and the batch alone: it does not depend on the tree, on slot order, on
 * split-clipped duplicate references, on how samples map to lanes or on the order a walk meets hits in.
 *
 * Validation (RT_ERR_INVALID_ARG + rt_last_error, before any HIP call; nothing is written): a NULL scene, description, batch
 * or out; a wrong abi_version; NULL point, normal or table with n_points > 0; n_samples outside 1 ..
 * RT_MAX_OCCLUSION_SAMPLES; n_table == 0; a non-finite bias; a flag bit other than RT_OCCLUSION_PASS_TRANSMISSIVE; every
 * output NULL.  n_points == 0 is a valid no-op.
 *
 * Streams and concurrency: as the ray queries above.
 *
 * Not offered: per-sample weights, transmittance-weighted occlusion, culling, distance falloff, a max_distance per point,
 * more than RT_MAX_OCCLUSION_SAMPLES samples in a call (the caller pages through a longer table with `first`). */
#define RT_MAX_OCCLUSION_SAMPLES 256u
#define RT_OCCLUSION_PASS_TRANSMISSIVE 0x1u /* rt_occlusion_batch.flags: transmissive objects do not occlude */

typedef struct rt_occlusion_batch {
  uint32_t abi_version;   /* RT_ABI_VERSION */
  uint32_t n_points;      /* 0 is a valid no-op */
  const float* point;     /* [n_points][3] */
  const float* normal;    /* [n_points][3], any length */
  uint32_t n_samples;     /* S: 1 .. RT_MAX_OCCLUSION_SAMPLES samples per point */
  uint32_t n_table;       /* rows of `table`, >= 1 */
  const float* table;     /* [n_table][3] directions in the local frame (z along the normal), any length */
  const uint32_t* first;  /* [n_points] table row of sample 0, any value (taken modulo n_table); NULL = 0 */
  float bias;             /* the origin is moved this far along the normal; finite */
  float max_distance;     /* hits at t <= max_distance occlude; +inf allowed */
  uint32_t flags;         /* RT_OCCLUSION_PASS_TRANSMISSIVE or 0 */
} rt_occlusion_batch;

/* output of rt_ambient_occlusion*.  Every member nullable, at least one non-NULL: a NULL plane is not written. */
typedef struct rt_occlusion_out {
  uint32_t* bits;      /* [n_points][(S + 31) / 32] occluded samples */
  uint32_t* clear;     /* [n_points] samples that are not occluded, 0 .. S */
  float* visibility;   /* [n_points] clear / S */
  float* bent_normal;  /* [n_points][3] unit, or 0 */
} rt_occlusion_out;

/* HOST arrays: staged through device memory allocated for the call; returns when the results are in host memory. */
int rt_ambient_occlusion(rt_scene* scene, const rt_occlusion_batch* batch, const rt_occlusion_out* out);
/* DEVICE arrays on the scene's device, the table included: ONE launch enqueued on `hip_stream` (NULL = default stream);
 * allocates nothing, needs no workspace, returns once the work is enqueued. */
int rt_ambient_occlusion_device(rt_scene* scene, const rt_occlusion_batch* batch, const rt_occlusion_out* out, void* hip_stream);
/* The specification, without a device or a tree: a LINEAR scan of `desc` with the same arithmetic.  HOST arrays; no HIP call.
 * The two calls above return the same bits. */
int rt_ambient_occlusion_model(const rt_scene_desc* desc, const rt_occlusion_batch* batch, const rt_occlusion_out* out);
/* The rays of the definition (no device needed), every output nullable: origin [n_points][3]; direction [n_points][S][3], the
 * world direction of each sample BEFORE normalisation (a ray batch of these origins and directions is normalised exactly as
 * the query normalises them); alive [n_points], 0 for a dead point. */
int rt_occlusion_rays_model(const rt_occlusion_batch* batch, float* origin, float* direction, uint8_t* alive);

/* ---- containment and signed-distance queries for closed surfaces -------------------------------------------------------------------
 *
 * "Is this point inside something, and how deep?" (trimesh's contains / signed_distance, Open3D's occupancy and SDF grids), on
 * whatever the handle holds after rt_scene_update*, rt_pose_apply*, rt_skin_apply* and rt_scene_rebuild*: collision and
 * voxelisation loops against the current pose without a host round trip.
 *
 * Definition (csrc/rt_solid.h holds the formulas; every float result is one correctly rounded operation or an fmaf).  A batch
 * is n points, a table of R = n_directions rows (1 .. RT_MAX_SOLID_DIRECTIONS, any length; a HOST array in every entry point:
 * it is validated and passed to the kernel by value) and a rule.  Per point p and direction r a ray is cast from p along row
 * r, normalised as every ray's direction is, without bias and without max_distance.  A CROSSING is a triangle the ray hits as
 * rt_list_intersections defines a hit (the literal test, no culling, transmissive objects included).
 *   crossings[i][r]  the number of distinct triangles crossed
 *   winding[i][r]    the sum over the crossings of the sign of dot(direction, stored normal): +1 where the ray leaves through
 *                    the triangle, -1 where it enters, 0 for a zero or NaN product.  The orientation is the stored normal's,
 *                    never the vertex order's.
 *   spheres          are decided analytically: a sphere contains p when |p - c|^2 - r_sq < 0 as the sphere test computes it (a NaN
 *                    or negative r_sq never contains); k_s = the number of containing spheres.
 *   the vote of r    RT_SOLID_RULE_PARITY: (crossings + k_s) & 1;  RT_SOLID_RULE_WINDING: winding + k_s > 0.
 *   votes[i] = the directions voting inside; inside[i] = 2 votes > R.  R odd is recommended; a tie at an even R is outside.
 * The rules differ where solids overlap: in the intersection of two boxes parity says outside, winding says inside.
 *
 * Open and inconsistent surfaces get a defined, diagnosable answer, not a refusal: votes not in {0, R} means the directions
 * disagree -- the point lies on or near a surface, or the surface is open or inconsistently oriented there.  (The letters of the
 * built-in text meshes are open surfaces; this is how they show.)
 *
 * Dead points: a point with a non-finite coordinate gets inside 0, votes 0, crossings 0, winding 0.
 *
 * Signed distance: rt_closest_points' result for the point, unchanged bit for bit, every plane of it available, and
 * signed_distance = inside ? -distance : distance (a miss is +inf or -inf).  max_distance applies to the closest-point search
 * only; rt_contains_points* ignore it.
 *
 * The result is a function of the scene description and the batch alone: it does not depend on the tree, on slot order or on the
 * order a walk meets crossings in.
 *
 * Split-clipped trees (rt_bvh_tuning.split_depth > 0; off by default) are refused with RT_ERR_UNSUPPORTED, as rt_scene_update
 * and rt_scene_rebuild refuse them: every reference of such a triangle evaluates the whole triangle, so a counting walk would
 * count it once per reference reached.
 *
 * Validation (RT_ERR_INVALID_ARG + rt_last_error, before any HIP call; nothing is written): a NULL scene, description, batch or
 * out; a wrong abi_version; NULL point with n_points > 0; NULL directions; n_directions outside 1 .. RT_MAX_SOLID_DIRECTIONS;
 * a row that does not normalise to finite components, not all zero (a zero, NaN or infinite row, one whose squared length under-
 * or overflows); an unknown rule; every output NULL.
 * n_points == 0 is a valid no-op.
 *
 * Streams and concurrency: as the ray queries above.
 *
 * Not offered: generalized winding numbers, a watertight triangle test, split-clipped trees, per-object containment ids, a flag
 * that skips transmissive objects, the k nearest objects. */
#define RT_MAX_SOLID_DIRECTIONS 8u
#define RT_SOLID_RULE_PARITY 0u
#define RT_SOLID_RULE_WINDING 1u

typedef struct rt_solid_batch {
  uint32_t abi_version;       /* RT_ABI_VERSION */
  uint32_t n_points;          /* 0 is a valid no-op */
  const float* point;         /* [n_points][3] */
  const float* max_distance;  /* [n_points] search radius of the closest-point part of rt_signed_distance*; NULL = +inf */
  uint32_t n_directions;      /* R: 1 .. RT_MAX_SOLID_DIRECTIONS */
  uint32_t rule;              /* RT_SOLID_RULE_PARITY or RT_SOLID_RULE_WINDING */
  const float* directions;    /* [R][3] HOST array in every entry point, any length */
} rt_solid_batch;

/* output of rt_contains_points*.  Every member nullable, at least one non-NULL: a NULL plane is not written. */
typedef struct rt_solid_out {
  uint8_t* inside;     /* [n_points] 0 or 1 */
  uint8_t* votes;      /* [n_points] directions voting inside, 0 .. R */
  uint32_t* crossings; /* [n_points][R] */
  int32_t* winding;    /* [n_points][R] */
} rt_solid_out;

/* output of rt_signed_distance*.  Every member nullable, at least one non-NULL: a NULL plane is not written. */
typedef struct rt_signed_distance_out {
  float* signed_distance; /* [n_points] inside ? -distance : distance */
  rt_solid_out solid;     /* as rt_contains_points */
  rt_point_hits closest;  /* as rt_closest_points */
} rt_signed_distance_out;

/* HOST arrays: staged through device memory allocated for the call; returns when the results are in host memory. */
int rt_contains_points(rt_scene* scene, const rt_solid_batch* batch, const rt_solid_out* out);
int rt_signed_distance(rt_scene* scene, const rt_solid_batch* batch, const rt_signed_distance_out* out);
/* DEVICE arrays on the scene's device (points, max_distance and every output; the direction table stays a HOST array): enqueued
 * on `hip_stream` (NULL = default stream); allocates nothing.  rt_signed_distance_device enqueues the closest-point kernel and
 * then the containment kernel, which reads the distance plane; it needs no plane beyond those asked for (without
 * closest.distance the unsigned distance travels in the signed_distance plane itself). */
int rt_contains_points_device(rt_scene* scene, const rt_solid_batch* batch, const rt_solid_out* out, void* hip_stream);
int rt_signed_distance_device(rt_scene* scene, const rt_solid_batch* batch, const rt_signed_distance_out* out, void* hip_stream);
/* The specification, without a device or a tree: a LINEAR scan of `desc` with the same arithmetic.  HOST arrays; no HIP call.
 * The calls above return the same bits. */
int rt_contains_points_model(const rt_scene_desc* desc, const rt_solid_batch* batch, const rt_solid_out* out);
int rt_signed_distance_model(const rt_scene_desc* desc, const rt_solid_batch* batch, const rt_signed_distance_out* out);

/* ---- radiance queries: Whitted shading of caller-supplied rays -------------------------------------------------------------
 *
 * The colour of each ray, as the render computes it for its camera rays:
 *   single_raytrace(origin, direction, air_ior, objects, lights, depth None).0 -- raytracer_renderer.rs:147-264.
 * Ray i plays the role of pixel i wherever the render uses the pixel index: its light-cloud set is
 * rt_cloud_hash(cloud_seed, i, light) % n_cloud_sets.  Its weight is 1: the result is what a frame without anti-aliasing writes
 * to rt_aux.rgb for a pixel whose camera ray is that ray.  Dead rays follow the query rule above (a miss; not counted).
 *
 * `batch`: rt_ray_batch as above; max_distance must be NULL and flags 0 (culling comes from shading->flags).
 * `shading`: an rt_params of which fw, fh, fd, eps_distance, air_ior, ambient, flags, light_mult, cloud_seed, n_cloud_sets,
 * cloud_sets, max_depth_*, traversal and tuning are read.  flags may carry REFLECTIONS, REFRACTIONS and BACKFACE_CULLING;
 * RT_FLAG_ANTI_ALIASING is refused (the caller supplies its samples as rays).  The camera members (width, height, focus,
 * aa_*, win_*, tile_size, n_ranks, rank) are ignored: a caller can pass the params it renders with, minus the AA bit.
 * tuning.levels, tuning.phases, tuning.tile_order and tuning.no_aa_dedup are ignored too: a batch with secondary rays always
 * runs the chained level schedule with fused phases (the other forms derive the camera ray from the work-item index).
 *
 * Order matters for speed, not for the result: the walks are wave-cooperative (64 consecutive rays share one), so
 * neighbouring rays of a batch should be neighbours in space.  These two calls do not reorder the caller's rays;
 * rt_trace_rays_ordered* (below) read the batch through a permutation built on the device, with the same results.
 *
 * rt_stats (host form; device form: rt_render_collect_stats after synchronising): rays_primary = live rays,
 * rays_reflection / rays_refraction / rays_shadow as the reference casts them, pixels_written = valid rays, rays_traced =
 * the sum of the three ray kinds (nothing is deduplicated).
 *
 * Validation (RT_ERR_INVALID_ARG + rt_last_error, before any HIP call): NULL scene, shading, batch or output struct; wrong
 * abi_version in either struct; max_distance or batch flags set; RT_FLAG_ANTI_ALIASING; NULL origin / direction with
 * n_rays > 0; every output plane NULL; and what rt_render rejects in an rt_params (clouds, depths, tuning ranges, secondary
 * flags with depth 0).  At most 2^31 - 1 rays.  n_rays == 0 is a valid no-op.
 *
 * A radiance call is a RENDER call: it uses the scene's parameter tables, frame slots and workspaces.  One such call per
 * scene at a time, as for rt_render; refused while rt_render_begin owns the scene.
 * Blocking: without REFLECTIONS / REFRACTIONS rt_trace_rays_device is ONE asynchronous kernel launch and allocates nothing
 * (a changed light-cloud table is uploaded first, as by rt_render_device).  With them it enqueues the chained levels and
 * then BLOCKS until the batch is through: ray counts do not repeat from batch to batch as they do from frame to frame, so
 * every batch is verified -- its counters are read back, and if a ray or pair queue dropped anything the queues grow and
 * the batch runs again (rt_stats.queue_bytes shows the growth).  It allocates the accumulator (32 bytes per ray), the
 * queues, and an argb plane of its own when the caller gives none.  A camera frame that follows a batch verifies its queue
 * sizes afresh. */
typedef struct rt_ray_radiance {
  float* rgb;     /* [n][3] un-quantised linear RGB; (0,0,0) on a miss */
  uint8_t* valid; /* [n] 1 = the ray hit something (single_raytrace's valid mask) */
  int32_t* id;    /* [n] canonical object index of the primary hit, -1 on a miss */
  float* t;       /* [n] its distance, +inf on a miss (as rt_ray_hits.t) */
  uint32_t* argb; /* [n] packed 0xFFRRGGBB (OutputColorEncoder::to_output); UNTOUCHED on a miss, as rt_render */
} rt_ray_radiance; /* every member nullable, at least one non-NULL */

/* HOST arrays: staged through one device allocation made for the call, on a stream of its own; returns when the results
 * are in host memory.  stats may be NULL. */
int rt_trace_rays(rt_scene* scene, const rt_params* shading, const rt_ray_batch* batch, const rt_ray_radiance* out, rt_stats* stats);
/* DEVICE arrays on the scene's device, enqueued on `hip_stream` (a hipStream_t, NULL = default stream). */
int rt_trace_rays_device(rt_scene* scene, const rt_params* shading, const rt_ray_batch* batch, const rt_ray_radiance* out,
                         void* hip_stream);

/* ---- ray orders: coherent wavefronts for radiance queries, sorted on the device ----------------------------------------------
 *
 * An rt_ray_order is a permutation of one batch's rays (and the workspace that builds it) on one device.  The ordered
 * radiance calls read the batch THROUGH it: wavefront w works on rays perm[64 w .. 64 w + 63] instead of rays 64 w ..
 * 64 w + 63, so that rays which are neighbours in space share the wave-cooperative walks.
 *
 * Results: an ordered call returns exactly what rt_trace_rays[_device] returns for the same batch, whatever the order is
 * -- every plane bit for bit, argb untouched on a miss, every rt_stats counter, the same validation and blocking rules.
 * Ray identity: ray i remains ray i.  Its light-cloud set (keyed by i), its accumulator entry and its output index do not
 * move; only which 64 rays share a wavefront changes.  (A caller who permutes its own arrays instead changes the cloud
 * set of every ray, and with it the soft-shadow result.)
 *
 * rt_ray_order_build* sorts the rays by a key made of the batch alone: the Morton code of origin and normalised
 * direction, quantised inside the bounds of the batch's live rays, origins first.  Each origin axis on which the rays
 * differ gets `origin_bits` bits (0 = default: min(10, 30 / number of such axes), but 5 when all three origin axes and
 * some direction axis differ -- unrelated rays in a volume, where 5 + 5 measured fastest), each such direction axis
 * min(10, (30 - origin bits in all) / number of such axes); dead rays (the query rule) get key 0xFFFFFFFF and come last.
 * The major part of the key (the origins; the directions of a batch with one origin) is not a Morton code all the way up:
 * its cells form blocks of about 4096 rays that follow one another row-major, with the Morton code inside a block -- a
 * camera batch walked in nested squares traced slower than in rows of blocks.
 * Rays of equal key follow one another in an unspecified order.  The key is specified by a host model compiled from the
 * same source as the kernels (csrc/rt_ray_key.h); rt_ray_order_read returns the device's keys.
 *
 * Not tied to a scene: the key uses only the batch, so an order stays valid across rt_scene_update*, may be used with any
 * scene on its device, and may be reused for any batch of the same n_rays -- it is as good as the rays are similar to
 * the ones it was built from.
 *
 * Refused with RT_ERR_INVALID_ARG (+ rt_last_error) before any HIP call: a NULL pointer or wrong abi_version; capacity 0 or above
 * 2^27 = 134 217 728 rays; origin_bits > 10; n > capacity; an order whose n_rays differs from batch->n_rays, that lives on another device than the
 * scene, or that has never been built or set; an rt_ray_order_set array that is not a permutation of [0, n).
 *
 * Stream ordering is the caller's: rt_ray_order_build_device and a trace that reads the order run on the same stream, or
 * are ordered with events.  rt_ray_order_destroy waits for the last build; traces still in flight that read the order are
 * the caller's to finish first (the queries' rule).
 *
 * rt_cast_rays* and rt_any_intersection* take no order: their kernels walk per lane, so wavefront packing matters less.
 * A caller who wants it can apply rt_ray_order_read's permutation to its own arrays (the queries have no per-index state). */
typedef struct rt_ray_order rt_ray_order;
typedef struct rt_ray_order_desc {
  uint32_t abi_version; /* RT_ABI_VERSION */
  uint32_t capacity;    /* most rays a batch of this order may have, 1 .. 2^27 */
  uint32_t origin_bits; /* bits per active origin axis, 0 = default, at most 10 */
  uint32_t reserved;    /* 0 */
} rt_ray_order_desc;
typedef struct rt_ray_order_info {
  uint32_t n_rays, n_live;                    /* rays of the batch; of them not dead (0 after rt_ray_order_set) */
  uint32_t origin_bits, direction_bits;       /* bits per active axis as applied */
  uint32_t n_origin_axes, n_direction_axes;   /* axes on which the live rays differ */
  uint64_t bytes;                             /* device memory the order holds */
  double device_ms;                           /* rt_ray_order_build: the kernels of the last build (0 otherwise) */
} rt_ray_order_info;

/* allocates the permutation, the keys and the sort workspace for `capacity` rays on `device` (20 bytes per ray + tables) */
int rt_ray_order_create(const rt_ray_order_desc* desc, int device, rt_ray_order** out);
void rt_ray_order_destroy(rt_ray_order* order);
/* HOST arrays (origin, direction; max_distance and flags are not read): staged through device memory of the call; returns
 * when the order is built */
int rt_ray_order_build(rt_ray_order* order, const rt_ray_batch* host_batch);
/* DEVICE arrays on the order's device: enqueues the bounds, key and sort kernels on `hip_stream`; allocates nothing, reads
 * nothing back and never synchronises */
int rt_ray_order_build_device(rt_ray_order* order, const rt_ray_batch* batch, void* hip_stream);
/* the caller's own order (its tiles, say): perm_host[k] = the ray at position k; checked on the host; blocks */
int rt_ray_order_set(rt_ray_order* order, const uint32_t* perm_host, uint32_t n);
/* blocks until the last build is done; every output nullable: perm_host [n_rays], keys_host [n_rays] (the key of ray i;
 * refused after rt_ray_order_set, which has none) */
int rt_ray_order_read(rt_ray_order* order, uint32_t* perm_host, uint32_t* keys_host, rt_ray_order_info* info);
/* rt_trace_rays through `order`; order NULL: one is built for this call (and freed), rt_stats.kernel_ms includes it */
int rt_trace_rays_ordered(rt_scene* scene, const rt_params* shading, const rt_ray_batch* batch, const rt_ray_order* order,
                          const rt_ray_radiance* out, rt_stats* stats);
/* rt_trace_rays_device through `order` (not NULL: the device form allocates nothing) */
int rt_trace_rays_ordered_device(rt_scene* scene, const rt_params* shading, const rt_ray_batch* batch, const rt_ray_order* order,
                                 const rt_ray_radiance* out, void* hip_stream);

/* ---- camera views: anti-aliased frames from any camera, rays made and samples resolved on the device -------------------------
 *
 * No reference counterpart beyond its one compile-time view (renderer/mod.rs:176-180, antialiased_raytrace,
 * raytracer_renderer.rs:918-1016).  An rt_view is a frame shape, a table of sample offsets and, once set, a camera; it owns
 * the device memory a frame of it needs.  rt_render_view_device enqueues, all on the caller's stream:
 *   1. the ray generator: one ray per (pixel, DISTINCT sample),
 *   2. rt_ray_order_build_device on those rays, when the order mode asks for it,
 *   3. rt_trace_rays_ordered_device (RT_VIEW_ORDER_NONE: rt_trace_rays_device) into the view's per-ray planes,
 *   4. the resolve: the reference's accumulation of a pixel's sample colours, into the caller's per-pixel planes.
 * It allocates nothing itself.  Blocking, validation of `shading` and the one-render-call-per-scene rule are the trace's,
 * unchanged: with REFLECTIONS / REFRACTIONS the call blocks in step 3 and allocates there what rt_trace_rays_device
 * allocates; it is refused while rt_render_begin owns the scene.  RT_FLAG_ANTI_ALIASING in `shading` is refused: the view's
 * samples are the anti-aliasing.
 *
 * Rays.  The caller gives n_samples (1..64) offsets; the bit-distinct ones, in first-occurrence order, are the n_distinct
 * sample planes (the reference's deterministic table repeats 7 of 16), and plane_of[k] is the plane of sample k.  The ray
 * of pixel p = y * width + x (row 0 is the top) and distinct sample u has batch index i = u * width * height + p, which is
 * also its light-cloud key (rt_trace_rays' rule).  Repeated samples read the plane they repeat: exact by definition.
 *   RT_VIEW_PINHOLE    offsets (sx, sy) in PIXELS from the pixel centre; origin = eye, direction = forward + a right + b up,
 *                      a = (2 (x + 0.5 + sx) - W) / H * tan_half_fov_y, b = (H - 2 (y + 0.5 + sy)) / H * tan_half_fov_y
 *                      (square pixels; right / up / forward: the caller's orthonormal basis; not normalised -- the trace does)
 *   RT_VIEW_REFERENCE  offsets in the units of rt_params.aa_offsets (that table can be passed as is);
 *                      coords = (float(x) fw, float(y) fh, 0), origin = coords + (sx, sy, 0), direction = coords - focus
 * Every operation is one correctly rounded fp32 operation, evaluated as written, left to right.
 *
 * Resolve, over all n_samples with repeats read through plane_of: scale = 1 / (8 ceil(n / 8)); a valid sample k contributes
 * cs = c scale -- k < 8: first[k] = cs, else rest[k & 7] = cs + rest[k & 7]; lane[l] = rest[l] + first[l]; the pixel is
 * ((l0 + l4) + (l2 + l6)) + ((l1 + l5) + (l3 + l7)).  n_samples == 1: the sample's colour, unscaled.  The pixel planes are
 * an rt_ray_radiance of width * height entries: rgb (0, 0, 0) if no sample is valid; valid = any sample valid; id / t those
 * of sample 0 (-1 / +inf on its miss); argb packed as everywhere, UNTOUCHED when no sample is valid.
 * Both formulas are specified by a host model compiled from the same source as the kernels (csrc/rt_view.h):
 * rt_view_rays_model and rt_view_resolve_model.
 *
 * Order modes.  RT_VIEW_ORDER_ONCE (0, the default): the first render after rt_view_create builds the order, later ones
 * reuse it -- an order depends only on the batch, and a camera that moves keeps its pixel-to-ray pattern.
 * RT_VIEW_ORDER_ALWAYS rebuilds it every frame, RT_VIEW_ORDER_NONE traces without one.  Same image, bit for bit.
 *
 * Memory: rt_view_create allocates everything the device form needs -- per ray 24 bytes of origin and direction, 21 bytes
 * of rgb / valid / id / t planes and the 20 bytes of an rt_ray_order of capacity n_rays (+ tables); rt_view_info.bytes.
 * n_rays = n_distinct * width * height must not exceed 2^27, the orders' limit.
 *
 * rt_stats are the trace's (host form; device form: rt_render_collect_stats after synchronising): rays_primary counts the
 * live DISTINCT rays, pixels_written the valid RAYS (not pixels), the others as rt_trace_rays counts them.
 *
 * Soft shadows, a deviation from rt_render: each distinct sample of a pixel draws its own light-cloud set, keyed by
 * u * width * height + p, where rt_render gives every sample of a pixel the pixel's set.  Both are seeded stand-ins for the
 * reference's unseeded per-pixel sets; a view frame with soft shadows is not comparable pixel for pixel with rt_render's.
 *
 * Refused with RT_ERR_INVALID_ARG (+ rt_last_error) before any HIP call: a NULL pointer or wrong abi_version; width or
 * height 0; n_samples 0 or above 64; a non-finite sample offset; n_rays above 2^27; an unknown kind or order mode; a
 * non-finite camera member; tan_half_fov_y <= 0 (pinhole); a render before any rt_view_set_camera; a view on another device
 * than the scene; every output plane NULL; and whatever rt_trace_rays refuses in `shading`.
 * One render per view at a time, and a view's frames go on one stream or are ordered by the caller (a reused order is
 * read by the next frame's trace); rt_view_destroy and rt_view_read wait for the view's last work. */
#define RT_VIEW_PINHOLE 0u
#define RT_VIEW_REFERENCE 1u
#define RT_VIEW_ORDER_ONCE 0u
#define RT_VIEW_ORDER_ALWAYS 1u
#define RT_VIEW_ORDER_NONE 2u
typedef struct rt_view rt_view;
typedef struct rt_view_desc {
  uint32_t abi_version; /* RT_ABI_VERSION */
  uint32_t width, height;
  uint32_t n_samples;   /* 1 .. 64 */
  const float* samples; /* [n_samples][2] */
  uint32_t order;       /* RT_VIEW_ORDER_* */
} rt_view_desc;
typedef struct rt_view_camera {
  uint32_t abi_version; /* RT_ABI_VERSION */
  uint32_t kind;        /* RT_VIEW_PINHOLE: eye .. tan_half_fov_y are read; RT_VIEW_REFERENCE: focus, fw, fh */
  float eye[3], right[3], up[3], forward[3];
  float tan_half_fov_y;
  float focus[3], fw, fh;
} rt_view_camera;
typedef struct rt_view_info {
  uint32_t n_pixels, n_samples, n_distinct, n_rays;
  uint64_t bytes;       /* device memory the view holds, its ray order included */
  uint32_t order_built; /* 1: the view holds a built order */
  uint32_t reserved;
  double rays_ms, order_ms, resolve_ms; /* rt_render_view: device time of the generator, the order build (0 when reused) and the resolve */
} rt_view_info;

int rt_view_create(const rt_view_desc* desc, int device, rt_view** out);
void rt_view_destroy(rt_view* view);
/* validates and stores the camera of the next frames; no allocation, no HIP call */
int rt_view_set_camera(rt_view* view, const rt_view_camera* camera);
/* the generator alone, for callers with a pipeline of their own: n_rays rays into DEVICE arrays [n_rays][3] on the view's device */
int rt_view_rays_device(rt_view* view, float* origin_dev, float* direction_dev, void* hip_stream);
/* HOST arrays; blocks */
int rt_view_rays(rt_view* view, float* origin_host, float* direction_host);
/* pixels_dev: DEVICE planes of width * height entries on the scene's device; enqueued on `hip_stream` */
int rt_render_view_device(rt_scene* scene, rt_view* view, const rt_params* shading, const rt_ray_radiance* pixels_dev, void* hip_stream);
/* HOST planes (argb is uploaded first: pixels without a valid sample keep the caller's value); blocks.  stats may be NULL. */
int rt_render_view(rt_scene* scene, rt_view* view, const rt_params* shading, const rt_ray_radiance* pixels_host, rt_stats* stats);
/* waits for the view's device work; plane_of_host [n_samples] bytes and info are nullable */
int rt_view_read(rt_view* view, uint8_t* plane_of_host, rt_view_info* info);
/* The host models (no device needed).  origin / direction: [n_distinct * width * height][3], sized by the caller for
 * n_samples planes at most; plane_of [n_samples]; every output nullable. */
int rt_view_rays_model(const rt_view_desc* desc, const rt_view_camera* camera, float* origin, float* direction, uint8_t* plane_of,
                       uint32_t* n_distinct);
/* rays: the per-ray planes of a trace of the model's rays (all four required); pixels: [n_pixels] planes, every member nullable */
int rt_view_resolve_model(uint32_t n_pixels, uint32_t n_samples, const uint8_t* plane_of, const rt_ray_radiance* rays,
                          const rt_ray_radiance* pixels);

/* ---- adaptive camera views: all samples only where sample 0 shows an edge ----------------------------------------------------
 *
 * rt_render_view_adaptive_device traces sample 0 of every pixel (plane 0), picks the pixels to refine from what plane 0 saw,
 * and traces the other distinct samples of those pixels only.  All on the caller's stream, nothing allocated or read back:
 *   1. pass 1: the generator for plane 0 and a trace of its width * height rays -- batch indices, hence light-cloud keys,
 *      those of the full view -- through the plane-0 part of the view's order, into base planes the view owns,
 *   2. classify: one thread per pixel applies the refine rule -> mask,
 *   3. the sparse generator: ray (u, p) with u >= 1 and mask[p] set as rt_render_view makes it, every other ray dead
 *      (direction 0),
 *   4. a stable partition of the view's order by liveness: live rays first, in the order they had,
 *   5. pass 2: a trace of all n_rays rays through that permutation (dead rays are misses, in whole wavefronts at the tail),
 *   6. the adaptive resolve.
 * n_distinct == 1: steps 3 to 5 are skipped.  RT_VIEW_ORDER_ONCE: the first frame builds the order from one run of the full
 * generator; ALWAYS does so every frame; NONE partitions the identity.
 *
 * The refine rule.  Pixel p is refined iff criteria has RT_REFINE_EVERY, or for one of its up to 8 neighbours q in the frame
 *   any of ID / DEPTH / COLOUR is set and valid0[p] != valid0[q], or
 *   RT_REFINE_ID      and id0[p] != id0[q]  (ids are canonical object indices: inside a mesh every triangle edge is one), or
 *   RT_REFINE_DEPTH   and both are valid and NOT |t_p - t_q| <= depth_tol * min(t_p, t_q), or
 *   RT_REFINE_COLOUR  and both are valid and, in some channel, NOT |c_p - c_q| <= colour_tol
 * (negated comparisons: a NaN refines; criteria == 0 refines nothing; symmetric: both sides of an edge refine).
 *
 * Pixels.  A refined pixel is rt_render_view's pixel, bit for bit.  An unrefined pixel is the resolve formula above with every
 * sample reading plane 0 (n_samples and scale unchanged): what the full resolve gives a pixel whose samples all agree.  id and
 * t are those of plane 0; argb is untouched when no contributing sample is valid.  A feature thinner than a pixel that sample
 * 0 of the pixel and of all its neighbours misses is not found: the method's limit.
 * Host models, compiled from the kernels' source (csrc/rt_view_adapt.h): rt_view_refine_model, rt_view_resolve_adaptive_model.
 *
 * Blocking, validation of `shading`, the one-render-call-per-scene rule and the behaviour with REFLECTIONS / REFRACTIONS are
 * the trace's, twice.  rt_stats of the host form: the two traces summed.
 * Refused with RT_ERR_INVALID_ARG before any HIP call: a NULL pointer or wrong abi_version; unknown criteria bits; a
 * tolerance that is negative or NaN; a view without rt_view_enable_adaptive; everything rt_render_view refuses. */
#define RT_REFINE_ID 1u
#define RT_REFINE_DEPTH 2u
#define RT_REFINE_COLOUR 4u
#define RT_REFINE_EVERY 8u
typedef struct rt_view_refine {
  uint32_t abi_version; /* RT_ABI_VERSION */
  uint32_t criteria;    /* RT_REFINE_* */
  float colour_tol, depth_tol;
} rt_view_refine;
typedef struct rt_view_adaptive_info {
  uint32_t n_refined, n_live_rays; /* of the last adaptive frame: refined pixels; live rays of pass 2 */
  uint64_t bytes;                  /* the adaptive workspace (beside rt_view_info.bytes) */
  double pass1_ms, classify_ms, partition_ms, pass2_ms, resolve_ms; /* rt_render_view_adaptive: device time per stage (partition: with the sparse generator) */
} rt_view_adaptive_info;
/* allocates the workspace: base planes (21 bytes per pixel), mask, a second permutation (4 bytes per ray), the plane-0 order,
 * flags and scan arrays; blocks; idempotent */
int rt_view_enable_adaptive(rt_view* view);
/* pixels_dev as rt_render_view_device; mask_dev: [width * height] bytes on the device, nullable */
int rt_render_view_adaptive_device(rt_scene* scene, rt_view* view, const rt_params* shading, const rt_view_refine* refine,
                                   const rt_ray_radiance* pixels_dev, uint8_t* mask_dev, void* hip_stream);
/* HOST planes and mask (nullable); blocks.  stats may be NULL. */
int rt_render_view_adaptive(rt_scene* scene, rt_view* view, const rt_params* shading, const rt_view_refine* refine,
                            const rt_ray_radiance* pixels_host, uint8_t* mask_host, rt_stats* stats);
/* waits for the view's device work */
int rt_view_adaptive_read(rt_view* view, rt_view_adaptive_info* info);
/* The host models (no device needed).  plane0: the rgb, valid, id and t of sample 0 of every pixel (all four required);
 * mask_out [width * height] and n_refined_out nullable. */
int rt_view_refine_model(uint32_t width, uint32_t height, const rt_view_refine* refine, const rt_ray_radiance* plane0, uint8_t* mask_out,
                         uint32_t* n_refined_out);
/* base: plane 0 (all four planes); rays: per-ray rgb and valid of n_distinct * n_pixels rays, plane 0 of them not read (NULL
 * allowed when every plane_of is 0); pixels as rt_view_resolve_model */
int rt_view_resolve_adaptive_model(uint32_t n_pixels, uint32_t n_samples, const uint8_t* plane_of, const uint8_t* mask,
                                   const rt_ray_radiance* base, const rt_ray_radiance* rays, const rt_ray_radiance* pixels);

/* ---- thin-lens camera views: depth of field from a table of lens offsets, adaptive frames included -----------------------------
 *
 * No reference counterpart: its camera is a compile-time pinhole (renderer/mod.rs, raytracer_renderer.rs).  A lens view is a
 * view with a second table beside the pixel offsets: n_samples lens offsets (lx, ly) in unit-disk coordinates (finite, not
 * otherwise constrained).  Per frame rt_view_set_lens gives an aperture radius A in scene units and a focus distance F
 * measured along `forward`.  With a, b and d0 = forward + a right + b up as RT_VIEW_PINHOLE makes them from (sx, sy):
 *   off[k] = (A lx) right[k] + (A ly) up[k],   origin[k] = eye[k] + off[k],   direction[k] = F d0[k] - off[k]
 * every operation one correctly rounded fp32 operation, evaluated as written, left to right.  All lens samples of a pixel
 * offset meet at eye + F d0: the plane at distance F along `forward` is in focus.  RT_VIEW_REFERENCE cameras have no lens.
 *
 * Planes.  Two samples share a plane only if all four floats (sx, sy, lx, ly) are bit-identical; the planes are in
 * first-occurrence order, as those of rt_view_create.  Ray index, layout and light-cloud key stay u * width * height + p; the
 * 2^27-ray limit counts these planes.  The ray order is still built once (RT_VIEW_ORDER_ONCE) and reused while camera,
 * aperture and focus change.
 * A == 0 switches the lens off: the view runs the pinhole generator on the pixel offsets of its planes (any camera kind).  A
 * lens view without rt_view_set_lens behaves as A == 0.  Every call that takes a view takes a lens view.
 *
 * Adaptive frames.  The refine rule above looks for edges in sample 0 and never refines a smooth out-of-focus region, which
 * then comes out sharp.  With A > 0 and a finite coc_tol a lens view therefore runs the defocus criterion behind the classify
 * step, on plane 0 -- sample 0 should have lens offset (0, 0), so that plane 0 is the view through the lens centre (not
 * required).  The circle of confusion of pixel p, in pixels:
 *   len = sqrt((dx dx + dy dy) + dz dz) of d0 through plane 0's pixel offset,   z = t0[p] / len,
 *   coc[p] = ((A |z - F|) / (z F)) * (H / (2 tan_half_fov_y)),   0 where plane 0 missed
 * and pixel p is added to the mask iff some pixel q of the frame with max(|dx|, |dy|) <= spread has
 *   NOT coc[q] <= coc_tol   and   NOT coc[q] < max(|dx|, |dy|)        (q = p included; negated comparisons: a NaN refines)
 * -- q is out of focus and its blur reaches p.  n_refined counts every pixel once.  Everything behind the mask is unchanged:
 * a refined pixel is the full lens frame's pixel bit for bit, an unrefined one reads plane 0 for every sample.
 * coc_tol = +inf turns the criterion off (the mask is the refine rule's alone).  Blur wider than `spread` pixels (0 .. 16) is
 * cut off: the method's limit.  The coc plane costs 4 bytes per pixel, allocated by rt_view_create_lens (rt_view_info.bytes).
 * Host models, compiled from the kernels' source (csrc/rt_view_lens.h): rt_view_lens_rays_model, rt_view_defocus_model.
 *
 * Refused with RT_ERR_INVALID_ARG (+ rt_last_error) before any HIP call: a NULL pointer or wrong abi_version; a non-finite
 * lens offset; more than 2^27 rays; rt_view_set_lens on a view made by rt_view_create; an aperture that is negative, NaN or
 * inf; a focus_distance that is not finite and positive; a coc_tol that is NaN or negative; spread > 16; a non-zero
 * `reserved`; rays or a render with A > 0 and an RT_VIEW_REFERENCE camera; everything rt_view_create / rt_render_view refuse. */
typedef struct rt_view_lens {
  uint32_t abi_version; /* RT_ABI_VERSION */
  uint32_t spread;      /* 0 .. 16 pixels: how far the defocus criterion lets a blur reach */
  float aperture;       /* A: the lens radius in scene units; 0: no lens */
  float focus_distance; /* F: along `forward`; finite and positive */
  float coc_tol;        /* pixels; a circle of confusion above it refines; +inf: the criterion is off */
  uint32_t reserved;    /* 0 */
} rt_view_lens;
/* rt_view_create with a lens table: lens_samples [desc->n_samples][2] */
int rt_view_create_lens(const rt_view_desc* desc, const float* lens_samples, int device, rt_view** out);
/* validates and stores the lens of the next frames; no allocation, no HIP call */
int rt_view_set_lens(rt_view* view, const rt_view_lens* lens);
/* The host models (no device needed).  rt_view_rays_model for a lens view: plane_of and n_distinct count 4-tuples. */
int rt_view_lens_rays_model(const rt_view_desc* desc, const float* lens_samples, const rt_view_camera* camera, const rt_view_lens* lens,
                            float* origin, float* direction, uint8_t* plane_of, uint32_t* n_distinct);
/* The defocus criterion on plane 0 of a desc->width x desc->height frame (desc->samples[0]: its pixel offset; an RT_VIEW_PINHOLE
 * camera): valid0 and t0 [width * height] are required; coc_out receives the coc plane, mask_inout [width * height] bytes the
 * pixels the criterion picks (set to 1, the others left alone), n_added_out how many of them were 0 before -- all three
 * nullable.  With A == 0 or coc_tol = +inf the criterion is off: coc_out is zeroed and nothing is added. */
int rt_view_defocus_model(const rt_view_desc* desc, const rt_view_camera* camera, const rt_view_lens* lens, const uint8_t* valid0,
                          const float* t0, float* coc_out, uint8_t* mask_inout, uint32_t* n_added_out);

/* thread-local message for the last non-RT_OK return on this thread */
const char* rt_last_error(void);

/* hash of the sources and flags this library was built from (profiles/ summaries record it: a rocprof summary is
 * only quoted for the build it was taken on) */
const char* rt_build_id(void);

/* diagnostics: the kernels' correctly rounded sqrt and reciprocal (normal-range sequences, csrc/rt_kernels.hip
 * exact_sqrt / exact_rcp) evaluated on `n` host values on `device` -- tests compare them with IEEE sqrtf / division */
int rt_selftest_exact_math(int device, const float* in, float* out_sqrt, float* out_rcp, uint32_t n);

/* introspection for DESIGN.md / tests: BVH size of a created scene */
typedef struct rt_bvh_info {
  uint32_t n_nodes;
  uint32_t n_leaves;
  uint32_t max_depth;
  uint32_t max_leaf_size;
  uint64_t bytes_nodes;
  uint64_t bytes_triangles;
  uint32_t n_references; /* triangle references in the leaves (>= n_triangles: split clipping) */
} rt_bvh_info;
int rt_scene_bvh_info(const rt_scene* scene, rt_bvh_info* out);

/* What a scene handle holds in device memory, by purpose (the reference's Scene: src/scene/scene.rs:24-27, < 1 MB of host memory). */
typedef struct rt_scene_info {
  uint64_t bytes_geometry;    /* spheres, triangle records (intersection + shading), ids, materials, lights, receiver records */
  uint64_t bytes_bvh;         /* BVH nodes + the 8 per-octant copies + the threaded copy */
  uint64_t bytes_flags;       /* receiver flags + the cell geometry rt_flags_kernel reads (optional table, under the budget) */
  uint64_t bytes_cell_lists;  /* per-cell candidate lists, the work list of their third stage and the pool of wide records (64 bytes per list of 9 to 32
                                 candidates; RT_CELL_WIDE=0 in the environment leaves it out) -- optional tables, under the budget; 0 = not built */
  uint64_t bytes_tables;      /* AA samples, light clouds, tile lists, counters */
  uint64_t bytes_workspace;   /* ray queues, sort workspace, pair queues, set records, pixel accumulators of every frame slot in use */
  uint64_t bytes_frames;      /* frame buffer + aux planes rt_render keeps for host callers */
  uint64_t bytes_total;
  uint64_t budget_bytes;      /* rt_scene_desc.device_budget_bytes as applied (bounds bytes_flags + bytes_cell_lists) */
  uint32_t n_receiver_cells;
  uint32_t cell_lists_built;  /* 1 = the lists exist (they are built by the first frame with soft shadows) */
} rt_scene_info;
int rt_scene_memory_info(const rt_scene* scene, rt_scene_info* out);

/* ---- in-place scene updates: new values for the objects of an existing handle, BVH refitted on the device ------------------
 *
 * No reference counterpart (its Scene is immutable during a render).  A delta carries new VALUES for objects the scene
 * already has: counts and the object -> material assignment are those of rt_scene_create.  The tree keeps its topology;
 * its boxes, the per-octant and threaded copies, the intersection / shading / receiver records and the scene bounds are
 * recomputed by small kernels (csrc/rt_update.hip) with the arithmetic of the scene packer.
 *
 * After the call returns, every render, progressive render, multi-GPU render and query on this handle behaves exactly as
 * on a handle freshly created from the updated description; the exceptions are speed (a refitted tree is looser than a
 * rebuilt one, and the receiver-cell allocation is the one of creation) and rt_scene_bvh_info (the topology is kept).
 *
 * Both forms BLOCK: at entry they wait for every frame of this scene still in flight, at exit they synchronise their
 * stream (the new scene bounds are read back there).  Ray queries the caller still has in flight on streams of its own are
 * NOT waited for: finish them first.  Asynchronous updates are out of scope; so are adding or removing
 * objects, a rebuild heuristic (the rebuild itself: rt_scene_rebuild), and the refit of split-clipped trees.
 *
 * RT_ERR_INVALID_ARG (rt_last_error names the field): NULL scene or delta; wrong abi_version; a partial group;
 * tri_first + tri_count > n_triangles; a delta that changes nothing; a progressive render owns the scene; a material row
 * whose transmissive class -- has_opacity != 0 && !(fabs(opacity) <= 1.1920929e-7f) -- changes while a triangle uses it
 * (the tree was built for that class).  All of these are found before any kernel runs; the device form reads the
 * material rows back to check them.
 * RT_ERR_UNSUPPORTED: a triangle group on a scene whose n_references > n_triangles (split clipping was on: clipped
 * reference boxes cannot be refitted).  The default split_depth is 0.
 * Multi-GPU: the caller updates each per_gpu[i]. */
typedef struct rt_scene_delta {
  uint32_t abi_version;          /* RT_ABI_VERSION */
  /* every group: NULL = unchanged */
  const float* sphere_center;    /* [n_spheres][3]  | the three sphere arrays are given together or not at all */
  const float* sphere_r_sq;      /* [n_spheres]     | */
  const float* sphere_r_inv;     /* [n_spheres]     | (not read by the library, as in rt_scene_desc) */
  uint32_t tri_first, tri_count; /* canonical triangles [tri_first, tri_first + tri_count) are replaced; 0 = none */
  const float* tri_v1;           /* [tri_count][3]  | all four together */
  const float* tri_e1;
  const float* tri_e2;
  const float* tri_normal;
  const float* materials;        /* [n_materials][RT_MATERIAL_STRIDE] */
  const float* lights;           /* [n_lights][RT_LIGHT_STRIDE] */
} rt_scene_delta;

#define RT_UPDATE_INVALIDATES_RECEIVER_TABLES 1u /* receiver flags / cell lists: rebuilt by the next soft-shadow frame */
#define RT_UPDATE_INVALIDATES_TILE_COSTS 2u      /* RT_TILE_ORDER_COST: the next such frame calibrates again */
#define RT_UPDATE_INVALIDATES_QUEUE_SIZES 4u     /* the next frame with secondary rays verifies its queue sizes as a first frame does */

typedef struct rt_update_info {
  double device_ms;             /* device time of the update's kernels and copies */
  double total_ms;              /* wall time of the call */
  uint32_t nodes_refitted;      /* BVH nodes whose boxes were recomputed (0: no geometry in the delta) */
  uint32_t slots_rewritten;     /* leaf slots whose intersection / shading records were rewritten */
  uint32_t receivers_disabled;  /* triangles whose receiver grid is off (R = 0: their hit points walk the tree for soft shadows)
                                   because the new maps are not finite or too ill-conditioned for the R of creation */
  uint32_t tables_invalidated;  /* RT_UPDATE_INVALIDATES_* */
} rt_update_info;

/* host arrays (staged through one pinned buffer); `info` may be NULL */
int rt_scene_update(rt_scene* scene, const rt_scene_delta* delta, rt_update_info* info);
/* device arrays on the scene's device; the kernels run on `hip_stream` */
int rt_scene_update_device(rt_scene* scene, const rt_scene_delta* delta, void* hip_stream, rt_update_info* info);

/* ---- part poses: rigid parts of a scene placed by similarity transforms on the device, then refitted ------------------------
 *
 * Reference: Scene::from_obj(path, Some(Similarity3)) (src/scene/scene.rs:43-134) places a mesh with
 * Similarity3::transform_vec on its vertices and rotated_by(rotation) on its normals, once, at load time.  An rt_pose does
 * that per frame: it holds the REST pose of the parts of a scene on the device, one kernel (csrc/rt_pose.hip) writes the
 * posed arrays of an rt_scene_delta from 32 bytes of transform per part, and rt_scene_update_device takes them.
 *
 * A transform is 8 floats: translation, a rotor {s, xy, xz, yz} in the layout of ultraviolet's Rotor3 (NOT normalised by the
 * library), and a scale.  Every operation is one correctly rounded fp32 operation, evaluated as written, left to right,
 * never fused; a - b is a + (-b):
 *   rotate(v):  fx = (s vx + xy vy) + xz vz      fy = (s vy - xy vx) + yz vz
 *               fz = (s vz - xz vx) - yz vy      fw = (xy vz - xz vy) + yz vx
 *               x' = ((s fx + xy fy) + xz fz) + yz fw
 *               y' = ((s fy - xy fx) - xz fw) + yz fz
 *               z' = ((s fz + xy fw) - xz fx) - yz fy
 *   T(v)     =  rotate(v) scale + translation        (per component: one multiply, one add)
 *   triangle:   v1' = T(v1), v2' = T(v2), v3' = T(v3);  e1' = v2' - v1';  e2' = v3' - v1';  n' = rotate(n)
 *   sphere:     c' = T(c);  r' = r scale;  r_sq' = r' r';  r_inv' = 1 / r'
 * The formulas are specified by a host model compiled from the same source as the kernel (csrc/rt_pose.h): rt_pose_model.
 * The rest pose holds the VERTICES v2 and v3, not the edges, and the radius, not its square: only then is a posed mesh the
 * mesh from_obj would have loaded, v1 / e1 / e2 bit for bit.  Deviation: the reference rotates per-vertex normals and lerps
 * afterwards, a pose rotates the stored normal; the two differ by a few 2^-24 per component (csrc/rt_pose.h).
 *
 * Parts.  A part is a range of canonical triangles and / or a range of spheres that share one transform.  The pose's
 * COVERING triangle range [tri_first, tri_first + tri_count) is the smallest range that holds every part's triangles; it is
 * the triangle group of every apply, and the posed triangle arrays (rt_pose_read, rt_pose_model) cover it, element 0 being
 * triangle tri_first.  A triangle of the covering range that belongs to no part is restated by every apply with its rest
 * values v1, v2 - v1, v3 - v1, normal.  When some part has spheres, every apply carries the sphere group (an update replaces
 * all spheres): spheres of no part are restated as centre, r r, 1 / r, and the posed sphere arrays cover all n_spheres;
 * otherwise the pose has no sphere arrays and the sphere outputs are not written.  The rest arrays are read inside the
 * covering range (triangles) and in full (spheres, when a part has some), at rt_pose_create only.
 *
 * rt_pose_create allocates everything: the rest pose, the part tables, the posed arrays (initialised with the rest values)
 * and room for n_parts staged transforms.  The device forms allocate nothing.
 * rt_pose_apply_device enqueues the kernel on `hip_stream` and calls rt_scene_update_device with the pose's own device
 * arrays: everything about blocking, invalidation, refusals (RT_ERR_UNSUPPORTED on split-clipped trees included) and
 * rt_update_info is that call's, unchanged.  rt_pose_apply stages the transforms through the pose's buffer on the null
 * stream and does the same.  rt_pose_geometry_device is the kernel alone, for callers with a pipeline of their own.
 * One apply per pose at a time; a pose's work goes on one stream or is ordered by the caller.
 *
 * Refused with RT_ERR_INVALID_ARG (+ rt_last_error) before any HIP call: a NULL pointer or wrong abi_version; n_parts == 0
 * or a part with both counts 0; a range beyond n_triangles / n_spheres; overlapping ranges; NULL rest arrays for a kind some
 * part uses; on apply a pose whose counts differ from the scene's, a pose on another device than the scene, and what
 * rt_scene_update_device refuses in the delta; in the HOST form only, a non-finite transform member.  The device form
 * cannot look at the transforms: what non-finite geometry does is what rt_scene_update_device does with it.
 * Out of scope: lights are not posed (a caller moves them through rt_scene_update); hierarchies of parts.  A mesh that
 * BENDS is an rt_skin (below). */
typedef struct rt_transform {
  float translation[3];
  float rotor[4]; /* s, xy, xz, yz */
  float scale;
} rt_transform;
typedef struct rt_pose_part {
  uint32_t tri_first, tri_count, sphere_first, sphere_count;
} rt_pose_part;
typedef struct rt_pose_desc {
  uint32_t abi_version; /* RT_ABI_VERSION */
  uint32_t n_parts;
  const rt_pose_part* parts;        /* triangle ranges pairwise disjoint, sphere ranges pairwise disjoint; either count may be 0, not both */
  uint32_t n_triangles, n_spheres;  /* those of the scene the pose is for */
  const float* tri_v1;              /* rest pose, [n_triangles][3]; read only inside the covering range */
  const float* tri_v2;
  const float* tri_v3;
  const float* tri_normal;
  const float* sphere_center;       /* rest pose, [n_spheres][3]; ALL spheres (an update replaces all) */
  const float* sphere_radius;       /* [n_spheres] */
} rt_pose_desc;
typedef struct rt_pose rt_pose;

int rt_pose_create(const rt_pose_desc* desc, int device, rt_pose** out);
void rt_pose_destroy(rt_pose* pose);
/* the kernel alone: transforms_dev [n_parts] on the pose's device; enqueued on `hip_stream` */
int rt_pose_geometry_device(rt_pose* pose, const rt_transform* transforms_dev, void* hip_stream);
/* kernel + rt_scene_update_device on `hip_stream`; blocks as that call does; `info` may be NULL */
int rt_pose_apply_device(rt_scene* scene, rt_pose* pose, const rt_transform* transforms_dev, void* hip_stream, rt_update_info* info);
/* host transforms [n_parts]; blocks */
int rt_pose_apply(rt_scene* scene, rt_pose* pose, const rt_transform* transforms_host, rt_update_info* info);
/* waits for the pose's device work; the posed arrays as the last kernel left them: triangle arrays [tri_count][3] over the
 * covering range, sphere arrays [n_spheres][3] / [n_spheres]; every output nullable */
int rt_pose_read(rt_pose* pose, float* tri_v1, float* tri_e1, float* tri_e2, float* tri_normal, uint32_t* tri_first, uint32_t* tri_count,
                 float* sphere_center, float* sphere_r_sq, float* sphere_r_inv);
/* The host model (no device needed): the same layout as rt_pose_read; every output nullable.  Transforms are not checked. */
int rt_pose_model(const rt_pose_desc* desc, const rt_transform* transforms, float* tri_v1, float* tri_e1, float* tri_e2, float* tri_normal,
                  float* sphere_center, float* sphere_r_sq, float* sphere_r_inv);

/* ---- skinned meshes: an indexed mesh deformed by linear blend skinning on the device, then refitted ---------------------------
 *
 * Reference: Scene::from_obj (src/scene/scene.rs:43-134, tobj with single_index: true) works on an INDEXED mesh in two
 * steps: it transforms the unified vertices and rotates the per-vertex normals, then lerps the three normals per face.  An
 * rt_skin holds such a mesh in rest pose on the device and does the same per frame, with up to four bones per vertex in
 * place of the one transform: two kernels (csrc/rt_skin.hip) write the triangle arrays of an rt_scene_delta from 32 bytes
 * per bone, and rt_scene_update_device takes them.  The mesh IS one range of canonical triangles of a scene,
 * [tri_first, tri_first + tri_count): triangle tri_first + t is indices[t].
 *
 * A bone is an rt_transform, not normalised by the library; T(v) and rotate(n) are those of a pose (above).  Every operation
 * is one correctly rounded fp32 operation, evaluated as written, left to right, never fused (except the two fma of the
 * face normal); a - b is a + (-b):
 *   vertex i:    influences (bone[i][k], weight[i][k]), k = 0..3, in that order; a weight of +0 or -0 is skipped;
 *                the first influence kept sets   acc = w T_b(v)          (three multiplies)
 *                every later one adds            acc = acc + w T_b(v)    (per component one multiply, one add)
 *                normals: the same with rotate_b(n).  No influence kept: the rest position and the rest normal.
 *                Weights are NOT normalised and no sum is required: one influence of weight 1 gives T_b(v) exactly, so a
 *                mesh skinned to one bone is the mesh from_obj would have loaded with that transform, normals included
 *                (a pose, which rotates the lerped normal, deviates there by a few 2^-24).
 *   triangle t:  indices (i0, i1, i2);  v1 = V[i0];  e1 = V[i1] - V[i0];  e2 = V[i2] - V[i0]
 *                with vertex normals:     n = (N[i0] 0.5 + N[i1] 0.5) 0.5 + N[i2] 0.5, per component
 *                without (normal NULL):   c = e1 x e2, cx = e1y e2z + (-e1z) e2y, ...;  d = fma(cx, cx, fma(cy, cy, cz cz));
 *                                         r = 1 / sqrt(d);  n = c r.  A degenerate triangle gives a non-finite normal: what
 *                                         such geometry does is what rt_scene_update_device does with it.
 * The formulas are specified by a host model compiled from the same source as the kernels (csrc/rt_skin.h): rt_skin_model.
 *
 * rt_skin_create allocates everything: the rest arrays, the index, bone and weight tables, the skinned vertices, the four
 * posed triangle arrays (initialised on the host with the rest mesh run through the triangle formula), room for n_bones
 * staged transforms and a pinned stage.  The device forms allocate nothing.
 * rt_skin_apply_device enqueues the vertex kernel and the triangle kernel on `hip_stream`, back to back, and calls
 * rt_scene_update_device with the skin's own device arrays: everything about blocking, invalidation, refusals
 * (RT_ERR_UNSUPPORTED on split-clipped trees included) and rt_update_info is that call's, unchanged.  rt_skin_apply stages
 * the bones through the skin's buffer on the null stream and does the same.  rt_skin_geometry_device is the kernels alone.
 * One apply per skin at a time; a skin's work goes on one stream or is ordered by the caller.
 *
 * Refused with RT_ERR_INVALID_ARG (+ rt_last_error, naming the field) before any HIP call: a NULL pointer (normal may be
 * NULL) or wrong abi_version; n_vertices, tri_count or n_bones 0; n_bones > 65536; tri_first + tri_count > n_triangles; an
 * index >= n_vertices; a bone index >= n_bones in any of the four slots, zero weight or not; a non-finite weight; on apply
 * a NULL scene, skin or bones, a skin whose n_triangles differs from the scene's, a skin on another device than the scene,
 * a progressive render that owns the scene, and what rt_scene_update_device refuses in the delta; in the HOST form only, a
 * non-finite bone member.
 * Out of scope: bone hierarchies (bones are final transforms relative to the rest pose: the caller composes parent chains
 * and inverse binds); morph targets; more than four influences; meshes with normals on some corners only; several skins
 * batched into one update (each apply is one update; the ranges of different skins must not overlap, which is the caller's
 * to ensure); lights and spheres. */
typedef struct rt_skin_desc {
  uint32_t abi_version;           /* RT_ABI_VERSION */
  uint32_t n_vertices;            /* >= 1 */
  uint32_t n_bones;               /* 1 .. 65536 */
  uint32_t tri_first, tri_count;  /* the canonical triangles this mesh IS; tri_count >= 1 */
  uint32_t n_triangles;           /* of the scene the skin is for */
  const float* position;          /* [n_vertices][3] rest */
  const float* normal;            /* [n_vertices][3] rest, or NULL: face normals from the skinned edges */
  const uint32_t* indices;        /* [tri_count][3] */
  const uint16_t* bone;           /* [n_vertices][4] */
  const float* weight;            /* [n_vertices][4] */
} rt_skin_desc;
typedef struct rt_skin rt_skin;

int rt_skin_create(const rt_skin_desc* desc, int device, rt_skin** out);
void rt_skin_destroy(rt_skin* skin);
/* the kernels alone: bones_dev [n_bones] on the skin's device; enqueued on `hip_stream` */
int rt_skin_geometry_device(rt_skin* skin, const rt_transform* bones_dev, void* hip_stream);
/* kernels + rt_scene_update_device on `hip_stream`; blocks as that call does; `info` may be NULL */
int rt_skin_apply_device(rt_scene* scene, rt_skin* skin, const rt_transform* bones_dev, void* hip_stream, rt_update_info* info);
/* host bones [n_bones]; blocks */
int rt_skin_apply(rt_scene* scene, rt_skin* skin, const rt_transform* bones_host, rt_update_info* info);
/* waits for the skin's device work; the arrays as the last kernels left them (before any kernel: the rest mesh): skinned
 * vertices [n_vertices][3], triangle arrays [tri_count][3]; every output nullable; `normal` is not written for a mesh
 * without vertex normals */
int rt_skin_read(rt_skin* skin, float* position, float* normal, float* tri_v1, float* tri_e1, float* tri_e2, float* tri_normal);
/* The host model (no device needed): the same layout as rt_skin_read; every output nullable.  Bones are not checked. */
int rt_skin_model(const rt_skin_desc* desc, const rt_transform* bones, float* position, float* normal, float* tri_v1, float* tri_e1,
                  float* tri_e2, float* tri_normal);

/* ---- SAH report: how good is the tree an update left behind? -----------------------------------------------------------------
 *
 * No reference counterpart.  A refit keeps the topology of creation, so a tree that is deformed without bound decays; this
 * is the number that says by how much.  For every node and every present child, ratio = half_area(child box) / A_root, with
 * half_area(lo, hi) = dx dy + dy dz + dz dx in fp64 (left to right, never fused) and A_root the half area of the union of
 * the root's present child boxes.  q = (uint64_t)(ratio 2^30), truncated; inner_q sums q over inner children, leaf_q sums
 * q n over leaves of n slots; a ratio that is NaN, negative or above 1 counts in n_bad and adds nothing.
 *   sah = (inner_q + tri_cost leaf_q) / 2^30,   tri_cost: rt_bvh_tuning.tri_cost as applied at creation.
 * The sums are 64-bit integers, so the device's are the host model's (rt_sah_packed, csrc/rt_scene_pack.cpp) bit for bit.
 * sah_created is the value of the tree rt_scene_create built, sah_now of the tree as it stands; their ratio is what a
 * caller watches.  A scene without triangles reports 0 for both.
 *
 * The call BLOCKS and runs on a stream of its own (csrc/rt_sah.hip: one thread per node, one atomic add per sum and
 * workgroup).  It only reads the node array, as a query does: it may run while frames render.  It must not overlap an
 * rt_scene_update* / rt_pose_apply* / rt_skin_apply* of the same scene; all block, so this is a rule about the caller's
 * threads only.
 * Out of scope: an automatic rebuild -- the threshold at which rebuilding (rt_scene_rebuild) pays has not been measured. */
typedef struct rt_bvh_quality {
  double sah_created, sah_now;
  uint64_t inner_q, leaf_q; /* the integer sums behind sah_now */
  uint32_t n_bad, reserved;
  double device_ms;
} rt_bvh_quality;
int rt_scene_bvh_quality(rt_scene* scene, rt_bvh_quality* out);

/* ---- BVH rebuild: a new tree for an existing handle, on the device, from the geometry the handle holds right now --------------
 *
 * No reference counterpart.  A refit (rt_scene_update*, rt_pose_apply*, rt_skin_apply*) keeps the topology of creation, so a scene that keeps
 * deforming gets slower; rt_scene_bvh_quality says by how much.  A rebuild replaces the tree without a host round trip: its
 * input is the leaf-slot intersection records of the scene as it stands, nothing comes from the caller.
 *
 * The tree is an LBVH (csrc/rt_lbvh.h): canonical triangle t gets a 30-bit Morton key of its centre, 0.5 (min + max) of its
 * three vertices per axis, quantised to 10 bits per axis inside the bounds of all finite centres; the triangles are sorted
 * by (key, canonical index), the sorted position being the new leaf slot; the hierarchy is Karras' radix tree over the sorted
 * 62-bit values key << 32 | index, in which every range of at most max_leaf triangles (rt_bvh_tuning.max_leaf as applied at
 * creation) becomes one leaf.  The boxes, the per-octant copies, the threaded copy, the scene bounds and the receiver records
 * are then computed by the refit kernels of rt_scene_update.  A host model compiled from the same sources specifies every
 * byte (rt_rebuild_packed, csrc/rt_scene_pack.cpp).  An LBVH splits at Morton cells, not by surface area: on UNDEFORMED
 * geometry it is looser than the binned-SAH tree of rt_scene_create; it pays once a refitted tree has decayed past it
 * (profiles/rebuild.md has the SAH figures).
 *
 * After the call returns, renders and queries behave as on a handle freshly created from the current geometry: hit ids and
 * distances are the same bits; colours agree within the rounding of sums taken in another leaf order.  rt_scene_bvh_info
 * and rt_scene_memory_info describe the new tree; rt_scene_bvh_quality.sah_created stays the value of creation, sah_now is
 * the rebuilt tree's.  Receiver tables, tile costs and queue estimates are invalidated as a geometry update invalidates
 * them (the cell lists hold leaf slots).  rt_pose, rt_skin, rt_ray_order and rt_view handles stay valid: they speak in
 * canonical indices.  Later rt_scene_update* / rt_pose_apply* / rt_skin_apply* calls refit the new tree.
 *
 * Both forms BLOCK: at entry they wait for every frame of this scene still in flight, at exit they synchronise their stream.
 * Ray queries the caller still has in flight on streams of its own are NOT waited for: finish them first.  While the call
 * runs the scene holds a SECOND blob next to the old one, plus 48 bytes of scratch per triangle; the old blob and the
 * scratch are freed before it returns.  Any failure before the swap -- a refusal, an allocation, a HIP error -- leaves the
 * handle exactly as it was.
 *
 * RT_ERR_INVALID_ARG, before any HIP call: NULL scene; a progressive render owns the scene; a scene without triangles
 * ("nothing to rebuild").
 * RT_ERR_UNSUPPORTED: a split-clipped tree (n_references > n_triangles: a clipped reference has no record to rebuild
 * from), also before any HIP call; more than 2^23 - 8 triangles; a rebuilt tree deeper than the traversal stack (max_depth
 * + 2 > 64, the rule of rt_scene_create -- a guard only: a radix tree over 30 key bits and 23 index bits is at most 53 deep).
 * Multi-GPU: the caller rebuilds each per_gpu[i].  A rebuild can lose (profiles/rebuild.md): use rt_scene_rebuild_with and
 * RT_REBUILD_KEEP_BETTER, which compares before it swaps.  Out of scope: an automatic trigger (the numbers of
 * tools/rebuild_bench.py on one scene are not enough to pick a threshold); asynchronous rebuilds; rebuilding with another
 * max_leaf than the one of creation. */
typedef struct rt_rebuild_info {
  double device_ms, total_ms;
  uint32_t n_nodes, n_leaves, max_depth, max_leaf_size; /* of the new tree, as rt_bvh_info */
  uint32_t tables_invalidated;                          /* RT_UPDATE_INVALIDATES_* */
  uint32_t reserved;
} rt_rebuild_info;
/* on a private stream; `info` may be NULL */
int rt_scene_rebuild(rt_scene* scene, rt_rebuild_info* info);
/* the kernels run on `hip_stream` */
int rt_scene_rebuild_device(rt_scene* scene, void* hip_stream, rt_rebuild_info* info);

/* ---- BVH rebuild, the method chosen: an LBVH as above, or PLOC, which clusters by surface area ------------------------------
 *
 * rt_scene_rebuild_with* are rt_scene_rebuild* with a descriptor and a report.  RT_REBUILD_LBVH builds the tree rt_scene_rebuild
 * builds, byte for byte.  RT_REBUILD_PLOC (csrc/rt_ploc.h; Meister & Bittner 2018, parallel locally-ordered clustering)
 * starts from the same Morton order, but builds the hierarchy bottom-up: every cluster looks at the `radius` clusters on
 * either side of it in that order for the one whose common box with it has the smallest surface area, pairs that chose each
 * other merge, and the loop runs until one cluster is left -- tens of iterations of a few short launches, against the
 * LBVH's single pass.  Ties are broken by (position xor position), which is symmetric: the closest pair of all is always
 * mutual, and n identical triangles halve per iteration.  The collapse into leaves of at most max_leaf triangles, the boxes,
 * the copies, the bounds and the receiver records are the LBVH's.  A host model compiled from the same sources specifies
 * every byte (rt_rebuild_ploc_packed, csrc/rt_scene_pack.cpp).  The tree costs less SAH than the LBVH's on meshes and
 * terrains and comes close to the tree of rt_scene_create (profiles/rebuild.md has the figures); it costs more time to
 * build, and on a one-dimensional strip of triangles it is the looser of the two.
 *
 * A rebuild can LOSE: on a scene of a few wall-sized triangles either tree is worse than the refitted tree of creation.
 * RT_REBUILD_KEEP_BETTER makes the call compare before it swaps: the candidate tree is built, the SAH sums of both trees
 * are taken on the device (the kernel and the integers of rt_scene_bvh_quality; both trees bound the same padded triangle
 * boxes, so the two costs share their root area), and a candidate whose SAH is not LOWER is freed: report.swapped = 0,
 * report.info.tables_invalidated = 0, and the handle is exactly as it was, cached receiver tables and queue sizes included.
 * The report is filled either way; `info` describes the tree in place when the call returns, the *_after sums the candidate.
 * An automatic trigger -- when to call this at all -- stays out of scope.
 *
 * Scratch while the call runs, next to the second blob: 48 bytes per triangle for the LBVH, about 160 for PLOC (the sort's
 * 20, a 48-byte node and a 16-byte place for each of the 2n - 1 clusters ever made, 16 for the loop's arrays).
 *
 * RT_ERR_INVALID_ARG, checked on the descriptor before the scene is looked at and before any HIP call (the message names
 * the field): NULL desc, an unknown method, a radius above 32, a radius given for the LBVH, unknown flag bits, reserved != 0.
 * Then everything rt_scene_rebuild refuses.  RT_ERR_UNSUPPORTED, the handle untouched: a PLOC loop of more than 256
 * iterations (a guard: the scenes measured take 6 to 52) and a tree deeper than the traversal stack (max_depth + 2 > 64;
 * PLOC has no depth guarantee, so with it this guard can fire).  `report` may be NULL. */
#define RT_REBUILD_LBVH 0u
#define RT_REBUILD_PLOC 1u
#define RT_REBUILD_KEEP_BETTER 0x1u /* swap only if the candidate's SAH is lower than the tree's in place */
typedef struct rt_rebuild_desc {
  uint32_t method;   /* RT_REBUILD_LBVH / RT_REBUILD_PLOC */
  uint32_t radius;   /* PLOC: 0 = 8, else 1..32; LBVH: must be 0 */
  uint32_t flags;    /* RT_REBUILD_KEEP_BETTER */
  uint32_t reserved; /* 0 */
} rt_rebuild_desc;
typedef struct rt_rebuild_report {
  rt_rebuild_info info; /* of the tree in place when the call returns */
  uint64_t inner_q_before, leaf_q_before, inner_q_after, leaf_q_after; /* rt_bvh_quality's sums; "after" = the candidate's */
  double sah_before, sah_after;
  uint32_t swapped, iterations; /* iterations: of the PLOC loop, 0 for the LBVH */
} rt_rebuild_report;
int rt_scene_rebuild_with(rt_scene* scene, const rt_rebuild_desc* desc, rt_rebuild_report* report);
int rt_scene_rebuild_with_device(rt_scene* scene, const rt_rebuild_desc* desc, void* hip_stream, rt_rebuild_report* report);

/* ---- multi-GPU: tile-partitioned frame + ONE gather of the packed pixels to rank 0 (RCCL over xGMI) ---------
 *
 * Reference: Renderer::render hands RENDER_STRIDE tiles to rayon workers that all write one ImageBuffer
 * (src/renderer/mod.rs:80-94,146-209, src/image_buffer.rs:48-97).  Here rank r renders the tiles with
 * rt_tile_owner(tx, ty, n_ranks) == r on its own GPU (scene replicated), straight into a rank-compact staging
 * buffer; the gather is one ncclGroupStart / ncclRecv x (n-1) on the root, ncclSend on the others / ncclGroupEnd --
 * every peer sends over its own xGMI link, no ring -- followed by a scatter kernel on the root.  No other
 * communication exists on the path.
 *
 * Staging layout (ABI spec): a rank's staging buffer holds its tiles in row-major tile order, each as
 * tile_size x tile_size pixels, row-major inside the tile (edge tiles padded); a staged 0 = "no hit" (the pixel
 * keeps the caller's fill).  rt_gather_layout computes it on the host (no GPU needed). */

/* tile_slot[ty * tiles_x + tx] = index of tile (tx, ty) inside its owner's staging buffer; tiles_per_rank[r] =
 * number of tiles rank r owns.  tiles_x = ceil(width / tile_size).  Either output may be NULL.  tile_size 0 -> 48. */
int rt_gather_layout(uint32_t width, uint32_t height, uint32_t tile_size, uint32_t n_ranks, uint32_t* tile_slot,
                     uint32_t* tiles_per_rank);

/* (a) ONE process drives all GPUs -- the shape of the reference's single-process Renderer::render.  per_gpu[i] is
 * the same scene created on GPU i (rt_scene_create(desc, device_i, ...)); per_gpu[0]'s GPU is the root.  argb is a
 * HOST buffer, W*H, as in rt_render; params->n_ranks / rank are ignored (n_gpu and i are used).  Blocks until argb is
 * complete.  stats (nullable): ray counters summed over the GPUs, kernel_ms = slowest GPU's render, gather_ms, d2h_ms.
 * n_gpu == 1 is rt_render without aux planes.  Scenes on distinct GPUs use RCCL; several scenes on ONE GPU (only
 * useful to rehearse the tile logic on a single-GPU machine) are gathered with device-to-device copies. */
int rt_render_multi(rt_scene* const* per_gpu, int n_gpu, const rt_params* params, uint32_t* argb, rt_stats* stats);
/* The same frame in two halves, for a host that renders frame after frame (the reference's window loop calls render()
 * once per displayed frame, src/main.rs:342-347): `begin` uploads the caller's fill, enqueues every GPU's render and
 * the gather, and returns a ticket (frames with reflections / refractions block until their ray-queue levels are through,
 * as rt_render_device does); `end` waits for that frame and copies it into the argb given to `begin` (which must stay
 * valid until then).  TWO frames may be in flight: the head of frame k+1 fills the compute units that the drain of
 * frame k leaves idle -- a rank's share of a frame is a sub-millisecond launch that cannot end before its longest
 * wavefront does.  A third `begin` before an `end` is refused (RT_ERR_INVALID_ARG).  rt_render_multi = begin + end. */
int rt_render_multi_begin(rt_scene* const* per_gpu, int n_gpu, const rt_params* params, uint32_t* argb, int* ticket);
int rt_render_multi_end(int ticket, rt_stats* stats);
/* frees the communicators / staging buffers rt_render_multi caches between calls.  The cache is deliberately NOT freed
 * at process exit (the HIP / RCCL runtimes may be gone by then); call this to release it earlier. */
void rt_multi_release(void);

/* (b) one process per GPU (torch.distributed / MPI style launchers): rank 0 makes an id, the host ships its 128 bytes
 * to the other ranks by any out-of-band means, every rank creates its communicator (collective call). */
#define RT_COMM_ID_BYTES 128
typedef struct rt_comm rt_comm;
int rt_comm_unique_id(uint8_t id[RT_COMM_ID_BYTES]);
int rt_comm_create(const uint8_t* id, uint32_t n_ranks, uint32_t rank, int device, rt_comm** out); /* n_ranks 1: id may be NULL */
void rt_comm_destroy(rt_comm* comm);
/* Renders this rank's tiles and takes part in the gather; everything is enqueued on hip_stream (the render part
 * blocks only where rt_render_device does, e.g. on the first frame of a shape).  On rank 0
 * argb_dev (DEVICE, W*H, pre-filled by the caller) holds the complete frame once the stream has drained; on the
 * other ranks it is not touched and may be NULL.  params->n_ranks / rank are ignored (the communicator's are used). */
/* The render runs on hip_stream, the gather on a stream the communicator owns (in call order, behind this rank's render);
 * hip_stream then waits for the gather, so work enqueued on it afterwards sees the complete frame.  Staging and receive
 * buffers are double buffered: frame k+1 may be enqueued on ANOTHER stream while frame k drains and travels (two frames
 * in flight; give rank 0 a second argb_dev for it).
 * Failure on one rank: a rank whose render fails still sends its (zeroed) tiles / posts its receives and returns the
 * error afterwards, so its peers are not left waiting; a rank that cannot even set the frame up (invalid arguments,
 * no memory for the staging buffers) aborts the communicator (ncclCommAbort) -- the peers' calls fail instead of hanging,
 * and the communicator must be re-created. */
int rt_render_gather_device(rt_scene* scene, rt_comm* comm, const rt_params* params, uint32_t* argb_dev, void* hip_stream);

#define RT_TRANSPORT_NONE 0u  /* one rank: nothing to gather */
#define RT_TRANSPORT_RCCL 1u  /* ncclSend / ncclRecv */
#define RT_TRANSPORT_LOCAL 2u /* rt_render_multi with several scenes on one GPU: device-to-device copies */
typedef struct rt_gather_info {
  double render_ms;        /* device time of this rank's render kernels in the last call */
  double gather_ms;        /* device time from the end of the render to the end of send / recv (+ scatter on the root) */
  uint64_t bytes_sent;     /* by this rank in the last call */
  uint64_t bytes_received; /* root only */
  uint32_t n_ranks, rank;  /* as RCCL reports them (ncclCommCount / ncclCommUserRank) when transport is RCCL */
  uint32_t tiles_owned;
  uint32_t transport; /* RT_TRANSPORT_* */
} rt_gather_info;
/* timings / sizes of the last rt_render_gather_device on this communicator; call after the stream has drained */
int rt_comm_last_gather(rt_comm* comm, rt_gather_info* out);

#ifdef __cplusplus
}
#endif
#endif /* RT_HIP_H */
