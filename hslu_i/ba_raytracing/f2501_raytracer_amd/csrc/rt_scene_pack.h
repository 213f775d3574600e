// rt_scene_pack.h -- the device-free half of the host side: what a scene looks like in device memory
// (rt_scene_pack.cpp) and the arithmetic behind a frame's parameter tables (rt_tables.cpp).  Neither file makes a HIP
// call, so both are compiled host-only and checked on the CPU (tests/test_scene_pack_host.py).
// Not part of the public ABI.
#pragma once

#include <vector>

#include "rt_internal.h"

// records the thread-local message of rt_last_error() and returns `code` (rt_scene_pack.cpp)
int rt_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// ---- scene packer ------------------------------------------------------------------------------------------------------
// What an in-place update (rt_scene_update*, rt_refit_packed) needs beyond the blob: the tree's topology in the order a
// refit walks it, and what was decided once at creation.  It lives outside the blob (device copies: rt_scene::plan_dev).
struct RtRefitPlan {
  // node indices grouped by height: first the nodes without an inner child, last the root; the nodes of height h are
  // height_nodes[height_offset[h] .. height_offset[h + 1]), and every inner child of one of them has a smaller height
  std::vector<uint32_t> height_nodes, height_offset;
  std::vector<uint32_t> thr_src;    // per threaded entry: node * 2 + child, the child box it mirrors
  std::vector<uint32_t> recv_cell;  // per canonical triangle: {R, first cell} as allocated at creation
  std::vector<uint32_t> tri_slot;   // per canonical triangle: its first leaf slot
  std::vector<uint8_t> mat_class;   // per material: bit 0 = transmissive at creation, bit 1 = a triangle uses it
  uint32_t receivers_disabled = 0;  // triangles whose receiver record has R = 0 though cells were allocated (last update)
};

// Everything rt_scene_create computes before it touches the device.
struct RtPackedScene {
  std::vector<unsigned char> blob;  // the one allocation the kernels address as base + offset (rt_scene::blob)
  RtDevScene dev{};                 // offsets into `blob` and counts; `base` stays null
  rt_bvh_info info{};
  std::vector<float> flag_geo;      // input of rt_flags_kernel, 12 floats per triangle; empty when n_cells == 0
  uint32_t n_cells = 0;             // receiver cells of triangles and spheres
  uint32_t n_tri_cells = 0;         // ... of which the first n_tri_cells belong to triangles
  size_t bytes_bvh = 0;             // of `blob`: nodes + octant copies + threaded copy
  float aabb_lo[3] = {0.f, 0.f, 0.f}, aabb_hi[3] = {1.f, 1.f, 1.f};  // bounds of everything a ray can hit
  RtRefitPlan plan;
  uint32_t max_leaf = 4;            // rt_bvh_tuning.max_leaf as applied at creation (a rebuild collapses to the same size)
};

// ---- blob layout ------------------------------------------------------------------------------------------------------------
// The one place that decides where the sections of a blob go (rt_pack_scene, rt_rebuild_packed, rt_scene_rebuild*): every
// section on a multiple of 256 bytes with 64 bytes of slack behind it.  Sets every off_* and count of `dev` (base stays) and
// returns the size of the blob, or 0 when it would not stay below 4 GiB.
struct RtBlobCounts {
  uint32_t n_spheres, n_triangles, n_slots, n_nodes, n_thr, n_materials, n_lights;
};
size_t rt_blob_layout(const RtBlobCounts& c, RtDevScene* dev);
// the sections that do not depend on the tree (spheres, their radii and materials, canonical shading records, receiver
// records, sphere receivers, materials, lights): where each lies in one layout and in another
#define RT_BLOB_CANONICAL_SECTIONS 8
struct RtBlobSection {
  size_t from, to, bytes;
};
void rt_blob_canonical_sections(const RtDevScene& from, const RtDevScene& to, uint32_t n_materials, RtBlobSection out[RT_BLOB_CANONICAL_SECTIONS]);

// the checks of an rt_scene_desc that need no device: RT_OK or RT_ERR_INVALID_ARG
int rt_check_scene_desc(const rt_scene_desc* d);
// Lays out a checked description.  `budget` (bytes) bounds the receiver flags and their kernel input.
// RT_OK, or RT_ERR_UNSUPPORTED (2^24 triangle references, 4 GiB of scene data, a BVH deeper than the traversal stack).
int rt_pack_scene(const rt_scene_desc* d, uint64_t budget, RtPackedScene* out);

// ---- in-place updates ------------------------------------------------------------------------------------------------------
// The checks of an rt_scene_delta that need no device, against the scene it is meant for: RT_OK, RT_ERR_INVALID_ARG (the
// message names the field) or RT_ERR_UNSUPPORTED (a triangle group on a split-clipped tree).  `materials_host`: the delta's
// material rows in host memory (null when the delta has none).
int rt_check_scene_delta(const RtDevScene& dev, const RtRefitPlan& plan, const rt_scene_delta* d, const float* materials_host);
// Applies a delta of HOST arrays to a packed scene with the arithmetic of the update kernels (rt_refit.h: the same
// functions): the specification of rt_scene_update, checked on the CPU.  Same return codes as rt_check_scene_delta.
int rt_refit_packed(RtPackedScene* pk, const rt_scene_delta* d);

// ---- rebuild (rt_scene_rebuild*; the tree: rt_lbvh.h) ----------------------------------------------------------------------------
// what a rebuild refuses of a scene, without a device: no triangles (RT_ERR_INVALID_ARG), a split-clipped tree or too many
// triangles (RT_ERR_UNSUPPORTED)
int rt_check_rebuild(const RtDevScene& dev);
// The shape of a rebuilt tree from the counts of phase 1 (`result`: the words RT_LBVH_RES_* of rt_lbvh.h; not read when
// n_triangles <= max_leaf): what the new blob is laid out with, and the plan's groups -- kept nodes by descending depth.
// RT_ERR_UNSUPPORTED for a tree deeper than the traversal stack (the rule of rt_pack_scene).
struct RtRebuildShape {
  uint32_t n_nodes = 0, n_thr = 0, n_leaves = 0, max_leaf_size = 0, max_depth = 0;
  std::vector<uint32_t> group_offset;
};
int rt_rebuild_shape(uint32_t n_triangles, uint32_t max_leaf, const uint32_t* result, RtRebuildShape* out);
void rt_rebuild_info_of(const RtRebuildShape& sh, uint32_t n_triangles, rt_bvh_info* info, size_t* bytes_bvh);
// Rebuilds the tree of a packed scene from the slot records it holds, with the functions of rt_lbvh.h and rt_refit.h -- the
// same functions the kernels are made of: the specification of rt_scene_rebuild, checked on the CPU.  max_leaf as
// rt_bvh_tuning.max_leaf (0 = default).  Any refusal leaves `pk` untouched.
int rt_rebuild_packed(RtPackedScene* pk, uint32_t max_leaf);
// The same with the tree of rt_ploc.h: the specification of rt_scene_rebuild_with(RT_REBUILD_PLOC).  radius as
// rt_rebuild_desc.radius (0 = 8, at most 32: rt_check_ploc_radius); *iterations (may be null): the iterations of the loop,
// 0 for the single root of n_triangles <= max_leaf.  Also refuses a loop of more than RT_PLOC_MAX_ITERATIONS iterations.
int rt_check_ploc_radius(uint32_t radius, uint32_t* applied);
int rt_rebuild_ploc_packed(RtPackedScene* pk, uint32_t max_leaf, uint32_t radius, uint32_t* iterations = nullptr);

// ---- SAH report ------------------------------------------------------------------------------------------------------------
// The two integer sums of rt_sah.h over the tree of a packed scene as it stands: sums[0] = inner_q, sums[1] = leaf_q, and
// the number of refused ratios.  The specification of rt_scene_bvh_quality, checked on the CPU; all zero without triangles.
void rt_sah_packed(const RtPackedScene& pk, uint64_t sums[2], uint32_t* n_bad);

// ---- closest-point queries (rt_closest_points*; the arithmetic and the walk: rt_closest.h) ----------------------------------
// The KERNEL's walk -- spheres, seed descent, threaded walk with rt_closest_may_skip -- over the packed blob for a batch of
// HOST arrays: the same functions rt_closest_kernel is made of, so the pruning is checked on the CPU against the linear scan
// of rt_closest_points_model.
struct RtClosestArgs;
void rt_closest_packed(const RtPackedScene& pk, const RtClosestArgs& a);

// ---- multi-hit ray queries (rt_list_intersections*; the arithmetic and the walk: rt_multihit.h) -----------------------------
// The KERNEL's walk -- spheres, threaded walk with rt_mh_box_enter, passes for `total` -- over the packed blob for a batch of
// HOST arrays: the same functions rt_multihit_kernel is made of, so the pruning is checked on the CPU against the linear scan
// of rt_list_intersections_model.
struct RtMultiHitArgs;
void rt_multihit_packed(const RtPackedScene& pk, const RtMultiHitArgs& a);

// ---- ambient-occlusion queries (rt_ambient_occlusion*; the arithmetic and the walk: rt_occlusion.h) ---------------------------
// The KERNEL's walk -- spheres, threaded walk with rt_mh_box_enter at the limit max_distance, ended at the first hit -- over the
// packed blob for a batch of HOST arrays, one sample after the other: the same functions the kernels are made of, so the
// pruning is checked on the CPU against the linear scan of rt_ambient_occlusion_model.
struct RtOcclusionArgs;
void rt_occlusion_packed(const RtPackedScene& pk, const RtOcclusionArgs& a);

// ---- containment and signed-distance queries (rt_contains_points*, rt_signed_distance*; the arithmetic and the walk: rt_solid.h) --
// what these queries refuse of a scene, without a device: a split-clipped tree (RT_ERR_UNSUPPORTED; the message names the
// reference and triangle counts), as rt_check_scene_delta and rt_check_rebuild do
int rt_check_solid(const RtDevScene& dev, const char* fn);
// The KERNEL's walk -- spheres by their cc, per direction the threaded walk with rt_mh_box_enter at the limit +inf, counting --
// over the packed blob for a batch of HOST arrays: the same functions rt_solid_kernel is made of, so the pruning is checked on
// the CPU against the linear scan of rt_contains_points_model.  With a.signed_distance it reads a.distance, as the kernel does
// (rt_closest_packed writes that plane).  Returns rt_check_solid's code; nothing is written when it refuses.
struct RtSolidArgs;
int rt_solid_packed(const RtPackedScene& pk, const RtSolidArgs& a);

// ---- parameter tables of a frame -----------------------------------------------------------------------------------------
// AA samples: the distinct offsets in first-occurrence order (compared as values; `dedup` off: every sample is distinct),
// their multiplicities and the sample -> thread map, as the device image [2U offsets (float bits) | U | n].  Returns U.
uint32_t rt_build_aa_table(const float* offsets, uint32_t n, bool dedup, std::vector<uint32_t>* table);
// Light clouds: one float4 {dx * fw, dy * fh, dz * fd, 0} per sample position (`cloud`: n_floats = 3 per position), and
// the bounding ball of those offsets: ball[0..2] = its centre, ball[3] = its radius.
void rt_scale_cloud(const float* cloud, size_t n_floats, const float f[3], std::vector<float>* scaled, float ball[4]);
// the beam_* constants of the soft-shadow beam tests from P->cloud_delta and eps_distance
void rt_beam_constants(float eps_distance, RtDevParams* P);
// the frame Morton keys of secondary hit points are taken in: the scene bounds, widened by 1 % on either side
void rt_morton_frame(const float aabb_lo[3], const float aabb_hi[3], float morton_lo[3], float morton_scale[3]);
// The 16x16 super-tiles (window-relative index, row-major) of window win = {x0, y0, w, h} that hold a pixel of a tile of
// `rank`; all of them for n_ranks <= 1.  `cost` (one entry per super-tile of the window, or null): heaviest first.
void rt_super_tiles(const uint32_t win[4], uint32_t tile_size, uint32_t n_ranks, uint32_t rank, const std::vector<uint32_t>* cost,
                    std::vector<uint32_t>* out);
