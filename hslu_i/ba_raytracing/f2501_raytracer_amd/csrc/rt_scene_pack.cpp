// rt_scene_pack.cpp -- lays out every byte the kernels read from a scene (RtDevScene, rt_internal.h), on the host and
// without a HIP call: rt_scene_create (rt_api.cpp) uploads what rt_pack_scene returns.  One function per section, in the
// order of the blob.  Also rt_fail / rt_last_error, so that host-only code links without rt_api.cpp.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

#include "rt_closest.h"
#include "rt_lbvh.h"
#include "rt_multihit.h"
#include "rt_occlusion.h"
#include "rt_solid.h"
#include "rt_refit.h"
#include "rt_ploc.h"
#include "rt_sah.h"
#include "rt_scene_pack.h"

static thread_local std::string g_err;

int rt_fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

extern "C" const char* rt_last_error(void) { return g_err.c_str(); }

int rt_check_scene_desc(const rt_scene_desc* d) {
  if (!d) return rt_fail(RT_ERR_INVALID_ARG, "null argument");
  if (d->abi_version != RT_ABI_VERSION)
    return rt_fail(RT_ERR_INVALID_ARG, "rt_scene_desc.abi_version %u != %u", d->abi_version, RT_ABI_VERSION);
  if (d->n_spheres && (!d->sphere_center || !d->sphere_r_sq || !d->sphere_material))
    return rt_fail(RT_ERR_INVALID_ARG, "sphere arrays missing");
  if (d->n_triangles && (!d->tri_v1 || !d->tri_e1 || !d->tri_e2 || !d->tri_normal || !d->tri_material))
    return rt_fail(RT_ERR_INVALID_ARG, "triangle arrays missing");
  if ((d->n_spheres || d->n_triangles) && (!d->n_materials || !d->materials))
    return rt_fail(RT_ERR_INVALID_ARG, "materials missing");
  if (d->n_lights && !d->lights) return rt_fail(RT_ERR_INVALID_ARG, "lights missing");
  for (uint32_t i = 0; i < d->n_spheres; i++)
    if (d->sphere_material[i] >= d->n_materials) return rt_fail(RT_ERR_INVALID_ARG, "sphere %u: material out of range", i);
  for (uint32_t i = 0; i < d->n_triangles; i++)
    if (d->tri_material[i] >= d->n_materials) return rt_fail(RT_ERR_INVALID_ARG, "triangle %u: material out of range", i);
  return RT_OK;
}

// All scene arrays live in ONE device allocation (`blob`): the kernels address them as base + 32-bit byte offset, which
// the scalar loads take as an SGPR offset (2 scalar instructions per address instead of 4, and one base pointer instead
// of nine in SGPRs).  Every section starts on a multiple of 256 bytes.
// rt_blob_layout decides where every section goes; put() fills one.
static void put(std::vector<unsigned char>& blob, const uint32_t* off, const void* src, size_t bytes) {
  if (bytes) memcpy(blob.data() + *off, src, bytes);
}

size_t rt_blob_layout(const RtBlobCounts& c, RtDevScene* dev) {
  size_t at = 0;
  bool fits = true;
  auto place = [&](uint32_t* off, size_t bytes) {
    at = (at + 255) / 256 * 256;
    fits = fits && at < ((size_t)1 << 32);
    *off = (uint32_t)at;
    at += bytes + 64;  // the widest scalar load may read past the last record
  };
  const size_t ns = c.n_spheres, nt = c.n_triangles, n_slots = c.n_slots, nn = c.n_nodes;
  place(&dev->off_spheres, 16 * ns);
  place(&dev->off_sphere_rad, 4 * ns);
  place(&dev->off_sphere_mat, 4 * ns);
  place(&dev->off_tri_isect, 48 * n_slots);
  place(&dev->off_recv, 48 * nt);
  place(&dev->off_srecv, 4 * (2 * ns + 2));
  place(&dev->off_tri_shade, 16 * (n_slots + nt));
  place(&dev->off_tri_id, 4 * n_slots);
  place(&dev->off_nodes, sizeof(RtNode) * nn);
  place(&dev->off_nodes_oct, sizeof(RtNode) * 8 * nn);
  place(&dev->off_nodes_thr, sizeof(RtThrNode) * (size_t)c.n_thr);
  place(&dev->off_materials, 48 * (size_t)c.n_materials);
  place(&dev->off_lights, 32 * (size_t)c.n_lights);
  dev->n_thr = c.n_thr, dev->n_spheres = c.n_spheres, dev->n_triangles = c.n_triangles, dev->n_lights = c.n_lights;
  dev->n_nodes = c.n_nodes, dev->n_slots = c.n_slots;
  return fits && at < ((size_t)1 << 32) ? at : 0;
}

// {cx, cy, cz, r_sq} per sphere, then one float per sphere: an upper bound of the radius (candidate culling)
static void pack_spheres(const rt_scene_desc* d, RtPackedScene* o) {
  const uint32_t ns = d->n_spheres;
  std::vector<float> sp(5 * (size_t)ns);
  for (uint32_t i = 0; i < ns; i++) {
    sp[4 * i + 0] = d->sphere_center[3 * i + 0];
    sp[4 * i + 1] = d->sphere_center[3 * i + 1];
    sp[4 * i + 2] = d->sphere_center[3 * i + 2];
    sp[4 * i + 3] = d->sphere_r_sq[i];
    sp[4 * (size_t)ns + i] = std::sqrt(std::fabs(d->sphere_r_sq[i])) * (1.0f + 4e-7f);
  }
  put(o->blob, &o->dev.off_spheres, sp.data(), 16 * (size_t)ns);
  put(o->blob, &o->dev.off_sphere_rad, sp.data() + 4 * (size_t)ns, 4 * (size_t)ns);
  put(o->blob, &o->dev.off_sphere_mat, d->sphere_material, (size_t)ns * 4);
}

// the tree; no_split[t] = triangle t is transmissive: it must be referenced exactly once (its shadow contributions add up)
static void build_bvh(const rt_scene_desc* d, std::vector<uint8_t>* no_split, RtBvh* bvh) {
  no_split->assign(d->n_triangles, 0);
  for (uint32_t i = 0; i < d->n_triangles; i++) {
    const float* r = d->materials + (size_t)d->tri_material[i] * RT_MATERIAL_STRIDE;
    (*no_split)[i] = (r[RT_MAT_HAS_OPACITY] != 0.0f && !(std::fabs(r[RT_MAT_OPACITY]) <= 1.1920929e-7f)) ? 1 : 0;
  }
  rt_build_bvh(d->tri_v1, d->tri_e1, d->tri_e2, no_split->data(), d->n_triangles, d->bvh, bvh);
}

// bounds of everything a ray can hit (Morton keys of secondary hit points)
static void scene_bounds(const rt_scene_desc* d, float aabb_lo[3], float aabb_hi[3]) {
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  auto grow = [&](float x, float y, float z) {
    const float v[3] = {x, y, z};
    for (int a = 0; a < 3; a++)
      if (std::isfinite(v[a])) lo[a] = std::fmin(lo[a], v[a]), hi[a] = std::fmax(hi[a], v[a]);
  };
  for (uint32_t i = 0; i < d->n_spheres; i++) {
    const float* c = d->sphere_center + 3 * (size_t)i;
    const float r = std::sqrt(std::fabs(d->sphere_r_sq[i]));
    grow(c[0] - r, c[1] - r, c[2] - r), grow(c[0] + r, c[1] + r, c[2] + r);
  }
  for (uint32_t i = 0; i < d->n_triangles; i++) {
    const float *v = d->tri_v1 + 3 * (size_t)i, *a = d->tri_e1 + 3 * (size_t)i, *b = d->tri_e2 + 3 * (size_t)i;
    grow(v[0], v[1], v[2]), grow(v[0] + a[0], v[1] + a[1], v[2] + a[2]), grow(v[0] + b[0], v[1] + b[1], v[2] + b[2]);
  }
  for (int a = 0; a < 3; a++) {
    if (!(lo[a] <= hi[a])) lo[a] = 0.f, hi[a] = 1.f;
    aabb_lo[a] = lo[a], aabb_hi[a] = hi[a];
  }
}

// intersection records in leaf order: {v1, e1, e2, X} of the triangle each slot references
static void pack_isect_records(const rt_scene_desc* d, const RtBvh& bvh, RtPackedScene* o) {
  const uint32_t n_slots = (uint32_t)bvh.tri_order.size();
  std::vector<float> isect(12 * (size_t)n_slots);
  for (uint32_t slot = 0; slot < n_slots; slot++) {
    uint32_t t = bvh.tri_order[slot] & ~RT_TRI_DUPLICATE;
    const float* v1 = d->tri_v1 + 3 * (size_t)t;
    const float* e1 = d->tri_e1 + 3 * (size_t)t;
    const float* e2 = d->tri_e2 + 3 * (size_t)t;
    // X = e1 x e2 in ultraviolet's cross form, bit-equal to cross(-e1, -e2) (triangle.rs:174-177).
    // volatile keeps the host compiler from contracting mul+add into an fma.
    volatile float a0 = e1[1] * e2[2], b0 = e1[2] * e2[1];
    volatile float a1 = e1[2] * e2[0], b1 = e1[0] * e2[2];
    volatile float a2 = e1[0] * e2[1], b2 = e1[1] * e2[0];
    float X[3] = {a0 + (-b0), a1 + (-b1), a2 + (-b2)};
    float* q = &isect[12 * (size_t)slot];
    q[0] = v1[0], q[1] = v1[1], q[2] = v1[2], q[3] = e1[0];
    q[4] = e1[1], q[5] = e1[2], q[6] = e2[0], q[7] = e2[1];
    q[8] = e2[2], q[9] = X[0], q[10] = X[1], q[11] = X[2];
  }
  put(o->blob, &o->dev.off_tri_isect, isect.data(), isect.size() * 4);
}

// One pass of the receiver grid at a given cell size: the receiver record (`q`) and flags-kernel input (`g`) of every
// triangle.  Returns the number of cells.
static uint64_t triangle_cells(const rt_scene_desc* d, double cell, double pmax, std::vector<float>* recv, std::vector<float>* geo) {
  uint64_t total = 0;
  for (uint32_t t = 0; t < d->n_triangles; t++) {
    const float *v1 = d->tri_v1 + 3 * (size_t)t, *e1 = d->tri_e1 + 3 * (size_t)t, *e2 = d->tri_e2 + 3 * (size_t)t;
    const double n[3] = {(double)e1[1] * e2[2] - (double)e1[2] * e2[1], (double)e1[2] * e2[0] - (double)e1[0] * e2[2],
                         (double)e1[0] * e2[1] - (double)e1[1] * e2[0]};
    const double nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
    double l1 = 0, l2 = 0;
    for (int a = 0; a < 3; a++) l1 += (double)e1[a] * e1[a], l2 += (double)e2[a] * e2[a];
    uint32_t Rr = 0;
    float* q = &(*recv)[12 * (size_t)t];
    for (int k = 0; k < 12; k++) q[k] = 0.f;
    if (nn > 0.0 && std::isfinite(nn) && cell > 0.0) {
      Rr = (uint32_t)std::fmin(1024.0, std::fmax(1.0, std::ceil(std::sqrt(std::fmax(l1, l2)) / cell)));
      // u = (p - v1) . (e2 x n) / n.n,  v = (p - v1) . (n x e1) / n.n
      const double au[3] = {(e2[1] * n[2] - e2[2] * n[1]) / nn, (e2[2] * n[0] - e2[0] * n[2]) / nn, (e2[0] * n[1] - e2[1] * n[0]) / nn};
      const double av[3] = {(n[1] * e1[2] - n[2] * e1[1]) / nn, (n[2] * e1[0] - n[0] * e1[2]) / nn, (n[0] * e1[1] - n[1] * e1[0]) / nn};
      const double au0 = -(v1[0] * au[0] + v1[1] * au[1] + v1[2] * au[2]), av0 = -(v1[0] * av[0] + v1[1] * av[1] + v1[2] * av[2]);
      q[0] = (float)au[0], q[1] = (float)au[1], q[2] = (float)au[2], q[3] = (float)au0;
      q[4] = (float)av[0], q[5] = (float)av[1], q[6] = (float)av[2], q[7] = (float)av0;
      for (int k = 0; k < 8; k++)
        if (!std::isfinite(q[k])) Rr = 0;
      // The kernel evaluates the maps in fp32: a sliver's are ill-conditioned.  The cells are computed 5 % larger
      // than they are; keep the error of u * R, v * R below 4 % of a cell (R = 1 needs no coordinates at all).
      const double err = 4e-7 * std::fmax((std::fabs(au[0]) + std::fabs(au[1]) + std::fabs(au[2])) * pmax + std::fabs(au0),
                                          (std::fabs(av[0]) + std::fabs(av[1]) + std::fabs(av[2])) * pmax + std::fabs(av0));
      if (Rr > 1u && err * Rr > 0.04) Rr = (uint32_t)std::fmax(1.0, std::floor(0.04 / err));
    }
    const uint32_t first = (uint32_t)total;
    memcpy(&q[8], &Rr, 4), memcpy(&q[9], &first, 4);
    float* g = &(*geo)[12 * (size_t)t];
    g[0] = v1[0], g[1] = v1[1], g[2] = v1[2], memcpy(&g[3], &Rr, 4);
    g[4] = e1[0], g[5] = e1[1], g[6] = e1[2], memcpy(&g[7], &first, 4);
    g[8] = e2[0], g[9] = e2[1], g[10] = e2[2], g[11] = 0.f;
    total += (uint64_t)Rr * Rr;
  }
  return total;
}

// Receiver cells: every triangle carries an R x R grid over its (u, v) coordinates, cells of about 1/1024 of the scene's
// diagonal (R = 1 for the small triangles of a mesh, up to 1024 for a wall).  The flags themselves depend on the light
// clouds and are computed by rt_flags_kernel when a frame first needs them (prepare()).
// Returns the cell size used, or 0 when not even the coarsest flags fit the budget: no receiver cells at all
// (rt_stats.notes: RT_NOTE_RECV_FLAGS_OFF_SCENE).
static double pack_triangle_receivers(const rt_scene_desc* d, uint64_t budget, RtPackedScene* o) {
  const uint32_t nt = d->n_triangles;
  double diag2 = 0.0, pmax = 0.0;
  for (int a = 0; a < 3; a++) {
    diag2 += (double)(o->aabb_hi[a] - o->aabb_lo[a]) * (o->aabb_hi[a] - o->aabb_lo[a]);
    pmax = std::fmax(pmax, std::fmax(std::fabs((double)o->aabb_lo[a]), std::fabs((double)o->aabb_hi[a])));
  }
  std::vector<float> recv(12 * (size_t)nt);
  std::vector<float>& geo = o->flag_geo;
  geo.assign(12 * (size_t)nt, 0.f);
  // the flags -- 2 bytes per cell, plus their kernel's input of 48 bytes per triangle -- must fit the scene's budget for
  // optional tables, and stay below 2^26 cells = 128 MiB
  auto fits = [&](uint64_t total) { return total <= (1ull << 26) && total * 2u + geo.size() * 4u <= budget; };
  uint64_t total = 0;
  // (a scene of many wall-sized triangles: coarser cells until the flags fit)
  double cell = std::sqrt(diag2) / 1024.0;
  for (;; cell *= 2.0) {
    total = triangle_cells(d, cell, pmax, &recv, &geo);
    if (fits(total)) break;
    if (total <= nt) break;  // (one cell per triangle: coarser does not exist)
  }
  const bool cells_fit = fits(total);
  put(o->blob, &o->dev.off_recv, recv.data(), recv.size() * 4);
  o->n_tri_cells = cells_fit ? (uint32_t)total : 0u;
  return cells_fit ? cell : 0.0;
}

// sphere receivers: a cube map of directions per sphere, cells of about the same size on its surface (`cell`; 0 = none)
static void pack_sphere_receivers(const rt_scene_desc* d, uint64_t budget, double cell, RtPackedScene* o) {
  const uint32_t ns = d->n_spheres;
  const size_t geo_bytes = o->flag_geo.size() * 4u;
  uint64_t total = o->n_tri_cells;
  std::vector<uint32_t> srecv(2 * (size_t)ns + 2, 0u);
  for (uint32_t i = 0; i < ns; i++) {
    const double r = std::sqrt(std::fabs((double)d->sphere_r_sq[i]));
    uint32_t Rs = 0;
    if (std::isfinite(r) && r > 0.0 && cell > 0.0) Rs = (uint32_t)std::fmin(256.0, std::fmax(1.0, std::ceil(1.5708 * r / cell)));
    if (total + 6ull * Rs * Rs > (1ull << 27) || (total + 6ull * Rs * Rs) * 2u + geo_bytes > budget) Rs = 0;
    srecv[2 * i] = Rs, srecv[2 * i + 1] = (uint32_t)total;
    total += 6ull * Rs * Rs;
  }
  put(o->blob, &o->dev.off_srecv, srecv.data(), srecv.size() * 4);
  o->n_cells = (uint32_t)total;
}

// shading records {normal, bits(material row)}: [0, n_slots) leaf order, then canonical order
static void pack_shade_records(const rt_scene_desc* d, const RtBvh& bvh, RtPackedScene* o) {
  const uint32_t nt = d->n_triangles, n_slots = (uint32_t)bvh.tri_order.size();
  std::vector<float> shade(4 * ((size_t)n_slots + nt));
  auto put_shade = [&](size_t dst, uint32_t t) {
    float* sh = &shade[4 * dst];
    sh[0] = d->tri_normal[3 * (size_t)t + 0];
    sh[1] = d->tri_normal[3 * (size_t)t + 1];
    sh[2] = d->tri_normal[3 * (size_t)t + 2];
    uint32_t m = d->tri_material[t];
    memcpy(&sh[3], &m, 4);
  };
  for (uint32_t t = 0; t < nt; t++) put_shade((size_t)n_slots + t, t);
  for (uint32_t slot = 0; slot < n_slots; slot++) put_shade(slot, bvh.tri_order[slot] & ~RT_TRI_DUPLICATE);
  put(o->blob, &o->dev.off_tri_shade, shade.data(), shade.size() * 4);
}

// per-octant copies for the soft-shadow candidate walk: planes pre-selected (lo = entry, hi = exit), the child that is
// entered first along the octant's diagonal stored first
static void pack_octant_nodes(const RtBvh& bvh, RtPackedScene* o) {
  const size_t nn = bvh.nodes.size();
  std::vector<RtNode> oct(8 * nn);
  for (uint32_t oc = 0; oc < 8; oc++)
    for (size_t i = 0; i < nn; i++) {
      const RtNode& src = bvh.nodes[i];
      RtNode d0 = src;
      float key[2] = {0.f, 0.f};
      for (int a = 0; a < 3; a++) {
        const bool neg = (oc >> a) & 1u;
        if (src.c0 != RT_NODE_EMPTY) {
          d0.lo0[a] = neg ? src.hi0[a] : src.lo0[a];
          d0.hi0[a] = neg ? src.lo0[a] : src.hi0[a];
          key[0] += neg ? -src.hi0[a] : src.lo0[a];
        }
        if (src.c1 != RT_NODE_EMPTY) {
          d0.lo1[a] = neg ? src.hi1[a] : src.lo1[a];
          d0.hi1[a] = neg ? src.lo1[a] : src.hi1[a];
          key[1] += neg ? -src.hi1[a] : src.lo1[a];
        }
      }
      if (src.c0 != RT_NODE_EMPTY && src.c1 != RT_NODE_EMPTY && key[1] < key[0]) {
        RtNode sw = d0;
        memcpy(sw.lo0, d0.lo1, 12), memcpy(sw.hi0, d0.hi1, 12), sw.c0 = d0.c1, sw.n0 = d0.n1;
        memcpy(sw.lo1, d0.lo0, 12), memcpy(sw.hi1, d0.hi0, 12), sw.c1 = d0.c0, sw.n1 = d0.n0;
        d0 = sw;
      }
      oct[oc * nn + i] = d0;
    }
  put(o->blob, &o->dev.off_nodes_oct, oct.data(), oct.size() * sizeof(RtNode));
}

// threaded copy (depth first, skip links) for the stackless per-lane walk of incoherent wavefronts
static void pack_threaded_nodes(const RtBvh& bvh, RtPackedScene* o) {
  std::vector<RtThrNode> thr;
  struct Emit {
    const std::vector<RtNode>& nodes;
    std::vector<RtThrNode>& out;
    std::vector<uint32_t>& src;  // RtRefitPlan::thr_src
    void child(uint32_t from, const float* lo, const float* hi, uint32_t c, uint32_t n) {
      if (c == RT_NODE_EMPTY) return;
      src.push_back(from);
      const size_t idx = out.size();
      RtThrNode t;
      memcpy(t.lo, lo, 12), memcpy(t.hi, hi, 12);
      t.skip = 0;
      t.leaf = n ? ((n << 24) | c) : 0u;
      out.push_back(t);
      if (!n) node(c);
      out[idx].skip = (uint32_t)out.size();
    }
    void node(uint32_t i) {
      const RtNode nd = nodes[i];
      child(2 * i, nd.lo0, nd.hi0, nd.c0, nd.n0);
      child(2 * i + 1, nd.lo1, nd.hi1, nd.c1, nd.n1);
    }
  } emit{bvh.nodes, thr, o->plan.thr_src};
  if (!bvh.nodes.empty()) emit.node(0);
  o->dev.n_thr = (uint32_t)thr.size();
  put(o->blob, &o->dev.off_nodes_thr, thr.data(), thr.size() * sizeof(RtThrNode));
}

// 3 x float4 per material: the description's row, then the constants of compute_fresnel
static void pack_materials(const rt_scene_desc* d, RtPackedScene* o) {
  std::vector<float> m(12 * (size_t)d->n_materials, 0.f);
  for (uint32_t i = 0; i < d->n_materials; i++) {
    const float* r = d->materials + (size_t)i * RT_MATERIAL_STRIDE;
    float* q = &m[12 * (size_t)i];
    q[0] = r[RT_MAT_R], q[1] = r[RT_MAT_G], q[2] = r[RT_MAT_B], q[3] = r[RT_MAT_METALLIC];
    q[4] = r[RT_MAT_SHININESS], q[5] = r[RT_MAT_IOR], q[6] = r[RT_MAT_OPACITY], q[7] = r[RT_MAT_BOOST];
    q[8] = r[RT_MAT_HAS_OPACITY];
    // constants of compute_fresnel against other_ior = 1.0 (every shadow ray, raytracer.rs:64-66): the two IEEE
    // divisions of a wave-uniform material would otherwise run on the vector ALU per occluder hit per sample.
    // volatile: no host-side contraction; the same single-precision operations the kernel would execute.
    volatile float ior = r[RT_MAT_IOR], one = 1.0f;
    volatile float inv_ior = one / ior;
    volatile float k = (one - ior) / (one + ior);
    volatile float f0 = k * k;
    q[9] = inv_ior, q[10] = f0;
  }
  put(o->blob, &o->dev.off_materials, m.data(), m.size() * 4);
}

// 2 x float4 per light: {x, y, z, intensity} {r, g, b, 0}
static void pack_lights(const rt_scene_desc* d, RtPackedScene* o) {
  std::vector<float> l(8 * (size_t)d->n_lights, 0.f);
  for (uint32_t i = 0; i < d->n_lights; i++) {
    const float* r = d->lights + (size_t)i * RT_LIGHT_STRIDE;
    float* q = &l[8 * (size_t)i];
    q[0] = r[0], q[1] = r[1], q[2] = r[2], q[3] = r[6];
    q[4] = r[3], q[5] = r[4], q[6] = r[5];
  }
  put(o->blob, &o->dev.off_lights, l.data(), l.size() * 4);
}

// what an update needs to know of the tree and of the decisions of creation (RtRefitPlan)
static void make_refit_plan(const rt_scene_desc* d, const RtBvh& bvh, const std::vector<uint8_t>& no_split, RtPackedScene* o) {
  RtRefitPlan& pl = o->plan;
  const uint32_t nn = (uint32_t)bvh.nodes.size(), nt = d->n_triangles;
  // heights: a child's index is larger than its parent's (the builder reserves a node before it recurses)
  std::vector<uint32_t> height(nn, 0);
  uint32_t top = 0;
  for (uint32_t i = nn; i-- > 0;) {
    const RtNode& nd = bvh.nodes[i];
    if (nd.c0 != RT_NODE_EMPTY && !nd.n0) height[i] = std::max(height[i], height[nd.c0] + 1u);
    if (nd.c1 != RT_NODE_EMPTY && !nd.n1) height[i] = std::max(height[i], height[nd.c1] + 1u);
    top = std::max(top, height[i]);
  }
  pl.height_offset.assign(top + 2u, 0u);
  for (uint32_t i = 0; i < nn; i++) pl.height_offset[height[i] + 1]++;
  for (uint32_t h = 0; h <= top; h++) pl.height_offset[h + 1] += pl.height_offset[h];
  pl.height_nodes.resize(nn);
  std::vector<uint32_t> at(pl.height_offset.begin(), pl.height_offset.end() - 1);
  for (uint32_t i = 0; i < nn; i++) pl.height_nodes[at[height[i]]++] = i;
  const uint32_t* recv = (const uint32_t*)(o->blob.data() + o->dev.off_recv);
  pl.recv_cell.resize(2 * (size_t)nt);
  for (uint32_t t = 0; t < nt; t++) pl.recv_cell[2 * (size_t)t] = recv[12 * (size_t)t + 8], pl.recv_cell[2 * (size_t)t + 1] = recv[12 * (size_t)t + 9];
  pl.tri_slot.assign(nt, 0u);
  for (uint32_t slot = (uint32_t)bvh.tri_order.size(); slot-- > 0;) pl.tri_slot[bvh.tri_order[slot] & ~RT_TRI_DUPLICATE] = slot;
  pl.mat_class.assign(d->n_materials, 0);
  for (uint32_t t = 0; t < nt; t++) pl.mat_class[d->tri_material[t]] = (uint8_t)(2u | (no_split[t] ? 1u : 0u));
}

int rt_check_scene_delta(const RtDevScene& dev, const RtRefitPlan& plan, const rt_scene_delta* d, const float* materials_host) {
  if (!d) return rt_fail(RT_ERR_INVALID_ARG, "null argument");
  if (d->abi_version != RT_ABI_VERSION)
    return rt_fail(RT_ERR_INVALID_ARG, "rt_scene_delta.abi_version %u != %u", d->abi_version, RT_ABI_VERSION);
  const int n_sph = (d->sphere_center != nullptr) + (d->sphere_r_sq != nullptr) + (d->sphere_r_inv != nullptr);
  if (n_sph != 0 && n_sph != 3)
    return rt_fail(RT_ERR_INVALID_ARG, "rt_scene_delta: sphere_center, sphere_r_sq and sphere_r_inv are given together or not at all");
  const int n_tri = (d->tri_v1 != nullptr) + (d->tri_e1 != nullptr) + (d->tri_e2 != nullptr) + (d->tri_normal != nullptr);
  if ((n_tri != 0 && n_tri != 4) || (n_tri == 4) != (d->tri_count != 0))
    return rt_fail(RT_ERR_INVALID_ARG, "rt_scene_delta: tri_v1, tri_e1, tri_e2, tri_normal and a tri_count > 0 are given together or not at all");
  if ((uint64_t)d->tri_first + d->tri_count > dev.n_triangles)
    return rt_fail(RT_ERR_INVALID_ARG, "rt_scene_delta: tri_first %u + tri_count %u > n_triangles %u", d->tri_first, d->tri_count, dev.n_triangles);
  if (!n_sph && !n_tri && !d->materials && !d->lights) return rt_fail(RT_ERR_INVALID_ARG, "rt_scene_delta changes nothing: every group is NULL");
  if (n_tri && dev.n_slots > dev.n_triangles)
    return rt_fail(RT_ERR_UNSUPPORTED, "rt_scene_delta.tri_*: the tree was built with split clipping (%u references of %u triangles); "
                   "clipped boxes cannot be refitted", dev.n_slots, dev.n_triangles);
  if (d->materials && materials_host)
    for (size_t m = 0; m < plan.mat_class.size(); m++)
      if ((plan.mat_class[m] & 2u) && rt_material_transmissive(materials_host + m * RT_MATERIAL_STRIDE) != ((plan.mat_class[m] & 1u) != 0))
        return rt_fail(RT_ERR_INVALID_ARG, "rt_scene_delta.materials: row %zu changes its transmissive class (has_opacity, opacity) "
                       "while triangles use it", m);
  return RT_OK;
}

int rt_refit_packed(RtPackedScene* pk, const rt_scene_delta* d) {
  if (!pk) return rt_fail(RT_ERR_INVALID_ARG, "null argument");
  const int rc = rt_check_scene_delta(pk->dev, pk->plan, d, d ? d->materials : nullptr);
  if (rc != RT_OK) return rc;
  const RtDevScene& sc = pk->dev;
  const RtRefitPlan& pl = pk->plan;
  char* base = (char*)pk->blob.data();
  if (d->sphere_center)
    for (uint32_t i = 0; i < sc.n_spheres; i++) rt_upd_sphere(sc, base, i, d->sphere_center, d->sphere_r_sq);
  if (d->tri_count) {
    const RtTriDelta td{d->tri_first, d->tri_count, d->tri_v1, d->tri_e1, d->tri_e2, d->tri_normal};
    for (uint32_t slot = 0; slot < sc.n_slots; slot++) rt_upd_slot(sc, base, slot, td);
    float* geo = pk->flag_geo.empty() ? nullptr : pk->flag_geo.data();
    for (uint32_t k = 0; k < td.count; k++) rt_upd_tri(sc, base, geo, k, td);
    for (uint32_t i : pl.height_nodes) rt_upd_node(sc, base, i);  // (by height: children before parents)
    for (uint32_t oc = 0; oc < 8; oc++)
      for (uint32_t i = 0; i < sc.n_nodes; i++) rt_upd_octant(sc, base, oc, i);
    for (uint32_t i = 0; i < sc.n_thr; i++) rt_upd_thr(sc, base, pl.thr_src.data(), i);
  }
  if (d->sphere_center || d->tri_count) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, b[6];
    for (uint32_t i = 0; i < sc.n_spheres; i++) rt_bounds_sphere(sc, base, i, lo, hi);
    for (uint32_t s = 0; s < sc.n_slots; s++) rt_bounds_slot(sc, base, s, lo, hi);
    rt_bounds_finish(lo, hi, b);
    memcpy(pk->aabb_lo, b, 12), memcpy(pk->aabb_hi, b + 3, 12);
    pk->plan.receivers_disabled = 0;
    for (uint32_t t = 0; t < sc.n_triangles; t++)
      pk->plan.receivers_disabled += rt_upd_recv(sc, base, pl.recv_cell.data(), pl.tri_slot.data(), b, t) ? 1u : 0u;
  }
  if (d->materials)
    for (uint32_t i = 0; i < (uint32_t)pl.mat_class.size(); i++) rt_upd_material(sc, base, i, d->materials);
  if (d->lights)
    for (uint32_t i = 0; i < sc.n_lights; i++) rt_upd_light(sc, base, i, d->lights);
  return RT_OK;
}

void rt_sah_packed(const RtPackedScene& pk, uint64_t sums[2], uint32_t* n_bad) {
  sums[0] = sums[1] = 0u;
  uint32_t bad = 0u;
  const RtNode* nodes = (const RtNode*)(pk.blob.data() + pk.dev.off_nodes);
  if (pk.dev.n_triangles && pk.dev.n_nodes) {
    const double a_root = rt_sah_root_area(nodes[0]);
    for (uint32_t i = 0; i < pk.dev.n_nodes; i++) rt_sah_node(nodes[i], a_root, sums, &bad);
  }
  if (n_bad) *n_bad = bad;
}

void rt_closest_packed(const RtPackedScene& pk, const RtClosestArgs& a) {
  const char* base = (const char*)pk.blob.data();
  for (size_t i = 0; i < a.n; i++) {
    const float p[3] = {a.point[3 * i], a.point[3 * i + 1], a.point[3 * i + 2]};
    RtClosestHit h;
    rt_closest_query(pk.dev, base, p, a.max_distance ? a.max_distance[i] : INFINITY, true, h);
    rt_closest_store(a, i, h);
  }
}

void rt_multihit_packed(const RtPackedScene& pk, const RtMultiHitArgs& a) {
  const RtMhBlob S = {pk.dev, (const char*)pk.blob.data()};
  for (uint32_t i = 0; i < a.n; i++) rt_mh_query<RT_MH_KMAX>(S, RtMhArgsRef{a}, i, true);
}

void rt_occlusion_packed(const RtPackedScene& pk, const RtOcclusionArgs& a) {
  const RtMhBlob S = {pk.dev, (const char*)pk.blob.data()};
  for (uint32_t i = 0; i < a.n; i++) rt_occ_query_host(S, RtOccArgsRef{a}, i);
}

int rt_check_solid(const RtDevScene& dev, const char* fn) {
  if (dev.n_slots > dev.n_triangles)
    return rt_fail(RT_ERR_UNSUPPORTED, "%s: the tree was built with split clipping (%u references of %u triangles); "
                   "a counting walk would count a triangle once per reference", fn, dev.n_slots, dev.n_triangles);
  return RT_OK;
}

int rt_solid_packed(const RtPackedScene& pk, const RtSolidArgs& a) {
  const int rc = rt_check_solid(pk.dev, "rt_solid_packed");
  if (rc != RT_OK) return rc;
  const RtMhBlob S = {pk.dev, (const char*)pk.blob.data()};
  for (uint32_t i = 0; i < a.n; i++) rt_solid_query(S, RtSolidArgsRef{a}, i, true);
  return RT_OK;
}

int rt_pack_scene(const rt_scene_desc* d, uint64_t budget, RtPackedScene* o) {
  *o = RtPackedScene();
  const uint32_t nt = d->n_triangles;
  RtBvh bvh;
  std::vector<uint8_t> no_split;
  build_bvh(d, &no_split, &bvh);
  const uint32_t n_slots = (uint32_t)bvh.tri_order.size();
  if (n_slots >= (1u << 24)) return rt_fail(RT_ERR_UNSUPPORTED, "more than 2^24 triangle references");
  RtBlobCounts counts{d->n_spheres, nt, n_slots, (uint32_t)bvh.nodes.size(), 0u, d->n_materials, d->n_lights};
  for (const RtNode& nd : bvh.nodes) counts.n_thr += (nd.c0 != RT_NODE_EMPTY) + (nd.c1 != RT_NODE_EMPTY);  // (one threaded entry per child)
  const size_t bytes = rt_blob_layout(counts, &o->dev);
  if (!bytes) return rt_fail(RT_ERR_UNSUPPORTED, "scene data exceeds 4 GiB");
  o->blob.assign(bytes, 0);
  pack_spheres(d, o);
  scene_bounds(d, o->aabb_lo, o->aabb_hi);
  pack_isect_records(d, bvh, o);
  const double cell = pack_triangle_receivers(d, budget, o);
  pack_sphere_receivers(d, budget, cell, o);
  if (!o->n_cells) o->flag_geo.clear();
  pack_shade_records(d, bvh, o);
  // leaf slot -> canonical triangle index, RT_TRI_DUPLICATE as built, RT_TRI_TRANSMISSIVE added here
  std::vector<uint32_t> ids(bvh.tri_order);
  for (uint32_t slot = 0; slot < n_slots; slot++)
    if (no_split[ids[slot] & ~RT_TRI_DUPLICATE]) ids[slot] |= RT_TRI_TRANSMISSIVE;
  put(o->blob, &o->dev.off_tri_id, ids.data(), (size_t)n_slots * 4);
  put(o->blob, &o->dev.off_nodes, bvh.nodes.data(), bvh.nodes.size() * sizeof(RtNode));
  pack_octant_nodes(bvh, o);
  pack_threaded_nodes(bvh, o);
  pack_materials(d, o);
  pack_lights(d, o);
  make_refit_plan(d, bvh, no_split, o);
  if (bvh.max_depth + 2 > 64) return rt_fail(RT_ERR_UNSUPPORTED, "BVH depth %u exceeds the traversal stack", bvh.max_depth);

  o->bytes_bvh = bvh.nodes.size() * sizeof(RtNode) * 9u + (size_t)o->dev.n_thr * sizeof(RtThrNode);
  o->info.n_nodes = (uint32_t)bvh.nodes.size();
  o->info.n_leaves = bvh.n_leaves;
  o->info.max_depth = bvh.max_depth;
  o->info.max_leaf_size = bvh.max_leaf;
  o->info.bytes_nodes = bvh.nodes.size() * sizeof(RtNode);
  o->info.bytes_triangles = (size_t)n_slots * (48 + 16 + 4) + (size_t)nt * 16;
  o->info.n_references = n_slots;
  o->max_leaf = rt_lbvh_max_leaf(d->bvh.max_leaf);
  return RT_OK;
}

// ---- rebuild --------------------------------------------------------------------------------------------------------------------
int rt_check_rebuild(const RtDevScene& dev) {
  if (!dev.n_triangles) return rt_fail(RT_ERR_INVALID_ARG, "rt_scene_rebuild: the scene has no triangles: nothing to rebuild");
  if (dev.n_slots > dev.n_triangles)
    return rt_fail(RT_ERR_UNSUPPORTED, "rt_scene_rebuild: the tree was built with split clipping (%u references of %u triangles); "
                   "clipped boxes cannot be rebuilt from the slot records", dev.n_slots, dev.n_triangles);
  if (dev.n_triangles > RT_LBVH_MAX_TRIANGLES)
    return rt_fail(RT_ERR_UNSUPPORTED, "rt_scene_rebuild: more than %u triangles", RT_LBVH_MAX_TRIANGLES);
  return RT_OK;
}

int rt_rebuild_shape(uint32_t n_triangles, uint32_t max_leaf, const uint32_t* result, RtRebuildShape* out) {
  RtRebuildShape& sh = *out;
  sh = RtRebuildShape();
  if (n_triangles <= max_leaf) {
    sh.n_nodes = 1u, sh.n_thr = 1u, sh.n_leaves = 1u, sh.max_leaf_size = n_triangles, sh.max_depth = 1u;
    sh.group_offset = {0u, 1u};
    return RT_OK;
  }
  const uint32_t deepest = result[RT_LBVH_RES_DEPTH];
  sh.n_nodes = result[RT_LBVH_RES_NODES], sh.n_thr = 2u * sh.n_nodes;
  sh.n_leaves = result[RT_LBVH_RES_LEAVES], sh.max_leaf_size = result[RT_LBVH_RES_LARGEST];
  sh.max_depth = deepest + 1u;  // (the leaves below the deepest kept node: rt_build_bvh's count)
  if (sh.max_depth + 2u > 64u) return rt_fail(RT_ERR_UNSUPPORTED, "rt_scene_rebuild: BVH depth %u exceeds the traversal stack", sh.max_depth);
  // groups by descending depth: every child before its parent
  sh.group_offset.assign(deepest + 1u, 0u);
  for (uint32_t g = 0; g < deepest; g++) sh.group_offset[g + 1u] = sh.group_offset[g] + result[RT_LBVH_RES_HIST + (deepest - 1u - g)];
  return RT_OK;
}

namespace {

// the PLOC loop of rt_ploc.h over n > max_leaf sorted triangles: the nodes, and a place for every kept node and every leaf
struct PlocTree {
  std::vector<RtPlocNode> node;
  std::vector<RtPlocPlace> place;
  uint32_t iterations = 0;
};
int ploc_tree(const RtDevScene& old, const char* old_base, const uint32_t* old_tri_slot, const std::vector<uint32_t>& idx, uint32_t max_leaf,
              uint32_t radius, std::vector<uint32_t>* result, PlocTree* out) {
  const uint32_t n = (uint32_t)idx.size(), n_ids = 2u * n - 1u;
  std::vector<RtPlocNode>& node = out->node;
  node.assign(n_ids, RtPlocNode());
  for (uint32_t x = n; x < n_ids; x++) node[x].parent = RT_LBVH_NONE;
  std::vector<uint32_t> cid[2] = {std::vector<uint32_t>(n), std::vector<uint32_t>(n)}, nn(n), scan(n);
  for (uint32_t s = 0; s < n; s++) rt_ploc_leaf(old, old_base, old_tri_slot[idx[s]], &node[s]), cid[0][s] = s;
  RtPlocState state[2] = {{n, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
  std::vector<float> box;
  uint32_t it = 0;
  for (; state[it & 1u].m > 1u; it++) {
    if (it >= RT_PLOC_MAX_ITERATIONS)
      return rt_fail(RT_ERR_UNSUPPORTED, "rt_scene_rebuild: PLOC did not finish within %u iterations (%u clusters left)", RT_PLOC_MAX_ITERATIONS,
                     state[it & 1u].m);
    const RtPlocState st = state[it & 1u];
    const std::vector<uint32_t>& in = cid[it & 1u];
    const uint32_t m = st.m;
    box.resize(6 * (size_t)m);
    for (uint32_t p = 0; p < m; p++)
      for (int a = 0; a < 3; a++) box[(size_t)a * m + p] = node[in[p]].lo[a], box[(size_t)(3 + a) * m + p] = node[in[p]].hi[a];
    for (uint32_t i = 0; i < m; i++) nn[i] = rt_ploc_nearest(box.data(), m, 0u, m, radius, i);
    uint32_t run = 0;
    for (uint32_t i = 0; i < m; i++) scan[i] = run, run += rt_ploc_survives(nn.data(), m, i) ? 1u : 0u;
    for (uint32_t i = 0; i < m; i++)
      rt_ploc_merge(node.data(), n, in.data(), nn.data(), scan.data(), st, max_leaf, i, cid[(it + 1u) & 1u].data(), &state[(it + 1u) & 1u]);
  }
  out->iterations = state[it & 1u].iterations;
  // the climb, and the counts of phase 1
  std::vector<uint32_t>& res = *result;
  out->place.assign(n_ids, RtPlocPlace());
  res[RT_LBVH_RES_NODES] = node[n_ids - 1u].kept;
  for (uint32_t x = 0; x < n_ids; x++) {
    const bool kept = rt_ploc_keeps(node[x], max_leaf);
    if (!kept && x >= n) continue;
    RtPlocPlace& p = out->place[x];
    rt_ploc_climb(node.data(), x, kept ? RT_PLOC_CLIMB_KEPT : RT_PLOC_CLIMB_LEAF, &p);
    if (!kept) continue;
    res[RT_LBVH_RES_DEPTH] = std::max(res[RT_LBVH_RES_DEPTH], p.depth);
    res[RT_LBVH_RES_HIST + (p.depth - 1u)]++;
    for (int k = 0; k < 2; k++) {
      const RtLbvhChild ch = rt_ploc_child(node.data(), max_leaf, x, p, k);
      if (ch.n) res[RT_LBVH_RES_LEAVES]++, res[RT_LBVH_RES_LARGEST] = std::max(res[RT_LBVH_RES_LARGEST], ch.n);
    }
  }
  return RT_OK;
}

// what rt_rebuild_packed and rt_rebuild_ploc_packed share: keys, layout, gather, refit, info.  radius 0: the LBVH.
int rebuild_packed(RtPackedScene* pk, uint32_t max_leaf, uint32_t radius, uint32_t* iterations) {
  if (!pk) return rt_fail(RT_ERR_INVALID_ARG, "null argument");
  int rc = rt_check_rebuild(pk->dev);
  if (rc != RT_OK) return rc;
  max_leaf = rt_lbvh_max_leaf(max_leaf);
  const RtDevScene& old = pk->dev;
  const char* old_base = (const char*)pk->blob.data();
  const uint32_t n = old.n_triangles;
  const uint32_t* old_tri_slot = pk->plan.tri_slot.data();
  // keys
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  std::vector<float> centre(3 * (size_t)n);
  for (uint32_t t = 0; t < n; t++) {
    float* c = &centre[3 * (size_t)t];
    rt_lbvh_centre((const float*)(old_base + old.off_tri_isect) + 12 * (size_t)old_tri_slot[t], c);
    rt_bounds_grow(lo, hi, c[0], c[1], c[2]);
  }
  std::vector<uint32_t> key_of(n), idx(n), key(n);
  for (uint32_t t = 0; t < n; t++) key_of[t] = rt_lbvh_key(lo, hi, &centre[3 * (size_t)t]), idx[t] = t;
  std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return key_of[a] < key_of[b]; });
  for (uint32_t s = 0; s < n; s++) key[s] = key_of[idx[s]];
  // hierarchy
  std::vector<RtLbvhNode> kn(n);
  std::vector<uint32_t> rank(n, 0u), depth(n, 0u), start(n, 0u), result(RT_LBVH_RES_WORDS, 0u);
  const bool ploc = radius != 0u && n > max_leaf;  // (n <= max_leaf: the single root of either method)
  PlocTree tree;
  if (ploc) {
    rc = ploc_tree(old, old_base, old_tri_slot, idx, max_leaf, radius, &result, &tree);
    if (rc != RT_OK) return rc;
  } else if (n > max_leaf) {
    for (uint32_t i = 0; i + 1u < n; i++) {
      RtLbvhNode nd;
      rt_lbvh_karras(key.data(), idx.data(), n, i, &nd);
      kn[i].f = nd.f, kn[i].l = nd.l, kn[i].split = nd.split;
      if (i == 0u) kn[0].parent = RT_LBVH_NONE;
      if (nd.split > nd.f) kn[nd.split].parent = i;
      if (nd.split + 1u < nd.l) kn[nd.split + 1u].parent = i;
    }
    uint32_t run = 0;
    for (uint32_t i = 0; i < n; i++) rank[i] = run, run += (i + 1u < n && rt_lbvh_keeps(kn[i], max_leaf)) ? 1u : 0u;
    result[RT_LBVH_RES_NODES] = rank[n - 1u];
    for (uint32_t i = 0; i + 1u < n; i++) {
      if (!rt_lbvh_keeps(kn[i], max_leaf)) continue;
      rt_lbvh_climb(kn.data(), rank.data(), max_leaf, i, &depth[i], &start[i]);
      result[RT_LBVH_RES_DEPTH] = std::max(result[RT_LBVH_RES_DEPTH], depth[i]);
      result[RT_LBVH_RES_HIST + (depth[i] - 1u)]++;
      for (int k = 0; k < 2; k++) {
        const RtLbvhChild ch = rt_lbvh_child(rank.data(), max_leaf, kn[i], k);
        if (ch.n) result[RT_LBVH_RES_LEAVES]++, result[RT_LBVH_RES_LARGEST] = std::max(result[RT_LBVH_RES_LARGEST], ch.n);
      }
    }
  }
  RtRebuildShape sh;
  rc = rt_rebuild_shape(n, max_leaf, result.data(), &sh);
  if (rc != RT_OK) return rc;
  // the new blob
  RtPackedScene o;
  const RtBlobCounts counts{old.n_spheres, n, n, sh.n_nodes, sh.n_thr, (uint32_t)pk->plan.mat_class.size(), old.n_lights};
  const size_t bytes = rt_blob_layout(counts, &o.dev);
  if (!bytes) return rt_fail(RT_ERR_UNSUPPORTED, "scene data exceeds 4 GiB");
  o.blob.assign(bytes, 0);
  char* base = (char*)o.blob.data();
  RtBlobSection sec[RT_BLOB_CANONICAL_SECTIONS];
  rt_blob_canonical_sections(old, o.dev, counts.n_materials, sec);
  for (const RtBlobSection& c : sec)
    if (c.bytes) memcpy(base + c.to, old_base + c.from, c.bytes);
  o.plan = pk->plan;
  RtRefitPlan& pl = o.plan;
  pl.height_nodes.assign(sh.n_nodes, 0u), pl.height_offset = sh.group_offset, pl.thr_src.assign(sh.n_thr, 0u);
  for (uint32_t s = 0; s < n; s++) rt_lbvh_gather(old, old_base, old_tri_slot, o.dev, base, pl.tri_slot.data(), ploc ? tree.place[s].first : s, idx[s]);
  if (ploc) {
    std::vector<uint32_t> cursor(RT_LBVH_DEPTH_BINS + 1u, 0u), by_number(sh.n_nodes, 0u);
    for (uint32_t g = 0; g + 1u < sh.group_offset.size(); g++) cursor[sh.max_depth - 2u - g] = sh.group_offset[g];  // (depth k + 1 at k)
    for (uint32_t x = n; x < 2u * n - 1u; x++)
      if (rt_ploc_keeps(tree.node[x], max_leaf)) by_number[tree.place[x].number] = x;
    for (uint32_t x : by_number) {  // (ascending node number inside a group)
      const RtPlocPlace& p = tree.place[x];
      rt_lbvh_emit_pair(rt_ploc_child(tree.node.data(), max_leaf, x, p, 0), rt_ploc_child(tree.node.data(), max_leaf, x, p, 1), p.number, p.start,
                        (RtNode*)(base + o.dev.off_nodes), (RtThrNode*)(base + o.dev.off_nodes_thr), pl.thr_src.data());
      pl.height_nodes[cursor[p.depth - 1u]++] = p.number;
    }
  } else if (n <= max_leaf) {
    rt_lbvh_single_root(n, (RtNode*)(base + o.dev.off_nodes), (RtThrNode*)(base + o.dev.off_nodes_thr), pl.thr_src.data(), pl.height_nodes.data());
  } else {
    std::vector<uint32_t> cursor(RT_LBVH_DEPTH_BINS + 1u, 0u);
    for (uint32_t g = 0; g + 1u < sh.group_offset.size(); g++) cursor[sh.max_depth - 2u - g] = sh.group_offset[g];  // (depth k + 1 at k)
    for (uint32_t i = 0; i + 1u < n; i++) {  // (ascending Karras index = ascending node number: a stable counting sort by depth)
      if (!rt_lbvh_keeps(kn[i], max_leaf)) continue;
      rt_lbvh_emit(rank.data(), max_leaf, kn[i], rank[i], start[i], (RtNode*)(base + o.dev.off_nodes), (RtThrNode*)(base + o.dev.off_nodes_thr),
                   pl.thr_src.data());
      pl.height_nodes[cursor[depth[i] - 1u]++] = rank[i];
    }
  }
  // the boxes: the refit of this topology
  for (uint32_t i : pl.height_nodes) rt_upd_node(o.dev, base, i);
  for (uint32_t oc = 0; oc < 8; oc++)
    for (uint32_t i = 0; i < o.dev.n_nodes; i++) rt_upd_octant(o.dev, base, oc, i);
  for (uint32_t i = 0; i < o.dev.n_thr; i++) rt_upd_thr(o.dev, base, pl.thr_src.data(), i);
  float blo[3] = {INFINITY, INFINITY, INFINITY}, bhi[3] = {-INFINITY, -INFINITY, -INFINITY}, b[6];
  for (uint32_t i = 0; i < o.dev.n_spheres; i++) rt_bounds_sphere(o.dev, base, i, blo, bhi);
  for (uint32_t s = 0; s < o.dev.n_slots; s++) rt_bounds_slot(o.dev, base, s, blo, bhi);
  rt_bounds_finish(blo, bhi, b);
  memcpy(o.aabb_lo, b, 12), memcpy(o.aabb_hi, b + 3, 12);
  pl.receivers_disabled = 0;
  for (uint32_t t = 0; t < n; t++) pl.receivers_disabled += rt_upd_recv(o.dev, base, pl.recv_cell.data(), pl.tri_slot.data(), b, t) ? 1u : 0u;
  // what stays, what follows the new tree
  o.flag_geo = pk->flag_geo, o.n_cells = pk->n_cells, o.n_tri_cells = pk->n_tri_cells, o.max_leaf = pk->max_leaf;
  o.info = pk->info;
  rt_rebuild_info_of(sh, n, &o.info, &o.bytes_bvh);
  *pk = std::move(o);
  if (iterations) *iterations = tree.iterations;
  return RT_OK;
}

}  // namespace

int rt_rebuild_packed(RtPackedScene* pk, uint32_t max_leaf) { return rebuild_packed(pk, max_leaf, 0u, nullptr); }

int rt_check_ploc_radius(uint32_t radius, uint32_t* applied) {
  if (radius > RT_PLOC_MAX_RADIUS) return rt_fail(RT_ERR_INVALID_ARG, "rt_rebuild_desc.radius = %u: at most %u", radius, RT_PLOC_MAX_RADIUS);
  *applied = radius ? radius : RT_PLOC_DEFAULT_RADIUS;
  return RT_OK;
}

int rt_rebuild_ploc_packed(RtPackedScene* pk, uint32_t max_leaf, uint32_t radius, uint32_t* iterations) {
  int rc = rt_check_ploc_radius(radius, &radius);
  if (rc != RT_OK) return rc;
  return rebuild_packed(pk, max_leaf, radius, iterations);
}

void rt_rebuild_info_of(const RtRebuildShape& sh, uint32_t n_triangles, rt_bvh_info* info, size_t* bytes_bvh) {
  info->n_nodes = sh.n_nodes, info->n_leaves = sh.n_leaves, info->max_depth = sh.max_depth, info->max_leaf_size = sh.max_leaf_size;
  info->bytes_nodes = (size_t)sh.n_nodes * sizeof(RtNode);
  info->bytes_triangles = (size_t)n_triangles * (48 + 16 + 4) + (size_t)n_triangles * 16;
  info->n_references = n_triangles;
  *bytes_bvh = (size_t)sh.n_nodes * sizeof(RtNode) * 9u + (size_t)sh.n_thr * sizeof(RtThrNode);
}

void rt_blob_canonical_sections(const RtDevScene& from, const RtDevScene& to, uint32_t n_materials, RtBlobSection out[RT_BLOB_CANONICAL_SECTIONS]) {
  const size_t ns = from.n_spheres, nt = from.n_triangles;
  out[0] = {from.off_spheres, to.off_spheres, 16 * ns};
  out[1] = {from.off_sphere_rad, to.off_sphere_rad, 4 * ns};
  out[2] = {from.off_sphere_mat, to.off_sphere_mat, 4 * ns};
  out[3] = {from.off_tri_shade + 16 * (size_t)from.n_slots, to.off_tri_shade + 16 * (size_t)to.n_slots, 16 * nt};
  out[4] = {from.off_recv, to.off_recv, 48 * nt};
  out[5] = {from.off_srecv, to.off_srecv, 4 * (2 * ns + 2)};
  out[6] = {from.off_materials, to.off_materials, 48 * (size_t)n_materials};
  out[7] = {from.off_lights, to.off_lights, 32 * (size_t)from.n_lights};
}
