// rt_tables.cpp -- the arithmetic behind a frame's parameter tables (AA samples, light clouds, beam constants, Morton
// frame, super-tile list): pure functions of their inputs, no HIP call.  prepare() (rt_api.cpp) decides WHEN a table is
// rebuilt and uploads it.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "rt_scene_pack.h"

uint32_t rt_build_aa_table(const float* offsets, uint32_t n, bool dedup, std::vector<uint32_t>* table) {
  // Distinct offsets in first-occurrence order.  Offsets are compared as VALUES: the origin is pixel + offset,
  // and equal values (+0 / -0 included: the pixel coordinate is never -0) give bit-identical rays.
  std::vector<float> uq;
  std::vector<uint32_t> mult, src(n);
  for (size_t k = 0; k < n; k++) {
    const float x = offsets[2 * k], y = offsets[2 * k + 1];
    size_t j = uq.size() / 2;
    if (dedup)
      for (j = 0; j < uq.size() / 2; j++)
        if (uq[2 * j] == x && uq[2 * j + 1] == y) break;
    if (j == uq.size() / 2) uq.push_back(x), uq.push_back(y), mult.push_back(0);
    mult[j]++;
    src[k] = (uint32_t)j;
  }
  const size_t U = mult.size();
  table->resize(3 * U + n);
  memcpy(table->data(), uq.data(), 2 * U * 4);
  memcpy(table->data() + 2 * U, mult.data(), U * 4);
  memcpy(table->data() + 3 * U, src.data(), (size_t)n * 4);
  return (uint32_t)U;
}

void rt_scale_cloud(const float* cloud, size_t n_floats, const float f[3], std::vector<float>* scaled, float ball[4]) {
  // The device table holds the offsets already multiplied by (fw, fh, fd) (light.rs:218: the same IEEE single
  // multiply the kernel would do, done once here), one float4 per sample position.
  scaled->assign(n_floats / 3 * 4, 0.0f);
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (size_t i = 0; i < n_floats; i++) {
    const float v = cloud[i] * f[i % 3];
    (*scaled)[i / 3 * 4 + i % 3] = v;
    lo[i % 3] = std::fmin(lo[i % 3], v);
    hi[i % 3] = std::fmax(hi[i % 3], v);
  }
  float r2 = 0.f;
  for (int a = 0; a < 3; a++) {
    ball[a] = 0.5f * (lo[a] + hi[a]);
    float h = 0.5f * (hi[a] - lo[a]);
    r2 += h * h;
  }
  ball[3] = std::sqrt(r2) * 1.001f + 1e-6f;
}

void rt_beam_constants(float eps_distance, RtDevParams* P) {
  const float e = eps_distance;
  P->beam_delta = P->cloud_delta + 2.0f * e;
  P->beam_delta_e5 = P->beam_delta + 1e-5f;
  P->beam_eps_push = 0.998f * e;
  P->beam_eps_ulp = (1.3e-7f + 2.5e-6f) * e;
  P->beam_eps_o = 1.01f * e + 2.0f * P->beam_eps_ulp;
  P->beam_eps_198 = 1.98f * e;
}

void rt_morton_frame(const float aabb_lo[3], const float aabb_hi[3], float morton_lo[3], float morton_scale[3]) {
  for (int a = 0; a < 3; a++) {
    const float ext = aabb_hi[a] - aabb_lo[a];
    morton_lo[a] = aabb_lo[a] - 0.01f * ext;
    morton_scale[a] = ext > 0.f ? 1024.0f / (1.02f * ext) : 0.f;
  }
}

void rt_super_tiles(const uint32_t win[4], uint32_t tile_size, uint32_t n_ranks, uint32_t rank, const std::vector<uint32_t>* cost,
                    std::vector<uint32_t>* out) {
  const uint32_t wx0 = win[0], wy0 = win[1], ww = win[2], wh = win[3];
  const uint32_t st_x = (ww + 15u) / 16u, st_y = (wh + 15u) / 16u;
  out->clear();
  for (uint32_t sy = 0; sy < st_y; sy++)
    for (uint32_t sx = 0; sx < st_x; sx++) {
      // a 16x16 super-tile spans at most 2 tiles per axis (tile_size >= 16): its corners decide
      uint32_t x0 = wx0 + sx * 16u, y0 = wy0 + sy * 16u;
      uint32_t x1 = x0 + 15u < wx0 + ww - 1u ? x0 + 15u : wx0 + ww - 1u;
      uint32_t y1 = y0 + 15u < wy0 + wh - 1u ? y0 + 15u : wy0 + wh - 1u;
      bool own = n_ranks <= 1;
      for (uint32_t yy : {y0, y1})
        for (uint32_t xx : {x0, x1}) own = own || rt_tile_owner(xx / tile_size, yy / tile_size, n_ranks) == rank;
      if (own) out->push_back(sy * st_x + sx);
    }
  if (cost && cost->size() == (size_t)st_x * st_y)
    std::stable_sort(out->begin(), out->end(), [&](uint32_t a, uint32_t b) { return (*cost)[a] > (*cost)[b]; });
}
