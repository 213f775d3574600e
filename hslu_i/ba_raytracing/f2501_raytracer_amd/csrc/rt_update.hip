// rt_update.hip -- the kernels of an in-place scene update (rt_scene_update*): one thread per record, each kernel one
// function of rt_refit.h with a thread index, so what they compute is what rt_refit_packed computes on the host.
//
// These are small kernels over a few hundred kilobytes; an update costs launches, not bytes.  The refit goes bottom-up
// with ONE LAUNCH PER HEIGHT of the tree (RtRefitPlan): a launch boundary is the only ordering used, no kernel ever waits
// for another workgroup.
#include <hip/hip_runtime.h>

#include "rt_refit.h"

#define RT_UPD_WG 256u

__global__ __launch_bounds__(RT_UPD_WG) void rt_upd_spheres_kernel(RtDevScene sc, char* base, const float* centre, const float* r_sq) {
  const uint32_t i = blockIdx.x * RT_UPD_WG + threadIdx.x;
  if (i < sc.n_spheres) rt_upd_sphere(sc, base, i, centre, r_sq);
}

__global__ __launch_bounds__(RT_UPD_WG) void rt_upd_slots_kernel(RtDevScene sc, char* base, RtTriDelta d) {
  const uint32_t slot = blockIdx.x * RT_UPD_WG + threadIdx.x;
  if (slot < sc.n_slots) rt_upd_slot(sc, base, slot, d);
}

__global__ __launch_bounds__(RT_UPD_WG) void rt_upd_tris_kernel(RtDevScene sc, char* base, float* geo, RtTriDelta d) {
  const uint32_t k = blockIdx.x * RT_UPD_WG + threadIdx.x;
  if (k < d.count) rt_upd_tri(sc, base, geo, k, d);
}

// the nodes of one height: list[0 .. n)
__global__ __launch_bounds__(RT_UPD_WG) void rt_upd_nodes_kernel(RtDevScene sc, char* base, const uint32_t* list, uint32_t n) {
  const uint32_t i = blockIdx.x * RT_UPD_WG + threadIdx.x;
  if (i < n) rt_upd_node(sc, base, list[i]);
}

__global__ __launch_bounds__(RT_UPD_WG) void rt_upd_octants_kernel(RtDevScene sc, char* base) {
  const uint32_t i = blockIdx.x * RT_UPD_WG + threadIdx.x;
  if (i < sc.n_nodes) rt_upd_octant(sc, base, blockIdx.y, i);
}

__global__ __launch_bounds__(RT_UPD_WG) void rt_upd_threaded_kernel(RtDevScene sc, char* base, const uint32_t* thr_src) {
  const uint32_t i = blockIdx.x * RT_UPD_WG + threadIdx.x;
  if (i < sc.n_thr) rt_upd_thr(sc, base, thr_src, i);
}

// Scene bounds: ONE workgroup strides over the spheres and the leaf slots, then reduces in LDS.  out[0..6) = lo, hi;
// out[6] (bits) = the counter of disabled receivers, cleared here for rt_upd_recv_kernel.
#define RT_UPD_BOUNDS_WG 1024u
__global__ __launch_bounds__(RT_UPD_BOUNDS_WG) void rt_upd_bounds_kernel(RtDevScene sc, const char* base, float* out) {
  __shared__ float red[6][RT_UPD_BOUNDS_WG];
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t i = threadIdx.x; i < sc.n_spheres; i += RT_UPD_BOUNDS_WG) rt_bounds_sphere(sc, base, i, lo, hi);
  for (uint32_t s = threadIdx.x; s < sc.n_slots; s += RT_UPD_BOUNDS_WG) rt_bounds_slot(sc, base, s, lo, hi);
  for (int a = 0; a < 3; a++) red[a][threadIdx.x] = lo[a], red[3 + a][threadIdx.x] = hi[a];
  __syncthreads();
  for (uint32_t w = RT_UPD_BOUNDS_WG / 2u; w > 0u; w >>= 1) {
    if (threadIdx.x < w)
      for (int a = 0; a < 3; a++) {
        red[a][threadIdx.x] = fminf(red[a][threadIdx.x], red[a][threadIdx.x + w]);
        red[3 + a][threadIdx.x] = fmaxf(red[3 + a][threadIdx.x], red[3 + a][threadIdx.x + w]);
      }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    for (int a = 0; a < 3; a++) lo[a] = red[a][0], hi[a] = red[3 + a][0];
    float b[6];
    rt_bounds_finish(lo, hi, b);
    for (int k = 0; k < 6; k++) out[k] = b[k];
    ((uint32_t*)out)[6] = 0u;
  }
}

__global__ __launch_bounds__(RT_UPD_WG) void rt_upd_recv_kernel(RtDevScene sc, char* base, const uint32_t* recv_cell, const uint32_t* tri_slot,
                                                                float* bounds) {
  const uint32_t t = blockIdx.x * RT_UPD_WG + threadIdx.x;
  if (t >= sc.n_triangles) return;
  float b[6];
  for (int k = 0; k < 6; k++) b[k] = bounds[k];
  if (rt_upd_recv(sc, base, recv_cell, tri_slot, b, t)) atomicAdd((uint32_t*)bounds + 6, 1u);
}

__global__ __launch_bounds__(RT_UPD_WG) void rt_upd_materials_kernel(RtDevScene sc, char* base, const float* rows, uint32_t n) {
  const uint32_t i = blockIdx.x * RT_UPD_WG + threadIdx.x;
  if (i < n) rt_upd_material(sc, base, i, rows);
}

__global__ __launch_bounds__(RT_UPD_WG) void rt_upd_lights_kernel(RtDevScene sc, char* base, const float* rows) {
  const uint32_t i = blockIdx.x * RT_UPD_WG + threadIdx.x;
  if (i < sc.n_lights) rt_upd_light(sc, base, i, rows);
}

static inline uint32_t wgs(uint32_t n) { return (n + RT_UPD_WG - 1u) / RT_UPD_WG; }

// Enqueues the kernels of one checked delta (DEVICE arrays) in their order of dependence; returns hipError_t as int.
int rt_launch_update(const RtDevScene& sc, const RtUpdateArgs& u, const rt_scene_delta& d, void* stream_, uint32_t* n_launches) {
  hipStream_t stream = (hipStream_t)stream_;
  uint32_t n = 0;
#define RT_UPD_LAUNCH(kernel, grid, block, ...)                          \
  do {                                                                   \
    hipLaunchKernelGGL(kernel, grid, dim3(block), 0, stream, __VA_ARGS__); \
    const hipError_t e_ = hipGetLastError();                             \
    if (e_ != hipSuccess) return (int)e_;                                \
    n++;                                                                 \
  } while (0)
  if (d.sphere_center && sc.n_spheres) RT_UPD_LAUNCH(rt_upd_spheres_kernel, dim3(wgs(sc.n_spheres)), RT_UPD_WG, sc, u.base, d.sphere_center, d.sphere_r_sq);
  if (d.tri_count) {
    const RtTriDelta td{d.tri_first, d.tri_count, d.tri_v1, d.tri_e1, d.tri_e2, d.tri_normal};
    RT_UPD_LAUNCH(rt_upd_slots_kernel, dim3(wgs(sc.n_slots)), RT_UPD_WG, sc, u.base, td);
    RT_UPD_LAUNCH(rt_upd_tris_kernel, dim3(wgs(td.count)), RT_UPD_WG, sc, u.base, u.flag_geo, td);
    for (uint32_t h = 0; h < u.n_heights; h++) {
      const uint32_t first = u.height_offset[h], cnt = u.height_offset[h + 1] - first;
      if (cnt) RT_UPD_LAUNCH(rt_upd_nodes_kernel, dim3(wgs(cnt)), RT_UPD_WG, sc, u.base, u.height_nodes + first, cnt);
    }
    RT_UPD_LAUNCH(rt_upd_octants_kernel, dim3(wgs(sc.n_nodes), 8), RT_UPD_WG, sc, u.base);
    if (sc.n_thr) RT_UPD_LAUNCH(rt_upd_threaded_kernel, dim3(wgs(sc.n_thr)), RT_UPD_WG, sc, u.base, u.thr_src);
  }
  if (d.sphere_center || d.tri_count) {
    RT_UPD_LAUNCH(rt_upd_bounds_kernel, dim3(1), RT_UPD_BOUNDS_WG, sc, (const char*)u.base, u.bounds);
    if (sc.n_triangles) RT_UPD_LAUNCH(rt_upd_recv_kernel, dim3(wgs(sc.n_triangles)), RT_UPD_WG, sc, u.base, u.recv_cell, u.tri_slot, u.bounds);
  }
  if (d.materials && u.n_materials) RT_UPD_LAUNCH(rt_upd_materials_kernel, dim3(wgs(u.n_materials)), RT_UPD_WG, sc, u.base, d.materials, u.n_materials);
  if (d.lights && sc.n_lights) RT_UPD_LAUNCH(rt_upd_lights_kernel, dim3(wgs(sc.n_lights)), RT_UPD_WG, sc, u.base, d.lights);
  if (n_launches) *n_launches = n;
  return (int)hipSuccess;
}

int rt_launch_refit(const RtDevScene& sc, const RtUpdateArgs& u, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  uint32_t n = 0;
  for (uint32_t h = 0; h < u.n_heights; h++) {
    const uint32_t first = u.height_offset[h], cnt = u.height_offset[h + 1] - first;
    if (cnt) RT_UPD_LAUNCH(rt_upd_nodes_kernel, dim3(wgs(cnt)), RT_UPD_WG, sc, u.base, u.height_nodes + first, cnt);
  }
  RT_UPD_LAUNCH(rt_upd_octants_kernel, dim3(wgs(sc.n_nodes), 8), RT_UPD_WG, sc, u.base);
  if (sc.n_thr) RT_UPD_LAUNCH(rt_upd_threaded_kernel, dim3(wgs(sc.n_thr)), RT_UPD_WG, sc, u.base, u.thr_src);
  RT_UPD_LAUNCH(rt_upd_bounds_kernel, dim3(1), RT_UPD_BOUNDS_WG, sc, (const char*)u.base, u.bounds);
  if (sc.n_triangles) RT_UPD_LAUNCH(rt_upd_recv_kernel, dim3(wgs(sc.n_triangles)), RT_UPD_WG, sc, u.base, u.recv_cell, u.tri_slot, u.bounds);
  (void)n;
  return (int)hipSuccess;
}
#undef RT_UPD_LAUNCH
