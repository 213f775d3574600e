// rt_order.hip -- the kernels of rt_ray_order_build*: the bounds of a batch's live rays, the key of every ray
// (rt_ray_key.h: the functions of the host model with a thread index), and a full sort of (key, ray index) by key.
//
// The sort is an LSD radix sort, 8 bits per pass, four passes, each pass stable:
//   rt_order_hist_kernel     one workgroup per RT_ORDER_TILE keys: its digit histogram -> hist[digit][workgroup]
//   rt_order_sums / tops / scan_kernel  exclusive prefix over hist in that order = where each workgroup's keys of each digit go
//                            (block sums, one workgroup over the sums, the blocks again)
//   rt_order_scatter_kernel  the same tiles again, 256 keys per round: rank inside the wavefront from ballots and mbcnt,
//                            across the wavefronts of a round and across rounds from counts in LDS
// The size n is a kernel argument (the host knows it); nothing is read back, no kernel waits for another workgroup.
// Contention: a wavefront adds ONE count per distinct digit to the workgroup's LDS histogram (the lowest lane of each
// group of equal digits); global memory sees no atomics at all.  HBM-bound integer work: 20 bytes per ray and pass.
#include <hip/hip_runtime.h>

#include "rt_lbvh.h"  // (rt_ray_key.h; the declarations of rt_launch_sort_keys / rt_launch_exclusive_scan)

namespace {

#define RT_ORDER_WG 256u
#define RT_ORDER_ROUNDS (RT_ORDER_TILE / RT_ORDER_WG)
#define RT_ORDER_SCAN_WG 1024u
#define RT_ORDER_SCAN_BLOCK (RT_ORDER_WG * 8u)  // counts per workgroup of the scan

__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// ---- bounds -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void wave_merge(RtKeyBounds& b) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int a = 0; a < 6; a++) {
      b.lo[a] = rt_min_keep(b.lo[a], __shfl_xor(b.lo[a], off, 64));
      b.hi[a] = rt_max_keep(b.hi[a], __shfl_xor(b.hi[a], off, 64));
    }
    b.n_live += (uint32_t)__shfl_xor((int)b.n_live, off, 64);
  }
}

// the workgroup's bounds, valid in thread 0
__device__ __forceinline__ void block_merge(RtKeyBounds& b, RtKeyBounds* lds /* [4] */) {
  wave_merge(b);
  const uint32_t wave = threadIdx.x >> 6;
  if (lane_id() == 0u) lds[wave] = b;
  __syncthreads();
  if (threadIdx.x == 0u)
    for (uint32_t w = 1; w < RT_ORDER_WG / 64u; w++) rt_key_bounds_merge(b, lds[w]);
}

__global__ __launch_bounds__(RT_ORDER_WG) void rt_order_bounds_kernel(const float* __restrict__ origin, const float* __restrict__ direction,
                                                                      uint32_t n, RtKeyBounds* __restrict__ partial) {
  __shared__ RtKeyBounds lds[RT_ORDER_WG / 64u];
  RtKeyBounds b;
  rt_key_bounds_clear(b);
  for (uint32_t i = blockIdx.x * RT_ORDER_WG + threadIdx.x; i < n; i += gridDim.x * RT_ORDER_WG) {
    const size_t k = 3u * (size_t)i;
    const float o[3] = {origin[k], origin[k + 1], origin[k + 2]}, d[3] = {direction[k], direction[k + 1], direction[k + 2]};
    float c[6];
    if (rt_key_coords(o, d, c)) rt_key_bounds_add(b, c);
  }
  block_merge(b, lds);
  if (threadIdx.x == 0u) partial[blockIdx.x] = b;
}

__global__ __launch_bounds__(RT_ORDER_WG) void rt_order_frame_kernel(const RtKeyBounds* __restrict__ partial, uint32_t n_partial,
                                                                     uint32_t origin_bits, RtKeyFrame* __restrict__ frame) {
  __shared__ RtKeyBounds lds[RT_ORDER_WG / 64u];
  RtKeyBounds b;
  rt_key_bounds_clear(b);
  for (uint32_t i = threadIdx.x; i < n_partial; i += RT_ORDER_WG) rt_key_bounds_merge(b, partial[i]);
  block_merge(b, lds);
  if (threadIdx.x == 0u) {
    RtKeyFrame f;
    rt_key_frame(b, origin_bits, f);
    *frame = f;
  }
}

// ---- keys -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RT_ORDER_WG) void rt_order_keys_kernel(const float* __restrict__ origin, const float* __restrict__ direction,
                                                                    uint32_t n, const RtKeyFrame* __restrict__ frame, uint32_t* __restrict__ keys) {
  const uint32_t i = blockIdx.x * RT_ORDER_WG + threadIdx.x;
  if (i >= n) return;
  const RtKeyFrame f = *frame;  // (uniform: scalar loads)
  const size_t k = 3u * (size_t)i;
  const float o[3] = {origin[k], origin[k + 1], origin[k + 2]}, d[3] = {direction[k], direction[k + 1], direction[k + 2]};
  keys[i] = rt_key_of(f, o, d);
}

// ---- sort ---------------------------------------------------------------------------------------------------------------------
// The lanes of this wavefront that are `on` and hold the same digit as this lane.
__device__ __forceinline__ unsigned long long same_digit(bool on, uint32_t digit) {
  unsigned long long m = __ballot(on);
#pragma unroll
  for (uint32_t b = 0; b < 8u; b++) {
    const bool bit = (digit >> b) & 1u;
    const unsigned long long set = __ballot(on && bit);
    m &= bit ? set : ~set;
  }
  return m;
}
// how many lanes of `m` are below this one (mbcnt)
__device__ __forceinline__ uint32_t lanes_below(unsigned long long m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__global__ __launch_bounds__(RT_ORDER_WG) void rt_order_hist_kernel(const uint32_t* __restrict__ keys, uint32_t n, uint32_t shift,
                                                                    uint32_t* __restrict__ hist, uint32_t n_wgs) {
  __shared__ uint32_t cnt[256];
  cnt[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t base = blockIdx.x * RT_ORDER_TILE;
  for (uint32_t r = 0; r < RT_ORDER_ROUNDS; r++) {
    const uint32_t e = base + r * RT_ORDER_WG + threadIdx.x;
    const bool on = e < n;
    const uint32_t digit = on ? (keys[e] >> shift) & 255u : 0u;
    const unsigned long long m = same_digit(on, digit);
    if (on && lanes_below(m) == 0u) atomicAdd(&cnt[digit], (uint32_t)__popcll(m));  // one LDS add per wavefront and digit
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * n_wgs + blockIdx.x] = cnt[threadIdx.x];
}

// Exclusive prefix over `total` counts (a multiple of 8), in place, in three launches: the sum of every block of
// RT_ORDER_SCAN_BLOCK counts; ONE workgroup's exclusive prefix over those sums (at most RT_ORDER_SCAN_BLOCKS of them: the
// capacity limit of an order); every block again, from its base.  A thread holds 8 consecutive counts (two 16-byte loads).
__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t* lds, uint32_t n_waves, uint32_t* total) {
  uint32_t inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)inc, off, 64);
    if (lane_id() >= (uint32_t)off) inc += o;
  }
  const uint32_t wave = threadIdx.x >> 6;
  if (lane_id() == 63u) lds[wave] = inc;
  __syncthreads();
  uint32_t before = 0u, all = 0u;
  for (uint32_t w = 0; w < n_waves; w++) {
    const uint32_t t = lds[w];
    if (w < wave) before += t;
    all += t;
  }
  *total = all;
  return before + inc - v;
}

__device__ __forceinline__ uint32_t load8(const uint32_t* hist, uint32_t total, uint32_t c[8]) {
  const uint32_t i = (blockIdx.x * RT_ORDER_WG + threadIdx.x) * 8u;
  uint32_t sum = 0u;
  if (i < total) {  // (total is a multiple of 8: all eight or none)
    const uint4 a = *(const uint4*)(hist + i), b = *(const uint4*)(hist + i + 4u);
    c[0] = a.x, c[1] = a.y, c[2] = a.z, c[3] = a.w, c[4] = b.x, c[5] = b.y, c[6] = b.z, c[7] = b.w;
  } else {
#pragma unroll
    for (int k = 0; k < 8; k++) c[k] = 0u;
  }
#pragma unroll
  for (int k = 0; k < 8; k++) sum += c[k];
  return sum;
}

__global__ __launch_bounds__(RT_ORDER_WG) void rt_order_sums_kernel(const uint32_t* __restrict__ hist, uint32_t total, uint32_t* __restrict__ sums) {
  __shared__ uint32_t lds[RT_ORDER_WG / 64u];
  uint32_t c[8], all;
  block_exclusive(load8(hist, total, c), lds, RT_ORDER_WG / 64u, &all);
  if (threadIdx.x == 0u) sums[blockIdx.x] = all;
}

__global__ __launch_bounds__(RT_ORDER_SCAN_WG) void rt_order_tops_kernel(uint32_t* __restrict__ sums, uint32_t n_blocks) {
  __shared__ uint32_t lds[RT_ORDER_SCAN_WG / 64u];
  const uint32_t i = threadIdx.x * 4u;  // n_blocks <= RT_ORDER_SCAN_BLOCKS = 4 per thread
  uint32_t c[4], sum = 0u, all;
#pragma unroll
  for (uint32_t k = 0; k < 4u; k++) c[k] = i + k < n_blocks ? sums[i + k] : 0u, sum += c[k];
  uint32_t run = block_exclusive(sum, lds, RT_ORDER_SCAN_WG / 64u, &all);
#pragma unroll
  for (uint32_t k = 0; k < 4u; k++) {
    if (i + k < n_blocks) sums[i + k] = run;
    run += c[k];
  }
}

__global__ __launch_bounds__(RT_ORDER_WG) void rt_order_scan_kernel(uint32_t* __restrict__ hist, uint32_t total, const uint32_t* __restrict__ sums) {
  __shared__ uint32_t lds[RT_ORDER_WG / 64u];
  uint32_t c[8], all;
  uint32_t run = sums[blockIdx.x] + block_exclusive(load8(hist, total, c), lds, RT_ORDER_WG / 64u, &all);
  const uint32_t i = (blockIdx.x * RT_ORDER_WG + threadIdx.x) * 8u;
  if (i >= total) return;
  uint32_t o[8];
#pragma unroll
  for (int k = 0; k < 8; k++) o[k] = run, run += c[k];
  *(uint4*)(hist + i) = make_uint4(o[0], o[1], o[2], o[3]);
  *(uint4*)(hist + i + 4u) = make_uint4(o[4], o[5], o[6], o[7]);
}

// idx_in == nullptr: the identity (the first pass)
__global__ __launch_bounds__(RT_ORDER_WG) void rt_order_scatter_kernel(const uint32_t* __restrict__ key_in, const uint32_t* __restrict__ idx_in,
                                                                       uint32_t* __restrict__ key_out, uint32_t* __restrict__ idx_out, uint32_t n,
                                                                       uint32_t shift, const uint32_t* __restrict__ hist, uint32_t n_wgs) {
  __shared__ uint32_t run[256];     // where the next key of each digit goes
  __shared__ uint32_t cnt[4][256];  // this round: keys of each digit per wavefront
  run[threadIdx.x] = hist[(size_t)threadIdx.x * n_wgs + blockIdx.x];
#pragma unroll
  for (int w = 0; w < 4; w++) cnt[w][threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t base = blockIdx.x * RT_ORDER_TILE, wave = threadIdx.x >> 6;
  for (uint32_t r = 0; r < RT_ORDER_ROUNDS; r++) {
    if (base + r * RT_ORDER_WG >= n) break;  // (uniform)
    const uint32_t e = base + r * RT_ORDER_WG + threadIdx.x;
    const bool on = e < n;
    const uint32_t key = on ? key_in[e] : 0u;
    const uint32_t idx = on ? (idx_in ? idx_in[e] : e) : 0u;
    const uint32_t digit = (key >> shift) & 255u;
    const unsigned long long m = same_digit(on, digit);
    const uint32_t rank = lanes_below(m);
    if (on && rank == 0u) cnt[wave][digit] = (uint32_t)__popcll(m);
    __syncthreads();
    if (on) {
      uint32_t pos = run[digit] + rank;
      for (uint32_t w = 0; w < wave; w++) pos += cnt[w][digit];
      if (pos < n) key_out[pos] = key, idx_out[pos] = idx;  // (always: the histogram counted these keys)
    }
    __syncthreads();
    uint32_t s = 0u;
#pragma unroll
    for (int w = 0; w < 4; w++) s += cnt[w][threadIdx.x], cnt[w][threadIdx.x] = 0u;
    run[threadIdx.x] += s;
    __syncthreads();
  }
}

}  // namespace

#define RT_ORDER_LAUNCH(kernel, grid, block, ...)                         \
  do {                                                                    \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, __VA_ARGS__); \
    const hipError_t e_ = hipGetLastError();                              \
    if (e_ != hipSuccess) return (int)e_;                                 \
  } while (0)

int rt_launch_exclusive_scan(uint32_t* counts, uint32_t total, uint32_t* sums, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const uint32_t n_blocks = (total + RT_ORDER_SCAN_BLOCK - 1u) / RT_ORDER_SCAN_BLOCK;  // <= RT_ORDER_SCAN_BLOCKS
  RT_ORDER_LAUNCH(rt_order_sums_kernel, n_blocks, RT_ORDER_WG, (const uint32_t*)counts, total, sums);
  RT_ORDER_LAUNCH(rt_order_tops_kernel, 1u, RT_ORDER_SCAN_WG, sums, n_blocks);
  RT_ORDER_LAUNCH(rt_order_scan_kernel, n_blocks, RT_ORDER_WG, counts, total, (const uint32_t*)sums);
  return (int)hipSuccess;
}

int rt_launch_sort_keys(const RtOrderWs& w, uint32_t n, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const uint32_t n_tiles = (n + RT_ORDER_TILE - 1u) / RT_ORDER_TILE;
  const uint32_t* key_in = w.keys;
  const uint32_t* idx_in = nullptr;
  for (uint32_t pass = 0; pass < 4u; pass++) {
    uint32_t* key_out = (pass & 1u) ? w.key_b : w.key_a;
    uint32_t* idx_out = (pass & 1u) ? w.idx_b : w.idx_a;
    RT_ORDER_LAUNCH(rt_order_hist_kernel, n_tiles, RT_ORDER_WG, key_in, n, 8u * pass, w.hist, n_tiles);
    const int e = rt_launch_exclusive_scan(w.hist, 256u * n_tiles, w.sums, stream_);  // (256 n_tiles / 2048 blocks <= RT_ORDER_SCAN_BLOCKS: RT_ORDER_MAX_RAYS)
    if (e != (int)hipSuccess) return e;
    RT_ORDER_LAUNCH(rt_order_scatter_kernel, n_tiles, RT_ORDER_WG, key_in, idx_in, key_out, idx_out, n, 8u * pass, (const uint32_t*)w.hist, n_tiles);
    key_in = key_out, idx_in = idx_out;
  }
  return (int)hipSuccess;
}

int rt_launch_order_build(const RtOrderWs& w, const float* origin, const float* direction, uint32_t n, uint32_t origin_bits, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const uint32_t n_wgs = (n + RT_ORDER_WG - 1u) / RT_ORDER_WG;
  const uint32_t n_partial = n_wgs < RT_ORDER_BOUNDS_WGS ? n_wgs : RT_ORDER_BOUNDS_WGS;
  RT_ORDER_LAUNCH(rt_order_bounds_kernel, n_partial, RT_ORDER_WG, origin, direction, n, w.partial);
  RT_ORDER_LAUNCH(rt_order_frame_kernel, 1u, RT_ORDER_WG, (const RtKeyBounds*)w.partial, n_partial, origin_bits, w.frame);
  RT_ORDER_LAUNCH(rt_order_keys_kernel, n_wgs, RT_ORDER_WG, origin, direction, n, (const RtKeyFrame*)w.frame, w.keys);
  return rt_launch_sort_keys(w, n, stream_);
}
#undef RT_ORDER_LAUNCH
