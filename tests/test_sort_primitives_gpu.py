"""The three device primitives under the ray orders, the rebuild and the secondary levels, each on its own: the exclusive
scan and the stable 4-pass radix sort of csrc/rt_order.hip (rt_launch_exclusive_scan, rt_launch_sort_keys) and the hit-point
counting sort of csrc/rt_sort.hip (rt_launch_sort).  A probe links against the built librt_hip.so, so the launches driven
here are the ones that ship; it uploads, launches, synchronises and downloads, and tests/sort_cases.py holds the inputs and
what numpy expects.  Every comparison is array_equal on 32-bit words.

The sizes are the ones at which the code takes another path: the one-workgroup step of the scan (rt_order_tops_kernel, 16
wavefronts, four block sums per thread) holds a non-zero sum in wavefront 1 from 257 blocks on -- a scan of more than
256 * 2048 counts, a sort of more than 2^23 keys -- and in all 1024 threads at 4096 * 2048 counts; the scatter kernel breaks
ties inside a wavefront, across the four wavefronts of a round, and across rounds and tiles; the bases kernel of the counting
sort gives a thread 1, 4 or 16 tiles."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sort_cases as sc
from test_scene_pack_host import CSRC, HIPCC, ROOT
from test_scene_update_kernels_gpu import hip_ok
from hslu_i.ba_raytracing.f2501_raytracer_amd import _lib

gpu = pytest.mark.gpu
U32 = np.uint32
MISUSED = -100  # the probe refused its arguments before any HIP call

PROBE = r'''
#include <hip/hip_runtime.h>
#include <vector>
#include "rt_internal.h"
#include "rt_lbvh.h"
namespace {
hipStream_t stream = nullptr;
std::vector<void*> live;  // every device allocation of the call in progress
int dead = 0;             // the first HIP error, sticky: nothing further is started on the device after it
#define TRY(x)                                                 \
  do {                                                         \
    const hipError_t e_ = (x);                                 \
    if (e_ != hipSuccess) return dead = 1000 + (int)e_;        \
  } while (0)

int begin() {
  if (dead) return dead;
  TRY(hipSetDevice(0));
  if (!stream) TRY(hipStreamCreate(&stream));
  return 0;
}
int dev_alloc(void** p, size_t bytes) {
  *p = nullptr;
  TRY(hipMalloc(p, bytes ? bytes : 4));
  live.push_back(*p);
  return 0;
}
int upload(void** p, const void* src, size_t bytes) {
  const int rc = dev_alloc(p, bytes);
  if (rc) return rc;
  if (bytes) TRY(hipMemcpy(*p, src, bytes, hipMemcpyHostToDevice));
  return 0;
}
int release() {
  if (dead) return dead;
  while (!live.empty()) {
    TRY(hipFree(live.back()));
    live.pop_back();
  }
  return 0;
}
}  // namespace
#define OK(x)                 \
  do {                        \
    const int rc_ = (x);      \
    if (rc_) return rc_;      \
  } while (0)

extern "C" {
int probe_release() {
  OK(release());
  if (stream) {
    TRY(hipStreamDestroy(stream));
    stream = nullptr;
  }
  return 0;
}

// counts[total] -> its exclusive prefix, in place
int probe_scan(uint32_t* counts, uint32_t total) {
  if (!total || total % 8u || total > RT_ORDER_SCAN_BLOCKS * 2048u) return -100;
  OK(begin());
  uint32_t *d, *sums;
  OK(upload((void**)&d, counts, (size_t)total * 4));
  OK(dev_alloc((void**)&sums, RT_ORDER_SCAN_BLOCKS * 4));
  TRY(hipMemsetAsync(sums, 0xFF, RT_ORDER_SCAN_BLOCKS * 4, stream));  // (whatever a scan before left there)
  TRY((hipError_t)rt_launch_exclusive_scan(d, total, sums, stream));
  TRY(hipStreamSynchronize(stream));
  TRY(hipMemcpy(counts, d, (size_t)total * 4, hipMemcpyDeviceToHost));
  return release();
}

// keys[n] -> key_b[n], idx_b[n]; the workspace as rt_rebuild.cpp sizes it
int probe_sort(const uint32_t* keys, uint32_t n, uint32_t* key_b, uint32_t* idx_b) {
  if (!n || n > RT_ORDER_MAX_RAYS) return -100;
  OK(begin());
  const uint32_t n_tiles = (n + RT_ORDER_TILE - 1u) / RT_ORDER_TILE;
  RtOrderWs w{};
  OK(upload((void**)&w.keys, keys, (size_t)n * 4));
  uint32_t** pairs[4] = {&w.key_a, &w.key_b, &w.idx_a, &w.idx_b};
  for (uint32_t** p : pairs) {
    OK(dev_alloc((void**)p, (size_t)n * 4));
    TRY(hipMemsetAsync(*p, 0xFF, (size_t)n * 4, stream));
  }
  OK(dev_alloc((void**)&w.hist, (size_t)256u * n_tiles * 4));
  OK(dev_alloc((void**)&w.sums, RT_ORDER_SCAN_BLOCKS * 4));
  TRY((hipError_t)rt_launch_sort_keys(w, n, stream));
  TRY(hipStreamSynchronize(stream));
  TRY(hipMemcpy(key_b, w.key_b, (size_t)n * 4, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(idx_b, w.idx_b, (size_t)n * 4, hipMemcpyDeviceToHost));
  return release();
}

// The level's rays are [first, n) with n = min(seg_hi or q_in_count, q_capacity), first = min(seg_lo, n) (use_seg: the slice
// pointers are given).  slots: q_capacity {bucket, rank}; hist: the histogram of the hits among those rays; sh_idx: q_capacity
// words, prefilled by the caller.  Refused before any launch unless every position the place kernel can form lies inside
// sh_idx: bucket < 2^sort_bits, rank < hist[bucket], and the histogram sums to at most n - first.
int probe_counting_sort(uint32_t sort_bits, const uint32_t* slots, uint32_t q_in_count, uint32_t q_capacity, int use_seg, uint32_t seg_lo,
                        uint32_t seg_hi, uint32_t n_wgs_place, uint32_t* hist, uint32_t* sh_idx, uint32_t* sort_hits, uint32_t* offs, uint32_t* tile) {
  if (sort_bits < 12u || sort_bits > 24u || !q_capacity) return -100;
  const size_t n_buckets = (size_t)1 << sort_bits, n_tiles = n_buckets / RT_SORT_TILE;
  uint32_t n = use_seg ? seg_hi : q_in_count;
  n = n < q_capacity ? n : q_capacity;
  uint32_t first = use_seg ? seg_lo : 0u;
  first = first < n ? first : n;
  uint64_t sum = 0;
  for (size_t b = 0; b < n_buckets; b++) sum += hist[b];
  if (sum > n - first) return -100;
  for (uint32_t i = first; i < n; i++) {
    const uint32_t b = slots[2 * (size_t)i], r = slots[2 * (size_t)i + 1];
    if (b != 0xFFFFFFFFu && (b >= n_buckets || r >= hist[b])) return -100;
  }
  OK(begin());
  RtDevParams P{};
  P.sort_bits = sort_bits, P.q_capacity = q_capacity;
  uint32_t* words;  // q_in_count, seg_lo, seg_hi, sort_hits
  const uint32_t init[4] = {q_in_count, seg_lo, seg_hi, 0xFFFFFFFFu};
  OK(upload((void**)&words, init, sizeof(init)));
  P.q_in_count = words, P.sort_hits = words + 3;
  if (use_seg) P.seg_lo = words + 1, P.seg_hi = words + 2;
  OK(upload((void**)&P.sort_hist, hist, n_buckets * 4));
  OK(dev_alloc((void**)&P.sort_offs, n_buckets * 4));
  OK(dev_alloc((void**)&P.sort_tile, n_tiles * 4));
  TRY(hipMemsetAsync(P.sort_offs, 0xFF, n_buckets * 4, stream));
  TRY(hipMemsetAsync(P.sort_tile, 0xFF, n_tiles * 4, stream));
  OK(upload((void**)&P.sort_slot, slots, (size_t)q_capacity * 8));
  OK(upload((void**)&P.sh_idx, sh_idx, (size_t)q_capacity * 4));
  TRY(hipStreamSynchronize(stream));
  TRY((hipError_t)rt_launch_sort(P, n_wgs_place, stream));
  TRY(hipStreamSynchronize(stream));
  TRY(hipMemcpy(sh_idx, P.sh_idx, (size_t)q_capacity * 4, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(sort_hits, P.sort_hits, 4, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(hist, P.sort_hist, n_buckets * 4, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(offs, P.sort_offs, n_buckets * 4, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(tile, P.sort_tile, n_tiles * 4, hipMemcpyDeviceToHost));
  return release();
}
}
'''


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("sort_primitives_probe")
    src = d / "probe.cpp"
    src.write_text(PROBE)
    so = d / "probe.so"
    lib_dir, lib_name = os.path.split(os.path.abspath(_lib.LIB_PATH))
    # none of the csrc sources: the launchers and their kernels come from the library under test
    out = subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip", "--cuda-host-only", "-I", CSRC,
                          "-I", os.path.join(ROOT, "include"), "-shared", "-o", str(so), str(src),
                          "-L", lib_dir, f"-l:{lib_name}", f"-Wl,-rpath,{lib_dir}"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lib = C.CDLL(str(so))
    u32 = C.c_uint32
    lib.probe_scan.argtypes = [C.c_void_p, u32]
    lib.probe_sort.argtypes = [C.c_void_p, u32, C.c_void_p, C.c_void_p]
    lib.probe_counting_sort.argtypes = [u32, C.c_void_p, u32, u32, C.c_int, u32, u32, u32] + [C.c_void_p] * 5
    yield lib
    lib.probe_release()


def ptr(a):
    assert a.flags["C_CONTIGUOUS"] and a.dtype == U32
    return a.ctypes.data


def scan(probe, counts):
    out = counts.copy()
    hip_ok(probe.probe_scan(ptr(out), len(out)), "probe_scan")
    return out


def sort(probe, keys):
    key_b, idx_b = np.empty_like(keys), np.empty_like(keys)
    hip_ok(probe.probe_sort(ptr(keys), len(keys), ptr(key_b), ptr(idx_b)), "probe_sort")
    return key_b, idx_b


def counting_sort(probe, case, q_in_count, n_wgs_place, seg=None):
    """-> sh_idx, *sort_hits, sort_hist, sort_offs, sort_tile as the device left them"""
    hist, sh = case.hist.copy(), np.full(case.capacity, sc.SENTINEL, U32)
    hits, offs, tile = np.zeros(1, U32), np.empty(case.n_buckets, U32), np.empty(case.n_tiles, U32)
    lo, hi = seg or (0, 0)
    rc = probe.probe_counting_sort(case.sort_bits, ptr(case.slots), q_in_count, case.capacity, seg is not None, lo, hi, n_wgs_place,
                                   ptr(hist), ptr(sh), ptr(hits), ptr(offs), ptr(tile))
    hip_ok(rc, "probe_counting_sort")
    return sh, int(hits[0]), hist, offs, tile


def test_the_probe_builds_against_the_library(probe):
    """without a GPU: the probe links against the library's three launchers, and refuses arguments that would leave a buffer
    before it makes any HIP call"""
    eight = np.ones(12, U32)
    assert probe.probe_scan(ptr(eight), 12) == MISUSED and probe.probe_scan(ptr(eight), 0) == MISUSED
    assert probe.probe_scan(ptr(eight), 4096 * 2048 + 8) == MISUSED
    assert probe.probe_sort(ptr(eight), 0, ptr(eight), ptr(eight)) == MISUSED
    case = sc.CountingCase(12, 100, seed=1)
    out = [np.zeros(case.n_buckets, U32) for _ in range(4)]
    args = (ptr(case.slots), 100, 100, 0, 0, 0, 1)
    short = case.hist.copy()
    short[case.slots[case.slots[:, 0] != sc.MISS][0, 0]] = 0  # a hit whose rank is not below its bucket's count
    assert probe.probe_counting_sort(12, *args, ptr(short), *map(ptr, out)) == MISUSED
    assert probe.probe_counting_sort(11, *args, ptr(case.hist.copy()), *map(ptr, out)) == MISUSED
    long = case.hist.copy()
    long[7] += 100  # more hits than rays
    assert probe.probe_counting_sort(12, *args, ptr(long), *map(ptr, out)) == MISUSED
    assert probe.probe_release() == 0


# ---- the exclusive scan against a uint64 cumsum --------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("pattern", sc.SCAN_PATTERNS)
@pytest.mark.parametrize("total", sc.SCAN_TOTALS)
def test_exclusive_scan_equals_cumsum(probe, total, pattern):
    counts = sc.scan_counts(total, pattern)
    want, s = sc.scan_expected(counts)
    if pattern == "sum_2_32_minus_1":
        assert s == 2 ** 32 - 1
    got = scan(probe, counts)
    diff = np.flatnonzero(got != want)
    assert diff.size == 0, (f"{total} counts ({-(-total // 2048)} blocks), {pattern}: {diff.size} prefixes differ, the first at {diff[0]} "
                            f"(block {diff[0] // 2048}): device {got[diff[0]]}, numpy {want[diff[0]]}")


# ---- the radix sort against the unique stable order ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("pattern", sc.SORT_PATTERNS)
@pytest.mark.parametrize("n", sc.SORT_SIZES)
def test_radix_sort_is_the_stable_order(probe, n, pattern):
    keys = sc.sort_keys(n, pattern)
    assert keys.dtype == U32 and len(keys) == n
    key_b, idx_b = sort(probe, keys)
    sc.check_stable_sort(keys, key_b, idx_b)


# ---- the counting sort against numpy -------------------------------------------------------------------------------------------
def check_counting_sort(case, got, what):
    sh, hits, hist, offs, tile = got
    assert hits == case.n_hits, f"{what}: *sort_hits {hits}, {case.n_hits} rays hit"
    assert not hist.any(), f"{what}: the histogram is not zero again at {np.flatnonzero(hist)[:5]}"
    assert np.array_equal(tile, case.expected_tile), f"{what}: sort_tile differs at {np.flatnonzero(tile != case.expected_tile)[:5]}"
    assert np.array_equal(offs, case.expected_offs), f"{what}: sort_offs differs at {np.flatnonzero(offs != case.expected_offs)[:5]}"
    diff = np.flatnonzero(sh != case.expected_sh_idx)
    assert diff.size == 0, f"{what}: {diff.size} words of sh_idx differ, the first at {diff[0]}: device {sh[diff[0]]:#x}, numpy {case.expected_sh_idx[diff[0]]:#x}"


@gpu
@pytest.mark.parametrize("single_bucket", [False, True], ids=["uniform", "one_bucket"])
@pytest.mark.parametrize("sort_bits", sc.COUNTING_BITS)
def test_counting_sort_at_every_tile_count(probe, sort_bits, single_bucket):
    n = 20011
    case = sc.CountingCase(sort_bits, n, seed=100 + sort_bits, single_bucket=single_bucket)
    assert case.n_tiles == {12: 1, 13: 2, 20: 256, 22: 1024, 24: 4096}[sort_bits] and 0.7 * n < case.n_hits < 0.8 * n
    assert (case.hist.max() == case.n_hits) == single_bucket
    check_counting_sort(case, counting_sort(probe, case, n, n_wgs_place=(n + 255) // 256), f"{sort_bits} bits")


@gpu
@pytest.mark.parametrize("n,n_wgs_place", [(1, 1), (255, 1), (257, 2), (100003, 1), (100003, 64)])
def test_counting_sort_sizes_and_the_grid_stride_loop(probe, n, n_wgs_place):
    case = sc.CountingCase(22, n, seed=200 + n)
    check_counting_sort(case, counting_sort(probe, case, n, n_wgs_place), f"n {n}, {n_wgs_place} workgroups")


@gpu
def test_counting_sort_clamps_a_counter_beyond_the_capacity(probe):
    """q_in_count counts dropped children too: only the first q_capacity rays exist"""
    capacity = 5000
    case = sc.CountingCase(22, capacity, seed=300)
    check_counting_sort(case, counting_sort(probe, case, capacity + 17, n_wgs_place=8), "q_in_count = q_capacity + 17")


@gpu
def test_counting_sort_of_a_slice(probe):
    """merged levels: the rays are [seg_lo, seg_hi) of one queue, their sorted positions start at seg_lo, the rest is untouched"""
    lo, hi, capacity = 1000, 60000, 70000
    case = sc.CountingCase(22, hi, seed=400, capacity=capacity, first=lo)
    assert (case.expected_sh_idx[:lo] == sc.SENTINEL).all() and (case.expected_sh_idx[lo + case.n_hits:] == sc.SENTINEL).all()
    assert (case.expected_sh_idx[lo:lo + case.n_hits] >= lo).all() and (case.expected_sh_idx[lo:lo + case.n_hits] < hi).all()
    check_counting_sort(case, counting_sort(probe, case, capacity, n_wgs_place=32, seg=(lo, hi)), "slice [1000, 60000)")
