"""The inputs of the sort and scan primitive tests (tests/test_sort_primitives_gpu.py) and what numpy expects of them: count
patterns for the exclusive scan of csrc/rt_order.hip, key patterns for its stable radix sort, and (bucket, rank) slots for
the counting sort of csrc/rt_sort.hip.  Everything is seeded; nothing here touches a device."""
import functools

import numpy as np

U32 = np.uint32
SORT_TILE = 4096         # RT_SORT_TILE: buckets per workgroup of the counting sort's offset scan
MISS = 0xFFFFFFFF
SENTINEL = 0xDEADBEEF    # prefill of sh_idx: no ray index of a case reaches it

# ---- the exclusive scan ----------------------------------------------------------------------------------------------------------
# one block and its edge; block sum 256 is the first one wavefront 1 of the tops kernel holds; the rebuild's limit; capacity
SCAN_TOTALS = [8, 2040, 2048, 2056, 256 * 2048 - 8, 256 * 2048, 256 * 2048 + 8, 1024 * 2048 + 8, 4096 * 2048 - 8, 4096 * 2048]
SCAN_PATTERNS = ["uniform", "ones", "last_only", "sum_2_32_minus_1"]


def scan_counts(total, pattern):
    if pattern == "uniform":
        return np.random.default_rng(total).integers(0, 512, total, dtype=np.int64).astype(U32)
    if pattern == "ones":
        return np.ones(total, U32)
    if pattern == "last_only":
        c = np.zeros(total, U32)
        c[-1] = 0xFFFFFFFF
        return c
    if pattern == "sum_2_32_minus_1":  # as even as it goes: every prefix fits, the last inclusive one is 2^32 - 1
        q, r = divmod(2 ** 32 - 1, total)
        c = np.full(total, q, np.uint64)
        c[np.random.default_rng(total + 1).permutation(total)[:r]] += np.uint64(1)
        return c.astype(U32)
    raise KeyError(pattern)


def scan_expected(counts):
    """(the exclusive prefix as uint32, the sum): computed in uint64, and asserted to fit"""
    inc = np.cumsum(counts, dtype=np.uint64)
    assert int(inc[-1]) < 2 ** 32, "the pattern must keep every prefix below 2^32"
    return (inc - counts).astype(U32), int(inc[-1])


# ---- the radix sort ----------------------------------------------------------------------------------------------------------------
# a wavefront, a round of 256, a tile of 4096 and their edges; three tiles; 257 tiles = 33 scan blocks; 2049 tiles = 257 scan
# blocks, the smallest sort whose tops kernel uses a second wavefront
SORT_SIZES = [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 2 * 4096 + 1, (1 << 20) + 3, (1 << 23) + 1]
SORT_PATTERNS = ["equal", "two_values", "byte0", "byte1", "byte2", "byte3", "random", "masked_third", "sorted", "reversed"]
ARGSORT_MAX = (1 << 20) + 3  # up to here idx_b is also compared with numpy's stable argsort


@functools.lru_cache(maxsize=2)
def _random_keys(n):
    return np.random.default_rng(1000 + n).integers(0, 1 << 32, n, dtype=np.uint64).astype(U32)


@functools.lru_cache(maxsize=2)
def _sorted_keys(n):
    return np.sort(_random_keys(n))


def sort_keys(n, pattern):
    if pattern == "equal":
        return np.full(n, 0x5A5AA5A5, U32)
    if pattern == "two_values":
        return np.where(np.arange(n) & 1, U32(0xFFFFFFFF), U32(0)).astype(U32)
    if pattern.startswith("byte"):  # one byte carries the order, the other three passes must be stable no-ops
        b = int(pattern[4])
        r = np.random.default_rng(2000 + 4 * n + b).integers(0, 256, n, dtype=np.int64).astype(U32)
        return (U32(0xA5C3E197) & ~U32(0xFF << (8 * b))) | (r << U32(8 * b))
    if pattern == "random":
        return _random_keys(n).copy()
    if pattern == "masked_third":  # long runs of equal keys across tiles, distinct keys between them
        k = _random_keys(n).copy()
        third = np.random.default_rng(3000 + n).random(n) < 1.0 / 3.0
        k[third] &= U32(0xFF00FF00)
        return k
    if pattern == "sorted":
        return _sorted_keys(n).copy()
    if pattern == "reversed":
        return _sorted_keys(n)[::-1].copy()
    raise KeyError(pattern)


def check_stable_sort(keys, key_b, idx_b):
    """the four O(n) properties that together determine the result: sorted, keys[idx], a permutation, ties by index"""
    n = len(keys)
    assert len(key_b) == len(idx_b) == n
    assert np.all(key_b[1:] >= key_b[:-1]), f"key_b decreases at {np.flatnonzero(key_b[1:] < key_b[:-1])[:5]}"
    assert idx_b.max() < n, "idx_b leaves [0, n)"
    assert np.array_equal(key_b, keys[idx_b]), f"key_b != keys[idx_b] at {np.flatnonzero(key_b != keys[idx_b])[:5]}"
    seen = np.zeros(n, bool)
    seen[idx_b] = True
    assert seen.all(), f"idx_b is not a permutation: {np.flatnonzero(~seen)[:5]} missing"
    unstable = (key_b[1:] == key_b[:-1]) & (idx_b[1:] <= idx_b[:-1])
    assert not unstable.any(), f"equal keys out of index order at sorted positions {np.flatnonzero(unstable)[:5]}"
    if n <= ARGSORT_MAX:
        want = np.argsort(keys, kind="stable").astype(U32)
        diff = np.flatnonzero(idx_b != want)
        assert diff.size == 0, f"first wrong position {diff[0]}: ray {idx_b[diff[0]]}, numpy's stable order has {want[diff[0]]}"


# ---- the counting sort -------------------------------------------------------------------------------------------------------------
COUNTING_BITS = [12, 13, 20, 22, 24]  # n_tiles 1, 2, 256, 1024, 4096: tiles per thread of the bases kernel 1, 1, 1, 4, 16


class CountingCase:
    """`capacity` slots of which the level's rays are [first, n): about a quarter misses, the hits in seeded buckets (uniform,
    or all in one), ranks a seeded permutation inside each bucket.  The slots outside [first, n) look like hits of rank 0 in
    random buckets, so placing one of them would show.  hist / expected_*: the numpy side"""

    def __init__(self, sort_bits, n, seed, capacity=None, first=0, single_bucket=False):
        r = np.random.default_rng(seed)
        self.sort_bits, self.n, self.first = sort_bits, n, first
        self.capacity = capacity = n if capacity is None else capacity
        assert first <= n <= capacity
        n_buckets = self.n_buckets = 1 << sort_bits
        self.n_tiles = n_buckets // SORT_TILE
        bucket = r.integers(0, n_buckets, capacity, dtype=np.int64)
        if single_bucket:
            bucket[first:n] = int(r.integers(SORT_TILE // 2, n_buckets))
        rank = np.zeros(capacity, np.int64)
        live = np.arange(first, n)
        hit = live[r.random(len(live)) >= 0.25] if len(live) > 1 else live
        # a seeded order of the hits, grouped by bucket: the position inside the group is the rank
        order = hit[r.permutation(len(hit))]
        order = order[np.argsort(bucket[order], kind="stable")]
        sorted_b = bucket[order]
        hist = np.bincount(sorted_b, minlength=n_buckets)
        excl = np.cumsum(hist) - hist
        rank[order] = np.arange(len(order)) - excl[sorted_b]
        miss = np.ones(capacity, bool)
        miss[hit] = False
        miss[:first] = miss[n:] = False
        slots = np.stack([np.where(miss, MISS, bucket), rank], 1).astype(U32)
        self.slots, self.hist, self.n_hits = np.ascontiguousarray(slots), hist.astype(U32), len(hit)
        assert (rank[hit] < hist[bucket[hit]]).all() and int(hist.sum()) == len(hit) <= n - first
        sh = np.full(capacity, SENTINEL, U32)
        sh[first + excl[bucket[hit]] + rank[hit]] = hit
        self.expected_sh_idx = sh
        tile_total = hist.reshape(self.n_tiles, SORT_TILE).sum(1)
        tile_base = np.cumsum(tile_total) - tile_total
        self.expected_tile = tile_base.astype(U32)
        self.expected_offs = (excl - np.repeat(tile_base, SORT_TILE)).astype(U32)
