"""The layouts the handles share (csrc/rt_host.h), checked on the CPU: the arena that carves one allocation into 256-byte
aligned parts, the device copy of the refit plan, and the radix sort's workspace.  Each is written once and used by several
handle types; the numbers here are the formulas those handle types used to write out by hand.  A small
stand-alone program that includes rt_host.h and makes no HIP call prints the offsets; the test restates them in Python."""
import os
import subprocess

import pytest

from test_scene_pack_host import CSRC, HIPCC, ROOT

RT_ORDER_TILE, RT_ORDER_SCAN_BLOCKS = 4096, 4096  # csrc/rt_ray_key.h
ARENA_PARTS = (0, 1, 255, 256, 257, 60)
PLAN_PARTS = (0, 4, 8, 1028)
SORT_KEYS = (1, 4097)  # 4097: one key past a tile, so two tiles of histogram

PROGRAM = r'''
#include <cstdio>
#include "rt_host.h"
int main() {
  RtArena a;
  printf("arena");
  for (size_t bytes : {%(arena)s}) printf(" %%zu", a.add(bytes));
  printf(" %%zu\n", a.total());
  const size_t part[4] = {%(plan)s};
  size_t off[5];
  const size_t total = rt_plan_layout(part, off);
  printf("plan %%zu %%zu %%zu %%zu %%zu %%zu\n", off[0], off[1], off[2], off[3], off[4], total);
  for (size_t n : {%(sort)s}) {
    RtArena lay;
    RtOrderWs ws{};
    rt_sort_ws_add(lay, n, &ws);
    std::vector<char> mem(lay.total());
    lay.bind(mem.data());
    printf("sort");
    for (const uint32_t* p : {ws.keys, ws.key_a, ws.key_b, ws.idx_a, ws.idx_b, ws.hist, ws.sums}) printf(" %%td", (const char*)p - mem.data());
    printf(" %%zu\n", lay.total());
  }
  return 0;
}
'''


def pad256(n):
    return (n + 255) // 256 * 256


def laid_out(parts):
    """(offsets, total) of parts that follow one another, each padded to 256 bytes"""
    offsets, at = [], 0
    for bytes_ in parts:
        offsets.append(at)
        at += pad256(bytes_)
    return offsets, at


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("host_layout")
    src, exe = d / "layout.cpp", d / "layout"
    join = lambda v: ", ".join(f"(size_t){x}" for x in v)
    src.write_text(PROGRAM % {"arena": join(ARENA_PARTS), "plan": join(PLAN_PARTS), "sort": join(SORT_KEYS)})
    out = subprocess.run([HIPCC, "-O2", "-std=c++17", "-Wall", "-x", "hip", "--cuda-host-only", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                          "-o", str(exe), str(src)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr[-3000:]
    print(run.stdout)
    return [[int(w) for w in l.split()[1:]] for l in run.stdout.splitlines()], [l.split()[0] for l in run.stdout.splitlines()]


def test_arena_parts_start_on_256_bytes_and_an_empty_part_takes_none(lines):
    rows, names = lines
    assert names[0] == "arena"
    assert rows[0] == [0, 0, 256, 512, 768, 1280, 1536]
    offsets, total = laid_out(ARENA_PARTS)
    assert rows[0] == offsets + [total]


def test_plan_layout_is_the_one_scenes_and_rebuilds_wrote_by_hand(lines):
    """before: `for k < 4: off[k] = bytes, bytes += (part[k] + 255) / 256 * 256;  off[4] = bytes, bytes += 256` in
    rt_scene_upload_plan, and the same with rt_pad256 in rt_rebuild_device"""
    rows, names = lines
    assert names[1] == "plan"
    assert rows[1] == [0, 0, 256, 512, 1792, 2048]
    off, at = [], 0
    for k in range(4):
        off.append(at)
        at += (PLAN_PARTS[k] + 255) // 256 * 256
    off.append(at)
    at += 256
    assert rows[1] == off + [at]


@pytest.mark.parametrize("k", range(len(SORT_KEYS)))
def test_sort_workspace_is_five_key_arrays_the_histogram_and_the_block_sums(lines, k):
    """before: keys, key_a, key_b, idx_a, idx_b at multiples of pad256(4 n), hist at 5 of them, sums behind pad256(256 *
    n_tiles * 4), in order_alloc and in rt_rebuild_device"""
    rows, names = lines
    n = SORT_KEYS[k]
    assert names[2 + k] == "sort"
    n_tiles = (n + RT_ORDER_TILE - 1) // RT_ORDER_TILE
    assert n_tiles == (1, 2)[k]
    per = pad256(4 * n)
    want = [0, per, 2 * per, 3 * per, 4 * per, 5 * per, 5 * per + pad256(256 * n_tiles * 4)]
    total = want[-1] + pad256(RT_ORDER_SCAN_BLOCKS * 4)
    assert rows[2 + k] == want + [total]
    offsets, end = laid_out([4 * n] * 5 + [256 * n_tiles * 4, RT_ORDER_SCAN_BLOCKS * 4])
    assert (offsets, end) == (want, total)  # each part starts where the one before it ended
