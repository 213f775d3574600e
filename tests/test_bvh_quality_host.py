"""The host model of the SAH report (rt_sah_packed, csrc/rt_scene_pack.cpp: the functions of csrc/rt_sah.h in a loop -- the
same functions rt_sah_kernel is made of) checked on the CPU with a host-only probe, compiled and linked as
test_scene_update_host.py compiles its own.  The two sums are 64-bit integers and n_bad a count: every check is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scene_update_cases as cases
import test_scene_update_host as T
from test_scene_pack_host import CSRC, EMPTY, HIPCC, ROOT, ptr

PROBE = T.PROBE + r'''
extern "C" void probe_sah(int k, uint64_t* sums, uint32_t* n_bad) { rt_sah_packed(g[k], sums, n_bad); }
'''
TRI_COST = 2.0  # rt_bvh_tuning.tri_cost as applied when the description leaves it 0


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("sah_probe")
    src = d / "probe.cpp"
    src.write_text(PROBE)
    so = d / "probe.so"
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip", "--cuda-host-only", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), "-shared", "-o", str(so), str(src)] +
                   [os.path.join(CSRC, f) for f in ("rt_scene_pack.cpp", "rt_tables.cpp", "rt_bvh.cpp")],
                   check=True, capture_output=True, timeout=600)
    lib = C.CDLL(str(so))
    lib.probe_error.restype = C.c_char_p
    return lib


def sah_packed(probe, k):
    sums, bad = np.zeros(2, np.uint64), np.zeros(1, np.uint32)
    probe.probe_sah(k, ptr(sums), ptr(bad))
    return int(sums[0]), int(sums[1]), int(bad[0])


def sah_value(inner_q, leaf_q, tri_cost=TRI_COST):
    return (float(inner_q) + tri_cost * float(leaf_q)) / 2.0 ** 30


def sah_numpy(p):
    """csrc/rt_sah.h restated over the blob's nodes in numpy float64 -> (inner_q, leaf_q, n_bad)"""
    if not p.dev["n_triangles"]:
        return 0, 0, 0
    nodes = T.section(p, "off_nodes", p.dev["n_nodes"], 16)
    f = nodes.view(np.float32).astype(np.float64)

    def half_area(lo, hi):
        d = hi - lo
        return d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0]

    lo = np.stack([f[:, 0:3], f[:, 8:11]], 1)   # [node, child, axis]
    hi = np.stack([f[:, 4:7], f[:, 12:15]], 1)
    c = np.stack([nodes[:, 3], nodes[:, 11]], 1)
    n = np.stack([nodes[:, 7], nodes[:, 15]], 1).astype(np.uint64)
    present = c != EMPTY
    root = present[0]
    a_root = half_area(lo[0][root].min(0), hi[0][root].max(0))
    with np.errstate(all="ignore"):
        ratio = half_area(lo, hi) / a_root
        ok = present & (ratio >= 0.0) & (ratio <= 1.0)
        q = np.where(ok, ratio * 2.0 ** 30, 0.0).astype(np.uint64)  # (truncates)
    inner = int(q[ok & (n == 0)].sum(dtype=np.uint64))
    leaf = int((q * n)[ok & (n != 0)].sum(dtype=np.uint64))
    return inner, leaf, int((present & ~ok).sum())


@pytest.mark.parametrize("name", sorted(T.SCENES))
def test_sums_equal_the_numpy_restatement(probe, name):
    flat = T.SCENES[name]()
    p = T.pack(probe, 0, flat)
    got = sah_packed(probe, 0)
    assert got == sah_numpy(p), name
    nodes = T.section(p, "off_nodes", p.dev["n_nodes"], 16)
    print(f"{name}: {p.dev['n_nodes']} nodes, inner_q {got[0]}, leaf_q {got[1]}, n_bad {got[2]}, sah {sah_value(*got[:2]):.4f}")
    if name == "empty":
        assert got == (0, 0, 0)
    elif name == "one_triangle":  # a one-leaf tree: the root's first child is the leaf, its second is absent
        assert p.dev["n_nodes"] == 1 and nodes[0, 7] == 1 and nodes[0, 11] == EMPTY
        assert got == (0, 1 << 30, 0), "the leaf's box IS the root's: ratio 1, one slot"
    else:
        assert got[0] > 0 and got[1] > 0 and got[2] == 0


def test_a_bad_ratio_is_counted_and_adds_nothing(probe):
    """a triangle at the edge of fp32: its padded box overflows to infinities, the ratio is inf / inf"""
    big = np.finfo(np.float32).max
    flat = T.flat_of(v1=[[-big, -big, -big]], e1=[[big, 0.0, 0.0]], e2=[[0.0, big, big]], nrm=[[0, 0, 1]], tm=[0],
                     mats=[[0.8, 0.7, 0.6, 0.0, 0.3, 1.0, 0.0, 0.0, 0.0]], lights=[[0.5, 0.1, 0.2, 1.0, 0.9, 0.8, 3.0]]).contiguous()
    p = T.pack(probe, 0, flat)
    got = sah_packed(probe, 0)
    assert got == sah_numpy(p) and got == (0, 0, 1), got


def test_identity_refit_keeps_the_sums(probe):
    for name in ("test_scene", "semesterbild"):
        flat = T.SCENES[name]()
        T.pack(probe, 0, flat)
        created = sah_packed(probe, 0)
        assert T.refit(probe, 0, flat, flat, full=True) == 0, probe.probe_error()
        assert sah_packed(probe, 0) == created


def test_jitter_loosens_the_tree_and_the_way_back_restores_it(probe):
    """a 5 % jitter of every vertex leaves widely overlapping boxes -- the refitted tree costs more than the
    tree of creation; the step back to the creation arrays restores the sums exactly"""
    flat = cases.flat_semesterbild()
    T.pack(probe, 0, flat)
    created = sah_packed(probe, 0)
    moved = cases.jitter(flat, 0.05)
    assert T.refit(probe, 0, flat, moved) == 0, probe.probe_error()
    p = T.get(probe, 0, moved)
    now = sah_packed(probe, 0)
    assert now == sah_numpy(p) and now[2] == 0
    print(f"semesterbild, 5 % jitter: sah {sah_value(*created[:2]):.4f} -> {sah_value(*now[:2]):.4f} "
          f"(x {sah_value(*now[:2]) / sah_value(*created[:2]):.3f})")
    assert sah_value(*now[:2]) > sah_value(*created[:2])
    assert T.refit(probe, 0, moved, flat) == 0, probe.probe_error()
    assert sah_packed(probe, 0) == created
