"""The inputs of the BVH rebuild tests (host model and GPU): small scenes that reach every path of csrc/rt_lbvh.h.  Everything
is a FlatScene from a seeded generator, so the host model, the device and a fresh handle all see the same arrays."""
import functools

import numpy as np

import scene_update_cases as cases
from test_scene_pack_host import LIGHT, MAT_DIFFUSE, flat_of
from test_scene_update_host import SCENES

F32 = np.float32
MAX_LEAF = 4  # rt_bvh_tuning.max_leaf as applied by default


def soup(n, seed=40):
    """n small triangles in the unit cube"""
    r = np.random.default_rng(seed + n)
    v1, e1, e2 = r.uniform(0.1, 0.9, (n, 3)), r.normal(0, 0.2, (n, 3)), r.normal(0, 0.2, (n, 3))
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return flat_of(v1=v1, e1=e1, e2=e2, nrm=nrm, tm=[0] * n, mats=[MAT_DIFFUSE], lights=[LIGHT]).contiguous()


def copies(n=9):
    """n copies of one triangle: all keys are equal, the canonical index breaks every tie"""
    one = np.ones((n, 1))
    return flat_of(v1=one * [[0.1, 0.2, 0.3]], e1=one * [[0.5, 0.0, 0.1]], e2=one * [[0.0, 0.6, 0.1]], nrm=one * [[0, 0, 1]], tm=[0] * n,
                   mats=[MAT_DIFFUSE], lights=[LIGHT]).contiguous()


def clusters(n=9000, distinct=37, seed=5):
    """n triangles drawn from `distinct` different ones in a seeded interleaved order: runs of about n / distinct equal keys that
    lie across every boundary of the sort (wavefront, round of 256, tile of 4096), with distinct keys between them"""
    base = soup(distinct)
    pick = np.random.default_rng(seed).integers(0, distinct, n)
    pick[:distinct] = np.arange(distinct)  # (every one of them appears)
    return flat_of(v1=base.tri_v1[pick], e1=base.tri_e1[pick], e2=base.tri_e2[pick], nrm=base.tri_normal[pick], tm=[0] * n,
                   mats=[MAT_DIFFUSE], lights=[LIGHT]).contiguous()


def nan_vertex(n=20, victim=7):
    """one triangle whose first vertex has a NaN x among n: its centre is not finite on that axis"""
    f = soup(n)
    v1 = f.tri_v1.copy()
    v1[victim, 0] = np.nan
    return cases.copy(f, tri_v1=v1)


def strip(n=40):
    """a flat strip along x: every centre has the same y and z, so two axes of the key frame are degenerate"""
    x = np.arange(n, dtype=np.float64)[:, None]
    one = np.ones((n, 1))
    return flat_of(v1=np.concatenate([x, 0 * x, 0 * x], 1), e1=one * [[1, 0, 0]], e2=one * [[0, 1, 0]], nrm=one * [[0, 0, 1]], tm=[0] * n,
                   mats=[MAT_DIFFUSE], lights=[LIGHT]).contiguous()


def heightfield(m=65):
    """an m x m heightfield, 2 (m - 1)^2 triangles: 8192 for m = 65, two boundaries of the 4096-key sort tile"""
    r = np.random.default_rng(3)
    g = np.linspace(0.0, 1.0, m)
    x, z = np.meshgrid(g, g, indexing="ij")
    y = 0.1 * np.sin(7 * x) * np.cos(5 * z) + r.uniform(0, 0.01, x.shape)
    p = np.stack([x, y, z], -1)
    a, b, c, d = p[:-1, :-1], p[1:, :-1], p[:-1, 1:], p[1:, 1:]
    v1 = np.concatenate([a.reshape(-1, 3), d.reshape(-1, 3)])
    e1 = np.concatenate([(b - a).reshape(-1, 3), (c - d).reshape(-1, 3)])
    e2 = np.concatenate([(c - a).reshape(-1, 3), (b - d).reshape(-1, 3)])
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    n = len(v1)
    return flat_of(v1=v1, e1=e1, e2=e2, nrm=nrm, tm=[0] * n, mats=[MAT_DIFFUSE], lights=[LIGHT]).contiguous()


def shuffled(flat, seed=9):
    """triangle t takes the geometry of triangle perm(t): the same triangle soup, but the tree of creation now groups strangers"""
    perm = np.random.default_rng(seed).permutation(flat.n_triangles)
    return cases.copy(flat, tri_v1=flat.tri_v1[perm], tri_e1=flat.tri_e1[perm], tri_e2=flat.tri_e2[perm], tri_normal=flat.tri_normal[perm])


CASES = {name: fn for name, fn in SCENES.items() if name != "empty"}
CASES.update({"max_leaf": lambda: soup(MAX_LEAF), "max_leaf_plus_1": lambda: soup(MAX_LEAF + 1), "copies": copies, "nan_vertex": nan_vertex,
              "strip": strip, "heightfield": heightfield})
# ties at scale: equal keys across a wavefront, a round and a tile of the sort, where only the canonical index orders them
CASES.update({"copies_65": lambda: copies(65), "copies_257": lambda: copies(257), "copies_4097": lambda: copies(4097), "clusters": clusters})


@functools.lru_cache(maxsize=None)
def flat_case(name):
    return CASES[name]()


def deformed(name):
    """(creation, current) of a case: the scene is created as `creation` and refitted to `current` before it is rebuilt.
    "shuffle" is semesterbild refitted to its shuffled self; every other case is rebuilt as created"""
    if name == "shuffle":
        f = flat_case("semesterbild")
        return f, shuffled(f)
    f = flat_case(name)
    return f, f


ALL = sorted(CASES) + ["shuffle"]
