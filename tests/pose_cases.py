"""Cases shared by the part-pose tests (host model and GPU): scenes, part layouts, transforms, the edge values, and the numpy
float32 restatement of `f32math.Rotor3.rotate_vec` / `Similarity3.transform_vec` that every output word is compared with.
numpy rounds every float32 array operation once and fuses nothing, as the Python scalars of f32math do."""
import ctypes as C

import numpy as np

import scene_update_cases as cases
from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, _lib
from hslu_i.ba_raytracing.f2501_raytracer_amd.f32math import Rotor3, Similarity3, Vec3

F32 = np.float32
NONE = 0xFFFFFFFF
TRI_OUT = ("tri_v1", "tri_e1", "tri_e2", "tri_normal")
SPH_OUT = ("sphere_center", "sphere_r_sq", "sphere_r_inv")
SCENES = {"test_scene": cases.flat_test_scene, "semesterbild": cases.flat_semesterbild}


def rest_of(flat):
    """the rest pose DevicePose takes from a FlatScene by default: vertices v1 + e1, v1 + e2 and radius sqrt(r_sq), in fp32"""
    return dict(v1=flat.tri_v1, v2=(flat.tri_v1 + flat.tri_e1).astype(F32), v3=(flat.tri_v1 + flat.tri_e2).astype(F32), normal=flat.tri_normal,
                centre=flat.sphere_center, radius=np.sqrt(flat.sphere_r_sq).astype(F32))


def layouts(nt, ns):
    """part layouts [(tri_first, tri_count, sphere_first, sphere_count)] for a scene of nt triangles and ns spheres"""
    a = max(nt // 5, 1)
    out = {"whole": [(0, nt, 0, ns)], "one_triangle": [(nt // 2, 1, 0, 0)],
           # a gap of 3 triangles of no part between the first two, the last two adjacent; the covering range starts at 1
           "three_parts": [(1, a, 0, 0), (1 + a + 3, a, 0, 0), (1 + 2 * a + 3, a, 0, 0)]}
    assert 1 + 3 * a + 3 <= nt
    if ns:
        out["spheres_only"] = [(0, 0, ns // 2, ns - ns // 2)]  # (the first ns // 2 spheres belong to no part)
    return out


def transforms():
    ident = Similarity3.identity()
    turn = Similarity3(Vec3(0.1, -0.2, 0.05), Rotor3.from_euler_angles(0.3, -0.2, 1.1), 0.75)
    flat0 = Similarity3(Vec3(0.3, 0.4, 0.5), Rotor3.from_euler_angles(0.3, -0.2, 1.1), 0.0)
    return {"identity": ident, "turn": turn, "scale0": flat0}


def rows_for(parts, first):
    """one transform per part: `first` for part 0, the others cyclically after it"""
    t = transforms()
    names = sorted(t)
    k = names.index(first)
    return _abi.transform_rows([t[names[(k + p) % len(names)]] for p in range(len(parts))])


# ---- the formulas, vectorised: q (n, 8) one transform row per object, v (n, 3) ---------------------------------------------------
def rotate(q, v):
    s, xy, xz, yz = q[:, 3], q[:, 4], q[:, 5], q[:, 6]
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        fx = s * x + xy * y + xz * z
        fy = s * y - xy * x + yz * z
        fz = s * z - xz * x - yz * y
        fw = xy * z - xz * y + yz * x
        out = np.stack([s * fx + xy * fy + xz * fz + yz * fw, s * fy - xy * fx - xz * fw + yz * fz, s * fz + xy * fw - xz * fx - yz * fy], 1)
    assert out.dtype == F32
    return out


def transform(q, v):
    with np.errstate(all="ignore"):
        out = rotate(q, v) * q[:, 7:8] + q[:, 0:3]
    assert out.dtype == F32
    return out


def covering(parts):
    p = np.asarray(parts, np.int64).reshape(-1, 4)
    tri = p[p[:, 1] > 0]
    lo, hi = (int(tri[:, 0].min()), int((tri[:, 0] + tri[:, 1]).max())) if len(tri) else (0, 0)
    return lo, hi, bool((p[:, 3] > 0).any())


def expected(rest, parts, rows):
    """the arrays rt_pose_read / rt_pose_model give, from the numpy formulas: triangle arrays over the covering range, sphere
    arrays over all spheres (empty when no part has spheres); objects of no part restated from their rest values"""
    lo, hi, has_spheres = covering(parts)
    ns = len(rest["radius"]) if has_spheres else 0
    tri_part, sph_part = np.full(hi - lo, -1, np.int64), np.full(ns, -1, np.int64)
    for k, (tf, tc, sf, sc) in enumerate(parts):
        tri_part[tf - lo:tf - lo + tc] = k
        sph_part[sf:sf + sc] = k
    v1, v2, v3, n = (np.array(rest[k][lo:hi], F32, copy=True) for k in ("v1", "v2", "v3", "normal"))
    m = tri_part >= 0
    q = rows[tri_part[m]]
    v1[m], v2[m], v3[m], n[m] = transform(q, v1[m]), transform(q, v2[m]), transform(q, v3[m]), rotate(q, n[m])
    c, r = np.array(rest["centre"][:ns], F32, copy=True), np.array(rest["radius"][:ns], F32, copy=True)
    m = sph_part >= 0
    q = rows[sph_part[m]]
    with np.errstate(all="ignore"):
        c[m], r[m] = transform(q, c[m]), r[m] * q[:, 7]
        out = dict(tri_v1=v1, tri_e1=v2 - v1, tri_e2=v3 - v1, tri_normal=n, sphere_center=c, sphere_r_sq=r * r, sphere_r_inv=F32(1) / r)
    assert all(a.dtype == F32 for a in out.values())
    return out


def restated(rest, parts):
    """the posed arrays before any kernel ran: every object from its rest values -- v1, v2 - v1, v3 - v1, normal; centre, r r, 1 / r"""
    lo, hi, has_spheres = covering(parts)
    ns = len(rest["radius"]) if has_spheres else 0
    v1, v2, v3, n = (np.asarray(rest[k][lo:hi], F32) for k in ("v1", "v2", "v3", "normal"))
    c, r = np.asarray(rest["centre"][:ns], F32), np.asarray(rest["radius"][:ns], F32)
    with np.errstate(all="ignore"):
        return dict(tri_v1=v1, tri_e1=v2 - v1, tri_e2=v3 - v1, tri_normal=n, sphere_center=c, sphere_r_sq=r * r, sphere_r_inv=F32(1) / r)


def desc_of(rest, parts, nt=None, ns=None):
    nt = len(rest["v1"]) if nt is None else nt
    ns = len(rest["radius"]) if ns is None else ns
    return _abi.make_pose_desc(parts, nt, ns, rest["v1"], rest["v2"], rest["v3"], rest["normal"], rest["centre"], rest["radius"])


def empty_outputs(rest, parts):
    lo, hi, has_spheres = covering(parts)
    ns = len(rest["radius"]) if has_spheres else 0
    out = {k: np.full((hi - lo, 3), 7.0, F32) for k in TRI_OUT}
    out.update(sphere_center=np.full((ns, 3), 7.0, F32), sphere_r_sq=np.full(ns, 7.0, F32), sphere_r_inv=np.full(ns, 7.0, F32))
    return out


def model(rest, parts, rows):
    """rt_pose_model through ctypes on the built library -> the arrays in rt_pose_read's layout"""
    lib = _lib.load()
    d, keep = desc_of(rest, parts)
    out = empty_outputs(rest, parts)
    rows = np.ascontiguousarray(rows, F32)
    rc = lib.rt_pose_model(C.byref(d), rows.ctypes.data, *[out[k].ctypes.data for k in TRI_OUT + SPH_OUT])
    assert rc == 0, lib.rt_last_error()
    return out


def assert_same_words(got, want, nan_ok=False, what=""):
    """every output word bit-equal; nan_ok: two words that are both NaN count as equal (inf - inf has another sign bit on
    the device than in numpy, the one exemption tests/test_scene_update_kernels_gpu.py uses)"""
    for k in TRI_OUT + SPH_OUT:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        differ = a.view(np.uint32) != b.view(np.uint32)
        if nan_ok:
            differ &= ~(np.isnan(a) & np.isnan(b))
        assert not differ.any(), f"{what} {k}: {int(differ.sum())} words differ, first at {np.argwhere(differ)[0]}: " \
                                 f"{a[differ][0]!r} != {b[differ][0]!r}"


# ---- edge values: 4096 seeded triangles, spheres and transforms at the edges of fp32 -----------------------------------------------
N_EDGE = 4096


def random_floats(r, n):
    """random bit patterns: every exponent, either sign, infinities and NaNs among them"""
    return r.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(F32)


def subnormals(r, n):
    return (r.integers(1, 1 << 23, n).astype(np.uint32) | (r.integers(0, 2, n).astype(np.uint32) << np.uint32(31))).view(F32)


def log_uniform(r, shape, lo, hi):
    with np.errstate(over="ignore", under="ignore"):
        return (np.power(10.0, r.uniform(lo, hi, shape)) * r.choice([-1.0, 1.0], shape)).astype(F32)


def edge_case(seed=77):
    """-> (rest, parts, rows): one part per object pair (triangle k, sphere k) with its own transform.  Quarters: subnormal
    coordinates, magnitudes whose products overflow (and meet as inf - inf), log-uniform over every exponent, random bits."""
    r = np.random.default_rng(seed)
    n, q = N_EDGE, N_EDGE // 4

    def field(shape):
        cols = int(np.prod(shape[1:])) if len(shape) > 1 else 1
        a = np.concatenate([subnormals(r, q * cols), log_uniform(r, q * cols, 18, 38.5), log_uniform(r, q * cols, -44, 38.5), random_floats(r, q * cols)])
        return np.ascontiguousarray(a.reshape(4, q, cols).reshape(n, cols).reshape(shape))

    rest = dict(v1=field((n, 3)), v2=field((n, 3)), v3=field((n, 3)), normal=field((n, 3)), centre=field((n, 3)), radius=field((n,)))
    rows = field((n, 8))
    rows[:8] = _abi.transform_rows([Similarity3.identity()] * 8)  # a few tame ones, against everything else
    fixed = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, np.finfo(F32).max, np.finfo(F32).tiny, 2.0 ** -149], F32)
    rest["radius"][:8] = fixed
    rows[8:16, 7] = fixed
    parts = [(k, 1, k, 1) for k in range(n)]
    return rest, parts, rows


def soup(n, seed=40):
    """n small seeded triangles scattered in the unit cube, one material, one light: the smallest meshes with a chosen BVH size"""
    from test_scene_pack_host import flat_of

    r = np.random.default_rng(seed)
    v1 = r.uniform(0.05, 0.95, (n, 3))
    e1, e2 = r.uniform(-0.04, 0.04, (n, 3)), r.uniform(-0.04, 0.04, (n, 3))
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return flat_of(v1=v1, e1=e1, e2=e2, nrm=nrm, tm=[0] * n, mats=[[0.8, 0.7, 0.6, 0.0, 0.3, 1.0, 0.0, 0.0, 0.0]],
                   lights=[[0.5, 0.1, -1.2, 1.0, 0.9, 0.8, 3.0]]).contiguous()
