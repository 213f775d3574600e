"""The host model of part poses (rt_pose_model, csrc/rt_pose.cpp: the functions of csrc/rt_pose.h in loops -- the same
functions rt_pose_kernel is made of) checked on the CPU through ctypes on the built library.  The reference for every word
is `f32math`'s Rotor3.rotate_vec / Similarity3.transform_vec, vectorised over numpy float32 (pose_cases.py); all checks
are bit-exact except the one stated bound on normals."""
import ctypes as C
import os

import numpy as np
import pytest

import pose_cases as P
from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, _abi, _lib, scenes
from hslu_i.ba_raytracing.f2501_raytracer_amd.f32math import F, Rotor3, Similarity3, Vec3
from hslu_i.ba_raytracing.f2501_raytracer_amd.obj import load_obj_scene

F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.fixture(scope="module", params=sorted(P.SCENES))
def rest(request):
    flat = P.SCENES[request.param]()
    return request.param, P.rest_of(flat)


def test_transform_row_is_the_struct(lib):
    t = P.transforms()["turn"]
    row = _abi.transform_rows([t])
    assert C.sizeof(_abi.rt_transform) == 32 and row.shape == (1, 8)
    s = _abi.rt_transform.from_buffer_copy(row.tobytes())
    assert (s.translation[0], s.rotor[0], s.rotor[3], s.scale) == (float(t.translation.x), float(t.rotation.s), float(t.rotation.yz), float(t.scale))


def test_numpy_formulas_are_f32math_term_for_term():
    """the vectorised restatement against the scalar classes, on a few vectors"""
    t = P.transforms()["turn"]
    row = _abi.transform_rows([t])
    r = np.random.default_rng(1)
    v = r.uniform(-3, 3, (64, 3)).astype(F32)
    q = np.repeat(row, len(v), 0)
    rot, tra = P.rotate(q, v), P.transform(q, v)
    for k in range(len(v)):
        a, b = t.rotation.rotate_vec(Vec3(*v[k])), t.transform_vec(Vec3(*v[k]))
        assert [F32(x) for x in a] == list(rot[k]) and [F32(x) for x in b] == list(tra[k])


@pytest.mark.parametrize("first", ["identity", "turn", "scale0"])
@pytest.mark.parametrize("layout", ["whole", "three_parts", "spheres_only", "one_triangle"])
def test_model_equals_the_formulas_bit_for_bit(lib, rest, layout, first):
    name, rs = rest
    parts = P.layouts(len(rs["v1"]), len(rs["radius"]))[layout]
    rows = P.rows_for(parts, first)
    got, want = P.model(rs, parts, rows), P.expected(rs, parts, rows)
    P.assert_same_words(got, want, what=f"{name} / {layout} / {first}")
    lo, hi, has_spheres = P.covering(parts)
    assert got["tri_v1"].shape == (hi - lo, 3) and got["sphere_r_sq"].shape == ((len(rs["radius"]) if has_spheres else 0),)
    if layout == "three_parts":  # the gap: rest values v1, v2 - v1, v3 - v1, normal
        a = parts[0][1]
        gap = slice(a, a + 3)
        assert np.array_equal(got["tri_v1"][gap], rs["v1"][lo:hi][gap]) and np.array_equal(got["tri_normal"][gap], rs["normal"][lo:hi][gap])
        assert np.array_equal(got["tri_e1"][gap], (rs["v2"] - rs["v1"])[lo:hi][gap])
        assert not np.array_equal(got["tri_v1"][:a], rs["v1"][lo:hi][:a]) or first == "identity"
    if layout == "spheres_only":  # spheres of no part: centre, r r, 1 / r
        k = parts[0][2]
        assert np.array_equal(got["sphere_center"][:k], rs["centre"][:k]) and np.array_equal(got["sphere_r_sq"][:k], rs["radius"][:k] * rs["radius"][:k])
    if first == "scale0" and layout == "whole":
        assert (got["tri_e1"] == 0).all() and np.isinf(got["sphere_r_inv"]).all(), "scale 0 collapses every part onto its translation"


def test_identity_restates_exact_rest_vertices(lib):
    """with the identity every product is exact: v1, v2 - v1, v3 - v1, normal and centre, r r, 1 / r"""
    rs = P.rest_of(P.SCENES["test_scene"]())
    parts = P.layouts(len(rs["v1"]), len(rs["radius"]))["whole"]
    got = P.model(rs, parts, _abi.transform_rows([Similarity3.identity()]))
    assert np.array_equal(got["tri_v1"], rs["v1"]) and np.array_equal(got["tri_e1"], rs["v2"] - rs["v1"]) and np.array_equal(got["tri_normal"], rs["normal"])
    assert np.array_equal(got["sphere_center"], rs["centre"]) and np.array_equal(got["sphere_r_inv"], F32(1) / rs["radius"])


def test_edge_values(lib):
    """4096 seeded triangles, spheres and transforms at the edges of fp32: subnormals, products that overflow, inf - inf"""
    rs, parts, rows = P.edge_case()
    got, want = P.model(rs, parts, rows), P.expected(rs, parts, rows)
    P.assert_same_words(got, want, nan_ok=True, what="edge values")
    x = got["tri_v1"]
    tiny = (np.abs(x) < np.finfo(F32).tiny) & (x != 0)
    print(f"edge values: {int(np.isnan(x).sum())} NaN, {int(np.isinf(x).sum())} inf, {int(tiny.sum())} subnormal words of v1'")
    assert np.isnan(x).sum() >= 100 and np.isinf(x).sum() >= 100 and tiny.sum() >= 10, "the classes the case is drawn for are there"
    assert np.isfinite(x).sum() >= 1000


def semesterbild_transform(cfg, turn=-0.015):
    """a transform of semesterbild's form (scenes.semesterbild): translation components scaled by constants, a pitch, a scale of about 1.226"""
    return Similarity3.new(Vec3.new(F(0.0135) * cfg.scene_width, F(0.145) * cfg.scene_height, F(0.885) * cfg.scene_depth),
                           Rotor3.from_euler_angles(0.0, turn, 0.0), F(1.226) * cfg.average_scene_dimension)


def arrays_of(scene):
    t = scene.triangles
    col = lambda f: np.array([[F32(x) for x in getattr(k, f)] for k in t], F32)  # noqa: E731
    return dict(v1=col("vertex1"), v2=col("vertex2"), v3=col("vertex3"), e1=col("edge1"), e2=col("edge2"), normal=col("normal"))


def test_posing_equals_loading(lib, turn=-0.015):
    """`load_obj_scene(text_lowres.npz, None)` gives rest vertices; posing them reproduces v1, e1, e2 of
    `load_obj_scene(text_lowres.npz, transform)` BIT FOR BIT.  Normals: the reference rotates per-vertex normals and lerps
    afterwards, the pose rotates the lerped normal; bound 8 * 2^-24 per component (measured between the two Python formulas:
    3 * 2^-24 for semesterbild's own transform; the margin is for another transform's roundings)."""
    cfg = RenderConfig.from_features([])
    path = scenes.mesh_path(cfg, "text_lowres")
    tr = semesterbild_transform(cfg, turn)
    rest, loaded = arrays_of(load_obj_scene(path, None)), arrays_of(load_obj_scene(path, tr))
    nt = len(rest["v1"])
    assert nt == 1639
    rs = dict(v1=rest["v1"], v2=rest["v2"], v3=rest["v3"], normal=rest["normal"], centre=np.zeros((0, 3), F32), radius=np.zeros(0, F32))
    got = P.model(rs, [(0, nt, 0, 0)], _abi.transform_rows([tr]))
    for k, ref in (("tri_v1", "v1"), ("tri_e1", "e1"), ("tri_e2", "e2")):
        assert np.array_equal(got[k].view(np.uint32), loaded[ref].view(np.uint32)), k
    d = float(np.abs(got["tri_normal"].astype(np.float64) - loaded["normal"].astype(np.float64)).max())
    print(f"posing equals loading (pitch {turn}): max |normal difference| = {d:.3e} = {d * 2 ** 24:.2f} * 2^-24")
    assert d <= 8 * 2.0 ** -24


# ---- refusals: every one by message, none needs a device -------------------------------------------------------------------------
def test_refusals(lib):
    rs = P.rest_of(P.SCENES["test_scene"]())
    nt, ns = len(rs["v1"]), len(rs["radius"])
    assert ns >= 2
    bad = _abi.RT_ERR_INVALID_ARG
    rows = _abi.transform_rows([Similarity3.identity()] * 4)

    def code(parts=((0, nt, 0, ns),), change=lambda d: None, transforms=rows, create=False):
        d, keep = P.desc_of(rs, list(parts))
        change(d)
        out = P.empty_outputs(rs, [(0, nt, 0, ns)])
        if create:
            h = C.c_void_p()
            rc = lib.rt_pose_create(C.byref(d), 0, C.byref(h))
            assert not h.value
        else:
            rc = lib.rt_pose_model(C.byref(d), None if transforms is None else transforms.ctypes.data,
                                   *[out[k].ctypes.data for k in P.TRI_OUT + P.SPH_OUT])
        return rc, lib.rt_last_error().decode()

    assert code()[0] == 0
    for create in (False, True):
        rc, msg = code(change=lambda d: setattr(d, "abi_version", _abi.RT_ABI_VERSION + 1), create=create)
        assert rc == bad and "abi_version" in msg
        rc, msg = code(change=lambda d: setattr(d, "n_parts", 0), create=create)
        assert rc == bad and "n_parts" in msg
        rc, msg = code(change=lambda d: setattr(d, "parts", None), create=create)
        assert rc == bad and "null parts" in msg
        rc, msg = code(parts=[(0, 2, 0, 0), (5, 0, 0, 0)], create=create)
        assert rc == bad and "part 1 is empty" in msg
        rc, msg = code(parts=[(nt - 1, 2, 0, 0)], create=create)
        assert rc == bad and "tri_first" in msg and "n_triangles" in msg
        rc, msg = code(parts=[(0xFFFFFFFF, 2, 0, 0)], create=create)
        assert rc == bad and "tri_first" in msg, "no 32-bit wrap-around"
        rc, msg = code(parts=[(0, 0, ns - 1, 2)], create=create)
        assert rc == bad and "sphere_first" in msg and "n_spheres" in msg
        rc, msg = code(parts=[(0, 4, 0, 0), (3, 4, 0, 0)], create=create)
        assert rc == bad and "triangle ranges overlap" in msg
        rc, msg = code(parts=[(6, 2, 0, 1), (0, 4, 0, 0), (2, 5, 1, 1)], create=create)
        assert rc == bad and "triangle ranges overlap" in msg, "found whatever the order of the parts"
        rc, msg = code(parts=[(0, 4, 0, 2), (4, 4, 1, 1)], create=create)
        assert rc == bad and "sphere ranges overlap" in msg
        for field in ("tri_v1", "tri_v2", "tri_v3", "tri_normal"):
            rc, msg = code(change=lambda d: setattr(d, field, None), create=create)
            assert rc == bad and "tri_v2" in msg and "required" in msg
        for field in ("sphere_center", "sphere_radius"):
            rc, msg = code(change=lambda d: setattr(d, field, None), create=create)
            assert rc == bad and "sphere_radius" in msg and "required" in msg
        # rest arrays of a kind no part uses may be missing
        if not create:
            assert code(parts=[(0, 0, 0, ns)], change=lambda d: setattr(d, "tri_v1", None))[0] == 0
            assert code(parts=[(0, nt, 0, 0)], change=lambda d: setattr(d, "sphere_radius", None))[0] == 0
    rc, msg = code(transforms=None)
    assert rc == bad and "null transforms" in msg
    h = C.c_void_p()
    assert lib.rt_pose_create(None, 0, C.byref(h)) == bad and lib.rt_pose_model(None, rows.ctypes.data, *[None] * 7) == bad
    assert lib.rt_pose_apply(None, None, rows.ctypes.data, None) == bad and "null scene" in lib.rt_last_error().decode()
    assert lib.rt_pose_apply_device(None, None, None, None, None) == bad
    assert lib.rt_pose_geometry_device(None, None, None) == bad and lib.rt_pose_read(None, *[None] * 9) == bad
    assert lib.rt_scene_bvh_quality(None, None) == bad
    lib.rt_pose_destroy(None)
