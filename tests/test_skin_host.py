"""The host model of skinned meshes (rt_skin_model, csrc/rt_skin.cpp: the functions of csrc/rt_skin.h in loops -- the same
functions the kernels of rt_skin.hip are made of) checked on the CPU through ctypes on the built library.  The reference
for every word is the numpy float32 restatement of skin_cases.py, and for a mesh on one bone of weight 1 the loader itself
(`load_obj_scene(path, transform)`): all checks are bit-exact."""
import ctypes as C
import os

import numpy as np
import pytest

import pose_cases as P
import scene_update_cases as cases
import skin_cases as S
from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, _abi, _lib, scenes
from hslu_i.ba_raytracing.f2501_raytracer_amd.f32math import F, Rotor3, Similarity3, Vec3
from hslu_i.ba_raytracing.f2501_raytracer_amd.obj import load_indexed_mesh, load_obj_scene
from hslu_i.ba_raytracing.f2501_raytracer_amd.scene import Material, ColorType, TriangleData

F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_desc_is_the_struct(lib):
    assert C.sizeof(_abi.rt_skin_desc) == 24 + 5 * C.sizeof(C.c_void_p)
    assert _abi.rt_skin_desc.position.offset == 24 and _abi.rt_skin_desc.weight.offset == 24 + 4 * C.sizeof(C.c_void_p)


def test_fma_restatement_rounds_once():
    """the restated fma against exact rational arithmetic on values chosen to round twice in the naive float64 form"""
    from fractions import Fraction

    r = np.random.default_rng(2)
    a, b = r.uniform(-4, 4, 2000).astype(F32), r.uniform(-4, 4, 2000).astype(F32)
    c = (r.uniform(-4, 4, 2000) * 2.0 ** r.integers(-40, 30, 2000)).astype(F32)
    # ties of the float32 grid with a remainder far below float64's last bit: the naive sum rounds to the tie, then to even
    a[:4], b[:4] = F32(1 + 2.0 ** -12), F32(1 + 2.0 ** -12)
    c[:4] = np.array([2.0 ** -60, -2.0 ** -60, 2.0 ** -80, -2.0 ** -80], F32)
    got = S.fma32(a, b, c)
    for k in range(len(a)):
        exact = Fraction(float(a[k])) * Fraction(float(b[k])) + Fraction(float(c[k]))
        lo = F32(float(exact))  # (float(Fraction) is correctly rounded to float64; this double rounding is what fma32 avoids)
        cands = sorted({lo, np.nextafter(lo, F32(np.inf)), np.nextafter(lo, F32(-np.inf))}, key=lambda v: abs(Fraction(float(v)) - exact))
        best = cands[0]
        if abs(Fraction(float(cands[1])) - exact) == abs(Fraction(float(best)) - exact):  # a true tie: to even
            best = best if (best.view(np.uint32) & 1) == 0 else cands[1]
        assert got[k] == best, (k, a[k], b[k], c[k], got[k], best)


# ---- 1. the model equals the formulas ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(2 * len(S.SIZES)))
def test_model_equals_the_formulas_bit_for_bit(lib, case):
    label, mesh, bones = S.seeded_cases()[case]
    got, want = S.model(mesh, bones), S.expected(mesh, bones)
    S.assert_same_words(got, want, nan_ok=len(mesh["position"]) == 1 and mesh["normal"] is None, what=label)
    nv, w = len(mesh["position"]), mesh["weight"]
    assert mesh["indices"][-1, 2] == nv - 1, "the last vertex is referenced by the last triangle"
    assert mesh["bone"][-1, 0] == mesh["n_bones"] - 1 and w[-1, 0] != 0, "a vertex on the last bone"
    if nv >= 255:
        kept = (w != 0).astype(int) @ (1 << np.arange(4))
        assert set(kept.tolist()) == set(range(16)), "every pattern of zero weights"
        assert np.signbit(w[w == 0]).any() and not np.signbit(w[w == 0]).all(), "+0 and -0"
        none = kept == 0
        assert none.any() and np.array_equal(got["position"][none], mesh["position"][none]), "no influence kept: the rest position"
        if mesh["normal"] is not None:
            assert np.array_equal(got["normal"][none], mesh["normal"][none])
        assert not np.array_equal(got["position"][~none], mesh["position"][~none])
    if mesh["normal"] is None:  # the face normal against TriangleData.with_material, triangle by triangle
        V = got["position"]
        mat = Material.diffuse(ColorType(1, 1, 1))
        for t in range(0, len(mesh["indices"]), 7):
            i = mesh["indices"][t]
            with np.errstate(all="ignore"):  # (the one-vertex mesh is one degenerate triangle: 0 / 0)
                tri = TriangleData.with_material(Vec3(*V[i[0]]), Vec3(*V[i[1]]), Vec3(*V[i[2]]), mat)
            n = np.array([F32(x) for x in tri.normal], F32)
            same = (n.view(np.uint32) == got["tri_normal"][t].view(np.uint32)) | (np.isnan(n) & np.isnan(got["tri_normal"][t]))
            assert same.all(), (label, t, n, got["tri_normal"][t])


def test_single_influence_of_weight_one_is_the_transform_exactly(lib):
    mesh = S.seeded_mesh(300, 700, 3, True)
    mesh["weight"][:] = [0, 0, 1, 0]
    bones = S.seeded_bones(3)
    got = S.model(mesh, bones)
    q = bones[mesh["bone"][:, 2].astype(np.int64)]
    assert np.array_equal(got["position"].view(np.uint32), P.transform(q, mesh["position"]).view(np.uint32))
    assert np.array_equal(got["normal"].view(np.uint32), P.rotate(q, mesh["normal"]).view(np.uint32))


# ---- 2. a mesh on one bone is the mesh the loader gives ------------------------------------------------------------------------------
def arrays_of(scene):
    f = scene.flatten().contiguous()
    return {k: getattr(f, k) for k in S.TRI_OUT}


@pytest.fixture(scope="module")
def text_mesh():
    cfg = RenderConfig.from_features([])
    path = scenes.mesh_path(cfg, "text_lowres")
    m = load_indexed_mesh(path)
    assert m.position.shape == (1689, 3) and m.normal.shape == (1689, 3) and m.indices.shape == (1639, 3) and m.indices.dtype == np.uint32
    nv = len(m.position)
    mesh = dict(position=m.position, normal=m.normal, indices=m.indices, bone=np.zeros((nv, 4), np.uint16),
                weight=np.tile(np.array([1, 0, 0, 0], F32), (nv, 1)), n_bones=1, tri_first=0, n_triangles=len(m.indices))
    return cfg, path, mesh


@pytest.mark.parametrize("which", ["identity", "turn", "semesterbild"])
def test_one_bone_equals_loading(lib, text_mesh, which):
    cfg, path, mesh = text_mesh
    tr = scenes.semesterbild_text_transform(cfg) if which == "semesterbild" else P.transforms()[which]
    rows = _abi.transform_rows([tr])
    got = S.model(mesh, rows)
    loaded = arrays_of(load_obj_scene(path, tr))
    for k in S.TRI_OUT:
        assert np.array_equal(got[k].view(np.uint32), loaded[k].view(np.uint32)), f"{which}: {k}"
    if which == "semesterbild":
        flat = cases.flat_semesterbild()
        for k in S.TRI_OUT:
            assert np.array_equal(got[k].view(np.uint32), getattr(flat, k)[:1639].view(np.uint32)), f"flat_semesterbild: {k}"
    # v1 / e1 / e2 are also those of a pose of the same mesh as one part
    i = mesh["indices"].astype(np.int64)
    rest = dict(v1=mesh["position"][i[:, 0]], v2=mesh["position"][i[:, 1]], v3=mesh["position"][i[:, 2]], normal=mesh["normal"][i[:, 0]],
                centre=np.zeros((0, 3), F32), radius=np.zeros(0, F32))
    posed = P.model(rest, [(0, len(i), 0, 0)], rows)
    for k in ("tri_v1", "tri_e1", "tri_e2"):
        assert np.array_equal(got[k].view(np.uint32), posed[k].view(np.uint32)), f"{which}: {k} vs rt_pose_model"


def test_load_indexed_mesh_unifies_as_single_index(tmp_path):
    """distinct (v, vn) pairs in first-occurrence order, triangles in file order (fan triangulation); .obj and .npz agree"""
    from hslu_i.ba_raytracing.f2501_raytracer_amd.obj import pack_obj

    obj = tmp_path / "m.obj"
    obj.write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvn 0 0 1\nvn 0 1 0\nf 1//1 2//1 3//2 4//1\nf 3//1 2//1 1//2\n")
    m = load_indexed_mesh(str(obj))
    # corners: (0,0) (1,0) (2,1) | (0,0) (2,1) (3,0) | (2,0) (1,0) (0,1)
    assert m.indices.tolist() == [[0, 1, 2], [0, 2, 3], [4, 1, 5]]
    assert m.position.tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [1, 1, 0], [0, 0, 0]]
    assert m.normal.tolist() == [[0, 0, 1], [0, 0, 1], [0, 1, 0], [0, 0, 1], [0, 0, 1], [0, 1, 0]]
    pack_obj(str(obj), str(tmp_path / "m.npz"))
    z = load_indexed_mesh(str(tmp_path / "m.npz"))
    assert all(np.array_equal(a, b) for a, b in zip(m, z))
    bare = tmp_path / "bare.obj"
    bare.write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nf 1 2 3\nf 3 2 1\n")
    b = load_indexed_mesh(str(bare))
    assert b.normal is None and b.indices.tolist() == [[0, 1, 2], [2, 1, 0]] and len(b.position) == 3
    some = tmp_path / "some.obj"
    some.write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nvn 0 0 1\nf 1//1 2 3//1\n")
    with pytest.raises(ValueError, match="corners have no normal"):
        load_indexed_mesh(str(some))


# ---- 3. edge values ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normals", [True, False])
def test_edge_values(lib, normals):
    """4096 seeded vertices, triangles and bones at the edges of fp32: subnormals, products that overflow, inf - inf"""
    mesh, bones = S.edge_case(normals)
    got, want = S.model(mesh, bones), S.expected(mesh, bones)
    S.assert_same_words(got, want, nan_ok=True, what="edge values")
    x = got["tri_v1"]
    tiny = (np.abs(x) < np.finfo(F32).tiny) & (x != 0)
    print(f"edge values: {int(np.isnan(x).sum())} NaN, {int(np.isinf(x).sum())} inf, {int(tiny.sum())} subnormal words of v1")
    assert np.isnan(x).sum() >= 100 and np.isinf(x).sum() >= 100 and tiny.sum() >= 10, "the classes the case is drawn for are there"
    assert np.isfinite(x).sum() >= 1000


# ---- 4. refusals: every one by code and message, none needs a device ------------------------------------------------------------------
def test_refusals(lib):
    mesh = S.seeded_mesh(20, 30, 3, True)
    bones = S.seeded_bones(3)
    bad = _abi.RT_ERR_INVALID_ARG

    def code(change=lambda d: None, edit=lambda m: None, bones=bones, create=False):
        m = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in mesh.items()}
        edit(m)
        d, keep = S.desc_of(m)
        change(d)
        out = S.empty_outputs(m)
        if create:
            h = C.c_void_p()
            rc = lib.rt_skin_create(C.byref(d), 0, C.byref(h))
            assert not h.value
        else:
            rc = lib.rt_skin_model(C.byref(d), None if bones is None else bones.ctypes.data, *S.pointers(out))
        return rc, lib.rt_last_error().decode()

    def put(array, at, value):
        def edit(m):
            m[array][at] = value
        return edit

    assert code()[0] == 0
    for create in (False, True):
        rc, msg = code(change=lambda d: setattr(d, "abi_version", _abi.RT_ABI_VERSION + 1), create=create)
        assert rc == bad and "abi_version" in msg
        for field in ("n_vertices", "tri_count", "n_bones"):
            rc, msg = code(change=lambda d: setattr(d, field, 0), create=create)
            assert rc == bad and f"{field} is 0" in msg, msg
        rc, msg = code(change=lambda d: setattr(d, "n_bones", 65537), create=create)
        assert rc == bad and "n_bones 65537 > 65536" in msg
        rc, msg = code(change=lambda d: setattr(d, "n_triangles", 30), create=create)
        assert rc == bad and "tri_first 1 + tri_count 30 > n_triangles 30" in msg
        rc, msg = code(change=lambda d: setattr(d, "tri_first", 0xFFFFFFFF), create=create)
        assert rc == bad and "tri_first" in msg, "no 32-bit wrap-around"
        for field in ("position", "indices", "bone", "weight"):
            rc, msg = code(change=lambda d: setattr(d, field, None), create=create)
            assert rc == bad and f"null {field}" in msg, msg
        rc, msg = code(edit=put("indices", (29, 1), 20), create=create)
        assert rc == bad and "indices of triangle 29" in msg and "n_vertices 20" in msg
        rc, msg = code(edit=put("indices", (4, 0), 0xFFFFFFFF), create=create)
        assert rc == bad and "indices of triangle 4" in msg

        def zero_weight_bad_bone(m):
            m["weight"][7, 3], m["bone"][7, 3] = 0.0, 3

        rc, msg = code(edit=zero_weight_bad_bone, create=create)
        assert rc == bad and "bone of vertex 7" in msg and "n_bones 3" in msg, "zero weight or not"
        rc, msg = code(edit=put("bone", (19, 0), 65535), create=create)
        assert rc == bad and "bone of vertex 19" in msg
        for value in (np.nan, np.inf, -np.inf):
            rc, msg = code(edit=put("weight", (11, 2), value), create=create)
            assert rc == bad and "weight of vertex 11" in msg and "not finite" in msg
    rc, msg = code(bones=None)
    assert rc == bad and "null bones" in msg
    # a mesh without vertex normals is no refusal, and the model runs with no output at all
    assert code(change=lambda d: setattr(d, "normal", None))[0] == 0
    d, keep = S.desc_of(mesh)
    assert lib.rt_skin_model(C.byref(d), bones.ctypes.data, *[None] * 6) == 0
    nan_bones = bones.copy()
    nan_bones[1, 4] = np.nan
    assert lib.rt_skin_model(C.byref(d), nan_bones.ctypes.data, *[None] * 6) == 0, "the model does not check bones"
    h = C.c_void_p()
    assert lib.rt_skin_create(None, 0, C.byref(h)) == bad and lib.rt_skin_model(None, bones.ctypes.data, *[None] * 6) == bad
    assert lib.rt_skin_create(C.byref(d), 0, None) == bad
    assert lib.rt_skin_apply(None, None, bones.ctypes.data, None) == bad and "null scene" in lib.rt_last_error().decode()
    assert lib.rt_skin_apply_device(None, None, None, None, None) == bad and "null scene" in lib.rt_last_error().decode()
    assert lib.rt_skin_geometry_device(None, None, None) == bad and "null skin" in lib.rt_last_error().decode()
    assert lib.rt_skin_read(None, *[None] * 6) == bad and "null skin" in lib.rt_last_error().decode()
    lib.rt_skin_destroy(None)


def test_semesterbild_is_unchanged_by_the_refactor(lib):
    """`scenes.semesterbild` calls `semesterbild_text_transform`; the inline transform it replaced, restated here, places the
    mesh on the same bytes"""
    for features in ([], ["scene_backface_culling"]):
        cfg = RenderConfig.from_features(features)
        inline = Similarity3.new(Vec3.new(F(0.0135) * cfg.scene_width, F(0.145) * cfg.scene_height, F(0.885) * cfg.scene_depth),
                                 Rotor3.from_euler_angles(0.0, -0.015, 0.0), F(1.226) * cfg.average_scene_dimension)
        assert np.array_equal(_abi.transform_rows([scenes.semesterbild_text_transform(cfg)]).view(np.uint32), _abi.transform_rows([inline]).view(np.uint32))
    cfg = RenderConfig.from_features([])
    flat = scenes.semesterbild(cfg, model="text_lowres").flatten().contiguous()
    loaded = arrays_of(load_obj_scene(scenes.mesh_path(cfg, "text_lowres"), inline))
    first, count = cases.mesh_range("semesterbild", flat)
    assert (first, count) == (0, 1639)
    for k in S.TRI_OUT:
        assert np.array_equal(getattr(flat, k)[:count].view(np.uint32), loaded[k].view(np.uint32)), k
