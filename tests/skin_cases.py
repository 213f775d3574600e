"""Cases shared by the skinned-mesh tests (host model and GPU): seeded indexed meshes, bone tables, the edge values, and the
numpy float32 restatement of the formulas of csrc/rt_skin.h that every output word is compared with.  numpy rounds every
float32 array operation once and fuses nothing; the two fma of the face normal are float64 products of float32 inputs
(exact) added in float64 with the sum rounded to odd, so that the one rounding to float32 is the fused operation's."""
import ctypes as C

import numpy as np

import pose_cases as P
from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, _lib

F32 = np.float32
VERT_OUT = ("position", "normal")
TRI_OUT = P.TRI_OUT
OUT = VERT_OUT + TRI_OUT
# (vertices, triangles, bones) of the seeded meshes: the last thread of the vertex grid and of the triangle grid on either
# side of a 256-thread workgroup, and one mesh of several workgroups with more triangles than vertices
SIZES = ((1, 1, 1), (255, 255, 3), (256, 256, 65536), (257, 257, 3), (300, 700, 65536))


# ---- the formulas, vectorised ------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, correctly rounded: the product is exact in float64; the sum is rounded to odd there
    (TwoSum gives its error), which makes the final rounding to float32 the only one that counts"""
    with np.errstate(all="ignore"):
        p, c = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        bits = s.view(np.int64).copy()
        adjust = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((bits & 1) == 0)
        away = (err > 0) == (s > 0)  # the exact sum lies further from zero than s
        bits = np.where(adjust, np.where(away, bits + 1, bits - 1), bits)
        return bits.view(np.float64).astype(F32)


def skin_vertices(mesh, bones):
    """V, N of the formulas; bones None: the rest vertices"""
    pos, nrm = mesh["position"], mesh["normal"]
    V, N = pos.copy(), None if nrm is None else nrm.copy()
    if bones is None:
        return V, N
    kept = np.zeros(len(pos), bool)
    with np.errstate(all="ignore"):
        for k in range(4):
            w = mesh["weight"][:, k]
            use = w != 0  # (+0 and -0 are skipped)
            q = bones[mesh["bone"][:, k].astype(np.int64)]
            first, later = use & ~kept, use & kept
            term = w[:, None] * P.transform(q, pos)
            V[first], V[later] = term[first], (V + term)[later]
            if N is not None:
                term = w[:, None] * P.rotate(q, nrm)
                N[first], N[later] = term[first], (N + term)[later]
            kept |= use
    assert V.dtype == F32 and (N is None or N.dtype == F32)
    return V, N


def triangles(mesh, V, N):
    i0, i1, i2 = (mesh["indices"][:, c].astype(np.int64) for c in range(3))
    half = F32(0.5)
    with np.errstate(all="ignore"):
        v1, e1, e2 = V[i0], V[i1] - V[i0], V[i2] - V[i0]
        if N is not None:
            n = (N[i0] * half + N[i1] * half) * half + N[i2] * half
        else:
            cx = e1[:, 1] * e2[:, 2] + (-e1[:, 2]) * e2[:, 1]
            cy = e1[:, 2] * e2[:, 0] + (-e1[:, 0]) * e2[:, 2]
            cz = e1[:, 0] * e2[:, 1] + (-e1[:, 1]) * e2[:, 0]
            d = fma32(cx, cx, fma32(cy, cy, cz * cz))
            r = F32(1) / np.sqrt(d)
            n = np.stack([cx * r, cy * r, cz * r], 1)
    out = dict(tri_v1=v1, tri_e1=e1, tri_e2=e2, tri_normal=n)
    assert all(a.dtype == F32 for a in out.values())
    return out


def expected(mesh, bones):
    """the arrays rt_skin_read / rt_skin_model give, from the numpy formulas (normal: None for a mesh without vertex normals)"""
    V, N = skin_vertices(mesh, bones)
    out = dict(position=V, normal=N)
    out.update(triangles(mesh, V, N))
    return out


def restated(mesh):
    """the arrays before any kernel ran: the rest mesh through the triangle formula"""
    return expected(mesh, None)


# ---- the library -------------------------------------------------------------------------------------------------------------------
def desc_of(mesh):
    return _abi.make_skin_desc(mesh["position"], mesh["normal"], mesh["indices"], mesh["bone"], mesh["weight"], mesh["n_bones"],
                               mesh["tri_first"], mesh["n_triangles"])


def empty_outputs(mesh):
    nv, nt = len(mesh["position"]), len(mesh["indices"])
    out = {k: np.full((nv if k in VERT_OUT else nt, 3), 7.0, F32) for k in OUT}
    if mesh["normal"] is None:
        out["normal"] = None
    return out


def pointers(out):
    return [None if out[k] is None else out[k].ctypes.data for k in OUT]


def model(mesh, bones):
    """rt_skin_model through ctypes on the built library -> the arrays in rt_skin_read's layout"""
    lib = _lib.load()
    d, keep = desc_of(mesh)
    out = empty_outputs(mesh)
    bones = np.ascontiguousarray(bones, F32)
    rc = lib.rt_skin_model(C.byref(d), bones.ctypes.data, *pointers(out))
    assert rc == 0, lib.rt_last_error()
    return out


def assert_same_words(got, want, nan_ok=False, what="", keys=OUT):
    """every output word bit-equal; nan_ok: two words that are both NaN count as equal (the exemption of
    pose_cases.assert_same_words: inf - inf has another sign bit on the device than in numpy)"""
    for k in keys:
        if want[k] is None:
            assert got[k] is None, (what, k)
            continue
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        differ = a.view(np.uint32) != b.view(np.uint32)
        if nan_ok:
            differ &= ~(np.isnan(a) & np.isnan(b))
        assert not differ.any(), f"{what} {k}: {int(differ.sum())} words differ, first at {np.argwhere(differ)[0]}: " \
                                 f"{a[differ][0]!r} != {b[differ][0]!r}"


# ---- seeded meshes -------------------------------------------------------------------------------------------------------------------
def zero_patterns(nv):
    """which of the four slots of vertex i carry a weight (bit k: slot k): all 16 patterns in turn, 15 (all four) first, 0 (no
    influence kept) among them"""
    return (np.arange(nv) * 7 + 15) % 16


def seeded_mesh(nv, nt, n_bones, normals, seed=None):
    """an indexed mesh of nv vertices and nt triangles inside a scene of nt + 2 (tri_first = 1).  Weights: every pattern of
    zero slots, the zeros alternately +0 and -0; the last vertex is on bone n_bones - 1 in slot 0 and is the last index of the
    last triangle."""
    r = np.random.default_rng(1000 + nv + nt if seed is None else seed)
    pos = r.uniform(-2, 2, (nv, 3)).astype(F32)
    nrm = r.uniform(-1, 1, (nv, 3)).astype(F32) if normals else None
    idx = r.integers(0, nv, (nt, 3))
    if nv >= 3:  # three distinct vertices per triangle: no degenerate face normal among the seeded cases
        idx[:, 1] = (idx[:, 0] + r.integers(1, nv, nt)) % nv
        while True:
            again = (idx[:, 2] == idx[:, 0]) | (idx[:, 2] == idx[:, 1])
            if not again.any():
                break
            idx[again, 2] = r.integers(0, nv, int(again.sum()))
        idx[-1] = (0, 1, nv - 1)
    idx = idx.astype(np.uint32)
    idx[-1, 2] = nv - 1
    bone = r.integers(0, n_bones, (nv, 4)).astype(np.uint16)
    weight = (r.uniform(0.05, 0.9, (nv, 4)) * r.choice([1.0, 1.0, 1.0, -1.0], (nv, 4))).astype(F32)
    pattern = zero_patterns(nv)
    pattern[-1] |= 1
    bone[-1, 0] = n_bones - 1
    zero = np.where((np.arange(nv) // 16) % 2 == 1, F32(-0.0), F32(0.0)).astype(F32)
    for k in range(4):
        off = (pattern >> k) & 1 == 0
        weight[off, k] = zero[off]
    return dict(position=pos, normal=nrm, indices=idx, bone=bone, weight=weight, n_bones=n_bones, tri_first=1, n_triangles=nt + 2)


def seeded_bones(n_bones, seed=3):
    """rows of 8 floats that are NOT normalised rotors: the library does not care"""
    r = np.random.default_rng(seed + n_bones)
    rows = r.uniform(-1.5, 1.5, (n_bones, 8)).astype(F32)
    rows[0] = _abi.transform_rows([P.transforms()["turn"]])[0]
    return rows


def seeded_cases():
    """[(label, mesh, bones)]: the five sizes in both normal modes"""
    out = []
    for nv, nt, nb in SIZES:
        for normals in (True, False):
            mesh = seeded_mesh(nv, nt, nb, normals)
            out.append((f"{nv} vertices, {nt} triangles, {nb} bones, {'vertex' if normals else 'face'} normals", mesh, seeded_bones(nb)))
    return out


# ---- edge values -----------------------------------------------------------------------------------------------------------------------
def edge_case(normals=True, seed=78):
    """4096 vertices, triangles and bones with fields built as pose_cases.edge_case builds its own -- quarters of subnormals,
    magnitudes whose products overflow (and meet as inf - inf), every exponent, random bits -- except the weights, which come
    from the three finite kinds only (create refuses a non-finite weight).  -> (mesh, bones)"""
    r = np.random.default_rng(seed)
    n, q = P.N_EDGE, P.N_EDGE // 4

    def field(shape, finite=False):
        cols = int(np.prod(shape[1:]))
        last = P.log_uniform(r, q * cols, -44, 38.5) if finite else P.random_floats(r, q * cols)
        a = np.concatenate([P.subnormals(r, q * cols), P.log_uniform(r, q * cols, 18, 38.5), P.log_uniform(r, q * cols, -44, 38.5), last])
        return np.ascontiguousarray(a.reshape(4, q, cols).reshape(n, cols).reshape(shape))

    pos, nrm, weight, bones = field((n, 3)), field((n, 3)) if normals else None, field((n, 4), finite=True), field((n, 8))
    assert np.isfinite(weight).all()
    bones[:8] = _abi.transform_rows([P.transforms()["identity"]] * 8)  # a few tame ones, against everything else
    bone = r.integers(0, n, (n, 4)).astype(np.uint16)
    bone[::5, 0] = r.integers(0, 8, len(bone[::5]))
    weight[::7, 1:] = 0  # single influences among them
    idx = np.stack([np.arange(n), r.integers(0, n, n), r.integers(0, n, n)], 1).astype(np.uint32)
    mesh = dict(position=pos, normal=nrm, indices=idx, bone=bone, weight=weight, n_bones=n, tri_first=0, n_triangles=n)
    return mesh, bones


# ---- a strip that bends ----------------------------------------------------------------------------------------------------------------
def strip_mesh(n_quads=20, length=1.0, width=0.25, normals=True):
    """a strip of 2 n_quads triangles along x in the plane z = 0, two bones: weights ramp linearly from bone 0 at x = 0 to
    bone 1 at x = length.  -> position, normal (or None), indices, bone, weight"""
    x = np.linspace(0.0, length, n_quads + 1)
    pos = np.stack([np.repeat(x, 2), np.tile([0.0, width], n_quads + 1), np.zeros(2 * (n_quads + 1))], 1).astype(F32)
    nrm = np.tile(np.array([0.0, 0.0, -1.0], F32), (len(pos), 1)) if normals else None
    tri = []
    for k in range(n_quads):
        a, b, c, d = 2 * k, 2 * k + 1, 2 * k + 2, 2 * k + 3
        tri += [(a, b, c), (c, b, d)]  # (normals -z: towards a camera in front of the scene)
    w1 = (pos[:, 0] / F32(length)).astype(F32)
    weight = np.stack([F32(1) - w1, w1, np.zeros_like(w1), np.zeros_like(w1)], 1).astype(F32)
    bone = np.tile(np.array([0, 1, 0, 0], np.uint16), (len(pos), 1))
    return pos, nrm, np.asarray(tri, np.uint32), bone, weight


# ---- whole scenes with a skinned mesh in them ------------------------------------------------------------------------------------------
def ramp_weights(position, axis=None):
    """two bones: the weight of bone 1 ramps linearly from 0 to 1 along the mesh's long axis, bone 0 takes the rest"""
    lo, hi = position.min(0), position.max(0)
    axis = int(np.argmax(hi - lo)) if axis is None else axis
    w1 = ((position[:, axis] - lo[axis]) / (hi[axis] - lo[axis])).astype(F32)
    zero = np.zeros_like(w1)
    return np.tile(np.array([0, 1, 0, 0], np.uint16), (len(position), 1)), np.stack([F32(1) - w1, w1, zero, zero], 1).astype(F32)


def with_mesh(flat, mesh, bones):
    """`flat` with the skin's triangle range replaced by the model's arrays under `bones`"""
    import scene_update_cases as cases

    g = model(mesh, bones)
    lo, hi = mesh["tri_first"], mesh["tri_first"] + len(mesh["indices"])
    changed = {}
    for k in TRI_OUT:
        a = np.array(getattr(flat, k), copy=True)
        a[lo:hi] = g[k]
        changed[k] = a
    return cases.copy(flat, **changed)


def semesterbild_skin(model_name="text_lowres"):
    """-> (flat0, mesh): semesterbild's text mesh (text_lowres, or the full text mesh) as a skin of two bones.  The rest mesh
    is the mesh AS PLACED in the scene (the unified vertices under semesterbild's transform, from the model), so that bones
    are transforms of scene space; flat0 is the scene with the mesh restated by the model under two identities."""
    from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, scenes
    from hslu_i.ba_raytracing.f2501_raytracer_amd.obj import load_indexed_mesh

    cfg = RenderConfig.from_features([])
    flat = scenes.semesterbild(cfg, model=model_name).flatten().contiguous()
    m = load_indexed_mesh(scenes.mesh_path(cfg, model_name))
    nv = len(m.position)
    one = dict(position=m.position, normal=m.normal, indices=m.indices, bone=np.zeros((nv, 4), np.uint16),
               weight=np.tile(np.array([1, 0, 0, 0], F32), (nv, 1)), n_bones=1, tri_first=0, n_triangles=flat.n_triangles)
    placed = model(one, _abi.transform_rows([scenes.semesterbild_text_transform(cfg)]))
    bone, weight = ramp_weights(placed["position"])
    mesh = dict(position=placed["position"], normal=placed["normal"], indices=m.indices, bone=bone, weight=weight, n_bones=2, tri_first=0,
                n_triangles=flat.n_triangles)
    return with_mesh(flat, mesh, identity_bones(2)), mesh


def strip_scene(normals=True, seed=12):
    """-> (flat0, mesh): a seeded strip of 40 triangles and two bones in front of a wall triangle, in the frame of the default
    camera; the strip is canonical triangles [1, 41) of 41"""
    from test_scene_pack_host import flat_of

    pos, nrm, idx, bone, weight = strip_mesh(20, 0.5, 0.25, normals)
    r = np.random.default_rng(seed)
    pos = (pos + [0.25, 0.3, 0.45] + r.uniform(-0.004, 0.004, pos.shape) * [1, 1, 0]).astype(F32)
    nt = len(idx) + 1
    mesh = dict(position=pos, normal=nrm, indices=idx, bone=bone, weight=weight, n_bones=2, tri_first=1, n_triangles=nt)
    z = np.zeros((nt, 3))
    v1, e1, e2, n = z.copy(), z.copy(), z.copy(), z.copy()
    v1[0], e1[0], e2[0], n[0] = (-1.0, -1.0, 0.9), (3.0, 0.0, 0.0), (0.0, 3.0, 0.0), (0.0, 0.0, -1.0)
    e1[1:, 0], e2[1:, 1], n[1:, 2] = 0.1, 0.1, -1.0  # (placeholders: the model's arrays replace them)
    flat = flat_of(v1=v1, e1=e1, e2=e2, nrm=n, tm=[1] + [0] * (nt - 1),
                   mats=[[0.9, 0.6, 0.2, 0.1, 0.4, 1.0, 0.0, 0.0, 0.0], [0.5, 0.75, 0.75, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]],
                   lights=[[0.8, 0.1, 0.0, 1.0, 1.0, 1.0, 0.9]]).contiguous()
    return with_mesh(flat, mesh, identity_bones(2)), mesh


def identity_bones(n):
    return _abi.transform_rows([P.transforms()["identity"]] * n)


def about(centre, rotor, scale=1.0, shift=(0.0, 0.0, 0.0)):
    """the similarity that turns by `rotor` and scales by `scale` about `centre`, then shifts"""
    from hslu_i.ba_raytracing.f2501_raytracer_amd.f32math import Similarity3, Vec3

    c = Vec3(*centre)
    return Similarity3(c - rotor.rotate_vec(c) * F32(scale) + Vec3(*shift), rotor, scale)


def yaw(degrees):
    """the rotor of a turn about the vertical (y) axis: the xz plane"""
    from hslu_i.ba_raytracing.f2501_raytracer_amd.f32math import Rotor3

    return Rotor3.from_rotation_xz(np.deg2rad(degrees))


def bend(mesh, degrees, scale=1.0, shift=(0.0, 0.0, 0.0)):
    """bones of a bend: bone 0 the identity, bone 1 a turn by `degrees` about the vertical axis through the mesh's centre"""
    c = 0.5 * (mesh["position"].astype(np.float64).min(0) + mesh["position"].astype(np.float64).max(0))
    return _abi.transform_rows([P.transforms()["identity"], about(c, yaw(degrees), scale, shift)])


def four_steps(mesh):
    """[(label, bones)]: bend, bend further, bend with a scaled bone, back to rest"""
    return [("bend", bend(mesh, 15.0)), ("bend further", bend(mesh, 40.0, 1.0, (0.01, -0.005, 0.0))), ("scaled bone", bend(mesh, 40.0, 0.8)),
            ("back to rest", identity_bones(2))]
