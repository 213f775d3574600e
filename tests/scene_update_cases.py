"""Scenes and scene edits shared by the in-place update tests (host model and GPU): what moves, by how much, in which
order.  Everything is a FlatScene -> FlatScene function with a seeded generator, so the host model, the device and a fresh
handle all see the same arrays."""
import numpy as np

from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, scenes
from hslu_i.ba_raytracing.f2501_raytracer_amd.scene import FlatScene

F32 = np.float32


def flat_test_scene(cfg=None):
    return scenes.test_scene(cfg or RenderConfig.from_features([])).flatten().contiguous()


def flat_semesterbild(cfg=None):
    return scenes.semesterbild(cfg or RenderConfig.from_features([]), model="text_lowres").flatten().contiguous()


def plane_triangles():
    """triangles of one BoundedPlane: test_scene is 3 loose triangles and 7 planes"""
    nt = flat_test_scene().n_triangles
    assert (nt - 3) % 7 == 0
    return (nt - 3) // 7


def mesh_range(name, flat):
    """(first, count) of the triangles the edits treat as "the mesh": semesterbild's text mesh (it is loaded first, four
    planes follow); in test_scene the two tilted planes behind the three loose triangles"""
    m = plane_triangles()
    if name == "semesterbild":
        return 0, flat.n_triangles - 4 * m
    if name == "test_scene":
        return 3, 2 * m
    return 0, flat.n_triangles


def copy(flat, **changed):
    f = {k: np.array(getattr(flat, k), copy=True) for k in FlatScene.__dataclass_fields__}
    f.update(changed)
    return FlatScene(**f).contiguous()


def diagonal(flat):
    r = np.sqrt(np.abs(flat.sphere_r_sq.astype(np.float64)))[:, None]
    pts = np.concatenate([flat.sphere_center - r, flat.sphere_center + r, flat.tri_v1, flat.tri_v1 + flat.tri_e1, flat.tri_v1 + flat.tri_e2])
    return float(np.linalg.norm(pts.max(0) - pts.min(0))) if len(pts) else 1.0


def turn_mesh(flat, rng, degrees=20.0, shift=(0.0, 0.0, 0.0)):
    """a rigid turn about y through the centroid of triangles [first, first + count), plus a translation"""
    first, count = rng
    s = slice(first, first + count)
    a = np.deg2rad(degrees)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    v1, e1, e2, n = (getattr(flat, k).astype(np.float64) for k in ("tri_v1", "tri_e1", "tri_e2", "tri_normal"))
    if count:
        c = np.concatenate([v1[s], v1[s] + e1[s], v1[s] + e2[s]]).mean(0)
        v1[s] = (v1[s] - c) @ R.T + c + np.asarray(shift, np.float64)
        e1[s], e2[s], n[s] = e1[s] @ R.T, e2[s] @ R.T, n[s] @ R.T
    return copy(flat, tri_v1=v1.astype(F32), tri_e1=e1.astype(F32), tri_e2=e2.astype(F32), tri_normal=n.astype(F32))


def jitter(flat, fraction=0.05, seed=5):
    """every vertex of every triangle moves by up to `fraction` of the scene diagonal; normals follow their triangles"""
    r = np.random.default_rng(seed)
    nt = flat.n_triangles
    amp = fraction * diagonal(flat)
    j = r.uniform(-amp, amp, (3, nt, 3))
    v1, e1, e2, n = (getattr(flat, k).astype(np.float64) for k in ("tri_v1", "tri_e1", "tri_e2", "tri_normal"))
    p1, p2, p3 = v1 + j[0], v1 + e1 + j[1], v1 + e2 + j[2]
    nn = np.cross(p2 - p1, p3 - p1)
    nn /= np.maximum(np.linalg.norm(nn, axis=1, keepdims=True), 1e-300)
    nn *= np.where((nn * n).sum(1, keepdims=True) < 0, -1.0, 1.0)  # (the side the old normal pointed to)
    return copy(flat, tri_v1=p1.astype(F32), tri_e1=(p2 - p1).astype(F32), tri_e2=(p3 - p1).astype(F32), tri_normal=nn.astype(F32))


def move_spheres(flat, seed=6, fraction=0.03):
    r = np.random.default_rng(seed)
    c = flat.sphere_center.astype(np.float64) + r.uniform(-1, 1, flat.sphere_center.shape) * fraction * diagonal(flat)
    r_sq = (flat.sphere_r_sq.astype(np.float64) * r.uniform(0.8, 1.2, flat.sphere_r_sq.shape)).astype(F32)
    with np.errstate(divide="ignore"):
        r_inv = (F32(1) / np.sqrt(np.abs(r_sq))).astype(F32)
    return copy(flat, sphere_center=c.astype(F32), sphere_r_sq=r_sq, sphere_r_inv=r_inv)


def orbit_lights(flat, degrees=25.0):
    """every light turns about the vertical axis through the centre of the scene's objects"""
    li = flat.lights.astype(np.float64)
    pts = np.concatenate([flat.sphere_center, flat.tri_v1]).astype(np.float64)
    c = pts.mean(0) if len(pts) else np.zeros(3)
    a = np.deg2rad(degrees)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    li[:, 0:3] = (li[:, 0:3] - c) @ R.T + c
    return copy(flat, lights=li.astype(F32))


def recolour(flat, seed=7):
    """colours, shininess and ior change; has_opacity and opacity -- the transmissive class -- stay"""
    r = np.random.default_rng(seed)
    m = flat.materials.astype(np.float64)
    m[:, 0:3] = np.clip(m[:, 0:3] * r.uniform(0.5, 1.0, (len(m), 3)), 0, 1)
    m[:, 4] = np.clip(m[:, 4] + 0.1, 0, 1)
    m[:, 5] = m[:, 5] * 1.05
    return copy(flat, materials=m.astype(F32))


def animation(name, flat):
    """the scripted six steps: [(label, FlatScene)], each applied on top of the one before; the last is the start again"""
    rng = mesh_range(name, flat)
    d = diagonal(flat)
    s1 = orbit_lights(flat)
    s2 = move_spheres(s1)
    s3 = turn_mesh(s2, rng, 20.0, (0.01 * d, -0.005 * d, 0.0))
    s4 = jitter(s3, 0.05)
    s5 = recolour(s4)
    return [("light orbit", s1), ("sphere move", s2), ("mesh turn", s3), ("5 % jitter", s4), ("material colours", s5), ("back to the start", flat)]
