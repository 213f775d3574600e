"""The fat-beam rule of rt_flags_kernel as designed, checked on the CPU before any GPU is involved (flags_cases.py: scenes and
references, f64_fat_beam.py: the rule in float64).

1. The rule is sound: every leaf slot the oracle's literal triangle test accepts (EPS < t <= tmax) for any shadow ray the
   render can cast from a cell -- the hit points and light points of test_cell_prune_host.py -- is kept or near by the f64
   rule.  Every slot whose box meets the padded box of the cell's hull and the light's ball is offered.  Zero tolerance,
   nothing excluded.
2. The near band is narrow: at most 2 % of the triples the rule rejects, per scene.  A condition on the scenes.
3. The render's receiver lookup (receiver_cell, restated in float32 from the packed blob) maps a hit point to an active cell
   whose enlarged hull contains it within 4e-7 |p|_1: lookup and kernel share the i / j order and the face numbering.
4. The sphere literal test is the oracle's (rt_oracle_sphere), as `literal` is the oracle's triangle test.
5. Ablation: with the t-rejection taken at the cell's centre only, item 1 fails -- the scenes can see such a mistake."""
import ctypes as C

import numpy as np
import pytest

import f64_fat_beam as fb
import flags_cases as fc
import oracle_lib

F32 = np.float32
pytestmark = pytest.mark.skipif(not fc.have_hipcc(), reason="no hipcc")


def figures(name, R):
    k = R.k
    rej, near = fc.near_share(R)
    return (f"{name}: {k.n_cells} cells ({int(k.active.sum())} active), {k.dev['n_lights']} lights, {k.dev['n_slots']} slots; literal test on {len(R.checked)} cells, "
            f"{R.offered} triples, {R.rays} rays: accepted {sum(len(v) for v in R.accepted.values())}; f64 rule on {len(R.f64_cells)} cells: kept or near "
            f"{sum(int((~v).sum()) for v in R.clear.values())}, rejected {rej}, near band {near} ({100.0 * near / max(rej, 1):.2f} %)")


@pytest.mark.parametrize("name", fc.SCENES)
def test_every_literally_accepted_slot_is_kept_by_the_rule(name):
    R = fc.reference(name)
    print(figures(name, R))
    assert R.offered > 0 and R.rays > 0
    bad = fc.unsound(R)
    assert not bad, f"accepted by the literal test, clearly rejected by the rule (cell, light, slot): {bad[:10]}"
    # the numpy restatements are the oracle's tests: same verdict and same t on a sample of the rays just cast
    lib = oracle_lib.load()
    fp = C.POINTER(C.c_float)
    k = R.k
    for s, o, d, valid, t in R.sample_rays:
        out = np.zeros(4, F32)
        got = lib.rt_oracle_triangle(C.byref(k.desc), int(k.tri_id[s]), o.ctypes.data_as(fp), d.ctypes.data_as(fp), 0, out.ctypes.data_as(fp))
        assert bool(got) == valid and (not got or abs(float(out[0]) - t) <= 5e-7 * abs(t)), (s, o, d, valid, t, got, out)


def test_the_scenes_reach_what_they_aim_at():
    """conditions on the inputs: the literal test accepts something everywhere, the ragged scene is ragged, the grazing one grazes"""
    for name in fc.SCENES:
        R = fc.reference(name)
        assert any(R.accepted.values()), name
    k = fc.case("ragged")
    o = k.dev["off_recv"]
    Rs = sorted(int(v) for v in k.blob[o:o + 48 * k.dev["n_triangles"]].view(np.uint32).reshape(-1, 12)[:, 8])
    assert k.n_cells == fc.RAGGED_CELLS and k.n_cells % 64 == 1 and Rs[:2] == [0, 1], (k.n_cells, Rs)
    k = fc.case("grazing")
    c1 = k.lights[1].astype(np.float64) + k.consts.cloud_centre
    assert min(np.linalg.norm(k.hulls[c][0] - c1) for c in range(k.n_cells) if k.active[c]) < k.consts.beam_delta, "a cell centre inside the cloud's ball"
    assert fc.case("eight_lights").dev["n_lights"] == 8
    k, R = fc.case("sphere_edges"), fc.reference("sphere_edges")
    assert k.n_cells > k.n_tri_cells and any(R.sphere_hit.values()) and not all(R.sphere_hit.values())
    assert any(v[2].all() for v in R.sph.values()), "some cell has every sphere clearly out of reach"


@pytest.mark.parametrize("name", fc.SCENES)
def test_the_near_band_is_narrow(name):
    R = fc.reference(name)
    rej, near = fc.near_share(R)
    print(f"{name}: rejected {rej}, near band {near} = {100.0 * near / max(rej, 1):.3f} %")
    assert near <= fc.NEAR_CAP * rej, (name, rej, near)


@pytest.mark.parametrize("name", ["behind_and_through", "sphere_edges", "sphere_receiver", "ragged", "far_and_tiny_far", "synthetic"])
def test_receiver_lookup_lands_in_a_cell_whose_hull_holds_the_point(name):
    k = fc.case(name)
    rng = np.random.default_rng(5)
    ns, nt = k.dev["n_spheres"], k.dev["n_triangles"]
    flat = k.flat
    n_pts = n_none = 0
    worst = 0.0

    def check(prim, p, may_miss):
        nonlocal n_pts, n_none, worst
        p = np.asarray(p, F32)
        cell = fc.receiver_cell(k, prim, p)
        n_pts += 1
        if cell is None:
            n_none += 1
            assert may_miss, (prim, p)
            return
        assert 0 <= cell < k.n_cells and k.active[cell], (prim, p, cell)
        pm, pt = k.hulls[cell]
        out = fc.outside_hull(pm, pt, p)
        tol = 4e-7 * float(np.abs(p.astype(np.float64)).sum())
        worst = max(worst, out / tol)
        assert out <= tol, (prim, p, cell, out, tol)

    def via_ray(q):
        """p = fl(o + t d) for a ray that starts near the scene and aims at q"""
        o = (q + rng.normal(0, 1, 3) * 0.5 * k.scene_size).astype(F32)
        dv = q.astype(np.float64) - o
        t = F32(np.linalg.norm(dv))
        d = (dv / np.linalg.norm(dv)).astype(F32)
        return np.array([fc._fma(d[i], t, o[i]) for i in range(3)], F32)

    for t in range(nt):
        v1, e1, e2 = (a[t].astype(np.float64) for a in (flat.tri_v1, flat.tri_e1, flat.tri_e2))
        o = k.dev["off_recv"] + t * 48
        R = int(k.blob[o + 32:o + 36].view(np.uint32)[0])
        if R == 0:
            check(ns + t, v1 + 0.3 * e1 + 0.3 * e2, True)
            continue
        uv = list(rng.dirichlet(np.ones(3), 24)[:, :2])
        for _ in range(24):  # within 1e-6 of a cell border, of the hypotenuse, and of both
            i, j = int(rng.integers(R)), int(rng.integers(R))
            sg = rng.choice([-1e-6, 1e-6])
            uv += [(min(max(i / R + sg, 0.0), 1.0), rng.random() * (1 - i / R) * 0.999), (rng.random() * (1 - j / R) * 0.999, min(max(j / R + sg, 0.0), 1.0))]
            u = rng.random()
            uv += [(u, 1.0 - u - 1e-6), (i / R + sg, max(1.0 - i / R - sg - 1e-6, 0.0))]
        for u, v in uv:
            if u < 0 or v < 0 or u + v >= 1:
                continue
            q = v1 + u * e1 + v * e2
            near_hyp = u + v >= 1.0 - 1e-5  # (a point this close to the hypotenuse may round across it: no cell, no flags, a walk)
            check(ns + t, q, near_hyp)
            check(ns + t, via_ray(q.astype(F32)), near_hyp)
    for s in range(ns):
        ctr, rad = k.spheres[s, :3].astype(np.float64), float(np.sqrt(k.spheres[s, 3]))
        o = k.dev["off_srecv"] + s * 8
        Rs = int(k.blob[o:o + 4].view(np.uint32)[0])
        dirs = list(rng.normal(0, 1, (48, 3)))
        for sx in (1, -1):
            for sy in (1, -1):
                for sz in (1, -1):
                    dirs += [np.array([sx, sy, sz], float), np.array([sx, sy, sz * 0.999999]), np.array([sx * 0.999999, sy, sz])]          # corners
                    dirs += [np.array([sx, sy, sz * rng.random()]), np.array([sx, sy * rng.random(), sz]), np.array([sx * rng.random(), sy, sz])]  # edges
        for _ in range(24):  # within 1e-6 of a cell border of the cube map
            i = int(rng.integers(max(Rs, 1)))
            a = 2.0 * i / max(Rs, 1) - 1.0 + rng.choice([-1e-6, 1e-6])
            d = np.array([1.0, a, rng.uniform(-1, 1)])
            dirs.append(np.roll(d, int(rng.integers(3))) * rng.choice([-1, 1]))
        for d in dirs:
            q = ctr + rad * d / np.linalg.norm(d)
            check(s, q, Rs == 0)
            check(s, via_ray(q.astype(F32)), Rs == 0)
    print(f"{name}: {n_pts} hit points on {nt} triangles and {ns} spheres, {n_none} without a cell, worst distance outside a hull {worst:.3f} of 4e-7 |p|_1")
    assert n_pts > 100 and n_none < n_pts // 4


@pytest.mark.parametrize("name", ["sphere_edges", "sphere_receiver", "synthetic"])
def test_the_sphere_literal_test_is_the_oracles(name):
    R = fc.reference(name)
    lib = oracle_lib.load()
    fp = C.POINTER(C.c_float)
    assert len(R.sample_sphere_rays) >= 16
    hits = 0
    for i, o, d, hit, t in R.sample_sphere_rays:
        out = np.zeros(7, F32)
        got = lib.rt_oracle_sphere(C.byref(R.k.desc), i, o.ctypes.data_as(fp), d.ctypes.data_as(fp), 0, out.ctypes.data_as(fp))
        hits += bool(got)
        assert bool(got) == hit and (not got or abs(float(out[0]) - t) <= 5e-7 * abs(t)), (i, o, d, hit, t, got, out)
    print(f"{name}: {len(R.sample_sphere_rays)} rays, {hits} hits")


def test_the_t_rejection_at_the_centre_only_is_caught():
    """a single-term ablation of the rule: the t-rejection taken at the cell's centre instead of its 8 hull points rejects slots
    the literal test accepts from the cell's rim -- the scenes can see such a mistake.  (The other ablation, fb.r left out of
    delta, only removes slack the 1-norm bounds have to spare: it shows in what the kernel lists, test_flags_kernel_gpu.py)"""
    caught = {}
    for name in ("behind_and_through", "grazing", "eight_lights", "ragged", "sphere_edges"):
        R = fc.reference(name)
        clear = {(c, l): fb.triangles(fc.beam_of(R.k, c, l), R.k.isect, centre_only=True)[1] for (c, l) in R.accepted}
        bad = fc.unsound(R, clear)
        if bad:
            caught[name] = len(bad)
    print(f"accepted slots the ablated rule clearly rejects, per scene: {caught}")
    assert caught, "no scene sees the mistake"
