"""An independent float64 brute force for the closest-point queries, in numpy: every point against every object.  A triangle
is handled by the textbook route -- project the point onto the plane, keep the projection when it lies inside (edge functions
against the normal), otherwise take the nearest of the three clamped segment projections; a triangle without a usable normal is
its three segments.  Not a restatement of csrc/rt_closest.h: other formulas, other order, float64 throughout."""
import numpy as np


def _segment(p, a, b):
    """nearest points of segments a -> b to points p (all (..., 3)) -> (q, d)"""
    e = b - a
    ee = (e * e).sum(-1)
    t = np.where(ee > 0, ((p - a) * e).sum(-1) / np.where(ee > 0, ee, 1.0), 0.0)
    t = np.clip(t, 0.0, 1.0)
    q = a + t[..., None] * e
    return q, np.linalg.norm(q - p, axis=-1)


def triangles(p, v1, e1, e2):
    """p (m, 3) against triangles (k, 3) -> (q (m, k, 3), d (m, k)), float64"""
    p = p[:, None, :]
    a, b, c = v1[None], (v1 + e1)[None], (v1 + e2)[None]
    n = np.cross(e1, e2)[None]
    nn = (n * n).sum(-1)
    ok = nn > 1e-300
    nn1 = np.where(ok, nn, 1.0)
    s = ((p - a) * n).sum(-1) / nn1
    proj = p - s[..., None] * n
    # inside: the projection is on the inner side of all three edges
    inside = ok
    for x, y in ((a, b), (b, c), (c, a)):
        inside = inside & ((np.cross(y - x, proj - x) * n).sum(-1) >= 0.0)
    q = np.where(inside[..., None], proj, 0.0)
    d = np.where(inside, np.abs(s) * np.sqrt(nn1), np.inf)
    for x, y in ((a, b), (a, c), (b, c)):
        qs, ds = _segment(p, x, y)
        better = ~inside & (ds < d)
        q = np.where(better[..., None], qs, q)
        d = np.where(better, ds, d)
    return q, d


def spheres(p, c, r_sq):
    """-> (q (m, k, 3), d (m, k)); the direction at the centre is (1, 0, 0)"""
    w = p[:, None, :] - c[None]
    l = np.linalg.norm(w, axis=-1)
    r = np.sqrt(r_sq)[None]
    dirn = np.where((l > 0)[..., None], w / np.where(l > 0, l, 1.0)[..., None], np.array([1.0, 0.0, 0.0]))
    return c[None] + dirn * r[..., None], np.abs(l - r)


def brute(flat, pts, chunk=64):
    """-> (dmin (n,), of): the float64 minimum distance over all objects of every point, and of(ids) -> (q, d), the float64
    closest point / distance of object ids[i] for point i (canonical ids: spheres first; -1: none)"""
    P = np.asarray(pts, np.float64)
    n = P.shape[0]
    c, r_sq = flat.sphere_center.astype(np.float64).reshape(-1, 3), flat.sphere_r_sq.astype(np.float64)
    v1, e1, e2 = (a.astype(np.float64).reshape(-1, 3) for a in (flat.tri_v1, flat.tri_e1, flat.tri_e2))
    ns = c.shape[0]
    dmin = np.full(n, np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(0, n, chunk):
            p = P[i:i + chunk]
            if ns:
                dmin[i:i + chunk] = np.minimum(dmin[i:i + chunk], spheres(p, c, r_sq)[1].min(axis=1))
            if v1.shape[0]:
                dmin[i:i + chunk] = np.minimum(dmin[i:i + chunk], triangles(p, v1, e1, e2)[1].min(axis=1))

    def of(ids):
        ids = np.asarray(ids)
        q, d = np.zeros((n, 3)), np.full(n, np.inf)
        with np.errstate(invalid="ignore", over="ignore"):
            for i in np.nonzero(ids >= 0)[0]:
                k = int(ids[i])
                if k < ns:
                    qq, dd = spheres(P[i:i + 1], c[k:k + 1], r_sq[k:k + 1])
                else:
                    t = k - ns
                    qq, dd = triangles(P[i:i + 1], v1[t:t + 1], e1[t:t + 1], e2[t:t + 1])
                q[i], d[i] = qq[0, 0], dd[0, 0]
        return q, d

    return dmin, of


def scale_of(flat, pts, ids):
    """max(|p|_inf, largest |coordinate| of object ids[i]) per point (1 where there is no object)"""
    P = np.abs(np.asarray(pts, np.float64)).max(axis=1)
    ns = flat.n_spheres
    c, r = flat.sphere_center.astype(np.float64).reshape(-1, 3), np.sqrt(np.abs(flat.sphere_r_sq.astype(np.float64)))
    v1, e1, e2 = (a.astype(np.float64).reshape(-1, 3) for a in (flat.tri_v1, flat.tri_e1, flat.tri_e2))
    big_s = (np.abs(c) + r[:, None]).max(axis=1) if ns else np.zeros(0)
    big_t = np.abs(np.stack([v1, v1 + e1, v1 + e2])).max(axis=(0, 2)) if v1.shape[0] else np.zeros(0)
    big = np.concatenate([big_s, big_t, [0.0]])
    ids = np.asarray(ids)
    return np.maximum(P, big[np.where(ids >= 0, ids, len(big) - 1)])
