"""The fat-beam rule of rt_flags_kernel (csrc/rt_kernels.hip: collect_light_candidates<.., COLLECT_FLAGS>, beam_rejects_all)
restated in plain numpy float64, from the inequalities in the kernel's comments.  No box walk: box tests only ever remove
more, so "listed by the kernel => not clearly rejected here" holds without them.

The beam of a receiver cell for one light: centre p of the cell, the 8 points pt of its enlarged hull, the light cloud's
centre c.  With r = max_k |pt_k - p|_1:

  fb.r   = 1.0001 r + 4e-7 |p|_1                    every point of the cell lies within fb.r (1-norm) of p
  delta  = beam_delta + fb.r                        directions within delta of dseg = c - p
  len    = max(|dseg|, 1e-20),  lenp = len + delta
  t_push = beam_eps_push / lenp
  p_max  = max_i |p_i| + fb.r
  p_ulp  = 4e-7 (|p|_1 + fb.r) + beam_eps_ulp      a hit point lies off its surface by the rounding of o + t d, 4e-7 |p|_1
  eps_o  = 2.6e-7 p_max + beam_eps_o + fb.r + 4e-7 p_max      origins within eps_o of p

and for a leaf slot {v1, e1, e2, X} with c1 = -e1, c2 = -e2, b = v1 - p, b_k = v1 - pt_k:

  det    = dseg.X,  ad = |det|,  sgn = sign(det),  X1 = |X|_1,  B = |b|_1 + eps_o
  dslack = delta X1 + 2e-6 lenp X1
  geo    = delta B + lenp eps_o + 2e-6 lenp B
  closed : ad > 1.001 dslack                                   (otherwise the sign of det is unknown: `open`, kept)
  t      : 4e-6 sum_i |X_i b_k,i| + X1 p_ulp + sgn X.b_k < t_push (ad - dslack)     at EVERY one of the 8 hull points
  u      : sgn (c2 x dseg).b + |c2|_1 geo < 0
  v      : sgn (dseg x c1).b + |c1|_1 geo < 0
  u + v  : sgn (c2 x dseg).b + sgn (dseg x c1).b - ad - (|c1|_1 + |c2|_1) geo - dslack - 2e-6 ad > 0

A slot is rejected when it is closed and at least one of t, u, v, u + v holds; everything else is kept.

Verdicts.  Every inequality is evaluated as (margin, S): margin = the amount by which it holds, S = the sum of the absolute
values of the terms it is made of (products taken apart down to the coordinates).  An inequality holds CLEARLY when
margin > NEAR * S.  A slot is *clearly rejected* when `closed` holds clearly and at least one rejection holds clearly (t: at
all 8 points); everything else is *kept or near*.  The *near band* is what the rule rejects, but not clearly.

NEAR.  The kernel evaluates each side of an inequality in float32 with at most about 20 operations (products, fused
multiply-adds, rcpf of lenp included), each correct to 1 ulp = 2^-24 = 6e-8 relative to its result, and every
intermediate result is bounded by S.  The computed margin is therefore off by at most 20 * 6e-8 * S = 1.2e-6 S.  The hull
points come out of a different float32 sequence on the device (fused multiply-adds, rsqf, rcpf) than on the host, a
difference of a few ulp of the coordinates, which moves each term by the same order.  Eight times the first figure,
9.5e-6, rounded: NEAR = 1e-5.  It is derived, not tuned: a case that misses it is a finding.

The sphere bit restates the same way: the distance q of the sphere's centre from the centre segment against
reach = rad + delta, near when |q|^2 <= 1.0002 reach^2 + 1e-12."""
import numpy as np

NEAR = 1e-5


class Consts:
    """beam constants of a frame (rt_beam_constants) and the cloud's centre"""

    def __init__(self, beam_delta, beam_eps_push, beam_eps_ulp, beam_eps_o, cloud_centre):
        self.beam_delta, self.beam_eps_push, self.beam_eps_ulp, self.beam_eps_o = (float(v) for v in (beam_delta, beam_eps_push, beam_eps_ulp, beam_eps_o))
        self.cloud_centre = np.asarray(cloud_centre, np.float64)


class Beam:
    pass


def cell_beam(k, pm, pt, light, drop_r=False):
    """the fat beam of the cell (centre pm, hull pt[8]) towards `light`; drop_r: the ablation that leaves fb.r out of delta"""
    B = Beam()
    B.p, B.pt = np.asarray(pm, np.float64), np.asarray(pt, np.float64)
    B.c = np.asarray(light, np.float64) + k.cloud_centre
    r = np.abs(B.pt - B.p).sum(1).max()
    B.r = r * 1.0001 + 4e-7 * np.abs(B.p).sum()
    B.delta = k.beam_delta + (0.0 if drop_r else B.r)
    B.dseg = B.c - B.p
    B.len = max(np.linalg.norm(B.dseg), 1e-20)
    B.lenp = B.len + B.delta
    B.t_push = k.beam_eps_push / B.lenp
    B.p_max = np.abs(B.p).max() + B.r
    B.p_ulp = 4e-7 * (np.abs(B.p).sum() + B.r) + k.beam_eps_ulp
    B.eps_o = 2.6e-7 * B.p_max + k.beam_eps_o + B.r + 4e-7 * B.p_max
    return B


def _cross_abs(a, b):
    """sum of the absolute products of a x b, per component"""
    a, b = np.abs(a), np.abs(b)
    return np.stack([a[..., 1] * b[..., 2] + a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] + a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]], -1)


def triangles(B, Q, centre_only=False, near=NEAR):
    """verdicts for the leaf records Q [S, 12] -> (rejected, clearly_rejected), bool [S]; centre_only: the ablation that takes
    the t-rejection at the cell's centre instead of its 8 hull points; near: the width of the band (negative: the second
    result is "rejected, or kept by less than |near| S", its complement *clearly kept*)"""
    Q = np.asarray(Q, np.float64).reshape(-1, 12)
    v1, c1, c2, x = Q[:, 0:3], -Q[:, 3:6], -Q[:, 6:9], Q[:, 9:12]
    dseg = B.dseg[None]
    b = v1 - B.p
    det = (x * dseg).sum(1)
    s_det = np.abs(x * dseg).sum(1)
    ad = np.abs(det)
    sgn = np.where(np.signbit(det), -1.0, 1.0)
    X1 = np.abs(x).sum(1)
    Bn = np.abs(b).sum(1) + B.eps_o
    geo = B.delta * Bn + B.lenp * B.eps_o + 2e-6 * B.lenp * Bn
    dslack = B.delta * X1 + 2e-6 * B.lenp * X1

    def verdict(margin, S):
        return margin > 0.0, margin > near * S

    closed, closed_c = verdict(ad - 1.001 * dslack, s_det + 1.001 * dslack)
    # t, at every hull point
    pts = B.p[None] if centre_only else B.pt
    rhs = B.t_push * (ad - dslack)
    t, t_c = np.ones(len(Q), bool), np.ones(len(Q), bool)
    for pk in pts:
        bk = v1 - pk
        sk = np.abs(x * bk).sum(1)
        xk = sgn * (x * bk).sum(1)
        h, hc = verdict(rhs - (4e-6 * sk + X1 * B.p_ulp + xk), B.t_push * (s_det + dslack) + 4e-6 * sk + X1 * B.p_ulp + sk)
        t &= h
        t_c &= hc
    # u, v, u + v
    y, z = np.cross(c2, dseg), np.cross(dseg, c1)
    ybs, zbs = sgn * (y * b).sum(1), sgn * (z * b).sum(1)
    s_y, s_z = (_cross_abs(c2, dseg) * np.abs(b)).sum(1), (_cross_abs(dseg, c1) * np.abs(b)).sum(1)
    su, sv = np.abs(c2).sum(1) * geo, np.abs(c1).sum(1) * geo
    u, u_c = verdict(-(ybs + su), s_y + su)
    v, v_c = verdict(-(zbs + sv), s_z + sv)
    w, w_c = verdict((ybs + zbs) - ad - (su + sv) - dslack - 2e-6 * ad, s_y + s_z + s_det + su + sv + dslack + 2e-6 * ad)
    return closed & (t | u | v | w), closed_c & (t_c | u_c | v_c | w_c)


def spheres(B, centres, rad):
    """the sphere bit: per sphere (near, clearly near, clearly far) for the centres [n, 3] and the radii' upper bounds [n]"""
    centres, rad = np.asarray(centres, np.float64).reshape(-1, 3), np.asarray(rad, np.float64).reshape(-1)
    w = centres - B.p
    inv_len2 = 1.0 / max(float(B.dseg @ B.dseg), 1e-30)
    sp = np.clip((w @ B.dseg) * inv_len2, 0.0, 1.0)
    q = w - B.dseg[None] * sp[:, None]
    reach = rad + B.delta
    rhs = reach * reach * 1.0002 + 1e-12
    margin = rhs - (q * q).sum(1)
    S = ((np.abs(w) + np.abs(B.dseg)[None] * sp[:, None]) ** 2).sum(1) + rhs
    return margin >= 0.0, margin > NEAR * S, -margin > NEAR * S
