// rt_pose.h -- the arithmetic of device-side part poses (rt_pose*): a rigid part of a scene placed by a similarity
// transform, as Scene::from_obj(path, Some(Similarity3)) places a mesh (reference src/scene/scene.rs:43-134: transform_vec
// on the vertices, rotated_by(rotation) on the normals).
//
// Compiled twice, as rt_refit.h and rt_view.h are: rt_pose_model (rt_pose.cpp) calls these functions in loops on the host,
// and rt_pose_kernel (rt_pose.hip) is the same functions with a thread index.  Every operation is ONE correctly rounded
// fp32 operation (rt_fmul / rt_fadd / rt_fdiv of rt_refit.h), evaluated as written, left to right, never fused;
// a - b is rt_fadd(a, -b).
//
// A transform is 8 floats {translation[3], s, xy, xz, yz, scale}: the rotor in the layout of ultraviolet's Rotor3, which
// the library does not normalise.
//   rotate(v):  fx = (s vx + xy vy) + xz vz      fy = (s vy - xy vx) + yz vz
//               fz = (s vz - xz vx) - yz vy      fw = (xy vz - xz vy) + yz vx
//               x' = ((s fx + xy fy) + xz fz) + yz fw
//               y' = ((s fy - xy fx) - xz fw) + yz fz
//               z' = ((s fz + xy fw) - xz fx) - yz fy
//   T(v)     =  rotate(v) scale + translation        (per component: one multiply, one add)
//   triangle:   v1' = T(v1), v2' = T(v2), v3' = T(v3);  e1' = v2' - v1';  e2' = v3' - v1';  n' = rotate(n)
//   sphere:     c' = T(c);  r' = r scale;  r_sq' = r' r';  r_inv' = 1 / r'
// These are Rotor3.rotate_vec and Similarity3.transform_vec of f32math.py, term for term.
//
// The rest pose holds the VERTICES v2, v3, not the edges: only then is a posed mesh the mesh from_obj would have loaded
// (v1, e1, e2 bit for bit).  Deviation on normals: the reference rotates the per-vertex normals and lerps them afterwards,
// here the stored (lerped) normal is rotated; measured between the two Python formulas on semesterbild's text mesh the
// stored normals differ by at most 1.79e-7 = 3 * 2^-24 per component.
// Not part of the public ABI.
#pragma once

#include "rt_refit.h"

#define RT_POSE_WG 256u
#define RT_POSE_NONE 0xFFFFFFFFu  // part_of entry of an object that belongs to no part

// q: the 8 floats of an rt_transform
RT_HD static inline void rt_pose_rotate(const float* q, const float v[3], float out[3]) {
  const float s = q[3], xy = q[4], xz = q[5], yz = q[6];
  const float fx = rt_fadd(rt_fadd(rt_fmul(s, v[0]), rt_fmul(xy, v[1])), rt_fmul(xz, v[2]));
  const float fy = rt_fadd(rt_fadd(rt_fmul(s, v[1]), -rt_fmul(xy, v[0])), rt_fmul(yz, v[2]));
  const float fz = rt_fadd(rt_fadd(rt_fmul(s, v[2]), -rt_fmul(xz, v[0])), -rt_fmul(yz, v[1]));
  const float fw = rt_fadd(rt_fadd(rt_fmul(xy, v[2]), -rt_fmul(xz, v[1])), rt_fmul(yz, v[0]));
  out[0] = rt_fadd(rt_fadd(rt_fadd(rt_fmul(s, fx), rt_fmul(xy, fy)), rt_fmul(xz, fz)), rt_fmul(yz, fw));
  out[1] = rt_fadd(rt_fadd(rt_fadd(rt_fmul(s, fy), -rt_fmul(xy, fx)), -rt_fmul(xz, fw)), rt_fmul(yz, fz));
  out[2] = rt_fadd(rt_fadd(rt_fadd(rt_fmul(s, fz), rt_fmul(xy, fw)), -rt_fmul(xz, fx)), -rt_fmul(yz, fy));
}

RT_HD static inline void rt_pose_point(const float* q, const float v[3], float out[3]) {
  float r[3];
  rt_pose_rotate(q, v, r);
  for (int a = 0; a < 3; a++) out[a] = rt_fadd(rt_fmul(r[a], q[7]), q[a]);
}

// the arrays of a pose, rest and posed.  Triangle arrays cover the pose's triangle range [lo, lo + n_cover) and are
// indexed from its start; sphere arrays cover all spheres.  The posed arrays are the groups of an rt_scene_delta.
struct RtPoseArrays {
  uint32_t lo, n_cover, n_spheres;
  const uint32_t *tri_part, *sphere_part;          // part of each object, RT_POSE_NONE for none
  const float *v1, *v2, *v3, *normal;              // rest, [n_cover][3]
  const float *centre, *radius;                    // rest, [n_spheres][3] / [n_spheres]
  float *o_v1, *o_e1, *o_e2, *o_normal;            // posed, [n_cover][3]
  float *o_centre, *o_r_sq, *o_r_inv;              // posed, [n_spheres][3] / [n_spheres]
};

// triangle k of the covering range under transform q (null: the rest pose, restated as v1, v2 - v1, v3 - v1, normal)
RT_HD static inline void rt_pose_tri(const RtPoseArrays& p, uint32_t k, const float* q) {
  const size_t s = 3 * (size_t)k;
  float v1[3] = {p.v1[s], p.v1[s + 1], p.v1[s + 2]}, v2[3] = {p.v2[s], p.v2[s + 1], p.v2[s + 2]};
  float v3[3] = {p.v3[s], p.v3[s + 1], p.v3[s + 2]}, n[3] = {p.normal[s], p.normal[s + 1], p.normal[s + 2]};
  if (q) {
    float t1[3], t2[3], t3[3], tn[3];
    rt_pose_point(q, v1, t1), rt_pose_point(q, v2, t2), rt_pose_point(q, v3, t3), rt_pose_rotate(q, n, tn);
    for (int a = 0; a < 3; a++) v1[a] = t1[a], v2[a] = t2[a], v3[a] = t3[a], n[a] = tn[a];
  }
  for (int a = 0; a < 3; a++) {
    p.o_v1[s + a] = v1[a];
    p.o_e1[s + a] = rt_fadd(v2[a], -v1[a]);
    p.o_e2[s + a] = rt_fadd(v3[a], -v1[a]);
    p.o_normal[s + a] = n[a];
  }
}

// sphere i under transform q (null: the rest pose, restated as centre, r r, 1 / r)
RT_HD static inline void rt_pose_sphere(const RtPoseArrays& p, uint32_t i, const float* q) {
  const size_t s = 3 * (size_t)i;
  float c[3] = {p.centre[s], p.centre[s + 1], p.centre[s + 2]}, r = p.radius[i];
  if (q) {
    float t[3];
    rt_pose_point(q, c, t);
    for (int a = 0; a < 3; a++) c[a] = t[a];
    r = rt_fmul(r, q[7]);
  }
  p.o_centre[s] = c[0], p.o_centre[s + 1] = c[1], p.o_centre[s + 2] = c[2];
  p.o_r_sq[i] = rt_fmul(r, r);
  p.o_r_inv[i] = rt_fdiv(1.0f, r);
}

// rt_pose.hip: enqueues rt_pose_kernel over the covering range and the spheres; returns hipError_t as int
int rt_launch_pose(const RtPoseArrays& p, const rt_transform* transforms_dev, void* stream);
