// rt_skin.h -- the arithmetic of device-side skinned meshes (rt_skin*): an INDEXED mesh in rest pose, deformed by linear blend
// skinning.  The reference loads a mesh with tobj's single_index (src/scene/scene.rs:43-134): it transforms the unified
// vertices, rotates the per-vertex normals, and lerps the three normals per face afterwards.  A skin does the same in that
// order, with up to four bones per vertex in place of the one transform.
//
// Compiled twice, as rt_pose.h is: rt_skin_model (rt_skin.cpp) calls these functions in loops on the host, and the kernels
// of rt_skin.hip are the same functions with a thread index.  Every operation is ONE correctly rounded fp32 operation
// (rt_fmul / rt_fadd / rt_fdiv / rt_fsqrt of rt_refit.h), evaluated as written, left to right, never fused, except the two
// fused steps of the face normal named below; a - b is rt_fadd(a, -b).
//
// A bone is an rt_transform (8 floats, not normalised by the library): T(v) is rt_pose_point, rotate(n) is rt_pose_rotate.
//   vertex i:   influences (bone[i][k], weight[i][k]), k = 0..3, in that order; a weight of +0 or -0 is skipped;
//               the first influence kept sets   acc = w T_b(v)          (three multiplies)
//               every later one adds            acc = acc + w T_b(v)    (per component one multiply, one add)
//               normals: the same with rotate_b(n); no influence kept: the rest position and the rest normal.
//               Weights are not normalised: one influence of weight 1 gives T_b(v) exactly.
//   triangle t, indices (i0, i1, i2), skinned V, N:
//               v1 = V[i0];  e1 = V[i1] - V[i0];  e2 = V[i2] - V[i0]
//               vertex normals:  n = (N[i0] 0.5 + N[i1] 0.5) 0.5 + N[i2] 0.5        (n1.lerp(n2, 0.5).lerp(n3, 0.5) of f32math)
//               face normals:    c = e1 x e2, cx = e1y e2z + (-e1z) e2y, ...;  d = fma(cx, cx, fma(cy, cy, cz cz));
//                                r = 1 / sqrt(d);  n = c r                          (TriangleData.with_material of scene.py)
// Not part of the public ABI.
#pragma once

#include <string.h>

#include "rt_pose.h"

#define RT_SKIN_WG 256u
#define RT_SKIN_INFLUENCES 4

// the one fused operation of the specification: fmaf on the host, __fmaf_rn on the device
#if defined(__HIP_DEVICE_COMPILE__)
RT_HD static inline float rt_skin_fma(float a, float b, float c) { return __fmaf_rn(a, b, c); }
#else
static inline float rt_skin_fma(float a, float b, float c) { return fmaf(a, b, c); }
#endif

// the four bone indices and the four weights of a vertex: one 8-byte and one 16-byte load on the device, where the arrays
// start on 256 bytes; the host model reads the caller's arrays, which promise no alignment
struct alignas(8) RtSkinBones { uint16_t b[RT_SKIN_INFLUENCES]; };
struct alignas(16) RtSkinWeights { float w[RT_SKIN_INFLUENCES]; };

// the arrays of a skin, rest and skinned.  The posed triangle arrays are the triangle group of an rt_scene_delta.
struct RtSkinArrays {
  uint32_t n_vertices, n_tris;
  const float *position, *normal;    // rest, [n_vertices][3]; normal null: face normals from the skinned edges
  const uint16_t* bone;              // [n_vertices][4]
  const float* weight;               // [n_vertices][4]
  const uint32_t* indices;           // [n_tris][3]
  float *V, *N;                      // skinned, [n_vertices][3]; N null with normal
  float *o_v1, *o_e1, *o_e2, *o_normal;  // posed, [n_tris][3]
};

// vertex i under `bones` (null: the rest pose, restated)
RT_HD static inline void rt_skin_vertex(const RtSkinArrays& a, uint32_t i, const float* bones) {
  const size_t s = 3 * (size_t)i;
  const bool has_n = a.normal != nullptr;
  const float p[3] = {a.position[s], a.position[s + 1], a.position[s + 2]};
  float n[3] = {0.f, 0.f, 0.f};
  if (has_n) n[0] = a.normal[s], n[1] = a.normal[s + 1], n[2] = a.normal[s + 2];
  float vp[3] = {p[0], p[1], p[2]}, vn[3] = {n[0], n[1], n[2]};
  if (bones) {
    RtSkinBones bi;
    RtSkinWeights wt;
#if defined(__HIP_DEVICE_COMPILE__)
    bi = ((const RtSkinBones*)a.bone)[i], wt = ((const RtSkinWeights*)a.weight)[i];
#else
    memcpy(&bi, a.bone + RT_SKIN_INFLUENCES * (size_t)i, sizeof bi), memcpy(&wt, a.weight + RT_SKIN_INFLUENCES * (size_t)i, sizeof wt);
#endif
    bool kept = false;
#pragma unroll
    for (int k = 0; k < RT_SKIN_INFLUENCES; k++) {
      const float w = wt.w[k];
      if (w == 0.0f) continue;  // (+0 and -0; create refuses a non-finite weight)
      const float* q = bones + 8 * (size_t)bi.b[k];
      float t[3];
      rt_pose_point(q, p, t);
      for (int c = 0; c < 3; c++) vp[c] = kept ? rt_fadd(vp[c], rt_fmul(w, t[c])) : rt_fmul(w, t[c]);
      if (has_n) {
        rt_pose_rotate(q, n, t);
        for (int c = 0; c < 3; c++) vn[c] = kept ? rt_fadd(vn[c], rt_fmul(w, t[c])) : rt_fmul(w, t[c]);
      }
      kept = true;
    }
  }
  a.V[s] = vp[0], a.V[s + 1] = vp[1], a.V[s + 2] = vp[2];
  if (has_n) a.N[s] = vn[0], a.N[s + 1] = vn[1], a.N[s + 2] = vn[2];
}

// v1, e1, e2 of triangle t from the skinned vertices; the edges come back for the face normal
RT_HD static inline void rt_skin_edges(const RtSkinArrays& a, uint32_t t, const uint32_t i[3], float e1[3], float e2[3]) {
  const size_t s = 3 * (size_t)t, s0 = 3 * (size_t)i[0], s1 = 3 * (size_t)i[1], s2 = 3 * (size_t)i[2];
  for (int c = 0; c < 3; c++) {
    const float v1 = a.V[s0 + c];
    e1[c] = rt_fadd(a.V[s1 + c], -v1), e2[c] = rt_fadd(a.V[s2 + c], -v1);
    a.o_v1[s + c] = v1, a.o_e1[s + c] = e1[c], a.o_e2[s + c] = e2[c];
  }
}

// triangle t of a mesh with vertex normals: n = (N[i0] 0.5 + N[i1] 0.5) 0.5 + N[i2] 0.5
RT_HD static inline void rt_skin_tri(const RtSkinArrays& a, uint32_t t) {
  const size_t s = 3 * (size_t)t;
  const uint32_t i[3] = {a.indices[s], a.indices[s + 1], a.indices[s + 2]};
  float e1[3], e2[3];
  rt_skin_edges(a, t, i, e1, e2);
  for (int c = 0; c < 3; c++) {
    const float n01 = rt_fadd(rt_fmul(a.N[3 * (size_t)i[0] + c], 0.5f), rt_fmul(a.N[3 * (size_t)i[1] + c], 0.5f));
    a.o_normal[s + c] = rt_fadd(rt_fmul(n01, 0.5f), rt_fmul(a.N[3 * (size_t)i[2] + c], 0.5f));
  }
}

// triangle t of a mesh without vertex normals: the normalised cross product of the skinned edges
RT_HD static inline void rt_skin_face(const RtSkinArrays& a, uint32_t t) {
  const size_t s = 3 * (size_t)t;
  const uint32_t i[3] = {a.indices[s], a.indices[s + 1], a.indices[s + 2]};
  float e1[3], e2[3];
  rt_skin_edges(a, t, i, e1, e2);
  const float cx = rt_fadd(rt_fmul(e1[1], e2[2]), rt_fmul(-e1[2], e2[1]));
  const float cy = rt_fadd(rt_fmul(e1[2], e2[0]), rt_fmul(-e1[0], e2[2]));
  const float cz = rt_fadd(rt_fmul(e1[0], e2[1]), rt_fmul(-e1[1], e2[0]));
  const float d = rt_skin_fma(cx, cx, rt_skin_fma(cy, cy, rt_fmul(cz, cz)));
  const float r = rt_fdiv(1.0f, rt_fsqrt(d));
  a.o_normal[s] = rt_fmul(cx, r), a.o_normal[s + 1] = rt_fmul(cy, r), a.o_normal[s + 2] = rt_fmul(cz, r);
}

// rt_skin.hip: enqueues the vertex kernel, then the triangle kernel of the mesh's normal mode; returns hipError_t as int
int rt_launch_skin(const RtSkinArrays& a, const rt_transform* bones_dev, void* stream);
