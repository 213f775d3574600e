// rt_deform.h -- what the handles that deform a scene's geometry on the device share (rt_pose.cpp, rt_skin.cpp).  Host only.
//
// A deformer is a handle H with one device allocation, a table of rt_transform per apply and a kernel that makes the
// arrays of an rt_scene_delta from them; the apply itself is rt_scene_update_device's.  H has a member `RtDeformer m` and
//   int launch(const rt_transform* table_dev, hipStream_t stream);   its kernels; refuses with its own text
//   static int check_apply(const rt_scene*, const H*, const rt_transform*, const char* fn, rt_scene_delta*);
//   static int check_table(const rt_transform* table_host, uint32_t n, const char* fn);
// Every refusal that names the handle stays in H's file; the rest is here.
#pragma once

#include <cstring>

#include "rt_host.h"

static_assert(sizeof(rt_transform) == 32, "a transform is 8 floats");

struct RtDeformer {
  int device = 0;
  uint32_t n_xf = 0;                 // transforms of one apply
  DevBuf buf;                        // the handle's arrays, the staged transforms last
  rt_transform* xf_dev = nullptr;
  rt_transform* xf_stage = nullptr;  // pinned, [n_xf]
  RtPending done;                    // behind the last kernel enqueued for this handle
};

template <class H>
void rt_deform_free(H* h) {
  if (!h) return;
  (void)hipSetDevice(h->m.device);
  h->m.done.destroy();
  if (h->m.xf_stage) (void)hipHostFree(h->m.xf_stage);
  h->m.buf.release();
  delete h;
}

inline int rt_deform_wait(RtDeformer& m) {
  HIP_TRY(hipSetDevice(m.device));
  return m.done.wait();
}

// the first transform of a table with a non-finite member, -1: none
inline int64_t rt_deform_first_non_finite(const rt_transform* t, uint32_t n) {
  for (uint32_t p = 0; p < n; p++) {
    const float* q = (const float*)(t + p);
    for (int k = 0; k < 8; k++)
      if (!rt_finite(q[k])) return p;
  }
  return -1;
}

// the end of every check_apply: rt_scene_update_device's own refusals of the delta `d`, made before the kernel runs
inline int rt_deform_check_delta(const rt_scene* s, const rt_scene_delta& d, rt_scene_delta* delta) {
  if (s->progress_active) return fail(RT_ERR_INVALID_ARG, "a progressive render owns this scene until rt_render_end");
  const int rc = rt_check_scene_delta(s->dev, s->plan, &d, nullptr);
  if (rc != RT_OK) return rc;
  *delta = d;
  return RT_OK;
}

// the end of every create: the host image `img` (laid out by `lay`, every device pointer of the handle a slot of it)
// uploaded in one copy, the pinned stage, the event, and the slots bound to the device copy.  Frees the handle on failure.
template <class H>
int rt_deform_upload(H* h, const RtArena& lay, const std::vector<unsigned char>& img) {
  RtDeformer& m = h->m;
  const size_t xf_bytes = (size_t)m.n_xf * 32;
  int rc = m.buf.ensure(lay.total());
  if (rc == RT_OK) {
    const hipError_t e = hipMemcpy(m.buf.p, img.data(), lay.total(), hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = fail(RT_ERR_HIP, "hipMemcpy H2D failed: %s", hipGetErrorString(e));
  }
  if (rc == RT_OK && hipHostMalloc((void**)&m.xf_stage, xf_bytes, hipHostMallocDefault) != hipSuccess)
    m.xf_stage = nullptr, rc = fail(RT_ERR_OOM, "hipHostMalloc(%zu) failed", xf_bytes);
  if (rc == RT_OK && m.done.create() != RT_OK) m.done.ev = nullptr, rc = fail(RT_ERR_HIP, "hipEventCreate failed");
  if (rc != RT_OK) {
    rt_deform_free(h);
    return rc;
  }
  lay.bind(m.buf.p);
  return RT_OK;
}

template <class H>
int rt_deform_enqueue(H* h, const rt_transform* table_dev, hipStream_t stream) {
  const int rc = h->launch(table_dev, stream);
  return rc != RT_OK ? rc : h->m.done.mark(stream);
}

// rt_*_geometry_device behind its null checks
template <class H>
int rt_deform_geometry_device(H* h, const rt_transform* table_dev, void* hip_stream) {
  HIP_TRY(hipSetDevice(h->m.device));
  return rt_deform_enqueue(h, table_dev, (hipStream_t)hip_stream);
}

template <class H>
int rt_deform_apply_device(rt_scene* s, H* h, const rt_transform* table_dev, void* hip_stream, rt_update_info* info, const char* fn) {
  rt_scene_delta d;
  int rc = H::check_apply(s, h, table_dev, fn, &d);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(h->m.device));
  if ((rc = rt_deform_enqueue(h, table_dev, (hipStream_t)hip_stream)) != RT_OK) return rc;
  rc = rt_scene_update_device(s, &d, hip_stream, info);  // (blocks: the stream has drained)
  if (rc == RT_OK) h->m.done.clear();
  return rc;
}

template <class H>
int rt_deform_apply(rt_scene* s, H* h, const rt_transform* table_host, rt_update_info* info, const char* fn) {
  rt_scene_delta d;
  int rc = H::check_apply(s, h, table_host, fn, &d);
  if (rc == RT_OK) rc = H::check_table(table_host, h->m.n_xf, fn);
  if (rc != RT_OK) return rc;
  RtDeformer& m = h->m;
  if ((rc = rt_deform_wait(m)) != RT_OK) return rc;  // (a kernel still in flight reads the staged transforms)
  memcpy(m.xf_stage, table_host, (size_t)m.n_xf * 32);
  HIP_TRY(hipMemcpyAsync(m.xf_dev, m.xf_stage, (size_t)m.n_xf * 32, hipMemcpyHostToDevice, nullptr));
  if ((rc = rt_deform_enqueue(h, m.xf_dev, nullptr)) != RT_OK) return rc;
  rc = rt_scene_update_device(s, &d, nullptr, info);
  if (rc == RT_OK) m.done.clear();
  return rc;
}

// rt_*_read behind rt_deform_wait: the arrays the caller wants and the handle has
struct RtReadBack {
  float* host;
  const float* dev;
  size_t bytes;
};
template <size_t N>
int rt_deform_read(const RtReadBack (&arrays)[N]) {
  for (const RtReadBack& a : arrays)
    if (a.host && a.dev && a.bytes) HIP_TRY(hipMemcpy(a.host, a.dev, a.bytes, hipMemcpyDeviceToHost));
  return RT_OK;
}

// rt_*_model: outputs the caller does not want land in scratch arrays
template <size_t N>
void rt_deform_scratch(float* (&o)[N], const size_t (&floats)[N], std::vector<float> (&scratch)[N]) {
  for (size_t k = 0; k < N; k++)
    if (!o[k]) scratch[k].resize(floats[k] + 1), o[k] = scratch[k].data();
}
