// rt_view.cpp -- the host side of device-side camera views (rt_view*, rt_render_view*): validation (before any HIP call),
// the handle and its one device allocation, the launch sequence generator -> order -> trace -> resolve, the host forms'
// staging, and the host models of the two formulas (the functions of rt_view.h in loops).
//
// A view is built ON TOP of the radiance queries: it makes a ray batch and hands it to rt_ray_order_build_device and
// rt_trace_rays[_ordered]_device through their public entry points, so every blocking, validation and scene-state rule of a
// frame is the trace's.
//
// Also the host side of adaptive frames (rt_view_enable_adaptive, rt_render_view_adaptive*): the second allocation and the
// sequence pass 1 -> classify -> sparse generator -> partition -> pass 2 -> adaptive resolve.  Their arithmetic is in
// rt_view_adapt.h, their kernels in rt_view_adapt.hip, their host models in rt_view_adapt.cpp.
//
// And of thin-lens views (rt_view_create_lens, rt_view_set_lens): the lens table and the coc plane in the view's allocation,
// the choice of the generator (A > 0: the lens generators of rt_view_lens.hip) and the two defocus launches behind the
// classify.  Their arithmetic is in rt_view_lens.h, their checks and host models in rt_view_lens.cpp.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>

#include "rt_host.h"
#include "rt_view_lens.h"

struct rt_view {
  int device = 0;
  uint32_t width = 0, height = 0, n_pixels = 0, n_samples = 0, n_distinct = 0, n_rays = 0, order_mode = RT_VIEW_ORDER_ONCE;
  float distinct[2 * RT_VIEW_MAX_SAMPLES] = {};
  uint8_t plane_of[RT_VIEW_MAX_SAMPLES] = {};
  rt_view_desc desc{};  // (samples: not kept)
  bool has_camera = false;
  RtViewCam cam{};
  // one allocation: origin, direction, the per-ray rgb / valid / id / t planes, the two sample tables
  DevBuf buf;
  float *origin = nullptr, *direction = nullptr, *rgb = nullptr, *t = nullptr, *distinct_dev = nullptr;
  uint8_t *valid = nullptr, *plane_of_dev = nullptr;
  int32_t* id = nullptr;
  rt_ray_order* order = nullptr;  // capacity n_rays; none with RT_VIEW_ORDER_NONE
  bool order_built = false;
  RtPending done;                // behind the last work enqueued for this view
  hipEvent_t ev[5] = {};         // host form: before / after the generator, after the order, before / after the resolve
  double rays_ms = 0.0, order_ms = 0.0, resolve_ms = 0.0;
  // adaptive frames (rt_view_enable_adaptive): one more allocation, the plane-0 order's state, the stage events and times
  bool adaptive = false;
  DevBuf abuf;
  RtViewAdaptWs aws{};
  bool order0_built = false;     // aws.order0 is the plane-0 part of the order the view holds now
  hipEvent_t aev[6] = {};        // host form: begin, after pass 1, the classify, the partition, pass 2, the resolve
  uint32_t n_refined = 0;
  bool n_refined_read = true;    // n_refined holds the word of the last adaptive frame
  double astage_ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  // a thin lens (rt_view_create_lens): `distinct` holds the pixel offset of every 4-tuple plane, lens_tab its lens offset;
  // both tables and the coc plane (4 bytes per pixel) are parts of `buf`
  bool lens = false;
  float lens_tab[2 * RT_VIEW_MAX_SAMPLES] = {};
  float *lens_dev = nullptr, *coc = nullptr;
  float aperture = 0.0f, focus_distance = 1.0f, coc_tol = INFINITY;  // (rt_view_set_lens; A == 0: the pinhole generator)
  uint32_t spread = 0;
};

int rt_view_check_desc(const rt_view_desc* d, const char* fn) {
  if (!d) return fail(RT_ERR_INVALID_ARG, "%s: null view description", fn);
  if (d->abi_version != RT_ABI_VERSION) return fail(RT_ERR_INVALID_ARG, "%s: rt_view_desc.abi_version %u != %u", fn, d->abi_version, RT_ABI_VERSION);
  if (d->width == 0 || d->height == 0) return fail(RT_ERR_INVALID_ARG, "%s: empty frame (%u x %u)", fn, d->width, d->height);
  if (d->n_samples == 0 || d->n_samples > RT_VIEW_MAX_SAMPLES)
    return fail(RT_ERR_INVALID_ARG, "%s: n_samples %u outside 1 .. %u", fn, d->n_samples, RT_VIEW_MAX_SAMPLES);
  if (!d->samples) return fail(RT_ERR_INVALID_ARG, "%s: null sample table", fn);
  if (d->order > RT_VIEW_ORDER_NONE) return fail(RT_ERR_INVALID_ARG, "%s: unknown order mode %u", fn, d->order);
  for (uint32_t k = 0; k < 2u * d->n_samples; k++)
    if (!rt_finite(d->samples[k])) return fail(RT_ERR_INVALID_ARG, "%s: sample %u has a non-finite offset", fn, k / 2u);
  float distinct[2 * RT_VIEW_MAX_SAMPLES];
  uint8_t plane_of[RT_VIEW_MAX_SAMPLES];
  const uint64_t n_rays = (uint64_t)rt_view_dedup(d->samples, d->n_samples, distinct, plane_of) * d->width * d->height;
  if ((uint64_t)d->width * d->height > ((uint64_t)1 << 27) || n_rays > ((uint64_t)1 << 27))
    return fail(RT_ERR_INVALID_ARG, "%s: %u x %u pixels of distinct samples exceed the 2^27 rays a ray order sorts", fn, d->width, d->height);
  return RT_OK;
}

int rt_view_check_camera(const rt_view_camera* c, const char* fn) {
  if (!c) return fail(RT_ERR_INVALID_ARG, "%s: null camera", fn);
  if (c->abi_version != RT_ABI_VERSION) return fail(RT_ERR_INVALID_ARG, "%s: rt_view_camera.abi_version %u != %u", fn, c->abi_version, RT_ABI_VERSION);
  if (c->kind != RT_VIEW_PINHOLE && c->kind != RT_VIEW_REFERENCE) return fail(RT_ERR_INVALID_ARG, "%s: unknown camera kind %u", fn, c->kind);
  bool finite = rt_finite(c->tan_half_fov_y) && rt_finite(c->fw) && rt_finite(c->fh);
  for (int k = 0; k < 3; k++)
    finite = finite && rt_finite(c->eye[k]) && rt_finite(c->right[k]) && rt_finite(c->up[k]) && rt_finite(c->forward[k]) && rt_finite(c->focus[k]);
  if (!finite) return fail(RT_ERR_INVALID_ARG, "%s: a camera member is not finite", fn);
  if (c->kind == RT_VIEW_PINHOLE && !(c->tan_half_fov_y > 0.0f))
    return fail(RT_ERR_INVALID_ARG, "%s: tan_half_fov_y %g must be positive", fn, (double)c->tan_half_fov_y);
  return RT_OK;
}

RtViewCam rt_view_cam_of(const rt_view_desc& d, const rt_view_camera& c) {
  RtViewCam m{};
  m.kind = c.kind, m.width = d.width, m.height = d.height, m.n_pixels = d.width * d.height;
  for (int k = 0; k < 3; k++) m.eye[k] = c.eye[k], m.right[k] = c.right[k], m.up[k] = c.up[k], m.forward[k] = c.forward[k], m.focus[k] = c.focus[k];
  m.tan_half = c.tan_half_fov_y, m.fw = c.fw, m.fh = c.fh;
  return m;
}

namespace {

int view_alloc(rt_view* v) {
  const size_t n = v->n_rays;
  RtArena lay;
  lay.add(n * 12, &v->origin), lay.add(n * 12, &v->direction), lay.add(n * 12, &v->rgb);
  lay.add(n * 4, &v->id), lay.add(n * 4, &v->t), lay.add(n, &v->valid);
  lay.add(sizeof(v->distinct), &v->distinct_dev), lay.add(sizeof(v->plane_of), &v->plane_of_dev);
  if (v->lens) lay.add(sizeof(v->lens_tab), &v->lens_dev), lay.add((size_t)v->n_pixels * 4, &v->coc);
  int rc = v->buf.ensure(lay.total());
  if (rc != RT_OK) return rc;
  lay.bind(v->buf.p);
  HIP_TRY(hipMemcpy(v->distinct_dev, v->distinct, sizeof(v->distinct), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(v->plane_of_dev, v->plane_of, sizeof(v->plane_of), hipMemcpyHostToDevice));
  if (v->lens) HIP_TRY(hipMemcpy(v->lens_dev, v->lens_tab, sizeof(v->lens_tab), hipMemcpyHostToDevice));
  if ((rc = v->done.create()) != RT_OK) return rc;
  for (hipEvent_t& e : v->ev) HIP_TRY(hipEventCreate(&e));
  if (v->order_mode != RT_VIEW_ORDER_NONE) {
    rt_ray_order_desc od{};
    od.abi_version = RT_ABI_VERSION, od.capacity = v->n_rays;
    if ((rc = rt_ray_order_create(&od, v->device, &v->order)) != RT_OK) return rc;
  }
  return RT_OK;
}

void view_free(rt_view* v) {
  if (!v) return;
  (void)hipSetDevice(v->device);
  v->done.destroy();
  rt_ray_order_destroy(v->order);
  for (hipEvent_t e : v->ev)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : v->aev)
    if (e) (void)hipEventDestroy(e);
  v->abuf.release();
  v->buf.release();
  delete v;
}

// is the lens on?  (a lens view with A > 0: the lens generators; else the pinhole generator on the planes' pixel offsets)
bool lens_on(const rt_view* v) { return v->lens && v->aperture > 0.0f; }

// what every call that makes rays refuses for a lens view, before any HIP call
int check_lens_camera(const rt_view* v, const char* fn) {
  if (lens_on(v) && v->cam.kind != RT_VIEW_PINHOLE)
    return fail(RT_ERR_INVALID_ARG, "%s: an RT_VIEW_REFERENCE camera has no lens (aperture %g)", fn, (double)v->aperture);
  return RT_OK;
}

// the generator for the first n_planes planes of the view
int rays_enqueue(rt_view* v, uint32_t n_planes, float* origin, float* direction, hipStream_t stream) {
  const hipError_t e = (hipError_t)(lens_on(v) ? rt_launch_view_lens_rays(v->cam, v->distinct_dev, v->lens_dev, n_planes, v->aperture,
                                                                          v->focus_distance, origin, direction, stream)
                                               : rt_launch_view_rays(v->cam, v->distinct_dev, n_planes, origin, direction, stream));
  if (e != hipSuccess) return fail(RT_ERR_HIP, "view ray generator launch failed: %s", hipGetErrorString(e));
  return RT_OK;
}

// everything a render refuses, before any HIP call; the scene and the view are looked at last
int check_render(const rt_scene* s, const rt_view* v, const rt_params* p, const rt_ray_radiance* out, const char* fn) {
  if (!s) return fail(RT_ERR_INVALID_ARG, "%s: null scene", fn);
  if (!v) return fail(RT_ERR_INVALID_ARG, "%s: null view", fn);
  if (!p) return fail(RT_ERR_INVALID_ARG, "%s: null shading parameters", fn);
  if (!out) return fail(RT_ERR_INVALID_ARG, "%s: null output struct", fn);
  // the trace's own checks of `shading` (a batch of one ray stands in: they do not depend on the batch)
  static const float one_ray[3] = {0.f, 0.f, 0.f};
  rt_ray_batch b{};
  b.abi_version = RT_ABI_VERSION, b.n_rays = 1, b.origin = one_ray, b.direction = one_ray;
  const int rc = rt_trace_rays_check(s, p, &b, out, fn);
  if (rc != RT_OK) return rc;
  if (!v->has_camera) return fail(RT_ERR_INVALID_ARG, "%s: the view has no camera yet (rt_view_set_camera)", fn);
  // (the trace refuses this too, but behind the generator's launch: a refusal comes before any HIP call)
  if (s->progress_active) return fail(RT_ERR_INVALID_ARG, "%s: a progressive render owns this scene until rt_render_end", fn);
  if (v->device != s->device) return fail(RT_ERR_INVALID_ARG, "%s: the view lives on device %d, the scene on device %d", fn, v->device, s->device);
  return check_lens_camera(v, fn);
}

// generator -> order -> trace -> resolve on `stream`; `out`: DEVICE pixel planes.  timed: record the view's stage events.
int render_enqueue(rt_scene* s, rt_view* v, const rt_params* p, const rt_ray_radiance* out, hipStream_t stream, bool timed) {
  int rc;
  if (timed) HIP_TRY(hipEventRecord(v->ev[0], stream));
  if ((rc = rays_enqueue(v, v->n_distinct, v->origin, v->direction, stream)) != RT_OK) return rc;
  if (timed) HIP_TRY(hipEventRecord(v->ev[1], stream));
  rt_ray_batch b{};
  b.abi_version = RT_ABI_VERSION, b.n_rays = v->n_rays, b.origin = v->origin, b.direction = v->direction;
  const bool build = v->order && (v->order_mode == RT_VIEW_ORDER_ALWAYS || !v->order_built);
  if (build) {
    if ((rc = rt_ray_order_build_device(v->order, &b, stream)) != RT_OK) return rc;
    v->order_built = true, v->order0_built = false;
  }
  if (timed) HIP_TRY(hipEventRecord(v->ev[2], stream));
  rt_ray_radiance rays{};
  rays.rgb = v->rgb, rays.valid = v->valid, rays.id = v->id, rays.t = v->t;
  rc = v->order ? rt_trace_rays_ordered_device(s, p, &b, v->order, &rays, stream) : rt_trace_rays_device(s, p, &b, &rays, stream);
  if (rc != RT_OK) return rc;
  if (timed) HIP_TRY(hipEventRecord(v->ev[3], stream));
  const hipError_t e = (hipError_t)rt_launch_view_resolve(v->n_pixels, v->n_samples, v->plane_of_dev, v->rgb, v->valid, v->id, v->t, *out, stream);
  if (e != hipSuccess) return fail(RT_ERR_HIP, "view resolve launch failed: %s", hipGetErrorString(e));
  if (timed) HIP_TRY(hipEventRecord(v->ev[4], stream));
  if (timed) v->order_ms = build ? -1.0 : 0.0;  // (-1: read from the events once the stream has drained)
  return v->done.mark(stream);
}

// ---- adaptive frames ------------------------------------------------------------------------------------------------------------
#define ADAPT_TRY(what, expr)                                                                     \
  do {                                                                                            \
    const hipError_t e_ = (hipError_t)(expr);                                                     \
    if (e_ != hipSuccess) return fail(RT_ERR_HIP, what " launch failed: %s", hipGetErrorString(e_)); \
  } while (0)

int check_render_adaptive(const rt_scene* s, const rt_view* v, const rt_params* p, const rt_view_refine* rf, const rt_ray_radiance* out, const char* fn) {
  if (!s) return fail(RT_ERR_INVALID_ARG, "%s: null scene", fn);
  if (!v) return fail(RT_ERR_INVALID_ARG, "%s: null view", fn);
  int rc = rt_view_check_refine(rf, fn);
  if (rc != RT_OK) return rc;
  if ((rc = check_render(s, v, p, out, fn)) != RT_OK) return rc;
  if (!v->adaptive) return fail(RT_ERR_INVALID_ARG, "%s: the view has no adaptive workspace (rt_view_enable_adaptive)", fn);
  return RT_OK;
}

// pass 1 -> classify -> sparse generator -> partition -> pass 2 -> adaptive resolve on `stream`; `out`, mask_out: DEVICE.
// timed: record the stage events.  pass1_stats (host form): the stream is drained behind pass 1 and its counters are read,
// because pass 2 may take the same frame slot of the scene.
int adaptive_enqueue(rt_scene* s, rt_view* v, const rt_params* p, const rt_view_refine* rf, const rt_ray_radiance* out, uint8_t* mask_out,
                     hipStream_t stream, bool timed, rt_stats* pass1_stats, const char* fn) {
  int rc;
  const RtViewAdaptWs& w = v->aws;
  const bool planes = v->n_distinct > 1u;
  if (timed) HIP_TRY(hipEventRecord(v->aev[0], stream));
  // the order: built from one complete run of the full generator (which makes plane 0 as well); its plane-0 part when it changed
  const bool build = v->order && (v->order_mode == RT_VIEW_ORDER_ALWAYS || !v->order_built);
  if (build) {
    if ((rc = rays_enqueue(v, v->n_distinct, v->origin, v->direction, stream)) != RT_OK) return rc;
    rt_ray_batch all{};
    all.abi_version = RT_ABI_VERSION, all.n_rays = v->n_rays, all.origin = v->origin, all.direction = v->direction;
    if ((rc = rt_ray_order_build_device(v->order, &all, stream)) != RT_OK) return rc;
    v->order_built = true, v->order0_built = false;
  } else if ((rc = rays_enqueue(v, 1u, v->origin, v->direction, stream)) != RT_OK) {
    return rc;
  }
  const uint32_t* order = v->order ? rt_ray_order_perm(v->order) : nullptr;
  if (order && planes && !v->order0_built) {
    ADAPT_TRY("view flags", rt_launch_view_flags(order, v->n_rays, v->n_pixels, nullptr, w.flags, stream));
    ADAPT_TRY("partition", rt_launch_partition(order, w.flags, v->n_rays, v->n_pixels, w.counts, w.sums, w.order0, stream));
    v->order0_built = true;
  }
  // pass 1: plane 0 = the first n_pixels rays of the layout, into the base planes
  rt_ray_batch b0{};
  b0.abi_version = RT_ABI_VERSION, b0.n_rays = v->n_pixels, b0.origin = v->origin, b0.direction = v->direction;
  rt_ray_radiance base{};
  base.rgb = w.rgb0, base.valid = w.valid0, base.id = w.id0, base.t = w.t0;
  if ((rc = rt_trace_rays_perm_device(s, p, &b0, order ? (planes ? w.order0 : order) : nullptr, &base, stream, fn)) != RT_OK) return rc;
  if (pass1_stats) {
    HIP_TRY(hipStreamSynchronize(stream));
    if ((rc = rt_render_collect_stats(s, pass1_stats)) != RT_OK) return rc;
  }
  if (timed) HIP_TRY(hipEventRecord(v->aev[1], stream));
  HIP_TRY(hipMemsetAsync(w.n_refined, 0, 4, stream));
  ADAPT_TRY("view classify", rt_launch_view_classify(v->width, v->height, rf->criteria, rf->colour_tol, rf->depth_tol, w, mask_out, stream));
  v->n_refined_read = false;
  if (v->lens && rt_view_defocus_active(v->aperture, v->coc_tol)) {
    // the defocus criterion: the out-of-focus pixels of plane 0, and the pixels their blur reaches, join the mask
    ADAPT_TRY("view coc", rt_launch_view_coc(v->cam, v->distinct_dev, v->aperture, v->focus_distance, w.valid0, w.t0, v->coc, stream));
    ADAPT_TRY("view defocus spread", rt_launch_view_defocus_spread(v->width, v->height, v->spread, v->coc_tol, v->coc, w.mask, mask_out, w.n_refined, stream));
  }
  if (timed) HIP_TRY(hipEventRecord(v->aev[2], stream));
  if (planes) {
    if (lens_on(v))
      ADAPT_TRY("sparse lens ray generator", rt_launch_view_lens_sparse_rays(v->cam, v->distinct_dev, v->lens_dev, v->n_distinct, v->aperture,
                                                                             v->focus_distance, w.mask, v->origin, v->direction, stream));
    else
      ADAPT_TRY("sparse view ray generator", rt_launch_view_sparse_rays(v->cam, v->distinct_dev, v->n_distinct, w.mask, v->origin, v->direction, stream));
    ADAPT_TRY("view flags", rt_launch_view_flags(order, v->n_rays, v->n_pixels, w.mask, w.flags, stream));
    ADAPT_TRY("partition", rt_launch_partition(order, w.flags, v->n_rays, v->n_rays, w.counts, w.sums, w.perm2, stream));
  }
  if (timed) HIP_TRY(hipEventRecord(v->aev[3], stream));
  if (planes) {
    rt_ray_batch b{};
    b.abi_version = RT_ABI_VERSION, b.n_rays = v->n_rays, b.origin = v->origin, b.direction = v->direction;
    rt_ray_radiance rays{};
    rays.rgb = v->rgb, rays.valid = v->valid;  // (id and t are plane 0's)
    if ((rc = rt_trace_rays_perm_device(s, p, &b, w.perm2, &rays, stream, fn)) != RT_OK) return rc;
  }
  if (timed) HIP_TRY(hipEventRecord(v->aev[4], stream));
  ADAPT_TRY("adaptive view resolve", rt_launch_view_resolve_adaptive(v->n_pixels, v->n_samples, v->plane_of_dev, w, v->rgb, v->valid, *out, stream));
  if (timed) HIP_TRY(hipEventRecord(v->aev[5], stream));
  return v->done.mark(stream);
}
#undef ADAPT_TRY

}  // namespace

extern "C" {

// rt_view_create (lens_samples == nullptr) and rt_view_create_lens
static int view_create(const rt_view_desc* d, const float* lens_samples, bool lens, int device, rt_view** out, const char* fn) {
  if (!d || !out) return fail(RT_ERR_INVALID_ARG, "%s: null argument", fn);
  *out = nullptr;
  int rc = lens ? rt_view_lens_check_desc(d, lens_samples, fn) : rt_view_check_desc(d, fn);
  if (rc != RT_OK) return rc;
  if ((rc = rt_open_device(device)) != RT_OK) return rc;
  rt_view* v = new rt_view();
  v->device = device, v->width = d->width, v->height = d->height, v->n_pixels = d->width * d->height, v->n_samples = d->n_samples;
  v->order_mode = d->order, v->lens = lens;
  v->desc = *d, v->desc.samples = nullptr;
  v->n_distinct = lens ? rt_view_lens_dedup(d->samples, lens_samples, d->n_samples, v->distinct, v->lens_tab, v->plane_of)
                       : rt_view_dedup(d->samples, d->n_samples, v->distinct, v->plane_of);
  v->n_rays = v->n_distinct * v->n_pixels;
  if ((rc = view_alloc(v)) != RT_OK) {
    view_free(v);
    return rc;
  }
  *out = v;
  return RT_OK;
}

int rt_view_create(const rt_view_desc* d, int device, rt_view** out) { return view_create(d, nullptr, false, device, out, "rt_view_create"); }

int rt_view_create_lens(const rt_view_desc* d, const float* lens_samples, int device, rt_view** out) {
  return view_create(d, lens_samples, true, device, out, "rt_view_create_lens");
}

int rt_view_set_lens(rt_view* v, const rt_view_lens* l) {
  if (!v) return fail(RT_ERR_INVALID_ARG, "rt_view_set_lens: null view");
  const int rc = rt_view_check_lens(l, "rt_view_set_lens");
  if (rc != RT_OK) return rc;
  if (!v->lens) return fail(RT_ERR_INVALID_ARG, "rt_view_set_lens: the view has no lens table (rt_view_create_lens)");
  v->aperture = l->aperture, v->focus_distance = l->focus_distance, v->coc_tol = l->coc_tol, v->spread = l->spread;
  return RT_OK;
}

void rt_view_destroy(rt_view* v) { view_free(v); }

int rt_view_set_camera(rt_view* v, const rt_view_camera* c) {
  if (!v) return fail(RT_ERR_INVALID_ARG, "rt_view_set_camera: null view");
  const int rc = rt_view_check_camera(c, "rt_view_set_camera");
  if (rc != RT_OK) return rc;
  v->cam = rt_view_cam_of(v->desc, *c), v->has_camera = true;
  return RT_OK;
}

int rt_view_rays_device(rt_view* v, float* origin, float* direction, void* hip_stream) {
  const char* fn = "rt_view_rays_device";
  if (!v) return fail(RT_ERR_INVALID_ARG, "%s: null view", fn);
  if (!origin || !direction) return fail(RT_ERR_INVALID_ARG, "%s: origin / direction missing", fn);
  if (!v->has_camera) return fail(RT_ERR_INVALID_ARG, "%s: the view has no camera yet (rt_view_set_camera)", fn);
  int rc = check_lens_camera(v, fn);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(v->device));
  rc = rays_enqueue(v, v->n_distinct, origin, direction, (hipStream_t)hip_stream);
  return rc != RT_OK ? rc : v->done.mark((hipStream_t)hip_stream);
}

int rt_view_rays(rt_view* v, float* origin, float* direction) {
  const char* fn = "rt_view_rays";
  if (!v) return fail(RT_ERR_INVALID_ARG, "%s: null view", fn);
  if (!origin || !direction) return fail(RT_ERR_INVALID_ARG, "%s: origin / direction missing", fn);
  if (!v->has_camera) return fail(RT_ERR_INVALID_ARG, "%s: the view has no camera yet (rt_view_set_camera)", fn);
  int rc = check_lens_camera(v, fn);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(v->device));
  HostCall c;
  c.out(&origin, (size_t)v->n_rays * 12), c.out(&direction, (size_t)v->n_rays * 12);
  if ((rc = c.begin()) != RT_OK) return rc;
  if ((rc = rays_enqueue(v, v->n_distinct, origin, direction, c.stream)) != RT_OK) return rc;
  return c.finish();
}

int rt_render_view_device(rt_scene* s, rt_view* v, const rt_params* p, const rt_ray_radiance* out, void* hip_stream) {
  const int rc = check_render(s, v, p, out, "rt_render_view_device");
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(s->device));
  return render_enqueue(s, v, p, out, (hipStream_t)hip_stream, false);
}

int rt_render_view(rt_scene* s, rt_view* v, const rt_params* p, const rt_ray_radiance* out, rt_stats* stats) {
  int rc = check_render(s, v, p, out, "rt_render_view");
  if (rc != RT_OK) return rc;
  if (stats) memset(stats, 0, sizeof(*stats));
  HIP_TRY(hipSetDevice(s->device));
  if ((rc = v->done.wait()) != RT_OK) return rc;
  const auto t_begin = std::chrono::steady_clock::now();
  const size_t n = v->n_pixels;
  rt_ray_radiance dev = *out;
  HostCall c;
  c.out(&dev.rgb, n * 12), c.out(&dev.valid, n), c.out(&dev.id, n * 4), c.out(&dev.t, n * 4), c.out(&dev.argb, n * 4, true);
  Forget forget{s, c};
  if ((rc = c.begin()) != RT_OK) return rc;
  if ((rc = render_enqueue(s, v, p, &dev, c.stream, true)) != RT_OK) return rc;
  if ((rc = c.finish()) != RT_OK) return rc;
  v->done.clear();
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, v->ev[0], v->ev[1]));
  v->rays_ms = ms;
  if (v->order_ms < 0.0) {
    HIP_TRY(hipEventElapsedTime(&ms, v->ev[1], v->ev[2]));
    v->order_ms = ms;
  }
  HIP_TRY(hipEventElapsedTime(&ms, v->ev[3], v->ev[4]));
  v->resolve_ms = ms;
  if (stats) {
    if ((rc = rt_render_collect_stats(s, stats)) != RT_OK) return rc;
    HIP_TRY(hipEventElapsedTime(&ms, v->ev[0], v->ev[4]));
    stats->kernel_ms = ms;  // generator .. resolve (with secondary rays: every attempt of the batch, as rt_trace_rays)
    stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  }
  return RT_OK;
}

int rt_view_enable_adaptive(rt_view* v) {
  if (!v) return fail(RT_ERR_INVALID_ARG, "rt_view_enable_adaptive: null view");
  if (v->adaptive) return RT_OK;
  HIP_TRY(hipSetDevice(v->device));
  int rc = v->done.wait();
  if (rc != RT_OK) return rc;
  RtArena lay;
  rt_view_adapt_ws_add(lay, v->n_pixels, v->n_rays, RT_ORDER_SCAN_BLOCKS, &v->aws);
  if ((rc = v->abuf.ensure(lay.total())) != RT_OK) return rc;
  lay.bind(v->abuf.p);
  for (hipEvent_t& e : v->aev)
    if (!e) HIP_TRY(hipEventCreate(&e));
  v->adaptive = true;
  return RT_OK;
}

int rt_render_view_adaptive_device(rt_scene* s, rt_view* v, const rt_params* p, const rt_view_refine* rf, const rt_ray_radiance* out,
                                   uint8_t* mask_dev, void* hip_stream) {
  const char* fn = "rt_render_view_adaptive_device";
  const int rc = check_render_adaptive(s, v, p, rf, out, fn);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(s->device));
  for (double& ms : v->astage_ms) ms = 0.0;
  return adaptive_enqueue(s, v, p, rf, out, mask_dev, (hipStream_t)hip_stream, false, nullptr, fn);
}

int rt_render_view_adaptive(rt_scene* s, rt_view* v, const rt_params* p, const rt_view_refine* rf, const rt_ray_radiance* out, uint8_t* mask,
                            rt_stats* stats) {
  const char* fn = "rt_render_view_adaptive";
  int rc = check_render_adaptive(s, v, p, rf, out, fn);
  if (rc != RT_OK) return rc;
  if (stats) memset(stats, 0, sizeof(*stats));
  HIP_TRY(hipSetDevice(s->device));
  if ((rc = v->done.wait()) != RT_OK) return rc;
  const auto t_begin = std::chrono::steady_clock::now();
  const size_t n = v->n_pixels;
  rt_ray_radiance dev = *out;
  HostCall c;
  c.out(&dev.rgb, n * 12), c.out(&dev.valid, n), c.out(&dev.id, n * 4), c.out(&dev.t, n * 4), c.out(&dev.argb, n * 4, true);
  c.out(&mask, n);
  Forget forget{s, c};
  if ((rc = c.begin()) != RT_OK) return rc;
  rt_stats pass1;
  memset(&pass1, 0, sizeof(pass1));
  if ((rc = adaptive_enqueue(s, v, p, rf, &dev, mask, c.stream, true, stats ? &pass1 : nullptr, fn)) != RT_OK) return rc;
  if ((rc = c.finish()) != RT_OK) return rc;
  v->done.clear();
  for (int k = 0; k < 5; k++) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, v->aev[k], v->aev[k + 1]));
    v->astage_ms[k] = ms;
  }
  if (stats) {
    if (v->n_distinct > 1u) {
      if ((rc = rt_render_collect_stats(s, stats)) != RT_OK) return rc;
      stats->rays_primary += pass1.rays_primary, stats->rays_reflection += pass1.rays_reflection, stats->rays_refraction += pass1.rays_refraction;
      stats->rays_shadow += pass1.rays_shadow, stats->pixels_written += pass1.pixels_written, stats->rays_traced += pass1.rays_traced;
      stats->wave_ray_passes += pass1.wave_ray_passes, stats->wave_ray_lanes += pass1.wave_ray_lanes;
      stats->wave_nearest_nodes += pass1.wave_nearest_nodes, stats->wave_nearest_tris += pass1.wave_nearest_tris;
      stats->wave_shadow_nodes += pass1.wave_shadow_nodes, stats->wave_shadow_tris += pass1.wave_shadow_tris;
      stats->wave_shadow_passes += pass1.wave_shadow_passes, stats->wave_nearest_tris_exact += pass1.wave_nearest_tris_exact;
      stats->wave_shadow_tris_exact += pass1.wave_shadow_tris_exact;
      stats->notes |= pass1.notes;
    } else {
      *stats = pass1;
    }
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, v->aev[0], v->aev[5]));
    stats->kernel_ms = ms;  // pass 1 .. resolve (the host form drains the stream behind pass 1 to read its counters: that wait is in here)
    stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  }
  return RT_OK;
}

int rt_view_adaptive_read(rt_view* v, rt_view_adaptive_info* info) {
  if (!v) return fail(RT_ERR_INVALID_ARG, "rt_view_adaptive_read: null view");
  if (!info) return fail(RT_ERR_INVALID_ARG, "rt_view_adaptive_read: null info");
  if (!v->adaptive) return fail(RT_ERR_INVALID_ARG, "rt_view_adaptive_read: the view has no adaptive workspace (rt_view_enable_adaptive)");
  HIP_TRY(hipSetDevice(v->device));
  const int rc = v->done.wait();
  if (rc != RT_OK) return rc;
  if (!v->n_refined_read) {
    HIP_TRY(hipMemcpy(&v->n_refined, v->aws.n_refined, 4, hipMemcpyDeviceToHost));
    v->n_refined_read = true;
  }
  *info = rt_view_adaptive_info{};
  info->n_refined = v->n_refined, info->n_live_rays = v->n_refined * (v->n_distinct - 1u), info->bytes = v->abuf.cap;
  info->pass1_ms = v->astage_ms[0], info->classify_ms = v->astage_ms[1], info->partition_ms = v->astage_ms[2];
  info->pass2_ms = v->astage_ms[3], info->resolve_ms = v->astage_ms[4];
  return RT_OK;
}

int rt_view_read(rt_view* v, uint8_t* plane_of, rt_view_info* info) {
  if (!v) return fail(RT_ERR_INVALID_ARG, "rt_view_read: null view");
  HIP_TRY(hipSetDevice(v->device));
  const int rc = v->done.wait();
  if (rc != RT_OK) return rc;
  if (plane_of) memcpy(plane_of, v->plane_of, v->n_samples);
  if (info) {
    *info = rt_view_info{};
    info->n_pixels = v->n_pixels, info->n_samples = v->n_samples, info->n_distinct = v->n_distinct, info->n_rays = v->n_rays;
    info->bytes = v->buf.cap + rt_ray_order_bytes(v->order);
    info->order_built = v->order_built ? 1u : 0u;
    info->rays_ms = v->rays_ms, info->order_ms = v->order_ms < 0.0 ? 0.0 : v->order_ms, info->resolve_ms = v->resolve_ms;
  }
  return RT_OK;
}

int rt_view_rays_model(const rt_view_desc* d, const rt_view_camera* c, float* origin, float* direction, uint8_t* plane_of, uint32_t* n_distinct) {
  int rc = rt_view_check_desc(d, "rt_view_rays_model");
  if (rc != RT_OK) return rc;
  if ((rc = rt_view_check_camera(c, "rt_view_rays_model")) != RT_OK) return rc;
  float distinct[2 * RT_VIEW_MAX_SAMPLES];
  uint8_t po[RT_VIEW_MAX_SAMPLES];
  const uint32_t nd = rt_view_dedup(d->samples, d->n_samples, distinct, po);
  if (plane_of) memcpy(plane_of, po, d->n_samples);
  if (n_distinct) *n_distinct = nd;
  if (!origin && !direction) return RT_OK;
  const RtViewCam cam = rt_view_cam_of(*d, *c);
  for (uint32_t u = 0; u < nd; u++)
    for (uint32_t p = 0; p < cam.n_pixels; p++) {
      float o[3], dir[3];
      rt_view_ray(cam, p % cam.width, p / cam.width, distinct[2 * u], distinct[2 * u + 1], o, dir);
      const size_t k = 3u * ((size_t)u * cam.n_pixels + p);
      if (origin) memcpy(origin + k, o, 12);
      if (direction) memcpy(direction + k, dir, 12);
    }
  return RT_OK;
}

int rt_view_resolve_model(uint32_t n_pixels, uint32_t n_samples, const uint8_t* plane_of, const rt_ray_radiance* rays, const rt_ray_radiance* pixels) {
  const char* fn = "rt_view_resolve_model";
  if (!plane_of || !rays || !pixels) return fail(RT_ERR_INVALID_ARG, "%s: null argument", fn);
  if (n_samples == 0 || n_samples > RT_VIEW_MAX_SAMPLES) return fail(RT_ERR_INVALID_ARG, "%s: n_samples %u outside 1 .. %u", fn, n_samples, RT_VIEW_MAX_SAMPLES);
  if (!rays->rgb || !rays->valid || !rays->id || !rays->t) return fail(RT_ERR_INVALID_ARG, "%s: the per-ray rgb, valid, id and t planes are all required", fn);
  if (plane_of[0] != 0) return fail(RT_ERR_INVALID_ARG, "%s: plane_of[0] must be 0", fn);
  for (uint32_t k = 0; k < n_samples; k++)
    if (plane_of[k] > k) return fail(RT_ERR_INVALID_ARG, "%s: plane_of[%u] = %u is not a first-occurrence index", fn, k, plane_of[k]);
  const float scale = rt_view_scale(n_samples);
  for (uint32_t p = 0; p < n_pixels; p++)
    rt_view_resolve_pixel(p, n_pixels, n_samples, scale, plane_of, rays->rgb, rays->valid, rays->id, rays->t, pixels->rgb, pixels->valid, pixels->id,
                          pixels->t, pixels->argb);
  return RT_OK;
}

}  // extern "C"
