// atmrt_probes.hip — the harness and debug entry points of include/atmrt.h: single device functions behind host arrays, and what
// the last frame's set-up left in the context (tables, work queue, march route).  Host code only: the kernels they launch are
// compiled by atmrt_kernels.hip.  (atmrt_debug_interp_blend is in atmrt_api.hip, beside the blend it drives.)
#include <cstring>
#include <initializer_list>
#include <vector>

#include "atmrt_ctx.h"
#include "atmrt_multi.h"

using namespace atmrt;

// ---------------------------------------------------------------------------------------------
// harnesses: host arrays in, host arrays out (staged through one device buffer, d_io)
// ---------------------------------------------------------------------------------------------
static int harness_frame(atmrt_ctx* c, Frame* f) {
  if (!c->have_params) {
    atmrt_params_t p;
    atmrt_params_default(&p);
    int rc = atmrt_set_params(c, &p);
    if (rc) return rc;
  }
  return prepare_frame(c, f);
}

// One harness call on c's stream: the uploads, the launch, the downloads, then the synchronisation and the launch's status.
// A copy whose host end is null is skipped: an input or output the caller left out.
struct HarnessCopy {
  void* dst;
  const void* src;
  size_t bytes;
};
template <class Launch>
static int harness_call(atmrt_ctx* c, std::initializer_list<HarnessCopy> uploads, Launch&& launch, std::initializer_list<HarnessCopy> downloads) {
  hipStream_t s = c->stream;
  for (const HarnessCopy& u : uploads)
    if (u.src) HIP_TRY(c, hipMemcpyAsync(u.dst, u.src, u.bytes, hipMemcpyHostToDevice, s));
  launch(s);
  for (const HarnessCopy& d : downloads)
    if (d.dst) HIP_TRY(c, hipMemcpyAsync(d.dst, d.src, d.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  HIP_TRY(c, hipGetLastError());
  return ATMRT_OK;
}

extern "C" int atmrt_terrain_get_elev(atmrt_ctx* c, size_t n, const double* lat, const double* lon, double* elev,
                                      uint8_t* valid) {
  if (!c || (n && (!lat || !lon || !elev || !valid))) return ATMRT_ERR_INVALID_ARGUMENT;
  FORWARD_TO_FIRST_DEVICE(c, atmrt_terrain_get_elev(k_, n, lat, lon, elev, valid));
  Frame f;
  int rc = harness_frame(c, &f);
  if (rc) return rc;
  if (!n) return ATMRT_OK;
  double *d_lat, *d_lon, *d_elev;
  uint8_t* d_valid;
  HIP_TRY(c, reserve_carved(c->d_io, [&](Carve& k) { k(d_lat, n * 8), k(d_lon, n * 8), k(d_elev, n * 8), k(d_valid, n); }));
  return harness_call(c, {{d_lat, lat, n * 8}, {d_lon, lon, n * 8}}, [&](hipStream_t s) { launch_get_elev(f, n, d_lat, d_lon, d_elev, d_valid, s); },
                      {{elev, d_elev, n * 8}, {valid, d_valid, n}});
}

extern "C" int atmrt_ray_paths(atmrt_ctx* c, double h0, size_t n_angles, const double* angles_deg, int32_t straight,
                               double step, size_t n_steps, double* x, double* h) {
  if (!c || (n_angles && (!angles_deg || !x || !h))) return ATMRT_ERR_INVALID_ARGUMENT;
  FORWARD_TO_FIRST_DEVICE(c, atmrt_ray_paths(k_, h0, n_angles, angles_deg, straight, step, n_steps, x, h));
  if (!(step > 0.0)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "step must be positive"); // ray_path.rs:53
  if (n_steps > 50000000) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "too many steps");
  Frame f;
  int rc = harness_frame(c, &f);
  if (rc) return rc;
  if (!n_angles) return ATMRT_OK;
  size_t m = n_angles * (n_steps + 1);
  double *d_ang, *d_x, *d_h;
  HIP_TRY(c, reserve_carved(c->d_io, [&](Carve& k) { k(d_ang, n_angles * 8), k(d_x, m * 8), k(d_h, m * 8); }));
  return harness_call(c, {{d_ang, angles_deg, n_angles * 8}},
                      [&](hipStream_t s) { launch_ray_paths(f, h0, n_angles, d_ang, straight, step, n_steps, d_x, d_h, s); },
                      {{x, d_x, m * 8}, {h, d_h, m * 8}});
}

extern "C" int atmrt_atmosphere_sample(atmrt_ctx* c, size_t n, const double* altitude, double* temperature,
                                       double* pressure, double* n_index, double* dn_dh) {
  if (!c || (n && (!altitude || !temperature || !pressure || !n_index || !dn_dh))) return ATMRT_ERR_INVALID_ARGUMENT;
  FORWARD_TO_FIRST_DEVICE(c, atmrt_atmosphere_sample(k_, n, altitude, temperature, pressure, n_index, dn_dh));
  Frame f;
  int rc = harness_frame(c, &f);
  if (rc) return rc;
  if (!n) return ATMRT_OK;
  double *d_alt, *d_t, *d_p, *d_n, *d_dn;
  HIP_TRY(c, reserve_carved(c->d_io, [&](Carve& k) { k(d_alt, n * 8), k(d_t, n * 8), k(d_p, n * 8), k(d_n, n * 8), k(d_dn, n * 8); }));
  return harness_call(c, {{d_alt, altitude, n * 8}}, [&](hipStream_t s) { launch_atm_sample(f, n, d_alt, d_t, d_p, d_n, d_dn, s); },
                      {{temperature, d_t, n * 8}, {pressure, d_p, n * 8}, {n_index, d_n, n * 8}, {dn_dh, d_dn, n * 8}});
}

extern "C" int atmrt_coords_at_dist(atmrt_ctx* c, double lat0, double lon0, double dir_deg, size_t n,
                                    const double* dist, double* lat, double* lon) {
  if (!c || (n && (!dist || !lat || !lon))) return ATMRT_ERR_INVALID_ARGUMENT;
  FORWARD_TO_FIRST_DEVICE(c, atmrt_coords_at_dist(k_, lat0, lon0, dir_deg, n, dist, lat, lon));
  Frame f;
  int rc = harness_frame(c, &f);
  if (rc) return rc;
  if (!n) return ATMRT_OK;
  double *d_dist, *d_lat, *d_lon;
  HIP_TRY(c, reserve_carved(c->d_io, [&](Carve& k) { k(d_dist, n * 8), k(d_lat, n * 8), k(d_lon, n * 8); }));
  return harness_call(c, {{d_dist, dist, n * 8}}, [&](hipStream_t s) { launch_coords_at_dist(f, lat0, lon0, dir_deg, n, d_dist, d_lat, d_lon, s); },
                      {{lat, d_lat, n * 8}, {lon, d_lon, n * 8}});
}

// ---------------------------------------------------------------------------------------------
// debug probes: what a frame's set-up computed, read back
// ---------------------------------------------------------------------------------------------
extern "C" int atmrt_debug_step_trig(atmrt_ctx* c, size_t cap, double* xs, double* sin_out, double* cos_out, size_t* n_out) {
  if (!c || !n_out || (cap && (!xs || !sin_out || !cos_out))) return ATMRT_ERR_INVALID_ARGUMENT;
  FORWARD_TO_FIRST_DEVICE(c, atmrt_debug_step_trig(k_, cap, xs, sin_out, cos_out, n_out));
  Frame f;
  int rc = harness_frame(c, &f);
  if (rc) return rc;
  *n_out = f.xs_sin ? (size_t)f.march_steps + 1 : 0;
  const size_t n = *n_out < cap ? *n_out : cap;
  if (!n) return ATMRT_OK;
  HIP_TRY(c, hipMemcpyAsync(xs, f.xs, n * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(sin_out, f.xs_sin, n * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(cos_out, f.xs_cos, n * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipGetLastError());
  return ATMRT_OK;
}

extern "C" int atmrt_debug_normal_trig(atmrt_ctx* c, size_t cap, double* out, size_t* n_out) {
  if (!c || !n_out || (cap && !out)) return ATMRT_ERR_INVALID_ARGUMENT;
  FORWARD_TO_FIRST_DEVICE(c, atmrt_debug_normal_trig(k_, cap, out, n_out));
  Frame f;
  int rc = harness_frame(c, &f);
  if (rc) return rc;
  static_assert(sizeof(NormalTrig) == 17 * sizeof(double), "the record is 17 doubles, in the order include/atmrt.h documents");
  *n_out = f.normal_trig ? sizeof(NormalTrig) / sizeof(double) : 0;
  const size_t n = *n_out < cap ? *n_out : cap;
  if (!n) return ATMRT_OK;
  HIP_TRY(c, hipMemcpyAsync(out, f.normal_trig, n * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipGetLastError());
  return ATMRT_OK;
}

extern "C" int atmrt_debug_ceiling_table(atmrt_ctx* c, size_t cap, float* cell, float* suffix, int32_t* rows, int32_t* n_bins, double layout[3]) {
  if (!c || !rows || !n_bins || !layout || (cap && (!cell || !suffix))) return ATMRT_ERR_INVALID_ARGUMENT;
  FORWARD_TO_FIRST_DEVICE(c, atmrt_debug_ceiling_table(k_, cap, cell, suffix, rows, n_bins, layout));
  *rows = *n_bins = 0;
  layout[0] = layout[1] = layout[2] = 0.0;
  if (!c->last.valid || !c->last.ceil_rows) return ATMRT_OK;
  if (c->ceiling.serial() != c->last.ceil_serial)
    return c->fail(ATMRT_ERR_STATE, "the ceiling table of the last frame is gone: a later call built another one in its place");
  const CeilLayout& L = c->last.ceil_layout;
  *rows = c->last.ceil_rows;
  *n_bins = L.n_bins;
  layout[0] = L.dir0, layout[1] = L.rel_lo, layout[2] = L.w;
  const size_t total = (size_t)*rows * (size_t)(L.n_bins + 1), n = total < cap ? total : cap;
  if (!n) return ATMRT_OK;
  std::vector<CeilEntry> host(n);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(host.data(), c->d_ceil.as<CeilEntry>(), n * sizeof(CeilEntry), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (size_t k = 0; k < n; k++) cell[k] = host[k].cell, suffix[k] = host[k].suffix;
  return ATMRT_OK;
}

extern "C" int atmrt_debug_march_order(atmrt_ctx* c, size_t cap, uint32_t* order, uint32_t* n_groups) {
  if (!c || !n_groups || (cap && !order)) return ATMRT_ERR_INVALID_ARGUMENT;
  FORWARD_TO_FIRST_DEVICE(c, atmrt_debug_march_order(k_, cap, order, n_groups));
  *n_groups = 0;
  if (!c->last.valid || !c->last.order_groups) return ATMRT_OK;
  if (c->ceil_order.serial() != c->last.order_serial)
    return c->fail(ATMRT_ERR_STATE, "the march order of the last frame is gone: a later call built another one in its place");
  *n_groups = c->last.order_groups;
  const size_t n = *n_groups < cap ? *n_groups : cap;
  if (!n) return ATMRT_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(order, c->d_ceil_order.as<uint32_t>(), n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return ATMRT_OK;
}

extern "C" int atmrt_debug_march_order_steps(atmrt_ctx* c, size_t cap, uint32_t* order_steps, uint32_t* n_groups) {
  if (!c || !n_groups || (cap && !order_steps)) return ATMRT_ERR_INVALID_ARGUMENT;
  FORWARD_TO_FIRST_DEVICE(c, atmrt_debug_march_order_steps(k_, cap, order_steps, n_groups));
  *n_groups = 0;
  if (!c->last.valid || !c->last.order_groups) return ATMRT_OK;
  if (c->ceil_order.serial() != c->last.order_serial)
    return c->fail(ATMRT_ERR_STATE, "the march order of the last frame is gone: a later call built another one in its place");
  *n_groups = c->last.order_groups;
  const size_t n = *n_groups < cap ? *n_groups : cap;
  if (!n) return ATMRT_OK;
  MarchOrder o{};
  Carve carved(c->d_ceil_order.ptr); // the carving of the build (prepare_ceiling): a queued frame has a table of march_steps + 1 rows
  march_order_layout(c->last.order_groups, (size_t)(c->last.ceil_rows > 0 ? c->last.ceil_rows - 1 : 0), carved, o);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(order_steps, o.order_steps, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return ATMRT_OK;
}

extern "C" int atmrt_debug_last_march_route(atmrt_ctx* c, int32_t index, int32_t* route) {
  if (!c || !route) return ATMRT_ERR_INVALID_ARGUMENT;
  if (c->multi) {
    if (index < 0 || index >= multi_size(c)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "device index %d outside the context's %d devices", index, multi_size(c));
    atmrt_ctx* k = multi_child(c, index);
    const int rc = atmrt_debug_last_march_route(k, -1, route);
    if (rc) c->error = k->error;
    return rc;
  }
  if (index != -1 && index != 0) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "a context of one device has no tile %d", index);
  if (!c->last.valid) return c->fail(ATMRT_ERR_STATE, "atmrt_debug_last_march_route needs a frame: call atmrt_generate first");
  *route = (int32_t)c->last.march_route;
  return ATMRT_OK;
}

extern "C" int atmrt_debug_march_plan(int32_t width, int32_t height, int32_t samples, int32_t n_objects, uint64_t out[6]) {
  if (!out || width < 0 || height < 0 || samples < 0 || n_objects < 0) return ATMRT_ERR_INVALID_ARGUMENT;
  Frame f{};
  f.p.generator = ATMRT_GEN_RECTILINEAR;
  f.wl = width;
  f.h = height;
  f.n_t = samples;
  f.n_objects = n_objects;
  f.opaque = n_objects == 0; // (the plan of a frame over opaque terrain: translucent terrain is not sliced, like scenes with objects)
  const MarchPlan plan = frame_march_plan(f, false);
  const bool sliced = plan.route == MarchRoute::Sliced;
  const SliceLayout& L = plan.slices;
  out[0] = sliced ? 1 : 0;
  out[1] = sliced ? L.n_groups : 0;
  out[2] = sliced ? L.cap : 0;
  out[3] = sliced ? L.bytes : 0;
  out[4] = sliced ? L.slices_after : 0;
  out[5] = MARCH_SLICE_STEPS;
  return ATMRT_OK;
}

extern "C" int atmrt_math_probe(atmrt_ctx* c, int32_t op, size_t n, const double* a, const double* b, double* out0, double* out1) {
  if (!c || (n && (!a || !out0)) || op < 0 || op > ATMRT_PROBE_POW3_SHARED) return ATMRT_ERR_INVALID_ARGUMENT;
  FORWARD_TO_FIRST_DEVICE(c, atmrt_math_probe(k_, op, n, a, b, out0, out1));
  if (!n) return ATMRT_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  double *d_a, *d_b, *d_out0, *d_out1;
  HIP_TRY(c, reserve_carved(c->d_io, [&](Carve& k) { k(d_a, n * 8), k(d_b, n * 8), k(d_out0, n * 8), k(d_out1, n * 8); }));
  return harness_call(c, {{d_a, a, n * 8}, {d_b, b, n * 8}}, [&](hipStream_t s) { launch_math_probe(op, n, d_a, b ? d_b : nullptr, d_out0, d_out1, s); },
                      {{out0, d_out0, n * 8}, {out1, d_out1, n * 8}});
}

extern "C" int atmrt_math_probe3(atmrt_ctx* c, int32_t op, size_t n, const double* a, const double* b0, const double* b1, const double* b2,
                                 double* out0, double* out1, double* out2, int32_t* took) {
  if (!c || (n && (!a || !b0 || !b1 || !b2 || !out0 || !out1 || !out2 || !took)) || op < 0 || op > ATMRT_PROBE3_EXP3_TIGHT || n > ((size_t)1 << 40))
    return ATMRT_ERR_INVALID_ARGUMENT;
  FORWARD_TO_FIRST_DEVICE(c, atmrt_math_probe3(k_, op, n, a, b0, b1, b2, out0, out1, out2, took));
  if (!n) return ATMRT_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  double *d_in[4], *d_out[3]; // a, b0, b1, b2; out0, out1, out2
  int32_t* d_took;
  HIP_TRY(c, reserve_carved(c->d_io, [&](Carve& k) {
    for (double*& d : d_in) k(d, n * 8);
    for (double*& d : d_out) k(d, n * 8);
    k(d_took, n * 4);
  }));
  return harness_call(c, {{d_in[0], a, n * 8}, {d_in[1], b0, n * 8}, {d_in[2], b1, n * 8}, {d_in[3], b2, n * 8}},
                      [&](hipStream_t s) { launch_math_probe3(op, n, d_in[0], d_in[1], d_in[2], d_in[3], d_out[0], d_out[1], d_out[2], d_took, s); },
                      {{out0, d_out[0], n * 8}, {out1, d_out[1], n * 8}, {out2, d_out[2], n * 8}, {took, d_took, n * 4}});
}
