// atmrt_consumers.hip — the entry points of include/atmrt.h that read a finished frame, the context's last one (c->last) or the
// caller's planes of one: the image, the overlay, the visibility map and the frame's bounds, the landmarks, the cast shadows and
// shadow lights, the shadowed image, the sky rays.  Host code only: their kernels are compiled by atmrt_kernels.hip, atmrt_shadow.hip and atmrt_sky.hip.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <vector>

#include "atmrt_ctx.h"
#include "atmrt_multi.h"
#include "atmrt_polar_plan.h"
#include "atmrt_render.h"
#include "atmrt_shadow.h"
#include "atmrt_sky.h"

using namespace atmrt;

// ---------------------------------------------------------------------------------------------
// renderer compositing + colouring
// ---------------------------------------------------------------------------------------------
extern "C" int atmrt_coloring_from_conf(const atmrt_params_t* params, int32_t kind, double water_level, double ambient_light,
                                        double light_zenith_angle, double light_dir, int32_t palette, int32_t has_fog,
                                        double fog_distance, atmrt_coloring_t* out) {
  if (!params || !out) return ATMRT_ERR_INVALID_ARGUMENT;
  if (palette != ATMRT_PALETTE_LEGACY && palette != ATMRT_PALETTE_IMPROVED) return ATMRT_ERR_INVALID_ARGUMENT;
  return coloring_from_conf(*params, kind, water_level, ambient_light, light_zenith_angle, light_dir, palette, has_fog,
                            fog_distance, *out)
             ? ATMRT_ERR_INVALID_ARGUMENT
             : ATMRT_OK;
}

extern "C" int atmrt_draw_image_device(atmrt_ctx* c, const atmrt_coloring_t* coloring, uint8_t* rgb_device) {
  if (!c || !coloring || !rgb_device) return ATMRT_ERR_INVALID_ARGUMENT;
  if (c->multi) return c->fail(ATMRT_ERR_STATE, "a multi-device context draws through atmrt_draw_image (host image) or atmrt_draw_image_gathered_device");
  if (!c->last.valid) return c->fail(ATMRT_ERR_STATE, "atmrt_draw_image needs a frame: call atmrt_generate first");
  if (coloring->kind != ATMRT_COLORING_SIMPLE && coloring->kind != ATMRT_COLORING_SHADING)
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "unknown coloring kind %d", coloring->kind);
  if (coloring->has_fog && !(coloring->fog_distance > 0.0)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "fog_distance must be positive");
  HIP_TRY(c, hipSetDevice(c->device));
  const LastFrame& l = c->last;
  launch_draw_image(l.npx, *coloring, l.alpha, l.packed, l.dense.hit_count, l.offset, l.hits, l.dense, rgb_device, c->stream);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipGetLastError());
  return ATMRT_OK;
}

extern "C" int atmrt_draw_image(atmrt_ctx* c, const atmrt_coloring_t* coloring, uint8_t* rgb) {
  if (!c || !coloring || !rgb) return ATMRT_ERR_INVALID_ARGUMENT;
  if (c->multi) return multi_draw_image(c, coloring, rgb);
  if (!c->last.valid) return c->fail(ATMRT_ERR_STATE, "atmrt_draw_image needs a frame: call atmrt_generate first");
  HIP_TRY(c, hipSetDevice(c->device)); // the staging buffer must live on this context's device
  uint8_t* d_rgb = nullptr;
  HIP_TRY(c, reserve_into(c->d_io, d_rgb, 3 * c->last.npx + 256));
  if (int rc = atmrt_draw_image_device(c, coloring, d_rgb)) return rc;
  HIP_TRY(c, hipMemcpy(rgb, d_rgb, 3 * c->last.npx, hipMemcpyDeviceToHost));
  return ATMRT_OK;
}

// ---------------------------------------------------------------------------------------------
// the annotations of renderer::output_image: ticks resolved on the host (W + H values), lines searched and drawn on the device
// ---------------------------------------------------------------------------------------------
namespace {

double diff_azimuth(double az1, double az2) { // renderer/mod.rs:28-37
  const double diff = az1 - az2;
  if (diff < -180.0) return diff + 360.0;
  if (diff > 180.0) return diff - 360.0;
  return diff;
}

// Iterator::min_by keeps the first of equal minima: strict `<` in ascending index.  (A NaN makes the reference panic in
// partial_cmp().unwrap(); here it never wins.)
bool azimuth_to_x(double azimuth, const double* row, int w, uint32_t* x) { // :39-59
  int candidate = 0;
  double best = std::fabs(diff_azimuth(azimuth, row[0]));
  for (int i = 1; i < w; i++) {
    const double d = std::fabs(diff_azimuth(azimuth, row[i]));
    if (d < best || best != best) best = d, candidate = i;
  }
  const int neighbour = candidate == 0 ? 1 : candidate - 1;
  const double diff_per_pixel = std::fabs(diff_azimuth(row[candidate], row[neighbour]));
  *x = (uint32_t)candidate;
  return std::fabs(diff_azimuth(row[candidate], azimuth)) < diff_per_pixel * 1.5;
}

bool elevation_to_y(double elevation, const double* col, int h, uint32_t* y) { // :61-80
  int candidate = 0;
  double best = std::fabs(elevation - col[0]);
  for (int i = 1; i < h; i++) {
    const double d = std::fabs(elevation - col[i]);
    if (d < best || best != best) best = d, candidate = i;
  }
  const int neighbour = candidate == 0 ? 1 : candidate - 1;
  const double diff_per_pixel = std::fabs(col[candidate] - col[neighbour]);
  *y = (uint32_t)candidate;
  return std::fabs(col[candidate] - elevation) < diff_per_pixel * 1.5;
}

int num_decimals(double x) { // :208-216; f64::round is half away from zero, like round()
  double mul = 1.0;
  for (int i = 0; i < 10; i++, mul *= 10.0) { // 10^i is exact below 10^23
    const double mul_x = x * mul;
    if (std::fabs(std::round(mul_x) - mul_x) < 0.001) return i;
  }
  return 10;
}

int round_decimals(const atmrt_tick_t* ticks, uint32_t n) { // :218-225; TickLike::angle is the step of a Multiple (params.rs:347-352)
  int decimals = 0;
  for (uint32_t i = 0; i < n; i++)
    if (ticks[i].labelled) decimals = std::max(decimals, num_decimals(ticks[i].kind == ATMRT_TICK_SINGLE ? ticks[i].angle : ticks[i].step));
  return decimals;
}

constexpr int OVERLAY_MAX_TICKS_PER_DEF = 1 << 20;

const char* overlay_check(const atmrt_overlay_t& o) {
  if ((o.n_ticks && !o.ticks) || (o.n_vertical_ticks && !o.vertical_ticks)) return "a tick list is NULL";
  for (int v = 0; v < 2; v++) {
    const atmrt_tick_t* t = v ? o.vertical_ticks : o.ticks;
    for (uint32_t i = 0, n = v ? o.n_vertical_ticks : o.n_ticks; i < n; i++) {
      if (t[i].kind != ATMRT_TICK_SINGLE && t[i].kind != ATMRT_TICK_MULTIPLE) return "unknown tick kind";
      if (t[i].kind == ATMRT_TICK_MULTIPLE && !(t[i].step > 0.0 && t[i].step < INFINITY)) return "the step of a Multiple tick must be positive and finite";
    }
  }
  return nullptr;
}

// gen_ticks (:227-268) over row 0 of the azimuth plane (w values) and column 0 of the elevation plane (h values); `out` sorted by
// (vertical, pos).  The label is glibc's %.*f: correctly rounded from the binary value and signed like Rust's {:.N}.
const char* resolve_ticks(const atmrt_params_t& p, const atmrt_overlay_t& o, const double* az, int w, const double* el, int h,
                          std::vector<atmrt_drawn_tick_t>* out) {
  out->clear();
  for (int v = 0; v < 2; v++) {
    const atmrt_tick_t* ticks = v ? o.vertical_ticks : o.ticks;
    const uint32_t n = v ? o.n_vertical_ticks : o.n_ticks;
    const int decimals = round_decimals(ticks, n);
    std::map<uint32_t, atmrt_drawn_tick_t> at; // HashMap<u32, DrawTick>: the larger size stays, the earlier one when equal (:237-246)
    auto put = [&](uint32_t pos, const atmrt_tick_t& t, double angle) {
      atmrt_drawn_tick_t d{};
      d.pos = pos, d.size = t.size, d.labelled = t.labelled ? 1 : 0, d.vertical = v;
      snprintf(d.label, sizeof d.label, "%.*f", decimals, angle);
      auto it = at.find(pos);
      if (it == at.end()) at.emplace(pos, d);
      else if (it->second.size < d.size) it->second = d;
    };
    for (uint32_t i = 0; i < n; i++) {
      const atmrt_tick_t& t = ticks[i];
      uint32_t pos;
      if (t.kind == ATMRT_TICK_SINGLE) { // :89-106, :149-166
        if (v ? elevation_to_y(t.angle, el, h, &pos) : azimuth_to_x(t.angle, az, w, &pos)) put(pos, t, t.angle);
        continue;
      }
      int count = 0;
      if (!v) { // :107-138: the UNWRAPPED current_az goes to azimuth_to_x, the wrapped one into the label
        const double min_az = p.frame.direction - p.frame.fov / 2.0, max_az = p.frame.direction + p.frame.fov / 2.0;
        for (double current_az = std::ceil((min_az - t.bias) / t.step) * t.step + t.bias; current_az < max_az; current_az += t.step) {
          if (++count > OVERLAY_MAX_TICKS_PER_DEF) return "a Multiple tick yields more than 2^20 ticks";
          const double azimuth = current_az < 0.0 ? current_az + 360.0 : current_az >= 360.0 ? current_az - 360.0 : current_az;
          if (azimuth_to_x(current_az, az, w, &pos)) put(pos, t, azimuth);
        }
      } else { // :167-199: the folded elevation goes to elevation_to_y and into the label
        const double aspect = (double)p.height / (double)p.width;
        const double min_elev = p.frame.tilt - p.frame.fov * aspect / 2.0, max_elev = p.frame.tilt + p.frame.fov * aspect / 2.0;
        for (double current_elev = std::ceil((min_elev - t.bias) / t.step) * t.step + t.bias; current_elev < max_elev; current_elev += t.step) {
          if (++count > OVERLAY_MAX_TICKS_PER_DEF) return "a Multiple tick yields more than 2^20 ticks";
          const double elevation = current_elev < -90.0 ? -180.0 - current_elev : current_elev > 90.0 ? 180.0 - current_elev : current_elev;
          if (elevation_to_y(elevation, el, h, &pos)) put(pos, t, elevation);
        }
      }
    }
    for (const auto& kv : at) out->push_back(kv.second);
  }
  return nullptr;
}

bool earth_shape_is_flat(int32_t kind) { // EarthModel::to_shape, earth_model/mod.rs:95-112
  return kind == ATMRT_EARTH_AZIMUTHAL_EQUIDISTANT || kind == ATMRT_EARTH_FLAT_DISTORTED || kind == ATMRT_EARTH_OBSERVER_AE ||
         kind == ATMRT_EARTH_SIMPLE_OBSERVER_AE;
}

// What the entry points that read the context's own last frame ask first; 0, or a status with the message set.  on_multi: the rest
// of the sentence a multi-device parent answers with, naming the feature's *_planes_device entry point.
int frame_state_check(atmrt_ctx* c, const char* what, const char* on_multi) {
  if (c->multi) return c->fail(ATMRT_ERR_STATE, "a multi-device context %s", on_multi);
  if (!c->last.valid) return c->fail(ATMRT_ERR_STATE, "%s needs a frame: call atmrt_generate first", what);
  return ATMRT_OK;
}
int u16_size_check(atmrt_ctx* c, uint32_t width, uint32_t height) {
  if (width > 65535 || height > 65535) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "width and height are u16 (params.rs:398-402)");
  return ATMRT_OK;
}
// *k: the device context that owns the memory `ptr` points at (its stream, its buffers, its copy of the observer altitude): c
// itself, or the sub-context of a multi-device c on the pointer's device.  `name` is the pointer's name in the messages.
int planes_context(atmrt_ctx* c, const void* ptr, const char* name, atmrt_ctx** k) {
  *k = c;
  if (!c->multi) return ATMRT_OK;
  hipPointerAttribute_t attr{};
  if (hipPointerGetAttributes(&attr, ptr) != hipSuccess) {
    (void)hipGetLastError();
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s is not a device allocation", name);
  }
  for (int i = 0; i < multi_size(c); i++)
    if (multi_child(c, i)->device == attr.device) return *k = multi_child(c, i), ATMRT_OK;
  return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s is in the memory of device %d, which is not a device of this context", name, attr.device);
}

// output_image's annotations (:419-431) over the planes `az`, `el` ([h][w], memory of c's device) of a frame c has generated with
// the position and atmosphere still set (its observer altitude is in d_alt, its atmosphere table in d_atm).
int draw_overlay_on(atmrt_ctx* c, atmrt_ctx* report, const atmrt_params_t& p, const atmrt_overlay_t& o, const double* az, const double* el,
                    int w, int h, uint8_t* rgb, atmrt_drawn_tick_t* drawn, size_t capacity, size_t* n_drawn, double* flat_horizon_deg) {
  if (flat_horizon_deg) *flat_horizon_deg = NAN;
  if (n_drawn) *n_drawn = 0;
  if (w < 2 || h < 2) return report->fail(ATMRT_ERR_INVALID_ARGUMENT, "the overlay needs an image of at least 2 x 2 pixels, not %d x %d", w, h);
  if (const char* msg = overlay_check(o)) return report->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s", msg);
  HIP_TRY(report, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  std::vector<atmrt_drawn_tick_t> ticks;
  if (o.n_ticks || o.n_vertical_ticks) { // row 0 and column 0: W + H doubles to the host
    std::vector<double> az0(w), el0(h);
    HIP_TRY(report, hipMemcpyAsync(az0.data(), az, (size_t)w * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(report, hipMemcpy2DAsync(el0.data(), 8, el, (size_t)w * 8, 8, (size_t)h, hipMemcpyDeviceToHost, s));
    HIP_TRY(report, hipStreamSynchronize(s));
    if (const char* msg = resolve_ticks(p, o, az0.data(), w, el0.data(), h, &ticks)) return report->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s", msg);
  }
  if (n_drawn) *n_drawn = ticks.size();
  if (drawn && capacity < ticks.size())
    return report->fail(ATMRT_ERR_INVALID_ARGUMENT, "capacity %zu is less than the %zu ticks of the frame", capacity, ticks.size());
  if (drawn) std::copy(ticks.begin(), ticks.end(), drawn);
  const bool flat = o.show_flat_horizon && earth_shape_is_flat(p.earth.kind) && !p.straight_rays; // :420-422
  const bool eye = o.show_eye_level != 0;
  int n_cu = 0;
  HIP_TRY(report, hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device));
  const int bands = overlay_bands(w, h, n_cu);
  struct DevTick {
    uint32_t pos, size;
    int32_t vertical, _pad;
  };
  DevTick* d_ticks = nullptr;
  double* d = nullptr; // the four values of one atmosphere sample
  char* d_work = nullptr;
  HIP_TRY(report, reserve_carved(c->d_overlay, [&](Carve& k) { k(d_ticks, ticks.size() * sizeof(DevTick)), k(d, 32), k(d_work, overlay_workspace_bytes(w, bands)); }));
  double target = NAN;
  if (flat) { // n at the observer's altitude through the library's own refr_n (k_atm_sample); acos and the degrees on the host
    Frame f{};
    f.atm = c->d_atm.as<AtmTable>();
    launch_atm_sample(f, 1, c->d_alt.as<double>(), d, d + 1, d + 2, d + 3, s);
    double n_at_observer = 0.0;
    HIP_TRY(report, hipMemcpyAsync(&n_at_observer, d + 2, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(report, hipStreamSynchronize(s));
    target = std::acos(1.0 / n_at_observer) * (180.0 / M_PI); // f64::to_degrees
    if (flat_horizon_deg) *flat_horizon_deg = target;
  }
  if (!ticks.empty()) {
    std::vector<DevTick> dt(ticks.size());
    for (size_t i = 0; i < ticks.size(); i++) dt[i] = DevTick{ticks[i].pos, ticks[i].size, ticks[i].vertical, 0};
    HIP_TRY(report, hipMemcpyAsync(d_ticks, dt.data(), dt.size() * sizeof(DevTick), hipMemcpyHostToDevice, s));
    HIP_TRY(report, hipStreamSynchronize(s)); // dt goes out of scope
    launch_overlay_ticks(d_ticks, (int)dt.size(), w, h, rgb, s);
  }
  if (flat || eye) { // a NaN target is never close to anything: its line is all None
    int32_t* y_of_x = nullptr;
    launch_overlay_find_elev(el, w, h, bands, target, eye ? 0.0 : NAN, d_work, &y_of_x, s);
    const uint8_t flat_color[3] = {0, 128, 255}, eye_color[3] = {255, 128, 255};
    if (flat) launch_overlay_lines(y_of_x, w, h, rgb, flat_color, s);
    if (eye) launch_overlay_lines(y_of_x + w, w, h, rgb, eye_color, s);
  }
  HIP_TRY(report, hipStreamSynchronize(s));
  HIP_TRY(report, hipGetLastError());
  return ATMRT_OK;
}

} // namespace

extern "C" int atmrt_overlay_resolve_ticks(const atmrt_params_t* params, const atmrt_overlay_t* overlay, const double* azimuth_row0,
                                           const double* elevation_col0, atmrt_drawn_tick_t* drawn, size_t capacity, size_t* n_drawn) {
  if (!params || !overlay || !azimuth_row0 || !elevation_col0 || !n_drawn) return ATMRT_ERR_INVALID_ARGUMENT;
  *n_drawn = 0;
  const bool whole = params->col_begin == 0 && params->col_end == 0;
  const int w = whole ? params->width : (int)params->col_end - (int)params->col_begin, h = params->height;
  if (w < 2 || h < 2 || overlay_check(*overlay)) return ATMRT_ERR_INVALID_ARGUMENT;
  std::vector<atmrt_drawn_tick_t> ticks;
  if (resolve_ticks(*params, *overlay, azimuth_row0, w, elevation_col0, h, &ticks)) return ATMRT_ERR_INVALID_ARGUMENT;
  *n_drawn = ticks.size();
  if (!drawn) return ATMRT_OK;
  if (capacity < ticks.size()) return ATMRT_ERR_INVALID_ARGUMENT;
  std::copy(ticks.begin(), ticks.end(), drawn);
  return ATMRT_OK;
}

extern "C" int atmrt_draw_overlay_device(atmrt_ctx* c, const atmrt_overlay_t* overlay, uint8_t* rgb_device, atmrt_drawn_tick_t* drawn,
                                         size_t capacity, size_t* n_drawn, double* flat_horizon_deg) {
  if (!c || !overlay || !rgb_device) return ATMRT_ERR_INVALID_ARGUMENT;
  if (int rc = frame_state_check(c, "atmrt_draw_overlay", "draws its overlay on the gathered planes: atmrt_draw_overlay_planes_device")) return rc;
  const LastFrame& l = c->last;
  return draw_overlay_on(c, c, l.params, *overlay, l.dense.azimuth, l.dense.elevation_angle, l.wl, l.h, rgb_device, drawn, capacity, n_drawn,
                         flat_horizon_deg);
}

extern "C" int atmrt_draw_overlay(atmrt_ctx* c, const atmrt_overlay_t* overlay, uint8_t* rgb, atmrt_drawn_tick_t* drawn, size_t capacity,
                                  size_t* n_drawn, double* flat_horizon_deg) {
  if (!c || !overlay || !rgb) return ATMRT_ERR_INVALID_ARGUMENT;
  if (int rc = frame_state_check(c, "atmrt_draw_overlay", "draws its overlay on the gathered planes: atmrt_draw_overlay_planes_device")) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  uint8_t* d_rgb = nullptr;
  HIP_TRY(c, reserve_into(c->d_io, d_rgb, 3 * c->last.npx + 256));
  HIP_TRY(c, hipMemcpy(d_rgb, rgb, 3 * c->last.npx, hipMemcpyHostToDevice));
  if (int rc = atmrt_draw_overlay_device(c, overlay, d_rgb, drawn, capacity, n_drawn, flat_horizon_deg)) return rc;
  HIP_TRY(c, hipMemcpy(rgb, d_rgb, 3 * c->last.npx, hipMemcpyDeviceToHost));
  return ATMRT_OK;
}

extern "C" int atmrt_draw_overlay_planes_device(atmrt_ctx* c, const atmrt_overlay_t* overlay, const double* azimuth,
                                                const double* elevation_angle, uint32_t width, uint32_t height, uint8_t* rgb_device,
                                                atmrt_drawn_tick_t* drawn, size_t capacity, size_t* n_drawn, double* flat_horizon_deg) {
  if (!c || !overlay || !azimuth || !elevation_angle || !rgb_device) return ATMRT_ERR_INVALID_ARGUMENT;
  if (int rc = u16_size_check(c, width, height)) return rc;
  if (!c->have_params) return c->fail(ATMRT_ERR_STATE, "atmrt_set_params has not been called");
  atmrt_ctx* k = nullptr;
  if (int rc = planes_context(c, rgb_device, "rgb_device", &k)) return rc;
  if (!k->last.valid) return c->fail(ATMRT_ERR_STATE, "atmrt_draw_overlay_planes_device needs a frame: call atmrt_generate_image_device first");
  return draw_overlay_on(k, c, c->params, *overlay, azimuth, elevation_angle, (int)width, (int)height, rgb_device, drawn, capacity, n_drawn,
                         flat_horizon_deg);
}

// ---------------------------------------------------------------------------------------------
// the visibility map: the frame's trace points binned over a latitude / longitude grid (kernels: atmrt_vismap.h)
// ---------------------------------------------------------------------------------------------
extern "C" int atmrt_geo_grid_cell(const atmrt_geo_grid_t* g, double lat, double lon, int64_t* cell) {
  if (!g || !cell) return ATMRT_ERR_INVALID_ARGUMENT;
  *cell = -1;
  if (geo_grid_check(*g)) return ATMRT_ERR_INVALID_ARGUMENT;
  *cell = geo_grid_cell(*g, lat, lon);
  return ATMRT_OK;
}

namespace {

bool vis_aggregate() { return !env_off("ATMRT_VIS_AGGREGATE"); } // read at every call, like ATMRT_ESCAPE

// k: the context whose device holds the memory; report: the context the caller handed in (its parent on a multi-device context).
// grid == nullptr: only the bounds.
int vis_run(atmrt_ctx* k, atmrt_ctx* report, const TracePoints& src, const atmrt_geo_grid_t* grid, uint32_t* count, double* min_distance,
            atmrt_visibility_stats_t* stats, double* bounds) {
  HIP_TRY(report, hipSetDevice(k->device));
  hipStream_t s = k->stream;
  HIP_TRY(report, k->d_vis.reserve(vis_block_bytes()));
  launch_vis_reset(k->d_vis.ptr, s);
  if (grid) launch_vis_map(src, *grid, vis_aggregate(), count, min_distance, k->d_vis.ptr, s);
  else launch_vis_bounds(src, k->d_vis.ptr, s);
  uint64_t block[16] = {};
  HIP_TRY(report, hipMemcpyAsync(block, k->d_vis.ptr, vis_block_bytes(), hipMemcpyDeviceToHost, s));
  HIP_TRY(report, hipStreamSynchronize(s));
  HIP_TRY(report, hipGetLastError());
  vis_block_decode(block, stats, bounds);
  return ATMRT_OK;
}

int vis_mode_check(atmrt_ctx* c, int32_t mode) {
  if (mode != ATMRT_VIS_FIRST && mode != ATMRT_VIS_ALL) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "unknown visibility mode %d", mode);
  return ATMRT_OK;
}
// the checks every map entry point shares; 0 or a status with the message set
int vis_check(atmrt_ctx* c, const atmrt_geo_grid_t* grid, int32_t mode, const void* count) {
  if (!grid) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "grid is NULL");
  if (!count) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "count is NULL");
  if (int rc = vis_mode_check(c, mode)) return rc;
  if (const char* msg = geo_grid_check(*grid)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s", msg);
  return ATMRT_OK;
}

} // namespace

extern "C" int atmrt_frame_bounds(atmrt_ctx* c, int32_t mode, double out[4]) {
  if (!c || !out) return ATMRT_ERR_INVALID_ARGUMENT;
  if (int rc = vis_mode_check(c, mode)) return rc;
  if (int rc = frame_state_check(c, "atmrt_frame_bounds", "has no frame of its own: atmrt_frame_bounds works on the gathered planes through atmrt_visibility_map_planes_device")) return rc;
  return vis_run(c, c, c->last.points(mode), nullptr, nullptr, nullptr, nullptr, out);
}

extern "C" int atmrt_visibility_map_device(atmrt_ctx* c, const atmrt_geo_grid_t* grid, int32_t mode, uint32_t* count_device,
                                           double* min_distance_device, atmrt_visibility_stats_t* stats) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (int rc = vis_check(c, grid, mode, count_device)) return rc;
  if (int rc = frame_state_check(c, "atmrt_visibility_map", "has no frame of its own: atmrt_visibility_map works on the gathered planes through atmrt_visibility_map_planes_device")) return rc;
  return vis_run(c, c, c->last.points(mode), grid, count_device, min_distance_device, stats, nullptr);
}

extern "C" int atmrt_visibility_map(atmrt_ctx* c, const atmrt_geo_grid_t* grid, int32_t mode, uint32_t* count, double* min_distance,
                                    atmrt_visibility_stats_t* stats) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (int rc = vis_check(c, grid, mode, count)) return rc;
  if (int rc = frame_state_check(c, "atmrt_visibility_map", "has no frame of its own: atmrt_visibility_map works on the gathered planes through atmrt_visibility_map_planes_device")) return rc;
  HIP_TRY(c, hipSetDevice(c->device)); // the staging buffer must live on this context's device
  const size_t n_cells = (size_t)grid->n_lat * grid->n_lon;
  uint32_t* d_count = nullptr;
  double* d_min = nullptr; // what is not asked for takes no room
  HIP_TRY(c, reserve_carved(c->d_io, [&](Carve& k) {
    k(d_count, n_cells * sizeof(uint32_t));
    if (min_distance) k(d_min, n_cells * sizeof(double));
  }));
  if (int rc = atmrt_visibility_map_device(c, grid, mode, d_count, d_min, stats)) return rc;
  HIP_TRY(c, hipMemcpy(count, d_count, n_cells * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (min_distance) HIP_TRY(c, hipMemcpy(min_distance, d_min, n_cells * sizeof(double), hipMemcpyDeviceToHost));
  return ATMRT_OK;
}

extern "C" int atmrt_visibility_map_planes_device(atmrt_ctx* c, const atmrt_geo_grid_t* grid, const double* lat, const double* lon,
                                                  const double* distance, const uint32_t* hit_count, uint32_t width, uint32_t height,
                                                  uint32_t* count_device, double* min_distance_device, atmrt_visibility_stats_t* stats) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (int rc = vis_check(c, grid, ATMRT_VIS_FIRST, count_device)) return rc;
  if (!lat || !lon || !distance || !hit_count) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "a plane is NULL");
  if (int rc = u16_size_check(c, width, height)) return rc;
  atmrt_ctx* k = nullptr;
  if (int rc = planes_context(c, count_device, "count_device", &k)) return rc;
  return vis_run(k, c, TracePoints{(size_t)width * height, width, hit_count, nullptr, lat, lon, distance, nullptr}, grid, count_device, min_distance_device, stats,
                 nullptr);
}

// ---------------------------------------------------------------------------------------------
// landmarks: the nearest trace point of each latitude / longitude (kernels: atmrt_landmarks.h)
// ---------------------------------------------------------------------------------------------
extern "C" int atmrt_landmark_d2(const atmrt_landmark_t* l, double lat, double lon, double* d2) {
  if (!l || !d2) return ATMRT_ERR_INVALID_ARGUMENT;
  *d2 = landmark_d2(*l, lat, lon);
  return ATMRT_OK;
}

namespace {

constexpr size_t LM_MAX = (size_t)1 << 20;        // landmarks per call
constexpr uint64_t LM_MAX_ITEMS = 1ull << 24;     // entries of the index: coarser cells above that
constexpr double LM_WORLD = 1e300;                // the index looks no further than this many degrees (a frame's coordinates are degrees)

// The bucket index of one call: cell c of `grid` lists the landmarks items[cell_start[c] .. cell_start[c + 1]), in ascending order.
// It is a FILTER for the exact rule landmark_d2(l, lat, lon) <= r2 and may only ever add candidates:
//  * a landmark's box is +-r in lat and +-r / lon_scale in lon, PADDED by far more than rounding can move a pair (d2 <= r2 bounds
//    |lat - l.lat| by r (1 + a few 2^-53); the padding is r 1e-6, plus 1e-12 of the magnitudes involved for the rounding of the box's
//    own corners, plus 1e-150 for a radius whose square underflows, where d2 <= 0 admits differences up to 1.6e-162);
//  * the cells a box covers are found with the floor rule of geo_grid_cell itself, applied to the box's corners: the rule is
//    monotone in lat and in lon, so every point inside the box falls into a cell between those of the corners.
// Landmarks whose box misses `bounds` (the frame's, {lat_min, lat_max, lon_min, lon_max}; NaN: no point at all) are in no cell.
// The grid covers the intersection of the bounds and the boxes' hull with cells of 2r x 2r / (largest lon_scale) or larger: at most
// 2000 per axis (2^22 cells in all), about 64 cells per landmark, and doubled until the index holds at most LM_MAX_ITEMS entries.
struct LandmarkIndex {
  atmrt_geo_grid_t grid{0.0, 0.0, 1.0, 1.0, 1u, 1u};
  std::vector<uint32_t> cell_start{0u, 0u}, items;
};

struct LmBox {
  double lat_lo, lat_hi, lon_lo, lon_hi;
};
LmBox landmark_box(const atmrt_landmark_t& l, double r) {
  const double w = r / l.lon_scale;
  const double h_lat = r + (r * 1e-6 + (fabs(l.lat) + r) * 1e-12 + 1e-150), h_lon = w + (w * 1e-6 + (fabs(l.lon) + w) * 1e-12 + 1e-150);
  return LmBox{l.lat - h_lat, l.lat + h_lat, l.lon - h_lon, l.lon + h_lon};
}
// the floor rule of geo_grid_cell on one axis, clamped to the grid's cells
uint32_t lm_axis_cell(double v, double v0, double cell, uint32_t n) {
  const double f = dm_floor((v - v0) / cell);
  if (!(f > 0.0)) return 0u;
  return f < (double)n ? (uint32_t)f : n - 1u;
}

LandmarkIndex landmark_index(const atmrt_landmark_t* lm, size_t n, double r, const double bounds[4]) {
  LandmarkIndex ix;
  std::vector<uint32_t> alive;
  std::vector<LmBox> boxes;
  double hull[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY}, scale_max = 0.0;
  for (size_t i = 0; i < n; i++) {
    const LmBox b = landmark_box(lm[i], r);
    if (!(b.lat_hi >= bounds[0] && b.lat_lo <= bounds[1] && b.lon_hi >= bounds[2] && b.lon_lo <= bounds[3])) continue; // NaN bounds: none
    alive.push_back((uint32_t)i), boxes.push_back(b);
    hull[0] = fmin(hull[0], b.lat_lo), hull[1] = fmax(hull[1], b.lat_hi), hull[2] = fmin(hull[2], b.lon_lo), hull[3] = fmax(hull[3], b.lon_hi);
    scale_max = fmax(scale_max, lm[i].lon_scale);
  }
  if (alive.empty()) return ix;
  const double lat_lo = fmax(fmax(hull[0], bounds[0]), -LM_WORLD), lat_hi = fmin(fmin(hull[1], bounds[1]), LM_WORLD);
  const double lon_lo = fmax(fmax(hull[2], bounds[2]), -LM_WORLD), lon_hi = fmin(fmin(hull[3], bounds[3]), LM_WORLD);
  if (!(lat_lo <= lat_hi && lon_lo <= lon_hi)) return ix;
  const double per_axis = fmin(2000.0, fmax(16.0, ceil(sqrt(64.0 * (double)alive.size()))));
  double cell_lat = fmax(2.0 * r, (lat_hi - lat_lo) / per_axis), cell_lon = fmax(2.0 * r / scale_max, (lon_hi - lon_lo) / per_axis);
  std::vector<uint32_t> i0(alive.size()), i1(alive.size()), j0(alive.size()), j1(alive.size());
  for (;; cell_lat *= 2.0, cell_lon *= 2.0) {
    atmrt_geo_grid_t& g = ix.grid;
    g = atmrt_geo_grid_t{lat_lo, lon_lo, cell_lat, cell_lon, 1u, 1u};
    // the rule's own answer for the far corner decides the cell counts: every point of the region falls into a cell
    g.n_lat = (uint32_t)fmin(dm_floor((lat_hi - lat_lo) / cell_lat), 4095.0) + 1u;
    g.n_lon = (uint32_t)fmin(dm_floor((lon_hi - lon_lo) / cell_lon), 4095.0) + 1u;
    uint64_t total = 0;
    for (size_t a = 0; a < alive.size(); a++) {
      const LmBox& b = boxes[a];
      i0[a] = lm_axis_cell(b.lat_lo, lat_lo, cell_lat, g.n_lat), i1[a] = lm_axis_cell(b.lat_hi, lat_lo, cell_lat, g.n_lat);
      j0[a] = lm_axis_cell(b.lon_lo, lon_lo, cell_lon, g.n_lon), j1[a] = lm_axis_cell(b.lon_hi, lon_lo, cell_lon, g.n_lon);
      total += (uint64_t)(i1[a] - i0[a] + 1u) * (j1[a] - j0[a] + 1u);
    }
    if (total <= LM_MAX_ITEMS || (g.n_lat == 1u && g.n_lon == 1u)) break;
  }
  const atmrt_geo_grid_t& g = ix.grid;
  const size_t n_cells = (size_t)g.n_lat * g.n_lon;
  ix.cell_start.assign(n_cells + 1, 0u);
  for (size_t a = 0; a < alive.size(); a++)
    for (uint32_t i = i0[a]; i <= i1[a]; i++)
      for (uint32_t j = j0[a]; j <= j1[a]; j++) ix.cell_start[(size_t)i * g.n_lon + j + 1]++;
  for (size_t c = 0; c < n_cells; c++) ix.cell_start[c + 1] += ix.cell_start[c];
  ix.items.resize(ix.cell_start[n_cells]);
  std::vector<uint32_t> fill(ix.cell_start.begin(), ix.cell_start.end() - 1);
  for (size_t a = 0; a < alive.size(); a++)
    for (uint32_t i = i0[a]; i <= i1[a]; i++)
      for (uint32_t j = j0[a]; j <= j1[a]; j++) ix.items[fill[(size_t)i * g.n_lon + j]++] = alive[a];
  return ix;
}

// what every landmark entry point refuses; nullptr when the arguments are fine
const char* landmark_args_check(const atmrt_landmark_t* lm, size_t n, double radius_deg) {
  if (!lm) return "landmarks is NULL";
  if (n == 0 || n > LM_MAX) return "the number of landmarks must lie in [1, 2^20]";
  if (!(radius_deg > 0.0 && radius_deg <= 1.0)) return "radius_deg must be finite, positive and at most 1 degree";
  for (size_t i = 0; i < n; i++)
    if (const char* msg = landmark_check(lm[i])) return msg;
  return nullptr;
}

// k: the context whose device holds the frame; report: the context the caller handed in (vis_run).
int landmarks_run(atmrt_ctx* k, atmrt_ctx* report, const TracePoints& src, const atmrt_landmark_t* lm, size_t n, double radius_deg,
                  atmrt_landmark_hit_t* hits, atmrt_landmark_stats_t* stats) {
  double bounds[4];
  if (int rc = vis_run(k, report, src, nullptr, nullptr, nullptr, nullptr, bounds)) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  const LandmarkIndex host = landmark_index(lm, n, radius_deg, bounds);
  report->lm_timings[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  HIP_TRY(report, hipSetDevice(k->device));
  hipStream_t s = k->stream;
  LmIndex ix{host.grid, nullptr, nullptr, nullptr, radius_deg * radius_deg};
  LmState st{};
  atmrt_landmark_hit_t* d_hits = nullptr;
  uint32_t *d_start = nullptr, *d_items = nullptr;
  atmrt_landmark_t* d_lm = nullptr;
  HIP_TRY(report, reserve_carved(k->d_landmarks, [&](Carve& c) {
    c(d_lm, n * sizeof(atmrt_landmark_t)), c(d_start, host.cell_start.size() * sizeof(uint32_t)), c(d_items, host.items.size() * sizeof(uint32_t));
    c(st.count, n * sizeof(uint32_t)), c(st.d2min, n * sizeof(unsigned long long)), c(st.key, n * sizeof(unsigned long long));
    c(st.ctr, LM_N * sizeof(unsigned long long)), c(d_hits, n * sizeof(atmrt_landmark_hit_t));
  }));
  ix.cell_start = d_start, ix.items = d_items, ix.lm = d_lm;
  HIP_TRY(report, hipEventRecord(k->ev[EV_LM_BEGIN], s));
  HIP_TRY(report, hipMemcpyAsync(d_lm, lm, n * sizeof(atmrt_landmark_t), hipMemcpyHostToDevice, s));
  HIP_TRY(report, hipMemcpyAsync(d_start, host.cell_start.data(), host.cell_start.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  if (!host.items.empty()) HIP_TRY(report, hipMemcpyAsync(d_items, host.items.data(), host.items.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  launch_lm_reset(n, st, s);
  HIP_TRY(report, hipEventRecord(k->ev[EV_LM_UPLOADED], s));
  launch_lm_pass(false, src, ix, st, s);
  HIP_TRY(report, hipEventRecord(k->ev[EV_LM_FIRST_PASS], s));
  launch_lm_pass(true, src, ix, st, s);
  HIP_TRY(report, hipEventRecord(k->ev[EV_LM_SECOND_PASS], s));
  launch_lm_finish(n, src, st, d_hits, s);
  HIP_TRY(report, hipEventRecord(k->ev[EV_LM_END], s));
  unsigned long long block[LM_N] = {};
  HIP_TRY(report, hipMemcpyAsync(hits, d_hits, n * sizeof(atmrt_landmark_hit_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(report, hipMemcpyAsync(block, st.ctr, sizeof block, hipMemcpyDeviceToHost, s));
  HIP_TRY(report, hipStreamSynchronize(s));
  HIP_TRY(report, hipGetLastError());
  HIP_TRY(report, event_intervals(k->ev + EV_LM_BEGIN, 4, report->lm_timings + 1));
  if (stats) *stats = atmrt_landmark_stats_t{block[LM_POINTS], block[LM_SKIPPED], block[LM_TESTED], block[LM_WITHIN]};
  return ATMRT_OK;
}

} // namespace

extern "C" int atmrt_locate_landmarks(atmrt_ctx* c, const atmrt_landmark_t* landmarks, size_t n, double radius_deg, int32_t mode,
                                      atmrt_landmark_hit_t* hits, atmrt_landmark_stats_t* stats) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (const char* msg = landmark_args_check(landmarks, n, radius_deg)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s", msg);
  if (!hits) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "hits is NULL");
  if (int rc = vis_mode_check(c, mode)) return rc;
  if (int rc = frame_state_check(c, "atmrt_locate_landmarks", "has no frame of its own: atmrt_locate_landmarks works on the gathered planes through atmrt_locate_landmarks_planes_device")) return rc;
  return landmarks_run(c, c, c->last.points(mode), landmarks, n, radius_deg, hits, stats);
}

extern "C" int atmrt_locate_landmarks_planes_device(atmrt_ctx* c, const atmrt_landmark_t* landmarks, size_t n, double radius_deg,
                                                    const double* lat, const double* lon, const double* distance, const double* elevation,
                                                    const uint32_t* hit_count, uint32_t width, uint32_t height, atmrt_landmark_hit_t* hits,
                                                    atmrt_landmark_stats_t* stats) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (const char* msg = landmark_args_check(landmarks, n, radius_deg)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s", msg);
  if (!hits) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "hits is NULL");
  if (!lat || !lon || !distance || !elevation || !hit_count) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "a plane is NULL");
  if (int rc = u16_size_check(c, width, height)) return rc;
  atmrt_ctx* k = nullptr;
  if (int rc = planes_context(c, lat, "lat", &k)) return rc;
  return landmarks_run(k, c, TracePoints{(size_t)width * height, width, hit_count, nullptr, lat, lon, distance, elevation}, landmarks, n, radius_deg, hits,
                       stats);
}

extern "C" int atmrt_last_landmark_timings(atmrt_ctx* c, double out[5]) {
  if (!c || !out) return ATMRT_ERR_INVALID_ARGUMENT;
  memcpy(out, c->lm_timings, sizeof c->lm_timings);
  return ATMRT_OK;
}

extern "C" int atmrt_landmark_index_probe(const atmrt_landmark_t* landmarks, size_t n, double radius_deg, const double bounds[4],
                                          const double* lat, const double* lon, size_t n_points, uint64_t* offsets, uint32_t* items,
                                          size_t capacity, size_t* n_items) {
  if (!n_items) return ATMRT_ERR_INVALID_ARGUMENT;
  *n_items = 0;
  if (landmark_args_check(landmarks, n, radius_deg) || !bounds || !offsets || (n_points && (!lat || !lon))) return ATMRT_ERR_INVALID_ARGUMENT;
  const LandmarkIndex ix = landmark_index(landmarks, n, radius_deg, bounds);
  std::vector<int64_t> cell(n_points);
  size_t need = 0;
  for (size_t i = 0; i < n_points; i++) {
    cell[i] = geo_grid_cell(ix.grid, lat[i], lon[i]);
    if (cell[i] >= 0) need += ix.cell_start[cell[i] + 1] - ix.cell_start[cell[i]];
  }
  *n_items = need;
  if (need > capacity || (need && !items)) return ATMRT_ERR_INVALID_ARGUMENT;
  size_t at = 0;
  for (size_t i = 0; i < n_points; i++) {
    offsets[i] = at;
    if (cell[i] >= 0)
      for (uint32_t k = ix.cell_start[cell[i]]; k < ix.cell_start[cell[i] + 1]; k++) items[at++] = ix.items[k];
  }
  offsets[n_points] = at;
  return ATMRT_OK;
}

// ---------------------------------------------------------------------------------------------
// cast shadows: which of a frame's first trace points the light reaches (kernels: atmrt_shadow.h; the rule: include/atmrt.h)
// ---------------------------------------------------------------------------------------------
namespace {

// ATMRT_SHADOW_ESCAPE=off: every ray marches to m or to its block (A/B runs, tests/test_gpu_shadows.py).  Read at every call.
bool shadow_escape_enabled() { return !env_off("ATMRT_SHADOW_ESCAPE"); }

// what every shadow entry point asks of reach and lift and of the context's parameters; *m: the samples to reach, the first index
// with d_m >= reach (atmrt_polar_plan.h).  0 or a status with the message set
int shadow_reach_check(atmrt_ctx* c, const char* what, double reach, double lift, int32_t* m) {
  if (!(std::isfinite(reach) && reach > 0.0)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: reach must be finite and positive", what);
  if (!(std::isfinite(lift) && lift >= 0.0)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: lift must be finite and not negative", what);
  if (!c->have_params) return c->fail(ATMRT_ERR_STATE, "%s: atmrt_set_params has not been called", what);
  if (!(c->params.simulation_step > 0.0)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: simulation_step must be positive", what);
  const int32_t steps = lattice_steps(c->params.simulation_step, reach, SHADOW_M_MAX);
  if (steps < 0) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: reach lies more than 65535 samples away", what);
  *m = steps;
  return ATMRT_OK;
}

// what the entry points of one light ask beyond that
int shadow_check(atmrt_ctx* c, const char* what, const atmrt_shadow_spec_t* spec, const void* status, int32_t* m) {
  if (!spec || !status) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: spec or status is NULL", what);
  if (!std::isfinite(spec->azimuth_deg)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: azimuth_deg is not finite", what);
  if (!(std::isfinite(spec->elevation_deg) && spec->elevation_deg > -90.0 && spec->elevation_deg < 90.0))
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: elevation_deg must lie strictly between -90 and 90", what);
  return shadow_reach_check(c, what, spec->reach, spec->lift, m);
}

// what the two entry points on the caller's planes ask of them
int shadow_planes_check(atmrt_ctx* c, const char* what, size_t n_pixels, const uint32_t* hit_count, const double* lat, const double* lon, const double* elev) {
  if (!hit_count || !lat || !lon || !elev) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: a plane is NULL", what);
  if (n_pixels == 0 || n_pixels > 0xffffffffull) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: n_pixels must lie in [1, 2^32 - 1]", what);
  return ATMRT_OK;
}

// The floor of the escape shortcut for THIS call, from the context's cached certificate and the mosaic's top (Frame::esc_floor is a
// Rectilinear frame's only; the shadowed frame may be a Fast one).  The certificate is stated "to max_distance", but nothing in its
// argument depends on a distance: above `from`, r'' > 0 whatever r' is, so a ray with dr/dphi > 0 there ascends for as long as it
// is integrated — the bound holds for any reach.  What does depend on the distance is the straight spherical ray's convexity
// (esc_ang_max): it is evaluated for this call's reach, one step past it (d_m < reach + step).  No certificate (flat earth,
// refracted; an atmosphere the sweep refuses): +inf, every ray marches to m.
double shadow_escape_floor(const atmrt_ctx* k, Frame& f, double reach) {
  f.esc_floor = INFINITY; // the frame's own floor is not this call's
  f.esc_ang_max = INFINITY;
  if (!shadow_escape_enabled()) return INFINITY;
  const double step = f.p.simulation_step;
  if (f.p.straight_rays) {
    if (k->earth.spherical) f.esc_ang_max = 1.5207963267948966 - (reach + step) * f.inv_shape_radius;
    return k->tv.skip_above;
  }
  if (!k->earth.spherical) return INFINITY;
  return std::max(k->tv.skip_above, k->escape.value().from + step);
}

struct Download { // a plane the host asked for (host null, or no bytes: not this one), downloaded inside the call's timed window
  void* host;
  const void* dev;
  size_t bytes;
};

// prepare_frame(k, f) for a shadow or a sky call; report: the context the caller handed in, which gets a child's error text
int prepare_frame_for(atmrt_ctx* k, atmrt_ctx* report, Frame* f) {
  const int rc = prepare_frame(k, f);
  if (rc && k != report) report->error = k->error;
  return rc;
}

// One shadow call around its kernels, for a ShadowJob or a ShadowLightsJob with its source, its m and its planes filled in.
// k: the context whose device holds the memory and whose setting is used; report: the context the caller handed in.
// carve_more: what the call carves from d_shadow beside the list and the counters; launch: its uploads and its kernels.
template <class Job>
int shadow_call(atmrt_ctx* k, atmrt_ctx* report, double reach, Job& job, const std::function<void(Carve&)>& carve_more,
                const std::function<int(const Frame&, hipStream_t)>& launch, std::initializer_list<Download> downloads, atmrt_shadow_stats_t* stats) {
  Frame f;
  if (int rc = prepare_frame_for(k, report, &f)) return rc;
  hipStream_t s = k->stream;
  job.esc_floor = shadow_escape_floor(k, f, reach);
  job.escape = job.esc_floor < INFINITY ? 1 : 0;
  HIP_TRY(report, reserve_carved(k->d_shadow, [&](Carve& cv) {
            cv(job.list, job.src.n_pixels * sizeof(uint32_t)), cv(job.ctr, SH_N * sizeof(unsigned long long)), carve_more(cv);
          }));
  HIP_TRY(report, hipEventRecord(k->ev[EV_SH_BEGIN], s));
  if (int rc = launch(f, s)) return rc;
  HIP_TRY(report, hipEventRecord(k->ev[EV_SH_MARCHED], s));
  unsigned long long ctr[SH_N] = {};
  HIP_TRY(report, hipMemcpyAsync(ctr, job.ctr, sizeof ctr, hipMemcpyDeviceToHost, s));
  for (const Download& d : downloads)
    if (d.host && d.bytes) HIP_TRY(report, hipMemcpyAsync(d.host, d.dev, d.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(report, hipEventRecord(k->ev[EV_SH_END], s));
  HIP_TRY(report, hipStreamSynchronize(s));
  HIP_TRY(report, hipGetLastError());
  HIP_TRY(report, event_intervals(k->ev + EV_SH_BEGIN, 3, report->shadow_timings));
  if (stats) {
    stats->lit = ctr[SH_LIT], stats->shadowed = ctr[SH_SHADOWED];
    stats->none = job.src.n_pixels - ctr[SH_LIST];
    stats->integrated_steps = ctr[SH_STEPS], stats->escaped_rays = ctr[SH_ESCAPED];
  }
  return ATMRT_OK;
}

// host_status / host_block: where the planes are downloaded to (null: none).
int shadow_run(atmrt_ctx* k, atmrt_ctx* report, const atmrt_shadow_spec_t& spec, int32_t m, const TracePoints& src, uint8_t* status_dev,
               uint16_t* block_dev, atmrt_shadow_stats_t* stats, uint8_t* host_status, uint16_t* host_block) {
  ShadowJob job{};
  job.src = src;
  job.azimuth_deg = spec.azimuth_deg, job.elevation_deg = spec.elevation_deg, job.lift = spec.lift;
  job.m = m;
  job.status = status_dev, job.block = block_dev;
  return shadow_call(k, report, spec.reach, job, [](Carve&) {},
                     [&](const Frame& f, hipStream_t s) -> int {
                       launch_shadow_mask(f, job, s, k->ev[EV_SH_COMPACTED]);
                       return ATMRT_OK;
                     },
                     {{host_status, status_dev, src.n_pixels}, {host_block, block_dev, src.n_pixels * sizeof(uint16_t)}}, stats);
}

const char* const SHADOW_ON_MULTI = "has no frame of its own: cast shadows work on the gathered planes through atmrt_shadow_mask_planes_device";

} // namespace

extern "C" int atmrt_shadow_steps(atmrt_ctx* c, double reach, int32_t* m) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (!m) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "atmrt_shadow_steps: m is NULL");
  return shadow_reach_check(c, "atmrt_shadow_steps", reach, 0.0, m);
}

extern "C" int atmrt_shadow_mask_device(atmrt_ctx* c, const atmrt_shadow_spec_t* spec, uint8_t* status_device, uint16_t* block_device,
                                        atmrt_shadow_stats_t* stats) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  int32_t m = 0;
  if (int rc = shadow_check(c, "atmrt_shadow_mask", spec, status_device, &m)) return rc;
  if (int rc = frame_state_check(c, "atmrt_shadow_mask", SHADOW_ON_MULTI)) return rc;
  return shadow_run(c, c, *spec, m, c->last.points(ATMRT_VIS_ALL), status_device, block_device, stats, nullptr, nullptr);
}

extern "C" int atmrt_shadow_mask(atmrt_ctx* c, const atmrt_shadow_spec_t* spec, uint8_t* status, uint16_t* block, atmrt_shadow_stats_t* stats) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  int32_t m = 0;
  if (int rc = shadow_check(c, "atmrt_shadow_mask", spec, status, &m)) return rc;
  if (int rc = frame_state_check(c, "atmrt_shadow_mask", SHADOW_ON_MULTI)) return rc;
  HIP_TRY(c, hipSetDevice(c->device)); // the staging buffer must live on this context's device
  const size_t n = c->last.npx;
  uint16_t* d_block = nullptr; // what is not asked for takes no room
  uint8_t* d_status = nullptr;
  HIP_TRY(c, reserve_carved(c->d_io, [&](Carve& k) { if (block) k(d_block, n * sizeof(uint16_t)); k(d_status, n); }));
  return shadow_run(c, c, *spec, m, c->last.points(ATMRT_VIS_ALL), d_status, d_block, stats, status, block);
}

extern "C" int atmrt_shadow_mask_planes_device(atmrt_ctx* c, const atmrt_shadow_spec_t* spec, size_t n_pixels, const uint32_t* hit_count,
                                               const double* lat, const double* lon, const double* elev, uint8_t* status_device,
                                               uint16_t* block_device, atmrt_shadow_stats_t* stats) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (int rc = shadow_planes_check(c, "atmrt_shadow_mask_planes_device", n_pixels, hit_count, lat, lon, elev)) return rc;
  int32_t m = 0;
  if (int rc = shadow_check(c, "atmrt_shadow_mask_planes_device", spec, status_device, &m)) return rc;
  atmrt_ctx* k = nullptr;
  if (int rc = planes_context(c, status_device, "status_device", &k)) return rc;
  HIP_TRY(c, hipSetDevice(k->device));
  return shadow_run(k, c, *spec, m, TracePoints{n_pixels, 0, hit_count, nullptr, lat, lon, nullptr, elev}, status_device, block_device, stats, nullptr,
                    nullptr);
}

// ---- shadow lights: a direction per point and a list of lights per call (include/atmrt.h, "shadow lights") -------------------
extern "C" int atmrt_shadow_light_direction(const atmrt_earth_model_t* earth, double lat, double lon, double azimuth_deg, double elevation_deg,
                                            double dir[3]) {
  if (!earth || !dir) return ATMRT_ERR_INVALID_ARGUMENT;
  if (!(std::isfinite(lat) && std::isfinite(lon) && std::isfinite(azimuth_deg) && std::isfinite(elevation_deg))) return ATMRT_ERR_INVALID_ARGUMENT;
  if (!(elevation_deg >= -90.0 && elevation_deg <= 90.0)) return ATMRT_ERR_INVALID_ARGUMENT;
  Earth e;
  if (earth_resolve(*earth, e)) return ATMRT_ERR_INVALID_ARGUMENT;
  Vec3 n, ea, u;
  world_directions(e, lat, lon, n, ea, u);
  double sin_az, cos_az, sin_el, cos_el;
  dm_sincos(dm_to_radians(azimuth_deg), &sin_az, &cos_az);
  dm_sincos(dm_to_radians(elevation_deg), &sin_el, &cos_el);
  const Vec3 v = n * (cos_el * cos_az) + ea * (cos_el * sin_az) + u * sin_el;
  dir[0] = v.x, dir[1] = v.y, dir[2] = v.z;
  return ATMRT_OK;
}

extern "C" int atmrt_shadow_local_direction(const atmrt_earth_model_t* earth, const double dir[3], double lat, double lon, double* azimuth_deg,
                                            double* elevation_deg) {
  if (!earth || !dir || !azimuth_deg || !elevation_deg) return ATMRT_ERR_INVALID_ARGUMENT;
  Earth e;
  Vec3 light;
  if (earth_resolve(*earth, e) || !shadow_light_normalise(dir, light)) return ATMRT_ERR_INVALID_ARGUMENT;
  Vec3 n, ea, u;
  world_directions(e, lat, lon, n, ea, u);
  shadow_local_direction(n, ea, u, light, *azimuth_deg, *elevation_deg);
  return ATMRT_OK;
}

namespace {

// what every shadow-lights entry point asks of its arguments and of the context's parameters; lights: [n_lights][3], normalised
int shadow_lights_check(atmrt_ctx* c, const char* what, const atmrt_shadow_lights_spec_t* spec, const void* lit_mask, const void* status,
                        int32_t* m, std::vector<double>& lights) {
  if (!spec || !spec->dir) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: spec or its dir is NULL", what);
  if (!lit_mask && !status) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: neither lit_mask nor status is given", what);
  if (spec->n_lights < 1 || spec->n_lights > SHADOW_LIGHTS_MAX) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: n_lights must lie in [1, 64], not %u", what, spec->n_lights);
  lights.resize(3 * (size_t)spec->n_lights);
  for (uint32_t l = 0; l < spec->n_lights; l++) {
    Vec3 v;
    if (!shadow_light_normalise(spec->dir + 3 * l, v))
      return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: light %u is not a finite vector of a finite, positive squared length", what, l);
    lights[3 * l] = v.x, lights[3 * l + 1] = v.y, lights[3 * l + 2] = v.z;
  }
  return shadow_reach_check(c, what, spec->reach, spec->lift, m);
}

const char* const SHADOW_LIGHTS_ON_MULTI = "has no frame of its own: shadow lights work on the gathered planes through atmrt_shadow_lights_planes_device";

const char* const SHADOW_TRUE_ON_MULTI = "has no frame of its own: true-direction shadow lights work on the gathered planes through atmrt_shadow_lights_true_planes_device";

// shadow_run for a list of lights.  host_*: where the planes are downloaded to (null: none).  table: null, or the refraction table
// of the true-direction rule ("apparent elevation").
int shadow_lights_run(atmrt_ctx* k, atmrt_ctx* report, const atmrt_shadow_lights_spec_t& spec, const std::vector<double>& lights, int32_t m,
                      const TracePoints& src, uint64_t* mask_dev, uint8_t* status_dev, uint16_t* block_dev, atmrt_shadow_stats_t* stats,
                      uint64_t* host_mask, uint8_t* host_status, uint16_t* host_block, const SkyTable* table) {
  ShadowLightsJob job{};
  job.src = src;
  if (table) job.true_dir = 1, job.table = *table;
  job.n_lights = spec.n_lights, job.lift = spec.lift, job.m = m;
  job.lit_mask = reinterpret_cast<unsigned long long*>(mask_dev), job.status = status_dev, job.block = block_dev;
  double* d_dirs = nullptr;
  const size_t planes = src.n_pixels * spec.n_lights;
  return shadow_call(k, report, spec.reach, job, [&](Carve& cv) { cv(d_dirs, 3 * SHADOW_LIGHTS_MAX * sizeof(double)); },
                     [&](const Frame& f, hipStream_t s) -> int {
                       job.dirs = d_dirs;
                       HIP_TRY(report, hipMemcpyAsync(d_dirs, lights.data(), lights.size() * sizeof(double), hipMemcpyHostToDevice, s));
                       launch_shadow_lights(f, job, s, k->ev[EV_SH_COMPACTED]);
                       return ATMRT_OK;
                     },
                     {{host_mask, mask_dev, src.n_pixels * sizeof(uint64_t)}, {host_status, status_dev, planes}, {host_block, block_dev, planes * sizeof(uint16_t)}},
                     stats);
}

// "apparent elevation", further down: the table spec checked and its step resolved; the table of k's setting built or found, every row usable
int sky_table_check(atmrt_ctx* c, const char* what, const atmrt_sky_table_spec_t* spec, atmrt_sky_table_spec_t* resolved);
int sky_table_for_inverse(atmrt_ctx* k, atmrt_ctx* report, const char* what, const atmrt_sky_table_spec_t& resolved, SkyTable* view);

// The routes' bodies, for atmrt_shadow_lights* (table_spec unused) and atmrt_shadow_lights_true* (true_dir).
int shadow_lights_frame(atmrt_ctx* c, const char* what, const atmrt_shadow_lights_spec_t* spec, bool true_dir, const atmrt_sky_table_spec_t* table_spec,
                        bool host, uint64_t* lit_mask, uint8_t* status, uint16_t* block, atmrt_shadow_stats_t* stats) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  int32_t m = 0;
  std::vector<double> lights;
  if (int rc = shadow_lights_check(c, what, spec, lit_mask, status, &m, lights)) return rc;
  atmrt_sky_table_spec_t resolved{};
  if (true_dir)
    if (int rc = sky_table_check(c, what, table_spec, &resolved)) return rc;
  if (int rc = frame_state_check(c, what, true_dir ? SHADOW_TRUE_ON_MULTI : SHADOW_LIGHTS_ON_MULTI)) return rc;
  SkyTable table{};
  if (true_dir)
    if (int rc = sky_table_for_inverse(c, c, what, resolved, &table)) return rc;
  const SkyTable* tab = true_dir ? &table : nullptr;
  if (!host) return shadow_lights_run(c, c, *spec, lights, m, c->last.points(ATMRT_VIS_ALL), lit_mask, status, block, stats, nullptr, nullptr, nullptr, tab);
  HIP_TRY(c, hipSetDevice(c->device)); // the staging buffer must live on this context's device
  // the staging buffer: the mask (8 n), then the block planes (2 n L), then the status planes (n L); what is not asked for takes no room
  const size_t n = c->last.npx, planes = n * spec->n_lights;
  uint64_t* d_mask = nullptr;
  uint16_t* d_block = nullptr;
  uint8_t* d_status = nullptr;
  HIP_TRY(c, reserve_carved(c->d_io, [&](Carve& k) {
    if (lit_mask) k(d_mask, n * sizeof(uint64_t));
    if (block) k(d_block, planes * sizeof(uint16_t));
    if (status) k(d_status, planes);
  }));
  return shadow_lights_run(c, c, *spec, lights, m, c->last.points(ATMRT_VIS_ALL), d_mask, d_status, d_block, stats, lit_mask, status, block, tab);
}

int shadow_lights_planes(atmrt_ctx* c, const char* what, const atmrt_shadow_lights_spec_t* spec, bool true_dir, const atmrt_sky_table_spec_t* table_spec,
                         size_t n_pixels, const uint32_t* hit_count, const double* lat, const double* lon, const double* elev, uint64_t* lit_mask_device,
                         uint8_t* status_device, uint16_t* block_device, atmrt_shadow_stats_t* stats) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (int rc = shadow_planes_check(c, what, n_pixels, hit_count, lat, lon, elev)) return rc;
  int32_t m = 0;
  std::vector<double> lights;
  if (int rc = shadow_lights_check(c, what, spec, lit_mask_device, status_device, &m, lights)) return rc;
  atmrt_sky_table_spec_t resolved{};
  if (true_dir)
    if (int rc = sky_table_check(c, what, table_spec, &resolved)) return rc;
  atmrt_ctx* k = nullptr;
  const bool by_mask = lit_mask_device != nullptr;
  if (int rc = planes_context(c, by_mask ? (const void*)lit_mask_device : (const void*)status_device, by_mask ? "lit_mask_device" : "status_device", &k)) return rc;
  HIP_TRY(c, hipSetDevice(k->device));
  SkyTable table{};
  if (true_dir)
    if (int rc = sky_table_for_inverse(k, c, what, resolved, &table)) return rc;
  return shadow_lights_run(k, c, *spec, lights, m, TracePoints{n_pixels, 0, hit_count, nullptr, lat, lon, nullptr, elev}, lit_mask_device, status_device,
                           block_device, stats, nullptr, nullptr, nullptr, true_dir ? &table : nullptr);
}

} // namespace

extern "C" int atmrt_shadow_lights_device(atmrt_ctx* c, const atmrt_shadow_lights_spec_t* spec, uint64_t* lit_mask_device, uint8_t* status_device,
                                          uint16_t* block_device, atmrt_shadow_stats_t* stats) {
  return shadow_lights_frame(c, "atmrt_shadow_lights", spec, false, nullptr, false, lit_mask_device, status_device, block_device, stats);
}

extern "C" int atmrt_shadow_lights(atmrt_ctx* c, const atmrt_shadow_lights_spec_t* spec, uint64_t* lit_mask, uint8_t* status, uint16_t* block,
                                   atmrt_shadow_stats_t* stats) {
  return shadow_lights_frame(c, "atmrt_shadow_lights", spec, false, nullptr, true, lit_mask, status, block, stats);
}

extern "C" int atmrt_shadow_lights_planes_device(atmrt_ctx* c, const atmrt_shadow_lights_spec_t* spec, size_t n_pixels, const uint32_t* hit_count,
                                                 const double* lat, const double* lon, const double* elev, uint64_t* lit_mask_device,
                                                 uint8_t* status_device, uint16_t* block_device, atmrt_shadow_stats_t* stats) {
  return shadow_lights_planes(c, "atmrt_shadow_lights_planes_device", spec, false, nullptr, n_pixels, hit_count, lat, lon, elev, lit_mask_device,
                              status_device, block_device, stats);
}

extern "C" int atmrt_shadow_lights_true_device(atmrt_ctx* c, const atmrt_shadow_lights_spec_t* spec, const atmrt_sky_table_spec_t* table,
                                               uint64_t* lit_mask_device, uint8_t* status_device, uint16_t* block_device, atmrt_shadow_stats_t* stats) {
  return shadow_lights_frame(c, "atmrt_shadow_lights_true", spec, true, table, false, lit_mask_device, status_device, block_device, stats);
}

extern "C" int atmrt_shadow_lights_true(atmrt_ctx* c, const atmrt_shadow_lights_spec_t* spec, const atmrt_sky_table_spec_t* table, uint64_t* lit_mask,
                                        uint8_t* status, uint16_t* block, atmrt_shadow_stats_t* stats) {
  return shadow_lights_frame(c, "atmrt_shadow_lights_true", spec, true, table, true, lit_mask, status, block, stats);
}

extern "C" int atmrt_shadow_lights_true_planes_device(atmrt_ctx* c, const atmrt_shadow_lights_spec_t* spec, const atmrt_sky_table_spec_t* table,
                                                      size_t n_pixels, const uint32_t* hit_count, const double* lat, const double* lon,
                                                      const double* elev, uint64_t* lit_mask_device, uint8_t* status_device, uint16_t* block_device,
                                                      atmrt_shadow_stats_t* stats) {
  return shadow_lights_planes(c, "atmrt_shadow_lights_true_planes_device", spec, true, table, n_pixels, hit_count, lat, lon, elev, lit_mask_device,
                              status_device, block_device, stats);
}

extern "C" int atmrt_draw_image_shadowed_device(atmrt_ctx* c, const atmrt_coloring_t* coloring, const uint8_t* status_device, uint8_t* rgb_device) {
  if (!c || !coloring || !status_device || !rgb_device) return ATMRT_ERR_INVALID_ARGUMENT;
  if (int rc = frame_state_check(c, "atmrt_draw_image_shadowed", "draws its shadowed image from the gathered planes: not part of this entry point")) return rc;
  if (coloring->kind != ATMRT_COLORING_SIMPLE && coloring->kind != ATMRT_COLORING_SHADING)
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "unknown coloring kind %d", coloring->kind);
  if (coloring->has_fog && !(coloring->fog_distance > 0.0)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "fog_distance must be positive");
  HIP_TRY(c, hipSetDevice(c->device));
  const LastFrame& l = c->last;
  launch_draw_image_shadowed(l.npx, *coloring, l.alpha, l.packed, l.dense.hit_count, l.offset, l.hits, l.dense, status_device, rgb_device, c->stream);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipGetLastError());
  return ATMRT_OK;
}

extern "C" int atmrt_draw_image_shadowed(atmrt_ctx* c, const atmrt_coloring_t* coloring, const uint8_t* status, uint8_t* rgb) {
  if (!c || !coloring || !status || !rgb) return ATMRT_ERR_INVALID_ARGUMENT;
  if (int rc = frame_state_check(c, "atmrt_draw_image_shadowed", "draws its shadowed image from the gathered planes: not part of this entry point")) return rc;
  HIP_TRY(c, hipSetDevice(c->device)); // the staging buffer must live on this context's device
  const size_t n = c->last.npx;
  uint8_t *d_rgb = nullptr, *d_status = nullptr;
  HIP_TRY(c, reserve_carved(c->d_io, [&](Carve& k) { k(d_rgb, 3 * n), k(d_status, n); }));
  HIP_TRY(c, hipMemcpy(d_status, status, n, hipMemcpyHostToDevice));
  if (int rc = atmrt_draw_image_shadowed_device(c, coloring, d_status, d_rgb)) return rc;
  HIP_TRY(c, hipMemcpy(rgb, d_rgb, 3 * n, hipMemcpyDeviceToHost));
  return ATMRT_OK;
}

extern "C" int atmrt_last_shadow_timings(atmrt_ctx* c, double out[3]) {
  if (!c || !out) return ATMRT_ERR_INVALID_ARGUMENT;
  memcpy(out, c->shadow_timings, sizeof c->shadow_timings);
  return ATMRT_OK;
}

// ---------------------------------------------------------------------------------------------
// sky rays and sky light: the true direction of every sky pixel, with the light the column per sky ray and the zenith column; the
// paint calls over them: sun and moon discs, the shade (kernels: atmrt_sky.h; the rules: include/atmrt.h).  A light call is the
// sky call of the same route with a column plane more; a shade call is the bodies call with a shade and a column more.
// ---------------------------------------------------------------------------------------------
namespace {

// ATMRT_SKY_ORDER=forward: the march takes the list from its head (A/B runs, tests/test_gpu_sky.py).  Read at every call.
bool sky_reverse_enabled() {
  const char* e = getenv("ATMRT_SKY_ORDER");
  return !(e && !strcmp(e, "forward"));
}

// what the rule asks of a spec and an h0, whatever the step's source; nullptr, or what is wrong
const char* sky_spec_check(const atmrt_sky_spec_t& s, double h0) {
  if (!(std::isfinite(s.step) && s.step >= 0.0)) return "step must be finite and not negative";
  if (!std::isfinite(s.top) || !std::isfinite(s.floor)) return "top and floor must be finite";
  if (!(s.floor < s.top)) return "floor must lie below top";
  if (s.m < 1 || s.m > SKY_M_MAX) return "m must lie in [1, 1048575]";
  if (!std::isfinite(h0)) return "h0 is not finite";
  return nullptr;
}

// what every sky entry point on a context asks of its spec and of the context's parameters; *step: the step of the march
int sky_check(atmrt_ctx* c, const char* what, const atmrt_sky_spec_t* spec, double h0, double* step) {
  if (!spec) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: spec is NULL", what);
  if (const char* msg = sky_spec_check(*spec, h0)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: %s", what, msg);
  if (!c->have_params) return c->fail(ATMRT_ERR_STATE, "%s: atmrt_set_params has not been called", what);
  *step = spec->step == 0.0 ? c->params.simulation_step : spec->step;
  if (!(std::isfinite(*step) && *step > 0.0)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: simulation_step must be positive", what);
  return ATMRT_OK;
}

// One march call as its entry point hands it on.  spec: the sky spec, null where the caller's spec is NULL; light: the light spec
// of a frame or planes call of the light (it asks for Z0), else null.  The planes are the caller's, host or device as the route
// says; column null: plain sky rays.
struct SkyCall {
  const char* what;
  const atmrt_sky_spec_t* spec;
  const atmrt_sky_light_spec_t* light;
  double* true_elevation;
  uint8_t* status;
  uint32_t* steps;
  double* column;
  atmrt_sky_stats_t* stats;
  double* zenith_column; // where Z0 goes (or null)
};
SkyCall sky_call(const char* what, const atmrt_sky_spec_t* spec, double* true_elevation, uint8_t* status, uint32_t* steps, atmrt_sky_stats_t* stats) {
  return SkyCall{what, spec, nullptr, true_elevation, status, steps, nullptr, stats, nullptr};
}
SkyCall sky_light_call(const char* what, const atmrt_sky_light_spec_t* spec, double* true_elevation, uint8_t* status, uint32_t* steps, double* column,
                       atmrt_sky_stats_t* stats, double* zenith_column) {
  return SkyCall{what, spec ? &spec->sky : nullptr, spec, true_elevation, status, steps, column, stats, zenith_column};
}

// sky_check, and what a light spec asks beyond it
int sky_call_check(atmrt_ctx* c, const SkyCall& a, double h0, double* step) {
  if (int rc = sky_check(c, a.what, a.spec, h0, step)) return rc;
  if (!a.light) return ATMRT_OK;
  if (!std::isfinite(a.light->ref_alt) || !(a.light->ref_alt < a.spec->top)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: ref_alt must be finite and lie below top", a.what);
  if (!(std::isfinite(a.light->column_dz) && a.light->column_dz >= 0.0)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: column_dz must be finite and not negative", a.what);
  return ATMRT_OK;
}

// One sky march around its kernels, for a SkyJob with its source, its h0 and its device planes filled in.  k: the context whose
// device holds the memory and whose setting is used; report: the context the caller handed in.  column: the device column plane
// (null: plain sky rays).  upload: the list call's elevations, inside the timed window.  With a light spec, Z0 of k's atmosphere.
int sky_run(atmrt_ctx* k, atmrt_ctx* report, const SkyCall& a, double step, SkyJob& job, double* column, const std::function<int(hipStream_t)>& upload,
            std::initializer_list<Download> downloads) {
  Frame f;
  if (int rc = prepare_frame_for(k, report, &f)) return rc;
  double z0 = 0.0;
  if (a.light) {
    const double dz = a.light->column_dz == 0.0 ? step : a.light->column_dz;
    if (!sky_zenith_column<true>(k->atm.value().table.table(), a.light->ref_alt, a.spec->top, dz, &z0))
      return report->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: the zenith column from %g m to %g m has more than 1048575 nodes of %g m", a.what, a.light->ref_alt, a.spec->top, dz);
  }
  hipStream_t s = k->stream;
  job.step = step, job.top = a.spec->top, job.floor = a.spec->floor, job.m = a.spec->m;
  job.reverse = sky_reverse_enabled() ? 1 : 0;
  HIP_TRY(report, reserve_carved(k->d_sky, [&](Carve& cv) {
            if (job.hit_count) cv(job.list, job.n_pixels * sizeof(uint32_t));
            cv(job.ctr, SKY_N * sizeof(unsigned long long));
          }));
  HIP_TRY(report, hipEventRecord(k->ev[EV_SKY_BEGIN], s));
  if (upload)
    if (int rc = upload(s)) return rc;
  launch_sky_march(f, job, column, s, k->ev[EV_SKY_COMPACTED]);
  HIP_TRY(report, hipEventRecord(k->ev[EV_SKY_MARCHED], s));
  unsigned long long ctr[SKY_N] = {};
  HIP_TRY(report, hipMemcpyAsync(ctr, job.ctr, sizeof ctr, hipMemcpyDeviceToHost, s));
  for (const Download& d : downloads)
    if (d.host && d.bytes) HIP_TRY(report, hipMemcpyAsync(d.host, d.dev, d.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(report, hipEventRecord(k->ev[EV_SKY_END], s));
  HIP_TRY(report, hipStreamSynchronize(s));
  HIP_TRY(report, hipGetLastError());
  HIP_TRY(report, event_intervals(k->ev + EV_SKY_BEGIN, 3, report->sky_timings));
  if (a.stats) {
    a.stats->none = job.hit_count ? job.n_pixels - ctr[SKY_LIST] : 0;
    a.stats->exit = ctr[SKY_EXIT], a.stats->ground = ctr[SKY_GROUND], a.stats->inside = ctr[SKY_INSIDE], a.stats->lost = ctr[SKY_LOST];
    a.stats->integrated_steps = ctr[SKY_STEPS];
  }
  if (a.light && a.zenith_column) *a.zenith_column = z0;
  return ATMRT_OK;
}

// The list call: n rays from h0 at the caller's elevations, staged like the host planes of the frame call.  light: with the
// column (a.column: the host's, [n]).
int sky_list_call(atmrt_ctx* c, const SkyCall& a, bool light, double h0, size_t n, const double* elevation_deg, atmrt_sky_ray_t* records) {
  if (n > 0xffffffffull) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: n must lie in [0, 2^32 - 1]", a.what);
  double step = 0.0;
  if (int rc = sky_call_check(c, a, h0, &step)) return rc;
  atmrt_ctx* k = c->multi ? multi_child(c, 0) : c;
  HIP_TRY(c, hipSetDevice(k->device));
  SkyJob job{};
  job.n_pixels = n, job.h0 = h0;
  double *d_elev = nullptr, *d_true = nullptr, *d_column = nullptr;
  uint8_t* d_status = nullptr;
  uint32_t* d_steps = nullptr;
  HIP_TRY(c, reserve_carved(k->d_io, [&](Carve& cv) { cv(d_elev, n * 8), cv(d_true, n * 8); if (light) cv(d_column, n * 8); cv(d_steps, n * 4), cv(d_status, n); }));
  job.elevation_angle = d_elev, job.true_elevation = d_true, job.status = d_status, job.steps = d_steps;
  std::vector<double> true_elevation(n);
  std::vector<uint8_t> status(n);
  std::vector<uint32_t> steps(n);
  int rc = sky_run(k, c, a, step, job, d_column,
                   [&](hipStream_t s) -> int {
                     if (n) HIP_TRY(c, hipMemcpyAsync(d_elev, elevation_deg, n * 8, hipMemcpyHostToDevice, s));
                     return ATMRT_OK;
                   },
                   {{true_elevation.data(), d_true, n * 8}, {status.data(), d_status, n}, {steps.data(), d_steps, n * 4}, {a.column, d_column, n * 8}});
  if (rc) return rc;
  for (size_t i = 0; i < n; i++) records[i] = atmrt_sky_ray_t{(int32_t)status[i], steps[i], true_elevation[i]};
  return ATMRT_OK;
}

// The frame call: the sky pixels of c's last frame.  host: a's planes are the host's, staged in d_io and downloaded inside the
// timed window; else they are device planes and the march writes them.
int sky_frame_call(atmrt_ctx* c, const SkyCall& a, const char* on_multi, bool host) {
  double step = 0.0;
  if (int rc = sky_call_check(c, a, 0.0, &step)) return rc;
  if (int rc = frame_state_check(c, a.what, on_multi)) return rc;
  const size_t n = c->last.npx;
  SkyJob job{};
  job.n_pixels = n, job.hit_count = c->last.dense.hit_count, job.elevation_angle = c->last.dense.elevation_angle;
  job.alt = c->d_alt.as<double>();
  double *d_true = a.true_elevation, *d_column = a.column;
  uint32_t* d_steps = a.steps;
  uint8_t* d_status = a.status;
  if (host) {
    HIP_TRY(c, hipSetDevice(c->device)); // the staging buffer must live on this context's device
    HIP_TRY(c, reserve_carved(c->d_io, [&](Carve& k) { // what is not asked for takes no room
              k(d_true, n * 8);
              if (a.column) k(d_column, n * 8);
              if (a.steps) k(d_steps, n * 4);
              k(d_status, n);
            }));
  }
  job.true_elevation = d_true, job.status = d_status, job.steps = d_steps;
  const SkyCall to = host ? a : SkyCall{};
  return sky_run(c, c, a, step, job, d_column, nullptr,
                 {{to.true_elevation, d_true, n * 8}, {to.status, d_status, n}, {to.steps, d_steps, n * 4}, {to.column, d_column, n * 8}});
}

// The gathered-planes call: the caller's device planes, on the context (a child of a multi context) whose device holds them.
int sky_planes_call(atmrt_ctx* c, const SkyCall& a, double h0, size_t n_pixels, const uint32_t* hit_count, const double* elevation_angle) {
  if (n_pixels == 0 || n_pixels > 0xffffffffull) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: n_pixels must lie in [1, 2^32 - 1]", a.what);
  double step = 0.0;
  if (int rc = sky_call_check(c, a, h0, &step)) return rc;
  atmrt_ctx* k = nullptr;
  if (int rc = planes_context(c, a.status, "status_device", &k)) return rc;
  HIP_TRY(c, hipSetDevice(k->device));
  SkyJob job{};
  job.n_pixels = n_pixels, job.hit_count = hit_count, job.elevation_angle = elevation_angle, job.h0 = h0;
  job.true_elevation = a.true_elevation, job.status = a.status, job.steps = a.steps;
  return sky_run(k, c, a, step, job, a.column, nullptr, {});
}

const char* const SKY_ON_MULTI = "has no frame of its own: sky rays work on the gathered planes through atmrt_sky_directions_planes_device and atmrt_sky_bodies_planes_device";
const char* const SKY_LIGHT_ON_MULTI = "has no frame of its own: sky light works on the gathered planes through atmrt_sky_light_planes_device and atmrt_sky_shade_planes_device";

// The paint calls, over the job of their kernel: SkyBodiesJob (the bodies' colours over an optional image) or SkyShadeJob (the
// shade and the column; the image is required, and only this one is timed: sky_shade_ms).
template <class Job>
constexpr bool SKY_SHADES = std::is_same<Job, SkyShadeJob>::value;

struct SkyPaintPlanes { // host or device, as the route says
  const double* true_elevation;
  const uint8_t* status;
  const double* column; // the shade only
  uint8_t* body;
  uint8_t* rgb;
};

// the shade (the shade call only) and the bodies of a call, checked and made into what the kernel holds
template <class Job>
int sky_paint_check(atmrt_ctx* c, const char* what, const atmrt_sky_shade_t* shade, const atmrt_sky_body_t* bodies, uint32_t n_bodies, Job& job) {
  if constexpr (SKY_SHADES<Job>) {
    if (!shade) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: shade is NULL", what);
    if (!sky_shade_valid(*shade))
      return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: the shade needs a finite positive zenith_column, finite tau and exposure that are not negative, and limb in [0, 1]", what);
  }
  uint32_t bad = 0;
  switch (sky_bodies_dev(bodies, n_bodies, job.bodies, &bad)) {
    case SKY_BODIES_TOO_MANY: return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: at most 32 bodies, not %u", what, n_bodies);
    case SKY_BODIES_NULL: return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: bodies is NULL", what);
    case SKY_BODIES_BAD: return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: body %u needs finite angles and a radius strictly between 0 and 90 degrees", what, bad);
    case SKY_BODIES_OK: break;
  }
  job.n_bodies = n_bodies;
  if constexpr (SKY_SHADES<Job>) job.shade = sky_shade_dev(*shade, bodies, n_bodies);
  else
    for (uint32_t k = 0; k < n_bodies; k++) memcpy(job.colour[k], bodies[k].rgb, 3);
  return ATMRT_OK;
}

template <class Job>
int sky_paint_run(atmrt_ctx* k, atmrt_ctx* report, Job& job, size_t n_pixels, const double* azimuth, const SkyPaintPlanes& dev) {
  job.n_pixels = n_pixels, job.azimuth = azimuth;
  job.true_elevation = dev.true_elevation, job.status = dev.status, job.body = dev.body, job.rgb = dev.rgb;
  HIP_TRY(report, hipSetDevice(k->device));
  if constexpr (SKY_SHADES<Job>) {
    job.column = dev.column;
    HIP_TRY(report, hipEventRecord(k->ev[EV_SKY_BEGIN], k->stream));
    launch_sky_shade(job, k->stream);
    HIP_TRY(report, hipEventRecord(k->ev[EV_SKY_COMPACTED], k->stream));
  } else {
    launch_sky_bodies(job, k->stream);
  }
  HIP_TRY(report, hipStreamSynchronize(k->stream));
  HIP_TRY(report, hipGetLastError());
  if constexpr (SKY_SHADES<Job>) HIP_TRY(report, event_intervals(k->ev + EV_SKY_BEGIN, 1, &report->sky_shade_ms));
  return ATMRT_OK;
}

// The frame call over c's last frame.  host: the planes are the host's, staged in d_io around the kernel (rgb only where given).
template <class Job>
int sky_paint_frame(atmrt_ctx* c, const char* what, const char* on_multi, const atmrt_sky_shade_t* shade, const atmrt_sky_body_t* bodies, uint32_t n_bodies,
                    const SkyPaintPlanes& a, bool host) {
  Job job{};
  if (int rc = sky_paint_check(c, what, shade, bodies, n_bodies, job)) return rc;
  if (int rc = frame_state_check(c, what, on_multi)) return rc;
  const size_t n = c->last.npx;
  if (!host) return sky_paint_run(c, c, job, n, c->last.dense.azimuth, a);
  HIP_TRY(c, hipSetDevice(c->device)); // the staging buffer must live on this context's device
  double *d_true = nullptr, *d_column = nullptr;
  uint8_t *d_status = nullptr, *d_body = nullptr, *d_rgb = nullptr;
  HIP_TRY(c, reserve_carved(c->d_io, [&](Carve& k) {
            k(d_true, n * 8);
            if (a.column) k(d_column, n * 8);
            k(d_status, n), k(d_body, n);
            if (a.rgb) k(d_rgb, 3 * n);
          }));
  HIP_TRY(c, hipMemcpy(d_true, a.true_elevation, n * 8, hipMemcpyHostToDevice));
  if (a.column) HIP_TRY(c, hipMemcpy(d_column, a.column, n * 8, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(d_status, a.status, n, hipMemcpyHostToDevice));
  if (a.rgb) HIP_TRY(c, hipMemcpy(d_rgb, a.rgb, 3 * n, hipMemcpyHostToDevice));
  if (int rc = sky_paint_run(c, c, job, n, c->last.dense.azimuth, SkyPaintPlanes{d_true, d_status, d_column, d_body, d_rgb})) return rc;
  HIP_TRY(c, hipMemcpy(a.body, d_body, n, hipMemcpyDeviceToHost));
  if (a.rgb) HIP_TRY(c, hipMemcpy(a.rgb, d_rgb, 3 * n, hipMemcpyDeviceToHost));
  return ATMRT_OK;
}

// The gathered-planes call: the caller's device planes, on the context whose device holds them.
template <class Job>
int sky_paint_planes(atmrt_ctx* c, const char* what, const atmrt_sky_shade_t* shade, const atmrt_sky_body_t* bodies, uint32_t n_bodies, size_t n_pixels,
                     const double* azimuth, const SkyPaintPlanes& a) {
  if (n_pixels == 0 || n_pixels > 0xffffffffull) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: n_pixels must lie in [1, 2^32 - 1]", what);
  Job job{};
  if (int rc = sky_paint_check(c, what, shade, bodies, n_bodies, job)) return rc;
  atmrt_ctx* k = nullptr;
  if (int rc = planes_context(c, a.body, "body_device", &k)) return rc;
  return sky_paint_run(k, c, job, n_pixels, azimuth, a);
}

// the serial march of the two host functions (no device): *out, and with `column` the light's column
int sky_ray_host(const atmrt_atmosphere_t* atmosphere, double wavelength, const atmrt_earth_model_t* earth, int32_t straight_rays, const atmrt_sky_spec_t* spec,
                 double h0, double elevation_deg, atmrt_sky_ray_t* out, double* column) {
  if (!atmosphere || !earth || !spec || !out) return ATMRT_ERR_INVALID_ARGUMENT;
  if (sky_spec_check(*spec, h0) || !(spec->step > 0.0)) return ATMRT_ERR_INVALID_ARGUMENT;
  Earth e;
  if (earth_resolve(*earth, e)) return ATMRT_ERR_INVALID_ARGUMENT;
  AtmTableBuf buf;
  if (atm_compile(*atmosphere, wavelength, buf)) return ATMRT_ERR_INVALID_ARGUMENT;
  const bool sph = e.spherical != 0, straight = straight_rays != 0;
  if (column) *out = sky_march_one<true, true>(buf.table(), sph, e.shape_radius, straight, spec->step, spec->top, spec->floor, spec->m, h0, elevation_deg, column);
  else *out = sky_march_one<true, false>(buf.table(), sph, e.shape_radius, straight, spec->step, spec->top, spec->floor, spec->m, h0, elevation_deg);
  return ATMRT_OK;
}

} // namespace

extern "C" int atmrt_sky_ray_host(const atmrt_atmosphere_t* atmosphere, double wavelength, const atmrt_earth_model_t* earth, int32_t straight_rays,
                                  const atmrt_sky_spec_t* spec, double h0, double elevation_deg, atmrt_sky_ray_t* out) {
  return sky_ray_host(atmosphere, wavelength, earth, straight_rays, spec, h0, elevation_deg, out, nullptr);
}

extern "C" int atmrt_sky_body_host(const atmrt_sky_body_t* bodies, uint32_t n_bodies, double azimuth_deg, double true_elevation_deg, uint32_t* body) {
  SkyBodyDev dev[SKY_BODIES_MAX];
  uint32_t bad = 0;
  if (!body || sky_bodies_dev(bodies, n_bodies, dev, &bad)) return ATMRT_ERR_INVALID_ARGUMENT;
  *body = sky_body_of(dev, n_bodies, azimuth_deg, true_elevation_deg);
  return ATMRT_OK;
}

extern "C" int atmrt_sky_rays(atmrt_ctx* c, const atmrt_sky_spec_t* spec, double h0, size_t n, const double* elevation_deg, atmrt_sky_ray_t* records,
                              atmrt_sky_stats_t* stats) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (n && (!elevation_deg || !records)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "atmrt_sky_rays: elevation_deg or records is NULL");
  return sky_list_call(c, sky_call("atmrt_sky_rays", spec, nullptr, nullptr, nullptr, stats), false, h0, n, elevation_deg, records);
}

extern "C" int atmrt_sky_directions_device(atmrt_ctx* c, const atmrt_sky_spec_t* spec, double* true_elevation_device, uint8_t* status_device,
                                           uint32_t* steps_device, atmrt_sky_stats_t* stats) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (!true_elevation_device || !status_device) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "atmrt_sky_directions: true_elevation or status is NULL");
  return sky_frame_call(c, sky_call("atmrt_sky_directions", spec, true_elevation_device, status_device, steps_device, stats), SKY_ON_MULTI, false);
}

extern "C" int atmrt_sky_directions(atmrt_ctx* c, const atmrt_sky_spec_t* spec, double* true_elevation, uint8_t* status, uint32_t* steps,
                                    atmrt_sky_stats_t* stats) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (!true_elevation || !status) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "atmrt_sky_directions: true_elevation or status is NULL");
  return sky_frame_call(c, sky_call("atmrt_sky_directions", spec, true_elevation, status, steps, stats), SKY_ON_MULTI, true);
}

extern "C" int atmrt_sky_directions_planes_device(atmrt_ctx* c, const atmrt_sky_spec_t* spec, double h0, size_t n_pixels, const uint32_t* hit_count,
                                                  const double* elevation_angle, double* true_elevation_device, uint8_t* status_device,
                                                  uint32_t* steps_device, atmrt_sky_stats_t* stats) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (!hit_count || !elevation_angle || !true_elevation_device || !status_device)
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "atmrt_sky_directions_planes_device: a plane is NULL");
  return sky_planes_call(c, sky_call("atmrt_sky_directions_planes_device", spec, true_elevation_device, status_device, steps_device, stats), h0, n_pixels,
                         hit_count, elevation_angle);
}

extern "C" int atmrt_sky_bodies_device(atmrt_ctx* c, const atmrt_sky_body_t* bodies, uint32_t n_bodies, const double* true_elevation_device,
                                       const uint8_t* status_device, uint8_t* body_device, uint8_t* rgb_device) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (!true_elevation_device || !status_device || !body_device) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "atmrt_sky_bodies: a plane is NULL");
  return sky_paint_frame<SkyBodiesJob>(c, "atmrt_sky_bodies", SKY_ON_MULTI, nullptr, bodies, n_bodies,
                                       SkyPaintPlanes{true_elevation_device, status_device, nullptr, body_device, rgb_device}, false);
}

extern "C" int atmrt_sky_bodies(atmrt_ctx* c, const atmrt_sky_body_t* bodies, uint32_t n_bodies, const double* true_elevation, const uint8_t* status,
                                uint8_t* body, uint8_t* rgb) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (!true_elevation || !status || !body) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "atmrt_sky_bodies: a plane is NULL");
  return sky_paint_frame<SkyBodiesJob>(c, "atmrt_sky_bodies", SKY_ON_MULTI, nullptr, bodies, n_bodies, SkyPaintPlanes{true_elevation, status, nullptr, body, rgb}, true);
}

extern "C" int atmrt_sky_bodies_planes_device(atmrt_ctx* c, const atmrt_sky_body_t* bodies, uint32_t n_bodies, size_t n_pixels, const double* azimuth,
                                              const double* true_elevation_device, const uint8_t* status_device, uint8_t* body_device,
                                              uint8_t* rgb_device) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (!azimuth || !true_elevation_device || !status_device || !body_device)
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "atmrt_sky_bodies_planes_device: a plane is NULL");
  return sky_paint_planes<SkyBodiesJob>(c, "atmrt_sky_bodies_planes_device", nullptr, bodies, n_bodies, n_pixels, azimuth,
                                        SkyPaintPlanes{true_elevation_device, status_device, nullptr, body_device, rgb_device});
}

extern "C" int atmrt_last_sky_timings(atmrt_ctx* c, double out[3]) {
  if (!c || !out) return ATMRT_ERR_INVALID_ARGUMENT;
  memcpy(out, c->sky_timings, sizeof c->sky_timings);
  return ATMRT_OK;
}

// sky light: the entry points

extern "C" int atmrt_sky_zenith_column_host(const atmrt_atmosphere_t* atmosphere, double wavelength, double ref_alt, double top, double dz,
                                            double* zenith_column) {
  if (!atmosphere || !zenith_column) return ATMRT_ERR_INVALID_ARGUMENT;
  AtmTableBuf buf;
  if (atm_compile(*atmosphere, wavelength, buf)) return ATMRT_ERR_INVALID_ARGUMENT;
  return sky_zenith_column<true>(buf.table(), ref_alt, top, dz, zenith_column) ? ATMRT_OK : ATMRT_ERR_INVALID_ARGUMENT;
}

extern "C" int atmrt_sky_light_ray_host(const atmrt_atmosphere_t* atmosphere, double wavelength, const atmrt_earth_model_t* earth, int32_t straight_rays,
                                        const atmrt_sky_spec_t* spec, double h0, double elevation_deg, atmrt_sky_ray_t* out, double* column) {
  if (!column) return ATMRT_ERR_INVALID_ARGUMENT;
  return sky_ray_host(atmosphere, wavelength, earth, straight_rays, spec, h0, elevation_deg, out, column);
}

extern "C" int atmrt_sky_shade_host(const atmrt_sky_shade_t* shade, const atmrt_sky_body_t* bodies, uint32_t n_bodies, double azimuth_deg,
                                    double true_elevation_deg, double column, uint32_t* body, uint8_t* rgb) {
  SkyBodyDev dev[SKY_BODIES_MAX];
  uint32_t bad = 0;
  if (!shade || !body || !rgb || !sky_shade_valid(*shade) || sky_bodies_dev(bodies, n_bodies, dev, &bad)) return ATMRT_ERR_INVALID_ARGUMENT;
  const SkyShadeDev sh = sky_shade_dev(*shade, bodies, n_bodies);
  *body = sky_shade_pixel(sh, dev, n_bodies, azimuth_deg, true_elevation_deg, column, rgb);
  return ATMRT_OK;
}

extern "C" int atmrt_sky_light_rays(atmrt_ctx* c, const atmrt_sky_spec_t* spec, double h0, size_t n, const double* elevation_deg, atmrt_sky_ray_t* records,
                                    double* column, atmrt_sky_stats_t* stats) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (n && (!elevation_deg || !records || !column)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "atmrt_sky_light_rays: elevation_deg, records or column is NULL");
  SkyCall a = sky_call("atmrt_sky_light_rays", spec, nullptr, nullptr, nullptr, stats);
  a.column = column;
  return sky_list_call(c, a, true, h0, n, elevation_deg, records);
}

extern "C" int atmrt_sky_light_device(atmrt_ctx* c, const atmrt_sky_light_spec_t* spec, double* true_elevation_device, uint8_t* status_device,
                                      uint32_t* steps_device, double* column_device, atmrt_sky_stats_t* stats, double* zenith_column) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (!true_elevation_device || !status_device || !column_device) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "atmrt_sky_light: true_elevation, status or column is NULL");
  return sky_frame_call(c, sky_light_call("atmrt_sky_light", spec, true_elevation_device, status_device, steps_device, column_device, stats, zenith_column),
                        SKY_LIGHT_ON_MULTI, false);
}

extern "C" int atmrt_sky_light(atmrt_ctx* c, const atmrt_sky_light_spec_t* spec, double* true_elevation, uint8_t* status, uint32_t* steps, double* column,
                               atmrt_sky_stats_t* stats, double* zenith_column) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (!true_elevation || !status || !column) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "atmrt_sky_light: true_elevation, status or column is NULL");
  return sky_frame_call(c, sky_light_call("atmrt_sky_light", spec, true_elevation, status, steps, column, stats, zenith_column), SKY_LIGHT_ON_MULTI, true);
}

extern "C" int atmrt_sky_light_planes_device(atmrt_ctx* c, const atmrt_sky_light_spec_t* spec, double h0, size_t n_pixels, const uint32_t* hit_count,
                                             const double* elevation_angle, double* true_elevation_device, uint8_t* status_device,
                                             uint32_t* steps_device, double* column_device, atmrt_sky_stats_t* stats, double* zenith_column) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (!hit_count || !elevation_angle || !true_elevation_device || !status_device || !column_device)
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "atmrt_sky_light_planes_device: a plane is NULL");
  return sky_planes_call(c, sky_light_call("atmrt_sky_light_planes_device", spec, true_elevation_device, status_device, steps_device, column_device, stats,
                                           zenith_column),
                         h0, n_pixels, hit_count, elevation_angle);
}

extern "C" int atmrt_sky_shade_device(atmrt_ctx* c, const atmrt_sky_shade_t* shade, const atmrt_sky_body_t* bodies, uint32_t n_bodies,
                                      const double* true_elevation_device, const uint8_t* status_device, const double* column_device,
                                      uint8_t* body_device, uint8_t* rgb_device) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (!true_elevation_device || !status_device || !column_device || !body_device || !rgb_device)
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "atmrt_sky_shade: a plane is NULL");
  return sky_paint_frame<SkyShadeJob>(c, "atmrt_sky_shade", SKY_LIGHT_ON_MULTI, shade, bodies, n_bodies,
                                      SkyPaintPlanes{true_elevation_device, status_device, column_device, body_device, rgb_device}, false);
}

extern "C" int atmrt_sky_shade(atmrt_ctx* c, const atmrt_sky_shade_t* shade, const atmrt_sky_body_t* bodies, uint32_t n_bodies, const double* true_elevation,
                               const uint8_t* status, const double* column, uint8_t* body, uint8_t* rgb) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (!true_elevation || !status || !column || !body || !rgb) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "atmrt_sky_shade: a plane is NULL");
  return sky_paint_frame<SkyShadeJob>(c, "atmrt_sky_shade", SKY_LIGHT_ON_MULTI, shade, bodies, n_bodies, SkyPaintPlanes{true_elevation, status, column, body, rgb},
                                      true);
}

extern "C" int atmrt_sky_shade_planes_device(atmrt_ctx* c, const atmrt_sky_shade_t* shade, const atmrt_sky_body_t* bodies, uint32_t n_bodies,
                                             size_t n_pixels, const double* azimuth, const double* true_elevation_device, const uint8_t* status_device,
                                             const double* column_device, uint8_t* body_device, uint8_t* rgb_device) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (!azimuth || !true_elevation_device || !status_device || !column_device || !body_device || !rgb_device)
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "atmrt_sky_shade_planes_device: a plane is NULL");
  return sky_paint_planes<SkyShadeJob>(c, "atmrt_sky_shade_planes_device", shade, bodies, n_bodies, n_pixels, azimuth,
                                       SkyPaintPlanes{true_elevation_device, status_device, column_device, body_device, rgb_device});
}

extern "C" int atmrt_last_sky_shade_timing(atmrt_ctx* c, double* ms) {
  if (!c || !ms) return ATMRT_ERR_INVALID_ARGUMENT;
  *ms = c->sky_shade_ms;
  return ATMRT_OK;
}

// ---------------------------------------------------------------------------------------------
// apparent elevation: the refraction table of the context's setting and its inverse (kernels: atmrt_sky.h; the rule: include/atmrt.h);
// the true-direction shadow lights above read the table through sky_table_for_inverse
// ---------------------------------------------------------------------------------------------
namespace {

// what the rule asks of a table spec, whatever the step's source; nullptr, or what is wrong
const char* sky_table_spec_check(const atmrt_sky_table_spec_t& s) {
  if (const char* msg = sky_spec_check(s.sky, 0.0)) return msg;
  if (!(std::isfinite(s.alt_lo) && std::isfinite(s.alt_hi) && std::isfinite(s.el_lo) && std::isfinite(s.el_hi))) return "alt_lo, alt_hi, el_lo and el_hi must be finite";
  if (!(s.alt_lo < s.alt_hi)) return "alt_lo must lie below alt_hi";
  if (!(-90.0 < s.el_lo && s.el_lo < s.el_hi && s.el_hi < 90.0)) return "el_lo and el_hi must satisfy -90 < el_lo < el_hi < 90";
  if (s.n_alt < 2 || s.n_alt > SKY_TABLE_ALT_MAX) return "n_alt must lie in [2, 1024]";
  if (s.n_el < 2 || s.n_el > SKY_TABLE_EL_MAX) return "n_el must lie in [2, 65536]";
  if ((uint64_t)s.n_alt * s.n_el > SKY_TABLE_ENTRIES_MAX) return "n_alt * n_el must not exceed 2^24";
  return nullptr;
}

int sky_table_check(atmrt_ctx* c, const char* what, const atmrt_sky_table_spec_t* spec, atmrt_sky_table_spec_t* resolved) {
  if (!spec) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: the table spec is NULL", what);
  if (const char* msg = sky_table_spec_check(*spec)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: table: %s", what, msg);
  *resolved = *spec;
  return sky_check(c, what, &spec->sky, 0.0, &resolved->sky.step);
}

// The table of k's setting under `spec` (its step resolved), built where the key differs from the last build's, and what the host
// asked for of it.  f: prepare_frame(k).  What it did goes to report->sky_table_rebuilt and sky_table_timings.
int sky_table_refresh(atmrt_ctx* k, atmrt_ctx* report, const Frame& f, const atmrt_sky_table_spec_t& spec, double* host_T, uint8_t* host_S,
                      uint32_t* host_tail, SkyTable* view) {
  hipStream_t s = k->stream;
  const SkyLattice lat = sky_lattice(spec);
  const size_t n = (size_t)spec.n_alt * spec.n_el;
  const SkyTableKey key{k->atm.serial(), f.p.straight_rays ? 1 : 0, f.earth.spherical, bits(f.earth.shape_radius), bits(spec.sky.step),
                        bits(spec.sky.top), bits(spec.sky.floor), spec.sky.m, bits(spec.alt_lo), bits(spec.alt_hi), bits(spec.el_lo),
                        bits(spec.el_hi), spec.n_alt, spec.n_el};
  double* d_T = nullptr;
  uint32_t* d_tail = nullptr;
  uint8_t* d_S = nullptr;
  const auto layout = [&](Carve& cv) { cv(d_T, n * sizeof(double)), cv(d_tail, spec.n_alt * sizeof(uint32_t)), cv(d_S, n); };
  HIP_TRY(report, hipEventRecord(k->ev[EV_SKY_BEGIN], s));
  bool rebuilt = false;
  int rc = k->sky_table.refresh(key, [&](SkyTableInfo& info) -> int {
    // the buffer grows inside the build, after the product is dropped: a reservation that fails leaves no table under the old key
    HIP_TRY(report, reserve_carved(k->d_sky_table, layout));
    SkyTableJob job{};
    job.lat = lat, job.step = spec.sky.step, job.top = spec.sky.top, job.floor = spec.sky.floor, job.m = spec.sky.m;
    job.T = d_T, job.S = d_S, job.tail = d_tail;
    HIP_TRY(report, reserve_carved(k->d_sky, [&](Carve& cv) { cv(job.ctr, SKY_N * sizeof(unsigned long long)); }));
    launch_sky_table(f, job, s, k->ev[EV_SKY_COMPACTED]);
    HIP_TRY(report, hipEventRecord(k->ev[EV_SKY_MARCHED], s));
    unsigned long long ctr[SKY_N] = {};
    info.tail.assign(spec.n_alt, 0);
    HIP_TRY(report, hipMemcpyAsync(ctr, job.ctr, sizeof ctr, hipMemcpyDeviceToHost, s));
    HIP_TRY(report, hipMemcpyAsync(info.tail.data(), d_tail, spec.n_alt * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(report, hipStreamSynchronize(s));
    HIP_TRY(report, hipGetLastError());
    info.stats = atmrt_sky_stats_t{0, ctr[SKY_EXIT], ctr[SKY_GROUND], ctr[SKY_INSIDE], ctr[SKY_LOST], ctr[SKY_STEPS]};
    info.first_unusable = -1;
    for (uint32_t j = 0; j < spec.n_alt && info.first_unusable < 0; j++)
      if (!sky_row_usable(info.tail[j], spec.n_el)) info.first_unusable = j;
    return ATMRT_OK;
  }, false, &rebuilt);
  if (rc) return rc;
  if (!rebuilt) { // found: an equal key means equal sizes, the table lies where its build carved it; nothing is reserved here
    Carve cv(k->d_sky_table.ptr);
    layout(cv);
    HIP_TRY(report, hipEventRecord(k->ev[EV_SKY_COMPACTED], s));
    HIP_TRY(report, hipEventRecord(k->ev[EV_SKY_MARCHED], s));
  }
  if (host_T) HIP_TRY(report, hipMemcpyAsync(host_T, d_T, n * sizeof(double), hipMemcpyDeviceToHost, s));
  if (host_S) HIP_TRY(report, hipMemcpyAsync(host_S, d_S, n, hipMemcpyDeviceToHost, s));
  if (host_tail) memcpy(host_tail, k->sky_table.value().tail.data(), spec.n_alt * sizeof(uint32_t));
  HIP_TRY(report, hipEventRecord(k->ev[EV_SKY_END], s));
  HIP_TRY(report, hipStreamSynchronize(s));
  HIP_TRY(report, hipGetLastError());
  HIP_TRY(report, event_intervals(k->ev + EV_SKY_BEGIN, 3, report->sky_table_timings));
  if (!rebuilt) report->sky_table_timings[0] = report->sky_table_timings[1] = 0.0;
  report->sky_table_rebuilt = rebuilt ? 1 : 0;
  *view = SkyTable{lat, d_T, d_S, d_tail};
  return ATMRT_OK;
}

int sky_table_prepare(atmrt_ctx* k, atmrt_ctx* report, Frame* f) {
  HIP_TRY(report, hipSetDevice(k->device));
  return prepare_frame_for(k, report, f);
}

int sky_table_for_inverse(atmrt_ctx* k, atmrt_ctx* report, const char* what, const atmrt_sky_table_spec_t& resolved, SkyTable* view) {
  Frame f;
  if (int rc = sky_table_prepare(k, report, &f)) return rc;
  if (int rc = sky_table_refresh(k, report, f, resolved, nullptr, nullptr, nullptr, view)) return rc;
  const SkyTableInfo& info = k->sky_table.value();
  if (info.first_unusable >= 0) {
    const uint32_t j = (uint32_t)info.first_unusable;
    return report->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: row %u of the table (altitude %g m) is not usable: its monotone tail starts at entry %u of %u", what, j,
                        sky_lattice_alt(view->lat, j), info.tail[j], resolved.n_el);
  }
  return ATMRT_OK;
}

} // namespace

extern "C" int atmrt_sky_table(atmrt_ctx* c, const atmrt_sky_table_spec_t* spec, double* true_elevation, uint8_t* status, uint32_t* tail,
                               atmrt_sky_stats_t* stats) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  atmrt_sky_table_spec_t resolved{};
  if (int rc = sky_table_check(c, "atmrt_sky_table", spec, &resolved)) return rc;
  atmrt_ctx* k = c->multi ? multi_child(c, 0) : c;
  Frame f;
  if (int rc = sky_table_prepare(k, c, &f)) return rc;
  SkyTable view{};
  if (int rc = sky_table_refresh(k, c, f, resolved, true_elevation, status, tail, &view)) return rc;
  if (stats) *stats = k->sky_table.value().stats;
  return ATMRT_OK;
}

extern "C" int atmrt_sky_tail_host(const atmrt_sky_table_spec_t* spec, const double* true_elevation, const uint8_t* status, uint32_t* tail) {
  if (!spec || !true_elevation || !status || !tail) return ATMRT_ERR_INVALID_ARGUMENT;
  if (sky_table_spec_check(*spec)) return ATMRT_ERR_INVALID_ARGUMENT;
  for (uint32_t j = 0; j < spec->n_alt; j++) tail[j] = sky_tail_of(true_elevation + (size_t)j * spec->n_el, status + (size_t)j * spec->n_el, spec->n_el);
  return ATMRT_OK;
}

extern "C" int atmrt_sky_apparent_host(const atmrt_sky_table_spec_t* spec, const double* true_elevation, const uint32_t* tail, double h, double t,
                                       double* apparent) {
  if (!spec || !true_elevation || !tail || !apparent) return ATMRT_ERR_INVALID_ARGUMENT;
  if (sky_table_spec_check(*spec)) return ATMRT_ERR_INVALID_ARGUMENT;
  for (uint32_t j = 0; j < spec->n_alt; j++)
    if (!sky_row_usable(tail[j], spec->n_el)) return ATMRT_ERR_INVALID_ARGUMENT;
  *apparent = sky_apparent(SkyTable{sky_lattice(*spec), true_elevation, nullptr, tail}, h, t);
  return ATMRT_OK;
}

extern "C" int atmrt_sky_apparent(atmrt_ctx* c, const atmrt_sky_table_spec_t* spec, size_t n, const double* h, const double* t, double* apparent) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (n && (!h || !t || !apparent)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "atmrt_sky_apparent: h, t or apparent is NULL");
  if (n > 0xffffffffull) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "atmrt_sky_apparent: n must lie in [0, 2^32 - 1]");
  atmrt_sky_table_spec_t resolved{};
  if (int rc = sky_table_check(c, "atmrt_sky_apparent", spec, &resolved)) return rc;
  atmrt_ctx* k = c->multi ? multi_child(c, 0) : c;
  SkyTable view{};
  if (int rc = sky_table_for_inverse(k, c, "atmrt_sky_apparent", resolved, &view)) return rc;
  if (!n) return ATMRT_OK;
  double *d_h = nullptr, *d_t = nullptr, *d_out = nullptr;
  HIP_TRY(c, reserve_carved(k->d_io, [&](Carve& cv) { cv(d_h, n * 8), cv(d_t, n * 8), cv(d_out, n * 8); }));
  hipStream_t s = k->stream;
  HIP_TRY(c, hipMemcpyAsync(d_h, h, n * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipMemcpyAsync(d_t, t, n * 8, hipMemcpyHostToDevice, s));
  launch_sky_apparent(view, k->params.straight_rays != 0, n, d_h, d_t, d_out, s);
  HIP_TRY(c, hipMemcpyAsync(apparent, d_out, n * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  HIP_TRY(c, hipGetLastError());
  return ATMRT_OK;
}

extern "C" int atmrt_last_sky_table_work(atmrt_ctx* c, int32_t* rebuilt, double ms[3]) {
  if (!c || !rebuilt || !ms) return ATMRT_ERR_INVALID_ARGUMENT;
  *rebuilt = c->sky_table_rebuilt;
  memcpy(ms, c->sky_table_timings, sizeof c->sky_table_timings);
  return ATMRT_OK;
}
