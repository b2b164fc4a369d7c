// atmrt_host.hpp — header-only C++17 host mirror of the reference's generator interface above the C ABI
// (include/atmrt.h).  Names, argument meaning and error behaviour follow the Rust reference:
//
//   reference (Rust)                                           here (namespace atmrt_host)
//   ---------------------------------------------------------  -------------------------------------------
//   Terrain::from_folder(path) / get_elev   terrain/mod.rs:66-126   Terrain::from_folder / get_elev
//   Params (view, model, env, straight_rays, simulation_step,       Params
//           output, scene)                   params.rs:496-505
//   trait Generator { fn generate(&self) -> Vec<Vec<ResultPixel>> }  struct Generator { virtual generate() const }
//   FastGenerator::new(&params, &terrain, start)  fast.rs:102-108     FastGenerator(params, terrain)
//   RectilinearGenerator / InterpolatingRectilinearGenerator         same names
//   match params.output.generator  generator/mod.rs:72-78            make_generator(params, terrain)
//   ResultPixel / TracePoint / PixelColor  generators/mod.rs:13-80   same names
//   panic!/expect on bad input                                       throws std::runtime_error with the library's message
//
//   (one GPU in the reference's world)                               Terrain(std::vector<int> devices): the same frame cut into
//                                                                    pixel-column tiles over several GPUs, inside the library
//
// Link with -latmrt.  There is no CPU path: constructing a Terrain without a gfx950 device throws.
#pragma once

#include <array>
#include <cmath>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "atmrt.h"

namespace atmrt_host {

struct Error : std::runtime_error {
  int status;
  Error(int s, const std::string& m) : std::runtime_error(m), status(s) {}
};

struct Altitude { // params.rs:17-21
  enum Kind { Absolute = ATMRT_ALT_ABSOLUTE, Relative = ATMRT_ALT_RELATIVE } kind = Relative;
  double value = 1.0;
};
struct Position { // params.rs:32-40
  double latitude = 0.0, longitude = 0.0;
  Altitude altitude;
};
struct Frame { // params.rs:145-155
  double direction = 0.0, tilt = 0.0, fov = 30.0, max_distance = 150000.0;
};
struct EarthModel { // earth_model/mod.rs:18-28
  atmrt_earth_model_t pod{ATMRT_EARTH_SPHERICAL, 0, 6371000.0, 0.0, 0.0};
  static EarthModel SimpleSphere() { return make(ATMRT_EARTH_SIMPLE_SPHERE); }
  static EarthModel Spherical(double radius) { EarthModel m = make(ATMRT_EARTH_SPHERICAL); m.pod.radius = radius; return m; }
  static EarthModel Ellipsoid(double a, double b) { EarthModel m = make(ATMRT_EARTH_ELLIPSOID); m.pod.a = a; m.pod.b = b; return m; }
  static EarthModel Wgs84() { return make(ATMRT_EARTH_WGS84); }
  static EarthModel AzimuthalEquidistant() { return make(ATMRT_EARTH_AZIMUTHAL_EQUIDISTANT); }
  static EarthModel FlatDistorted() { return make(ATMRT_EARTH_FLAT_DISTORTED); }
  static EarthModel ObserverAe(double proj_radius) { EarthModel m = make(ATMRT_EARTH_OBSERVER_AE); m.pod.radius = proj_radius; return m; }
  static EarthModel SimpleObserverAe() { return make(ATMRT_EARTH_SIMPLE_OBSERVER_AE); }
 private:
  static EarthModel make(int kind) { EarthModel m; m.pod = atmrt_earth_model_t{kind, 0, 0.0, 0.0, 0.0}; return m; }
};
enum class GeneratorDef { Fast = ATMRT_GEN_FAST, InterpolatingRectilinear = ATMRT_GEN_INTERPOLATING_RECTILINEAR, Rectilinear = ATMRT_GEN_RECTILINEAR };

struct Color { double r = 0, g = 0, b = 0, a = 1.0; }; // object/mod.rs:133-146
struct Object { // ConfObject after into_shape, object/mod.rs:42-75,156-161
  atmrt_object_t pod{};
  std::vector<uint8_t> texture; // RGBA8, top row first
  static Object Frustum(Position p, double r1, double r2, double height, Color c) {
    Object o; o.init(p); o.pod.kind = ATMRT_OBJ_FRUSTUM; o.pod.r1 = r1; o.pod.r2 = r2; o.pod.height = height;
    o.pod.color[0] = c.r; o.pod.color[1] = c.g; o.pod.color[2] = c.b; o.pod.color[3] = c.a; return o;
  }
  static Object Cylinder(Position p, double radius, double height, Color c) { return Frustum(p, radius, radius, height, c); }
  static Object Cone(Position p, double radius, double height, Color c) { return Frustum(p, radius, 0.0, height, c); }
  static Object Billboard(Position p, double width, double height, std::vector<uint8_t> rgba, uint32_t tex_w, uint32_t tex_h) {
    Object o; o.init(p); o.pod.kind = ATMRT_OBJ_BILLBOARD; o.pod.width = width; o.pod.height = height;
    o.texture = std::move(rgba); o.pod.texture_width = tex_w; o.pod.texture_height = tex_h; return o;
  }
 private:
  void init(Position p) { pod.position = atmrt_position_t{p.latitude, p.longitude, (int32_t)p.altitude.kind, 0, p.altitude.value}; }
};

struct Params { // params.rs:496-505 (the fields that reach the generators); defaults = Config::default :481-494
  Position position;
  Frame frame;
  EarthModel model;
  double wavelength = 530e-9;
  bool straight_rays = false;
  double simulation_step = 50.0;
  uint16_t width = 640, height = 480;
  GeneratorDef generator = GeneratorDef::Fast;
  double terrain_alpha = 1.0;
  std::vector<Object> objects;
  std::optional<atmrt_atmosphere_t> atmosphere; // None = AtmosphereDef::us_76(); the function table and spline points it points at
                                                // are the caller's and must outlive generate() (any number of either)
  uint16_t col_begin = 0, col_end = 0;          // pixel-column shard, 0/0 = whole image (leave 0/0 on a multi-device Terrain)

  atmrt_params_t pod(GeneratorDef gen) const {
    atmrt_params_t p{};
    p.position = atmrt_position_t{position.latitude, position.longitude, (int32_t)position.altitude.kind, 0, position.altitude.value};
    p.frame = atmrt_frame_t{frame.direction, frame.tilt, frame.fov, frame.max_distance};
    p.earth = model.pod;
    p.wavelength = wavelength;
    p.simulation_step = simulation_step;
    p.terrain_alpha = terrain_alpha;
    p.straight_rays = straight_rays ? 1 : 0;
    p.generator = (int32_t)gen;
    p.width = width;
    p.height = height;
    p.col_begin = col_begin;
    p.col_end = col_end;
    return p;
  }
};

// Terrain, terrain/mod.rs:55-57.  Owns the device context the tiles live in — one GPU, or several: with a device list the
// library cuts every frame into pixel-column tiles (one per device, one host thread each, the mosaic in every device's HBM) and
// generate() still returns the whole Vec<Vec<ResultPixel>>; nothing else in the host code changes.
class Terrain {
 public:
  explicit Terrain(int device = 0) {
    atmrt_ctx* c = nullptr;
    int rc = atmrt_ctx_create(&c, device);
    if (rc) throw Error(rc, atmrt_last_error(nullptr));
    ctx_.reset(c, atmrt_ctx_destroy);
  }
  explicit Terrain(const std::vector<int>& devices) {
    atmrt_ctx* c = nullptr;
    std::vector<int32_t> d(devices.begin(), devices.end());
    int rc = atmrt_ctx_create_multi(&c, d.data(), (int32_t)d.size());
    if (rc) throw Error(rc, atmrt_last_error(nullptr));
    ctx_.reset(c, atmrt_ctx_destroy);
  }
  static Terrain from_folder(const std::string& terrain_folder, int device = 0) { return Terrain(device).load(terrain_folder); }
  static Terrain from_folder(const std::string& terrain_folder, const std::vector<int>& devices) { return Terrain(devices).load(terrain_folder); }
  int devices() const { return atmrt_ctx_device_count(ctx()); }
  void add_tile(int lat0, int lon0, int n_lat, int n_lon, const int16_t* posts) { check(atmrt_terrain_add_tile(ctx(), lat0, lon0, n_lat, n_lon, posts)); }
  std::optional<double> get_elev(double latitude, double longitude) const {
    double e = 0.0;
    uint8_t ok = 0;
    check(atmrt_terrain_get_elev(ctx(), 1, &latitude, &longitude, &e, &ok));
    return ok ? std::optional<double>(e) : std::nullopt;
  }
  int files() const { return files_; }
  atmrt_ctx* ctx() const { return ctx_.get(); }
  Terrain& load(const std::string& terrain_folder) {
    int32_t n = 0;
    check(atmrt_terrain_load_dir(ctx(), terrain_folder.c_str(), &n));
    files_ = n;
    return *this;
  }
  void check(int rc) const { if (rc) throw Error(rc, atmrt_last_error(ctx())); }
 private:
  std::shared_ptr<atmrt_ctx> ctx_;
  int files_ = 0;
};

struct PixelColor { // generators/mod.rs:45-49
  bool terrain = true;
  Color rgba;        // Terrain(alpha): rgba.a = alpha
  double alpha() const { return rgba.a; }
};
struct TracePoint { // generators/mod.rs:21-30
  double lat, lon, distance, elevation, path_length;
  std::array<double, 3> normal;
  PixelColor color;
};
struct ResultPixel { // generators/mod.rs:13-19
  double elevation_angle, azimuth;
  std::vector<TracePoint> trace_points;
};

struct Generator { // generators/mod.rs:82-84
  virtual ~Generator() = default;
  virtual std::vector<std::vector<ResultPixel>> generate() const = 0;
  uint64_t last_ray_steps = 0;
};

class HipGenerator : public Generator {
 public:
  HipGenerator(const Params& params, const Terrain& terrain, GeneratorDef kind) : params_(params), terrain_(terrain), kind_(kind) {}
  std::vector<std::vector<ResultPixel>> generate() const override {
    atmrt_params_t pod = params_.pod(kind_);
    terrain_.check(atmrt_set_params(terrain_.ctx(), &pod));
    atmrt_atmosphere_t atm;
    if (params_.atmosphere) atm = *params_.atmosphere; else atmrt_atmosphere_us76(&atm);
    terrain_.check(atmrt_set_atmosphere(terrain_.ctx(), &atm));
    std::vector<atmrt_object_t> objs;
    for (const Object& o : params_.objects) {
      atmrt_object_t p = o.pod;
      p.texture_rgba = o.texture.empty() ? nullptr : o.texture.data();
      objs.push_back(p);
    }
    terrain_.check(atmrt_objects_set(terrain_.ctx(), objs.data(), objs.size()));
    atmrt_result_t r{};
    terrain_.check(atmrt_generate(terrain_.ctx(), &r));
    std::vector<std::vector<ResultPixel>> out(r.height);
    for (uint32_t y = 0; y < r.height; y++) {
      out[y].resize(r.width);
      for (uint32_t x = 0; x < r.width; x++) {
        size_t p = (size_t)y * r.width + x;
        ResultPixel& px = out[y][x];
        px.elevation_angle = r.elevation_angle[p];
        px.azimuth = r.azimuth[p];
        for (uint64_t k = r.hit_offset[p]; k < r.hit_offset[p] + r.hit_count[p]; k++) {
          TracePoint tp{r.lat[k], r.lon[k], r.distance[k], r.elevation[k], r.path_length[k],
                        {r.normal[3 * k], r.normal[3 * k + 1], r.normal[3 * k + 2]}, {}};
          tp.color.terrain = r.color_tag[k] == ATMRT_COLOR_TERRAIN;
          tp.color.rgba = Color{r.rgba[4 * k], r.rgba[4 * k + 1], r.rgba[4 * k + 2], r.rgba[4 * k + 3]};
          px.trace_points.push_back(tp);
        }
      }
    }
    const_cast<HipGenerator*>(this)->last_ray_steps = r.ray_steps;
    atmrt_result_free(&r);
    return out;
  }
 private:
  const Params& params_;
  const Terrain& terrain_;
  GeneratorDef kind_;
};

struct FastGenerator : HipGenerator { // fast.rs:102-108
  FastGenerator(const Params& p, const Terrain& t) : HipGenerator(p, t, GeneratorDef::Fast) {}
};
struct RectilinearGenerator : HipGenerator { // rectilinear.rs:70-76
  RectilinearGenerator(const Params& p, const Terrain& t) : HipGenerator(p, t, GeneratorDef::Rectilinear) {}
};
struct InterpolatingRectilinearGenerator : HipGenerator { // interpolating_rectilinear.rs:421-427
  InterpolatingRectilinearGenerator(const Params& p, const Terrain& t) : HipGenerator(p, t, GeneratorDef::InterpolatingRectilinear) {}
};

// generator::generate's `match params.output.generator` (src/generator/mod.rs:72-78)
inline std::unique_ptr<Generator> make_generator(const Params& params, const Terrain& terrain) {
  switch (params.generator) {
    case GeneratorDef::Fast: return std::make_unique<FastGenerator>(params, terrain);
    case GeneratorDef::InterpolatingRectilinear: return std::make_unique<InterpolatingRectilinearGenerator>(params, terrain);
    default: return std::make_unique<RectilinearGenerator>(params, terrain);
  }
}

// Output's annotations (params.rs:403-410): ticks, vertical_ticks, show_eye_level, show_flat_horizon.
struct Tick { // Tick / VerticalTick, params.rs:325-368
  atmrt_tick_t pod{};
  static Tick Single(double angle, uint32_t size, bool labelled) { return Tick{atmrt_tick_t{ATMRT_TICK_SINGLE, size, angle, 0.0, 0.0, labelled ? 1 : 0, 0}}; }
  static Tick Multiple(double bias, double step, uint32_t size, bool labelled) { return Tick{atmrt_tick_t{ATMRT_TICK_MULTIPLE, size, 0.0, bias, step, labelled ? 1 : 0, 0}}; }
};
struct Overlay {
  std::vector<Tick> ticks, vertical_ticks;
  bool show_eye_level = false, show_flat_horizon = false;
};
struct DrawnOverlay {
  std::vector<atmrt_drawn_tick_t> ticks; // with the label strings for the host's text renderer, sorted by (vertical, pos)
  double flat_horizon_deg;               // NaN when the flat-horizon line is not drawn
};
// renderer::output_image's draw_ticks / draw_const_elev (renderer/mod.rs:419-431) for the frame the last generate() on `terrain`
// produced, over rgb = [height][width][3] (e.g. of atmrt_draw_image); the labels' text is left to the host.
inline DrawnOverlay draw_overlay(const Terrain& terrain, const Overlay& overlay, uint8_t* rgb, uint32_t width, uint32_t height) {
  std::vector<atmrt_tick_t> h, v;
  for (const Tick& t : overlay.ticks) h.push_back(t.pod);
  for (const Tick& t : overlay.vertical_ticks) v.push_back(t.pod);
  atmrt_overlay_t pod{h.data(), v.data(), (uint32_t)h.size(), (uint32_t)v.size(), overlay.show_eye_level ? 1 : 0, overlay.show_flat_horizon ? 1 : 0};
  DrawnOverlay out;
  out.ticks.resize((h.empty() ? 0 : width) + (v.empty() ? 0 : height) + 1); // at most one tick per pixel position
  size_t n = 0;
  terrain.check(atmrt_draw_overlay(terrain.ctx(), &pod, rgb, out.ticks.data(), out.ticks.size(), &n, &out.flat_horizon_deg));
  out.ticks.resize(n);
  return out;
}

// The visibility map of the frame the last generate() on `terrain` produced (no reference counterpart): its trace points — the first
// of every pixel, or all of them — binned over `grid`.  count and min_distance are [n_lat][n_lon], rows south to north;
// min_distance is +inf where count is 0.
struct VisibilityMap {
  std::vector<uint32_t> count;
  std::vector<double> min_distance;
  atmrt_visibility_stats_t stats;
};
inline VisibilityMap visibility_map(const Terrain& terrain, const atmrt_geo_grid_t& grid, atmrt_visibility_mode mode = ATMRT_VIS_FIRST) {
  VisibilityMap out;
  const size_t n = (size_t)grid.n_lat * grid.n_lon;
  out.count.resize(n);
  out.min_distance.resize(n);
  terrain.check(atmrt_visibility_map(terrain.ctx(), &grid, mode, out.count.data(), out.min_distance.data(), &out.stats));
  return out;
}
// lat_min, lat_max, lon_min, lon_max of those trace points: the natural extent of a grid; all NaN for a frame of sky.
inline std::array<double, 4> frame_bounds(const Terrain& terrain, atmrt_visibility_mode mode = ATMRT_VIS_FIRST) {
  std::array<double, 4> out{};
  terrain.check(atmrt_frame_bounds(terrain.ctx(), mode, out.data()));
  return out;
}

// Landmarks located in the frame the last generate() on `terrain` produced (no reference counterpart; it inverts the `view` window's
// click, viewer/app.rs:112-176): per landmark the number of trace points within radius_deg and the nearest of them, n_within == 0
// when there is none — which does not say whether the landmark is outside the field of view or hidden behind terrain.
inline atmrt_landmark_t landmark(double lat, double lon) { return atmrt_landmark_t{lat, lon, std::cos(lat * 3.14159265358979323846 / 180.0)}; }
struct LocatedLandmarks {
  std::vector<atmrt_landmark_hit_t> hits;
  atmrt_landmark_stats_t stats;
};
inline LocatedLandmarks locate_landmarks(const Terrain& terrain, const std::vector<atmrt_landmark_t>& landmarks, double radius_deg,
                                         atmrt_visibility_mode mode = ATMRT_VIS_FIRST) {
  LocatedLandmarks out;
  out.hits.resize(landmarks.size());
  terrain.check(atmrt_locate_landmarks(terrain.ctx(), landmarks.data(), landmarks.size(), radius_deg, mode, out.hits.data(), &out.stats));
  return out;
}

// Sight lines (no reference counterpart; include/atmrt.h states the rule): for every target {azimuth_deg, distance, height} the
// elevation angle at which the point `height` metres above the ground there appears from the observer set on `terrain`'s context, or
// how much of it terrain hides and where that terrain is.  Needs parameters (a generator's configure or generate) and no frame.
inline std::vector<atmrt_sight_t> sight_lines(const Terrain& terrain, const std::vector<atmrt_sight_target_t>& targets, double fan_lo_deg = -5.0,
                                              double fan_hi_deg = 5.0, int32_t rounds = 3) {
  std::vector<atmrt_sight_t> out(targets.size());
  terrain.check(atmrt_sight_lines(terrain.ctx(), targets.data(), targets.size(), fan_lo_deg, fan_hi_deg, rounds, out.data()));
  return out;
}

// Viewshed (no reference counterpart; include/atmrt.h states the rule): the first round of the sight-line rule at every cell of the
// polar lattice spec describes, from the observer set on `terrain`'s context.  Planes are [n_az][m], cell (j, i) at j * m + (i - 1).
struct Viewshed {
  int32_t n_az = 0, m = 0;
  std::vector<uint16_t> k_star;
  std::vector<uint8_t> status;
  std::vector<double> hidden, ground, lat, lon;
  std::vector<int32_t> block_index;
};
inline Viewshed viewshed(const Terrain& terrain, const atmrt_viewshed_spec_t& spec) {
  Viewshed out;
  terrain.check(atmrt_viewshed_steps(terrain.ctx(), spec.reach, &out.m));
  out.n_az = spec.n_az;
  const size_t cells = (size_t)(spec.n_az > 0 ? spec.n_az : 0) * (size_t)out.m;
  out.k_star.resize(cells), out.status.resize(cells), out.hidden.resize(cells), out.block_index.resize(cells);
  out.ground.resize(cells), out.lat.resize(cells), out.lon.resize(cells);
  terrain.check(atmrt_viewshed(terrain.ctx(), &spec, out.k_star.data(), out.status.data(), out.hidden.data(), out.block_index.data(),
                               out.ground.data(), out.lat.data(), out.lon.data()));
  return out;
}

// Viewshed map (no reference counterpart; include/atmrt.h states the rule): that viewshed binned over `grid` on the device, its planes
// never downloaded.  n_samples, n_seen and min_hidden are [n_lat][n_lon], rows south to north; min_hidden is +inf where no sample
// takes part.  `into`: a map on the same grid to add to (counts are added, the minimum is taken against what is there).
struct ViewshedMap {
  std::vector<uint32_t> n_samples, n_seen;
  std::vector<double> min_hidden;
  atmrt_viewshed_map_stats_t stats{};
};
inline ViewshedMap viewshed_map(const Terrain& terrain, const atmrt_viewshed_spec_t& spec, const atmrt_geo_grid_t& grid, const ViewshedMap* into = nullptr) {
  ViewshedMap out;
  if (into) out = *into;
  const size_t n = (size_t)grid.n_lat * grid.n_lon;
  out.n_samples.resize(n), out.n_seen.resize(n), out.min_hidden.resize(n);
  terrain.check(atmrt_viewshed_map(terrain.ctx(), &spec, &grid, into ? 1 : 0, out.n_samples.data(), out.n_seen.data(), out.min_hidden.data(), &out.stats));
  return out;
}

// Horizon (no reference counterpart; include/atmrt.h states the rule): for every azimuth of spec the bracket of elevation angles
// between the highest ray that terrain within spec.reach stops and the ray above it, and the ridge that stops it, from the observer
// set on `terrain`'s context.  One record per azimuth.
inline std::vector<atmrt_horizon_t> horizon(const Terrain& terrain, const atmrt_horizon_spec_t& spec) {
  std::vector<atmrt_horizon_t> out((size_t)(spec.n_az > 0 ? spec.n_az : 0));
  terrain.check(atmrt_horizon(terrain.ctx(), &spec, out.data()));
  return out;
}

// Cast shadows (no reference counterpart; include/atmrt.h states the rule): for the first trace point of every pixel of the frame
// last generated on `terrain`'s context, whether a ray toward the light (spec: azimuth toward it, launch elevation, reach, lift)
// clears the terrain.  status (atmrt_shadow_status) and block are [height][width].
struct ShadowMask {
  std::vector<uint8_t> status;
  std::vector<uint16_t> block;
  atmrt_shadow_stats_t stats{};
};
inline ShadowMask shadow_mask(const Terrain& terrain, const atmrt_shadow_spec_t& spec, uint32_t width, uint32_t height) {
  ShadowMask out;
  out.status.resize((size_t)width * height), out.block.resize((size_t)width * height);
  terrain.check(atmrt_shadow_mask(terrain.ctx(), &spec, out.status.data(), out.block.data(), &out.stats));
  return out;
}
// renderer::draw_image of that frame, RGB8 [height][width][3], the first trace point of a SHADOWED pixel at the Shading method's ambient light
inline std::vector<uint8_t> draw_image_shadowed(const Terrain& terrain, const atmrt_coloring_t& coloring, const ShadowMask& mask, uint32_t width,
                                                uint32_t height) {
  if (mask.status.size() != (size_t)width * height) throw Error(ATMRT_ERR_INVALID_ARGUMENT, "the shadow mask is not the image's size");
  std::vector<uint8_t> rgb(3 * (size_t)width * height);
  terrain.check(atmrt_draw_image_shadowed(terrain.ctx(), &coloring, mask.status.data(), rgb.data()));
  return rgb;
}

// Shadow lights (include/atmrt.h, "shadow lights"): the same march toward each of up to 64 lights given as world-frame vectors, every
// point in the light's own local direction.  lit_mask [height][width]: bit l set where light l reaches the first trace point;
// status and block [n_lights][height][width] when asked for.
struct ShadowLights {
  std::vector<uint64_t> lit_mask;
  std::vector<uint8_t> status;
  std::vector<uint16_t> block;
  atmrt_shadow_stats_t stats{};
};
// a light seen from (lat, lon) under (azimuth_deg, elevation_deg) -> its world-frame vector (host code, no device)
inline std::array<double, 3> shadow_light_direction(const atmrt_earth_model_t& earth, double lat, double lon, double azimuth_deg, double elevation_deg) {
  std::array<double, 3> dir{};
  if (int rc = atmrt_shadow_light_direction(&earth, lat, lon, azimuth_deg, elevation_deg, dir.data())) throw Error(rc, "atmrt_shadow_light_direction refused its arguments");
  return dir;
}
// (azimuth_deg, elevation_deg) of a world-frame light in the local frame of (lat, lon): the function the kernel runs (host code, no device)
inline std::pair<double, double> shadow_local_direction(const atmrt_earth_model_t& earth, const std::array<double, 3>& dir, double lat, double lon) {
  std::pair<double, double> out{};
  if (int rc = atmrt_shadow_local_direction(&earth, dir.data(), lat, lon, &out.first, &out.second)) throw Error(rc, "atmrt_shadow_local_direction refused its arguments");
  return out;
}
inline ShadowLights shadow_lights(const Terrain& terrain, const std::vector<std::array<double, 3>>& dirs, double reach, double lift, uint32_t width,
                                  uint32_t height, bool status = false, bool block = false) {
  ShadowLights out;
  const size_t n = (size_t)width * height;
  out.lit_mask.resize(n);
  if (status) out.status.resize(n * dirs.size());
  if (block) out.block.resize(n * dirs.size());
  const atmrt_shadow_lights_spec_t spec{dirs.empty() ? nullptr : dirs[0].data(), (uint32_t)dirs.size(), 0, reach, lift};
  terrain.check(atmrt_shadow_lights(terrain.ctx(), &spec, out.lit_mask.data(), status ? out.status.data() : nullptr, block ? out.block.data() : nullptr, &out.stats));
  return out;
}

} // namespace atmrt_host
