// atmrt_ctx.h — internal: the context behind the C ABI (include/atmrt.h), shared by the translation units that implement it:
// atmrt_api.hip (one device: terrain store, frame set-up, launch sequences), atmrt_consumers.hip (the calls that read a finished
// frame: image, overlay, visibility map, landmarks, cast shadows), atmrt_polar.hip (the calls along azimuths from the observer: sight
// lines, viewshed, viewshed map, horizon), atmrt_probes.hip (the harness and debug probes) and atmrt_multi.hip (several devices:
// column tiles, the RCCL all-gather, image assembly).
#pragma once

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "atmrt_cached.h"
#include "atmrt_kernels.h"

namespace atmrt {

struct HostTile {
  int n_lat = 0, n_lon = 0;
  std::vector<int16_t> posts; // [n_lat][n_lon]
};
// Terrain (terrain/mod.rs:55-57): tiles keyed by integer degrees.  One store may serve several contexts (the sub-contexts of a
// multi-device context upload the same mosaic to their own HBM): `generation` tells a context that its copy is stale.
struct TileStore {
  std::map<std::pair<int, int>, HostTile> tiles;
  uint64_t generation = 1;
};

// grow-only device buffer
struct DevBuf {
  void* ptr = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    cap = 0;
    size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&ptr, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const { return static_cast<T*>(ptr); }
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : ptr(o.ptr), cap(o.cap) { o.ptr = nullptr, o.cap = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept { // std::swap of two buffers (run_interpolating keeps the lattice result that way)
    if (this != &o) {
      release();
      ptr = o.ptr, cap = o.cap;
      o.ptr = nullptr, o.cap = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); } // atmrt_ctx_destroy makes the context's device current before the context (and its buffers) goes
};
// `buf` grown to n elements and `field` pointed at it in one statement: a reservation and its pointer cannot drift apart
template <class T>
hipError_t reserve_into(DevBuf& buf, T*& field, size_t n) {
  const hipError_t e = buf.reserve(n * sizeof(T));
  field = buf.as<T>();
  return e;
}

// An owning copy of an atmrt_atmosphere_t (the ABI struct borrows its function table and spline points from the caller).
struct AtmDef {
  atmrt_atmosphere_t pod{};
  std::vector<atmrt_temp_function_t> functions;
  std::vector<std::vector<double>> xs, ys;
  void assign(const atmrt_atmosphere_t& a) {
    pod = a;
    functions.assign(a.functions, a.functions + a.n_functions);
    xs.assign(functions.size(), {});
    ys.assign(functions.size(), {});
    for (size_t j = 0; j < functions.size(); j++) {
      atmrt_temp_function_t& fn = functions[j];
      if (fn.kind == ATMRT_TEMP_SPLINE && fn.n_points > 0 && fn.point_altitude && fn.point_temperature) {
        xs[j].assign(fn.point_altitude, fn.point_altitude + fn.n_points);
        ys[j].assign(fn.point_temperature, fn.point_temperature + fn.n_points);
        fn.point_altitude = xs[j].data();
        fn.point_temperature = ys[j].data();
      } else {
        fn.point_altitude = fn.point_temperature = nullptr;
      }
    }
    pod.functions = functions.data();
  }
  AtmDef() = default;
  AtmDef(const AtmDef&) = delete;
  AtmDef& operator=(const AtmDef&) = delete;
};

// ---- what a context builds from a frame's inputs and keeps across frames: one rule, atmrt_cached.h (the table: DESIGN.md §3) ----
// A key is the tuple of a product's inputs in the order of its comment: doubles as their bits(), a source product as its serial().
using StepsKey = std::tuple<uint64_t, uint64_t>;                                    // simulation_step, max_distance
using TrigKey = std::tuple<uint64_t, uint64_t, int32_t>;                            // steps, calc_radius, EARTH_FAST_DIV
using NormalTrigKey = std::tuple<uint64_t, int32_t, uint64_t, uint64_t>;                // calc_radius, EARTH_FAST_DIV, observer's latitude, longitude
using AtmKey = std::tuple<uint64_t, uint64_t, uint64_t, uint64_t, int32_t>;         // atm_def_serial, wavelength, step, shape_radius, spherical
using EscapeKey = std::tuple<uint64_t, uint64_t>;                                   // atm, the mosaic's top
using BinsKey = std::tuple<uint64_t, uint64_t, uint64_t, int32_t, int32_t, int32_t, int32_t>; // direction, fov, tilt, width, height, column shard
using EarthKey = std::tuple<int32_t, int32_t, int32_t, int32_t, uint64_t, uint64_t, uint64_t, uint64_t, uint64_t>;
using LayoutKey = std::tuple<uint64_t, uint64_t, uint64_t, uint64_t, int32_t>;
using CeilKey = std::tuple<uint64_t, uint64_t, uint64_t, uint64_t, EarthKey, LayoutKey, int32_t>; // terrain_uploaded, steps, latitude, longitude (no altitude), earth, bins, trig table in use
// atm, terrain_uploaded, altitude_kind, latitude, longitude, altitude (what the observer's altitude is resolved from), fan lo, hi,
// simulation_step, K, m, straight_rays, earth
using ViewshedKey = std::tuple<uint64_t, uint64_t, int32_t, uint64_t, uint64_t, uint64_t, uint64_t, uint64_t, uint64_t, int32_t, int32_t, int32_t, EarthKey>;
using OrderKey = std::tuple<uint64_t, uint64_t, int32_t, int32_t, uint64_t>;        // ceiling, bins, image rows, altitude_kind, altitude
// atm (atmosphere, wavelength), straight_rays, spherical, shape_radius, then the table spec with its step resolved: step, top, floor,
// m, alt_lo, alt_hi, el_lo, el_hi, n_alt, n_el
using SkyTableKey = std::tuple<uint64_t, int32_t, int32_t, uint64_t, uint64_t, uint64_t, uint64_t, int32_t, uint64_t, uint64_t, uint64_t, uint64_t, uint32_t, uint32_t>;
inline EarthKey key_of(const Earth& e) {
  return {e.calc, e.flat_dirs, e.cart, e.spherical, bits(e.calc_radius), bits(e.cart_radius), bits(e.a), bits(e.b), bits(e.shape_radius)};
}
inline LayoutKey key_of(const CeilLayout& l) { return {bits(l.dir0), bits(l.rel_lo), bits(l.w), bits(l.inv_w), l.n_bins}; }
struct Steps {
  std::vector<double> xs;
  int n_t = 0, n_path_cap = 0, march_steps = 0; // march_steps = #{k >= 1 : xs[k] <= max_distance}: the steps of a ray that marches to the end
};
struct Atm {
  AtmTableBuf table;
  double ceil_from = 0.0; // the escape certificate's lowest altitude for the lowest value a ceiling entry can have (1 m) minus a step
};
struct Escape { // the certificate from the mosaic's top minus a step up: the lowest altitude from which it holds, the largest bound above that
  double from = 0.0, bound = 0.0;
};

struct SkyTableInfo { // beside the refraction table in d_sky_table: what the host keeps of it
  atmrt_sky_stats_t stats{};  // of the march that built it
  std::vector<uint32_t> tail; // [n_alt]
  int64_t first_unusable = -1; // the first row with tail > n_el - 2, or -1
};

// The last generated frame, for the calls that read it: run_generator (atmrt_api.hip) resets `valid`, `ceil_rows` and `march_route`
// when a frame starts and fills the rest when it has succeeded; a frame that fails leaves the rest as the frame before left it.
struct LastFrame {
  bool valid = false, packed = false; // packed: the frame has trace-point lists (hits, offset, nhits) beside its planes
  size_t npx = 0;
  int wl = 0, h = 0, c0 = 0;
  double alpha = 1.0;
  atmrt_params_t params{}; // the parameters that frame was generated with (atmrt_draw_overlay*)
  DensePlanes dense{};
  PackedHits hits{};
  const uint64_t* offset = nullptr;
  uint64_t nhits = 0;
  uint64_t ray_steps = 0, escaped_steps = 0, escaped_rays = 0; // atmrt_last_march_work
  // atmrt_debug_ceiling_table: the ceiling table that frame marched with — its rows (0: none), its bins and the build of
  // `ceiling` (its serial) that filled d_ceil then; a later build overwrites the buffer
  int32_t ceil_rows = 0;
  CeilLayout ceil_layout{};
  uint64_t ceil_serial = 0;
  // atmrt_debug_march_order: the work queue that frame marched with — its groups (0: none) and the build of `ceil_order` that filled it
  uint32_t order_groups = 0;
  uint64_t order_serial = 0;
  // atmrt_debug_last_march_route: the route that frame's first-pass march was launched by (None: not a Rectilinear frame)
  MarchRoute march_route = MarchRoute::None;

  // The trace points a mode reads.  ATMRT_VIS_ALL reads the packed lists where the frame has them; a frame without lists holds one
  // point per pixel at most, in its planes, and ALL is FIRST.
  TracePoints points(int32_t mode) const {
    if (mode == ATMRT_VIS_ALL && packed) return TracePoints{npx, (uint32_t)wl, dense.hit_count, offset, hits.lat, hits.lon, hits.distance, hits.elevation};
    return TracePoints{npx, (uint32_t)wl, dense.hit_count, nullptr, dense.lat, dense.lon, dense.distance, dense.elevation};
  }
};

// An environment switch that only "off" turns off.  When it is read is its caller's business: the named one-liners say.
inline bool env_off(const char* name) {
  const char* e = getenv(name);
  return e && !strcmp(e, "off");
}

// ms[i] = (add ? ms[i] : 0) + the milliseconds from ev[i] to ev[i + 1], for the n intervals of n + 1 recorded events
inline hipError_t event_intervals(const hipEvent_t* ev, int n, double* ms, bool add = false) {
  for (int i = 0; i < n; i++) {
    float v = 0.0f;
    const hipError_t e = hipEventElapsedTime(&v, ev[i], ev[i + 1]);
    if (e != hipSuccess) return e;
    ms[i] = (add ? ms[i] : 0.0) + v;
  }
  return hipSuccess;
}

struct MultiGroup; // atmrt_multi.hip: the devices of a multi-device context and their worker threads
struct Comm;       // atmrt_multi.hip: this context's place among the ranks that share one frame

} // namespace atmrt

struct atmrt_ctx {
  int device = 0;
  hipStream_t stream = nullptr, stream2 = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_t0 = nullptr, ev_t1 = nullptr;
  hipEvent_t ev[atmrt::EV_COUNT] = {};         // the phases of a frame (PhaseEvent, atmrt_kernels.h)
  hipEvent_t ev_seg[atmrt::FAST_SEGMENTS] = {}; // a path segment is integrated (stream2) -> its intersect scan may start
  hipEvent_t ev_scan[2 * atmrt::FAST_SEGMENTS] = {}; // begin / end of every scan segment (after its wait), for intersect_ms
  int scan_segments = 0;                       // segments of the last pipelined frame (0: EV_MARCH_BEGIN .. EV_MARCH_END time the scan)
  atmrt_timings_t timings{};
  atmrt_frame_stats_t stats{};
  bool inject_failure = false; // atmrt_debug_fail_next_frame
  std::string error;

  std::shared_ptr<atmrt::TileStore> terrain = std::make_shared<atmrt::TileStore>();
  uint64_t terrain_uploaded = 0; // generation of the mosaic in d_posts (0: none)
  atmrt::DevBuf d_posts, d_tiles, d_cells; // the mosaic: survives the frame, uploaded when the store's generation changes
  atmrt::TerrainView tv{};

  bool have_params = false;
  atmrt_params_t params{};       // as the caller set them (a rank of a shared frame: the WHOLE image; its columns are in `comm`)
  atmrt::AtmDef atm_def;
  std::vector<uint8_t> atm_def_bytes; // the definition as it was last set, byte for byte (atmrt_set_atmosphere)
  uint64_t atm_def_serial = 0;        // counts its changes
  atmrt::Earth earth{};
  atmrt::Cached<atmrt::AtmKey, atmrt::Atm> atm;          // the compiled, certified table (prepare_frame)
  atmrt::Cached<atmrt::EscapeKey, atmrt::Escape> escape; // its certificate above the mosaic's top (Frame::esc_floor)
  atmrt::Cached<atmrt::BinsKey, atmrt::CeilLayout> bins; // the ceiling table's bins (prepare_ceiling)
  bool ceil_built = false; // this frame built the ceiling table: EV_CEIL_BEGIN .. EV_CEIL_END hold its time

  atmrt::LastFrame last; // the last generated frame (run_generator)

  std::vector<atmrt::ObjectDev> objects; // host image of the device table (altitude kind in _pad until k_resolve)
  std::vector<uint8_t> textures;         // RGBA8 pool
  uint64_t objects_serial = 0;           // counts atmrt_objects_set

  // several devices / ranks (atmrt_multi.hip); both null for a plain one-device context
  atmrt::MultiGroup* multi = nullptr; // this is the PARENT of a multi-device context: every entry point forwards to its children
  atmrt::Comm* comm = nullptr;        // this context computes one column tile of a frame shared with other ranks

  // Device memory.  The scratch of a frame is ONE allocation, d_workspace, carved by workspace_layout (atmrt_kernels.h) and re-carved
  // by every prepare_workspace.  A buffer of its own needs a reason:
  // ... it survives the frame
  atmrt::DevBuf d_xs, d_atm;               // the distance table (`steps`) and the compiled atmosphere (`atm`)
  atmrt::Cached<atmrt::StepsKey, atmrt::Steps> steps;
  atmrt::DevBuf d_xs_trig;                 // Spherical calculator: sin, then cos, of xs[0 .. march_steps] / calc_radius (k_step_trig)
  atmrt::Cached<atmrt::TrigKey> trig;
  atmrt::DevBuf d_normal_trig;             // Spherical calculator: the record of the trace-point epilogue's frame constants (NormalTrig, k_normal_trig)
  atmrt::Cached<atmrt::NormalTrigKey> normal_trig;
  atmrt::DevBuf d_ceil;                    // Spherical calculator, Rectilinear: the terrain ceiling table (atmrt_ceiling.h), (march_steps + 1) x (bins + 1) entries
  atmrt::Cached<atmrt::CeilKey> ceiling;
  atmrt::DevBuf d_ceil_order;              // beside it: the work queue of the whole-frame march (Frame::ceil_order) and its sort's scratch (march_order_layout)
  atmrt::Cached<atmrt::OrderKey> ceil_order;
  atmrt::DevBuf d_alt;                     // the observer's altitude (k_resolve): atmrt_draw_overlay* samples the atmosphere there
  atmrt::DevBuf d_objects, d_textures;     // the scene: the object table is uploaded every frame, the textures when objects_serial changes
  atmrt::Cached<uint64_t> textures_dev;
  atmrt::DevBuf d_dense, d_packed, d_hit_offset; // the last frame's results (last.dense, last.hits, last.offset): draw, overlay, hits
  atmrt::DevBuf d_io, d_overlay;           // staging of the entry points that run between frames
  atmrt::DevBuf d_vis;                     // atmrt_visibility_map* / atmrt_frame_bounds: the call's statistics block (72 B), read while the last frame's buffers are live
  atmrt::DevBuf d_landmarks;               // atmrt_locate_landmarks*: the call's index, per-landmark state and records, sized by the call's landmarks
  double lm_timings[5] = {};               // atmrt_last_landmark_timings
  atmrt::DevBuf d_sight;                   // atmrt_sight_lines / atmrt_sight_fan_probe: the call's distance table and one batch of targets, profiles and records
  double sight_timings[3] = {};            // atmrt_last_sight_timings
  int32_t sight_batches = 0;               // atmrt_last_sight_batches
  atmrt::DevBuf d_viewshed_paths;          // atmrt_viewshed*: the path table H[i][k] of the last fan, kept across calls
  atmrt::Cached<atmrt::ViewshedKey> viewshed_paths;
  double viewshed_timings[4] = {};         // atmrt_last_viewshed_timings
  int32_t viewshed_batches = 0, viewshed_rebuilt = 0; // atmrt_last_viewshed_work
  atmrt::DevBuf d_vsmap;                   // atmrt_viewshed_map*: the call's statistics block (40 B)
  double horizon_timings[5] = {};          // atmrt_last_horizon_timings
  int32_t horizon_batches = 0, horizon_rebuilt = 0;   // atmrt_last_horizon_work
  atmrt::DevBuf d_shadow;                  // atmrt_shadow_mask*: the call's list of hit pixels and its counters
  double shadow_timings[3] = {};           // atmrt_last_shadow_timings
  atmrt::DevBuf d_sky;                     // atmrt_sky_*: the call's list of sky pixels and its counters
  double sky_timings[3] = {};              // atmrt_last_sky_timings
  double sky_shade_ms = 0.0;               // atmrt_last_sky_shade_timing
  atmrt::DevBuf d_sky_table;               // "apparent elevation": T [n_alt][n_el] f64, then tail [n_alt] u32, then S [n_alt][n_el] u8, kept across calls
  atmrt::Cached<atmrt::SkyTableKey, atmrt::SkyTableInfo> sky_table;
  int32_t sky_table_rebuilt = 0;           // atmrt_last_sky_table_work
  double sky_table_timings[3] = {};
  // ... it survives the second prepare_workspace of an InterpolatingRectilinear frame (lattice frame, then the image frame again)
  atmrt::DevBuf d_counters;                // zeroed once per frame: the lattice pass and the blend count into the same block
  atmrt::DevBuf d_interp;                  // InterpBuffers: the ray table and the lattice keys, read by the blend
  atmrt::DevBuf d_px_steps;                // the lattice's ray-steps and its referenced flags, read by the blend
  atmrt::DevBuf d_lat_dense, d_lat_packed, d_lat_offset; // the lattice result (the last two trade places with d_packed / d_hit_offset)
  // ... it is sized by a count the host reads back in mid-frame, while the workspace is live and must not move
  atmrt::DevBuf d_clist;                   // CTR_CLOSE_TOTAL: the close lists of a Fast frame with objects
  atmrt::DevBuf d_hit_lists;               // CTR_HITS, CTR_OVERFLOW_PIXELS: the fill pass's lists, carved in run_core
  atmrt::DevBuf d_blend_arena;             // CTR_BIG_BLEND_POINTS: BlendArena
  atmrt::DevBuf d_workspace;

  int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    error = buf;
    return code;
  }
};

#define HIP_TRY(ctx, expr)                                                                               \
  do {                                                                                                   \
    hipError_t e_ = (expr);                                                                              \
    if (e_ != hipSuccess) return (ctx)->fail(ATMRT_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

namespace atmrt {
// implemented in atmrt_api.hip; called by atmrt_polar.hip (every call), atmrt_consumers.hip (shadow_call) and atmrt_probes.hip
// (harness_frame): the context's cached frame inputs refreshed and handed out as a Frame
int prepare_frame(atmrt_ctx* c, Frame* out);
} // namespace atmrt
