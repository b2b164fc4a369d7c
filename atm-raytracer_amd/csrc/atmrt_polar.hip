// atmrt_polar.hip — the entry points of include/atmrt.h that march targets along azimuths from the observer: sight lines, viewshed,
// viewshed map and horizon.  They share one scratch buffer (d_sight), one plan of batches (atmrt_polar_plan.h) and one driver of
// those batches (polar_run); a call is its argument checks and a description of what it carves, launches and downloads per batch.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "atmrt_ctx.h"
#include "atmrt_polar_plan.h"
#include "atmrt_sight.h"
#include "atmrt_viewshed.h"
#include "atmrt_viewshed_map.h"
#include "atmrt_horizon.h"

using namespace atmrt;

// ---------------------------------------------------------------------------------------------
// sight lines (include/atmrt.h; kernels in atmrt_sight.h)
// ---------------------------------------------------------------------------------------------
extern "C" int atmrt_sight_fan_angles(double lo, double hi, double out[64]) {
  if (!out) return ATMRT_ERR_INVALID_ARGUMENT;
  const double delta = sight_fan_delta(lo, hi);
  for (int k = 0; k < SIGHT_FAN; k++) out[k] = sight_fan_angle(lo, delta, k);
  return ATMRT_OK;
}

extern "C" int atmrt_sight_pick(const uint8_t fails[64], int32_t* k_star) {
  if (!fails || !k_star) return ATMRT_ERR_INVALID_ARGUMENT;
  unsigned long long mask = 0;
  for (int k = 0; k < SIGHT_FAN; k++)
    if (fails[k]) mask |= 1ull << k;
  *k_star = sight_pick(mask);
  return ATMRT_OK;
}

namespace {

const char* sight_target_check(const atmrt_sight_target_t& t) {
  if (!std::isfinite(t.azimuth_deg)) return "a target's azimuth_deg is not finite";
  if (!(std::isfinite(t.distance) && t.distance > 0.0)) return "a target's distance must be finite and positive";
  if (!(std::isfinite(t.height) && t.height >= 0.0)) return "a target's height must be finite and not negative";
  return nullptr;
}

// What a call's targets must be, and *m_far: the samples to the farthest of them.  0 or a message.
const char* sight_steps(const atmrt_ctx* c, const atmrt_sight_target_t* targets, size_t n, int32_t* m_far) {
  const double step = c->params.simulation_step;
  if (!(step > 0.0)) return "simulation_step must be positive";
  double far = 0.0;
  for (size_t t = 0; t < n; t++) {
    if (const char* msg = sight_target_check(targets[t])) return msg;
    far = std::max(far, targets[t].distance);
  }
  const int32_t m = lattice_steps(step, far, SIGHT_M_MAX);
  if (m < 0) return "a target lies more than 65535 samples away";
  *m_far = m;
  return nullptr;
}

// The call's sample lattice on the host: d_i by repeated addition as far as the farthest target, and every target's m.
const char* sight_lattice(const atmrt_ctx* c, const atmrt_sight_target_t* targets, size_t n, std::vector<double>& dtab, std::vector<int32_t>& m) {
  int32_t m_far = 0;
  if (const char* msg = sight_steps(c, targets, n, &m_far)) return msg;
  dtab.assign(1, 0.0);
  for (int32_t i = 0; i < m_far; i++) dtab.push_back(dtab.back() + c->params.simulation_step);
  m.resize(n);
  for (size_t t = 0; t < n; t++) // the first index with d_m >= distance (the table ascends: step > 0)
    m[t] = (int32_t)(std::lower_bound(dtab.begin(), dtab.end(), targets[t].distance) - dtab.begin());
  return nullptr;
}

size_t sight_scratch_limit() { // read at call time: tests lower it to force several batches
  const char* e = getenv("ATMRT_SIGHT_SCRATCH_BYTES");
  const long long v = e ? atoll(e) : 0;
  return v > 0 && (size_t)v < SIGHT_SCRATCH_BYTES ? (size_t)v : SIGHT_SCRATCH_BYTES;
}

int sight_check_state(atmrt_ctx* c, const char* what) {
  if (c->multi) return c->fail(ATMRT_ERR_STATE, "%s solves on one device: a multi-device context has none of its own", what);
  if (!c->have_params) return c->fail(ATMRT_ERR_STATE, "%s: atmrt_set_params has not been called", what);
  return ATMRT_OK;
}

// ---- one batched call ------------------------------------------------------------------------------------------------------------------
// What a call hands the driver.  The driver records event ev0 before a batch's uploads, ev0 + 1 after its profiles and one more
// after every stage; ms[i] sums the interval from event ev0 + i to the next over the batches.
using PolarStage = std::function<int(const SightBatch& b, size_t t0, size_t nb)>; // b: the batch, targets [t0, t0 + nb) of the call
struct PolarCall {
  const atmrt_sight_target_t* targets; // [plan.meta.size()], on the host
  const std::vector<double>& dtab;
  const PolarPlan& plan;
  std::function<void(Carve&, size_t nb)> carve; // what a batch of nb targets carves beside its profiles
  int ev0;
  double* ms;                     // [1 + stages.size()]
  std::vector<PolarStage> stages; // the call's kernels in order, its downloads in the last
};

// everything every batch carves from d_sight; dtab first, so that it stays where the call put it
void polar_carve(Carve& k, size_t n_dtab, size_t nb, size_t entries, atmrt_sight_target_t*& targets, SightMeta*& meta, double*& dtab, SightBatch& b) {
  k(dtab, n_dtab * sizeof(double)), k(b.alt, sizeof(double));
  k(targets, nb * sizeof(atmrt_sight_target_t)), k(meta, nb * sizeof(SightMeta)), k(b.calc, nb * sizeof(DirCalc));
  k(b.T, entries * sizeof(double)), k(b.lat, entries * sizeof(double)), k(b.lon, entries * sizeof(double));
}

// the bytes of a batch of nb targets of m samples each, for polar_plan
std::function<size_t(size_t)> polar_layout_bytes(int32_t m, const std::function<void(Carve&, size_t)>& carve) {
  return [m, &carve](size_t nb) {
    Carve k(nullptr);
    atmrt_sight_target_t* targets;
    SightMeta* meta;
    double* dtab;
    SightBatch b{};
    polar_carve(k, (size_t)m + 1, nb, nb * ((size_t)m + 1), targets, meta, dtab, b);
    carve(k, nb);
    return k.bytes;
  };
}

// d_sight is reserved once for the largest batch (every array at its largest) and carved again by every batch: dtab, uploaded once,
// keeps its place.  A batch is synchronised before the next one carves the same bytes (and reads the host arrays again).
int polar_run(atmrt_ctx* c, const Frame& f, const PolarCall& call) {
  hipStream_t s = c->stream;
  const PolarPlan& plan = call.plan;
  const size_t n_dtab = call.dtab.size(), n_batches = plan.batch_begin.size() - 1;
  const int n_ms = 1 + (int)call.stages.size();
  size_t nb_max = 0;
  for (size_t k = 0; k < n_batches; k++) nb_max = std::max(nb_max, plan.batch_begin[k + 1] - plan.batch_begin[k]);
  atmrt_sight_target_t* d_targets = nullptr;
  SightMeta* d_meta = nullptr;
  double* d_dtab = nullptr;
  SightBatch b{};
  const auto carve = [&](Carve& k, size_t nb, size_t entries) { polar_carve(k, n_dtab, nb, entries, d_targets, d_meta, d_dtab, b), call.carve(k, nb); };
  HIP_TRY(c, reserve_carved(c->d_sight, [&](Carve& k) { carve(k, nb_max, plan.entries_max); }));
  HIP_TRY(c, hipMemcpyAsync(d_dtab, call.dtab.data(), n_dtab * sizeof(double), hipMemcpyHostToDevice, s));
  for (size_t k = 0; k < n_batches; k++) {
    const size_t t0 = plan.batch_begin[k], nb = plan.batch_begin[k + 1] - t0;
    const size_t entries = (size_t)plan.meta[t0 + nb - 1].off + plan.meta[t0 + nb - 1].m + 1;
    int m_max = 0;
    for (size_t t = t0; t < t0 + nb; t++) m_max = std::max(m_max, plan.meta[t].m);
    Carve k_batch(c->d_sight.ptr);
    carve(k_batch, nb, entries);
    b.n = (int32_t)nb, b.targets = d_targets, b.meta = d_meta, b.dtab = d_dtab;
    HIP_TRY(c, hipEventRecord(c->ev[call.ev0], s));
    HIP_TRY(c, hipMemcpyAsync(d_targets, call.targets + t0, nb * sizeof(atmrt_sight_target_t), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d_meta, plan.meta.data() + t0, nb * sizeof(SightMeta), hipMemcpyHostToDevice, s));
    launch_sight_profile(f, b, m_max, s);
    HIP_TRY(c, hipEventRecord(c->ev[call.ev0 + 1], s));
    for (int i = 1; i < n_ms; i++) {
      if (int rc = call.stages[i - 1](b, t0, nb)) return rc;
      HIP_TRY(c, hipEventRecord(c->ev[call.ev0 + 1 + i], s));
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, event_intervals(c->ev + call.ev0, n_ms, call.ms, true));
  }
  return ATMRT_OK;
}

} // namespace

extern "C" int atmrt_sight_lines(atmrt_ctx* c, const atmrt_sight_target_t* targets, size_t n, double fan_lo_deg, double fan_hi_deg,
                                 int32_t rounds, atmrt_sight_t* out) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (!targets || !out) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "targets or out is NULL");
  if (n == 0 || n > SIGHT_N_MAX) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "the number of targets must lie in [1, 65536]");
  if (!(std::isfinite(fan_lo_deg) && std::isfinite(fan_hi_deg) && fan_lo_deg < fan_hi_deg && fan_hi_deg - fan_lo_deg <= 180.0))
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "the fan must be finite, increasing and at most 180 degrees wide");
  if (rounds < 1 || rounds > 4) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "rounds must lie in [1, 4]");
  if (int rc = sight_check_state(c, "atmrt_sight_lines")) return rc;
  std::vector<double> dtab;
  std::vector<int32_t> m;
  if (const char* msg = sight_lattice(c, targets, n, dtab, m)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s", msg);
  const PolarPlan plan = polar_plan(m, sight_scratch_limit(), 0);
  Frame f;
  if (int rc = prepare_frame(c, &f)) return rc;
  hipStream_t s = c->stream;
  atmrt_sight_t* d_out = nullptr;
  double ms_sum[3] = {};
  const PolarCall call{targets, dtab, plan, [&](Carve& k, size_t nb) { k(d_out, nb * sizeof(atmrt_sight_t)); }, EV_SIGHT_BEGIN, ms_sum,
                       {[&](const SightBatch& b, size_t, size_t) -> int {
                          launch_sight_solve(f, b, fan_lo_deg, fan_hi_deg, rounds, d_out, s);
                          return ATMRT_OK;
                        },
                        [&](const SightBatch&, size_t t0, size_t nb) -> int {
                          HIP_TRY(c, hipMemcpyAsync(out + t0, d_out, nb * sizeof(atmrt_sight_t), hipMemcpyDeviceToHost, s));
                          return ATMRT_OK;
                        }}};
  if (int rc = polar_run(c, f, call)) return rc;
  memcpy(c->sight_timings, ms_sum, sizeof ms_sum);
  c->sight_batches = (int32_t)plan.batch_begin.size() - 1;
  return ATMRT_OK;
}

// One batch of one target through the driver: its events are the sight lines' own, its intervals are dropped.
extern "C" int atmrt_sight_fan_probe(atmrt_ctx* c, const atmrt_sight_target_t* target, size_t n_angles, const double* angles_deg,
                                     atmrt_sight_ray_t* rays) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (!target || !angles_deg || !rays) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "target, angles_deg or rays is NULL");
  if (n_angles == 0 || n_angles > SIGHT_PROBE_MAX) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "the number of angles must lie in [1, 4096]");
  if (int rc = sight_check_state(c, "atmrt_sight_fan_probe")) return rc;
  std::vector<double> dtab;
  std::vector<int32_t> m;
  if (const char* msg = sight_lattice(c, target, 1, dtab, m)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s", msg);
  const PolarPlan plan = polar_plan(m, SIGHT_SCRATCH_BYTES, 0);
  Frame f;
  if (int rc = prepare_frame(c, &f)) return rc;
  hipStream_t s = c->stream;
  atmrt_sight_ray_t* d_rays = nullptr;
  double* d_angles = nullptr;
  double ms_dropped[2] = {};
  const PolarCall call{target, dtab, plan,
                       [&](Carve& k, size_t) { k(d_rays, n_angles * sizeof(atmrt_sight_ray_t)), k(d_angles, n_angles * sizeof(double)); },
                       EV_SIGHT_BEGIN, ms_dropped,
                       {[&](const SightBatch& b, size_t, size_t) -> int {
                         HIP_TRY(c, hipMemcpyAsync(d_angles, angles_deg, n_angles * sizeof(double), hipMemcpyHostToDevice, s));
                         launch_sight_probe(f, b, n_angles, d_angles, d_rays, s);
                         HIP_TRY(c, hipMemcpyAsync(rays, d_rays, n_angles * sizeof(atmrt_sight_ray_t), hipMemcpyDeviceToHost, s));
                         return ATMRT_OK;
                       }}};
  return polar_run(c, f, call);
}

extern "C" int atmrt_last_sight_timings(atmrt_ctx* c, double out[3]) {
  if (!c || !out) return ATMRT_ERR_INVALID_ARGUMENT;
  memcpy(out, c->sight_timings, sizeof c->sight_timings);
  return ATMRT_OK;
}

extern "C" int atmrt_last_sight_batches(atmrt_ctx* c, int32_t* batches) {
  if (!c || !batches) return ATMRT_ERR_INVALID_ARGUMENT;
  *batches = c->sight_batches;
  return ATMRT_OK;
}

// ---------------------------------------------------------------------------------------------
// viewshed (include/atmrt.h; kernels in atmrt_viewshed.h)
// ---------------------------------------------------------------------------------------------
extern "C" int atmrt_viewshed_fan_angles(double lo, double hi, int32_t fan_rays, double* out) {
  if (!out || !viewshed_fan_rays_ok(fan_rays) || !std::isfinite(lo) || !std::isfinite(hi)) return ATMRT_ERR_INVALID_ARGUMENT;
  const double delta = viewshed_fan_delta(lo, hi, fan_rays);
  for (int k = 0; k < fan_rays; k++) out[k] = sight_fan_angle(lo, delta, k);
  return ATMRT_OK;
}

extern "C" int atmrt_debug_viewshed_shape(int32_t fan_rays, int32_t* az_per_load, int32_t* step_tile, int32_t* rays_per_lane) {
  if (az_per_load) *az_per_load = VIEWSHED_AZ;
  if (step_tile) *step_tile = VIEWSHED_TILE;
  if (rays_per_lane) *rays_per_lane = viewshed_fan_rays_ok(fan_rays) ? viewshed_rays_per_lane(fan_rays) : 0;
  return ATMRT_OK;
}

namespace {

// The planes of a viewshed that `asked` names, in carving order, with the bytes of one cell's entry: f(bytes, p.plane...) for each,
// over any number of ViewshedPlanes.
template <class F, class... P>
void viewshed_planes(const ViewshedAsked& asked, F&& f, P&... p) {
  if (asked.k_star) f(2, p.k_star...);
  f(1, p.status...), f(8, p.hidden...);
  if (asked.block_index) f(4, p.block_index...);
  if (asked.ground) f(8, p.ground...);
  if (asked.lat) f(8, p.lat...);
  if (asked.lon) f(8, p.lon...);
}

// What the viewshed and the horizon refuse alike, and what both begin with: one target per azimuth, the lattice and the call's m.
int polar_call_plan(atmrt_ctx* c, const char* what, double az_lo_deg, double az_step_deg, int32_t n_az, double reach, double height, double fan_lo_deg,
                    double fan_hi_deg, int32_t fan_rays, std::vector<atmrt_sight_target_t>& targets, std::vector<double>& dtab, int32_t* m) {
  if (!(std::isfinite(az_lo_deg) && std::isfinite(az_step_deg))) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: az_lo_deg and az_step_deg must be finite", what);
  if (n_az < 1 || (size_t)n_az > VIEWSHED_N_MAX) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: n_az must lie in [1, 65536]", what);
  if (!viewshed_fan_rays_ok(fan_rays)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: fan_rays must be a multiple of 64 in [64, 4096]", what);
  if (!(std::isfinite(fan_lo_deg) && std::isfinite(fan_hi_deg) && fan_lo_deg < fan_hi_deg && fan_hi_deg - fan_lo_deg <= 180.0))
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: the fan must be finite, increasing and at most 180 degrees wide", what);
  if (int rc = sight_check_state(c, what)) return rc;
  targets.resize((size_t)n_az);
  for (int32_t j = 0; j < n_az; j++) targets[j] = atmrt_sight_target_t{az_lo_deg + (double)j * az_step_deg, reach, height};
  if (!std::isfinite(targets.back().azimuth_deg)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: the last azimuth is not finite", what);
  std::vector<int32_t> m_first; // reach and height are the same for every azimuth: checked once, with the lattice
  if (const char* msg = sight_lattice(c, targets.data(), 1, dtab, m_first)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: %s", what, msg);
  *m = m_first[0];
  const size_t table_bytes = ((size_t)*m + 1) * (size_t)fan_rays * sizeof(double);
  if (table_bytes > SIGHT_SCRATCH_BYTES)
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: the path table of (m + 1) * K * 8 = %zu bytes exceeds the scratch limit of %zu", what, table_bytes, SIGHT_SCRATCH_BYTES);
  return ATMRT_OK;
}

// The path table H[i][k] of the fan, the one product of both calls under the one key: built where the key differs from the last
// build's.  *ms: what the build took between EV_VS_BEGIN and EV_VS_PATHS, 0 when the table was found.
int viewshed_paths_refresh(atmrt_ctx* c, const Frame& f, double fan_lo_deg, double fan_hi_deg, int K, int m, bool* rebuilt, double* ms_paths) {
  hipStream_t s = c->stream;
  const atmrt_position_t& pos = c->params.position;
  const ViewshedKey key{c->atm.serial(), c->terrain_uploaded, pos.altitude_kind, bits(pos.latitude), bits(pos.longitude), bits(pos.altitude),
                        bits(fan_lo_deg), bits(fan_hi_deg), bits(c->params.simulation_step), K, m, c->params.straight_rays ? 1 : 0, key_of(c->earth)};
  *ms_paths = 0.0;
  HIP_TRY(c, hipEventRecord(c->ev[EV_VS_BEGIN], s));
  int rc = c->viewshed_paths.refresh(key, [&](Nothing&) -> int {
    HIP_TRY(c, c->d_viewshed_paths.reserve(((size_t)m + 1) * (size_t)K * sizeof(double)));
    launch_viewshed_paths(f, fan_lo_deg, fan_hi_deg, K, m, c->d_viewshed_paths.as<double>(), s);
    HIP_TRY(c, hipEventRecord(c->ev[EV_VS_PATHS], s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    return ATMRT_OK;
  }, false, rebuilt);
  if (rc) return rc;
  if (*rebuilt) {
    float ms = 0.0f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[EV_VS_BEGIN], c->ev[EV_VS_PATHS]));
    *ms_paths = ms;
  }
  return ATMRT_OK;
}

// The map a fused call scatters its batches into (atmrt_viewshed_map*): device planes on c's device.
struct ViewshedMapSink {
  atmrt_geo_grid_t grid;
  VsMapPlanes planes;
  bool accumulate;
  atmrt_viewshed_map_stats_t* stats; // may be null
};

// The checks the three map entry points share; 0 or a status with the message set.
int viewshed_map_check(atmrt_ctx* c, const char* what, const atmrt_geo_grid_t* grid, const void* n_samples, const void* n_seen) {
  if (!grid || !n_samples || !n_seen) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: grid, n_samples or n_seen is NULL", what);
  if (const char* msg = geo_grid_check(*grid)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: %s", what, msg);
  return ATMRT_OK;
}

// The call's statistics block, read back once every scatter of the call has run.
int viewshed_map_stats(atmrt_ctx* c, atmrt_viewshed_map_stats_t* stats) {
  uint64_t block[VSMAP_N] = {};
  HIP_TRY(c, hipMemcpyAsync(block, c->d_vsmap.ptr, sizeof block, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipGetLastError());
  if (stats) *stats = atmrt_viewshed_map_stats_t{block[VSMAP_SAMPLES], block[VSMAP_BINNED], block[VSMAP_OUTSIDE], block[VSMAP_SKIPPED], block[VSMAP_SEEN]};
  return ATMRT_OK;
}

// map == nullptr: the viewshed into dst (host arrays, or device_planes).  map != nullptr: dst is empty; every batch's status, hidden,
// lat and lon are staged in d_sight like the host route's planes and scattered into the map where the host route downloads.
int viewshed_run(atmrt_ctx* c, const char* what, const atmrt_viewshed_spec_t* spec, const ViewshedPlanes& dst, bool device_planes,
                 const ViewshedMapSink* map = nullptr) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (!spec) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: spec is NULL", what);
  if (!map && (!dst.k_star || !dst.status || !dst.hidden)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: spec, k_star, status or hidden is NULL", what);
  const ViewshedAsked asked = map ? ViewshedAsked{false, false, false, true, true}
                                  : ViewshedAsked{true, dst.block_index != nullptr, dst.ground != nullptr, dst.lat != nullptr, dst.lon != nullptr};
  const atmrt_viewshed_spec_t v = *spec;
  std::vector<atmrt_sight_target_t> targets;
  std::vector<double> dtab;
  int32_t m = 0;
  if (int rc = polar_call_plan(c, what, v.az_lo_deg, v.az_step_deg, v.n_az, v.reach, v.height, v.fan_lo_deg, v.fan_hi_deg, v.fan_rays, targets, dtab, &m)) return rc;
  const int K = v.fan_rays;
  // beside its profiles a batch carves the planes of the host route and of the map; the device route writes the caller's own
  ViewshedPlanes staged{};
  const std::function<void(Carve&, size_t)> carve = [&](Carve& k, size_t nb) {
    staged = ViewshedPlanes{};
    if (!device_planes) viewshed_planes(asked, [&](size_t bytes, auto*& plane) { k(plane, nb * (size_t)m * bytes); }, staged);
  };
  const PolarPlan plan = polar_plan(std::vector<int32_t>((size_t)v.n_az, m), sight_scratch_limit(), device_planes ? 0 : viewshed_cell_bytes(asked) * (size_t)m,
                                    polar_layout_bytes(m, carve));
  Frame f;
  if (int rc = prepare_frame(c, &f)) return rc;
  hipStream_t s = c->stream;
  bool rebuilt = false;
  double ms_sum[4] = {};
  if (int rc = viewshed_paths_refresh(c, f, v.fan_lo_deg, v.fan_hi_deg, K, m, &rebuilt, &ms_sum[0])) return rc;
  if (map) {
    HIP_TRY(c, c->d_vsmap.reserve(VSMAP_N * sizeof(uint64_t)));
    launch_vsmap_reset(c->d_vsmap.ptr, s);
    if (!map->accumulate) launch_vsmap_clear(map->grid, map->planes, s);
  }
  const PolarCall call{targets.data(), dtab, plan, carve, EV_VS_BATCH, &ms_sum[1],
                       {[&](const SightBatch& b, size_t t0, size_t nb) -> int {
                          ViewshedScan scan{};
                          scan.n = (int32_t)nb, scan.m = m, scan.K = K, scan.height = v.height;
                          scan.H = c->d_viewshed_paths.as<double>();
                          scan.T = b.T, scan.lat = b.lat, scan.lon = b.lon;
                          scan.out = staged;
                          if (device_planes) viewshed_planes(asked, [&](size_t, auto*& out, auto* from) { out = from + t0 * (size_t)m; }, scan.out, dst);
                          launch_viewshed_scan(scan, s);
                          return ATMRT_OK;
                        },
                        [&](const SightBatch&, size_t t0, size_t nb) -> int {
                          const size_t cells = nb * (size_t)m, at = t0 * (size_t)m;
                          hipError_t e = hipSuccess;
                          if (map) {
                            launch_vsmap_scatter(VsMapSamples{cells, staged.status, staged.hidden, staged.lat, staged.lon}, map->grid, map->planes, c->d_vsmap.ptr, s);
                          } else if (!device_planes) {
                            viewshed_planes(asked, [&](size_t bytes, auto* to, auto* from) {
                              if (e == hipSuccess) e = hipMemcpyAsync(to + at, from, cells * bytes, hipMemcpyDeviceToHost, s);
                            }, dst, staged);
                          }
                          HIP_TRY(c, e);
                          return ATMRT_OK;
                        }}};
  if (int rc = polar_run(c, f, call)) return rc;
  memcpy(c->viewshed_timings, ms_sum, sizeof ms_sum);
  c->viewshed_batches = (int32_t)plan.batch_begin.size() - 1;
  c->viewshed_rebuilt = rebuilt ? 1 : 0;
  if (map) return viewshed_map_stats(c, map->stats);
  return ATMRT_OK;
}

} // namespace

extern "C" int atmrt_viewshed_steps(atmrt_ctx* c, double reach, int32_t* m) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (!m) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "atmrt_viewshed_steps: m is NULL");
  if (int rc = sight_check_state(c, "atmrt_viewshed_steps")) return rc;
  const atmrt_sight_target_t t{0.0, reach, 0.0};
  if (const char* msg = sight_steps(c, &t, 1, m)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "atmrt_viewshed_steps: %s", msg);
  return ATMRT_OK;
}

extern "C" int atmrt_viewshed(atmrt_ctx* c, const atmrt_viewshed_spec_t* spec, uint16_t* k_star, uint8_t* status, double* hidden,
                              int32_t* block_index, double* ground, double* lat, double* lon) {
  return viewshed_run(c, "atmrt_viewshed", spec, ViewshedPlanes{k_star, status, hidden, block_index, ground, lat, lon}, false);
}

extern "C" int atmrt_viewshed_device(atmrt_ctx* c, const atmrt_viewshed_spec_t* spec, uint16_t* k_star, uint8_t* status, double* hidden,
                                     int32_t* block_index, double* ground, double* lat, double* lon) {
  return viewshed_run(c, "atmrt_viewshed_device", spec, ViewshedPlanes{k_star, status, hidden, block_index, ground, lat, lon}, true);
}

extern "C" int atmrt_last_viewshed_timings(atmrt_ctx* c, double out[4]) {
  if (!c || !out) return ATMRT_ERR_INVALID_ARGUMENT;
  memcpy(out, c->viewshed_timings, sizeof c->viewshed_timings);
  return ATMRT_OK;
}

extern "C" int atmrt_last_viewshed_work(atmrt_ctx* c, int32_t* batches, int32_t* table_rebuilt) {
  if (!c || !batches || !table_rebuilt) return ATMRT_ERR_INVALID_ARGUMENT;
  *batches = c->viewshed_batches;
  *table_rebuilt = c->viewshed_rebuilt;
  return ATMRT_OK;
}

// ---------------------------------------------------------------------------------------------
// viewshed map (include/atmrt.h; kernels in atmrt_viewshed_map.h)
// ---------------------------------------------------------------------------------------------
extern "C" int atmrt_viewshed_map_planes_device(atmrt_ctx* c, const atmrt_geo_grid_t* grid, size_t n, const uint8_t* status, const double* hidden,
                                                const double* lat, const double* lon, int32_t accumulate, uint32_t* n_samples, uint32_t* n_seen,
                                                double* min_hidden, atmrt_viewshed_map_stats_t* stats) {
  const char* what = "atmrt_viewshed_map_planes_device";
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (int rc = viewshed_map_check(c, what, grid, n_samples, n_seen)) return rc;
  if (n > VSMAP_SAMPLES_MAX) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: n exceeds (2^31 - 1) * 256 samples", what);
  if (n && (!status || !hidden || !lat || !lon)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: status, hidden, lat or lon is NULL", what);
  if (int rc = sight_check_state(c, what)) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const VsMapPlanes map{n_samples, n_seen, min_hidden};
  HIP_TRY(c, c->d_vsmap.reserve(VSMAP_N * sizeof(uint64_t)));
  launch_vsmap_reset(c->d_vsmap.ptr, s);
  if (!accumulate) launch_vsmap_clear(*grid, map, s);
  launch_vsmap_scatter(VsMapSamples{n, status, hidden, lat, lon}, *grid, map, c->d_vsmap.ptr, s);
  return viewshed_map_stats(c, stats);
}

extern "C" int atmrt_viewshed_map_device(atmrt_ctx* c, const atmrt_viewshed_spec_t* spec, const atmrt_geo_grid_t* grid, int32_t accumulate,
                                         uint32_t* n_samples, uint32_t* n_seen, double* min_hidden, atmrt_viewshed_map_stats_t* stats) {
  const char* what = "atmrt_viewshed_map_device";
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (!spec) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: spec is NULL", what);
  if (int rc = viewshed_map_check(c, what, grid, n_samples, n_seen)) return rc;
  const ViewshedMapSink sink{*grid, VsMapPlanes{n_samples, n_seen, min_hidden}, accumulate != 0, stats};
  return viewshed_run(c, what, spec, ViewshedPlanes{}, false, &sink);
}

extern "C" int atmrt_viewshed_map(atmrt_ctx* c, const atmrt_viewshed_spec_t* spec, const atmrt_geo_grid_t* grid, int32_t accumulate,
                                  uint32_t* n_samples, uint32_t* n_seen, double* min_hidden, atmrt_viewshed_map_stats_t* stats) {
  const char* what = "atmrt_viewshed_map";
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (!spec) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: spec is NULL", what);
  if (int rc = viewshed_map_check(c, what, grid, n_samples, n_seen)) return rc;
  if (int rc = sight_check_state(c, what)) return rc; // before the staging buffer is touched
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t n_cells = (size_t)grid->n_lat * grid->n_lon, count_bytes = Carve::pad(n_cells * sizeof(uint32_t));
  HIP_TRY(c, c->d_io.reserve(2 * count_bytes + n_cells * sizeof(double)));
  uint32_t *d_samples = c->d_io.as<uint32_t>(), *d_seen = reinterpret_cast<uint32_t*>(c->d_io.as<char>() + count_bytes);
  double* d_min = min_hidden ? reinterpret_cast<double*>(c->d_io.as<char>() + 2 * count_bytes) : nullptr;
  if (accumulate) {
    HIP_TRY(c, hipMemcpy(d_samples, n_samples, n_cells * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d_seen, n_seen, n_cells * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (min_hidden) HIP_TRY(c, hipMemcpy(d_min, min_hidden, n_cells * sizeof(double), hipMemcpyHostToDevice));
  }
  const ViewshedMapSink sink{*grid, VsMapPlanes{d_samples, d_seen, d_min}, accumulate != 0, stats};
  if (int rc = viewshed_run(c, what, spec, ViewshedPlanes{}, false, &sink)) return rc;
  HIP_TRY(c, hipMemcpy(n_samples, d_samples, n_cells * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(n_seen, d_seen, n_cells * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (min_hidden) HIP_TRY(c, hipMemcpy(min_hidden, d_min, n_cells * sizeof(double), hipMemcpyDeviceToHost));
  return ATMRT_OK;
}

// ---------------------------------------------------------------------------------------------
// horizon (include/atmrt.h; kernels in atmrt_horizon.h)
// ---------------------------------------------------------------------------------------------
extern "C" int atmrt_debug_horizon_shape(int32_t fan_rays, int32_t* az_per_load, int32_t* step_tile, int32_t* rays_per_lane) {
  if (az_per_load) *az_per_load = HORIZON_AZ;
  if (step_tile) *step_tile = HORIZON_TILE;
  if (rays_per_lane) *rays_per_lane = viewshed_fan_rays_ok(fan_rays) ? horizon_rays_per_lane(fan_rays) : 0;
  return ATMRT_OK;
}

namespace {

int horizon_run(atmrt_ctx* c, const char* what, const atmrt_horizon_spec_t* spec, atmrt_horizon_t* dst, bool device_out) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (!spec || !dst) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: spec or out is NULL", what);
  const atmrt_horizon_spec_t v = *spec;
  if (v.rounds < 1 || v.rounds > 4) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "%s: rounds must lie in [1, 4]", what);
  std::vector<atmrt_sight_target_t> targets;
  std::vector<double> dtab;
  int32_t m = 0;
  if (int rc = polar_call_plan(c, what, v.az_lo_deg, v.az_step_deg, v.n_az, v.reach, 0.0, v.fan_lo_deg, v.fan_hi_deg, v.fan_rays, targets, dtab, &m)) return rc;
  const int K = v.fan_rays;
  // beside its profiles a batch carves the records of the host route; the device route writes the caller's own
  atmrt_horizon_t* staged = nullptr;
  const std::function<void(Carve&, size_t)> carve = [&](Carve& k, size_t nb) {
    if (!device_out) k(staged, nb * sizeof(atmrt_horizon_t));
  };
  const PolarPlan plan = polar_plan(std::vector<int32_t>((size_t)v.n_az, m), sight_scratch_limit(), device_out ? 0 : sizeof(atmrt_horizon_t), polar_layout_bytes(m, carve));
  Frame f;
  if (int rc = prepare_frame(c, &f)) return rc;
  hipStream_t s = c->stream;
  bool rebuilt = false;
  double ms_sum[5] = {};
  if (int rc = viewshed_paths_refresh(c, f, v.fan_lo_deg, v.fan_hi_deg, K, m, &rebuilt, &ms_sum[0])) return rc;
  const auto out_of = [&](size_t t0) { return device_out ? dst + t0 : staged; };
  const PolarCall call{targets.data(), dtab, plan, carve, EV_HZ_BATCH, &ms_sum[1],
                       {[&](const SightBatch& b, size_t t0, size_t nb) -> int {
                          HorizonScan scan{};
                          scan.n = (int32_t)nb, scan.m = m, scan.K = K, scan.lo = v.fan_lo_deg, scan.hi = v.fan_hi_deg;
                          scan.H = c->d_viewshed_paths.as<double>();
                          scan.T = b.T, scan.out = out_of(t0);
                          launch_horizon_scan(scan, s);
                          return ATMRT_OK;
                        },
                        [&](const SightBatch& b, size_t t0, size_t) -> int {
                          launch_horizon_refine(f, b, v.rounds, out_of(t0), s);
                          return ATMRT_OK;
                        },
                        [&](const SightBatch&, size_t t0, size_t nb) -> int {
                          if (!device_out) HIP_TRY(c, hipMemcpyAsync(dst + t0, staged, nb * sizeof(atmrt_horizon_t), hipMemcpyDeviceToHost, s));
                          return ATMRT_OK;
                        }}};
  if (int rc = polar_run(c, f, call)) return rc;
  memcpy(c->horizon_timings, ms_sum, sizeof ms_sum);
  c->horizon_batches = (int32_t)plan.batch_begin.size() - 1;
  c->horizon_rebuilt = rebuilt ? 1 : 0;
  return ATMRT_OK;
}

} // namespace

extern "C" int atmrt_horizon(atmrt_ctx* c, const atmrt_horizon_spec_t* spec, atmrt_horizon_t* out) {
  return horizon_run(c, "atmrt_horizon", spec, out, false);
}

extern "C" int atmrt_horizon_device(atmrt_ctx* c, const atmrt_horizon_spec_t* spec, atmrt_horizon_t* out) {
  return horizon_run(c, "atmrt_horizon_device", spec, out, true);
}

extern "C" int atmrt_last_horizon_timings(atmrt_ctx* c, double out[5]) {
  if (!c || !out) return ATMRT_ERR_INVALID_ARGUMENT;
  memcpy(out, c->horizon_timings, sizeof c->horizon_timings);
  return ATMRT_OK;
}

extern "C" int atmrt_last_horizon_work(atmrt_ctx* c, int32_t* batches, int32_t* table_rebuilt) {
  if (!c || !batches || !table_rebuilt) return ATMRT_ERR_INVALID_ARGUMENT;
  *batches = c->horizon_batches;
  *table_rebuilt = c->horizon_rebuilt;
  return ATMRT_OK;
}
