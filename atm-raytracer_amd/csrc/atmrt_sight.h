// atmrt_sight.h — sight lines (include/atmrt.h, "sight lines": the rule is stated there): at which elevation angle a target appears
// and what terrain hides it.  The two host halves of the rule and the launch interface for atmrt_polar.hip; the kernels themselves are
// compiled by atmrt_sight.hip only (ATMRT_SIGHT_KERNELS).
//
//   k_sight_calc     one thread per target: its DirectionalCalc, as k_fast_columns makes a column's (thread 0: the observer's altitude)
//   k_sight_profile  lane-parallel over the samples i <= m of a target: lat_i, lon_i, T_i, as k_terrain_profile makes a column's
//   k_sight_solve    one wavefront per target, lane k = ray k of the fan; the serial stepper per lane (the one k_ray_paths runs), the
//                    profile read wave-uniformly through the constant address space (scalar loads).  All rounds inside the kernel: a
//                    ballot finds the highest failing lane, lo / hi of the next fan are read from lanes k* - 1 and k*.  The step
//                    loop's bound is wave-uniform; a blocked lane idles (it is not in the stepper's votes any more) and every lane
//                    reaches every ballot; the wave leaves a round early only when all lanes are blocked.  No atomics.
//   k_sight_probe    the same per-lane ray (sight_trace) for a list of angles against one target: atmrt_sight_fan_probe
#pragma once

#include "atmrt_kernels.h"
#include "atmrt_polar_plan.h" // SightMeta, sight_target_bytes

namespace atmrt {

constexpr int SIGHT_FAN = 64;          // rays of a fan: one wavefront
constexpr int SIGHT_M_MAX = 65535;     // samples to the target
constexpr size_t SIGHT_N_MAX = 65536;  // targets of a call
constexpr size_t SIGHT_PROBE_MAX = 4096;
constexpr size_t SIGHT_SCRATCH_BYTES = 200u << 20; // what a batch may carve: the grow-only buffer keeps an eighth of headroom on top

// ---- the rule's host halves (atmrt_sight_fan_angles, atmrt_sight_pick), the same code on the device ------------------------------
ATMRT_HD double sight_fan_delta(double lo, double hi) { return (hi - lo) / 63.0; }
ATMRT_HD double sight_fan_angle(double lo, double delta, int k) { return lo + (double)k * delta; }
// k* from the fan's failing rays, bit k = ray k fails: one above the highest failing ray
ATMRT_HD int sight_pick(unsigned long long fails) { return fails ? 64 - __builtin_clzll(fails) : 0; }

// ---- launch interface -----------------------------------------------------------------------------------------------------------------
// One batch of targets in device memory.  dtab[i] = d_i for i <= the largest m of the call.
struct SightBatch {
  int32_t n;
  const atmrt_sight_target_t* targets; // [n]
  const SightMeta* meta;               // [n]
  DirCalc* calc;                       // [n]
  double *T, *lat, *lon;               // profiles, sum of (m + 1) entries
  const double* dtab;
  double* alt;                         // [1] the observer's altitude after Altitude::abs
};
void launch_sight_profile(const Frame& f, const SightBatch& b, int m_max, hipStream_t stream);
void launch_sight_solve(const Frame& f, const SightBatch& b, double lo, double hi, int rounds, atmrt_sight_t* out, hipStream_t stream);
void launch_sight_probe(const Frame& f, const SightBatch& b, size_t n_angles, const double* angles_deg, atmrt_sight_ray_t* rays,
                        hipStream_t stream);

} // namespace atmrt

#if defined(ATMRT_SIGHT_KERNELS)
#include "atmrt_device.h"

namespace atmrt {

typedef const __attribute__((address_space(4))) double* SightConstF64;

__global__ __launch_bounds__(256) void k_sight_calc(Frame f, SightBatch b) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) *b.alt = observer_altitude(f);
  if (t >= b.n) return;
  DirCalc c;
  dircalc_new(f.earth, f.p.position.latitude, f.p.position.longitude, b.targets[t].azimuth_deg, c);
  b.calc[t] = c;
}

// blockIdx.x = target, blockIdx.y = block of 256 samples (at most 256 of them: m <= 65535)
template <int CALC>
__global__ __launch_bounds__(256) void k_sight_profile(Frame f, SightBatch b) {
  const int t = blockIdx.x;
  const SightMeta me = b.meta[t];
  const int i = blockIdx.y * 256 + threadIdx.x;
  if (i > me.m) return;
  const Earth e = earth_for<CALC>(f);
  const DirCalc c = b.calc[t];
  const double d = b.dtab[i]; // == f.xs[i] where the frame's table reaches: the same additions
  double lat, lon;
  if (i <= f.march_steps) coords_at_step(f, e, c, i, d, lat, lon);
  else coords_at_dist(e, c, d, lat, lon);
  b.lat[me.off + i] = lat;
  b.lon[me.off + i] = lon;
  b.T[me.off + i] = terrain_elev_or_zero(f.tv, lat, lon);
}

// One ray against one profile (T: the target's, wave-uniform; m, prop wave-uniform): the per-lane part of the rule.  A lane that is
// not `live` (a surplus lane of the probe) starts blocked.  Every lane of the wavefront must call this together.
template <bool PROBE>
static __device__ __forceinline__ atmrt_sight_ray_t sight_trace(const Frame& f, double alt, SightConstF64 T, int m, double prop, double e_deg,
                                                              bool live) {
  const bool sph = f.earth.spherical != 0, straight = f.p.straight_rays != 0;
  const double radius = f.earth.shape_radius, step = f.p.simulation_step;
  Stepper s;
  stepper_init(s, sph, radius, alt, dm_to_radians(e_deg));
  double h_prev = alt, c_prev = alt - T[0];
  double h_m1 = alt, h_m = alt; // H_{m-1}, H_m
  bool blocked = !live;
  atmrt_sight_ray_t r;
  r.block_index = -1;
  r.min_index = 0;
  r.min_clearance = c_prev;
  for (int i = 1; i <= m; i++) {
    const double t = T[i];
    if (!blocked) {
      const RayState st = stepper_next(s, *f.atm, sph, radius, straight, step);
      if (i < m) {
        const double c = st.h - t;
        if (h_prev < -1000.0 || c_prev * c < 0.0) { // utils.rs:167, utils.rs:222
          blocked = true;
          r.block_index = i;
        }
        if (PROBE && c < r.min_clearance) r.min_clearance = c, r.min_index = i;
        c_prev = c;
        h_m1 = st.h;
      } else {
        h_m = st.h;
      }
      h_prev = st.h;
    }
    if (__all(blocked)) break;
  }
  const double arrival = h_m1 + prop * (h_m - h_m1);
  r.arrival = (r.block_index >= 0 || arrival != arrival) ? qnan() : arrival;
  return r;
}

constexpr int SIGHT_WAVES = 4; // wavefronts (targets) per block

__global__ __launch_bounds__(64 * SIGHT_WAVES) void k_sight_solve(Frame f, SightBatch b, double lo, double hi, int rounds,
                                                                  atmrt_sight_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int t = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * SIGHT_WAVES + (threadIdx.x >> 6)));
  if (t >= b.n) return; // the whole wavefront
  const SightMeta me = b.meta[t];
  const int m = me.m;
  const SightConstF64 T = (SightConstF64)(uintptr_t)(b.T + me.off);
  const atmrt_sight_target_t target = b.targets[t];
  const double d0 = b.dtab[m - 1], d1 = b.dtab[m];
  const double prop = (target.distance - d0) / (d1 - d0);
  const double t0 = T[m - 1], t1 = T[m];
  const double ground = t0 + prop * (t1 - t0);
  const double aim = ground + target.height;
  const double alt = *b.alt;
  atmrt_sight_ray_t ray;
  double e = lo, delta = 0.0;
  int k_star = 0, done = 0;
  for (int r = 0; r < rounds; r++) {
    delta = sight_fan_delta(lo, hi);
    e = sight_fan_angle(lo, delta, lane);
    ray = sight_trace<false>(f, alt, T, m, prop, e, true);
    const bool fails = ray.block_index >= 0 || !(ray.arrival >= aim); // blocked, low, or NaN
    k_star = sight_pick(__ballot(fails));
    done = r + 1;
    if (k_star == 0 || k_star == SIGHT_FAN || done == rounds) break;
    lo = __shfl(e, k_star - 1, 64);
    hi = __shfl(e, k_star, 64);
  }
  // lane k* holds the answer, lane k* - 1 what stopped the ray below it
  const int at = k_star < SIGHT_FAN ? k_star : SIGHT_FAN - 1, below = k_star > 0 ? k_star - 1 : 0;
  const double angle = __shfl(e, at, 64), arrival = __shfl(ray.arrival, at, 64);
  const int block = __shfl(ray.block_index, below, 64);
  if (lane != 0) return;
  atmrt_sight_t o;
  o.status = k_star == SIGHT_FAN ? ATMRT_SIGHT_ABOVE_FAN : k_star == 0 ? ATMRT_SIGHT_BELOW_FAN : block >= 0 ? ATMRT_SIGHT_HIDDEN : ATMRT_SIGHT_SEEN;
  o.rounds_done = done;
  o.m = m;
  o.ground = ground;
  o.resolution = delta;
  const bool none = o.status == ATMRT_SIGHT_ABOVE_FAN;
  const double hidden = arrival - aim;
  o.angle = none ? qnan() : angle;
  o.arrival = none ? qnan() : arrival;
  o.hidden = none || hidden != hidden ? qnan() : hidden;
  if (o.status == ATMRT_SIGHT_HIDDEN) {
    o.block_index = block;
    o.block_distance = b.dtab[block];
    o.block_lat = b.lat[me.off + block];
    o.block_lon = b.lon[me.off + block];
    o.block_elevation = b.T[me.off + block];
  } else {
    o.block_index = -1;
    o.block_distance = o.block_lat = o.block_lon = o.block_elevation = qnan();
  }
  out[t] = o;
}

// target 0 of the batch against n_angles angles: wavefront w takes angles 64 w .. 64 w + 63
__global__ __launch_bounds__(64 * SIGHT_WAVES) void k_sight_probe(Frame f, SightBatch b, size_t n_angles, const double* __restrict__ angles_deg,
                                                                  atmrt_sight_ray_t* __restrict__ rays) {
  const size_t first = (size_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * SIGHT_WAVES + (threadIdx.x >> 6))) * 64;
  if (first >= n_angles) return; // the whole wavefront
  const size_t a = first + (threadIdx.x & 63);
  const bool live = a < n_angles;
  const SightMeta me = b.meta[0];
  const int m = me.m;
  const SightConstF64 T = (SightConstF64)(uintptr_t)(b.T + me.off);
  const double d0 = b.dtab[m - 1], d1 = b.dtab[m];
  const double prop = (b.targets[0].distance - d0) / (d1 - d0);
  const atmrt_sight_ray_t r = sight_trace<true>(f, *b.alt, T, m, prop, angles_deg[live ? a : n_angles - 1], live);
  if (live) rays[a] = r;
}

void launch_sight_profile(const Frame& f, const SightBatch& b, int m_max, hipStream_t stream) {
  hipLaunchKernelGGL(k_sight_calc, dim3(cdiv((size_t)b.n, 256)), dim3(256), 0, stream, f, b);
  ATMRT_DISPATCH_CALC(f.earth.calc, hipLaunchKernelGGL((k_sight_profile<CALC>), dim3((unsigned)b.n, cdiv((size_t)m_max + 1, 256)), dim3(256), 0,
                                                       stream, f, b));
}
void launch_sight_solve(const Frame& f, const SightBatch& b, double lo, double hi, int rounds, atmrt_sight_t* out, hipStream_t stream) {
  hipLaunchKernelGGL(k_sight_solve, dim3(cdiv((size_t)b.n, SIGHT_WAVES)), dim3(64 * SIGHT_WAVES), 0, stream, f, b, lo, hi, rounds, out);
}
void launch_sight_probe(const Frame& f, const SightBatch& b, size_t n_angles, const double* angles_deg, atmrt_sight_ray_t* rays,
                        hipStream_t stream) {
  hipLaunchKernelGGL(k_sight_probe, dim3(cdiv(n_angles, 64 * SIGHT_WAVES)), dim3(64 * SIGHT_WAVES), 0, stream, f, b, n_angles, angles_deg, rays);
}

} // namespace atmrt
#endif
