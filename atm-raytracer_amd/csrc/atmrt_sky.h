// atmrt_sky.h — sky rays (include/atmrt.h, "sky rays": the rule is stated there): the true direction of every pixel of a finished
// frame that has no trace point, and the discs of the call's bodies over them.  The launch interface for atmrt_consumers.hip; the
// kernels themselves are compiled by atmrt_sky.hip only (ATMRT_SKY_KERNELS).
//
//   k_sky_compact  one thread per pixel: the pixels WITHOUT a trace point appended to a list, a wavefront's entries contiguous and
//                  in lane order (wave_compact_append), so that the march's wavefronts are full — the ground half of a frame costs no
//                  lanes; a pixel with a trace point gets ATMRT_SKY_NONE, NaN and 0 steps here
//   k_sky_march    one list entry per lane: the stepper from h0 at the pixel's launch elevation and the rule's test per step — a pure
//                  RK4 chain with no terrain and no geodesic in it (hence no CALC variants).  A lane that is decided idles (it is not
//                  in the stepper's votes any more, as in shadow_step_loop); the wavefront leaves when all its lanes are decided.
//                  Writes true_elevation, status and steps of its pixel; the counts of the call with one atomic per wavefront and
//                  counter.  The list is in pixel order: its head holds a frame's top rows (high elevation, a few hundred steps), its
//                  tail the horizon rows (the longest chains), so wavefront w takes group n_groups - 1 - w: the longest chains start
//                  first and the short ones fill the tail of the launch (SkyJob::reverse).
//   k_sky_bodies   one thread per pixel: the body rule (sky_body_of) for the EXIT pixels, the body plane and, where an image is given,
//                  the body's colour over it.
//
//   k_sky_table_march  ("apparent elevation" of include/atmrt.h) the march over the n_alt x n_el rays of a refraction table's lattice,
//                  each with its row's h0; k runs fastest: a wavefront holds neighbouring elevations of one altitude and chains of
//                  similar length.
//   k_sky_tail     one wavefront per row of the table: tail[j] (sky_tail_of), 64 entries at a time from the row's end.
//   k_sky_apparent one thread per (h, t) pair of a list call: sky_apparent over the table.
//
//   k_sky_light_march  ("sky light" of include/atmrt.h) k_sky_march's list order with the refractivity column carried along: h_prev,
//                  q_prev and the column live across the loop beside the stepper, and every step that is not LOST or GROUND
//                  evaluates q(h) once more, generically (sky_refractivity) — not taken from the next step's first stage, which
//                  evaluates n at the same height by the certified shortcuts: equal values are the certificate's claim, not this
//                  kernel's to rely on.  A decided lane stops accumulating.
//   k_sky_fill_nan the column plane set to NaN ahead of the march, which writes the list's pixels only.
//   k_sky_shade    one thread per pixel: sky_shade_pixel for the EXIT pixels — the body plane as k_sky_bodies writes it, the image
//                  shaded in place.
//
// The three marches are one lane body (sky_lane: the stepper, the loop, the rule's test, the EXIT epilogue, with LIGHT the column)
// and one counter tail (sky_count); the two list kernels share their addressing too (sky_list_march).  They are kernels of their
// own for what a kernel owns: its parameter struct and its occupancy attribute.
//
// The launch covers the pixels, not the list (its length stays on the device: no host round trip between the two kernels); a
// wavefront beyond the list's end leaves at once.  The list call (atmrt_sky_rays) marches without a list: entry i is ray i.
#pragma once

#include "atmrt_kernels.h"

namespace atmrt {

enum SkyCtr : int { SKY_LIST = 0, SKY_EXIT, SKY_GROUND, SKY_INSIDE, SKY_LOST, SKY_STEPS, SKY_N };

struct SkyJob {
  size_t n_pixels;
  const uint32_t* hit_count;     // [n_pixels]; null: no compaction, every entry is a ray (the list call)
  const double* elevation_angle; // [n_pixels] launch elevations [deg]
  const double* alt;             // device scalar h0 (the frame's observer altitude), or null: h0 below
  double h0;
  double step, top, floor;
  int32_t m;
  int32_t reverse;               // the march takes the list from its end
  uint32_t* list;                // [n_pixels], or null with hit_count
  unsigned long long* ctr;       // [SKY_N], zeroed by the launch
  double* true_elevation;        // [n_pixels]
  uint8_t* status;               // [n_pixels]
  uint32_t* steps;               // [n_pixels] or null
};
// f: the frame of the context's setting (prepare_frame); only its atmosphere, earth shape and straight_rays are read.
// column: [n_pixels], the "sky light" march with its column plane; null: plain sky rays
void launch_sky_march(const Frame& f, const SkyJob& job, double* column, hipStream_t stream, hipEvent_t ev_compacted);

struct SkyBodiesJob {
  size_t n_pixels;
  const double* azimuth;        // [n_pixels]
  const double* true_elevation; // [n_pixels]
  const uint8_t* status;        // [n_pixels]
  uint8_t* body;                // [n_pixels]
  uint8_t* rgb;                 // [n_pixels][3] or null
  uint32_t n_bodies;            // 0 .. SKY_BODIES_MAX
  SkyBodyDev bodies[SKY_BODIES_MAX];
  uint8_t colour[SKY_BODIES_MAX][4];
};
void launch_sky_bodies(const SkyBodiesJob& job, hipStream_t stream);

struct SkyShadeJob {
  size_t n_pixels;
  const double* azimuth;        // [n_pixels]
  const double* true_elevation; // [n_pixels]
  const uint8_t* status;        // [n_pixels]
  const double* column;         // [n_pixels]
  uint8_t* body;                // [n_pixels]
  uint8_t* rgb;                 // [n_pixels][3]
  uint32_t n_bodies;            // 0 .. SKY_BODIES_MAX
  SkyBodyDev bodies[SKY_BODIES_MAX];
  SkyShadeDev shade;
};
void launch_sky_shade(const SkyShadeJob& job, hipStream_t stream);

struct SkyTableJob {
  SkyLattice lat;
  double step, top, floor;
  int32_t m;
  unsigned long long* ctr; // [SKY_N], zeroed by the launch
  double* T;               // [n_alt][n_el]
  uint8_t* S;              // [n_alt][n_el]
  uint32_t* tail;          // [n_alt]
};
// the march, then (after ev_marched, where one is given) the tails
void launch_sky_table(const Frame& f, const SkyTableJob& job, hipStream_t stream, hipEvent_t ev_marched);
// out[i] = apparent(h[i], t[i]) over `tab`, or t[i] itself with straight rays
void launch_sky_apparent(const SkyTable& tab, bool straight, size_t n, const double* h, const double* t, double* out, hipStream_t stream);

} // namespace atmrt

#if defined(ATMRT_SKY_KERNELS)
#include "atmrt_device.h"

namespace atmrt {

__global__ __launch_bounds__(256) void k_sky_compact(SkyJob j) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = p < j.n_pixels;
  const bool sky = in && j.hit_count[p] == 0;
  wave_compact_append(sky, (uint32_t)p, j.list, &j.ctr[SKY_LIST]); // every lane of the wavefront
  if (in && !sky) {
    j.true_elevation[p] = dm_from_bits(0x7ff8000000000000ULL);
    j.status[p] = ATMRT_SKY_NONE;
    if (j.steps) j.steps[p] = 0;
  }
}

constexpr int SKY_WAVES = 4; // wavefronts per block

struct SkyLane { // what a lane's march gives; the doubles are NaN unless the ray EXITed (column: LIGHT only)
  int status, steps;
  double true_elevation, column;
};

// One lane of a wavefront from (h0, elevation_deg) to its result: sky_march_one<CUBIC, LIGHT> with the wavefront's loop.  A lane
// that is not live, or whose elevation does not march, is decided from the start.
template <bool CUBIC, bool LIGHT>
__device__ __forceinline__ SkyLane sky_lane(const Frame& f, double step, double top, double floor, int32_t m, double h0, double elevation_deg, bool live) {
  const bool sph = f.earth.spherical != 0, straight = f.p.straight_rays != 0;
  const double radius = f.earth.shape_radius;
  const bool marches = sky_marches(elevation_deg);
  Stepper s;
  stepper_init(s, sph, radius, h0, dm_to_radians(elevation_deg));
  int status = marches ? ATMRT_SKY_INSIDE : ATMRT_SKY_LOST, steps = 0;
  bool decided = !live || !marches;
  double h_prev = h0, q_prev = 0.0, column = 0.0;
  if constexpr (LIGHT) q_prev = sky_refractivity<CUBIC>(*f.atm, h0);
  for (int i = 1; i <= m; i++) {
    if (!decided) {
      const RayState st = stepper_next<CUBIC>(s, *f.atm, sph, radius, straight, step);
      steps = i;
      const int d = sky_step_status(st.h, floor, top);
      if constexpr (LIGHT) {
        if (d != ATMRT_SKY_LOST && d != ATMRT_SKY_GROUND) {
          const double q = sky_refractivity<CUBIC>(*f.atm, st.h);
          column = sky_column_add(sph, radius, step, column, h_prev, q_prev, st.h, q);
          h_prev = st.h, q_prev = q;
        }
      }
      if (d) {
        status = d;
        decided = true;
      }
    }
    if (__all(decided)) break;
  }
  const double nan = dm_from_bits(0x7ff8000000000000ULL);
  const bool exited = status == ATMRT_SKY_EXIT; // never a lane that is not live
  return SkyLane{status, steps, exited ? sky_true_elevation(s, sph, radius, straight, elevation_deg) : nan, LIGHT && exited ? column : nan};
}

// the counts of a wavefront's lanes: one atomic per wavefront and counter (every lane of the wavefront calls)
__device__ __forceinline__ void sky_count(unsigned long long* ctr, int lane, bool live, const SkyLane& r) {
  const unsigned long long n_exit = wave_sum(live && r.status == ATMRT_SKY_EXIT ? 1ull : 0ull), n_ground = wave_sum(live && r.status == ATMRT_SKY_GROUND ? 1ull : 0ull);
  const unsigned long long n_inside = wave_sum(live && r.status == ATMRT_SKY_INSIDE ? 1ull : 0ull), n_lost = wave_sum(live && r.status == ATMRT_SKY_LOST ? 1ull : 0ull);
  const unsigned long long n_steps = wave_sum((unsigned long long)r.steps);
  if (lane == 0) {
    if (n_exit) atomicAdd(&ctr[SKY_EXIT], n_exit);
    if (n_ground) atomicAdd(&ctr[SKY_GROUND], n_ground);
    if (n_inside) atomicAdd(&ctr[SKY_INSIDE], n_inside);
    if (n_lost) atomicAdd(&ctr[SKY_LOST], n_lost);
    if (n_steps) atomicAdd(&ctr[SKY_STEPS], n_steps);
  }
}

// What the two list kernels do: wavefront w takes group w of the list (or of the call's rays), from its end with j.reverse; a lane
// past the end marches nothing and stores nothing.  column: the plane of a LIGHT march.
template <bool CUBIC, bool LIGHT>
__device__ __forceinline__ void sky_list_march(const Frame& f, const SkyJob& j, double* column) {
  const int lane = threadIdx.x & 63;
  const size_t wave = (size_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * SKY_WAVES + (threadIdx.x >> 6)));
  const size_t n = j.list ? (size_t)j.ctr[SKY_LIST] : j.n_pixels;
  const size_t groups = (n + 63) / 64;
  if (wave >= groups) return; // the whole wavefront
  const size_t first = (j.reverse ? groups - 1 - wave : wave) * 64;
  const bool live = first + lane < n;
  const size_t at = live ? first + lane : n - 1;
  const size_t p = j.list ? (size_t)j.list[at] : at;
  const double elevation_deg = j.elevation_angle[p];
  const SkyLane r = sky_lane<CUBIC, LIGHT>(f, j.step, j.top, j.floor, j.m, j.alt ? *j.alt : j.h0, elevation_deg, live);
  if (live) {
    j.true_elevation[p] = r.true_elevation;
    if constexpr (LIGHT) column[p] = r.column;
    j.status[p] = (uint8_t)r.status;
    if (j.steps) j.steps[p] = (uint32_t)r.steps;
  }
  sky_count(j.ctr, lane, live, r);
}

// Five wavefronts per SIMD: left to itself the allocator takes 106 (Linear) / 118 (Spline) VGPRs, four wavefronts; asked for five it
// fits both variants into 94 without scratch (profiles/sky_resources.txt) — nothing but the stepper lives across the loop.
template <bool CUBIC>
__global__ __launch_bounds__(64 * SKY_WAVES) __attribute__((amdgpu_waves_per_eu(5, 5))) void k_sky_march(Frame f, SkyJob j) {
  sky_list_march<CUBIC, false>(f, j, nullptr);
}

__global__ __launch_bounds__(256) void k_sky_fill_nan(double* plane, size_t n) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < n) plane[p] = dm_from_bits(0x7ff8000000000000ULL);
}

#ifndef ATMRT_SKY_LIGHT_WAVES_PER_EU // (EXTRA=-DATMRT_SKY_LIGHT_WAVES_PER_EU=n: tools/measure_sky_light.py's A/B builds)
#define ATMRT_SKY_LIGHT_WAVES_PER_EU 5
#endif
constexpr int SKY_LIGHT_WAVES_PER_EU = ATMRT_SKY_LIGHT_WAVES_PER_EU;

struct SkyLightJob {
  SkyJob sky;
  double* column; // [n_pixels]
};
// Five wavefronts per SIMD, chosen by measurement: the three doubles that live across the loop beside the stepper do not fit the
// 96 VGPRs of five without three dwords of scratch per lane, and still the march is 5 to 6 % faster than at four wavefronts
// (114 / 126 VGPRs, no scratch): profiles/sky_light_resources.txt, profiles/sky_light.json.
template <bool CUBIC>
__global__ __launch_bounds__(64 * SKY_WAVES) __attribute__((amdgpu_waves_per_eu(SKY_LIGHT_WAVES_PER_EU, SKY_LIGHT_WAVES_PER_EU))) void k_sky_light_march(Frame f, SkyLightJob lj) {
  sky_list_march<CUBIC, true>(f, lj.sky, lj.column);
}

void launch_sky_march(const Frame& f, const SkyJob& job, double* column, hipStream_t stream, hipEvent_t ev_compacted) {
  const size_t n = job.n_pixels;
  (void)hipMemsetAsync(job.ctr, 0, SKY_N * sizeof(unsigned long long), stream);
  if (n && job.hit_count) {
    if (column) hipLaunchKernelGGL(k_sky_fill_nan, dim3(cdiv(n, 256)), dim3(256), 0, stream, column, n);
    hipLaunchKernelGGL(k_sky_compact, dim3(cdiv(n, 256)), dim3(256), 0, stream, job);
  }
  if (ev_compacted) (void)hipEventRecord(ev_compacted, stream);
  if (!n) return;
  const dim3 grid(cdiv(n, 64 * SKY_WAVES)), blk(64 * SKY_WAVES);
  const SkyLightJob light{job, column};
  if (!column && f.atm_cubic) hipLaunchKernelGGL((k_sky_march<true>), grid, blk, 0, stream, f, job);
  else if (!column) hipLaunchKernelGGL((k_sky_march<false>), grid, blk, 0, stream, f, job);
  else if (f.atm_cubic) hipLaunchKernelGGL((k_sky_light_march<true>), grid, blk, 0, stream, f, light);
  else hipLaunchKernelGGL((k_sky_light_march<false>), grid, blk, 0, stream, f, light);
}

__global__ __launch_bounds__(256) void k_sky_shade(SkyShadeJob j) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= j.n_pixels) return;
  uint32_t body = 0;
  if (j.status[p] == ATMRT_SKY_EXIT) {
    uint8_t out[3];
    body = sky_shade_pixel(j.shade, j.bodies, j.n_bodies, j.azimuth[p], j.true_elevation[p], j.column[p], out);
    j.rgb[3 * p] = out[0];
    j.rgb[3 * p + 1] = out[1];
    j.rgb[3 * p + 2] = out[2];
  }
  j.body[p] = (uint8_t)body;
}

void launch_sky_shade(const SkyShadeJob& job, hipStream_t stream) {
  if (!job.n_pixels) return;
  hipLaunchKernelGGL(k_sky_shade, dim3(cdiv(job.n_pixels, 256)), dim3(256), 0, stream, job);
}

__global__ __launch_bounds__(256) void k_sky_bodies(SkyBodiesJob j) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= j.n_pixels) return;
  uint32_t body = 0;
  if (j.status[p] == ATMRT_SKY_EXIT) body = sky_body_of(j.bodies, j.n_bodies, j.azimuth[p], j.true_elevation[p]);
  j.body[p] = (uint8_t)body;
  if (body && j.rgb) {
    j.rgb[3 * p] = j.colour[body - 1][0];
    j.rgb[3 * p + 1] = j.colour[body - 1][1];
    j.rgb[3 * p + 2] = j.colour[body - 1][2];
  }
}

void launch_sky_bodies(const SkyBodiesJob& job, hipStream_t stream) {
  if (!job.n_pixels) return;
  hipLaunchKernelGGL(k_sky_bodies, dim3(cdiv(job.n_pixels, 256)), dim3(256), 0, stream, job);
}

// the march with a per-ray h0: entry at = j * n_el + k of the lattice is the ray (h_j, e_k)
template <bool CUBIC>
__global__ __launch_bounds__(64 * SKY_WAVES) __attribute__((amdgpu_waves_per_eu(5, 5))) void k_sky_table_march(Frame f, SkyTableJob j) {
  const int lane = threadIdx.x & 63;
  const size_t first = (size_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * SKY_WAVES + (threadIdx.x >> 6))) * 64;
  const size_t n = (size_t)j.lat.n_alt * j.lat.n_el;
  if (first >= n) return; // the whole wavefront
  const bool live = first + lane < n;
  const size_t at = live ? first + lane : n - 1;
  const uint32_t row = (uint32_t)(at / j.lat.n_el), k = (uint32_t)(at - (size_t)row * j.lat.n_el);
  const double elevation_deg = sky_lattice_el(j.lat, k);
  const SkyLane r = sky_lane<CUBIC, false>(f, j.step, j.top, j.floor, j.m, sky_lattice_alt(j.lat, row), elevation_deg, live);
  if (live) {
    j.T[at] = r.true_elevation;
    j.S[at] = (uint8_t)r.status;
  }
  sky_count(j.ctr, lane, live, r);
}

// One wavefront per row: lane l of a round looks at the pair (k - 1, k) with k = base - l, from the row's end downward; the first
// pair that does not continue the tail ends it at its k (k = 0 has no entry below it and ends every row).
__global__ __launch_bounds__(64) void k_sky_tail(SkyTableJob j) {
  const uint32_t row = blockIdx.x, n_el = j.lat.n_el;
  const int lane = threadIdx.x;
  const double* T = j.T + (size_t)row * n_el;
  const uint8_t* S = j.S + (size_t)row * n_el;
  uint32_t tail = n_el;
  if (S[n_el - 1] == ATMRT_SKY_EXIT) {
    for (uint32_t base = n_el - 1;; base -= 64) { // wave-uniform
      const bool in = base >= (uint32_t)lane + 1; // k >= 1
      const uint32_t k = in ? base - (uint32_t)lane : 0;
      const bool goes_on = in && S[k - 1] == ATMRT_SKY_EXIT && T[k - 1] < T[k];
      const unsigned long long ends = __ballot(!goes_on);
      if (ends) {
        const uint32_t l = (uint32_t)__ffsll((long long)ends) - 1;
        tail = base >= l ? base - l : 0;
        break;
      }
    }
  }
  if (lane == 0) j.tail[row] = tail;
}

void launch_sky_table(const Frame& f, const SkyTableJob& job, hipStream_t stream, hipEvent_t ev_marched) {
  const size_t n = (size_t)job.lat.n_alt * job.lat.n_el;
  (void)hipMemsetAsync(job.ctr, 0, SKY_N * sizeof(unsigned long long), stream);
  const dim3 grid(cdiv(n, 64 * SKY_WAVES)), blk(64 * SKY_WAVES);
  if (f.atm_cubic) hipLaunchKernelGGL((k_sky_table_march<true>), grid, blk, 0, stream, f, job);
  else hipLaunchKernelGGL((k_sky_table_march<false>), grid, blk, 0, stream, f, job);
  if (ev_marched) (void)hipEventRecord(ev_marched, stream);
  hipLaunchKernelGGL(k_sky_tail, dim3(job.lat.n_alt), dim3(64), 0, stream, job);
}

__global__ __launch_bounds__(256) void k_sky_apparent(SkyTable tab, int straight, size_t n, const double* h, const double* t, double* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = straight ? t[i] : sky_apparent(tab, h[i], t[i]);
}

void launch_sky_apparent(const SkyTable& tab, bool straight, size_t n, const double* h, const double* t, double* out, hipStream_t stream) {
  if (!n) return;
  hipLaunchKernelGGL(k_sky_apparent, dim3(cdiv(n, 256)), dim3(256), 0, stream, tab, straight ? 1 : 0, n, h, t, out);
}

} // namespace atmrt
#endif
