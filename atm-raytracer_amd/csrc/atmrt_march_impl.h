// atmrt_march_impl.h — Rectilinear generator on gfx950: the per-pixel march (RK4 ray + geodesic point + terrain gather per step),
// its trace-point epilogue and the general tracer for scenes with objects.  Included by four translation units
// (atmrt_march_{linear,spline}.hip, atmrt_trace_{linear,spline}.hip) that instantiate the launchers of the lean march / of the
// general tracer for atmospheres without / with Spline segments, so the heavy template variants (4 + 2 modes x 4 DirectionalCalc
// kinds x 2) compile in parallel.
#pragma once
// exp/log tables of detmath.h in LDS for this translation unit (6 KB per block): every kernel below calls stage_dm_tables() first.
// The look-ups sit on the dependent chain of each n(h) evaluation; from LDS they cost ~1/3 of an L1 hit.
#if defined(__HIP_DEVICE_COMPILE__)
#define DM_TABLES_LDS atmrt_dm_tables_lds
__shared__ double atmrt_dm_tables_lds[768];
#endif
// In this translation unit the per-object collision code and the proximity filter of a sample are called out of line: they run at
// a few per cent of the marching steps, and inlined they push the general tracer to 256 VGPRs (2 waves per SIMD; config 5:
// 559 ms inlined at 2 waves, 507 ms out of line at 3 waves, 680 ms at 4 waves with the spills that needs).
#ifndef ATMRT_OBJ_FN
#define ATMRT_OBJ_FN __attribute__((noinline))
#endif
#include <cstdlib>
#include <cstring>
#include "atmrt_device.h"

namespace atmrt {


// ---------------------------------------------------------------------------------------------
// Rectilinear generator: one ray per lane — per-step geodesic point, bilinear terrain gather
// (4 int16 posts = 8 B), sign test, RK4 step (rectilinear.rs:161-185 driving utils.rs:201-289).
// MODE 0: opaque, write the dense first hit.  MODE 1: count.  MODE 2: write packed trace points.
// MODE 3: scenes with objects — count like MODE 1 (slots pixel-indexed, in the general tracer's arena), but give up on a ray
// (hit_count = OBJECT_RAY) at the first step that can involve an object; those rays are traced by k_rect_trace afterwards.
// ---------------------------------------------------------------------------------------------
// The march only records WHERE the ray crossed the terrain (step index + ray elevation and path
// length at the two bracketing samples); k_rect_finalize rebuilds the geodesic points, the four
// finite-difference terrain lookups per sample and the interpolation.  Keeping the hit epilogue out
// of the march keeps the RK4 loop at ~135 VGPRs without scratch.

// Wavefronts per SIMD.  Rounds 1-3 ran 4 (<= 128 VGPRs, no scratch): the loop then was saturated by its own issue slots (VALU 99.7 %
// busy) and a fifth wavefront bought 1.5 % for 40 x the algorithmic stores in scratch traffic.  With round 4's evaluation order
//  a ray-step is 752 lane-instructions instead of 1,154 and the four wavefronts also wait on their own dependency
// chains (busy 91.7 %): 5 per SIMD (96 VGPRs, 116 B/lane of scratch for state that is touched once per ray) measure 173.3 against
// 179.3 ms for the headline frame, 6 per SIMD (80 VGPRs) 175.9.  History: 402 ms (3 waves) / 366 (4) / 419 (5) in round 1.
#ifndef ATMRT_MARCH_WAVES
#define ATMRT_MARCH_WAVES 5
#endif
// Scenes with objects (MODE 3).  The general tracer pays for its generality at every step (candidate lists, step lists,
// collision geometry: 3 waves per SIMD), yet a step can only involve an object while the ray is inside the distance interval of a
// candidate object AND its segment enters that object's height band — for most rays never.  So the lean march runs first, with one
// candidate list PER WAVEFRONT in LDS: the wavefront's 64 rays are adjacent pixels of one row, they advance through the same
// distances x (x = 0 + step + ... is the same sum for every ray), and the list holds, for every object that is a candidate of any
// of its rays, the union of those rays' intervals [lo, hi] and the object's height band.  The per-step test is a wave-uniform
// scan of that list, executed only between the list's next interval start and the end of the intervals it is inside.  The union
// is a superset of every ray's own candidates (same candidate_interval as ray_candidates), the band test is the tracer's own
// (object_out_of_band), so a ray that is never flagged has provably no step with an object: its terrain-only result is final.
constexpr uint32_t OBJECT_RAY = 0xffffffffu; // hit_count of a ray left to k_rect_trace

// Wave priority against the drain at the end of a launch.  The SIMD issues oldest-wave-first, so the four wavefronts that share a
// SIMD in the LAST resident set do not finish together: the favoured one runs at its dependency-chain speed, and the last one
// ends alone on a SIMD it cannot fill (a launch of uniform 2000-step rays takes 4.02 ms per workgroup-per-CU + 3.5 ms: one resident
// set 19.5 ms, not 16.1).  A wavefront therefore starts at priority 3 and drops one level every DRAIN_PRIO_BAND steps: the
// wavefronts of a SIMD are kept within a band of one another and the last set drains together (16.8 ms; a shard of the headline at
// 8 GPUs 41.5 -> 39.0 ms).  In a launch of many resident sets the drain is 1 % and the priorities cost about as much, so only small
// launches use them: the kernel is compiled in both variants (DRAIN) and the frame's plan picks one by the size and kind of the
// grid (atmrt_march_plan.h: MarchRoute::GridDrain, march_drain_max_blocks; launch_march_grid below).
constexpr int DRAIN_PRIO_BAND = 512;
#ifndef ATMRT_MARCH_BLOCK_SMALL
#define ATMRT_MARCH_BLOCK_SMALL 256 // workgroup size of the small-launch (DRAIN) variant
#endif

// The DRAIN variant also runs 5 wavefronts per SIMD (96 VGPRs, 136 B of scratch per lane) instead of 4 (127 VGPRs, none): a shard's
// long wavefronts are 1.37 resident sets of 4096 but 1.09 sets of 5120, so far fewer of them are left to run on half-empty SIMDs at
// the end (mean occupancy of a shard launch at 8 GPUs 0.83, VALU busy 0.86 with 4 per SIMD): 8 x 39.3 -> 8 x 36.2 ms, 4 x 73.5 ->
// 4 x 71.2.  (Round 4: the plain and the sliced march run 5 per SIMD too, ATMRT_MARCH_WAVES.)
#ifndef ATMRT_MARCH_WAVES_SMALL
#define ATMRT_MARCH_WAVES_SMALL 5
#endif
// a crossing beyond the slots of its pixel: one record in the arena (0.7 % of the headline's pixels at terrain_alpha 0.5 have any)
static __device__ __forceinline__ void overflow_append(const OverflowArena& ovf, unsigned long long* counters, uint32_t p, unsigned ordinal,
                                                       uint32_t step, double re0, double pl0, double re1, double pl1) {
  if (!ovf.cap) return;
  const unsigned long long k = atomicAdd(&counters[CTR_OVERFLOW_RECORDS], 1ull);
  if (k < ovf.cap) {
    ovf.pixel[k] = p;
    ovf.ordinal[k] = ovf.color_tag ? ordinal | OVERFLOW_LEAN : ordinal;
    ovf.step[k] = step;
    rec_store(ovf, k, re0, pl0, re1, pl1);
    if (ovf.color_tag) ovf.color_tag[k] = ATMRT_COLOR_TERRAIN;
  }
}

// The escape test itself, escapes(), is atmrt_device.h's: the shadow march (atmrt_shadow.h) runs it too.
// MODE 3: the floor also clears the height band [vlo, vhi] of every object in the wavefront's candidate list (a ray can only meet
// an object of that list); + 1 m against the rounding of the samples
static __device__ __forceinline__ double escape_floor_objects(double floor, const double* w_vhi, int n_e) {
  for (int q = 0; q < n_e; q++) floor = w_vhi[q] + 1.0 > floor ? w_vhi[q] + 1.0 : floor;
  return floor;
}
// the rays that escaped and the steps they were credited (CTR_ESCAPED_RAYS / CTR_ESCAPED_STEPS), one atomic per wavefront
static __device__ __forceinline__ void escape_count(unsigned long long* counters, int esc_credit) {
  const unsigned long long rays = wave_sum(esc_credit >= 0 ? 1ull : 0ull);
  const unsigned long long credit = wave_sum(esc_credit > 0 ? (unsigned long long)esc_credit : 0ull);
  if ((threadIdx.x & 63) == 0 && rays) {
    atomicAdd(&counters[CTR_ESCAPED_RAYS], rays);
    atomicAdd(&counters[CTR_ESCAPED_STEPS], credit);
  }
}

// ---------------------------------------------------------------------------------------------
// MODE 3, the rare step.  Until round 3 a ray of the lean march that reached a step which could involve an object was abandoned
// there and traced again from x = 0 by the general tracer k_rect_trace — 11 % of config 5's rays, 38 ms of 333 for the frame and a
// launch of under two wavefronts per SIMD for a column tile (12 ms at the speed of a lone wavefront's dependency chain whatever the
// tile's size: config 5 did not strong-scale, 0.73 at 8 tiles).  Yet the steps that involve an object are a handful per such ray
// (the step must lie inside an object's distance interval AND enter its height band): 0.05 % of all steps.  So the lean march now
// keeps the ray and hands only THAT STEP to an out-of-line function that does what get_single_pixel does for a step in full
// (utils.rs:211-285): both samples' geodesic points and terrain heights, the terrain crossing, the proximity filter of the two
// samples over the wavefront's candidate objects (TerrainData::from_lat_lon, utils.rs:74-80), the collisions (frustum.rs:18-101,
// billboard.rs), the stable sort by `prop`, the emission into the tracer's slot arena / overflow arena — the general tracer's own
// building blocks (step_begin, step_object_impl, step_commit_count), so the trace points are the tracer's to the bit.  The function is
// called under divergent control flow a few times per flagged ray; it reads the frame and the sinks through pointers to copies in
// HBM (a kernel argument cannot be addressed) and is built, like every unit that calls device functions, without interprocedural
// register allocation (Makefile CALL_EXTRA).  Only a wavefront whose candidate list overflows (more than WAVE_CAND objects) or an
// earth model without the geometric pre-filter still leaves its rays to k_rect_trace.
struct ObjectStepIO {      // one lane's step, in scratch at the call site
  DirCalc c;
  double d0, sx, re0, sh, pl0, path_length; // the two samples: stepper x, ray elevation, path length
  double diff1;            // out: ray - terrain at the newer sample (the next step's diff0)
  uint32_t pixel;
  int32_t step_index;      // of the older sample
  unsigned count;          // in / out: trace points of the pixel so far
  int32_t finish;          // out: the ray ends with this step (utils.rs:237-239, 274-285)
};
template <int CALC>
static __device__ __attribute__((noinline)) void object_step_impl(const Frame* __restrict__ fg, const StepSinks* __restrict__ sk,
                                                                  ObjectStepIO* io, const double* w_lo, const double* w_hi,
                                                                  const int* w_obj, int n_e) {
  Earth e = fg->earth;
  e.calc = CALC;
  const DirCalc& c = io->c;
  const double d0 = io->d0, sx = io->sx, re0 = io->re0, sh = io->sh, pl0 = io->pl0, path_length = io->path_length;
  double lat0, lon0, lat1, lon1;
  coords_at_step(*fg, e, c, io->step_index, d0, lat0, lon0); // d0 = xs[step_index], sx = xs[step_index + 1] (march_steps)
  coords_at_step(*fg, e, c, io->step_index + 1, sx, lat1, lon1);
  const double te0 = terrain_elev_or_zero(fg->tv, lat0, lon0), te1 = terrain_elev_or_zero(fg->tv, lat1, lon1);
  const double diff1 = re0 - te0, diff2 = sh - te1;
  StepHits hits;
  step_begin(hits, diff1 * diff2 < 0.0, diff1, diff2, fg->p.terrain_alpha == 1.0); // utils.rs:222
  // the objects this step tests, ascending: those close to either sample (utils.rs:241-250) whose height band the segment enters
  const Vec3 pos1 = as_cartesian(e, lat0, lon0, re0), pos2 = as_cartesian(e, lat1, lon1, sh);
  const LatLonTrig t0 = latlon_trig(e, lat0, lon0), t1 = latlon_trig(e, lat1, lon1);
  const double x_prev = sx - fg->p.simulation_step * 1.000001;
  for (int q = 0; q < n_e; q++) {
    if (w_hi[q] < x_prev || w_lo[q] > sx) continue; // the wavefront's interval of this object does not reach the step
    const int j = w_obj[q];
    const ObjectDev& o = fg->objects[j];
    if (object_out_of_band(o, re0, sh)) continue;
    if (!(object_is_close(e, o, t0) || object_is_close(e, o, t1))) continue;
    step_object_impl(hits, fg->objects, fg->textures, j, pos1, pos2);
  }
  // emission: the counting pass of the general tracer (k_rect_trace<false>)
  step_commit_count<true>(hits, *sk, io->pixel, io->count, io->step_index, (size_t)fg->wl * fg->h,
                          StepGeom{lat0, lon0, re0, d0, pl0, lat1, lon1, sh, sx, path_length});
  atomicAdd(&sk->counters[CTR_OBJECT_STEPS], 1ull); // statistics (atmrt_last_stats().object_steps)
  io->count += (unsigned)hits.n;
  io->finish = hits.finish ? 1 : 0;
  io->diff1 = diff2;
}

#ifdef ATMRT_TIMELINE
// Experiment hook (tools/measure_march_timeline.py; never defined in the product build): start / end time and steps of every
// wavefront (k_rect_march_queue: of every 64-pixel group) of the last k_rect_march launch, read back through atmrt_debug_timeline.
// TIMELINE_WAVES covers the whole headline frame (4096 x 2048 / 64 = 131072 groups) twice over.
constexpr size_t TIMELINE_WAVES = 262144;
static __device__ unsigned long long g_timeline[3 * TIMELINE_WAVES];
static __device__ uint32_t g_timeline_estimate[TIMELINE_WAVES]; // k_rect_march_queue: the group's estimate | 1 << 31: marched by a long wavefront
static __device__ unsigned long long g_slices[4 * 262144 + 8]; // [0] = count; then {group | i0 << 32, start, end, wave | hw_id << 32}
static __device__ __forceinline__ int timeline_wave_max(int v) {
  for (int o = 32; o; o >>= 1) {
    const int u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}
#endif

// Where a lean march (k_rect_march, k_rect_march_first / _cont) leaves its results, by MODE
struct MarchSinks {
  int32_t* hit_step;    // MODE 0: [plane] step of the first crossing, or -1; MODE 3: [plane] 1 = the ray is left to the general tracer
                        // (which voids the ray's overflow records, k_scatter_overflow)
  RectRec rec;          // MODE 0: [plane]; MODE 1, 3: the slot arena (slot_index); MODE 2: the pixel-ordered list
  uint32_t* step;       // MODE 1 - 3: the step of every entry of rec
  OverflowArena ovf;    // MODE 1, 3: crossings beyond the slots
  uint32_t* slot_tag;   // MODE 3: the slot arena's colour tags (the march writes TERRAIN)
  // MODE 2: the crossings of pixel p are entries hit_offset[p] ... of the list; the launch may be restricted to a list of pixels
  // (those whose crossings did not fit the slots of the counting march)
  const uint64_t* hit_offset;
  uint32_t* list_pixel;
  const uint32_t* pixel_list; // or null: every pixel of the plane
  uint32_t n_list;
  // MODE 3: copies of the frame and of the tracer's arenas in HBM, for the out-of-line object step (object_step_impl)
  const Frame* frame_dev;
  const StepSinks* step_sinks_dev;
};

// Pixel p of the frame -> its ray: direction and elevation angle, geodesic calculator, stepper at the observer
static __device__ __forceinline__ void rect_ray_setup(const Frame& f, const Earth& e, size_t p, double alt, double& direction, double& elevation,
                                                      DirCalc& c, Stepper& s) {
  const int y = (int)(p / (size_t)f.wl), x = (int)(p % (size_t)f.wl);
  rect_ray_params(f.p, f.ph, f.c0 + x, y, direction, elevation);
  dircalc_new(e, f.p.position.latitude, f.p.position.longitude, dm_to_degrees(direction), c);
  stepper_init(s, e.spherical != 0, e.shape_radius, alt, elevation);
}
static __device__ __forceinline__ void store_ray_angles(const DensePlanes& out, size_t p, double direction, double elevation) {
  out.azimuth[p] = dm_to_degrees(direction); // not wrapped, rectilinear.rs:110-113
  out.elevation_angle[p] = dm_to_degrees(elevation);
}

// MODE 3: the candidate list of one wavefront (arrays in LDS) and the distance at which the march looks at it next
struct WaveList {
  double *lo, *hi, *vlo, *vhi; // the union of the rays' intervals [lo, hi] of an object and its height band [vlo, vhi]
  int* obj;
  int n;
  double x_wake;
};
// the lists of a workgroup of WAVES wavefronts: a __shared__ object of the kernel (nothing of it is touched unless MODE == 3)
template <int MODE, int WAVES>
struct WaveListLds {
  static constexpr int W = MODE == 3 ? WAVES : 1, N = MODE == 3 ? WAVE_CAND : 1;
  double lo[W][N], hi[W][N], vlo[W][N], vhi[W][N];
  int obj[W][N];
  __device__ __forceinline__ WaveList wave(int wv) { return WaveList{lo[wv], hi[wv], vlo[wv], vhi[wv], obj[wv], 0, dm_inf()}; }
};
// Builds the list of this wavefront from the rays of its active lanes (c: this lane's); false: the wavefront's rays are left to the
// general tracer (no geometric pre-filter for this earth model: every ray tests every object; or more than WAVE_CAND candidates)
template <int CALC>
static __device__ __forceinline__ bool wave_list_build(const Frame& f, const Earth& e, const DirCalc& c, WaveList& wl) {
  if (!candidates_supported<CALC>(e)) return false;
  const Vec3 nrm = track_normal<CALC>(c);
  int w_n = 0;
  for (int j = 0; j < f.n_objects; j++) { // wave-uniform loop; the object's fields are scalar loads
    double lo = dm_inf(), hi = -dm_inf();
    double l, h;
    if (candidate_interval<CALC>(e, c, nrm, f.objects[j], true, l, h)) lo = l, hi = h;
    unsigned long long holders = __ballot(lo <= hi); // the active lanes for which the object is a candidate
    if (holders) {
      double wlo = dm_inf(), whi = -dm_inf();
      for (; holders; holders &= holders - 1) { // union of their intervals (reads active lanes only)
        const int src = __builtin_ctzll(holders);
        const double l2 = __shfl(lo, src, 64), h2 = __shfl(hi, src, 64);
        wlo = l2 < wlo ? l2 : wlo;
        whi = h2 > whi ? h2 : whi;
      }
      if (w_n < WAVE_CAND && (threadIdx.x & 63) == 0) {
        wl.lo[w_n] = wlo;
        wl.hi[w_n] = whi;
        wl.vlo[w_n] = f.objects[j].vlo;
        wl.vhi[w_n] = f.objects[j].vhi;
        wl.obj[w_n] = j;
      }
      w_n++;
    }
  }
  wl.n = w_n < WAVE_CAND ? w_n : WAVE_CAND;
  // lane 0 wrote the list, every lane of the wavefront reads it from here on: DS operations of one wave issue in order, but the
  // dependence has to exist for the compiler too — a wavefront-scope release / acquire pair around a wave barrier
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  for (int q = 0; q < wl.n; q++) // first interval that is not behind the start
    if (wl.hi[q] >= 0.0) wl.x_wake = wl.lo[q] < wl.x_wake ? wl.lo[q] : wl.x_wake;
  return w_n <= WAVE_CAND; // overflowed: the whole wavefront goes to the tracer
}
// The step with the samples at x - step and x (elevations re0, sh) against the list — wave-uniform: x and the list are the same for
// every ray of the wavefront.  Inside an entry's interval and inside its height band: the step may involve that object (true).
// Next wake: the nearest interval start ahead, or the next step while an interval is being crossed.
static __device__ __forceinline__ bool wave_list_wake(WaveList& wl, double x_prev, double sx, double re0, double sh) {
  double next = dm_inf();
  bool object_step = false;
  for (int q = 0; q < wl.n; q++) {
    const double lo = wl.lo[q], hi = wl.hi[q];
    if (hi < x_prev) continue;               // behind the step
    if (lo > sx) {                           // ahead of it
      next = lo < next ? lo : next;
      continue;
    }
    next = sx;                               // being crossed: look again at the next step
    const double vlo = wl.vlo[q], vhi = wl.vhi[q];
    if (!((re0 < vlo && sh < vlo) || (re0 > vhi && sh > vhi))) object_step = true; // object_out_of_band is false
  }
  wl.x_wake = next;
  return object_step;
}

// The state of one ray of the lean march between two steps (SliceState is its form in HBM between two slices)
struct MarchRay {
  Stepper s;
  double sh, path_length;  // the newest sample (its x is s.x): ray elevation, path length
  double diff0, re0, pl0;  // the sample before it: ray - terrain, ray elevation, path length
  int first;               // MODE 0: step of the first crossing, or -1
  unsigned count;          // crossings so far
  uint64_t k;              // MODE 2: the ray's cursor in the pixel-ordered list
};
// what a lane adds to the device counters at the end of its kernel (count_wave_steps)
struct MarchCount {
  unsigned long long steps = 0, lookups = 0;
  int esc_credit = -1; // >= 0: the ray escaped and was credited this many steps (escapes)
};
#ifdef ATMRT_TIMELINE
// the steps the wavefront's loop ran: the most any of its lanes integrated (credited escape steps are not run)
static __device__ __forceinline__ int timeline_wave_steps(const MarchCount& n) {
  return timeline_wave_max((int)n.steps - (n.esc_credit > 0 ? n.esc_credit : 0));
}
// entry w of g_timeline: start, end, and steps | wavefront of its workgroup << 20 | HW_ID[15:0] (wave, simd, pipe, cu, sh, se) << 24 |
// XCC_ID << 40 | wave-steps << 44
static __device__ __forceinline__ void timeline_record(size_t w, unsigned long long t0, unsigned long long steps, int wave_steps) {
  if ((threadIdx.x & 63) != 0 || w >= TIMELINE_WAVES) return;
  g_timeline[3 * w] = t0;
  g_timeline[3 * w + 1] = wall_clock64();
  g_timeline[3 * w + 2] = (steps & 0xfffffull) | ((unsigned long long)((threadIdx.x >> 6) & 15u) << 20) | ((unsigned long long)(__builtin_amdgcn_s_getreg((15 << 11) | 4) & 0xffffu) << 24) |
                          ((unsigned long long)(__builtin_amdgcn_s_getreg((3 << 11) | 20) & 0xfu) << 40) |
                          ((unsigned long long)(wave_steps & 0xfffff) << 44);
}
#endif
enum MarchEnd {
  MARCH_ENDED,   // the ray has finished
  MARCH_ON,      // the slice has ended, the ray marches on
  MARCH_GIVEN_UP // MODE 3: the ray is left to the general tracer
};

// The start state and the first sample (PathIterator::next at the start state); false: an empty stream (the reference would panic)
static __device__ __forceinline__ bool march_begin(const Frame& f, const Earth& e, const DirCalc& c, double alt, MarchRay& r, MarchCount& n) {
  r.sh = r.re0 = alt; // TracingState::new(.., first_path.elev, 0.0, 0.0), utils.rs:208
  r.path_length = r.pl0 = r.diff0 = 0.0;
  r.first = -1;
  r.count = 0;
  if (0.0 > f.p.frame.max_distance || alt < -1000.0) return false;
  double lat, lon;
  coords_at_step(f, e, c, 0, 0.0, lat, lon);
  r.diff0 = alt - terrain_elev_or_zero(f.tv, lat, lon);
  n.lookups++;
  return true;
}

// A crossing between the ray's last two samples, MODE 1 - 3 (MODE 0 keeps the four values in registers: march_finish)
template <int MODE>
static __device__ __forceinline__ void crossing_store(const Frame& f, const MarchSinks& sinks, unsigned long long* counters, size_t p, MarchRay& r,
                                                      uint32_t step) {
  if (MODE == 2) {
    sinks.step[r.k] = step;
    sinks.list_pixel[r.k] = (uint32_t)p;
    rec_store(sinks.rec, r.k, r.re0, r.pl0, r.sh, r.path_length);
    r.k++;
  } else if (r.count < (unsigned)RECT_SLOTS) {
    const size_t q = slot_index<MODE == 3 ? SlotLayout::PixelMajor : SlotLayout::SlotMajor>(p, r.count, (size_t)f.wl * f.h);
    sinks.step[q] = step;
    if (MODE == 3) sinks.slot_tag[q] = ATMRT_COLOR_TERRAIN;
    rec_store(sinks.rec, q, r.re0, r.pl0, r.sh, r.path_length);
  } else {
    overflow_append(sinks.ovf, counters, (uint32_t)p, r.count, step, r.re0, r.pl0, r.sh, r.path_length);
  }
}

// THE step loop of the lean march: steps i0 + 1 ... of ray p, whose state is in registers.  SLICED: at most `slice` steps
// (k_rect_march_first / _cont), else to the end of the ray (k_rect_march; a whole-ray march is a slice that never ends).  DRAIN: the
// small-launch variant of k_rect_march (the priority ladder; object steps out of line, as in the slices).
template <int MODE, int CALC, bool CUBIC, bool SLICED, bool DRAIN>
static __device__ __forceinline__ MarchEnd march_steps(const Frame& f, const Earth& e, const DirCalc& c, MarchRay& r, MarchCount& n, int i0, int slice,
                                                       const MarchSinks& sinks, unsigned long long* counters, size_t p, WaveList& wl, int bin) {
  const bool sph = e.spherical != 0;
  const double radius = e.shape_radius;
  const bool straight = f.p.straight_rays != 0;
  const double step = f.p.simulation_step, max_dist = f.p.frame.max_distance;
  const double skip_above = f.tv.skip_above;
  const bool opaque = f.p.terrain_alpha == 1.0; // (MODE 0 is launched over opaque terrain only, MODE 1 over translucent only)
  // The terrain ceiling table (Frame::ceil), entry [i][bin] for the sample of step i: `cell` bounds the terrain under THIS sample
  // (never above skip_above), `suffix` under this and every later sample of the ray.  With the table the escape floor is the
  // suffix, the certificate's own lowest altitude (Frame::ceil_floor) and, MODE 3, the objects' bands; without it, Frame::esc_floor.
  const CeilEntry* const ceil = f.ceil;
  const unsigned ceil_stride = (unsigned)f.ceil_layout.n_bins + 1u;
  const double floor_base = f.ceil ? f.ceil_floor : f.esc_floor;
  const double esc_floor = MODE == 3 ? escape_floor_objects(floor_base, wl.vhi, wl.n) : floor_base;
  const int i_end = i0 + slice;
  double sx = r.s.x, lat, lon;
  for (int i = i0 + 1;; i++) {
    if (DRAIN && (i & (DRAIN_PRIO_BAND - 1)) == 0) { // see DRAIN_PRIO_BAND
      const int band = i / DRAIN_PRIO_BAND;
      if (band == 1) __builtin_amdgcn_s_setprio(2);
      else if (band == 2) __builtin_amdgcn_s_setprio(1);
      else if (band == 3) __builtin_amdgcn_s_setprio(0);
    }
    // this step's entry of the table, asked for ahead of the RK4 stages that hide its latency (one 8-byte load per lane; the rays
    // of a wavefront are in step, so the row is wave-uniform, and their bins are a handful of neighbours: one or two cache lines)
    double skip_i = skip_above, floor_i = esc_floor;
    if (ceil) {
      const int iu = SLICED ? __builtin_amdgcn_readfirstlane(i) : i;
      const CeilEntry ce = ceil[(size_t)(iu < f.march_steps ? iu : f.march_steps) * ceil_stride + (unsigned)bin];
      skip_i = (double)ce.cell;
      floor_i = (double)ce.suffix > esc_floor ? (double)ce.suffix : esc_floor;
    }
    bool tame;
    RayState nx = stepper_next<CUBIC>(r.s, *f.atm, sph, radius, straight, step, tame);
    if (straight) tame = __all(calc_dist_in_band(*f.atm, r.sh) && calc_dist_in_band(*f.atm, nx.h));
    r.path_length += calc_dist(sph, radius, sx, r.sh, nx.x, nx.h, tame, f.inv_shape_radius);
    sx = nx.x;
    r.sh = nx.h;
    if (sx > max_dist || r.sh < -1000.0 || !(sx <= max_dist)) return MARCH_ENDED; // rectilinear.rs:178 (+ NaN guard)
    // x_prev: a little before the older sample (its x is sx - step up to rounding)
    if (MODE == 3 && sx >= wl.x_wake && wave_list_wake(wl, sx - step * 1.000001, sx, r.re0, r.sh)) {
      // A launch of many resident sets (the whole frame: neither SLICED nor DRAIN) abandons the ray here and leaves it to the general
      // tracer, whose own launch is then large enough to fill the chip (config 5: 38 ms of VALU-saturated work for 11 % of the rays —
      // there is nothing to hide, and the out-of-line steps would only add their call overhead: 308 against 328 ms per frame).
      // A small launch (a column tile of a multi-GPU frame) keeps the ray and does the step out of line: the tracer's launch
      // for a tile would be under two wavefronts per SIMD, 12 ms whatever the tile's size (8 tiles: 54 -> 43 ms).
      if (!SLICED && !DRAIN) return MARCH_GIVEN_UP;
      ObjectStepIO io; // this lane's step in full, out of line (object_step_impl above); the others wait
      io.c = c;
      io.d0 = f.xs[i - 1]; // the stepper's x of the older sample: 0 + step + ... (the same additions as xs)
      io.sx = sx, io.re0 = r.re0, io.sh = r.sh, io.pl0 = r.pl0, io.path_length = r.path_length;
      io.pixel = (uint32_t)p, io.step_index = i - 1, io.count = r.count;
      object_step_impl<CALC>(sinks.frame_dev, sinks.step_sinks_dev, &io, wl.lo, wl.hi, wl.obj, wl.n);
      r.count = io.count;
      n.lookups += 2;
      n.steps++;
      if (io.finish) return MARCH_ENDED;
      r.diff0 = io.diff1;
      r.re0 = r.sh;
      r.pl0 = r.path_length;
      if (SLICED && i == i_end) return MARCH_ON;
      continue;
    }
    // A sample above every post of the mosaic is above the terrain, whatever its geodesic point: ray - terrain is positive and
    // only its SIGN enters the test below (the epilogue rebuilds the bracketing samples in full), so the geodesic point and
    // the lookup are skipped and any positive number stands for the difference.  Wavefronts are 64 columns of one row: sky
    // rows leave the terrain's height range together.  NaN heights take the full path.
    double diff1 = 1.0;
    if (!(r.sh > skip_i)) {
      // sx = xs[i]: r.s.x starts at 0 (or at xs[i0], slice_save) and only ever advances by x + step (stepper_next_with), the
      // additions of the table.  The rays of a wavefront march in step, so i is the same in every lane; a later slice reads its i0
      // from the group's state (a vector register: every ray still marching was saved with the same step), hence the readfirstlane
      // that makes the table read a scalar load there too.
      const int iu = SLICED ? __builtin_amdgcn_readfirstlane(i) : i;
      coords_at_step(f, e, c, iu, sx, lat, lon);
      diff1 = r.sh - terrain_elev_or_zero(f.tv, lat, lon);
      n.lookups++;
    }
    n.steps++;
    if (r.diff0 * diff1 < 0.0) { // utils.rs:222
      // MODE 0: the record is stored after the march (march_finish): opaque terrain ends the ray here, the four values stay as they are
      if (MODE == 0) r.first = i - 1;
      else crossing_store<MODE>(f, sinks, counters, p, r, (uint32_t)(i - 1));
      r.count++;
      if (opaque) return MARCH_ENDED; // utils.rs:237-239, 283-285
    }
    if (escapes(f, r.s, straight, r.sh, r.re0, floor_i)) { // nothing left to find: credit the rest of the march and leave
      n.esc_credit = f.march_steps - i;
      if (n.esc_credit >= 0) n.steps += (unsigned)n.esc_credit;
      return MARCH_ENDED;
    }
    r.diff0 = diff1;
    r.re0 = r.sh;
    r.pl0 = r.path_length;
    if (SLICED && i == i_end) return MARCH_ON;
  }
}

// the ray has ended with the march: its per-pixel results
template <int MODE>
static __device__ __forceinline__ void march_finish(const DensePlanes& out, const MarchSinks& sinks, unsigned long long* counters, size_t p,
                                                    const MarchRay& r) {
  if (MODE == 0) {
    // ray elevation and path length at the two samples that bracket the crossing
    if (r.first >= 0) rec_store(sinks.rec, p, r.re0, r.pl0, r.sh, r.path_length);
    out.hit_count[p] = r.first >= 0 ? 1u : 0u;
    sinks.hit_step[p] = r.first;
  } else if (MODE != 2) {
    out.hit_count[p] = r.count;
    if (MODE == 3) sinks.hit_step[p] = 0; // the ray stayed with the march: its overflow records count (k_scatter_overflow)
    if (r.count > (unsigned)RECT_SLOTS) atomicAdd(&counters[CTR_OVERFLOW_PIXELS], 1ull);
  }
}

// End of a marching kernel: the wavefront's ray-steps in one atomic — LEAN (the lean march): also its terrain lookups and the
// escape counters.  Returns the wavefront's steps.
template <bool LEAN>
static __device__ __forceinline__ unsigned long long count_wave_steps(unsigned long long* counters, unsigned long long steps,
                                                                      unsigned long long lookups, int esc_credit) {
  steps = wave_sum(steps);
  if (LEAN) lookups = wave_sum(lookups);
  if ((threadIdx.x & 63) == 0 && steps) {
    atomicAdd(&counters[CTR_RAY_STEPS], steps);
    if (LEAN) atomicAdd(&counters[CTR_TERRAIN_LOOKUPS], lookups);
  }
  if (LEAN) escape_count(counters, esc_credit);
  return steps;
}

template <int MODE, int CALC, bool CUBIC, bool DRAIN>
__global__ __launch_bounds__(DRAIN ? ATMRT_MARCH_BLOCK_SMALL : 256, DRAIN ? ATMRT_MARCH_WAVES_SMALL : ATMRT_MARCH_WAVES) void k_rect_march(
    Frame f, DensePlanes out, MarchSinks sinks, unsigned long long* __restrict__ counters) {
#ifdef ATMRT_TIMELINE
  const unsigned long long tl_t0 = wall_clock64();
#endif
  stage_dm_tables();
  if (DRAIN) __builtin_amdgcn_s_setprio(3);
  const size_t plane = (size_t)f.wl * f.h;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = sinks.pixel_list ? tid < sinks.n_list : tid < plane;
  const size_t p = sinks.pixel_list ? (live ? sinks.pixel_list[tid] : 0) : tid;
  MarchCount n;
  __shared__ WaveListLds<MODE, 4> lists;
  if (live) {
    const Earth e = earth_for<CALC>(f);
    const double alt = *f.alt;
    double direction, elevation;
    DirCalc c;
    MarchRay r;
    rect_ray_setup(f, e, p, alt, direction, elevation, c, r.s);
    const int bin = f.ceil ? ceiling_bin(f.ceil_layout, direction) : 0;
    r.k = MODE == 2 ? sinks.hit_offset[p] : 0;
    WaveList wl = lists.wave(threadIdx.x >> 6);
    bool object_ray = MODE == 3 && !wave_list_build<CALC>(f, e, c, wl); // MODE 3: this ray is left to the general tracer
    if (!object_ray && march_begin(f, e, c, alt, r, n))
      object_ray = march_steps<MODE, CALC, CUBIC, false, DRAIN>(f, e, c, r, n, 0, 0, sinks, counters, p, wl, bin) == MARCH_GIVEN_UP;
    if (MODE == 3 && object_ray) { // nothing of this ray counts: k_rect_trace starts it again
      out.hit_count[p] = OBJECT_RAY;
      sinks.hit_step[p] = 1;
      n = MarchCount{};
    } else if (MODE != 2) {
      store_ray_angles(out, p, direction, elevation);
      march_finish<MODE>(out, sinks, counters, p, r);
    }
  }
  if (MODE != 2) {
#ifdef ATMRT_TIMELINE
    const int tl_wave_steps = timeline_wave_steps(n);
#endif
    const unsigned long long steps = count_wave_steps<true>(counters, n.steps, n.lookups, n.esc_credit);
    (void)steps;
#ifdef ATMRT_TIMELINE
    if (MODE == 0) timeline_record(((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, tl_t0, steps, tl_wave_steps);
#endif
  }
}

// ---------------------------------------------------------------------------------------------
// The whole-frame work queue (opaque terrain, MODE 0).  After the escape shortcut and the ceiling table two thirds
// of the headline's wave-steps sit in a few thousand wavefronts around the skyline (250 - 1,700 steps each, against tens for the
// rest), and an ordinary grid deals a SIMD about five of them at random: the sum of five such draws, maximised over 1,024 SIMDs,
// is twice its mean, and the launch ends ragged.  Here the unit of work is an ITEM — a group of 64 consecutive pixels, marched
// whole, by exactly the per-ray code of k_rect_march — and the items come from a queue sorted by estimated length, longest first
// (Frame::ceil_order, k_march_length_estimate).  One persistent workgroup of 16 wavefronts per CU (1024 threads at <= 128 VGPRs: a
// CU holds no second one, so there are 4 wavefronts on every SIMD by construction), and on every SIMD `n_long` of them are LONG:
// they take one item at a time from the head of the queue and run at a raised priority, so a SIMD works on n_long long items at a
// time, each at the speed of its dependency chain, while the SHORT wavefronts (priority 0) fill the issue slots they leave with
// chunks of items from the tail.  A long wavefront sets its priority after every claim by the item it now owns (item_prio; DESIGN.md
// §7.10): 3 where the item's estimate is at least half of the head's (order_steps[0], the longest of the frame), 2 from an eighth,
// 1 below (queue_item_priority) — the long items of a SIMD are served in the order of their length, not by turns.  A chunk is sized
// by the estimate of the item it starts at (queue_chunk_for: a chunk is one wavefront's serial work, and chunks of 16 items that
// reach into the skyline band cost the frame 26 ms instead of 8) and capped by a wavefront's even share of what is left
// (`claimers`: the wavefronts of the launch; queue_chunk_cap), so that chunks shrink to single items as the queue empties and the launch drains in one
// item, not in one chunk.  Which wavefronts are long is elected per SIMD through LDS from the SIMD each wavefront finds itself on,
// not assumed from its index.  No wavefront ever waits for another: claims are single fetch-and-adds.  The claim arithmetic is
// atmrt_march_queue.h; `claim` is zeroed on the stream before every launch.
// ---------------------------------------------------------------------------------------------
template <int CALC, bool CUBIC>
__global__ __launch_bounds__(1024) void k_rect_march_queue(Frame f, DensePlanes out, MarchSinks sinks, unsigned long long* __restrict__ counters,
                                                           const uint32_t* __restrict__ order, const uint32_t* __restrict__ order_steps,
                                                           unsigned long long* __restrict__ claim, uint32_t n_groups, int n_long, bool item_prio,
                                                           uint32_t claimers) {
  __shared__ int simd_rank[4];
  if (threadIdx.x < 4) simd_rank[threadIdx.x] = 0;
  stage_dm_tables(); // (ends in a workgroup barrier: the ranks are zero from here on)
  const int lane = threadIdx.x & 63;
  int rank = 0;
  if (lane == 0) rank = atomicAdd(&simd_rank[(__builtin_amdgcn_s_getreg((15 << 11) | 4) >> 4) & 3], 1); // HW_ID[5:4]: SIMD_ID
  const bool is_long = __builtin_amdgcn_readfirstlane(rank) < n_long;
  if (is_long) __builtin_amdgcn_s_setprio(1);
  const size_t plane = (size_t)f.wl * f.h;
  const Earth e = earth_for<CALC>(f);
  const double alt = *f.alt;
  const uint32_t head_steps = n_groups ? order_steps[0] : 0u; // the longest estimate of the frame: what a long item's estimate is set against
  __shared__ WaveListLds<0, 1> lists;
  // The device counters of this wavefront's items, summed in LDS and added to the frame's once, when the wavefront leaves.  A
  // wavefront marches some thirty items, and four atomics per item on one cache line from each of 4,096 wavefronts are served one
  // after the other while the wavefront's next loads wait behind them.  A slot per counter the lean march
  // adds to: steps, lookups, escaped rays and their credited steps.
  __shared__ unsigned long long wave_counters[16][N_COUNTERS];
  unsigned long long* const my_counters = wave_counters[(threadIdx.x >> 6) & 15];
  if (lane < N_COUNTERS) my_counters[lane] = 0ull;
  // lanes 0 .. 15 wrote the slots, lane 0 adds to them from here on (count_wave_steps): the hand-off of wave_list_build
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  for (;;) {
    // a short wavefront sizes its chunk by the estimate of the item at the tail as it is now and by the items left (a look, not a
    // claim: the tail may have moved on by the time of the claim, towards longer items — by a few claims' worth)
    unsigned long long seen = 0;
    uint32_t chunk = 1;
    if (lane == 0) {
      if (!is_long) {
        const unsigned long long now = __hip_atomic_load(claim, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long tail = now >> 32;
        chunk = tail < (unsigned long long)n_groups
                    ? queue_chunk_for(order_steps[n_groups - 1u - (uint32_t)tail], queue_items_left(now, n_groups), claimers)
                    : 1u;
      }
      seen = atomicAdd(claim, queue_claim_increment(is_long, chunk));
    }
    chunk = (uint32_t)__builtin_amdgcn_readfirstlane((int)chunk);
    seen = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(seen >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)(seen & 0xffffffffull));
    uint32_t first;
    const uint32_t count = queue_claim_items(seen, is_long, chunk, n_groups, first);
    if (!count) break;
    if (is_long && item_prio) { // the priority of the item this wavefront now owns (s_setprio takes an immediate)
      const int prio = queue_item_priority(order_steps[first], head_steps);
      if (prio == 3) __builtin_amdgcn_s_setprio(3);
      else if (prio == 2) __builtin_amdgcn_s_setprio(2);
      else __builtin_amdgcn_s_setprio(1);
    }
    for (uint32_t k = 0; k < count; k++) {
#ifdef ATMRT_TIMELINE
      const unsigned long long tl_t0 = wall_clock64();
#endif
      const uint32_t group = order[is_long ? first : first - k];
      const size_t p = (size_t)group * 64 + lane;
      MarchCount n;
      if (p < plane) { // (also keeps a group number that is none out of every array)
        double direction, elevation;
        DirCalc c;
        MarchRay r;
        rect_ray_setup(f, e, p, alt, direction, elevation, c, r.s);
        const int bin = f.ceil ? ceiling_bin(f.ceil_layout, direction) : 0;
        r.k = 0;
        WaveList wl = lists.wave(0);
        if (march_begin(f, e, c, alt, r, n)) march_steps<0, CALC, CUBIC, false, false>(f, e, c, r, n, 0, 0, sinks, counters, p, wl, bin);
        store_ray_angles(out, p, direction, elevation);
        march_finish<0>(out, sinks, counters, p, r);
      }
#ifdef ATMRT_TIMELINE
      const int tl_wave_steps = timeline_wave_steps(n);
#endif
      const unsigned long long steps = count_wave_steps<true>(my_counters, n.steps, n.lookups, n.esc_credit);
      (void)steps;
#ifdef ATMRT_TIMELINE
      timeline_record(group, tl_t0, steps, tl_wave_steps);
      if (lane == 0 && group < TIMELINE_WAVES) g_timeline_estimate[group] = order_steps[is_long ? first : first - k] | (is_long ? 1u << 31 : 0u);
#endif
    }
  }
  // lane 0 wrote the sums, the lanes 0 .. 15 read them: the same hand-off the other way
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (lane < N_COUNTERS && my_counters[lane]) atomicAdd(&counters[lane], my_counters[lane]);
}

// ---------------------------------------------------------------------------------------------
// Time-sliced march (terrain only: MODE 0 opaque, MODE 1 translucent with the crossings counted into slots) for launches of a few
// resident sets: the column tiles of a multi-GPU frame.
//
// Why.  A tile of the headline at 8 GPUs is 16384 wavefronts of which 7688 march all 2000 steps: 1.5 resident sets of 5120.  The
// hardware hands the second set to whichever CUs drain first (the wavefront timeline of such a launch, tools/
// measure_march_timeline.py: 132 CUs take five more workgroups each, 124 take none and sit idle for the last 5 ms of 34), and no
// order of the grid changes that.  So the unit of work is made smaller than a ray: a SLICE of a group of 64 consecutive pixels.
// k_rect_march_first (an ordinary grid) marches the first `slice` steps of every ray and leaves, for the rays still marching, their
// state in HBM and their group in a FIFO; k_rect_march_cont serves the FIFO with one single-wavefront workgroup per entry: read the
// group's state, march `slice` steps, write it back, append the group again — or count it finished.  All groups advance together,
// the long ones end in the same round, and the launch drains in one slice instead of one ray.
// The state of a ray between two slices: x, a, b, the last sample's height, path length and ray-minus-terrain difference, the
// elevation angle (straight rays), step number, layer hint, crossings so far (MODE 1) — 64 B — and, written once, its geodesic
// calculator (128 B).
//
// FIFO: ctl[0] = entries claimed by readers, ctl[1] = entries written, ctl[2] = groups finished.  Entries are never reused (capacity:
// groups x slices a ray can need) and each has exactly one reader, the workgroup whose claim returned its index.  A reader whose
// entry is still empty waits for it — the writer is a wavefront that is marching, never one that waits — and gives up when every
// group has finished (its index is then beyond the last entry that will ever be written).  SliceState, its layout in HBM and a
// group's candidate list (GroupList, group_list): atmrt_march_plan.h.
constexpr uint32_t SLICE_EMPTY = 0xffffffffu, SLICE_EXIT = 0xfffffffeu;
#ifndef ATMRT_SLICE_WAVES
#define ATMRT_SLICE_WAVES 5 // per SIMD, like the plain march (round 4: 2 x 93.3 -> 90.0 ms, 4 x 47.8 -> 46.2, 8 x 24.24 -> 24.01; 6: slower)
#endif

// the ray marches on after step `step`: what changes from slice to slice (its elevation angle and geodesic calculator are written once)
template <int MODE>
static __device__ __forceinline__ void slice_save(const SliceState& st, size_t p, const MarchRay& r, int step) {
  st.x[p] = r.s.x;
  st.a[p] = r.s.a;
  st.b[p] = r.s.b;
  st.hint[p] = r.s.hint;
  st.sh[p] = r.sh;
  st.pl[p] = r.path_length;
  st.diff0[p] = r.diff0;
  st.step[p] = step;
  if (MODE == 1 || MODE == 3) st.count[p] = r.count;
}

// wave-uniform end of a group's slice: announce the group again, or count it as finished
static __device__ __forceinline__ void slice_requeue(const SliceState& st, uint32_t group, bool alive) {
  const bool again = __any(alive);
  if (again) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); // state before the entry that announces it
  if ((threadIdx.x & 63) == 0) {
    if (again) {
      const unsigned long long t = atomicAdd(&st.ctl[1], 1ull);
      if (t < st.cap) __hip_atomic_store(st.queue + t, group, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      atomicAdd(&st.ctl[2], 1ull);
    }
  }
}

// slice 0 of every group: an ordinary grid (it is short: the launch drains in a fraction of a slice)
template <int MODE, int CALC, bool CUBIC>
__global__ __launch_bounds__(256, ATMRT_SLICE_WAVES) void k_rect_march_first(Frame f, DensePlanes out, MarchSinks sinks,
                                                                             unsigned long long* __restrict__ counters, SliceState st,
                                                                             uint32_t n_groups, int slice) {
#ifdef ATMRT_TIMELINE
  const unsigned long long tl_t0 = wall_clock64();
#endif
  stage_dm_tables();
  const size_t plane = (size_t)f.wl * f.h;
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  MarchCount n;
  bool alive = false;
  __shared__ WaveListLds<MODE, 4> lists; // MODE 3: built here and kept in HBM for the group's later slices
  if (p < plane) {
    const Earth e = earth_for<CALC>(f);
    const double alt = *f.alt;
    double direction, elevation;
    DirCalc c;
    MarchRay r;
    rect_ray_setup(f, e, p, alt, direction, elevation, c, r.s);
    const int bin = f.ceil ? ceiling_bin(f.ceil_layout, direction) : 0;
    store_ray_angles(out, p, direction, elevation);
    WaveList wl = lists.wave(threadIdx.x >> 6);
    const bool object_ray = MODE == 3 && !wave_list_build<CALC>(f, e, c, wl); // MODE 3: the wavefront's rays go to the tracer
    if (!object_ray && march_begin(f, e, c, alt, r, n))
      alive = march_steps<MODE, CALC, CUBIC, true, false>(f, e, c, r, n, 0, slice, sinks, counters, p, wl, bin) == MARCH_ON;
    if (MODE == 3 && st.glist && __any(alive)) { // the group marches on: its list and wake distance for the slices to come
      const GroupList gl = group_list(st.glist, (uint32_t)(p >> 6));
      const int lane = threadIdx.x & 63;
      for (int q = lane; q < wl.n; q += 64) {
        gl.lo[q] = wl.lo[q];
        gl.hi[q] = wl.hi[q];
        gl.vlo[q] = wl.vlo[q];
        gl.vhi[q] = wl.vhi[q];
        gl.obj[q] = wl.obj[q];
      }
      const unsigned long long still = __ballot(alive); // (a lane that ended inside the slice holds an older wake distance)
      if (lane == __builtin_ctzll(still)) {
        gl.n_and_wake[0] = (double)wl.n;
        gl.n_and_wake[1] = wl.x_wake;
      }
    }
    if (MODE == 3 && object_ray) { // left to the general tracer (k_collect_object_rays, k_rect_trace)
      st.step[p] = -1;
      out.hit_count[p] = OBJECT_RAY;
      sinks.hit_step[p] = 1;
      n = MarchCount{};
    } else if (alive) {
      slice_save<MODE>(st, p, r, slice);
      st.ang[p] = r.s.ang;
      st.calc[p] = c;
    } else {
      st.step[p] = -1;
      march_finish<MODE>(out, sinks, counters, p, r);
    }
  }
  if ((p >> 6) < n_groups) slice_requeue(st, (uint32_t)(p >> 6), alive); // (the last block may hold wavefronts past the last group)
  const unsigned long long steps = count_wave_steps<true>(counters, n.steps, n.lookups, n.esc_credit);
  (void)steps;
#ifdef ATMRT_TIMELINE
  if ((threadIdx.x & 63) == 0 && (p >> 6) < 32768) {
    g_timeline[3 * (p >> 6)] = tl_t0;
    g_timeline[3 * (p >> 6) + 1] = wall_clock64();
    g_timeline[3 * (p >> 6) + 2] = steps;
  }
#endif
}

// the later slices: one single-wavefront workgroup per queue entry.  NOT a persistent grid: the SIMD issues oldest-wavefront-first,
// and persistent wavefronts keep their age order for the whole launch — the oldest of a SIMD ran its slices at the speed of its
// dependency chain (0.57 ms), the youngest in 5 ms (measured, tools/measure_slice_timeline.py), groups that met the slow ones fell
// five rounds behind and were a 4.5 ms tail; s_setprio per quarter slice did not change that.  A wavefront that lives for one slice
// starts youngest and ends oldest: every slice sees every rank and the groups stay in step.
template <int MODE, int CALC, bool CUBIC>
__global__ __launch_bounds__(64, ATMRT_SLICE_WAVES) void k_rect_march_cont(Frame f, DensePlanes out, MarchSinks sinks,
                                                                           unsigned long long* __restrict__ counters, SliceState st,
                                                                           uint32_t n_groups, int slice) {
  const size_t plane = (size_t)f.wl * f.h;
  const int lane = threadIdx.x;
  uint32_t item = 0;
  if (lane == 0) {
    const unsigned long long i = atomicAdd(&st.ctl[0], 1ull);
    if (i >= st.cap) {
      item = SLICE_EXIT; // more readers than entries: every entry has its reader already
    } else {
      const uint32_t* entry = st.queue + i;
      // An empty entry means the FIFO has run dry: the launch is in its last round and the groups still marching are held by
      // other wavefronts.  Poll rarely (every few microseconds, backing off to ~50): thousands of idle wavefronts polling two
      // addresses at full rate queue up on one memory channel, in front of the state traffic of the wavefronts still working.
      for (int backoff = 1;; backoff = backoff < 16 ? backoff * 2 : 16) {
        item = __hip_atomic_load(entry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (item != SLICE_EMPTY) break;
        if (__hip_atomic_load(&st.ctl[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= n_groups) {
          item = SLICE_EXIT;
          break;
        }
        __builtin_amdgcn_s_setprio(0);
        for (int k = 0; k < backoff; k++) __builtin_amdgcn_s_sleep(127); // 127 x 64 cycles = 3.4 us
      }
    }
  }
  item = (uint32_t)__shfl((int)item, 0, 64);
  if (item == SLICE_EXIT) return;
  // the group's state, written by the wavefront that announced it — on any XCD: agent scope it has to be (with workgroup-scope
  // fences the step counts of a frame change: stale state out of another XCD's L2)
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  stage_dm_tables();
#ifdef ATMRT_TIMELINE
  const unsigned long long tl_slice_t0 = wall_clock64();
#endif
  MarchCount n;
  const size_t p = (size_t)item * 64 + lane;
  bool alive = false;
  const int32_t i0 = p < plane ? st.step[p] : -1;
  __shared__ WaveListLds<MODE, 1> lists;
  WaveList wl = lists.wave(0);
  if (MODE == 3) { // the group's candidate list back into LDS (what its first slice built)
    const GroupList gl = group_list(st.glist, item);
    wl.n = (int)gl.n_and_wake[0];
    wl.x_wake = gl.n_and_wake[1];
    for (int q = lane; q < wl.n; q += 64) {
      wl.lo[q] = gl.lo[q];
      wl.hi[q] = gl.hi[q];
      wl.vlo[q] = gl.vlo[q];
      wl.vhi[q] = gl.vhi[q];
      wl.obj[q] = gl.obj[q];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  if (i0 >= 0) {
    const Earth e = earth_for<CALC>(f);
    MarchRay r;
    r.s.x = st.x[p];
    r.s.a = st.a[p];
    r.s.b = st.b[p];
    r.s.hint = st.hint[p];
    r.s.h0 = *f.alt;
    r.s.ang = st.ang[p];
    r.sh = r.re0 = st.sh[p];
    r.path_length = r.pl0 = st.pl[p];
    r.diff0 = st.diff0[p];
    const DirCalc c = st.calc[p];
    r.first = -1;
    r.count = MODE == 1 || MODE == 3 ? st.count[p] : 0u;
    // The ray's bin of the ceiling table is a function of its direction alone: a slice derives it again from the pixel (the
    // pinhole arithmetic of rect_ray_setup, once per 128 steps) rather than carry it in the state.
    int bin = 0;
    if (f.ceil) {
      double direction, elevation;
      rect_ray_params(f.p, f.ph, f.c0 + (int)(p % (size_t)f.wl), (int)(p / (size_t)f.wl), direction, elevation);
      bin = ceiling_bin(f.ceil_layout, direction);
    }
    alive = march_steps<MODE, CALC, CUBIC, true, false>(f, e, c, r, n, i0, slice, sinks, counters, p, wl, bin) == MARCH_ON;
    if (alive) {
      slice_save<MODE>(st, p, r, i0 + slice);
    } else {
      st.step[p] = -1;
      march_finish<MODE>(out, sinks, counters, p, r);
    }
  }
  if (MODE == 3) { // the group's next wake distance, from a lane that is still marching (the value is the same in all of them)
    const unsigned long long still = __ballot(alive); // (a lane that ended inside the slice holds an older one)
    if (still && lane == __builtin_ctzll(still)) group_list(st.glist, item).n_and_wake[1] = wl.x_wake;
  }
  slice_requeue(st, item, alive);
#ifdef ATMRT_TIMELINE
  {
    const int i0max = timeline_wave_max(i0);
    const bool tl_again = __any(alive);
    if (lane == 0) {
      const unsigned long long k = atomicAdd(&g_slices[0], 1ull);
      if (k < 262144) {
        unsigned long long* r = g_slices + 8 + 4 * k;
        r[0] = item | ((unsigned long long)(unsigned)i0max << 32);
        r[1] = tl_slice_t0;
        r[2] = wall_clock64();
        r[3] = blockIdx.x | ((unsigned long long)(__builtin_amdgcn_s_getreg((15 << 11) | 4) & 0xffffu) << 32) |
               ((unsigned long long)(__builtin_amdgcn_s_getreg((3 << 11) | 20) & 0xfu) << 48);
      }
      if (item < 32768 && !tl_again) g_timeline[3 * item + 2] = wall_clock64(); // the group's last slice ended
    }
  }
#endif
  count_wave_steps<true>(counters, n.steps, n.lookups, n.esc_credit);
}

// every group must have finished: anything else is reported through CTR_SLICE_UNFINISHED and fails the frame (atmrt_api.hip)
static __global__ void k_slice_check(const unsigned long long* __restrict__ ctl, uint32_t n_groups, unsigned long long* __restrict__ counters) {
  counters[CTR_SLICE_UNFINISHED] = ctl[2] == n_groups ? 0ull : 1ull + (n_groups > ctl[2] ? n_groups - ctl[2] : ctl[2] - n_groups);
}

// TracePoint of a recorded crossing of pixel (x, y) at step s
template <int CALC>
static __device__ __forceinline__ TracePointDev rect_hit(const Frame& f, int x, int y, int s, double re0, double pl0,
                                                         double re1, double pl1) {
  const Earth e = earth_for<CALC>(f);
  double direction, elevation;
  rect_ray_params(f.p, f.ph, f.c0 + x, y, direction, elevation);
  DirCalc c;
  NormalTrig nt;
  if (normal_trig_of(f, e, nt)) { // the observer's three vectors are the frame's: only the ray's azimuth is the lane's
    double sindir, cosdir;
    dm_sincos(dm_to_radians(dm_to_degrees(direction)), &sindir, &cosdir);
    for (int i = 0; i < 10; i++) c.p[i] = 0.0;
    spherical_calc_from(nt.obs_n, nt.obs_e, nt.obs_up, sindir, cosdir, c);
  } else {
    dircalc_new(e, f.p.position.latitude, f.p.position.longitude, dm_to_degrees(direction), c);
  }
  double d0 = f.xs[s], d1 = f.xs[s + 1]; // the stepper's x: 0 + step + ... (same additions as xs)
  double lat0, lon0, lat1, lon1;
  coords_at_step(f, e, c, s, d0, lat0, lon0);
  coords_at_step(f, e, c, s + 1, d1, lat1, lon1);
  double te0 = terrain_elev_or_zero(f.tv, lat0, lon0);
  double te1 = terrain_elev_or_zero(f.tv, lat1, lon1);
  return terrain_trace_point(f, e, lat0, lon0, te0, re0, d0, pl0, lat1, lon1, te1, re1, d1, pl1);
}

template <int CALC>
__global__ __launch_bounds__(256) void k_rect_finalize(Frame f, const int32_t* __restrict__ hit_step, RectRec rec,
                                                       DensePlanes out) {
  stage_dm_tables();
  const size_t plane = (size_t)f.wl * f.h;
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= plane) return;
  int s = hit_step[p];
  if (s < 0) {
    store_dense_miss(out, p, plane);
    return;
  }
  const int y = (int)(p / (size_t)f.wl), x = (int)(p % (size_t)f.wl);
  store_dense(out, p, plane, rect_hit<CALC>(f, x, y, s, rec.re0[p], rec.pl0[p], rec.re1[p], rec.pl1[p]));
}

template <int CALC>
__global__ __launch_bounds__(256) void k_rect_finalize_list(Frame f, uint64_t n_hits,
                                                            const uint32_t* __restrict__ list_step,
                                                            const uint32_t* __restrict__ list_pixel, RectRec rec,
                                                            PackedHits packed) {
  stage_dm_tables();
  uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_hits) return;
  if (f.n_objects && packed.color_tag[k] != ATMRT_COLOR_TERRAIN) return; // object points are already complete
  uint32_t p = list_pixel[k];
  int x = (int)(p % (uint32_t)f.wl), y = (int)(p / (uint32_t)f.wl);
  store_packed(packed, k, rect_hit<CALC>(f, x, y, (int)list_step[k], rec.re0[k], rec.pl0[k], rec.re1[k], rec.pl1[k]),
               f.p.terrain_alpha);
}


// proximity filter of one sample (TerrainData::from_lat_lon, utils.rs:74-80) over the ray's candidates: bit q = cand[q] is close.
// Any number of close objects fits (the candidate list has at most CAND_CAP = 24 entries), and the union over the two samples
// of a step is an OR; set bits ascending = object indices ascending.
static __device__ ATMRT_OBJ_FN unsigned close_mask_impl(const ObjectDev* objects, Earth e, double lat, double lon, const int* cand, int ncand) {
  const LatLonTrig t = latlon_trig(e, lat, lon);
  unsigned m = 0;
  for (int q = 0; q < ncand; q++)
    if (object_is_close(e, objects[cand[q]], t)) m |= 1u << q;
  return m;
}
static __device__ __forceinline__ unsigned close_mask(const Frame& f, const Earth& e, double lat, double lon, const int* cand,
                                                      int ncand) {
  return close_mask_impl(f.objects, e, lat, lon, cand, ncand);
}

// Rectilinear, general.  Per sample: geodesic point, terrain gather, proximity filter (TerrainData::from_lat_lon,
// utils.rs:72-88), then the step logic above.
// 4 waves per SIMD (128 VGPRs) with the object code out of line (see ATMRT_OBJ_FN above) — built with the register allocator's region
// splitting off (csrc/Makefile TRACE_RA).  With the default allocator this kernel at 128 VGPRs is wrong in object scenes with
// interprocedural register allocation already OFF (azimuth 0 for the rays without candidate objects, garbage step counts: round 4,
// full-size config 5 through 8 tiles, seed 500011 of the sweep, tools/trace_waves_probe.py): the compiler stores `direction`, `p`
// and `ncand` to their spill slots at the head of the block that follows the x_wake loop over the ray's candidates below, AHEAD of the
// exec restore, i.e. only for the lanes that have candidates.  profiles/r04/ipra/README.md part 3; `make check-isa` finds such blocks in any build.
#ifndef ATMRT_TRACE_WAVES
#define ATMRT_TRACE_WAVES 4
#endif
template <bool FILL, int CALC, bool CUBIC>
__global__ __launch_bounds__(256, ATMRT_TRACE_WAVES) void k_rect_trace(Frame f, DensePlanes out, const uint64_t* __restrict__ hit_offset,
                                                    PackedHits packed, RectRec rec, uint32_t* __restrict__ list_step,
                                                    uint32_t* __restrict__ list_pixel,
                                                    unsigned long long* __restrict__ counters,
                                                    const uint32_t* __restrict__ pixel_list, uint32_t n_list,
                                                    double* __restrict__ step_prop, OverflowArena ovf, PackedHits ovf_packed) {
  // FILL = false: count the trace points of every pixel and keep those of pixels with <= RECT_SLOTS of them in the slot arena
  // (packed / rec / list_step then are that arena, pixel-major: slot_index).  FILL = true: write every point at its place in
  // the pixel-ordered list, for all pixels or for the listed ones (those that did not fit their slots).
  stage_dm_tables();
  const size_t plane = (size_t)f.wl * f.h;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = pixel_list ? tid < n_list : tid < plane;
  const size_t p = pixel_list ? (live ? pixel_list[tid] : 0) : tid;
  unsigned long long steps = 0;
  if (live) {
    const Earth e = earth_for<CALC>(f);
    const bool sph = e.spherical != 0;
    const double radius = e.shape_radius;
    const bool straight = f.p.straight_rays != 0;
    const double step = f.p.simulation_step, max_dist = f.p.frame.max_distance;
    const bool terrain_opaque = f.p.terrain_alpha == 1.0;
    const double skip_above = f.tv.skip_above;
    const double alt = *f.alt;
    double direction, elevation;
    DirCalc c;
    Stepper s;
    rect_ray_setup(f, e, p, alt, direction, elevation, c, s);
    unsigned count = 0;
    uint64_t k = FILL ? hit_offset[p] : 0;
    const StepSinks sinks{packed, rec, list_step, list_pixel, ovf, ovf_packed, counters};
    if (!(0.0 > max_dist || alt < -1000.0)) {
      double lat0, lon0;
      coords_at_step(f, e, c, 0, 0.0, lat0, lon0);
      double te0 = terrain_elev_or_zero(f.tv, lat0, lon0);
      int cand[CAND_CAP];
      double clo[CAND_CAP], chi[CAND_CAP];
      int ncand = 0;
      // rays with a candidate list keep the close objects of a sample as a bit mask over it; the others (more than CAND_CAP
      // candidates, or a DirectionalCalc without the pre-filter) test every object against both samples of a step.
      // x_wake: the first stepper distance at which any candidate can be close — before it the proximity filter is skipped.
      const bool use_cand = ray_candidates<CALC, CAND_CAP>(f, e, c, cand, ncand, clo, chi);
      if (!FILL && !use_cand && ncand == CAND_CAP) atomicAdd(&counters[CTR_UNLISTED_RAYS], 1ull); // statistics only (atmrt_last_stats)
      unsigned m0 = use_cand ? close_mask(f, e, lat0, lon0, cand, ncand) : 0u, m1 = 0u;
      double x_wake = dm_inf();
      for (int q = 0; q < ncand; q++)
        if (chi[q] >= 0.0) x_wake = clo[q] < x_wake ? clo[q] : x_wake;
      double re0 = alt, d0 = 0.0, pl0 = 0.0; // TracingState::new(.., first_path.elev, 0.0, 0.0), utils.rs:208
      double sx = 0.0, sh_ = alt, path_length = 0.0;
      bool have0 = true; // lat0 / lon0 / te0 hold the previous sample's geodesic point and terrain elevation
      for (int i = 1;; i++) {
        bool tame;
        RayState st = stepper_next<CUBIC>(s, *f.atm, sph, radius, straight, step, tame);
        if (straight) tame = __all(calc_dist_in_band(*f.atm, sh_) && calc_dist_in_band(*f.atm, st.h));
        path_length += calc_dist(sph, radius, sx, sh_, st.x, st.h, tame, f.inv_shape_radius);
        sx = st.x;
        sh_ = st.h;
        if (sx > max_dist || sh_ < -1000.0 || !(sx <= max_dist)) break; // rectilinear.rs:178 (+ NaN guard)
        // The geodesic point and the terrain lookup of a sample are skipped while nothing can need them: the ray is above every
        // post of the mosaic (ray - terrain is positive for certain, only its sign enters the crossing test) and no candidate
        // object's distance interval has been reached (no proximity test at this sample).  If the step turns out to produce
        // trace points after all, the skipped samples are evaluated then.  Rays without a candidate list test every object at
        // every sample and never skip.
        const bool awake = use_cand && sx >= x_wake; // inside (or past the start of) some candidate's interval
        bool have1 = !use_cand || awake || !(sh_ > skip_above);
        double lat1 = 0.0, lon1 = 0.0, te1 = 0.0;
        if (have1) {
          coords_at_step(f, e, c, i, sx, lat1, lon1); // sx = xs[i]: the stepper's x after i steps
          te1 = terrain_elev_or_zero(f.tv, lat1, lon1);
        }
        m1 = 0u;
        if (awake) {
          m1 = close_mask(f, e, lat1, lon1, cand, ncand);
          x_wake = dm_inf(); // next distance of interest: the earliest start among the intervals not yet left behind
          for (int q = 0; q < ncand; q++)
            if (chi[q] >= sx) x_wake = clo[q] < x_wake ? clo[q] : x_wake;
        }
        steps++;
        double diff1 = have0 ? re0 - te0 : 1.0, diff2 = have1 ? sh_ - te1 : 1.0;
        const bool crossing = diff1 * diff2 < 0.0;
        // the objects this step tests, ascending: union of the close lists of its two samples (utils.rs:241-250)
        unsigned m = 0u;
        bool any_object = false;
        if (use_cand) {
          m = m0 | m1;
          for (unsigned mm = m; mm; mm &= mm - 1) // drop the objects whose height band the segment does not enter
            if (object_out_of_band(f.objects[cand[__builtin_ctz(mm)]], re0, sh_)) m &= ~(mm & (0u - mm));
          any_object = m != 0u;
        } else {
          any_object = f.n_objects != 0;
        }
        if ((crossing || any_object) && !(have0 && have1)) { // the step produces trace points: its samples in full after all
#pragma unroll 1
          for (int q = 0; q < 2; q++) { // rolled: one more instance of the geodesic code, not two (rare path)
            if (q == 0 ? have0 : have1) continue;
            double la, lo;
            coords_at_step(f, e, c, q == 0 ? i - 1 : i, q == 0 ? d0 : sx, la, lo);
            const double te = terrain_elev_or_zero(f.tv, la, lo);
            if (q == 0) lat0 = la, lon0 = lo, te0 = te;
            else lat1 = la, lon1 = lo, te1 = te;
          }
          have0 = have1 = true;
          diff1 = re0 - te0;
          diff2 = sh_ - te1;
        }
        StepHits hits;
        step_begin(hits, crossing, diff1, diff2, terrain_opaque);
        Vec3 pos1 = v3(0.0, 0.0, 0.0), pos2 = pos1;
        LatLonTrig t0{}, t1{};
        if (any_object) {
          pos1 = as_cartesian(e, lat0, lon0, re0);
          pos2 = as_cartesian(e, lat1, lon1, sh_);
          if (!use_cand) {
            t0 = latlon_trig(e, lat0, lon0);
            t1 = latlon_trig(e, lat1, lon1);
          }
        }
        auto for_each_object = [&](auto&& visit) {
          if (use_cand) {
            for (unsigned mm = m; mm; mm &= mm - 1) visit(cand[__builtin_ctz(mm)]);
          } else {
            for (int j = 0; j < f.n_objects; j++)
              if (!object_out_of_band(f.objects[j], re0, sh_) && (object_is_close(e, f.objects[j], t0) || object_is_close(e, f.objects[j], t1)))
                visit(j);
          }
        };
        if (any_object) for_each_object([&](int j) { step_object(hits, f, j, pos1, pos2); });
        const StepGeom g{lat0, lon0, re0, d0, pl0, lat1, lon1, sh_, sx, path_length};
        if (FILL) step_commit_fill<true>(hits, sinks, step_prop, k, (uint32_t)p, i - 1, g, crossing, diff1, diff2, f, pos1, pos2, for_each_object);
        else step_commit_count<true>(hits, sinks, (uint32_t)p, count, i - 1, plane, g);
        count += (unsigned)hits.n;
        if (hits.finish) break;
        lat0 = lat1; lon0 = lon1; te0 = te1; re0 = sh_; d0 = sx; pl0 = path_length;
        have0 = have1;
        m0 = m1;
      }
    }
    if (!FILL) {
      store_ray_angles(out, p, direction, elevation);
      out.hit_count[p] = count;
      if (count > (unsigned)RECT_SLOTS) atomicAdd(&counters[CTR_OVERFLOW_PIXELS], 1ull);
    }
  }
  if (!FILL) count_wave_steps<false>(counters, steps, 0, -1);
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------

// k_rect_march<MODE, CALC, CUBIC, DRAIN> over n rays / list entries; returns the route that is
template <int MODE, bool CUBIC>
static MarchRoute launch_march_grid(bool drain, size_t n, const Frame& f, const DensePlanes& out, const MarchSinks& sinks, unsigned long long* counters,
                                    hipStream_t stream) {
  if (drain) {
    ATMRT_DISPATCH_CALC(f.earth.calc, hipLaunchKernelGGL((k_rect_march<MODE, CALC, CUBIC, true>), dim3(cdiv(n, ATMRT_MARCH_BLOCK_SMALL)),
                                                          dim3(ATMRT_MARCH_BLOCK_SMALL), 0, stream, f, out, sinks, counters));
  } else {
    ATMRT_DISPATCH_CALC(f.earth.calc, hipLaunchKernelGGL((k_rect_march<MODE, CALC, CUBIC, false>), dim3(cdiv(n, 256)), dim3(256), 0, stream, f, out,
                                                          sinks, counters));
  }
  return drain ? MarchRoute::GridDrain : MarchRoute::Grid;
}

// The sliced march (route Sliced; ws.march.slices, ws.slice_state): slice 0 as an ordinary grid, one host round trip for the number
// of groups still marching (it bounds the entries the later slices can write: the grid of the second kernel), then one wavefront
// per entry.
template <int MODE, bool CUBIC>
static void launch_rect_march_sliced(const Frame& f, Workspace& ws, const DensePlanes& out, const MarchSinks& sinks, hipStream_t stream) {
  const SliceLayout& L = ws.march.slices;
  const size_t n = (size_t)f.wl * f.h;
  const int slice = MARCH_SLICE_STEPS;
  SliceState st;
  slice_state_layout(ws.slice_state, L, f.n_objects != 0, st);
  (void)hipMemsetAsync(st.ctl, 0, 64, stream);
  ATMRT_DISPATCH_CALC(f.earth.calc, hipLaunchKernelGGL((k_rect_march_first<MODE, CALC, CUBIC>), dim3(cdiv(n, 256)), dim3(256), 0, stream, f,
                                                        out, sinks, (unsigned long long*)ws.counters, st, L.n_groups, slice));
  unsigned long long ctl_host[4] = {0, 0, 0, 0};
  if (hipMemcpyAsync(ctl_host, st.ctl, sizeof ctl_host, hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return; // the error is sticky: the caller's next HIP call reports it
  // a group writes at most one entry per slice it survives
  const size_t entries = std::min<size_t>(L.cap, (size_t)ctl_host[1] * L.slices_after);
  if (entries) {
    (void)hipMemsetAsync(st.queue + ctl_host[1], 0xff, (entries - (size_t)ctl_host[1]) * sizeof(uint32_t), stream);
    ATMRT_DISPATCH_CALC(f.earth.calc, hipLaunchKernelGGL((k_rect_march_cont<MODE, CALC, CUBIC>), dim3((unsigned)entries), dim3(64), 0, stream,
                                                          f, out, sinks, (unsigned long long*)ws.counters, st, L.n_groups, slice));
  }
  hipLaunchKernelGGL(k_slice_check, dim3(1), dim3(1), 0, stream, (const unsigned long long*)st.ctl, L.n_groups,
                     (unsigned long long*)ws.counters);
}

// The whole-frame work queue (route Queue; k_rect_march_queue over Frame::ceil_order): one workgroup per CU.  Without a claim word
// or the device's CU count it launches the grid instead, and says so.
template <bool CUBIC>
static MarchRoute launch_rect_march_queue(const Frame& f, Workspace& ws, const DensePlanes& out, const MarchSinks& sinks, hipStream_t stream) {
  const size_t n = (size_t)f.wl * f.h;
  int device = 0, cus = 0;
  if (!f.ceil_order || !f.ceil_order_steps || !ws.march_claim || hipGetDevice(&device) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1)
    return launch_march_grid<0, CUBIC>(march_grid_drain(0, n, ws.march.override), n, f, out, sinks, (unsigned long long*)ws.counters, stream);
  const uint32_t n_groups = (uint32_t)((n + 63) / 64);
  (void)hipMemsetAsync(ws.march_claim, 0, sizeof(unsigned long long), stream);
  ATMRT_DISPATCH_CALC(f.earth.calc, hipLaunchKernelGGL((k_rect_march_queue<CALC, CUBIC>), dim3((unsigned)cus), dim3(1024), 0, stream, f, out, sinks,
                                                        (unsigned long long*)ws.counters, f.ceil_order, f.ceil_order_steps, ws.march_claim, n_groups,
                                                        march_queue_long(), march_queue_item_prio(),
                                                        march_queue_guided() ? (uint32_t)cus * 16u : 0u)); // the launch's wavefronts
  return MarchRoute::Queue;
}

// The first-pass march of the frame by the route its workspace was planned with (Workspace::march): MODE 0 opaque terrain, 1
// translucent terrain, 3 scenes with objects.  Returns the route it launched.
template <int MODE, bool CUBIC>
static MarchRoute launch_march_planned(const Frame& f, Workspace& ws, const DensePlanes& out, const MarchSinks& sinks, hipStream_t stream) {
  const size_t n = (size_t)f.wl * f.h;
  switch (ws.march.route) {
    case MarchRoute::Sliced:
      launch_rect_march_sliced<MODE, CUBIC>(f, ws, out, sinks, stream);
      return MarchRoute::Sliced;
    case MarchRoute::Queue: // (planned for opaque terrain only: MarchShape::queue_ok)
      if constexpr (MODE == 0) return launch_rect_march_queue<CUBIC>(f, ws, out, sinks, stream);
      break;
    case MarchRoute::Grid:
    case MarchRoute::GridDrain:
      return launch_march_grid<MODE, CUBIC>(ws.march.route == MarchRoute::GridDrain, n, f, out, sinks, (unsigned long long*)ws.counters, stream);
    case MarchRoute::None:
      break;
  }
  return MarchRoute::None; // no plan, no launch
}

template <bool CUBIC>
MarchRoute launch_rect_march_t(const Frame& f, Workspace& ws, const DensePlanes& out, hipStream_t stream, hipEvent_t ev_marched) {
  size_t n = (size_t)f.wl * f.h;
  RectRec rec = carve_rec(ws.rect_rec, n);
  MarchSinks sinks{};
  MarchRoute route;
  if (f.opaque) {
    sinks.hit_step = ws.hit_step;
    sinks.rec = rec;
    route = launch_march_planned<0, CUBIC>(f, ws, out, sinks, stream);
    (void)hipEventRecord(ev_marched, stream);
    ATMRT_DISPATCH_CALC(f.earth.calc, hipLaunchKernelGGL((k_rect_finalize<CALC>), dim3(cdiv(n, 256)), dim3(256), 0, stream,
                                                          f, ws.hit_step, rec, out));
  } else {
    sinks.rec = carve_rec(ws.slot_rec, n * RECT_SLOTS);
    sinks.step = ws.slot_step;
    sinks.ovf = carve_overflow(ws.overflow_arena, ws.overflow_cap);
    route = launch_march_planned<1, CUBIC>(f, ws, out, sinks, stream);
    (void)hipEventRecord(ev_marched, stream);
  }
  return route;
}

// terrain_alpha < 1, no usable overflow arena (launch_list_fill): the pixels with more crossings than slots, listed in ws.overflow
// by the gather, marched again — every crossing to its place in the pixel-ordered list
template <bool CUBIC>
void launch_rect_second_march_t(const Frame& f, Workspace& ws, uint64_t n_hits, const DensePlanes& dense, hipStream_t stream) {
  MarchSinks sinks{};
  sinks.rec = carve_rec(ws.rect_rec, (size_t)n_hits);
  sinks.step = ws.list_step;
  sinks.list_pixel = ws.list_pixel;
  sinks.hit_offset = ws.hit_offset;
  sinks.pixel_list = ws.overflow;
  sinks.n_list = (uint32_t)ws.n_overflow;
  launch_march_grid<2, CUBIC>(march_grid_drain(2, (size_t)ws.n_overflow, ws.march.override), (size_t)ws.n_overflow, f, dense, sinks,
                              (unsigned long long*)ws.counters, stream);
}

// the rays k_rect_march<3> left to the tracer, collected into a list (order irrelevant: every ray is independent); CTR_OBJECT_RAYS counts them
static __global__ __launch_bounds__(256) void k_collect_object_rays(size_t n, const uint32_t* __restrict__ hit_count,
                                                                    uint32_t* __restrict__ list, unsigned long long* __restrict__ counters) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  wave_compact_append(p < n && hit_count[p] == OBJECT_RAY, (uint32_t)p, list, &counters[CTR_OBJECT_RAYS]); // the rays the general tracer visits
}

// the overflow arena of a scene with objects: records + complete points
static inline OverflowArena trace_overflow_arena(const Workspace& ws) {
  OverflowArena a = carve_overflow(ws.overflow_arena, ws.overflow_cap);
  if (a.cap) a.color_tag = ws.overflow_packed.color_tag;
  return a;
}
// Scenes with objects, counting pass, phase 1: the lean march over every pixel (terrain crossings into the tracer's slot arena,
// rays that can meet an object flagged and listed); phase 2 (launch_rect_trace_objects_t, after the host has read the list's
// length) traces the listed rays with the general tracer.
template <bool CUBIC>
MarchRoute launch_rect_trace_count_t(const Frame& f, Workspace& ws, const DensePlanes& out, hipStream_t stream) {
  size_t n = (size_t)f.wl * f.h;
  RectRec slots = carve_rec(ws.slot_rec, n * RECT_SLOTS);
  // the frame and the tracer's arenas where the out-of-line object step can address them (object_step_impl): copies in HBM
  StepSinks sinks{};
  sinks.packed = ws.slot_packed;
  sinks.rec = slots;
  sinks.step = ws.slot_step;
  sinks.pixel = ws.slot_pixel;
  sinks.ovf = trace_overflow_arena(ws);
  sinks.ovf_packed = ws.overflow_packed;
  sinks.counters = (unsigned long long*)ws.counters;
  Frame* frame_dev;
  StepSinks* sinks_dev;
  Carve ctx(ws.step_ctx); // the layout run_core reserves
  ctx(frame_dev, sizeof(Frame));
  ctx(sinks_dev, STEP_SINKS_MAX_BYTES);
  (void)hipMemcpyAsync(frame_dev, &f, sizeof f, hipMemcpyHostToDevice, stream);
  (void)hipMemcpyAsync(sinks_dev, &sinks, sizeof sinks, hipMemcpyHostToDevice, stream);
  (void)hipStreamSynchronize(stream); // both sources are on this stack frame
  // the planned route: a grid, or (forced) the time-sliced march, its groups carrying their candidate lists
  MarchSinks msinks{};
  msinks.hit_step = ws.hit_step;
  msinks.rec = slots;
  msinks.step = ws.slot_step;
  msinks.ovf = sinks.ovf;
  msinks.slot_tag = ws.slot_packed.color_tag;
  msinks.frame_dev = frame_dev;
  msinks.step_sinks_dev = sinks_dev;
  const MarchRoute route = launch_march_planned<3, CUBIC>(f, ws, out, msinks, stream);
  hipLaunchKernelGGL(k_collect_object_rays, dim3(cdiv(n, 256)), dim3(256), 0, stream, n, (const uint32_t*)out.hit_count, ws.object_rays,
                     (unsigned long long*)ws.counters);
  return route;
}
template <bool CUBIC>
void launch_rect_trace_objects_t(const Frame& f, Workspace& ws, const DensePlanes& out, uint64_t n_rays, hipStream_t stream) {
  if (!n_rays) return;
  size_t n = (size_t)f.wl * f.h;
  RectRec slots = carve_rec(ws.slot_rec, n * RECT_SLOTS);
  ATMRT_DISPATCH_CALC(f.earth.calc, hipLaunchKernelGGL((k_rect_trace<false, CALC, CUBIC>), dim3(cdiv((size_t)n_rays, 256)), dim3(256), 0, stream, f, out,
                                                        (const uint64_t*)nullptr, ws.slot_packed, slots, ws.slot_step,
                                                        ws.slot_pixel, (unsigned long long*)ws.counters,
                                                        (const uint32_t*)ws.object_rays, (uint32_t)n_rays, (double*)nullptr,
                                                        trace_overflow_arena(ws), ws.overflow_packed));
}

// the same in a scene with objects: the general tracer's fill pass over those pixels
template <bool CUBIC>
void launch_rect_second_trace_t(const Frame& f, Workspace& ws, uint64_t n_hits, const DensePlanes& dense, const PackedHits& packed,
                                hipStream_t stream) {
  ATMRT_DISPATCH_CALC(f.earth.calc, hipLaunchKernelGGL((k_rect_trace<true, CALC, CUBIC>), dim3(cdiv((size_t)ws.n_overflow, 256)), dim3(256), 0,
                                                        stream, f, dense, ws.hit_offset, packed, carve_rec(ws.rect_rec, (size_t)n_hits),
                                                        ws.list_step, ws.list_pixel, (unsigned long long*)ws.counters,
                                                        (const uint32_t*)ws.overflow, (uint32_t)ws.n_overflow, ws.step_prop,
                                                        OverflowArena{}, PackedHits{}));
}

// explicit instantiation of the launchers for one value of CUBIC, in two groups so that four translation units (march / trace x
// linear / spline atmospheres) compile in parallel: the lean march (k_rect_march, all modes) and the general tracer (k_rect_trace)
#define ATMRT_INSTANTIATE_MARCH(CUBIC)                                                                                        \
  template MarchRoute launch_rect_march_t<CUBIC>(const Frame&, Workspace&, const DensePlanes&, hipStream_t, hipEvent_t);      \
  template void launch_rect_second_march_t<CUBIC>(const Frame&, Workspace&, uint64_t, const DensePlanes&, hipStream_t);       \
  template MarchRoute launch_rect_trace_count_t<CUBIC>(const Frame&, Workspace&, const DensePlanes&, hipStream_t);
#define ATMRT_INSTANTIATE_TRACE(CUBIC)                                                                                        \
  template void launch_rect_trace_objects_t<CUBIC>(const Frame&, Workspace&, const DensePlanes&, uint64_t, hipStream_t);      \
  template void launch_rect_second_trace_t<CUBIC>(const Frame&, Workspace&, uint64_t, const DensePlanes&, const PackedHits&,  \
                                                  hipStream_t);

} // namespace atmrt
