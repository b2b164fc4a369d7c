// atmrt_kernels.hip — gfx950 (MI355X, CDNA4) kernels of the ray-marching path.
//
// Wavefront = 64 lanes everywhere.  All arithmetic is IEEE binary64 with contraction disabled, in
// the operation order of atmrt_core.h, so results are bit-identical to the CPU checker.
//
// Fast generator (fast.rs:22-98) as four kernels:
//   k_fast_columns    per-column DirectionalCalc                  (utils.rs:183-189)
//   k_terrain_profile phase A: terrain elevation per (sample, column)   (utils.rs:176-199, 84)
//   k_fast_paths      phase B: one RK4 ray per image row          (utils.rs:136-174)
//   k_fast_intersect  phase C: sign-change scan of get_single_pixel     (utils.rs:211-240)
//   k_fast_finalize   TracePoint at the bracketing samples only   (utils.rs:108-125, 15-40)
// Rectilinear generator (rectilinear.rs:102-186): k_rect_march, one ray per lane.
// The per-object collision code is called out of line in this translation unit as well (only k_fast_trace uses it): inlined it
// takes the Fast tracer to 256 VGPRs / 2 waves per SIMD; out of line at 3 waves config 5 runs 26.0 -> 23.4 ms (Fast) and
// 73.4 -> 67.7 ms (InterpolatingRectilinear); 4 waves 26.9 ms.
#define ATMRT_OBJ_FN __attribute__((noinline))
#include "atmrt_device.h"
#include "atmrt_overlay.h"
#include "atmrt_render.h"
#include "atmrt_vismap.h"
#include "atmrt_landmarks.h"

namespace atmrt {

// ---------------------------------------------------------------------------------------------
// set-up: Altitude::abs for the observer and every object (params.rs:23-30, object/mod.rs:166-175)
// ---------------------------------------------------------------------------------------------
__global__ void k_resolve(Frame f, double* alt, ObjectDev* objects) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *alt = observer_altitude(f);
  if (i < f.n_objects) { // the host stores the altitude kind in _pad and the configured altitude in elev
    ObjectDev o = objects[i];
    if (o._pad == ATMRT_ALT_RELATIVE) o.elev = terrain_elev_or_zero(f.tv, o.lat, o.lon) + o.elev;
    o._pad = ATMRT_ALT_ABSOLUTE;
    object_derive(f.earth, f.p.simulation_step, o);
    objects[i] = o;
  }
}

// ---------------------------------------------------------------------------------------------
// Fast generator
// ---------------------------------------------------------------------------------------------
__global__ void k_fast_columns(Frame f, DirCalc* colcalc) {
  int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= f.wl) return;
  double dir = frame_col_dir(f, x);
  DirCalc c;
  dircalc_new(f.earth, f.p.position.latitude, f.p.position.longitude, dir, c);
  colcalc[x] = c;
}

// Phase A.  A wavefront covers 64 adjacent columns at one sample index, so its profile store is one
// coalesced 512-byte row segment and its terrain gathers fall on neighbouring posts of the mosaic.
constexpr int PROFILE_SAMPLES_PER_BLOCK = 16;
template <int CALC, bool STORE_LL>
__global__ __launch_bounds__(256) void k_terrain_profile(Frame f, const DirCalc* __restrict__ colcalc,
                                                         double* __restrict__ prof, double* __restrict__ plat,
                                                         double* __restrict__ plon) {
  // sample blocks on grid.x (up to 4e6 / 16 of them), column tiles on grid.y (at most 1024): grid.y is limited to 65535
  int x = blockIdx.y * 64 + (threadIdx.x & 63);
  int sub = threadIdx.x >> 6;
  if (x >= f.wl) return;
  const Earth e = earth_for<CALC>(f);
  const DirCalc c = colcalc[x];
  int i0 = blockIdx.x * PROFILE_SAMPLES_PER_BLOCK;
  for (int k = sub; k < PROFILE_SAMPLES_PER_BLOCK; k += 4) {
    int i = i0 + k;
    if (i >= f.n_t) break;
    double lat, lon;
    coords_at_step(f, e, c, i, f.xs[i], lat, lon); // i < n_t <= march_steps + 1
    prof[(size_t)i * f.wl + x] = terrain_elev_or_zero(f.tv, lat, lon);
    if (STORE_LL) {
      plat[(size_t)i * f.wl + x] = lat;
      plon[(size_t)i * f.wl + x] = lon;
    }
  }
}

// Phase B (k_fast_paths, one RK4 ray per image row on an octet of lanes) lives in atmrt_paths.hip.

// Phase C.  Lanes = 64 adjacent columns, each wavefront owns RR adjacent rows.  The terrain value prof[i][x] is
// loaded once per lane (coalesced) and reused for RR rows; the ray elevations pelev[y][i..i+CH) are wave-uniform and
// arrive as wide scalar loads.  The body is branch-free (selects), samples are processed CH at a time and the
// all-lanes-finished test (MODE 0) runs once per chunk.  MODE 0: opaque terrain, first sign change only.
// MODE 1: count every sign change (terrain_alpha < 1).
template <int RR, int MODE>
__global__ __launch_bounds__(256) void k_fast_intersect(Frame f, const double* __restrict__ prof,
                                                        const double* __restrict__ pelev,
                                                        const int32_t* __restrict__ npath,
                                                        int32_t* __restrict__ hit_step,
                                                        uint32_t* __restrict__ hit_count,
                                                        uint32_t* __restrict__ px_steps,
                                                        unsigned long long* __restrict__ counters, double* __restrict__ dprev_state,
                                                        int i_begin, int i_end, int last_segment, uint32_t* __restrict__ slot_step,
                                                        uint32_t* __restrict__ slot_tag, const uint8_t* __restrict__ traced) {
  // slot_tag != nullptr (scenes with objects, one launch over all samples): the slots are the general tracer's arena — pixel-major (slot_index),
  // tag ATMRT_COLOR_TERRAIN — and the pixels marked in `traced` are k_fast_trace's: their ray-steps are not
  // counted here (whatever this scan stores for them is overwritten).
  // Samples i_begin .. i_end - 1 (the frame is scanned in the segments in which its ray paths are integrated, so that the scan
  // of one segment overlaps the integration of the next); between segments a pixel's state is the difference at its last
  // sample (dprev_state), its first hit (hit_step) and its count (hit_count).
  constexpr int CH = 4;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // Tile order: blockIdx.x = column tile, blockIdx.y = row group.  Consecutive workgroups share a row group (its ray
  // elevations stay in the scalar cache / L2) and sweep the column tiles of the terrain profile.  An explicitly XCD-aware
  // order (XCD r owns column tiles r, r+8, ... and walks all their row groups) was measured and rejected: FETCH_SIZE 0.50 GB
  // vs 0.44 GB per frame and 2.46 ms vs 2.21 ms — the whole working set (65 MB profile + 33 MB paths) sits in the 256 MB
  // Infinity Cache and the kernel is not bandwidth-limited.
  const int x = blockIdx.x * 64 + lane;
  const bool xok = x < f.wl;
  const int xc = xok ? x : f.wl - 1;
  const int y0 = (blockIdx.y * 4 + wave) * RR;
  const int cap = f.n_path_cap;
  const size_t wl = (size_t)f.wl;
  const size_t plane_px = wl * (size_t)f.h;
  if (y0 >= f.h) return;

  // rows past the image repeat the last row (identical work, never stored), so the fast loop stays uniform
  const double* prow[RR];
  int nrow[RR];
  double dprev[RR];
  int first[RR];
  unsigned cnt[RR];
  int nmin = 0x7fffffff, nmax = 0;
  const double t0 = prof[xc];
#pragma unroll
  for (int r = 0; r < RR; r++) {
    int y = y0 + r < f.h ? y0 + r : f.h - 1;
    int n = npath[y];
    n = n < f.n_t ? n : f.n_t; // Iterator::zip, fast.rs:59-62
    nrow[r] = n;
    nmin = n < nmin ? n : nmin;
    nmax = n > nmax ? n : nmax;
    prow[r] = pelev + (size_t)y * cap;
    first[r] = -1;
    cnt[r] = 0;
    dprev[r] = prow[r][0] - t0;
  }
  int nfound = 0; // rows of this lane that have their first hit (MODE 0)
  if (i_begin > 1) { // resume from the previous segment
#pragma unroll
    for (int r = 0; r < RR; r++) {
      const size_t p = (size_t)(y0 + r < f.h ? y0 + r : f.h - 1) * wl + xc;
      dprev[r] = dprev_state[p];
      first[r] = hit_step[p];
      if (MODE == 0) nfound += first[r] >= 0 ? 1 : 0;
      else cnt[r] = hit_count[p];
    }
  }
  nmin = nmin < i_end ? nmin : i_end;
  nmax = nmax < i_end ? nmax : i_end;
  bool alldone = MODE == 0 && __all(nfound == RR);
  int i = i_begin;
  for (; !alldone && i + CH <= nmin; i += CH) {
    double t[CH];
#pragma unroll
    for (int k = 0; k < CH; k++) t[k] = prof[(size_t)(i + k) * wl + xc];
#pragma unroll
    for (int r = 0; r < RR; r++) {
      const double* pr = prow[r] + i;
      double p[CH];
#pragma unroll
      for (int k = 0; k < CH; k++) p[k] = pr[k];
      unsigned hitbits = 0;
      const unsigned cnt0 = cnt[r];
#pragma unroll
      for (int k = 0; k < CH; k++) {
        const double d = p[k] - t[k];
        const bool hit = dprev[r] * d < 0.0; // utils.rs:222
        const bool nh = hit && first[r] < 0;
        first[r] = nh ? i + k - 1 : first[r];
        if (MODE == 0) nfound += nh ? 1 : 0;
        else {
          cnt[r] += hit ? 1u : 0u;
          hitbits |= hit ? 1u << k : 0u;
        }
        dprev[r] = d;
      }
      if (MODE != 0 && hitbits && xok && y0 + r < f.h) { // rare: keep the first RECT_SLOTS crossings of the pixel for the list
        unsigned c = cnt0;
        const size_t pp = (size_t)(y0 + r) * wl + x;
        for (unsigned hb = hitbits; hb && c < (unsigned)RECT_SLOTS; hb &= hb - 1, c++) {
          const size_t q = slot_tag ? slot_index<SlotLayout::PixelMajor>(pp, c, plane_px) : slot_index<SlotLayout::SlotMajor>(pp, c, plane_px);
          slot_step[q] = (uint32_t)(i + __builtin_ctz(hb) - 1);
          if (slot_tag) slot_tag[q] = ATMRT_COLOR_TERRAIN;
        }
      }
    }
    if (MODE == 0 && __all(nfound == RR)) {
      alldone = true;
      break;
    }
  }
  if (!alldone) { // remainder of the chunking and rows whose path ended early (ray below -1000 m, utils.rs:167)
    for (; i < nmax; i++) {
      const double t = prof[(size_t)i * wl + xc];
#pragma unroll
      for (int r = 0; r < RR; r++) {
        if (i < nrow[r]) {
          const double d = prow[r][i] - t;
          const bool hit = dprev[r] * d < 0.0;
          const bool nh = hit && first[r] < 0;
          first[r] = nh ? i - 1 : first[r];
          if (MODE != 0 && hit) {
            if (cnt[r] < (unsigned)RECT_SLOTS && xok && y0 + r < f.h) {
              const size_t pp = (size_t)(y0 + r) * wl + x;
              const size_t q = slot_tag ? slot_index<SlotLayout::PixelMajor>(pp, cnt[r], plane_px) : slot_index<SlotLayout::SlotMajor>(pp, cnt[r], plane_px);
              slot_step[q] = (uint32_t)(i - 1);
              if (slot_tag) slot_tag[q] = ATMRT_COLOR_TERRAIN;
            }
            cnt[r]++;
          }
          dprev[r] = d;
        }
      }
    }
  }

  if (!last_segment) {
#pragma unroll
    for (int r = 0; r < RR; r++) {
      int y = y0 + r;
      if (y < f.h && xok) {
        size_t p = (size_t)y * f.wl + x;
        dprev_state[p] = dprev[r];
        hit_step[p] = first[r];
        if (MODE != 0) hit_count[p] = cnt[r];
      }
    }
    return;
  }
  unsigned long long steps = 0;
#pragma unroll
  for (int r = 0; r < RR; r++) {
    int y = y0 + r;
    if (y < f.h && xok) {
      size_t p = (size_t)y * f.wl + x;
      hit_step[p] = first[r];
      unsigned st;
      if (MODE == 0) {
        hit_count[p] = first[r] >= 0 ? 1u : 0u;
        st = first[r] >= 0 ? (unsigned)(first[r] + 1) : (unsigned)(nrow[r] > 0 ? nrow[r] - 1 : 0);
        if (slot_tag && first[r] >= 0) { // opaque terrain in a scene with objects: the first crossing is the pixel's only slot
          const size_t q = slot_index<SlotLayout::PixelMajor>(p, 0, plane_px);
          slot_step[q] = (uint32_t)first[r];
          slot_tag[q] = ATMRT_COLOR_TERRAIN;
        }
      } else {
        hit_count[p] = cnt[r];
        st = (unsigned)(nrow[r] > 0 ? nrow[r] - 1 : 0);
      }
      if (traced && traced[p]) st = 0;
      steps += st;
      if (px_steps) px_steps[p] = st;
    }
  }
  steps = wave_sum(steps); // one atomic per wavefront: 16 K of them at the headline size, spread over the kernel's 2 ms
  if (lane == 0 && steps) atomicAdd(&counters[CTR_RAY_STEPS], steps);
}

// The two samples that bracket step s of pixel (x, y), from the caches
static __device__ __forceinline__ TracePointDev fast_hit(const Frame& f, const Earth& e, const DirCalc& c, const double* prof, const double* pelev,
                                         const double* plen, int x, int y, int s) {
  double lat0, lon0, lat1, lon1;
  double d0 = f.xs[s], d1 = f.xs[s + 1];
  coords_at_step(f, e, c, s, d0, lat0, lon0); // the stepper's distances: s + 1 < n_t <= march_steps + 1
  coords_at_step(f, e, c, s + 1, d1, lat1, lon1);
  double te0 = prof[(size_t)s * f.wl + x], te1 = prof[(size_t)(s + 1) * f.wl + x];
  size_t base = (size_t)y * f.n_path_cap;
  double re0 = pelev[base + s], re1 = pelev[base + s + 1];
  // TracingState::new(&first_terrain, first_path.elev, 0.0, 0.0) (utils.rs:208): path[0] is (0, alt, 0) anyway
  double pl0 = plen[base + s], pl1 = plen[base + s + 1];
  return terrain_trace_point(f, e, lat0, lon0, te0, re0, d0, pl0, lat1, lon1, te1, re1, d1, pl1);
}

template <int CALC>
__global__ __launch_bounds__(256) void k_fast_finalize(Frame f, const DirCalc* __restrict__ colcalc,
                                                       const double* __restrict__ prof,
                                                       const double* __restrict__ pelev,
                                                       const double* __restrict__ plen,
                                                       const int32_t* __restrict__ hit_step, DensePlanes out) {
  int x = blockIdx.x * blockDim.x + threadIdx.x;
  int y = blockIdx.y;
  if (x >= f.wl) return;
  size_t plane = (size_t)f.wl * f.h;
  size_t p = (size_t)y * f.wl + x;
  out.azimuth[p] = frame_azimuth(f, x);
  out.elevation_angle[p] = frame_row_elev(f, y);
  int s = hit_step[p];
  if (s < 0) {
    store_dense_miss(out, p, plane);
    return;
  }
  const DirCalc c = colcalc[x];
  store_dense(out, p, plane, fast_hit(f, earth_for<CALC>(f), c, prof, pelev, plen, x, y, s));
}

// terrain_alpha < 1: the list of every sign change of every pixel (step index + pixel).  The counting scan kept the first
// RECT_SLOTS crossings of each pixel; k_gather_slots moves those, and only pixels with more are scanned a second time.
__global__ __launch_bounds__(256) void k_fast_list(Frame f, const double* __restrict__ prof,
                                                   const double* __restrict__ pelev,
                                                   const int32_t* __restrict__ npath,
                                                   const uint64_t* __restrict__ hit_offset,
                                                   const uint32_t* __restrict__ hit_count,
                                                   uint32_t* __restrict__ list_step,
                                                   uint32_t* __restrict__ list_pixel) {
  int x = blockIdx.x * blockDim.x + threadIdx.x;
  int y = blockIdx.y;
  if (x >= f.wl) return;
  int n = npath[y];
  n = n < f.n_t ? n : f.n_t;
  size_t p = (size_t)y * f.wl + x;
  if (hit_count[p] <= (uint32_t)RECT_SLOTS) return; // listed from the slots of the counting scan (k_gather_slots)
  uint64_t k = hit_offset[p];
  const double* row = pelev + (size_t)y * f.n_path_cap;
  double dprev = row[0] - prof[x];
  for (int i = 1; i < n; i++) {
    double d = row[i] - prof[(size_t)i * f.wl + x];
    if (dprev * d < 0.0) {
      list_step[k] = (uint32_t)(i - 1);
      list_pixel[k] = (uint32_t)p;
      k++;
    }
    dprev = d;
  }
}

template <int CALC>
__global__ __launch_bounds__(256) void k_fast_finalize_list(Frame f, uint64_t n_hits,
                                                            const DirCalc* __restrict__ colcalc,
                                                            const double* __restrict__ prof,
                                                            const double* __restrict__ pelev,
                                                            const double* __restrict__ plen,
                                                            const uint32_t* __restrict__ list_step,
                                                            const uint32_t* __restrict__ list_pixel, PackedHits packed) {
  uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_hits) return;
  if (f.n_objects && packed.color_tag[k] != ATMRT_COLOR_TERRAIN) return; // object points are already complete
  uint32_t p = list_pixel[k];
  int x = (int)(p % (uint32_t)f.wl), y = (int)(p / (uint32_t)f.wl);
  const DirCalc c = colcalc[x];
  store_packed(packed, k, fast_hit(f, earth_for<CALC>(f), c, prof, pelev, plen, x, y, (int)list_step[k]),
               f.p.terrain_alpha);
}

// azimuth / elevation planes and the dense first-hit view of a packed multi-hit result
__global__ __launch_bounds__(256) void k_dense_from_packed(Frame f, const uint64_t* __restrict__ hit_offset,
                                                           PackedHits packed, DensePlanes out, int fast_angles) {
  int x = blockIdx.x * blockDim.x + threadIdx.x;
  int y = blockIdx.y;
  if (x >= f.wl) return;
  size_t plane = (size_t)f.wl * f.h;
  size_t p = (size_t)y * f.wl + x;
  if (fast_angles) {
    out.azimuth[p] = frame_azimuth(f, x);
    out.elevation_angle[p] = frame_row_elev(f, y);
  }
  if (out.hit_count[p] == 0) {
    store_dense_miss(out, p, plane);
    return;
  }
  uint64_t k = hit_offset[p];
  TracePointDev tp;
  tp.lat = packed.lat[k];
  tp.lon = packed.lon[k];
  tp.distance = packed.distance[k];
  tp.elevation = packed.elevation[k];
  tp.path_length = packed.path_length[k];
  tp.normal = v3(packed.normal[3 * k], packed.normal[3 * k + 1], packed.normal[3 * k + 2]);
  store_dense(out, p, plane, tp);
}

// Fast, phase A extras: which objects are close to each terrain sample (TerrainData::from_lat_lon, utils.rs:74-80)
// Objects that can be close to ANY sample of a column (ray_candidates: exact superset, from the column's ground track), so that
// the per-sample proximity filter below tests a handful of objects instead of all of them.  ncand[x] < 0: no list for the
// column (more than COL_CAND candidates, or a DirectionalCalc without the pre-filter) — every object is tested.
constexpr int COL_CAND = 64;
template <int CALC>
__global__ __launch_bounds__(64) void k_column_candidates(Frame f, const DirCalc* __restrict__ colcalc, int32_t* __restrict__ ccand,
                                                          int32_t* __restrict__ ncand, double* __restrict__ cand_lo,
                                                          double* __restrict__ cand_hi, unsigned long long* __restrict__ counters) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= f.wl) return;
  int cand[COL_CAND];
  double lo[COL_CAND], hi[COL_CAND]; // distances at which a sample of the column can be close to the candidate (k_fast_flag_rows)
  int n = 0;
  const bool ok = ray_candidates<CALC, COL_CAND>(f, f.earth, colcalc[x], cand, n, lo, hi);
  ncand[x] = ok ? n : -1;
  if (!ok && n == COL_CAND) atomicAdd(&counters[CTR_UNLISTED_COLUMNS], 1ull); // statistics only (atmrt_last_stats)
  if (ok)
    for (int q = 0; q < n; q++) {
      ccand[(size_t)x * COL_CAND + q] = cand[q];
      cand_lo[(size_t)x * COL_CAND + q] = lo[q];
      cand_hi[(size_t)x * COL_CAND + q] = hi[q];
    }
}

// Fast generator with scene objects: which pixels can have a step that involves an object?  An object is tested at the sample pair
// (i - 1, i) of column x only if it is close to one of the two samples — possible only while the sample's distance lies in the
// candidate's interval [lo, hi] (candidate_interval: an exact superset) — and only by rows whose ray segment enters the object's height
// band (object_out_of_band, the tracer's own test).  Every other pixel's result is its terrain crossings alone: the plain intersect
// scan's.  One block per column and 256 rows: the column's candidates are wave-uniform, the ray elevations are read sample-major
// (coalesced over rows).  A column without a candidate list (more than COL_CAND candidates, or an earth model without the
// pre-filter) flags all its rows.
__global__ __launch_bounds__(256) void k_fast_flag_rows(Frame f, const int32_t* __restrict__ ccand, const int32_t* __restrict__ ncand,
                                                        const double* __restrict__ cand_lo, const double* __restrict__ cand_hi,
                                                        const double* __restrict__ pelev_t, const int32_t* __restrict__ npath,
                                                        uint8_t* __restrict__ flags) {
  const int x = blockIdx.x;
  const int y = blockIdx.y * blockDim.x + threadIdx.x;
  if (y >= f.h) return;
  const size_t p = (size_t)y * f.wl + x;
  const int nc = ncand[x];
  if (nc < 0) {
    flags[p] = 1;
    return;
  }
  int n = npath[y];
  n = n < f.n_t ? n : f.n_t; // Iterator::zip, fast.rs:59-62
  const size_t hh = (size_t)f.h;
  const double step = f.p.simulation_step;
  bool flag = false;
  for (int q = 0; q < nc && !flag; q++) {
    const ObjectDev& o = f.objects[ccand[(size_t)x * COL_CAND + q]];
    const double lo = cand_lo[(size_t)x * COL_CAND + q], hi = cand_hi[(size_t)x * COL_CAND + q];
    // samples whose distance xs[i] (= i * step up to rounding) can lie in [lo, hi], one more on either side; the pairs (i - 1, i)
    // that contain one of them
    double a = dm_floor(lo / step) - 1.0, b = dm_floor(hi / step) + 2.0;
    if (!(a >= 1.0)) a = 1.0;           // also NaN / -inf
    if (!(b <= (double)(n - 1))) b = (double)(n - 1);
    const int i0 = (int)a, i1 = (int)b + 1 < n ? (int)b + 1 : n - 1;
    for (int i = i0; i <= i1; i++) {
      const double re0 = pelev_t[(size_t)(i - 1) * hh + y], re1 = pelev_t[(size_t)i * hh + y];
      if (!((re0 < o.vlo && re1 < o.vlo) || (re0 > o.vhi && re1 > o.vhi))) {
        flag = true;
        break;
      }
    }
  }
  flags[p] = flag ? 1 : 0;
}

// TerrainData::from_lat_lon's proximity filter (utils.rs:74-80) for every (sample, column): count, then fill ascending lists
template <bool FILL>
__global__ __launch_bounds__(256) void k_close_objects(Frame f, const double* __restrict__ plat,
                                                       const double* __restrict__ plon, const int32_t* __restrict__ ccand,
                                                       const int32_t* __restrict__ ncand, uint32_t* __restrict__ ccount,
                                                       const uint64_t* __restrict__ coffset, uint32_t* __restrict__ clist) {
  size_t n = (size_t)f.n_t * f.wl;
  size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const int x = (int)(s % (size_t)f.wl);
  const int nc = ncand[x];
  const int32_t* cand = ccand + (size_t)x * COL_CAND;
  if (nc == 0) { // nothing can be close to this column
    if (!FILL) ccount[s] = 0;
    return;
  }
  const LatLonTrig t = latlon_trig(f.earth, plat[s], plon[s]);
  uint32_t c = 0;
  uint64_t k = FILL ? coffset[s] : 0;
  const int total = nc < 0 ? f.n_objects : nc;
  for (int q = 0; q < total; q++) {
    const int j = nc < 0 ? q : cand[q];
    if (object_is_close(f.earth, f.objects[j], t)) {
      if (FILL) clist[k + c] = (uint32_t)j;
      c++;
    }
  }
  if (!FILL) ccount[s] = c;
}

// Fast, phase C, general (scene objects: the full get_single_pixel, utils.rs:201-289).
// One image COLUMN per wavefront, lanes = 64 adjacent rows.  Everything that depends on the column only — the terrain
// profile value of a sample, its close-object list — is wave-uniform: scalar loads, and the "does this sample pair have close
// objects" test is a scalar branch, so the object logic runs for whole wavefronts at the 2 % of cells that need it and the
// other steps are a handful of vector instructions per row (one coalesced load of the ray elevations, which k_paths_transpose
// lays out sample-major for this kernel).  Inside an object cell a lane joins the geometry only if its segment enters the
// height band of an object (object_out_of_band).
#ifndef ATMRT_FAST_TRACE_WAVES
#define ATMRT_FAST_TRACE_WAVES 3
#endif
template <bool FILL>
__global__ __launch_bounds__(256, ATMRT_FAST_TRACE_WAVES) void k_fast_trace(Frame f, const double* __restrict__ prof,
                                                    const double* __restrict__ plat, const double* __restrict__ plon,
                                                    const uint32_t* __restrict__ ccount,
                                                    const uint64_t* __restrict__ coffset,
                                                    const uint32_t* __restrict__ clist, const double* __restrict__ pelev_t,
                                                    const double* __restrict__ plen_t, const int32_t* __restrict__ npath,
                                                    uint32_t* __restrict__ hit_count,
                                                    const uint64_t* __restrict__ hit_offset, PackedHits packed,
                                                    uint32_t* __restrict__ list_step, uint32_t* __restrict__ list_pixel,
                                                    uint32_t* __restrict__ px_steps,
                                                    unsigned long long* __restrict__ counters, double* __restrict__ step_prop,
                                                    const uint8_t* __restrict__ traced) {
  // traced (counting pass): only the rows marked by k_fast_flag_rows are traced here — the others cannot meet an object and keep
  // what the plain intersect scan found; a wavefront without a marked row leaves at once.
  // FILL = false: count the trace points of every pixel and keep those of pixels with <= RECT_SLOTS of them in the slot arena
  // (packed / list_step / list_pixel then are that arena, pixel-major: slot_index).  FILL = true: write every point at its
  // place in the pixel-ordered list — for the pixels that did not fit their slots (hit_count > RECT_SLOTS); the others were
  // moved by k_gather_slots and their lanes are idle here (most wavefronts leave at once).
  // caches written by earlier kernels, read-only here: through the constant address space a wave-uniform index is a scalar load
  typedef const __attribute__((address_space(4))) double* ConstF64;
  typedef const __attribute__((address_space(4))) uint32_t* ConstU32;
  typedef const __attribute__((address_space(4))) uint64_t* ConstU64;
  typedef const __attribute__((address_space(4))) ObjectDev* ConstObj;
  const ConstF64 kprof = (ConstF64)(uintptr_t)prof, kplat = (ConstF64)(uintptr_t)plat, kplon = (ConstF64)(uintptr_t)plon;
  const ConstU32 kccount = (ConstU32)(uintptr_t)ccount, kclist = (ConstU32)(uintptr_t)clist;
  const ConstU64 kcoffset = (ConstU64)(uintptr_t)coffset;
  const ConstObj kobjects = (ConstObj)(uintptr_t)f.objects;
  const int lane = threadIdx.x & 63;
  const int x = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); // wave-uniform column
  const int y = blockIdx.y * 64 + lane;
  if (x >= f.wl) return; // whole wavefront
  const bool row_ok = y < f.h;
  const size_t hh = (size_t)f.h;
  const bool terrain_opaque = f.p.terrain_alpha == 1.0;
  int n = 0;
  if (row_ok) {
    n = npath[y];
    n = n < f.n_t ? n : f.n_t; // Iterator::zip, fast.rs:59-62
  }
  int nmax = n;
  for (int o = 32; o; o >>= 1) {
    const int v = __shfl_xor(nmax, o, 64);
    nmax = v > nmax ? v : nmax;
  }
  const size_t p = (size_t)(row_ok ? y : 0) * f.wl + x;
  uint64_t k = (FILL && row_ok) ? hit_offset[p] : 0;
  unsigned count = 0, stp = 0;
  const bool mine = FILL || !traced || (row_ok && traced[p] != 0);
  bool active = n > 1 && mine && (!FILL || hit_count[p] > (uint32_t)RECT_SLOTS);
  if (!__any(mine)) return;
  double te0 = kprof[x], re0 = n > 0 ? pelev_t[y] : 0.0;
  uint32_t c0 = kccount[x];
  const StepSinks sinks{packed, RectRec{}, list_step, list_pixel, OverflowArena{}, PackedHits{}, counters}; // Fast: no record, no arena
  // a step without close objects whose samples the terrain separates: the crossing, its tag only (utils.rs:222-240)
  auto terrain_hit = [&](int step_index) {
    if (FILL || count < (unsigned)RECT_SLOTS) {
      const uint64_t kw = FILL ? k : slot_index<SlotLayout::PixelMajor>(p, count, (size_t)f.wl * hh);
      list_step[kw] = (uint32_t)step_index;
      list_pixel[kw] = (uint32_t)p;
      packed.color_tag[kw] = ATMRT_COLOR_TERRAIN;
      k++;
    }
    count++;
    if (terrain_opaque) active = false;
  };
  constexpr int TCH = 8; // samples fetched ahead: every step's scalar loads would otherwise be a dependent round trip
  int i = 1;
  while (i < nmax) {
    if (!__any(active)) break;
    if (c0 == 0 && i + TCH <= nmax) {
      double te[TCH], re[TCH];
      uint32_t cc = 0;
#pragma unroll
      for (int q = 0; q < TCH; q++) {
        te[q] = kprof[(size_t)(i + q) * f.wl + x];
        cc |= kccount[(size_t)(i + q) * f.wl + x];
        re[q] = i + q < n ? pelev_t[(size_t)(i + q) * hh + y] : 0.0;
      }
      if (cc == 0) { // no close objects anywhere in the chunk: terrain only, utils.rs:222-240
#pragma unroll
        for (int q = 0; q < TCH; q++) {
          active = active && i + q < n;
          stp += active ? 1u : 0u;
          const double diff1 = re0 - te0, diff2 = re[q] - te[q];
          if (active && diff1 * diff2 < 0.0) terrain_hit(i + q - 1);
          te0 = te[q];
          re0 = re[q];
        }
        i += TCH;
        continue;
      }
    }
    { // one sample pair, with or without close objects
    const size_t s1 = (size_t)i * f.wl + x, s0 = s1 - f.wl;
    const double te1 = kprof[s1];
    const uint32_t c1 = kccount[s1];
    const bool in_path = i < n;
    const double re1 = in_path ? pelev_t[(size_t)i * hh + y] : 0.0;
    active = active && in_path;
    stp += active ? 1u : 0u;
    const double diff1 = re0 - te0, diff2 = re1 - te1;
    const bool hit = active && diff1 * diff2 < 0.0; // utils.rs:222
    if ((c0 | c1) == 0) { // wave-uniform: no close objects at either sample — terrain only (utils.rs:222-240)
      if (hit) terrain_hit(i - 1);
    } else { // the same for every lane: the union of the two ascending close lists (utils.rs:241-280)
      const ConstU32 la = kclist + kcoffset[s0];
      const ConstU32 lb = kclist + kcoffset[s1];
      if (active) {
        StepHits sh;
        step_begin(sh, hit, diff1, diff2, terrain_opaque);
        const double lat0 = kplat[s0], lon0 = kplon[s0], lat1 = kplat[s1], lon1 = kplon[s1];
        bool have_pos = false;
        Vec3 pos1 = v3(0.0, 0.0, 0.0), pos2 = pos1;
        // the union of the two ascending close lists, for the lanes whose segment enters the object's height band
        auto for_each_object = [&](auto&& visit) {
          uint32_t ia = 0, ib = 0;
          while (ia < c0 || ib < c1) {
            uint32_t idx;
            if (ib >= c1 || (ia < c0 && la[ia] <= lb[ib])) {
              idx = la[ia];
              if (ib < c1 && lb[ib] == idx) ib++;
              ia++;
            } else {
              idx = lb[ib++];
            }
            const double vlo = kobjects[idx].vlo, vhi = kobjects[idx].vhi;
            if ((re0 < vlo && re1 < vlo) || (re0 > vhi && re1 > vhi)) continue; // most rows pass above or below the object
            if (!have_pos) {
              pos1 = as_cartesian(f.earth, lat0, lon0, re0);
              pos2 = as_cartesian(f.earth, lat1, lon1, re1);
              have_pos = true;
            }
            visit((int)idx);
          }
        };
        for_each_object([&](int idx) { step_object(sh, f, idx, pos1, pos2); });
        const double d0 = i == 1 ? 0.0 : f.xs[i - 1], pl0 = i == 1 ? 0.0 : plen_t[(size_t)(i - 1) * hh + y];
        if (sh.n) {
          const StepGeom g{lat0, lon0, re0, d0, pl0, lat1, lon1, re1, f.xs[i], plen_t[(size_t)i * hh + y]};
          if (FILL) step_commit_fill<false>(sh, sinks, step_prop, k, (uint32_t)p, i - 1, g, hit, diff1, diff2, f, pos1, pos2, for_each_object);
          else step_commit_count<false>(sh, sinks, (uint32_t)p, count, i - 1, (size_t)f.wl * hh, g);
        }
        count += (unsigned)sh.n;
        if (sh.finish) active = false;
      }
    }
    te0 = te1;
    re0 = re1;
    c0 = c1;

    }
    i++;
  }
  if (!FILL && row_ok && mine) {
    hit_count[p] = count;
    if (px_steps) px_steps[p] = stp;
  }
  if (!FILL) {
    unsigned long long steps = wave_sum((unsigned long long)(row_ok && mine ? stp : 0u));
    if (lane == 0 && steps) atomicAdd(&counters[CTR_RAY_STEPS], steps);
  }
}

// ---------------------------------------------------------------------------------------------
// From the counting pass to the pixel-ordered list (frames that can have several trace points per pixel; launch_list_fill).
// The counting pass of every route kept the first RECT_SLOTS trace points of each pixel in the slot arena (slot_index), and a
// Rectilinear one appended the points beyond them to the overflow arena (OverflowArena); the scan of hit_count then gave every
// pixel its place in the list, hit_offset[p].  k_gather_slots moves the slots there, k_scatter_overflow the arena's records.  What
// travels is fixed at compile time: the step and the pixel always; REC: the Rectilinear record (RectRec) k_rect_finalize_list
// needs; POINTS (scenes with objects): the tag, and for object points the complete trace point — terrain points get only their tag
// here, the *_finalize_list kernels complete them.
// ---------------------------------------------------------------------------------------------
// what the gather does with a pixel that has more trace points than slots
enum class Beyond {
  Skip,  // Fast: the second pass (k_fast_list, k_fast_trace<true>) finds such pixels by hit_count itself and lists all their points
  List,  // Rectilinear without a usable arena: the same, but the second pass visits a list of them — appended here, in any order
         // (CTR_OVERFLOW_CURSOR was reset by the host and hands out the positions)
  Clamp, // Rectilinear with the arena: the points beyond the slots come out of it, so the slots of every pixel count.  In a scene
         // with objects a pixel's last slots may be stale (a step whose points did not all fit went to the arena whole):
         // k_scatter_overflow overwrites them, so it runs after this kernel on the same stream.
};
// one thread per pixel
template <SlotLayout LAYOUT, bool REC, bool POINTS, Beyond BEYOND>
__global__ __launch_bounds__(256) void k_gather_slots(size_t plane, const uint32_t* __restrict__ hit_count,
                                                      const uint64_t* __restrict__ hit_offset,
                                                      const uint32_t* __restrict__ slot_step, RectRec slot_rec, PackedHits slot_packed,
                                                      uint32_t* __restrict__ list_step, uint32_t* __restrict__ list_pixel, RectRec rec,
                                                      PackedHits packed, uint32_t* __restrict__ overflow,
                                                      unsigned long long* __restrict__ counters) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t n = p < plane ? hit_count[p] : 0u;
  if (BEYOND == Beyond::Clamp) n = n < (uint32_t)RECT_SLOTS ? n : (uint32_t)RECT_SLOTS;
  // every lane of the wavefront takes part, those past the plane included
  if (BEYOND == Beyond::List) wave_compact_append(n > (uint32_t)RECT_SLOTS, (uint32_t)p, overflow, &counters[CTR_OVERFLOW_CURSOR]);
  if (p >= plane || n > (uint32_t)RECT_SLOTS) return;
  const uint64_t k0 = hit_offset[p];
  for (uint32_t j = 0; j < n; j++) {
    const size_t q = slot_index<LAYOUT>(p, j, plane);
    const uint64_t k = k0 + j;
    list_step[k] = slot_step[q];
    list_pixel[k] = (uint32_t)p;
    if (REC) rec_copy(rec, k, slot_rec, q);
    if (POINTS) {
      const uint32_t tag = slot_packed.color_tag[q];
      packed.color_tag[k] = tag;
      if (tag != ATMRT_COLOR_TERRAIN) packed_copy(packed, k, slot_packed, q);
    }
  }
}

// one thread per record of the overflow arena: trace point number `ordinal` of pixel p is entry hit_offset[p] + ordinal of the list.
// POINTS: a record of the lean march (OVERFLOW_LEAN) is void if the march handed the ray to the general tracer afterwards
// (handed_over = MarchSinks::hit_step) — the tracer appended that ray's points itself.
template <bool POINTS>
__global__ __launch_bounds__(256) void k_scatter_overflow(uint32_t n_records, OverflowArena ovf, PackedHits ovf_packed,
                                                          const int32_t* __restrict__ handed_over,
                                                          const uint64_t* __restrict__ hit_offset, uint32_t* __restrict__ list_step,
                                                          uint32_t* __restrict__ list_pixel, RectRec rec, PackedHits packed) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_records) return;
  const uint32_t p = ovf.pixel[r];
  uint32_t ordinal = ovf.ordinal[r];
  if (POINTS && (ordinal & OVERFLOW_LEAN)) {
    if (handed_over[p]) return;
    ordinal &= ~OVERFLOW_LEAN;
  }
  const uint64_t k = hit_offset[p] + ordinal;
  list_step[k] = ovf.step[r];
  list_pixel[k] = p;
  rec_copy(rec, k, ovf, r);
  if (POINTS) {
    const uint32_t tag = ovf_packed.color_tag[r];
    packed.color_tag[k] = tag;
    if (tag != ATMRT_COLOR_TERRAIN) packed_copy(packed, k, ovf_packed, r);
  }
}

// pelev / plen [h][n_path_cap] -> [n_path_cap][h] for k_fast_trace (lanes = rows)
__global__ __launch_bounds__(256) void k_paths_transpose(Frame f, const double* __restrict__ pelev, const double* __restrict__ plen,
                                                         const int32_t* __restrict__ npath, double* __restrict__ pelev_t,
                                                         double* __restrict__ plen_t) {
  const int y = blockIdx.y * blockDim.x + threadIdx.x; // rows on grid.y (h < 32768), samples on grid.x (up to 4e6)
  const int i = blockIdx.x;
  if (y >= f.h) return;
  const bool have = i < npath[y]; // entries past the end of a row's path were never written
  const size_t src = (size_t)y * f.n_path_cap + i, dst = (size_t)i * f.h + y;
  pelev_t[dst] = have ? pelev[src] : 0.0;
  plen_t[dst] = have ? plen[src] : 0.0;
}

// ---------------------------------------------------------------------------------------------
// exclusive scan of hit_count (u32) into hit_offset (u64): block sums -> one-block scan -> apply
// ---------------------------------------------------------------------------------------------
constexpr int SCAN_ITEMS = 8; // per thread
__global__ __launch_bounds__(256) void k_scan_block_sums(const uint32_t* __restrict__ in, size_t n,
                                                         uint64_t* __restrict__ block_sums) {
  __shared__ unsigned long long sh[4];
  size_t base = ((size_t)blockIdx.x * 256 + threadIdx.x) * SCAN_ITEMS;
  unsigned long long v = 0;
  for (int k = 0; k < SCAN_ITEMS; k++)
    if (base + k < n) v += in[base + k];
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) block_sums[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}
__global__ __launch_bounds__(256) void k_scan_sums(uint64_t* __restrict__ block_sums, size_t n_blocks,
                                                   unsigned long long* __restrict__ total) {
  __shared__ unsigned long long sh[256];
  size_t per = (n_blocks + 255) / 256;
  size_t b0 = (size_t)threadIdx.x * per, b1 = b0 + per < n_blocks ? b0 + per : n_blocks;
  unsigned long long v = 0;
  for (size_t b = b0; b < b1; b++) v += block_sums[b];
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) { // Hillis–Steele inclusive scan
    unsigned long long t = threadIdx.x >= (unsigned)off ? sh[threadIdx.x - off] : 0;
    __syncthreads();
    sh[threadIdx.x] += t;
    __syncthreads();
  }
  unsigned long long run = sh[threadIdx.x] - v;
  for (size_t b = b0; b < b1; b++) {
    unsigned long long t = block_sums[b];
    block_sums[b] = run;
    run += t;
  }
  if (threadIdx.x == 255) *total = sh[255];
}
__global__ __launch_bounds__(256) void k_scan_apply(const uint32_t* __restrict__ in, size_t n,
                                                    const uint64_t* __restrict__ block_sums,
                                                    uint64_t* __restrict__ out) {
  __shared__ unsigned long long sh[256];
  size_t base = ((size_t)blockIdx.x * 256 + threadIdx.x) * SCAN_ITEMS;
  unsigned vals[SCAN_ITEMS];
  unsigned long long v = 0;
  for (int k = 0; k < SCAN_ITEMS; k++) {
    vals[k] = base + k < n ? in[base + k] : 0u;
    v += vals[k];
  }
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    unsigned long long t = threadIdx.x >= (unsigned)off ? sh[threadIdx.x - off] : 0;
    __syncthreads();
    sh[threadIdx.x] += t;
    __syncthreads();
  }
  unsigned long long run = block_sums[blockIdx.x] + sh[threadIdx.x] - v;
  for (int k = 0; k < SCAN_ITEMS; k++) {
    if (base + k < n) out[base + k] = run;
    run += vals[k];
  }
}

// opaque mode: dense first hits -> packed list (pixel order)
__global__ __launch_bounds__(256) void k_pack_first_hits(Frame f, const uint64_t* __restrict__ hit_offset,
                                                         DensePlanes d, PackedHits packed) {
  size_t plane = (size_t)f.wl * f.h;
  size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= plane || d.hit_count[p] == 0) return;
  TracePointDev tp;
  tp.lat = d.lat[p];
  tp.lon = d.lon[p];
  tp.distance = d.distance[p];
  tp.elevation = d.elevation[p];
  tp.path_length = d.path_length[p];
  tp.normal = v3(d.normal[p], d.normal[plane + p], d.normal[2 * plane + p]);
  store_packed(packed, hit_offset[p], tp, f.p.terrain_alpha);
}


// ---------------------------------------------------------------------------------------------
// InterpolatingRectilinear (interpolating_rectilinear.rs): pinhole ray table -> angular lattice ->
// the lattice frame goes through the Fast pipeline above -> 4-corner blend per pixel.
// ---------------------------------------------------------------------------------------------

// gen_fov_data :456-468: ray_params_table for the FULL image (the lattice steps are global minima)
__global__ __launch_bounds__(256) void k_fov_table(Frame f, double* __restrict__ dir, double* __restrict__ elev) {
  int x = blockIdx.x * blockDim.x + threadIdx.x;
  int y = blockIdx.y;
  if (x >= f.p.width) return;
  double d, e;
  rect_ray_params(f.p, f.ph, x, y, d, e);
  dir[(size_t)y * f.p.width + x] = d;
  elev[(size_t)y * f.p.width + x] = e;
}
// min_elev_step per column :470-491 and min_dir_step per row :493-517 (before the global min and * SCALE)
// Both are minima over a whole column / row; they are folded in parallel (the values are positive, so their bit patterns order
// like the numbers and an integer atomicMin merges the partial results exactly).
constexpr int FOV_ROW_CHUNKS = 32;
__global__ __launch_bounds__(256) void k_fov_colmin_init(Frame f, double* __restrict__ colmin) {
  int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x < f.p.width) colmin[x] = dm_to_radians(360.0);
}
__global__ __launch_bounds__(256) void k_fov_colmin(Frame f, const double* __restrict__ elev, double* __restrict__ colmin) {
  int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= f.p.width) return;
  const int W = f.p.width, H = f.p.height;
  const int per = (H - 1 + FOV_ROW_CHUNKS - 1) / FOV_ROW_CHUNKS;
  const int y0 = 1 + blockIdx.y * per, y1 = y0 + per < H ? y0 + per : H; // this block's diffs: rows y0 .. y1 - 1 against y - 1
  if (y0 >= y1) return;
  const double min_diff = dm_to_radians(f.p.frame.fov) / (double)f.p.width / 3.0;
  double mn = dm_to_radians(360.0), last = elev[(size_t)(y0 - 1) * W + x];
  for (int y = y0; y < y1; y++) {
    double next = elev[(size_t)y * W + x];
    double diff = dm_fabs(next - last);
    if (diff < min_diff) diff = min_diff;
    if (diff < mn) mn = diff;
    last = next;
  }
  atomicMin((unsigned long long*)&colmin[x], (unsigned long long)dm_bits(mn));
}
__global__ __launch_bounds__(256) void k_fov_rowmin(Frame f, const double* __restrict__ dir, double* __restrict__ rowmin) {
  const int y = blockIdx.x * 4 + (threadIdx.x >> 6); // one row per wavefront
  const int lane = threadIdx.x & 63;
  if (y >= f.p.height) return;
  const int W = f.p.width;
  const double full = dm_to_radians(360.0);
  const double min_diff = dm_to_radians(f.p.frame.fov) / (double)f.p.width / 3.0;
  const double* row = dir + (size_t)y * W;
  double mn = full;
  for (int x = 1 + lane; x < W; x += 64) {
    double diff = dm_fabs(row[x] - row[x - 1]);
    if (diff > full) diff -= full;
    if (diff < min_diff) diff = min_diff;
    if (diff < mn) mn = diff;
  }
  for (int o = 32; o; o >>= 1) {
    const double v = __shfl_xor(mn, o, 64);
    mn = v < mn ? v : mn;
  }
  if (lane == 0) rowmin[y] = mn;
}

static __device__ __forceinline__ int sat_i32(double v) { // Rust `f as i32`
  if (v != v) return 0;
  if (v <= -2147483648.0) return (int)0x80000000;
  if (v >= 2147483647.0) return 2147483647;
  return (int)v;
}

// FovData::cache_coords :186-204 for every pixel of the shard + bounds of the referenced lattice.  Grid-stride over
// pixels; each block folds its bounds through LDS and issues four atomics (one word per bound would otherwise see one
// atomic per wavefront: 5.9 ms at the headline size, now 0.1 ms).
__global__ __launch_bounds__(256) void k_lattice_keys(Frame f, InterpBuffers ib, double min_elev_step, double min_dir_step) {
  __shared__ int sh[4][4];
  const size_t npx = (size_t)f.wl * f.h;
  int ei = 0x7fffffff, di = 0x7fffffff, ej = (int)0x80000000, dj = (int)0x80000000;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < npx; p += (size_t)gridDim.x * blockDim.x) {
    const int y = (int)(p / (size_t)f.wl), x = (int)(p % (size_t)f.wl);
    const size_t src = (size_t)y * f.p.width + f.c0 + x;
    const double ef = ib.elev[src] / min_elev_step, df = ib.dir[src] / min_dir_step;
    const int e = sat_i32(dm_floor(ef)), d = sat_i32(dm_floor(df));
    ib.key_e[p] = e;
    ib.key_d[p] = d;
    ib.rem_e[p] = ef - (double)e;
    ib.rem_d[p] = df - (double)d;
    ei = e < ei ? e : ei;
    ej = e > ej ? e : ej;
    di = d < di ? d : di;
    dj = d > dj ? d : dj;
  }
  for (int off = 32; off > 0; off >>= 1) {
    int a = __shfl_down(ei, off, 64), b = __shfl_down(di, off, 64), c = __shfl_down(ej, off, 64), d = __shfl_down(dj, off, 64);
    ei = a < ei ? a : ei;
    di = b < di ? b : di;
    ej = c > ej ? c : ej;
    dj = d > dj ? d : dj;
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sh[wave][0] = ei; sh[wave][1] = ej; sh[wave][2] = di; sh[wave][3] = dj;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++) {
      ei = sh[w][0] < ei ? sh[w][0] : ei;
      ej = sh[w][1] > ej ? sh[w][1] : ej;
      di = sh[w][2] < di ? sh[w][2] : di;
      dj = sh[w][3] > dj ? sh[w][3] : dj;
    }
    if (ei != 0x7fffffff) {
      atomicMin(&ib.bounds[0], ei);
      atomicMax(&ib.bounds[1], ej);
      atomicMin(&ib.bounds[2], di);
      atomicMax(&ib.bounds[3], dj);
    }
  }
}

// TracePoint incl. colour, generators/mod.rs:21-30
struct FullTP {
  double lat, lon, distance, elevation, path_length;
  Vec3 normal;
  uint32_t tag;
  double rgba[4];
};
static __device__ __forceinline__ FullTP load_tp(const PackedHits& h, uint64_t k) {
  FullTP t;
  t.lat = h.lat[k];
  t.lon = h.lon[k];
  t.distance = h.distance[k];
  t.elevation = h.elevation[k];
  t.path_length = h.path_length[k];
  t.normal = v3(h.normal[3 * k], h.normal[3 * k + 1], h.normal[3 * k + 2]);
  t.tag = h.color_tag[k];
  for (int q = 0; q < 4; q++) t.rgba[q] = h.rgba[4 * k + q];
  return t;
}
static __device__ __forceinline__ void store_tp(const PackedHits& h, uint64_t k, const FullTP& t) {
  h.lat[k] = t.lat;
  h.lon[k] = t.lon;
  h.distance[k] = t.distance;
  h.elevation[k] = t.elevation;
  h.path_length[k] = t.path_length;
  h.normal[3 * k] = t.normal.x;
  h.normal[3 * k + 1] = t.normal.y;
  h.normal[3 * k + 2] = t.normal.z;
  h.color_tag[k] = t.tag;
  for (int q = 0; q < 4; q++) h.rgba[4 * k + q] = t.rgba[q];
}
// TracePoint::interpolate (generators/mod.rs:33-43) + PixelColor::interpolate (:67-79)
static __device__ FullTP tp_interpolate(const FullTP& a, const FullTP& b, double c) {
  FullTP r;
  r.lat = a.lat * (1.0 - c) + b.lat * c;
  r.lon = a.lon * (1.0 - c) + b.lon * c;
  r.distance = a.distance * (1.0 - c) + b.distance * c;
  r.elevation = a.elevation * (1.0 - c) + b.elevation * c;
  r.path_length = a.path_length * (1.0 - c) + b.path_length * c;
  r.normal = v3(a.normal.x * (1.0 - c) + b.normal.x * c, a.normal.y * (1.0 - c) + b.normal.y * c,
                a.normal.z * (1.0 - c) + b.normal.z * c);
  if (a.tag == ATMRT_COLOR_TERRAIN && b.tag == ATMRT_COLOR_TERRAIN) {
    r.tag = ATMRT_COLOR_TERRAIN;
    r.rgba[0] = r.rgba[1] = r.rgba[2] = 0.0;
    r.rgba[3] = a.rgba[3] * (1.0 - c) + b.rgba[3] * c;
  } else if (a.tag == ATMRT_COLOR_RGBA && b.tag == ATMRT_COLOR_RGBA) {
    r.tag = ATMRT_COLOR_RGBA;
    for (int q = 0; q < 4; q++) r.rgba[q] = a.rgba[q] * (1.0 - c) + b.rgba[q] * c;
  } else {
    r.tag = ATMRT_COLOR_TERRAIN;
    r.rgba[0] = r.rgba[1] = r.rgba[2] = 0.0;
    r.rgba[3] = a.tag == ATMRT_COLOR_TERRAIN ? a.rgba[3] : b.rgba[3];
  }
  return r;
}

// Trace points of the four corner pixels together that the in-register member list holds; pixels with more are blended by
// k_interp_blend_big over a member arena in HBM.  4 = no middle instance: a 64-member in-register instance (round 1) cost 230-274
// VGPRs and 0.5-1 KB of scratch for its arrays, the arena instance needs 48-148 VGPRs and none — interpolating frame at
// terrain_alpha 0.5: 33.3 ms with 64, 26.5 (32), 20.7 (16), 20.1 ms with 4; config 5: 67.6 -> 53.5 ms.
#ifndef ATMRT_INTERP_MEMBERS
#define ATMRT_INTERP_MEMBERS 4
#endif
constexpr int INTERP_MEMBERS = ATMRT_INTERP_MEMBERS;

// interpolate_trace_points :267-337 on the group's corner members (index -1 = None)
static __device__ bool interp_group(const LatticeResult& lr, const uint64_t* member_k, const int e[4], double re, double rd,
                                    FullTP& out) {
  int mask = (e[0] >= 0 ? 1 : 0) | (e[1] >= 0 ? 2 : 0) | (e[2] >= 0 ? 4 : 0) | (e[3] >= 0 ? 8 : 0);
  auto tp = [&](int c) { return load_tp(lr.hits, member_k[e[c]]); };
  auto two_adjacent = [&](int c0, int c1, double rem_elev, double rem_dir) { // :339-350
    if (rem_elev >= 0.5) return false;
    out = tp_interpolate(tp(c0), tp(c1), rem_dir);
    return true;
  };
  auto two_diagonal = [&](int c0, int c1, double rem_elev, double rem_dir) { // :352-364
    if ((rem_elev >= 0.5 && rem_dir < 0.5) || (rem_elev < 0.5 && rem_dir >= 0.5)) return false;
    double coeff = rem_elev * rem_dir / (rem_elev * rem_dir + (1.0 - rem_elev) * (1.0 - rem_dir));
    out = tp_interpolate(tp(c0), tp(c1), coeff);
    return true;
  };
  auto three = [&](int c0, int c1, int c2, double rem_elev, double rem_dir) { // :366-380
    if (rem_elev >= 0.5 && rem_dir >= 0.5) return false;
    double sum = 1.0 - rem_elev + rem_elev * (1.0 - rem_dir);
    FullTP in = tp_interpolate(tp(c0), tp(c1), rem_dir);
    out = tp_interpolate(in, tp(c2), rem_elev * (1.0 - rem_dir) / sum);
    return true;
  };
  switch (mask) {
    case 0: return false;
    case 1: if (re < 0.5 && rd < 0.5) { out = tp(0); return true; } return false;
    case 2: if (re < 0.5 && rd >= 0.5) { out = tp(1); return true; } return false;
    case 4: if (re >= 0.5 && rd < 0.5) { out = tp(2); return true; } return false;
    case 8: if (re >= 0.5 && rd >= 0.5) { out = tp(3); return true; } return false;
    case 1 | 2: return two_adjacent(0, 1, re, rd);
    case 1 | 4: return two_adjacent(0, 2, rd, re);
    case 1 | 8: return two_diagonal(0, 3, re, rd);
    case 2 | 4: return two_diagonal(1, 2, re, 1.0 - rd);
    case 2 | 8: return two_adjacent(1, 3, 1.0 - rd, re);
    case 4 | 8: return two_adjacent(2, 3, 1.0 - re, rd);
    case 1 | 2 | 4: return three(0, 1, 2, re, rd);
    case 1 | 2 | 8: return three(1, 0, 3, re, 1.0 - rd);
    case 1 | 4 | 8: return three(0, 3, 2, 1.0 - re, rd);
    case 2 | 4 | 8: return three(3, 2, 1, 1.0 - re, 1.0 - rd);
    default: {
      FullTP i1 = tp_interpolate(tp(0), tp(1), rd);
      FullTP i2 = tp_interpolate(tp(2), tp(3), rd);
      out = tp_interpolate(i1, i2, re);
      return true;
    }
  }
}

// collect_trace_points :213-243 + match_sequence :245-265 + interpolate_trace_points per group for one pixel: the members
// (trace points of the four corners, corner by corner) are grouped — a point joins the first group, in creation order, that
// holds a point of its class within step_size of its distance — and every group is blended.  Returns the number of trace
// points of the pixel; FILL writes them at k_out.  The member arrays hold at least the corners' total number of points.
template <bool FILL, class GroupT>
static __device__ __forceinline__ unsigned blend_members(const LatticeResult& lr, const size_t corner[4], double rem_elev,
                                                         double rem_dir, double step_size, uint64_t* member_k, double* member_dist,
                                                         uint8_t* member_corner, uint8_t* member_tag, GroupT* member_group,
                                                         uint64_t k_out, const PackedHits& packed) {
  int n_members = 0, n_groups = 0;
  for (int c = 0; c < 4; c++) {
    uint64_t k0 = lr.hit_offset[corner[c]];
    uint32_t cnt = lr.hit_count[corner[c]];
    for (uint32_t q = 0; q < cnt; q++) {
      double dist = lr.hits.distance[k0 + q];
      uint8_t tag = (uint8_t)lr.hits.color_tag[k0 + q];
      int found = -1;
      for (int g = 0; g < n_groups && found < 0; g++) // first group (creation order) with any close point of the same class
        for (int m = 0; m < n_members; m++)
          if ((int)member_group[m] == g && dm_fabs(dist - member_dist[m]) < step_size && tag == member_tag[m]) {
            found = g;
            break;
          }
      if (found < 0) found = n_groups++;
      member_k[n_members] = k0 + q;
      member_dist[n_members] = dist;
      member_corner[n_members] = (uint8_t)c;
      member_tag[n_members] = tag;
      member_group[n_members] = (GroupT)found;
      n_members++;
    }
  }
  unsigned count = 0;
  for (int g = 0; g < n_groups; g++) {
    int e[4] = {-1, -1, -1, -1};
    for (int m = 0; m < n_members; m++)
      if ((int)member_group[m] == g) e[member_corner[m]] = m; // later entries overwrite, :247-263
    FullTP tp;
    if (interp_group(lr, member_k, e, rem_elev, rem_dir, tp)) {
      if (FILL) store_tp(packed, k_out + count, tp);
      count++;
    }
  }
  return count;
}

// interpolate :395-418 with collect_trace_points :213-243 and match_sequence :245-265
// CAP = 4: the pixels whose four lattice corners hold at most four trace points together (nearly all of them) — the member
// arrays are four registers wide; it also writes what does not depend on the members (referenced marks, blended angles) and sizes
// the arena of k_interp_blend_big, which blends the others.  (A middle instance, CAP = INTERP_MEMBERS > 4, exists in the template
// but is not launched: see INTERP_MEMBERS.)
template <bool FILL, int CAP>
__global__ __launch_bounds__(256) void k_interp_blend(Frame f, InterpBuffers ib, LatticeResult lr, DensePlanes out,
                                                      const uint64_t* __restrict__ hit_offset, PackedHits packed,
                                                      unsigned long long* __restrict__ counters) {
  int x = blockIdx.x * blockDim.x + threadIdx.x;
  int y = blockIdx.y;
  if (x >= f.wl) return;
  const size_t p = (size_t)y * f.wl + x;
  const double rem_elev = ib.rem_e[p], rem_dir = ib.rem_d[p];
  const double step_size = f.p.simulation_step;
  size_t corner[4]; // SEQUENCE = (0,0) (0,1) (1,0) (1,1): (elev_index + i, dir_index + j)
  for (int s = 0; s < 4; s++)
    corner[s] = (size_t)(ib.key_e[p] + (s >> 1) - f.ei0) * lr.nd + (size_t)(ib.key_d[p] + (s & 1) - f.di0);
  uint32_t total = 0;
  for (int c = 0; c < 4; c++) {
    if (!FILL && CAP == 4) ib.referenced[corner[c]] = 1;
    total += lr.hit_count[corner[c]];
  }
  if (!FILL && CAP == 4) {
    double e0 = lr.elevation_angle[corner[0]], e1 = lr.elevation_angle[corner[1]], e2 = lr.elevation_angle[corner[2]],
           e3 = lr.elevation_angle[corner[3]];
    double a0 = lr.azimuth[corner[0]], a1 = lr.azimuth[corner[1]], a2 = lr.azimuth[corner[2]], a3 = lr.azimuth[corner[3]];
    out.elevation_angle[p] = e0 * (1.0 - rem_elev) * (1.0 - rem_dir) + e1 * (1.0 - rem_elev) * rem_dir +
                             e2 * rem_elev * (1.0 - rem_dir) + e3 * rem_elev * rem_dir;
    out.azimuth[p] = a0 * (1.0 - rem_elev) * (1.0 - rem_dir) + a1 * (1.0 - rem_elev) * rem_dir + a2 * rem_elev * (1.0 - rem_dir) +
                     a3 * rem_elev * rem_dir;
  }
  if (!FILL && CAP == 4 && total > (uint32_t)INTERP_MEMBERS) { // k_interp_blend_big's pixel: size its member arena
    atomicAdd(&counters[CTR_BIG_BLEND_PIXELS], 1ull);
    atomicAdd(&counters[CTR_BIG_BLEND_POINTS], (unsigned long long)total);
  }
  if (CAP == 4 ? total > 4u : (total <= 4u || total > (uint32_t)INTERP_MEMBERS)) return; // another instance's pixel
  uint64_t member_k[CAP];
  double member_dist[CAP];
  uint8_t member_corner[CAP], member_tag[CAP], member_group[CAP];
  const unsigned count = blend_members<FILL>(lr, corner, rem_elev, rem_dir, step_size, member_k, member_dist, member_corner, member_tag,
                                             member_group, FILL ? hit_offset[p] : 0, packed);
  if (!FILL) out.hit_count[p] = count;
}

// The pixels whose four lattice corners hold more than INTERP_MEMBERS trace points together (the reference's Vec has no bound,
// interpolating_rectilinear.rs:213-243): same grouping and blend, member list in an HBM arena handed out by an atomic cursor
// (each pixel's range is private, so the order in which pixels take their ranges does not matter).
template <bool FILL>
__global__ __launch_bounds__(256) void k_interp_blend_big(Frame f, InterpBuffers ib, LatticeResult lr, DensePlanes out,
                                                          const uint64_t* __restrict__ hit_offset, PackedHits packed,
                                                          BlendArena arena, unsigned long long* __restrict__ counters) {
  int x = blockIdx.x * blockDim.x + threadIdx.x;
  int y = blockIdx.y;
  if (x >= f.wl) return;
  const size_t p = (size_t)y * f.wl + x;
  size_t corner[4];
  uint32_t total = 0;
  for (int s = 0; s < 4; s++) {
    corner[s] = (size_t)(ib.key_e[p] + (s >> 1) - f.ei0) * lr.nd + (size_t)(ib.key_d[p] + (s & 1) - f.di0);
    total += lr.hit_count[corner[s]];
  }
  if (total <= (uint32_t)INTERP_MEMBERS) return;
  const unsigned long long base = atomicAdd(&counters[CTR_BLEND_CURSOR], (unsigned long long)total);
  const unsigned count = blend_members<FILL>(lr, corner, ib.rem_e[p], ib.rem_d[p], f.p.simulation_step, arena.k + base, arena.dist + base,
                                             arena.corner + base, arena.tag + base, arena.group + base, FILL ? hit_offset[p] : 0, packed);
  if (!FILL) out.hit_count[p] = count;
}


// ray-steps of the lattice pixels the image actually references (the reference memoises exactly those); grid-stride,
// one atomic per block
__global__ __launch_bounds__(256) void k_lattice_steps(size_t n, const uint8_t* __restrict__ referenced,
                                                       const uint32_t* __restrict__ px_steps,
                                                       unsigned long long* __restrict__ counters) {
  __shared__ unsigned long long sh[4];
  unsigned long long v = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    if (referenced[i]) v += px_steps[i];
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    v = sh[0] + sh[1] + sh[2] + sh[3];
    if (v) atomicAdd(&counters[CTR_RAY_STEPS], v);
  }
}

void launch_fov_table(const Frame& f, const InterpBuffers& ib, hipStream_t stream) {
  hipLaunchKernelGGL(k_fov_table, dim3(cdiv(f.p.width, 256), f.p.height), dim3(256), 0, stream, f, ib.dir, ib.elev);
  hipLaunchKernelGGL(k_fov_colmin_init, dim3(cdiv(f.p.width, 256)), dim3(256), 0, stream, f, ib.colmin);
  hipLaunchKernelGGL(k_fov_colmin, dim3(cdiv(f.p.width, 256), FOV_ROW_CHUNKS), dim3(256), 0, stream, f, ib.elev, ib.colmin);
  hipLaunchKernelGGL(k_fov_rowmin, dim3(cdiv(f.p.height, 4)), dim3(256), 0, stream, f, ib.dir, ib.rowmin);
}
void launch_lattice_keys(const Frame& f, const InterpBuffers& ib, double min_elev_step, double min_dir_step, hipStream_t stream) {
  const size_t npx = (size_t)f.wl * f.h;
  hipLaunchKernelGGL(k_lattice_keys, dim3(npx < 1024 * 256 ? cdiv(npx, 256) : 1024), dim3(256), 0, stream, f, ib, min_elev_step,
                     min_dir_step);
}
void launch_interp_blend(const Frame& f, Workspace& ws, const InterpBuffers& ib, const LatticeResult& lr, bool fill,
                         const DensePlanes& dense, const PackedHits& packed, hipStream_t stream) {
  dim3 grid(cdiv(f.wl, 256), f.h);
  if (fill) {
    hipLaunchKernelGGL((k_interp_blend<true, 4>), grid, dim3(256), 0, stream, f, ib, lr, dense, ws.hit_offset, packed,
                       (unsigned long long*)ws.counters);
    if (INTERP_MEMBERS > 4)
      hipLaunchKernelGGL((k_interp_blend<true, INTERP_MEMBERS>), grid, dim3(256), 0, stream, f, ib, lr, dense, ws.hit_offset, packed,
                         (unsigned long long*)ws.counters);
  } else {
    hipLaunchKernelGGL((k_interp_blend<false, 4>), grid, dim3(256), 0, stream, f, ib, lr, dense, (const uint64_t*)nullptr, packed,
                       (unsigned long long*)ws.counters);
    if (INTERP_MEMBERS > 4)
      hipLaunchKernelGGL((k_interp_blend<false, INTERP_MEMBERS>), grid, dim3(256), 0, stream, f, ib, lr, dense, (const uint64_t*)nullptr,
                         packed, (unsigned long long*)ws.counters);
  }
}
void launch_interp_blend_big(const Frame& f, Workspace& ws, const InterpBuffers& ib, const LatticeResult& lr, bool fill,
                             const DensePlanes& dense, const PackedHits& packed, const BlendArena& arena, hipStream_t stream) {
  dim3 grid(cdiv(f.wl, 256), f.h);
  (void)hipMemsetAsync(&ws.counters[CTR_BLEND_CURSOR], 0, sizeof(uint64_t), stream);
  if (fill)
    hipLaunchKernelGGL((k_interp_blend_big<true>), grid, dim3(256), 0, stream, f, ib, lr, dense, ws.hit_offset, packed, arena,
                       (unsigned long long*)ws.counters);
  else
    hipLaunchKernelGGL((k_interp_blend_big<false>), grid, dim3(256), 0, stream, f, ib, lr, dense, (const uint64_t*)nullptr, packed,
                       arena, (unsigned long long*)ws.counters);
}
void launch_interp_finish(const Frame& f, Workspace& ws, const InterpBuffers& ib, const LatticeResult& lr,
                          const DensePlanes& dense, const PackedHits& packed, hipStream_t stream) {
  size_t n = (size_t)lr.nd * lr.ne;
  hipLaunchKernelGGL(k_lattice_steps, dim3(n < 1024 * 256 ? cdiv(n, 256) : 1024), dim3(256), 0, stream, n, ib.referenced, lr.px_steps,
                     (unsigned long long*)ws.counters);
  hipLaunchKernelGGL(k_dense_from_packed, dim3(cdiv(f.wl, 256), f.h), dim3(256), 0, stream, f, ws.hit_offset, packed, dense, 0);
}


// ---------------------------------------------------------------------------------------------
// renderer::draw_image (renderer/mod.rs:385-414) — front-to-back alpha compositing of each
// pixel's trace points with the colouring method and optional fog; 3 B per pixel leave the kernel instead of 88.
// PACKED: trace points from the packed lists; otherwise from the dense first-hit planes (opaque frames).
// ---------------------------------------------------------------------------------------------
// SHADOWED (include/atmrt.h, "cast shadows"): under Shading the first trace point of a pixel whose status is ATMRT_SHADOW_SHADOWED
// takes light_dot = 0.0 — a zero normal gives exactly that (0 >= 0.0 keeps it, whatever the zero's sign) — so its brightness is
// ambient_light.  One body for both kernels; the plain kernel's instantiations carry nothing of the status plane.
template <bool PACKED, bool SHADOWED>
static __device__ __forceinline__ void draw_pixel(size_t n_pixels, const atmrt_coloring_t& col, double terrain_alpha,
                                                  const uint32_t* __restrict__ hit_count, const uint64_t* __restrict__ hit_offset,
                                                  const PackedHits& hits, const DensePlanes& dense, const uint8_t* __restrict__ status,
                                                  uint8_t* __restrict__ rgb) {
  size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pixels) return;
  Rgb8 result{{0, 0, 0}};
  double accum_neg_alpha = 1.0;
  const uint32_t cnt = hit_count[p];
  const uint64_t k0 = PACKED ? hit_offset[p] : 0;
  for (uint32_t q = 0; q < cnt; q++) {
    double distance, elevation, path_length, nx, ny, nz, r = 0.0, g = 0.0, b = 0.0, alpha;
    uint32_t tag;
    if (PACKED) {
      uint64_t k = k0 + q;
      distance = hits.distance[k]; elevation = hits.elevation[k]; path_length = hits.path_length[k];
      nx = hits.normal[3 * k]; ny = hits.normal[3 * k + 1]; nz = hits.normal[3 * k + 2];
      tag = hits.color_tag[k];
      r = hits.rgba[4 * k]; g = hits.rgba[4 * k + 1]; b = hits.rgba[4 * k + 2]; alpha = hits.rgba[4 * k + 3];
    } else {
      distance = dense.distance[p]; elevation = dense.elevation[p]; path_length = dense.path_length[p];
      nx = dense.normal[p]; ny = dense.normal[n_pixels + p]; nz = dense.normal[2 * n_pixels + p];
      tag = ATMRT_COLOR_TERRAIN;
      alpha = terrain_alpha;
    }
    if (SHADOWED && q == 0 && status[p] == ATMRT_SHADOW_SHADOWED) nx = ny = nz = 0.0;
    Rgb8 c1 = col.kind == ATMRT_COLORING_SIMPLE ? simple_color(col, distance, elevation)
                                                 : shading_color(col, nx, ny, nz, elevation, tag, r, g, b);
    Rgb8 c2 = col.has_fog ? apply_fog(col.fog_distance, path_length, c1) : c1;
    result = add_rgb(result, c2, accum_neg_alpha * alpha);
    accum_neg_alpha *= 1.0 - alpha;
  }
  result = add_rgb(result, default_color(col), accum_neg_alpha);
  rgb[3 * p] = result.c[0];
  rgb[3 * p + 1] = result.c[1];
  rgb[3 * p + 2] = result.c[2];
}
template <bool PACKED>
__global__ __launch_bounds__(256) void k_draw_image(size_t n_pixels, atmrt_coloring_t col, double terrain_alpha,
                                                    const uint32_t* __restrict__ hit_count,
                                                    const uint64_t* __restrict__ hit_offset, PackedHits hits, DensePlanes dense,
                                                    uint8_t* __restrict__ rgb) {
  draw_pixel<PACKED, false>(n_pixels, col, terrain_alpha, hit_count, hit_offset, hits, dense, nullptr, rgb);
}
template <bool PACKED>
__global__ __launch_bounds__(256) void k_draw_image_shadowed(size_t n_pixels, atmrt_coloring_t col, double terrain_alpha,
                                                             const uint32_t* __restrict__ hit_count,
                                                             const uint64_t* __restrict__ hit_offset, PackedHits hits, DensePlanes dense,
                                                             const uint8_t* __restrict__ status, uint8_t* __restrict__ rgb) {
  draw_pixel<PACKED, true>(n_pixels, col, terrain_alpha, hit_count, hit_offset, hits, dense, status, rgb);
}

void launch_draw_image(size_t n_pixels, const atmrt_coloring_t& col, double terrain_alpha, bool packed_valid,
                       const uint32_t* hit_count, const uint64_t* hit_offset, const PackedHits& hits, const DensePlanes& dense,
                       uint8_t* rgb, hipStream_t stream) {
  if (packed_valid)
    hipLaunchKernelGGL((k_draw_image<true>), dim3(cdiv(n_pixels, 256)), dim3(256), 0, stream, n_pixels, col, terrain_alpha,
                       hit_count, hit_offset, hits, dense, rgb);
  else
    hipLaunchKernelGGL((k_draw_image<false>), dim3(cdiv(n_pixels, 256)), dim3(256), 0, stream, n_pixels, col, terrain_alpha,
                       hit_count, hit_offset, hits, dense, rgb);
}
void launch_draw_image_shadowed(size_t n_pixels, const atmrt_coloring_t& col, double terrain_alpha, bool packed_valid,
                                const uint32_t* hit_count, const uint64_t* hit_offset, const PackedHits& hits, const DensePlanes& dense,
                                const uint8_t* status, uint8_t* rgb, hipStream_t stream) {
  if (packed_valid)
    hipLaunchKernelGGL((k_draw_image_shadowed<true>), dim3(cdiv(n_pixels, 256)), dim3(256), 0, stream, n_pixels, col, terrain_alpha,
                       hit_count, hit_offset, hits, dense, status, rgb);
  else
    hipLaunchKernelGGL((k_draw_image_shadowed<false>), dim3(cdiv(n_pixels, 256)), dim3(256), 0, stream, n_pixels, col, terrain_alpha,
                       hit_count, hit_offset, hits, dense, status, rgb);
}

// ---------------------------------------------------------------------------------------------
// the annotations of renderer::output_image (kernels: atmrt_overlay.h)
// ---------------------------------------------------------------------------------------------
// Bands of k_overlay_find_elev.  The scan is a pure stream, so what matters is bytes in flight: a wavefront holds 4 row loads of
// 512 B, and 6.3 TB/s over a miss latency of the order of a microsecond is some 6 MB in flight, 24 KB per CU of 256 — 12 wavefronts
// per CU; 16 are asked for (half of the 32 a CU can hold, this kernel needs few registers).  W / 64 wavefronts per band give
// bands = 16 CUs / (W / 64): 64 bands of 32 rows at 4096 x 2048, 32 bands of 128 rows at 8192 x 4096.  A band is at least 32 rows,
// so that the 24 B of partials a lane writes per band stay below a tenth of the 256 B it reads, and there are at most 256 bands.
int overlay_bands(int w, int h, int n_cu) {
  const int groups = (w + 63) / 64;
  int bands = (16 * (n_cu > 0 ? n_cu : 256) + groups - 1) / groups;
  if (bands > h / 32) bands = h / 32;
  if (bands > 256) bands = 256;
  if (bands < 1) bands = 1;
  const int rows = (h + bands - 1) / bands;
  return (h + rows - 1) / rows; // no empty band
}
size_t overlay_workspace_bytes(int w, int bands) {
  return Carve::pad((size_t)OVERLAY_TARGETS * bands * w * sizeof(double)) + Carve::pad((size_t)OVERLAY_TARGETS * bands * w * sizeof(int32_t)) +
         Carve::pad((size_t)OVERLAY_TARGETS * w * sizeof(int32_t));
}
void launch_overlay_find_elev(const double* elev, int w, int h, int bands, double t0, double t1, void* workspace, int32_t** y_of_x,
                              hipStream_t stream) {
  Carve k(workspace);
  double* part_d;
  int32_t* part_y;
  k(part_d, (size_t)OVERLAY_TARGETS * bands * w * sizeof(double));
  k(part_y, (size_t)OVERLAY_TARGETS * bands * w * sizeof(int32_t));
  k(*y_of_x, (size_t)OVERLAY_TARGETS * w * sizeof(int32_t));
  const int rows = (h + bands - 1) / bands;
  hipLaunchKernelGGL(k_overlay_find_elev, dim3(cdiv((size_t)w, 64), bands), dim3(64), 0, stream, elev, w, h, rows, t0, t1, part_d, part_y);
  hipLaunchKernelGGL(k_overlay_pick_elev, dim3(cdiv((size_t)w, 256)), dim3(256), 0, stream, elev, w, h, bands, t0, t1, part_d, part_y,
                     *y_of_x);
}
void launch_overlay_lines(const int32_t* y_of_x, int w, int h, uint8_t* rgb, const uint8_t color[3], hipStream_t stream) {
  if (w > 1)
    hipLaunchKernelGGL(k_overlay_lines, dim3(cdiv((size_t)w - 1, 256)), dim3(256), 0, stream, y_of_x, w, h, rgb, color[0], color[1], color[2]);
}
void launch_overlay_ticks(const void* ticks, int n, int w, int h, uint8_t* rgb, hipStream_t stream) {
  if (n > 0)
    hipLaunchKernelGGL(k_overlay_ticks, dim3(cdiv((size_t)n, 64)), dim3(64), 0, stream, static_cast<const OverlayTick*>(ticks), n, w, h, rgb);
}

// ---------------------------------------------------------------------------------------------
// the visibility map (kernels: atmrt_vismap.h)
// ---------------------------------------------------------------------------------------------
size_t vis_block_bytes() { return VIS_N * sizeof(unsigned long long); }
void vis_block_decode(const void* block_host, atmrt_visibility_stats_t* stats, double bounds[4]) {
  const unsigned long long* b = static_cast<const unsigned long long*>(block_host);
  if (stats) *stats = atmrt_visibility_stats_t{b[VIS_POINTS], b[VIS_BINNED], b[VIS_OUTSIDE], b[VIS_SKIPPED], b[VIS_UPDATES]};
  if (bounds)
    for (int i = 0; i < 4; i++) { // the inverse of vis_key; no point at all: the maxima are still 0
      const unsigned long long k = b[VIS_LAT_MIN + i], bits = (k >> 63) ? k & 0x7fffffffffffffffull : ~k;
      double v;
      memcpy(&v, &bits, sizeof v);
      bounds[i] = b[VIS_LAT_MAX] == 0ull ? NAN : v;
    }
}
void launch_vis_reset(void* block, hipStream_t stream) {
  hipLaunchKernelGGL(k_vis_reset, dim3(1), dim3(64), 0, stream, static_cast<unsigned long long*>(block));
}
void launch_vis_map(const TracePoints& src, const atmrt_geo_grid_t& grid, bool aggregate, uint32_t* count, double* min_distance, void* block,
                    hipStream_t stream) {
  const size_t n_cells = (size_t)grid.n_lat * grid.n_lon;
  unsigned long long* mind = reinterpret_cast<unsigned long long*>(min_distance);
  unsigned long long* ctr = static_cast<unsigned long long*>(block);
  hipLaunchKernelGGL(k_vis_clear, dim3(cdiv(n_cells, 256)), dim3(256), 0, stream, n_cells, count, mind);
  if (!src.n_pixels) return;
  const dim3 grd(cdiv(src.n_pixels, 256)), blk(256);
#define VIS_LAUNCH(PACKED, AGG) hipLaunchKernelGGL((k_vis_scatter<PACKED, AGG>), grd, blk, 0, stream, src, grid, count, mind, ctr)
  if (src.hit_offset) {
    if (aggregate) VIS_LAUNCH(true, true);
    else VIS_LAUNCH(true, false);
  } else {
    if (aggregate) VIS_LAUNCH(false, true);
    else VIS_LAUNCH(false, false);
  }
#undef VIS_LAUNCH
}
void launch_vis_bounds(const TracePoints& src, void* block, hipStream_t stream) {
  if (!src.n_pixels) return;
  const dim3 grd(cdiv(src.n_pixels, 256)), blk(256);
  unsigned long long* ctr = static_cast<unsigned long long*>(block);
  if (src.hit_offset) hipLaunchKernelGGL((k_vis_bounds<true>), grd, blk, 0, stream, src, ctr);
  else hipLaunchKernelGGL((k_vis_bounds<false>), grd, blk, 0, stream, src, ctr);
}

// ---------------------------------------------------------------------------------------------
// the landmark search (kernels: atmrt_landmarks.h)
// ---------------------------------------------------------------------------------------------
void launch_lm_reset(size_t n, const LmState& state, hipStream_t stream) {
  hipLaunchKernelGGL(k_lm_reset, dim3(cdiv(n > (size_t)LM_N ? n : (size_t)LM_N, 256)), dim3(256), 0, stream, n, state);
}
void launch_lm_pass(bool pass_b, const TracePoints& src, const LmIndex& index, const LmState& state, hipStream_t stream) {
  if (!src.n_pixels) return;
  const dim3 grd(cdiv(src.n_pixels, 256)), blk(256);
#define LM_LAUNCH(PACKED, PASS_B) hipLaunchKernelGGL((k_lm_pass<PACKED, PASS_B>), grd, blk, 0, stream, src, index, state)
  if (src.hit_offset) {
    if (pass_b) LM_LAUNCH(true, true);
    else LM_LAUNCH(true, false);
  } else {
    if (pass_b) LM_LAUNCH(false, true);
    else LM_LAUNCH(false, false);
  }
#undef LM_LAUNCH
}
void launch_lm_finish(size_t n, const TracePoints& src, const LmState& state, atmrt_landmark_hit_t* hits, hipStream_t stream) {
  hipLaunchKernelGGL(k_lm_finish, dim3(cdiv(n, 256)), dim3(256), 0, stream, n, src, state, hits);
}

// ---------------------------------------------------------------------------------------------
// harness kernels
// ---------------------------------------------------------------------------------------------
__global__ void k_get_elev(Frame f, size_t n, const double* lat, const double* lon, double* elev, uint8_t* valid) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double e = 0.0;
  bool ok = terrain_get_elev(f.tv, lat[i], lon[i], e);
  elev[i] = ok ? e : 0.0;
  valid[i] = ok ? 1 : 0;
}
__global__ void k_ray_paths(Frame f, double h0, size_t n_angles, const double* angles_deg, int straight, double step,
                            size_t n_steps, double* x, double* h) {
  size_t a = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= n_angles) return;
  const bool sph = f.earth.spherical != 0;
  Stepper s;
  stepper_init(s, sph, f.earth.shape_radius, h0, dm_to_radians(angles_deg[a]));
  size_t base = a * (n_steps + 1);
  x[base] = 0.0;
  h[base] = h0;
  for (size_t k = 1; k <= n_steps; k++) {
    RayState st = stepper_next(s, *f.atm, sph, f.earth.shape_radius, straight != 0, step);
    x[base + k] = st.x;
    h[base + k] = st.h;
  }
}
__global__ void k_atm_sample(Frame f, size_t n, const double* alt, double* t, double* p, double* nidx, double* dn) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  t[i] = atm_temperature(*f.atm, alt[i]);
  p[i] = atm_pressure(*f.atm, alt[i]);
  // n and dn/dh through the steppers' own evaluation (the first call finds the lane's layer, the second then takes the certified
  // shortcut path when the whole wavefront sits in one certified interval, the IEEE path otherwise): same values as refr_n / refr_dn
  int hint = 0;
  double nv, dv;
  refr_n_dn_hint<true>(*f.atm, alt[i], hint, nv, dv);
  refr_n_dn_hint<true>(*f.atm, alt[i], hint, nv, dv);
  nidx[i] = nv;
  dn[i] = dv;
}
__global__ void k_coords_at_dist(Frame f, double lat0, double lon0, double dir, size_t n, const double* dist, double* lat,
                                 double* lon) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Earth e = f.earth;
  e.flat_dirs &= ~EARTH_FAST_DIV; // arbitrary distances here, not a stepper's
  DirCalc c;
  dircalc_new(e, lat0, lon0, dir, c);
  coords_at_dist(e, c, dist[i], lat[i], lon[i]);
}

// Frame::xs_sin / xs_cos: the device code of coords_at_dist on the distance table, once per entry instead of once per ray and sample
__global__ void k_step_trig(Earth e, size_t n, const double* __restrict__ xs, double* __restrict__ s, double* __restrict__ c) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  spherical_sincos(e, xs[i], s[i], c[i]);
}
void launch_step_trig(const Earth& e, size_t n, const double* xs, double* s, double* c, hipStream_t stream) {
  if (n) hipLaunchKernelGGL(k_step_trig, dim3(cdiv(n, 256)), dim3(256), 0, stream, e, n, xs, s, c);
}

// Frame::normal_trig: the device code of find_normal and of the observer's calculator on their frame constants, once instead of once
// per trace point.  One wavefront; its first lane writes.
__global__ __launch_bounds__(64) void k_normal_trig(Earth e, double obs_lat, double obs_lon, NormalTrig* __restrict__ out) {
  NormalTrig t;
  normal_trig_fill(e, obs_lat, obs_lon, t);
  if (threadIdx.x == 0) *out = t;
}
void launch_normal_trig(const Earth& e, double obs_lat, double obs_lon, NormalTrig* out, hipStream_t stream) {
  hipLaunchKernelGGL(k_normal_trig, dim3(1), dim3(64), 0, stream, e, obs_lat, obs_lon, out);
}

// Frame::ceil, the terrain ceiling table (atmrt_ceiling.h).  One thread per step i and bin j: the geodesic points of the bin's two
// edge directions at xs[i], by the code a ray of the march runs (dircalc_new on the direction in degrees, coords_at_step), and the
// cover of the arc between them.  Neighbouring threads are neighbouring bins of one step: their boxes share posts.  The thread of
// bin 0 also writes the row's entry n_bins, the one of the rays outside the bins: the mosaic's top.
__global__ __launch_bounds__(256) void k_ceiling_cells(Frame f, CeilEntry* __restrict__ table) {
  const CeilLayout L = f.ceil_layout;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t rows = (size_t)f.march_steps + 1;
  if (t >= rows * (size_t)L.n_bins) return;
  const int i = (int)(t / (size_t)L.n_bins), j = (int)(t % (size_t)L.n_bins);
  Earth e = f.earth;
  e.calc = 2;
  double d_lo, d_hi, lat0, lon0, lat1, lon1;
  ceiling_bin_edges(L, j, d_lo, d_hi);
  const double dist = f.xs[i];
  DirCalc c;
  dircalc_new(e, f.p.position.latitude, f.p.position.longitude, dm_to_degrees(d_lo), c);
  coords_at_step(f, e, c, i, dist, lat0, lon0);
  dircalc_new(e, f.p.position.latitude, f.p.position.longitude, dm_to_degrees(d_hi), c);
  coords_at_step(f, e, c, i, dist, lat1, lon1);
  CeilEntry* row = table + (size_t)i * (size_t)(L.n_bins + 1);
  row[j].cell = ceiling_cell(f.tv, L, e.calc_radius, lat0, lon0, lat1, lon1, dist);
  if (j == 0) row[L.n_bins] = CeilEntry{(float)f.tv.skip_above, (float)f.tv.skip_above};
}
// suffix[i][j] = max of cell[i'][j] over i' >= i: one wavefront per bin, every lane a run of consecutive steps — the maximum of its
// run, a suffix scan of the 64 maxima across the wavefront, then the run again from its end downwards
__global__ __launch_bounds__(64) void k_ceiling_suffix(CeilEntry* __restrict__ table, int rows, int stride) {
  CeilEntry* col = table + blockIdx.x;
  const int lane = threadIdx.x, run = (rows + 63) / 64;
  const int i0 = lane * run, i1 = i0 + run < rows ? i0 + run : rows;
  float m = 0.f;
  for (int i = i0; i < i1; i++) m = fmaxf(m, col[(size_t)i * stride].cell);
  for (int off = 1; off < 64; off <<= 1) { // inclusive: the maximum of the lanes lane ... 63
    const float o = __shfl_down(m, off, 64);
    if (lane + off < 64) m = fmaxf(m, o);
  }
  float above = __shfl_down(m, 1, 64); // of the runs behind this lane's
  if (lane == 63) above = 0.f;
  for (int i = i1 - 1; i >= i0; i--) {
    above = fmaxf(above, col[(size_t)i * stride].cell);
    col[(size_t)i * stride].suffix = above;
  }
}
void launch_ceiling(const Frame& f, CeilEntry* table, hipStream_t stream) {
  const size_t rows = (size_t)f.march_steps + 1, n = rows * (size_t)f.ceil_layout.n_bins;
  if (!n) return;
  hipLaunchKernelGGL(k_ceiling_cells, dim3(cdiv(n, 256)), dim3(256), 0, stream, f, table);
  hipLaunchKernelGGL(k_ceiling_suffix, dim3((unsigned)f.ceil_layout.n_bins), dim3(64), 0, stream, table, (int)rows, f.ceil_layout.n_bins + 1);
}

// Frame::ceil_order, the work queue of the whole-frame opaque march: the groups of 64 consecutive pixels by estimated length,
// longest first.  One wavefront per group estimates the march of four rays across the group from the ceiling table (a wavefront
// marches as long as its longest ray, and its 64 pixels span a dozen bins), 16 lanes to a ray and a step to a lane
// (ceiling_estimate_ends; a thread that walks a ray alone waits for one table entry per step: 2.7 ms for the headline's 131,072
// groups against 0.1 ms), and counts the longest into its estimate's bin; one workgroup turns the counts into the start of every
// estimate's run, highest estimate first; a scatter appends every group to its run.  The order inside a run is whatever the
// atomics make it: it decides scheduling only.
__global__ __launch_bounds__(256) void k_march_length_estimate(Frame f, uint32_t n_groups, uint32_t* __restrict__ estimate,
                                                               uint32_t* __restrict__ bin_count) {
  const uint32_t g = (uint32_t)(((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6); // wave-uniform
  if (g >= n_groups) return;
  const int lane = threadIdx.x & 63, ray = lane >> 4, sub = lane & 15;
  const size_t plane = (size_t)f.wl * f.h;
  const double r_eff = f.earth.shape_radius * (7.0 / 6.0), inv_2r = f.earth.spherical && r_eff > 0.0 ? 0.5 / r_eff : 0.0;
  const double alt = observer_altitude(f);
  size_t p = (size_t)g * 64 + (size_t)(ray * 21); // pixels 0, 21, 42, 63 of the group
  p = p < plane ? p : plane - 1;
  double direction, elevation;
  rect_ray_params(f.p, f.ph, f.c0 + (int)(p % (size_t)f.wl), (int)(p / (size_t)f.wl), direction, elevation);
  const double slope = tan(elevation);
  const size_t stride = (size_t)f.ceil_layout.n_bins + 1, bin = (size_t)ceiling_bin(f.ceil_layout, direction);
  int est = f.march_steps;
  bool done = false; // of this lane's ray: the same in its 16 lanes
  for (int base = 1; base <= f.march_steps; base += 16) {
    const int i = base + sub;
    const bool ends = !done && i <= f.march_steps && ceiling_estimate_ends(f.ceil[(size_t)i * stride + bin], f.xs[i], alt, slope, inv_2r);
    const unsigned first = (unsigned)(__ballot(ends) >> (16 * ray)) & 0xffffu; // the steps base ... base + 15 of this ray that end it
    if (!done && first) est = base + __builtin_ctz(first), done = true;
    if (__all(done)) break;
  }
  for (int off = 16; off < 64; off <<= 1) { // the longest of the four
    const int o = __shfl_xor(est, off, 64);
    est = o > est ? o : est;
  }
  if (lane == 0) {
    estimate[g] = (uint32_t)est; // 1 .. march_steps
    atomicAdd(&bin_count[est], 1u);
  }
}
// bin_count[b] -> the number of groups with an estimate above b: where the run of estimate b starts.  One workgroup; every thread
// sums a stretch of consecutive bins, the stretches are scanned through LDS, then every thread walks its stretch again.
__global__ __launch_bounds__(1024) void k_march_order_scan(uint32_t* __restrict__ bin_count, uint32_t n_bins) {
  __shared__ uint32_t part[1024];
  const uint32_t t = threadIdx.x, run = (n_bins + 1023u) / 1024u;
  // stretch t, counted from the HIGHEST bin down: positions r = t run ... of the reversed bins, bin = n_bins - 1 - r
  const uint32_t r0 = t * run < n_bins ? t * run : n_bins, r1 = r0 + run < n_bins ? r0 + run : n_bins;
  uint32_t sum = 0;
  for (uint32_t r = r0; r < r1; r++) sum += bin_count[n_bins - 1u - r];
  part[t] = sum;
  __syncthreads();
  for (uint32_t off = 1; off < 1024u; off <<= 1) { // inclusive scan of the stretch sums
    const uint32_t v = t >= off ? part[t - off] : 0u;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  uint32_t start = part[t] - sum;
  for (uint32_t r = r0; r < r1; r++) {
    const uint32_t c = bin_count[n_bins - 1u - r];
    bin_count[n_bins - 1u - r] = start;
    start += c;
  }
}
__global__ __launch_bounds__(256) void k_march_order_scatter(uint32_t n_groups, const uint32_t* __restrict__ estimate,
                                                             uint32_t* __restrict__ cursor, uint32_t* __restrict__ order,
                                                             uint32_t* __restrict__ order_steps) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_groups) return;
  const uint32_t est = estimate[g], at = atomicAdd(&cursor[est], 1u);
  if (at < n_groups) order[at] = g, order_steps[at] = est; // (the runs tile 0 .. n_groups - 1: the counts of the same estimates made them)
}
void launch_march_order(const Frame& f, const MarchOrder& o, hipStream_t stream) {
  const uint32_t n_groups = (uint32_t)(((size_t)f.wl * f.h + 63) / 64), n_bins = (uint32_t)f.march_steps + 1u;
  if (!n_groups || !f.ceil) return;
  (void)hipMemsetAsync(o.bin_count, 0, (size_t)n_bins * sizeof(uint32_t), stream);
  hipLaunchKernelGGL(k_march_length_estimate, dim3(cdiv((size_t)n_groups * 64, 256)), dim3(256), 0, stream, f, n_groups, o.estimate, o.bin_count);
  hipLaunchKernelGGL(k_march_order_scan, dim3(1), dim3(1024), 0, stream, o.bin_count, n_bins);
  hipLaunchKernelGGL(k_march_order_scatter, dim3(cdiv(n_groups, 256)), dim3(256), 0, stream, n_groups, (const uint32_t*)o.estimate,
                     o.bin_count, o.order, o.order_steps);
}

// detmath.h element-wise (atmrt_math_probe): the GPU's instruction sequences against the host's on arbitrary operands
__global__ void k_math_probe(int op, size_t n, const double* __restrict__ a, const double* __restrict__ b,
                             double* __restrict__ out0, double* __restrict__ out1) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x = a[i], y = b ? b[i] : 0.0;
  double r0 = 0.0, r1 = 0.0;
  switch (op) {
    case ATMRT_PROBE_DIV: r0 = dm_div(x, y); break;
    case ATMRT_PROBE_DIV_R: r0 = dm_div_r(x, y, 1.0 / y); break;
    case ATMRT_PROBE_SQRT_INRANGE: r0 = dm_sqrt_inrange(x); break;
    case ATMRT_PROBE_EXP: r0 = dm_exp(x); break;
    case ATMRT_PROBE_LOG: r0 = dm_log(x); break;
    case ATMRT_PROBE_POW: r0 = dm_pow(x, y); break;
    case ATMRT_PROBE_SINCOS: dm_sincos(x, &r0, &r1); break;
    case ATMRT_PROBE_ASIN: r0 = dm_asin(x); break;
    case ATMRT_PROBE_ATAN2: r0 = dm_atan2(x, y); break;
    case ATMRT_PROBE_IEEE_DIV: r0 = x / y; break;
    case ATMRT_PROBE_IEEE_SQRT: r0 = dm_sqrt(x); break;
    case ATMRT_PROBE_ATAN: r0 = dm_atan(x); break;
    case ATMRT_PROBE_TAN: r0 = dm_tan(x); break;
    case ATMRT_PROBE_POW3: { // the three-point form the stepping kernels use (wave votes on the range guards)
      double p1, p2;
      pow3(x, x * 0.99999981, x * 1.00000019, y, r0, p1, p2);
      r1 = p1 + p2;
      break;
    }
    case ATMRT_PROBE_DIV3: {
      double q0;
      dm_div3(x, y, x, y * 0.99999976158142090, x, y * 1.00000047683715820, &q0, &r0, &r1);
      break;
    }
    case ATMRT_PROBE_DIV3_SEEDED: {
      double q0;
      dm_div3_seeded(x, y, x, y * 0.99999976158142090, x, y * 1.00000023841857910, 0, 0.0, &q0, &r0, &r1);
      break;
    }
    case ATMRT_PROBE_DIV3_SEED_Z: {
      double q1;
      dm_div3_seeded(x, y, x, y * 0.99999976158142090, x, y * 1.00000023841857910, 1, 2.0 - y, &r0, &q1, &r1);
      break;
    }
    case ATMRT_PROBE_DIV_SEED_N: r0 = dm_div_seeded(x, 1.0 + y, 1.0 - y); break;
    case ATMRT_PROBE_POW3_SHARED: { // as refr_n_layer3 calls it on a tight segment (the threshold atm_certify stores)
      double p1, p2;
      pow3_tight(x, x * 0.99999976158142090, x * 1.00000023841857910, y, atm_exp_thr(y, false), r0, p1, p2);
      r1 = p1 + p2;
      break;
    }
    default: break;
  }
  out0[i] = r0;
  if (out1) out1[i] = r1;
}
void launch_math_probe(int op, size_t n, const double* a, const double* b, double* out0, double* out1, hipStream_t stream) {
  if (n) hipLaunchKernelGGL(k_math_probe, dim3(cdiv(n, 256)), dim3(256), 0, stream, op, n, a, b, out0, out1);
}
// the three-point forms with every operand the caller's (atmrt_math_probe3): the three results apart, and which form the lane's
// wavefront took.  Same launch shape as k_math_probe: elements 64 w .. 64 w + 63 are one wavefront.
__global__ void k_math_probe3(int op, size_t n, const double* __restrict__ a, const double* __restrict__ b0, const double* __restrict__ b1,
                              const double* __restrict__ b2, double* __restrict__ out0, double* __restrict__ out1, double* __restrict__ out2,
                              int32_t* __restrict__ took) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x = a[i], y0 = b0[i], y1 = b1[i], y2 = b2[i];
  double r0 = 0.0, r1 = 0.0, r2 = 0.0;
  int tk = 0;
  switch (op) {
    case ATMRT_PROBE3_DIV3: tk = dm_div3(x, y0, x, y1, x, y2, &r0, &r1, &r2); break;
    case ATMRT_PROBE3_DIV3_SEEDED:
      dm_div3_seeded(x, y0, x, y1, x, y2, 0, 0.0, &r0, &r1, &r2);
      tk = 1;
      break;
    case ATMRT_PROBE3_DIV3_SEED_Z:
      dm_div3_seeded(x, y0, x, y1, x, y2, 1, 2.0 - y0, &r0, &r1, &r2);
      tk = 1;
      break;
    case ATMRT_PROBE3_POW3_TIGHT: pow3_tight<true>(y0, y1, y2, x, atm_exp_thr(x, false), r0, r1, r2, &tk); break;
    case ATMRT_PROBE3_EXP3_TIGHT: exp3_tight<true>(x * y0, x * y1, x * y2, atm_exp_thr(x, true), r0, r1, r2, &tk); break; // expo1 * d_i, as refr_n_layer3
    default: break;
  }
  out0[i] = r0;
  out1[i] = r1;
  out2[i] = r2;
  took[i] = tk;
}
void launch_math_probe3(int op, size_t n, const double* a, const double* b0, const double* b1, const double* b2, double* out0, double* out1,
                        double* out2, int32_t* took, hipStream_t stream) {
  if (n) hipLaunchKernelGGL(k_math_probe3, dim3(cdiv(n, 256)), dim3(256), 0, stream, op, n, a, b0, b1, b2, out0, out1, out2, took);
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------

void launch_resolve(const Frame& f, Workspace& ws, ObjectDev* objects_mut, hipStream_t stream) {
  hipLaunchKernelGGL(k_resolve, dim3(cdiv((size_t)f.n_objects + 1, 64)), dim3(64), 0, stream, f, ws.alt, objects_mut);
}

constexpr int FAST_RR = 8;

void launch_fast_caches(const Frame& f, Workspace& ws, hipStream_t stream, hipStream_t stream2, hipEvent_t ev,
                        hipEvent_t ev_join, hipEvent_t* timing) {
  // phase B (few long sequential rays) runs beside phase A (many short samples) on a second stream
  (void)hipEventRecord(ev, stream);
  (void)hipStreamWaitEvent(stream2, ev, 0);
  (void)hipEventRecord(timing[EV_PATHS_BEGIN], stream2);
  launch_fast_paths(f, ws, stream2, 1, f.n_path_cap);
  (void)hipEventRecord(timing[EV_PATHS_END], stream2);
  (void)hipEventRecord(ev_join, stream2);
  (void)hipEventRecord(timing[EV_PROFILE_BEGIN], stream);
  hipLaunchKernelGGL(k_fast_columns, dim3(cdiv(f.wl, 256)), dim3(256), 0, stream, f, ws.colcalc);
  if (f.n_objects) {
    ATMRT_DISPATCH_CALC(f.earth.calc, hipLaunchKernelGGL((k_terrain_profile<CALC, true>),
                                                          dim3(cdiv(f.n_t, PROFILE_SAMPLES_PER_BLOCK), cdiv(f.wl, 64)),
                                                          dim3(256), 0, stream, f, ws.colcalc, ws.prof, ws.plat, ws.plon));
  } else {
    ATMRT_DISPATCH_CALC(f.earth.calc, hipLaunchKernelGGL((k_terrain_profile<CALC, false>),
                                                          dim3(cdiv(f.n_t, PROFILE_SAMPLES_PER_BLOCK), cdiv(f.wl, 64)),
                                                          dim3(256), 0, stream, f, ws.colcalc, ws.prof, ws.plat, ws.plon));
  }
  (void)hipEventRecord(timing[EV_PROFILE_END], stream);
  (void)hipStreamWaitEvent(stream, ev_join, 0);
}

static void launch_fast_intersect_segment(const Frame& f, Workspace& ws, const DensePlanes& out, hipStream_t stream, int i_begin,
                                          int i_end, int last) {
  dim3 grid(cdiv(f.wl, 64), cdiv(f.h, 4 * FAST_RR));
  if (f.opaque)
    hipLaunchKernelGGL((k_fast_intersect<FAST_RR, 0>), grid, dim3(256), 0, stream, f, ws.prof, ws.pelev, ws.npath,
                       ws.hit_step, out.hit_count, ws.px_steps, (unsigned long long*)ws.counters, ws.dprev, i_begin, i_end, last,
                       (uint32_t*)nullptr, (uint32_t*)nullptr, (const uint8_t*)nullptr);
  else
    hipLaunchKernelGGL((k_fast_intersect<FAST_RR, 1>), grid, dim3(256), 0, stream, f, ws.prof, ws.pelev, ws.npath,
                       ws.hit_step, out.hit_count, ws.px_steps, (unsigned long long*)ws.counters, ws.dprev, i_begin, i_end, last,
                       ws.slot_step, (uint32_t*)nullptr, (const uint8_t*)nullptr);
}

void launch_fast_intersect(const Frame& f, Workspace& ws, const DensePlanes& out, hipStream_t stream) {
  launch_fast_intersect_segment(f, ws, out, stream, 1, f.n_path_cap, 1);
}

// Phases A, B and C of a Fast frame without scene objects.  The ray paths are one long dependent chain per row (3.5 ms at the
// headline size on a tenth of the chip) and the intersect scan only ever needs the samples integrated so far: the paths are
// integrated in FAST_SEGMENTS pieces on the second stream and the scan of piece k (main stream, after the terrain profile)
// waits for piece k alone, so it overlaps the integration of piece k + 1.  timing[EV_MARCH_BEGIN] is recorded before the first scan.
int launch_fast_pipeline(const Frame& f, Workspace& ws, const DensePlanes& out, hipStream_t stream, hipStream_t stream2,
                         hipEvent_t ev_fork, hipEvent_t* ev_seg, hipEvent_t* ev_scan, hipEvent_t* timing) {
  const int cap = f.n_path_cap;
  const int nseg = cap >= 256 ? FAST_SEGMENTS : 1;
  int per = (cap - 1 + nseg - 1) / nseg;
  per = (per + 3) / 4 * 4; // whole chunks of the scan
  (void)hipEventRecord(ev_fork, stream);
  (void)hipStreamWaitEvent(stream2, ev_fork, 0);
  (void)hipEventRecord(timing[EV_PATHS_BEGIN], stream2);
  for (int k = 0; k < nseg; k++) {
    const int b0 = 1 + k * per, b1 = k == nseg - 1 ? cap : (b0 + per < cap ? b0 + per : cap);
    launch_fast_paths(f, ws, stream2, b0, b1);
    (void)hipEventRecord(ev_seg[k], stream2);
  }
  (void)hipEventRecord(timing[EV_PATHS_END], stream2);
  (void)hipEventRecord(timing[EV_PROFILE_BEGIN], stream);
  hipLaunchKernelGGL(k_fast_columns, dim3(cdiv(f.wl, 256)), dim3(256), 0, stream, f, ws.colcalc);
  ATMRT_DISPATCH_CALC(f.earth.calc, hipLaunchKernelGGL((k_terrain_profile<CALC, false>),
                                                        dim3(cdiv(f.n_t, PROFILE_SAMPLES_PER_BLOCK), cdiv(f.wl, 64)), dim3(256), 0,
                                                        stream, f, ws.colcalc, ws.prof, ws.plat, ws.plon));
  (void)hipEventRecord(timing[EV_PROFILE_END], stream);
  (void)hipEventRecord(timing[EV_MARCH_BEGIN], stream);
  for (int k = 0; k < nseg; k++) {
    const int b0 = 1 + k * per, b1 = k == nseg - 1 ? cap : (b0 + per < cap ? b0 + per : cap);
    (void)hipStreamWaitEvent(stream, ev_seg[k], 0);
    (void)hipEventRecord(ev_scan[2 * k], stream); // stamped once the wait is over
    launch_fast_intersect_segment(f, ws, out, stream, b0, b1, k == nseg - 1 ? 1 : 0);
    (void)hipEventRecord(ev_scan[2 * k + 1], stream);
  }
  return nseg;
}

void launch_fast_finalize(const Frame& f, Workspace& ws, const DensePlanes& out, hipStream_t stream) {
  ATMRT_DISPATCH_CALC(f.earth.calc, hipLaunchKernelGGL((k_fast_finalize<CALC>), dim3(cdiv(f.wl, 256), f.h), dim3(256), 0,
                                                        stream, f, ws.colcalc, ws.prof, ws.pelev, ws.plen, ws.hit_step, out));
}

void launch_scan_u32(const uint32_t* in, size_t n, uint64_t* tmp, uint64_t* out, unsigned long long* total,
                     hipStream_t stream) {
  unsigned nb = cdiv(n, 256 * SCAN_ITEMS);
  hipLaunchKernelGGL(k_scan_block_sums, dim3(nb), dim3(256), 0, stream, in, n, tmp);
  hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(256), 0, stream, tmp, (size_t)nb, total);
  hipLaunchKernelGGL(k_scan_apply, dim3(nb), dim3(256), 0, stream, in, n, tmp, out);
}

void launch_scan_counts(const Frame& f, Workspace& ws, const uint32_t* hit_count, hipStream_t stream) {
  launch_scan_u32(hit_count, (size_t)f.wl * f.h, ws.scan_tmp, ws.hit_offset, (unsigned long long*)&ws.counters[CTR_HITS], stream);
}

void launch_close_count(const Frame& f, Workspace& ws, hipStream_t stream) {
  size_t n = (size_t)f.n_t * f.wl;
  ATMRT_DISPATCH_CALC(f.earth.calc, hipLaunchKernelGGL((k_column_candidates<CALC>), dim3(cdiv(f.wl, 64)), dim3(64), 0, stream, f,
                                                        ws.colcalc, ws.col_cand, ws.col_ncand, ws.col_lo, ws.col_hi,
                                                        (unsigned long long*)ws.counters));
  hipLaunchKernelGGL((k_close_objects<false>), dim3(cdiv(n, 256)), dim3(256), 0, stream, f, ws.plat, ws.plon, ws.col_cand,
                     ws.col_ncand, ws.ccount, (const uint64_t*)nullptr, (uint32_t*)nullptr);
  launch_scan_u32(ws.ccount, n, ws.scan_tmp, ws.coffset, (unsigned long long*)&ws.counters[CTR_CLOSE_TOTAL], stream);
}

void launch_close_fill(const Frame& f, Workspace& ws, hipStream_t stream) {
  size_t n = (size_t)f.n_t * f.wl;
  hipLaunchKernelGGL((k_close_objects<true>), dim3(cdiv(n, 256)), dim3(256), 0, stream, f, ws.plat, ws.plon, ws.col_cand,
                     ws.col_ncand, ws.ccount, ws.coffset, ws.clist);
}

void launch_pack_first_hits(const Frame& f, Workspace& ws, const DensePlanes& dense, const PackedHits& packed,
                            hipStream_t stream) {
  size_t n = (size_t)f.wl * f.h;
  hipLaunchKernelGGL(k_pack_first_hits, dim3(cdiv(n, 256)), dim3(256), 0, stream, f, ws.hit_offset, dense, packed);
}

void launch_trace_count(const Frame& f, Workspace& ws, const DensePlanes& out, hipStream_t stream) {
  hipLaunchKernelGGL(k_paths_transpose, dim3(f.n_path_cap, cdiv(f.h, 256)), dim3(256), 0, stream, f, ws.pelev, ws.plen, ws.npath,
                     ws.pelev_t, ws.plen_t);
  // Counting pass in three parts: (1) mark the pixels that can have a step with an object (k_fast_flag_rows); (2) the plain
  // intersect scan over every pixel — terrain crossings only, at 6 instructions per ray-step — into the tracer's slot arena;
  // (3) the general tracer (one column per wavefront, sequential over the samples) only over the marked rows, overwriting what
  // the scan left for them.  Config 5: k_fast_trace<false> 14.2 -> 2.3 ms (+ 3.1 ms of scan, 0.3 ms of marking); frame 22.4 -> 15.2 ms.
  hipLaunchKernelGGL(k_fast_flag_rows, dim3(f.wl, cdiv(f.h, 256)), dim3(256), 0, stream, f, ws.col_cand, ws.col_ncand, ws.col_lo, ws.col_hi,
                     ws.pelev_t, ws.npath, ws.traced);
  {
    dim3 grid(cdiv(f.wl, 64), cdiv(f.h, 4 * FAST_RR));
    if (f.p.terrain_alpha == 1.0)
      hipLaunchKernelGGL((k_fast_intersect<FAST_RR, 0>), grid, dim3(256), 0, stream, f, ws.prof, ws.pelev, ws.npath, ws.hit_step,
                         out.hit_count, ws.px_steps, (unsigned long long*)ws.counters, ws.dprev, 1, f.n_path_cap, 1, ws.slot_step,
                         ws.slot_packed.color_tag, (const uint8_t*)ws.traced);
    else
      hipLaunchKernelGGL((k_fast_intersect<FAST_RR, 1>), grid, dim3(256), 0, stream, f, ws.prof, ws.pelev, ws.npath, ws.hit_step,
                         out.hit_count, ws.px_steps, (unsigned long long*)ws.counters, ws.dprev, 1, f.n_path_cap, 1, ws.slot_step,
                         ws.slot_packed.color_tag, (const uint8_t*)ws.traced);
  }
  hipLaunchKernelGGL((k_fast_trace<false>), dim3(cdiv(f.wl, 4), cdiv(f.h, 64)), dim3(256), 0, stream, f, ws.prof, ws.plat, ws.plon,
                     ws.ccount, ws.coffset, ws.clist, ws.pelev_t, ws.plen_t, ws.npath, out.hit_count, (const uint64_t*)nullptr,
                     ws.slot_packed, ws.slot_step, ws.slot_pixel, ws.px_steps, (unsigned long long*)ws.counters, (double*)nullptr,
                     (const uint8_t*)ws.traced);
}

template <SlotLayout LAYOUT, bool REC, bool POINTS, Beyond BEYOND>
static void launch_gather_slots(size_t n, const uint32_t* hit_count, const Workspace& ws, const RectRec& slot_rec, const RectRec& rec,
                                const PackedHits& packed, hipStream_t stream) {
  hipLaunchKernelGGL((k_gather_slots<LAYOUT, REC, POINTS, BEYOND>), dim3(cdiv(n, 256)), dim3(256), 0, stream, n, hit_count, ws.hit_offset,
                     ws.slot_step, slot_rec, ws.slot_packed, ws.list_step, ws.list_pixel, rec, packed, ws.overflow,
                     (unsigned long long*)ws.counters);
}

// A frame that can have several trace points per pixel (translucent terrain, scenes with objects), after the scan of hit_count:
// what the counting pass recorded goes to the pixel-ordered list (k_gather_slots, k_scatter_overflow), a second pass lists the
// pixels that recording did not cover, one thread per trace point completes the terrain points, and the dense planes get the
// first point of every pixel.  The route — generator, objects or not — picks the template arguments and the second pass only.
void launch_list_fill(const Frame& f, Workspace& ws, uint64_t n_hits, const DensePlanes& dense, const PackedHits& packed,
                      hipStream_t stream) {
  constexpr SlotLayout SM = SlotLayout::SlotMajor, PM = SlotLayout::PixelMajor;
  const bool rect = f.p.generator == ATMRT_GEN_RECTILINEAR, objects = f.n_objects > 0;
  const size_t n = (size_t)f.wl * f.h;
  const RectRec rec = rect ? carve_rec(ws.rect_rec, (size_t)n_hits) : RectRec{};
  const RectRec slot_rec = rect ? carve_rec(ws.slot_rec, n * RECT_SLOTS) : RectRec{};
  // Rectilinear, the points beyond the slots: out of the overflow arena when all of them fitted it — and, with objects, no step had
  // more points than the in-register step list (those are sorted in HBM by the fill pass).  Otherwise those pixels are visited a
  // second time: a launch of one wavefront per SIMD at the speed of its dependency chain (headline at terrain_alpha 0.5: 12.8 ms
  // for 0.7 % of the pixels, at any frame or tile size; config 5: 22.7 ms for 1.3 %).
  const bool arena = rect && ws.overflow_arena && ws.overflow_cap && ws.n_overflow_records <= ws.overflow_cap && !(objects && ws.step_prop);
  const uint32_t* hit_count = dense.hit_count;
  if (!rect && !objects) launch_gather_slots<SM, false, false, Beyond::Skip>(n, hit_count, ws, slot_rec, rec, packed, stream);
  else if (!rect) launch_gather_slots<PM, false, true, Beyond::Skip>(n, hit_count, ws, slot_rec, rec, packed, stream);
  else if (!objects && arena) launch_gather_slots<SM, true, false, Beyond::Clamp>(n, hit_count, ws, slot_rec, rec, packed, stream);
  else if (!objects) launch_gather_slots<SM, true, false, Beyond::List>(n, hit_count, ws, slot_rec, rec, packed, stream);
  else if (arena) launch_gather_slots<PM, true, true, Beyond::Clamp>(n, hit_count, ws, slot_rec, rec, packed, stream);
  else launch_gather_slots<PM, true, true, Beyond::List>(n, hit_count, ws, slot_rec, rec, packed, stream);
  if (arena) {
    const uint32_t n_records = (uint32_t)ws.n_overflow_records;
    const OverflowArena ovf = carve_overflow(ws.overflow_arena, ws.overflow_cap);
    if (n_records && objects)
      hipLaunchKernelGGL((k_scatter_overflow<true>), dim3(cdiv((size_t)n_records, 256)), dim3(256), 0, stream, n_records, ovf,
                         ws.overflow_packed, (const int32_t*)ws.hit_step, ws.hit_offset, ws.list_step, ws.list_pixel, rec, packed);
    else if (n_records)
      hipLaunchKernelGGL((k_scatter_overflow<false>), dim3(cdiv((size_t)n_records, 256)), dim3(256), 0, stream, n_records, ovf,
                         PackedHits{}, (const int32_t*)nullptr, ws.hit_offset, ws.list_step, ws.list_pixel, rec, packed);
  } else if (rect) {
    if (ws.n_overflow) launch_rect_second_pass(f, ws, n_hits, dense, packed, stream);
  } else if (objects) {
    hipLaunchKernelGGL((k_fast_trace<true>), dim3(cdiv(f.wl, 4), cdiv(f.h, 64)), dim3(256), 0, stream, f, ws.prof, ws.plat, ws.plon,
                       ws.ccount, ws.coffset, ws.clist, ws.pelev_t, ws.plen_t, ws.npath, dense.hit_count, ws.hit_offset, packed,
                       ws.list_step, ws.list_pixel, (uint32_t*)nullptr, (unsigned long long*)ws.counters, ws.step_prop,
                       (const uint8_t*)nullptr);
  } else {
    hipLaunchKernelGGL(k_fast_list, dim3(cdiv(f.wl, 256), f.h), dim3(256), 0, stream, f, ws.prof, ws.pelev, ws.npath,
                       ws.hit_offset, (const uint32_t*)dense.hit_count, ws.list_step, ws.list_pixel);
  }
  if (n_hits && rect) {
    launch_rect_finalize_list(f, ws, n_hits, packed, stream);
  } else if (n_hits) {
    ATMRT_DISPATCH_CALC(f.earth.calc, hipLaunchKernelGGL((k_fast_finalize_list<CALC>), dim3(cdiv(n_hits, 256)), dim3(256), 0,
                                                          stream, f, n_hits, ws.colcalc, ws.prof, ws.pelev, ws.plen,
                                                          ws.list_step, ws.list_pixel, packed));
  }
  launch_dense_from_packed(f, ws, packed, dense, rect ? 0 : 1, stream);
}

void launch_dense_from_packed(const Frame& f, Workspace& ws, const PackedHits& packed, const DensePlanes& dense, int fast_angles,
                              hipStream_t stream) {
  hipLaunchKernelGGL(k_dense_from_packed, dim3(cdiv(f.wl, 256), f.h), dim3(256), 0, stream, f, ws.hit_offset, packed, dense,
                     fast_angles);
}

void launch_get_elev(const Frame& f, size_t n, const double* lat, const double* lon, double* elev, uint8_t* valid,
                     hipStream_t stream) {
  if (n) hipLaunchKernelGGL(k_get_elev, dim3(cdiv(n, 256)), dim3(256), 0, stream, f, n, lat, lon, elev, valid);
}
void launch_ray_paths(const Frame& f, double h0, size_t n_angles, const double* angles_deg, int straight, double step,
                      size_t n_steps, double* x, double* h, hipStream_t stream) {
  if (n_angles)
    hipLaunchKernelGGL(k_ray_paths, dim3(cdiv(n_angles, 64)), dim3(64), 0, stream, f, h0, n_angles, angles_deg,
                       straight, step, n_steps, x, h);
}
void launch_atm_sample(const Frame& f, size_t n, const double* alt, double* t, double* p, double* nidx, double* dn,
                       hipStream_t stream) {
  if (n) hipLaunchKernelGGL(k_atm_sample, dim3(cdiv(n, 256)), dim3(256), 0, stream, f, n, alt, t, p, nidx, dn);
}
void launch_coords_at_dist(const Frame& f, double lat0, double lon0, double dir, size_t n, const double* dist,
                           double* lat, double* lon, hipStream_t stream) {
  if (n)
    hipLaunchKernelGGL(k_coords_at_dist, dim3(cdiv(n, 256)), dim3(256), 0, stream, f, lat0, lon0, dir, n, dist, lat, lon);
}

} // namespace atmrt
