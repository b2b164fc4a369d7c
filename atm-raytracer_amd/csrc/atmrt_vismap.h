// atmrt_vismap.h — kernels of the visibility map (include/atmrt.h, atmrt_visibility_map*): the frame's trace points scattered into
// a latitude / longitude grid, and the reduction that finds the frame's bounds.  Included by atmrt_kernels.hip only.
//
// The scatter is one pass over planes the frame left in HBM (24 B per point read, 12 B per update written), so what it costs is
// decided by its atomics: near the horizon thousands of neighbouring pixels fall into one cell, and one atomic per lane queues
// them all on one address.  Pixels are taken row-major, one per lane, so a wavefront is 64 consecutive pixels of an image row
// and its equal cells come in runs: a run makes ONE update (its point count, its smallest distance) from its first lane.
//
// Every update is an integer atomic at agent scope — a u32 add, and a u64 min on the bit pattern of the distance (non-negative
// doubles order like their bit patterns) — so the map does not depend on the order the wavefronts arrive in: bit-reproducible.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atmrt_core.h"
#include "atmrt_kernels.h"

namespace atmrt {

// The device block of one call (VIS_N u64): the statistics, then the bounds as order-preserving keys.
enum VisSlot : int {
  VIS_POINTS = 0,
  VIS_BINNED = 1,
  VIS_OUTSIDE = 2,
  VIS_SKIPPED = 3,
  VIS_UPDATES = 4,
  VIS_LAT_MIN = 5,
  VIS_LAT_MAX = 6,
  VIS_LON_MIN = 7,
  VIS_LON_MAX = 8,
};
constexpr int VIS_N = 9;
constexpr unsigned long long VIS_INF_BITS = 0x7ff0000000000000ull; // +inf: above the bit pattern of every finite distance

// u64 keys that order like the doubles they come from (negative: all bits flipped, else the sign bit set)
__device__ inline unsigned long long vis_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}

__global__ __launch_bounds__(64) void k_vis_reset(unsigned long long* __restrict__ ctr) {
  const int i = threadIdx.x;
  if (i < VIS_N) ctr[i] = (i == VIS_LAT_MIN || i == VIS_LON_MIN) ? ~0ull : 0ull;
}

// count = 0, min_distance = +inf (min_distance may be null)
__global__ __launch_bounds__(256) void k_vis_clear(size_t n_cells, uint32_t* __restrict__ count, unsigned long long* __restrict__ mind) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_cells) return;
  count[i] = 0u;
  if (mind) mind[i] = VIS_INF_BITS;
}

// The traversal every consumer of a frame's trace points (TracePoints, atmrt_kernels.h) shares: thread p is pixel p, row-major as
// in k_draw_image, and holds `cnt` points, entries k0 .. k0 + cnt - 1 of s.lat / lon / dist.  PACKED: the pixel's entries of the
// lists; else its one entry of the planes, present when hit_count[p] != 0.  A thread past the last pixel gets no point (and entry
// 0) rather than leaving: the callers' ballots, shuffles and __any need all 64 lanes.
struct VisSpan {
  uint32_t cnt;
  size_t k0;
};
template <bool PACKED>
__device__ inline VisSpan vis_span(const TracePoints& s, size_t p) {
  const bool in = p < s.n_pixels;
  uint32_t cnt = in ? s.hit_count[p] : 0u;
  if (!PACKED && cnt > 1u) cnt = 1u;
  return VisSpan{cnt, PACKED ? (in ? (size_t)s.hit_offset[p] : 0) : p};
}

// One trace point of a lane: is there one in this trip, and is it one the map looks up (none of lat, lon, distance NaN, distance
// not negative)?
struct VisPoint {
  double lat, lon, dist;
  bool active, valid;
};
__device__ inline VisPoint vis_point(bool active, size_t k, const double* __restrict__ lat, const double* __restrict__ lon,
                                     const double* __restrict__ dist) {
  VisPoint v{0.0, 0.0, 0.0, active, false};
  if (active) {
    v.lat = lat[k], v.lon = lon[k], v.dist = dist[k];
    v.valid = v.lat == v.lat && v.lon == v.lon && v.dist >= 0.0; // NaN fails each of them; -0.0 >= 0.0 holds
  }
  return v;
}

// The scatter: thread p = blockIdx.x * blockDim.x + threadIdx.x is pixel p, as in k_draw_image; no lane leaves early, the loop's
// trip count is the wavefront's largest point count and every cross-lane operation sees all 64 lanes.  Trip q: the lanes with
// more than q points take part.
// AGG: a maximal run of consecutive lanes that hold the same cell in this trip updates once.  `heads` marks the lanes whose lower
// neighbour holds another cell (or none: a lane without a binned point ends a run); a run reaches from its head to the lane
// before the next head or the next lane without a cell, so its point count is a distance between two bits of those masks, and
// only the smallest distance needs the log-step combine: after step d a lane holds the minimum over itself and the next 2d - 1
// lanes of its run.  A wavefront whose runs are all one lane long (a fine grid) skips the combine.
template <bool PACKED, bool AGG>
__global__ __launch_bounds__(256) void k_vis_scatter(TracePoints s, atmrt_geo_grid_t g, uint32_t* __restrict__ count,
                                                     unsigned long long* __restrict__ mind, unsigned long long* __restrict__ ctr) {
  const int lane = threadIdx.x & 63;
  const VisSpan span = vis_span<PACKED>(s, (size_t)blockIdx.x * blockDim.x + threadIdx.x);
  const uint32_t cnt = span.cnt;
  const size_t k0 = span.k0;
  const double *__restrict__ lat = s.lat, *__restrict__ lon = s.lon, *__restrict__ dist = s.dist;
  unsigned long long n_points = 0, n_binned = 0, n_skipped = 0, n_updates = 0; // wave-uniform
  for (uint32_t q = 0; __any(q < cnt); q++) {
    const VisPoint v = vis_point(q < cnt, k0 + q, lat, lon, dist);
    const int64_t cell = v.valid ? geo_grid_cell(g, v.lat, v.lon) : -1;
    const unsigned long long active = __ballot(v.active), looked_up = __ballot(v.valid), held = __ballot(cell >= 0);
    n_points += __popcll(active), n_skipped += __popcll(active & ~looked_up), n_binned += __popcll(held);
    unsigned long long bits = (unsigned long long)__double_as_longlong(v.dist) & 0x7fffffffffffffffull; // -0.0 counts as 0.0
    if (!AGG) {
      if (cell >= 0) {
        atomicAdd(&count[cell], 1u);
        if (mind) atomicMin(&mind[cell], bits);
      }
      n_updates += __popcll(held);
      continue;
    }
    const long long below = __shfl_up((long long)cell, 1);
    const bool head = cell >= 0 && (lane == 0 || below != cell);
    const unsigned long long heads = __ballot(head);
    // the first lane above this one that starts another run or holds no cell: one past the end of this lane's run
    const unsigned long long above = (heads | ~held) & (lane == 63 ? 0ull : ~0ull << (lane + 1));
    const int end = above ? __ffsll((long long)above) - 1 : 64;
    if (heads != held) {
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long other = __shfl_down(bits, d);
        if (lane + d < end && other < bits) bits = other;
      }
    }
    if (head) {
      atomicAdd(&count[cell], (uint32_t)(end - lane));
      if (mind) atomicMin(&mind[cell], bits);
    }
    n_updates += __popcll(heads);
  }
  if (lane == 0 && n_points) {
    atomicAdd(&ctr[VIS_POINTS], n_points);
    if (n_binned) atomicAdd(&ctr[VIS_BINNED], n_binned);
    if (n_points - n_binned - n_skipped) atomicAdd(&ctr[VIS_OUTSIDE], n_points - n_binned - n_skipped);
    if (n_skipped) atomicAdd(&ctr[VIS_SKIPPED], n_skipped);
    if (n_updates) atomicAdd(&ctr[VIS_UPDATES], n_updates);
  }
}

// The frame's bounds over the points the scatter would look up: each lane keeps the extremes of its pixel's points as keys, the
// wavefront combines them by butterfly, and one lane issues the four atomics (a wavefront without such a point issues none).
template <bool PACKED>
__global__ __launch_bounds__(256) void k_vis_bounds(TracePoints s, unsigned long long* __restrict__ ctr) {
  const int lane = threadIdx.x & 63;
  const VisSpan span = vis_span<PACKED>(s, (size_t)blockIdx.x * blockDim.x + threadIdx.x);
  const uint32_t cnt = span.cnt;
  const size_t k0 = span.k0;
  const double *__restrict__ lat = s.lat, *__restrict__ lon = s.lon, *__restrict__ dist = s.dist;
  unsigned long long lat_min = ~0ull, lat_max = 0ull, lon_min = ~0ull, lon_max = 0ull;
  for (uint32_t q = 0; q < cnt; q++) {
    const VisPoint v = vis_point(true, k0 + q, lat, lon, dist);
    if (!v.valid) continue;
    const unsigned long long ka = vis_key(v.lat), ko = vis_key(v.lon);
    lat_min = ka < lat_min ? ka : lat_min, lat_max = ka > lat_max ? ka : lat_max;
    lon_min = ko < lon_min ? ko : lon_min, lon_max = ko > lon_max ? ko : lon_max;
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long a = __shfl_xor(lat_min, d), b = __shfl_xor(lat_max, d), c = __shfl_xor(lon_min, d), e = __shfl_xor(lon_max, d);
    lat_min = a < lat_min ? a : lat_min, lat_max = b > lat_max ? b : lat_max;
    lon_min = c < lon_min ? c : lon_min, lon_max = e > lon_max ? e : lon_max;
  }
  if (lane == 0 && lat_max != 0ull) {
    atomicMin(&ctr[VIS_LAT_MIN], lat_min), atomicMax(&ctr[VIS_LAT_MAX], lat_max);
    atomicMin(&ctr[VIS_LON_MIN], lon_min), atomicMax(&ctr[VIS_LON_MAX], lon_max);
  }
}

} // namespace atmrt
