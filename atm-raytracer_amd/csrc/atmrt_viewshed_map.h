// atmrt_viewshed_map.h — the viewshed map (include/atmrt.h, "viewshed map": the rule is stated there): the samples of a viewshed —
// lattice cell (j, i) with its status, hidden, lat and lon — scattered into a latitude / longitude grid.  The launch interface for
// atmrt_polar.hip; the kernels are compiled by atmrt_viewshed.hip only (ATMRT_VIEWSHED_KERNELS).
//
//   k_vsmap_clear    n_samples = n_seen = 0, min_hidden = +inf.
//   k_vsmap_scatter  one sample per lane, in the planes' own order [j * m + (i - 1)]: a wavefront is 64 consecutive steps of one
//                    azimuth (or the end of one and the start of the next) and its four loads are coalesced.  No lane leaves before
//                    the ballots; the call's statistics are counted per wavefront and added once per wavefront.
//
// Every update is an integer atomic at agent scope — u32 adds, and a u64 min on the bit pattern of `hidden` (doubles without the sign
// bit order like their bit patterns, +0.0 below 5e-324 below +inf) — so the map does not depend on the order in which wavefronts
// arrive, nor on how a call was batched: bit-reproducible.  Every lane updates for itself: near the observer many steps of one
// azimuth share a cell, at 1-arcsecond cells and 100 m steps almost none do, and whether merging runs (as k_vis_scatter does) pays
// here has not been measured.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atmrt_core.h"

namespace atmrt {

// The device block of one call (VSMAP_N u64), in the order of atmrt_viewshed_map_stats_t.
enum VsMapSlot : int { VSMAP_SAMPLES = 0, VSMAP_BINNED = 1, VSMAP_OUTSIDE = 2, VSMAP_SKIPPED = 3, VSMAP_SEEN = 4 };
constexpr int VSMAP_N = 5;
constexpr unsigned long long VSMAP_INF_BITS = 0x7ff0000000000000ull; // +inf: not below the bit pattern of any hidden that takes part
constexpr size_t VSMAP_SAMPLES_MAX = (size_t)0x7fffffff * 256;        // one lane per sample, 256 lanes per block, 2^31 - 1 blocks

struct VsMapSamples { // n entries each, device memory
  size_t n;
  const uint8_t* status;
  const double *hidden, *lat, *lon;
};
struct VsMapPlanes { // [n_lat][n_lon] each, device memory; min_hidden may be null
  uint32_t *n_samples, *n_seen;
  double* min_hidden;
};
void launch_vsmap_reset(void* block, hipStream_t stream);
void launch_vsmap_clear(const atmrt_geo_grid_t& grid, const VsMapPlanes& map, hipStream_t stream);
void launch_vsmap_scatter(const VsMapSamples& s, const atmrt_geo_grid_t& grid, const VsMapPlanes& map, void* block, hipStream_t stream);

} // namespace atmrt

#if defined(ATMRT_VIEWSHED_KERNELS)
#include "atmrt_device.h"

namespace atmrt {

__global__ __launch_bounds__(64) void k_vsmap_reset(unsigned long long* __restrict__ ctr) {
  if (threadIdx.x < VSMAP_N) ctr[threadIdx.x] = 0ull;
}

__global__ __launch_bounds__(256) void k_vsmap_clear(size_t n_cells, uint32_t* __restrict__ n_samples, uint32_t* __restrict__ n_seen,
                                                     unsigned long long* __restrict__ minh) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_cells) return;
  n_samples[i] = 0u, n_seen[i] = 0u;
  if (minh) minh[i] = VSMAP_INF_BITS;
}

// Thread p = blockIdx.x * blockDim.x + threadIdx.x is sample p; a thread past the last sample holds none and stays for the ballots.
__global__ __launch_bounds__(256) void k_vsmap_scatter(VsMapSamples s, atmrt_geo_grid_t g, uint32_t* __restrict__ n_samples,
                                                       uint32_t* __restrict__ n_seen, unsigned long long* __restrict__ minh,
                                                       unsigned long long* __restrict__ ctr) {
  const int lane = threadIdx.x & 63;
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = p < s.n;
  int status = 255;
  double hidden = 0.0, lat = 0.0, lon = 0.0;
  if (active) status = s.status[p], hidden = s.hidden[p], lat = s.lat[p], lon = s.lon[p];
  const bool looked_up = active && lat == lat && lon == lon && status <= 3; // the others are skipped
  const int64_t cell = looked_up ? geo_grid_cell(g, lat, lon) : -1;
  const bool seen = cell >= 0 && (status == ATMRT_SIGHT_SEEN || status == ATMRT_SIGHT_BELOW_FAN);
  if (cell >= 0) {
    atomicAdd(&n_samples[cell], 1u);
    if (seen) atomicAdd(&n_seen[cell], 1u);
    if (minh && (status == ATMRT_SIGHT_SEEN || status == ATMRT_SIGHT_HIDDEN)) {
      const unsigned long long bits = (unsigned long long)__double_as_longlong(hidden);
      if (hidden == hidden && !(bits >> 63)) atomicMin(&minh[cell], bits); // not NaN, sign bit clear (-0.0 does not take part)
    }
  }
  const unsigned long long n_active = __popcll(__ballot(active)), n_looked = __popcll(__ballot(looked_up));
  const unsigned long long n_binned = __popcll(__ballot(cell >= 0)), n_sees = __popcll(__ballot(seen));
  if (lane == 0 && n_active) {
    atomicAdd(&ctr[VSMAP_SAMPLES], n_active);
    if (n_binned) atomicAdd(&ctr[VSMAP_BINNED], n_binned);
    if (n_looked - n_binned) atomicAdd(&ctr[VSMAP_OUTSIDE], n_looked - n_binned);
    if (n_active - n_looked) atomicAdd(&ctr[VSMAP_SKIPPED], n_active - n_looked);
    if (n_sees) atomicAdd(&ctr[VSMAP_SEEN], n_sees);
  }
}

void launch_vsmap_reset(void* block, hipStream_t stream) {
  hipLaunchKernelGGL(k_vsmap_reset, dim3(1), dim3(64), 0, stream, static_cast<unsigned long long*>(block));
}
void launch_vsmap_clear(const atmrt_geo_grid_t& grid, const VsMapPlanes& map, hipStream_t stream) {
  const size_t n_cells = (size_t)grid.n_lat * grid.n_lon;
  hipLaunchKernelGGL(k_vsmap_clear, dim3(cdiv(n_cells, 256)), dim3(256), 0, stream, n_cells, map.n_samples, map.n_seen,
                     reinterpret_cast<unsigned long long*>(map.min_hidden));
}
void launch_vsmap_scatter(const VsMapSamples& s, const atmrt_geo_grid_t& grid, const VsMapPlanes& map, void* block, hipStream_t stream) {
  if (s.n == 0) return;
  hipLaunchKernelGGL(k_vsmap_scatter, dim3(cdiv(s.n, 256)), dim3(256), 0, stream, s, grid, map.n_samples, map.n_seen,
                     reinterpret_cast<unsigned long long*>(map.min_hidden), static_cast<unsigned long long*>(block));
}

} // namespace atmrt
#endif
