// atmrt_landmarks.h — kernels of the landmark search (include/atmrt.h, atmrt_locate_landmarks*): for every landmark the number of
// the frame's trace points within a radius and the nearest of them.  Included by atmrt_kernels.hip only.
//
// The host lays a bucket index over the landmarks (atmrt_consumers.hip, LandmarkIndex: an atmrt_geo_grid_t whose cells list, as CSR,
// the landmarks whose padded boxes overlap them), so a trace point looks up ONE cell with geo_grid_cell and evaluates the exact
// rule landmark_d2 (atmrt_core.h) on that cell's list only.  The traversal is vis_span and vis_point (atmrt_vismap.h), as in
// k_vis_scatter: one pixel per lane, row-major, a trip loop over the wavefront's largest point count.
//   pass A  within pairs: u32 add on the landmark's count, u64 min on the bit pattern of d2 (a sum of squares, never negative:
//           it orders like its bits)
//   pass B  the same traversal; a pair whose d2 bits equal the landmark's minimum: u64 min on the key p << 32 | point index
//   pass C  one thread per landmark decodes the key, fetches the winner's distance and elevation and writes the record
// Integer atomics at agent scope only, so the records do not depend on the order the wavefronts arrive in.  No run aggregation
// inside the wavefront (k_vis_scatter has one): whether it pays here is for tools/measure_landmarks.py to say first.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atmrt_core.h"
#include "atmrt_kernels.h"
#include "atmrt_vismap.h"

namespace atmrt {

__global__ __launch_bounds__(256) void k_lm_reset(size_t n, LmState st) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (size_t)LM_N) st.ctr[i] = 0ull;
  if (i >= n) return;
  st.count[i] = 0u;
  st.d2min[i] = ~0ull; // above the bits of every d2 that can be within (all ones is a NaN)
  st.key[i] = ~0ull;
}

template <bool PACKED, bool PASS_B>
__global__ __launch_bounds__(256) void k_lm_pass(TracePoints s, LmIndex ix, LmState st) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const VisSpan span = vis_span<PACKED>(s, p);
  const uint32_t cnt = span.cnt;
  const size_t k0 = span.k0;
  unsigned long long n_points = 0, n_skipped = 0; // wave-uniform
  unsigned long long n_tested = 0, n_within = 0;  // this lane's; summed over the wavefront once, below
  for (uint32_t q = 0; __any(q < cnt); q++) {
    const VisPoint v = vis_point(q < cnt, k0 + q, s.lat, s.lon, s.dist);
    if (!PASS_B) {
      const unsigned long long active = __ballot(v.active), looked_up = __ballot(v.valid);
      n_points += __popcll(active), n_skipped += __popcll(active & ~looked_up);
    }
    const int64_t cell = v.valid ? geo_grid_cell(ix.grid, v.lat, v.lon) : -1;
    if (cell >= 0) { // no lane leaves the trip early: the ballots and the loop's __any see all 64 lanes
      const uint32_t begin = ix.cell_start[cell], end = ix.cell_start[cell + 1];
      n_tested += end - begin;
      for (uint32_t k = begin; k < end; k++) {
        const uint32_t l = ix.items[k];
        const double d2 = landmark_d2(ix.lm[l], v.lat, v.lon);
        if (d2 <= ix.r2) { // a NaN is never within
          const unsigned long long bits = (unsigned long long)__double_as_longlong(d2);
          if (!PASS_B) {
            n_within++;
            atomicAdd(&st.count[l], 1u);
            atomicMin(&st.d2min[l], bits);
          } else if (bits == st.d2min[l]) {
            atomicMin(&st.key[l], (unsigned long long)p << 32 | q);
          }
        }
      }
    }
  }
  if (PASS_B) return;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) n_tested += __shfl_xor(n_tested, d), n_within += __shfl_xor(n_within, d);
  if (lane == 0 && n_points) {
    atomicAdd(&st.ctr[LM_POINTS], n_points);
    if (n_skipped) atomicAdd(&st.ctr[LM_SKIPPED], n_skipped);
    if (n_tested) atomicAdd(&st.ctr[LM_TESTED], n_tested);
    if (n_within) atomicAdd(&st.ctr[LM_WITHIN], n_within);
  }
}

__global__ __launch_bounds__(256) void k_lm_finish(size_t n, TracePoints s, LmState st, atmrt_landmark_hit_t* __restrict__ hits) {
  const size_t l = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= n) return;
  atmrt_landmark_hit_t h{0u, 0xffffffffu, 0xffffffffu, 0u, __builtin_inf(), __builtin_nan(""), __builtin_nan("")};
  const uint32_t cnt = st.count[l];
  const unsigned long long key = st.key[l];
  if (cnt && (key >> 32) < s.n_pixels) {
    const size_t p = (size_t)(key >> 32);
    const uint32_t q = (uint32_t)key;
    const size_t k = s.hit_offset ? (size_t)s.hit_offset[p] + q : p;
    h.n_within = cnt;
    h.x = (uint32_t)(p % s.width), h.y = (uint32_t)(p / s.width);
    h.point = q;
    h.d2 = __longlong_as_double((long long)st.d2min[l]);
    h.distance = s.dist[k], h.elevation = s.elev[k];
  }
  hits[l] = h;
}

} // namespace atmrt
