// atmrt_horizon.h — the horizon profile (include/atmrt.h, "horizon": the rule is stated there): per azimuth the bracket of elevation
// angles between the highest ray that terrain stops and the ray above it, and the ridge that stops it.  The launch interface for
// atmrt_polar.hip; the kernels themselves are compiled by atmrt_horizon.hip only (ATMRT_HORIZON_KERNELS).
//
//   (path table)      the viewshed's k_viewshed_paths and its Cached product: H[i][k], step-major
//   (profiles)        k_sight_calc / k_sight_profile through launch_sight_profile: every azimuth is a target whose m is the call's
//   k_horizon_scan    round one.  The viewshed scan's access pattern: one block per HORIZON_AZ azimuths, a lane owns ray k (R rays
//                     where K > 64 x the block's wavefronts) and walks i upward with c_prev and the block index of every (ray,
//                     azimuth) in registers; each H[i][k] is loaded once for the HORIZON_AZ azimuths, T_{j,i} is wave-uniform and read
//                     through the constant address space.  Nothing is written per step.  Once per HORIZON_TILE steps a wavefront
//                     whose every lane is blocked for every azimuth leaves the loop (rays below the horizon do so early).  At the
//                     end a ballot per azimuth and chunk gives the wavefront's highest failing ray, a shuffle its block index; the
//                     wavefronts meet once through LDS and one thread per azimuth takes the highest over them and stores the record.
//   k_horizon_refine  one wavefront per azimuth, lane = ray: rounds 2 to `rounds` of a FOUND record inside the kernel (horizon_trace:
//                     the serial stepper per lane as sight_trace runs it, the block test through i = m and the NaN rule; lo / hi of
//                     the next fan are read from lanes k* - 1 and k*), then lane 0 gathers the ridge of every record.
//                     No atomics; nothing depends on the order in which wavefronts arrive.
#pragma once

#include "atmrt_viewshed.h"

namespace atmrt {

constexpr int HORIZON_AZ = 4;    // azimuths per load of H: the viewshed scan's, whose registers it was chosen for
constexpr int HORIZON_TILE = 32; // steps between two looks at whether the wavefront may leave the step loop
// the scan's shape is the viewshed's: rays a lane owns and wavefronts of a block
ATMRT_HD int horizon_rays_per_lane(int K) { return viewshed_rays_per_lane(K); }
ATMRT_HD int horizon_waves(int K) { return viewshed_waves(K); }

// One batch of azimuths: profiles of m + 1 entries each (azimuth j of the batch at j * (m + 1)), `out` at the batch's first record.
struct HorizonScan {
  int32_t n, m, K;
  double lo, hi;   // the first fan
  const double* H; // [m + 1][K]
  const double* T; // [n][m + 1]
  atmrt_horizon_t* out;
};
void launch_horizon_scan(const HorizonScan& s, hipStream_t stream);
// rounds 2 to `rounds` of the batch's FOUND records, and the ridge of every record; b.meta: every azimuth's profile, m the call's
void launch_horizon_refine(const Frame& f, const SightBatch& b, int rounds, atmrt_horizon_t* out, hipStream_t stream);

} // namespace atmrt

#if defined(ATMRT_HORIZON_KERNELS)
#include "atmrt_device.h"

namespace atmrt {

typedef const __attribute__((address_space(4))) double* HorizonConstF64;

// LDS: int32 kmax[A][W] (a wavefront's highest failing ray + 1), then int32 kblk[A][W] (that ray's block index, 0: it failed by NaN)
static inline size_t horizon_lds_bytes(int K) { return 2 * sizeof(int32_t) * HORIZON_AZ * (size_t)horizon_waves(K); }

template <int R>
__global__ __launch_bounds__(256 * R) void k_horizon_scan(HorizonScan s) {
  constexpr int A = HORIZON_AZ, TILE = HORIZON_TILE;
  extern __shared__ int32_t horizon_lds[];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), W = (int)(blockDim.x >> 6);
  const int K = s.K, m = s.m;
  int32_t* const kmax = horizon_lds;
  int32_t* const kblk = horizon_lds + A * W;
  const int j0 = blockIdx.x * A;
  const size_t row = (size_t)m + 1;
  HorizonConstF64 T[A];
  double t0[A];
#pragma unroll
  for (int a = 0; a < A; a++) { // a surplus azimuth of the last block repeats the batch's last one and stores nothing
    const int j = j0 + a < s.n ? j0 + a : s.n - 1;
    T[a] = (HorizonConstF64)(uintptr_t)(s.T + (size_t)j * row);
    t0[a] = T[a][0];
  }
  bool live[R]; // wave-uniform: the chunk lies inside the fan
  int k[R];
  double h_prev[R], c_prev[R][A];
  int blk[R][A]; // 0: not blocked so far; an index is at least 1
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int chunk = w * R + r;
    live[r] = chunk * 64 < K;
    k[r] = chunk * 64 + lane;
    h_prev[r] = live[r] ? s.H[k[r]] : 0.0;
#pragma unroll
    for (int a = 0; a < A; a++) c_prev[r][a] = h_prev[r] - t0[a], blk[r][a] = 0;
  }
  for (int i0 = 1; i0 <= m; i0 += TILE) {
    const int i1 = m - i0 + 1 < TILE ? m : i0 + TILE - 1;
    for (int i = i0; i <= i1; i++) {
      double h[R];
#pragma unroll
      for (int r = 0; r < R; r++) h[r] = live[r] ? s.H[(size_t)i * K + k[r]] : 0.0;
#pragma unroll
      for (int a = 0; a < A; a++) {
        const double t = T[a][i];
#pragma unroll
        for (int r = 0; r < R; r++) {
          if (live[r]) {
            const double c = h[r] - t;
            if (blk[r][a] == 0 && (h_prev[r] < -1000.0 || c_prev[r][a] * c < 0.0)) blk[r][a] = i;
            c_prev[r][a] = c;
          }
        }
      }
#pragma unroll
      for (int r = 0; r < R; r++) h_prev[r] = h[r];
    }
    bool stopped = true; // every ray of this lane, against every azimuth
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
      for (int a = 0; a < A; a++) stopped = stopped && (!live[r] || blk[r][a] != 0);
    if (__all(stopped)) break;
  }
  // h_prev is H_m unless the wavefront left early, and then every ray is blocked: the NaN rule is not asked
#pragma unroll
  for (int a = 0; a < A; a++) {
    int kw = 0, bw = 0; // chunks ascend with r: a later one with a failing ray replaces an earlier one
#pragma unroll
    for (int r = 0; r < R; r++) {
      if (live[r]) {
        const bool fails = blk[r][a] != 0 || h_prev[r] != h_prev[r];
        const unsigned long long b = __ballot(fails);
        const int p = sight_pick(b);
        const int bi = __shfl(blk[r][a], p > 0 ? p - 1 : 0, 64);
        if (b) kw = (w * R + r) * 64 + p, bw = bi;
      }
    }
    if (lane == 0) kmax[a * W + w] = kw, kblk[a * W + w] = bw;
  }
  __syncthreads();
  const int a = threadIdx.x, j = j0 + a;
  if (a >= A || j >= s.n) return;
  int ks = 0, bi = 0; // wavefronts ascend with the rays: a later one with a failing ray replaces an earlier one
  for (int ww = 0; ww < W; ww++) {
    const int v = kmax[a * W + ww];
    if (v > 0) ks = v, bi = kblk[a * W + ww];
  }
  const double delta = viewshed_fan_delta(s.lo, s.hi, K);
  atmrt_horizon_t o;
  o.status = ks == K ? ATMRT_HORIZON_ABOVE_FAN : ks == 0 ? ATMRT_HORIZON_BELOW_FAN : ATMRT_HORIZON_FOUND;
  o.rounds_done = 1;
  o.k_star = ks;
  o.block_index = bi > 0 ? bi : -1;
  o.angle_clear = ks == K ? qnan() : sight_fan_angle(s.lo, delta, ks);
  o.angle_blocked = ks == 0 ? qnan() : sight_fan_angle(s.lo, delta, ks - 1);
  o.resolution = delta;
  o.block_distance = o.block_lat = o.block_lon = o.block_elevation = qnan(); // the ridge: k_horizon_refine
  s.out[j] = o;
}

// One ray against one profile (T wave-uniform, m wave-uniform), the block test through i = m: the per-lane part of the rule.
// -> the ray fails; block: the i' it is blocked at, -1 if it is not.  Every lane of the wavefront must call this together.
static __device__ __forceinline__ bool horizon_trace(const Frame& f, double alt, HorizonConstF64 T, int m, double e_deg, int& block) {
  const bool sph = f.earth.spherical != 0, straight = f.p.straight_rays != 0;
  const double radius = f.earth.shape_radius, step = f.p.simulation_step;
  Stepper s;
  stepper_init(s, sph, radius, alt, dm_to_radians(e_deg));
  double h_prev = alt, c_prev = alt - T[0];
  bool blocked = false;
  block = -1;
  for (int i = 1; i <= m; i++) {
    const double t = T[i];
    if (!blocked) {
      const RayState st = stepper_next(s, *f.atm, sph, radius, straight, step);
      const double c = st.h - t;
      if (h_prev < -1000.0 || c_prev * c < 0.0) {
        blocked = true;
        block = i;
      }
      c_prev = c;
      h_prev = st.h;
    }
    if (__all(blocked)) break;
  }
  return blocked || h_prev != h_prev; // not blocked: h_prev is H_m
}

constexpr int HORIZON_WAVES = 4; // wavefronts (azimuths) per block

__global__ __launch_bounds__(64 * HORIZON_WAVES) void k_horizon_refine(Frame f, SightBatch b, int rounds, atmrt_horizon_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int t = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * HORIZON_WAVES + (threadIdx.x >> 6)));
  if (t >= b.n) return; // the whole wavefront
  const SightMeta me = b.meta[t];
  const int m = me.m;
  const HorizonConstF64 T = (HorizonConstF64)(uintptr_t)(b.T + me.off);
  const double alt = *b.alt;
  atmrt_horizon_t o = out[t]; // round one's, the same in every lane
  const int status = __builtin_amdgcn_readfirstlane(o.status);
  if (status == ATMRT_HORIZON_FOUND) {
    double lo = o.angle_blocked, hi = o.angle_clear;
    for (int r = 1; r < rounds; r++) {
      const double delta = sight_fan_delta(lo, hi);
      const double e = sight_fan_angle(lo, delta, lane);
      int bi;
      const bool fails = horizon_trace(f, alt, T, m, e, bi);
      const int ks = sight_pick(__ballot(fails));
      o.rounds_done = r + 1;
      if (ks == 0 || ks == SIGHT_FAN) { // discarded: the bracket stays, the failing ray of record is this round's ray 0
        o.block_index = __shfl(bi, 0, 64);
        break;
      }
      lo = __shfl(e, ks - 1, 64);
      hi = __shfl(e, ks, 64);
      o.block_index = __shfl(bi, ks - 1, 64);
      o.resolution = delta;
    }
    o.angle_blocked = lo;
    o.angle_clear = hi;
  }
  if (lane != 0) return;
  if (o.block_index >= 0) {
    o.block_distance = b.dtab[o.block_index];
    o.block_lat = b.lat[me.off + o.block_index];
    o.block_lon = b.lon[me.off + o.block_index];
    o.block_elevation = b.T[me.off + o.block_index];
  } else {
    o.block_distance = o.block_lat = o.block_lon = o.block_elevation = qnan();
  }
  out[t] = o;
}

void launch_horizon_scan(const HorizonScan& s, hipStream_t stream) {
  const dim3 grid(cdiv((size_t)s.n, HORIZON_AZ)), block(64 * horizon_waves(s.K));
  const size_t lds = horizon_lds_bytes(s.K);
  switch (horizon_rays_per_lane(s.K)) {
    case 1: hipLaunchKernelGGL(k_horizon_scan<1>, grid, block, lds, stream, s); break;
    case 2: hipLaunchKernelGGL(k_horizon_scan<2>, grid, block, lds, stream, s); break;
    default: hipLaunchKernelGGL(k_horizon_scan<4>, grid, block, lds, stream, s); break;
  }
}
void launch_horizon_refine(const Frame& f, const SightBatch& b, int rounds, atmrt_horizon_t* out, hipStream_t stream) {
  hipLaunchKernelGGL(k_horizon_refine, dim3(cdiv((size_t)b.n, HORIZON_WAVES)), dim3(64 * HORIZON_WAVES), 0, stream, f, b, rounds, out);
}

} // namespace atmrt
#endif
