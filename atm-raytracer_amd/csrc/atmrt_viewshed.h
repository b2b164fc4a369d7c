// atmrt_viewshed.h — the viewshed raster (include/atmrt.h, "viewshed": the rule is stated there): the first round of the sight-line
// rule at every cell of a polar lattice.  The host half of the rule, the kernels' shape and the launch interface for atmrt_polar.hip;
// the kernels themselves are compiled by atmrt_viewshed.hip only (ATMRT_VIEWSHED_KERNELS).
//
//   k_viewshed_paths  one lane per ray of the fan: the serial stepper exactly as sight_trace and k_ray_paths call it, all m steps
//                     whatever the ray meets.  The table is step-major, H[i][k]: a wavefront of the scan reads 64 consecutive doubles.
//   (profiles)        k_sight_calc / k_sight_profile through launch_sight_profile: every azimuth is a target whose m is the call's.
//   k_viewshed_scan   one block per VIEWSHED_AZ azimuths.  A lane owns ray k (R rays where K > 64 x the block's wavefronts) and walks
//                     i upward with c_prev and the block index of every (ray, azimuth) in registers; each H[i][k] is loaded once for
//                     the VIEWSHED_AZ azimuths.  T_{j,i} is wave-uniform and read through the constant address space.  Per step a
//                     ballot gives the chunk's highest failing ray; the wavefront keeps its own maximum of step i0 + t in lane t.
//                     Once per VIEWSHED_TILE steps the wavefronts meet through LDS: one thread per (azimuth, step) takes the maximum
//                     over wavefronts, reads ray k* - 1's block index from LDS, gathers the two H of ray k* and stores the record.
//                     No atomics; nothing depends on the order in which wavefronts arrive.
#pragma once

#include "atmrt_sight.h"

namespace atmrt {

constexpr int VIEWSHED_K_MAX = 4096;      // rays of a fan (a multiple of 64, at least 64)
constexpr size_t VIEWSHED_N_MAX = 65536;  // azimuths of a call
constexpr int VIEWSHED_AZ = 4;            // azimuths per load of H (profiles/viewshed_resources.txt)
constexpr int VIEWSHED_TILE = 64;         // steps between two meetings in LDS: lane t of a wavefront keeps step i0 + t

// ---- the rule's host half (atmrt_viewshed_fan_angles), the same code on the device: e_k = sight_fan_angle(lo, delta, k) ----------
ATMRT_HD double viewshed_fan_delta(double lo, double hi, int K) { return (hi - lo) / (double)(K - 1); }
ATMRT_HD bool viewshed_fan_rays_ok(int K) { return K >= 64 && K <= VIEWSHED_K_MAX && K % 64 == 0; }
// the scan's shape: rays a lane owns, and wavefronts of a block (chunk c = 64 consecutive rays belongs to wavefront c / R)
ATMRT_HD int viewshed_rays_per_lane(int K) { return K <= 256 ? 1 : K <= 1024 ? 2 : 4; }
ATMRT_HD int viewshed_waves(int K) { return (K / 64 + viewshed_rays_per_lane(K) - 1) / viewshed_rays_per_lane(K); }

// ---- launch interface -----------------------------------------------------------------------------------------------------------------
struct ViewshedPlanes { // [n_az][m], entry j * m + (i - 1); the last four may be null, and k_star where the viewshed map asks
  uint16_t* k_star;
  uint8_t* status;
  double* hidden;
  int32_t* block_index;
  double *ground, *lat, *lon;
};
// One batch of azimuths: profiles of m + 1 entries each (azimuth j of the batch at j * (m + 1)), `out` at the batch's first cell.
struct ViewshedScan {
  int32_t n, m, K;
  double height;
  const double* H;             // [m + 1][K]
  const double *T, *lat, *lon; // [n][m + 1]
  ViewshedPlanes out;
};
struct ViewshedAsked { // which planes a call wants beside status and hidden, which every call has
  bool k_star, block_index, ground, lat, lon;
};
static inline size_t viewshed_cell_bytes(const ViewshedAsked& a) { // of the planes asked for
  return (a.k_star ? 2 : 0) + 1 + 8 + (a.block_index ? 4 : 0) + (a.ground ? 8 : 0) + (a.lat ? 8 : 0) + (a.lon ? 8 : 0);
}
void launch_viewshed_paths(const Frame& f, double lo, double hi, int K, int m, double* H, hipStream_t stream);
void launch_viewshed_scan(const ViewshedScan& s, hipStream_t stream);

} // namespace atmrt

#if defined(ATMRT_VIEWSHED_KERNELS)
#include "atmrt_device.h"

namespace atmrt {

typedef const __attribute__((address_space(4))) double* ViewshedConstF64;

// K is a multiple of 64: every lane of every wavefront has a ray
__global__ __launch_bounds__(64) void k_viewshed_paths(Frame f, double lo, double hi, int K, int m, double* __restrict__ H) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  const bool sph = f.earth.spherical != 0, straight = f.p.straight_rays != 0;
  const double radius = f.earth.shape_radius, step = f.p.simulation_step;
  const double alt = observer_altitude(f);
  Stepper s;
  stepper_init(s, sph, radius, alt, dm_to_radians(sight_fan_angle(lo, viewshed_fan_delta(lo, hi, K), k)));
  H[k] = alt;
  for (int i = 1; i <= m; i++) {
    const RayState st = stepper_next(s, *f.atm, sph, radius, straight, step);
    H[(size_t)i * K + k] = st.h;
  }
}

// LDS: uint16 kmax[A][W][TILE] (a wavefront's highest failing ray + 1 of a step), then uint16 blk[A][W R 64] (a ray's block index,
// 0: none so far; an index is at least 1 and at most 65535)
static inline size_t viewshed_lds_bytes(int K) {
  const size_t W = (size_t)viewshed_waves(K), R = (size_t)viewshed_rays_per_lane(K);
  return 2 * VIEWSHED_AZ * (W * VIEWSHED_TILE + W * R * 64);
}

template <int R>
__global__ __launch_bounds__(256 * R) void k_viewshed_scan(ViewshedScan s) {
  constexpr int A = VIEWSHED_AZ, TILE = VIEWSHED_TILE;
  extern __shared__ uint16_t viewshed_lds[];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), W = (int)(blockDim.x >> 6);
  const int K = s.K, m = s.m, kpad = W * R * 64;
  uint16_t* const kmax = viewshed_lds;
  uint16_t* const blk_lds = viewshed_lds + A * W * TILE;
  const int j0 = blockIdx.x * A;
  const size_t row = (size_t)m + 1;
  ViewshedConstF64 T[A];
  double t_prev[A];
#pragma unroll
  for (int a = 0; a < A; a++) { // a surplus azimuth of the last block repeats the batch's last one and stores nothing
    const int j = j0 + a < s.n ? j0 + a : s.n - 1;
    T[a] = (ViewshedConstF64)(uintptr_t)(s.T + (size_t)j * row);
    t_prev[a] = T[a][0];
  }
  bool live[R]; // wave-uniform: the chunk lies inside the fan
  int k[R];
  double h_prev[R], c_prev[R][A];
  int blk[R][A];
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int chunk = w * R + r;
    live[r] = chunk * 64 < K;
    k[r] = chunk * 64 + lane;
    h_prev[r] = live[r] ? s.H[k[r]] : 0.0;
#pragma unroll
    for (int a = 0; a < A; a++) c_prev[r][a] = h_prev[r] - t_prev[a], blk[r][a] = 0;
  }
  for (int i0 = 1; i0 <= m; i0 += TILE) {
    const int n_t = m - i0 + 1 < TILE ? m - i0 + 1 : TILE;
    int mine[A];
#pragma unroll
    for (int a = 0; a < A; a++) mine[a] = 0;
    for (int it = 0; it < n_t; it++) {
      const int i = i0 + it;
      double h[R];
#pragma unroll
      for (int r = 0; r < R; r++) h[r] = live[r] ? s.H[(size_t)i * K + k[r]] : 0.0;
#pragma unroll
      for (int a = 0; a < A; a++) {
        const double t = T[a][i];
        const double ground = t_prev[a] + 1.0 * (t - t_prev[a]);
        const double aim = ground + s.height;
        int kw = 0; // chunks ascend with r: a later one with a failing ray replaces an earlier one
#pragma unroll
        for (int r = 0; r < R; r++) {
          if (live[r]) {
            const double arrival = h_prev[r] + 1.0 * (h[r] - h_prev[r]);
            const bool fails = blk[r][a] != 0 || !(arrival >= aim); // blocked at some i' <= i - 1, low, or NaN
            const unsigned long long b = __ballot(fails);
            if (b) kw = (w * R + r) * 64 + sight_pick(b);
            const double c = h[r] - t;
            if (blk[r][a] == 0 && (h_prev[r] < -1000.0 || c_prev[r][a] * c < 0.0)) blk[r][a] = i;
            c_prev[r][a] = c;
          }
        }
        if (lane == it) mine[a] = kw;
        t_prev[a] = t;
      }
#pragma unroll
      for (int r = 0; r < R; r++) h_prev[r] = h[r];
    }
#pragma unroll
    for (int a = 0; a < A; a++) {
      kmax[(a * W + w) * TILE + lane] = (uint16_t)mine[a];
#pragma unroll
      for (int r = 0; r < R; r++) blk_lds[a * kpad + (w * R + r) * 64 + lane] = (uint16_t)blk[r][a];
    }
    __syncthreads();
    for (int cell = threadIdx.x; cell < A * TILE; cell += blockDim.x) {
      const int a = cell / TILE, it = cell % TILE, j = j0 + a, i = i0 + it;
      if (it >= n_t || j >= s.n) continue;
      int ks = 0;
      for (int ww = 0; ww < W; ww++) {
        const int v = kmax[(a * W + ww) * TILE + it];
        ks = v > ks ? v : ks;
      }
      const double* Tj = s.T + (size_t)j * row;
      const double t0 = Tj[i - 1], t1 = Tj[i];
      const double ground = t0 + 1.0 * (t1 - t0);
      const double aim = ground + s.height;
      int block = -1; // of ray k* - 1, where the status is HIDDEN
      if (ks > 0 && ks < K) {
        const int bi = blk_lds[a * kpad + ks - 1];
        if (bi != 0 && bi <= i - 1) block = bi;
      }
      double hidden = qnan();
      if (ks < K) {
        const double h0 = s.H[(size_t)(i - 1) * K + ks], h1 = s.H[(size_t)i * K + ks];
        const double arrival = h0 + 1.0 * (h1 - h0);
        hidden = arrival - aim;
        if (hidden != hidden) hidden = qnan();
      }
      const size_t o = (size_t)j * m + (i - 1);
      if (s.out.k_star) s.out.k_star[o] = (uint16_t)ks;
      s.out.status[o] = (uint8_t)(ks == K ? ATMRT_SIGHT_ABOVE_FAN : ks == 0 ? ATMRT_SIGHT_BELOW_FAN : block >= 0 ? ATMRT_SIGHT_HIDDEN : ATMRT_SIGHT_SEEN);
      s.out.hidden[o] = hidden;
      if (s.out.block_index) s.out.block_index[o] = block;
      if (s.out.ground) s.out.ground[o] = ground;
      if (s.out.lat) s.out.lat[o] = s.lat[(size_t)j * row + i];
      if (s.out.lon) s.out.lon[o] = s.lon[(size_t)j * row + i];
    }
    __syncthreads(); // the next tile writes the same LDS
  }
}

void launch_viewshed_paths(const Frame& f, double lo, double hi, int K, int m, double* H, hipStream_t stream) {
  hipLaunchKernelGGL(k_viewshed_paths, dim3(K / 64), dim3(64), 0, stream, f, lo, hi, K, m, H);
}
void launch_viewshed_scan(const ViewshedScan& s, hipStream_t stream) {
  const dim3 grid(cdiv((size_t)s.n, VIEWSHED_AZ)), block(64 * viewshed_waves(s.K));
  const size_t lds = viewshed_lds_bytes(s.K);
  switch (viewshed_rays_per_lane(s.K)) {
    case 1: hipLaunchKernelGGL(k_viewshed_scan<1>, grid, block, lds, stream, s); break;
    case 2: hipLaunchKernelGGL(k_viewshed_scan<2>, grid, block, lds, stream, s); break;
    default: hipLaunchKernelGGL(k_viewshed_scan<4>, grid, block, lds, stream, s); break;
  }
}

} // namespace atmrt
#endif
