// atmrt_shadow.h — cast shadows (include/atmrt.h, "cast shadows": the rule is stated there): which of a finished frame's first
// trace points the light reaches.  The launch interface for atmrt_consumers.hip; the kernels themselves are compiled by atmrt_shadow.hip
// only (ATMRT_SHADOW_KERNELS).
//
//   k_shadow_compact  one thread per pixel: the pixels with a trace point appended to a list, a wavefront's entries contiguous and
//                     in lane order (wave_compact_append), so that the march's wavefronts are full — the sky half of a frame costs
//                     no lanes; a pixel without one gets ATMRT_SHADOW_NONE (and block 0) here
//   k_shadow_march    one list entry per lane: dircalc_new at the point, the stepper from H_0, then per step coords_at_dist,
//                     terrain_elev_or_zero and the rule's test.  A lane that is decided idles (it is not in the stepper's votes any
//                     more, as in sight_trace); the wavefront leaves when all its lanes are decided.  Writes status and block of
//                     its pixel; the counts of the call with one atomic per wavefront and counter.
//   k_shadow_lights   ("shadow lights" of include/atmrt.h) one list entry per lane over the same list and a wave-uniform loop over
//                     the call's lights: world_directions of the point, the light's local direction there
//                     (shadow_local_direction), dircalc_new, the stepper and k_shadow_march's step loop (shadow_step_loop, one
//                     function for both kernels).  The lane collects its LIT bits in a register and writes lit_mask[p] once: no
//                     atomics on the mask; the planes of the pixels without a trace point are cleared ahead of the compaction.
//                     The point and its three vectors are read and made again per light (keeping them across the step loop
//                     costs a wavefront per SIMD: profiles/shadow_lights_resources.txt).  TRUE_DIR ("apparent elevation" of
//                     include/atmrt.h: the lights are TRUE directions) puts sky_apparent(H_0, elevation) between the local
//                     direction and the three no-march tests: two bisections over the refraction table per pair, a dozen loads
//                     each, ahead of a march of 10 to 200 steps (profiles/shadow_true_resources.txt).
//
// The launch covers the pixels, not the list (its length stays on the device: no host round trip between the two kernels); a
// wavefront beyond the list's end leaves at once.
#pragma once

#include "atmrt_kernels.h"

namespace atmrt {

constexpr int SHADOW_M_MAX = 65535;
enum ShadowCtr : int { SH_LIST = 0, SH_LIT, SH_SHADOWED, SH_STEPS, SH_ESCAPED, SH_N };

struct ShadowJob {
  TracePoints src;      // dist and width are not read
  double azimuth_deg, elevation_deg, lift;
  int32_t m;
  int32_t escape;       // the shortcut is on
  double esc_floor;     // +inf: no certificate
  uint32_t* list;       // [n_pixels]
  unsigned long long* ctr; // [SH_N], zeroed by the launch
  uint8_t* status;      // [n_pixels]
  uint16_t* block;      // [n_pixels] or null
};
// f: the frame of the context's setting (prepare_frame), with esc_ang_max for this call's reach
void launch_shadow_mask(const Frame& f, const ShadowJob& job, hipStream_t stream, hipEvent_t ev_compacted);

constexpr uint32_t SHADOW_LIGHTS_MAX = 64;
struct ShadowLightsJob {
  TracePoints src;      // dist and width are not read
  const double* dirs;   // [n_lights][3] in device memory: the lights, normalised on the host
  uint32_t n_lights;    // 1 .. SHADOW_LIGHTS_MAX
  int32_t m;
  double lift;
  int32_t escape;       // the shortcut is on
  double esc_floor;     // +inf: no certificate
  uint32_t* list;       // [n_pixels]
  unsigned long long* ctr;      // [SH_N], zeroed by the launch
  unsigned long long* lit_mask; // [n_pixels] or null
  uint8_t* status;      // [n_lights][n_pixels] or null
  uint16_t* block;      // [n_lights][n_pixels] or null
  int32_t true_dir;     // the lights are true directions: the launch elevation is sky_apparent over `table`
  SkyTable table;       // read with true_dir alone
};
void launch_shadow_lights(const Frame& f, const ShadowLightsJob& job, hipStream_t stream, hipEvent_t ev_compacted);

} // namespace atmrt

#if defined(ATMRT_SHADOW_KERNELS)
#include "atmrt_device.h"

namespace atmrt {

__global__ __launch_bounds__(256) void k_shadow_compact(ShadowJob j) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = p < j.src.n_pixels;
  const bool hit = in && j.src.hit_count[p] != 0;
  wave_compact_append(hit, (uint32_t)p, j.list, &j.ctr[SH_LIST]); // every lane of the wavefront
  if (in && !hit && j.status) { // k_shadow_lights' planes are cleared by its launch: no status here
    j.status[p] = ATMRT_SHADOW_NONE;
    if (j.block) j.block[p] = 0;
  }
}

constexpr int SHADOW_WAVES = 4; // wavefronts per block

// The step loop of one wavefront, for both march kernels: from the stepper at H_0 = h0 and the geodesic `c`, the rule's test per step.
// `decided` lanes idle (they are not in the stepper's votes); the wavefront leaves when all its lanes are decided.  block: the
// index that shadows the ray (0: LIT); steps: the stepper steps taken; escaped: the ray passed the escape test before m.
template <bool CUBIC>
__device__ __forceinline__ void shadow_step_loop(const Frame& f, const Earth& e, const DirCalc& c, Stepper& s, double h0, int m, int escape,
                                                 double esc_floor, bool decided, int& block, int& steps, int& escaped) {
  const bool sph = e.spherical != 0, straight = f.p.straight_rays != 0;
  const double radius = e.shape_radius, step = f.p.simulation_step, skip_above = f.tv.skip_above;
  double h_prev = h0, d = 0.0;
  for (int i = 1; i <= m; i++) {
    d = d + step; // d_i: the additions of the stepper's x, wave-uniform
    if (!decided) {
      const RayState st = stepper_next<CUBIC>(s, *f.atm, sph, radius, straight, step);
      steps = i;
      // A sample above every post of the mosaic is above the terrain, whatever its geodesic point (skip_above, as in the frame's
      // march): H_i < T_i is false without the lookup.  A NaN height takes the full path and compares false there.
      bool under = false;
      if (!(st.h > skip_above)) {
        double lat, lon;
        coords_at_dist(e, c, d, lat, lon);
        under = st.h < terrain_elev_or_zero(f.tv, lat, lon);
      }
      if (h_prev < -1000.0 || under) { // utils.rs:167
        block = i;
        decided = true;
      } else if (escape && escapes(f, s, straight, st.h, h_prev, esc_floor)) { // LIT for good
        escaped = i < m ? 1 : 0;
        decided = true;
      }
      h_prev = st.h;
    }
    if (__all(decided)) break;
  }
}


template <int CALC, bool CUBIC>
__global__ __launch_bounds__(64 * SHADOW_WAVES) void k_shadow_march(Frame f, ShadowJob j) {
  const int lane = threadIdx.x & 63;
  const size_t first = (size_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * SHADOW_WAVES + (threadIdx.x >> 6))) * 64;
  const size_t n = (size_t)j.ctr[SH_LIST];
  if (first >= n) return; // the whole wavefront
  const bool live = first + lane < n;
  const uint32_t p = j.list[live ? first + lane : n - 1];
  const size_t k0 = j.src.hit_offset ? (size_t)j.src.hit_offset[p] : (size_t)p;
  const Earth e = earth_for<CALC>(f);
  DirCalc c;
  dircalc_new(e, j.src.lat[k0], j.src.lon[k0], j.azimuth_deg, c);
  const double h0 = j.src.elev[k0] + j.lift;
  Stepper s;
  stepper_init(s, e.spherical != 0, e.shape_radius, h0, dm_to_radians(j.elevation_deg));
  int block = 0, steps = 0, escaped = 0;
  shadow_step_loop<CUBIC>(f, e, c, s, h0, j.m, j.escape, j.esc_floor, !live, block, steps, escaped);
  if (live) {
    j.status[p] = block ? ATMRT_SHADOW_SHADOWED : ATMRT_SHADOW_LIT;
    if (j.block) j.block[p] = (uint16_t)block;
  }
  const unsigned long long n_lit = wave_sum(live && !block ? 1ull : 0ull), n_sh = wave_sum(live && block ? 1ull : 0ull);
  const unsigned long long n_steps = wave_sum((unsigned long long)steps), n_esc = wave_sum((unsigned long long)escaped);
  if (lane == 0) {
    if (n_lit) atomicAdd(&j.ctr[SH_LIT], n_lit);
    if (n_sh) atomicAdd(&j.ctr[SH_SHADOWED], n_sh);
    if (n_steps) atomicAdd(&j.ctr[SH_STEPS], n_steps);
    if (n_esc) atomicAdd(&j.ctr[SH_ESCAPED], n_esc);
  }
}

void launch_shadow_mask(const Frame& f, const ShadowJob& job, hipStream_t stream, hipEvent_t ev_compacted) {
  const size_t n = job.src.n_pixels;
  (void)hipMemsetAsync(job.ctr, 0, SH_N * sizeof(unsigned long long), stream);
  hipLaunchKernelGGL(k_shadow_compact, dim3(cdiv(n, 256)), dim3(256), 0, stream, job);
  if (ev_compacted) (void)hipEventRecord(ev_compacted, stream);
  const dim3 grid(cdiv(n, 64 * SHADOW_WAVES)), blk(64 * SHADOW_WAVES);
  if (f.atm_cubic) {
    ATMRT_DISPATCH_CALC(f.earth.calc, hipLaunchKernelGGL((k_shadow_march<CALC, true>), grid, blk, 0, stream, f, job));
  } else {
    ATMRT_DISPATCH_CALC(f.earth.calc, hipLaunchKernelGGL((k_shadow_march<CALC, false>), grid, blk, 0, stream, f, job));
  }
}

// include/atmrt.h, "shadow lights".  Per lane: one list entry, every light of the call in turn.  The loop over the lights is
// wave-uniform (n_lights and the lights are the call's), so the votes of the step loop are those of k_shadow_march.
template <int CALC, bool CUBIC, bool TRUE_DIR>
__global__ __launch_bounds__(64 * SHADOW_WAVES) void k_shadow_lights(Frame f, ShadowLightsJob j) {
  const int lane = threadIdx.x & 63;
  const size_t first = (size_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * SHADOW_WAVES + (threadIdx.x >> 6))) * 64;
  const size_t n = (size_t)j.ctr[SH_LIST];
  if (first >= n) return; // the whole wavefront
  const bool live = first + lane < n;
  const uint32_t p = j.list[live ? first + lane : n - 1];
  const Earth e = earth_for<CALC>(f);
  // Across the step loop the lane keeps its pixel, its LIT bits and one word of counts (steps in bits 0..23: at most 64 * 65535;
  // escaped rays from bit 24 on: at most 64) and reads its point again for every light: three loads and world_directions against
  // one march, and the registers that decide the kernel's occupancy.
  unsigned long long bits = 0;
  unsigned work = 0;
  for (uint32_t l = 0; l < j.n_lights; l++) {
    const size_t k0 = j.src.hit_offset ? (size_t)j.src.hit_offset[p] : (size_t)p;
    const double lat = j.src.lat[k0], lon = j.src.lon[k0];
    const double h0 = j.src.elev[k0] + j.lift;
    const Vec3 light = v3(j.dirs[3 * l], j.dirs[3 * l + 1], j.dirs[3 * l + 2]);
    double azimuth_deg, elevation_deg;
    {
      Vec3 vn, ve, vu;
      world_directions(e, lat, lon, vn, ve, vu);
      shadow_local_direction(vn, ve, vu, light, azimuth_deg, elevation_deg);
    }
    if (TRUE_DIR) { // the light's true elevation -> where it appears from H_0; straight rays: itself
      if (!f.p.straight_rays && elevation_deg > -90.0 && elevation_deg < 90.0) elevation_deg = sky_apparent(j.table, h0, elevation_deg);
    }
    // decided without a march: the zenith (LIT), the nadir (SHADOWED, block 1), a NaN (LIT); 0 steps
    const bool marches = elevation_deg > -90.0 && elevation_deg < 90.0;
    int block = !marches && elevation_deg <= -90.0 ? 1 : 0, steps = 0, escaped = 0;
    DirCalc c;
    dircalc_new(e, lat, lon, azimuth_deg, c);
    Stepper s;
    stepper_init(s, e.spherical != 0, e.shape_radius, h0, dm_to_radians(elevation_deg));
    shadow_step_loop<CUBIC>(f, e, c, s, h0, j.m, j.escape, j.esc_floor, !live || !marches, block, steps, escaped);
    if (live) {
      const size_t at = (size_t)l * j.src.n_pixels + p;
      if (j.status) j.status[at] = block ? ATMRT_SHADOW_SHADOWED : ATMRT_SHADOW_LIT;
      if (j.block) j.block[at] = (uint16_t)block;
      if (!block) bits |= 1ull << l;
      work += (unsigned)steps + ((unsigned)escaped << 24);
    }
  }
  if (live && j.lit_mask) j.lit_mask[p] = bits;
  const unsigned long long lit = live ? (unsigned long long)__popcll(bits) : 0ull;
  const unsigned long long n_lit = wave_sum(lit), n_sh = wave_sum(live ? j.n_lights - lit : 0ull);
  const unsigned long long n_steps = wave_sum((unsigned long long)(work & 0xffffffu)), n_esc = wave_sum((unsigned long long)(work >> 24));
  if (lane == 0) {
    if (n_lit) atomicAdd(&j.ctr[SH_LIT], n_lit);
    if (n_sh) atomicAdd(&j.ctr[SH_SHADOWED], n_sh);
    if (n_steps) atomicAdd(&j.ctr[SH_STEPS], n_steps);
    if (n_esc) atomicAdd(&j.ctr[SH_ESCAPED], n_esc);
  }
}

void launch_shadow_lights(const Frame& f, const ShadowLightsJob& job, hipStream_t stream, hipEvent_t ev_compacted) {
  const size_t n = job.src.n_pixels, planes = n * job.n_lights;
  (void)hipMemsetAsync(job.ctr, 0, SH_N * sizeof(unsigned long long), stream);
  // the pixels without a trace point: mask 0, ATMRT_SHADOW_NONE (0) in every light's plane, block 0; the march writes the others
  if (job.lit_mask) (void)hipMemsetAsync(job.lit_mask, 0, n * sizeof(unsigned long long), stream);
  if (job.status) (void)hipMemsetAsync(job.status, 0, planes, stream);
  if (job.block) (void)hipMemsetAsync(job.block, 0, planes * sizeof(uint16_t), stream);
  ShadowJob list{};
  list.src = job.src, list.list = job.list, list.ctr = job.ctr;
  hipLaunchKernelGGL(k_shadow_compact, dim3(cdiv(n, 256)), dim3(256), 0, stream, list);
  if (ev_compacted) (void)hipEventRecord(ev_compacted, stream);
  const dim3 grid(cdiv(n, 64 * SHADOW_WAVES)), blk(64 * SHADOW_WAVES);
  if (job.true_dir) {
    if (f.atm_cubic) {
      ATMRT_DISPATCH_CALC(f.earth.calc, hipLaunchKernelGGL((k_shadow_lights<CALC, true, true>), grid, blk, 0, stream, f, job));
    } else {
      ATMRT_DISPATCH_CALC(f.earth.calc, hipLaunchKernelGGL((k_shadow_lights<CALC, false, true>), grid, blk, 0, stream, f, job));
    }
  } else if (f.atm_cubic) {
    ATMRT_DISPATCH_CALC(f.earth.calc, hipLaunchKernelGGL((k_shadow_lights<CALC, true, false>), grid, blk, 0, stream, f, job));
  } else {
    ATMRT_DISPATCH_CALC(f.earth.calc, hipLaunchKernelGGL((k_shadow_lights<CALC, false, false>), grid, blk, 0, stream, f, job));
  }
}

} // namespace atmrt
#endif
