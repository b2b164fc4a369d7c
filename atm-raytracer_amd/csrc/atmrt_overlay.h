// atmrt_overlay.h — kernels of the image annotations of renderer::output_image (src/renderer/mod.rs:270-365, 416-431): tick
// lines, and the lines of constant elevation angle (flat-Earth horizon, eye level).  Included by atmrt_kernels.hip only.
//
// The one kernel with real work is k_overlay_find_elev: find_elev (:325-343) for every column is a scan of the whole [H][W] f64
// elevation plane (67 MB at 4096 x 2048), everything else touches W + H values or a few thousand pixels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace atmrt {

constexpr int OVERLAY_TARGETS = 2; // flat horizon, eye level: both searched in one pass over the plane

// One pixel of the RGB8 image; pixels outside the image are skipped, not clamped.
__device__ inline void overlay_plot(uint8_t* __restrict__ rgb, int w, int h, int x, int y, uint8_t r, uint8_t g, uint8_t b) {
  if (x < 0 || y < 0 || x >= w || y >= h) return;
  uint8_t* p = rgb + 3 * ((size_t)y * w + x);
  p[0] = r, p[1] = g, p[2] = b;
}

// The line rule (imageproc's draw_line_segment_mut is an absent crate): Bresenham over the longer axis — a steep
// line (|dy| > |dx|) is transposed, the end points ordered so that the running coordinate ascends, error = dx / 2 in f32; every
// running coordinate from start to end inclusive is plotted, then error -= dy and, once negative, the other coordinate steps and
// error += dx.
__device__ inline void overlay_segment(uint8_t* __restrict__ rgb, int w, int h, int x0, int y0, int x1, int y1, uint8_t r,
                                       uint8_t g, uint8_t b) {
  const int adx = x1 > x0 ? x1 - x0 : x0 - x1, ady = y1 > y0 ? y1 - y0 : y0 - y1;
  const bool steep = ady > adx;
  if (steep) {
    int t = x0; x0 = y0; y0 = t;
    t = x1; x1 = y1; y1 = t;
  }
  if (x0 > x1) {
    int t = x0; x0 = x1; x1 = t;
    t = y0; y0 = y1; y1 = t;
  }
  const float dx = (float)(x1 - x0), dy = (float)(y1 > y0 ? y1 - y0 : y0 - y1);
  const int ystep = y0 < y1 ? 1 : -1;
  float error = dx / 2.0f;
  int y = y0;
  for (int x = x0; x <= x1; x++) {
    if (steep) overlay_plot(rgb, w, h, y, x, r, g, b);
    else overlay_plot(rgb, w, h, x, y, r, g, b);
    error -= dy;
    if (error < 0.0f) {
      y += ystep;
      error += dx;
    }
  }
}

// find_elev's scan for every column and up to two targets, the rows cut into gridDim.y bands: block (bx, band) is one wavefront
// whose lane l owns column 64 bx + l, so every row it reads is 512 contiguous bytes, and each lane keeps (|e - target|, y) of the
// closest row of its band under the reference's strict `<` in ascending y — the first of equal minima stays, and a NaN row never
// wins because the distance starts at +inf like |closest_elev - elev| with closest_elev = +inf.  Four rows are loaded before they
// are compared so that four loads per lane are in flight.  part_d / part_y: [OVERLAY_TARGETS][bands][w].
__global__ __launch_bounds__(64) void k_overlay_find_elev(const double* __restrict__ elev, int w, int h, int rows_per_band,
                                                          double t0, double t1, double* __restrict__ part_d,
                                                          int32_t* __restrict__ part_y) {
  const int x = blockIdx.x * 64 + threadIdx.x;
  if (x >= w) return;
  const int band = blockIdx.y, bands = gridDim.y;
  const int y_begin = band * rows_per_band;
  const int y_end = y_begin + rows_per_band < h ? y_begin + rows_per_band : h;
  double d0 = INFINITY, d1 = INFINITY;
  int32_t b0 = 0, b1 = 0;
  const double* col = elev + x;
  int y = y_begin;
  for (; y + 4 <= y_end; y += 4) {
    double e[4];
#pragma unroll
    for (int k = 0; k < 4; k++) e[k] = col[(size_t)(y + k) * w];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const double a0 = fabs(e[k] - t0), a1 = fabs(e[k] - t1);
      if (a0 < d0) d0 = a0, b0 = y + k;
      if (a1 < d1) d1 = a1, b1 = y + k;
    }
  }
  for (; y < y_end; y++) {
    const double e = col[(size_t)y * w];
    const double a0 = fabs(e - t0), a1 = fabs(e - t1);
    if (a0 < d0) d0 = a0, b0 = y;
    if (a1 < d1) d1 = a1, b1 = y;
  }
  const size_t i0 = (size_t)band * w + x, i1 = ((size_t)bands + band) * w + x;
  part_d[i0] = d0, part_y[i0] = b0;
  part_d[i1] = d1, part_y[i1] = b1;
}

// The bands of a column combined in ascending order, again with strict `<` (together: the sequential scan), then find_elev's
// neighbour test: |closest - target| < |neighbour - closest| * 1.5 with the neighbour in row best - 1, row 1 when best is 0.
// y_of_x: [OVERLAY_TARGETS][w], -1 for None.  A column whose distance is still +inf (every row NaN or infinite) has
// closest_elev = +inf in the reference: inf < anything is false, None.
__global__ __launch_bounds__(256) void k_overlay_pick_elev(const double* __restrict__ elev, int w, int h, int bands, double t0,
                                                           double t1, const double* __restrict__ part_d,
                                                           const int32_t* __restrict__ part_y, int32_t* __restrict__ y_of_x) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= w) return;
  for (int t = 0; t < OVERLAY_TARGETS; t++) {
    const double target = t ? t1 : t0;
    double d = INFINITY;
    int32_t best = 0;
    for (int b = 0; b < bands; b++) {
      const size_t i = ((size_t)t * bands + b) * w + x;
      const double db = part_d[i];
      if (db < d) d = db, best = part_y[i];
    }
    int32_t out = -1;
    if (d < INFINITY) {
      const double closest = elev[(size_t)best * w + x];
      const double neighbour = elev[(size_t)(best == 0 ? 1 : best - 1) * w + x];
      if (fabs(closest - target) < fabs(neighbour - closest) * 1.5) out = best;
    }
    y_of_x[(size_t)t * w + x] = out;
  }
}

// draw_const_elev (:345-365): one thread per column x >= 1 joins (x - 1, y_old) and (x, y_new) when both columns found the target.
__global__ __launch_bounds__(256) void k_overlay_lines(const int32_t* __restrict__ y_of_x, int w, int h, uint8_t* __restrict__ rgb,
                                                       uint8_t r, uint8_t g, uint8_t b) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x + 1;
  if (x >= w) return;
  const int32_t y_old = y_of_x[x - 1], y_new = y_of_x[x];
  if (y_old < 0 || y_new < 0) return;
  overlay_segment(rgb, w, h, x - 1, y_old, x, y_new, r, g, b);
}

// draw_ticks (:285-322) without the text: thread i draws tick i, (pos, 0) -> (pos, size) or, vertical, (0, pos) -> (size, pos), in
// white.  The lines are axis-aligned, so the rule above plots every pixel between the end points; the part outside the image is
// cut off the loop instead of being skipped pixel by pixel (size is any u32).
struct OverlayTick {
  uint32_t pos, size;
  int32_t vertical, _pad;
};
__global__ __launch_bounds__(64) void k_overlay_ticks(const OverlayTick* __restrict__ ticks, int n, int w, int h,
                                                      uint8_t* __restrict__ rgb) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const OverlayTick t = ticks[i];
  const uint32_t across = t.vertical ? (uint32_t)h : (uint32_t)w, along = t.vertical ? (uint32_t)w : (uint32_t)h;
  if (t.pos >= across) return;
  const uint32_t last = t.size < along - 1 ? t.size : along - 1;
  for (uint32_t k = 0; k <= last; k++) {
    if (t.vertical) overlay_plot(rgb, w, h, (int)k, (int)t.pos, 255, 255, 255);
    else overlay_plot(rgb, w, h, (int)t.pos, (int)k, 255, 255, 255);
  }
}

} // namespace atmrt
