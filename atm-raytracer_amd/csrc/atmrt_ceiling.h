// atmrt_ceiling.h — the terrain ceiling table of the Rectilinear lean march (Spherical calculator): for every step i of the distance
// table and every azimuth bin j of the frame, an upper bound of the terrain under the sample of step i of ANY ray whose direction
// falls into bin j, and the maximum of those bounds over the steps from i on.  The march (atmrt_march_impl.h, march_steps) skips
// the geodesic point and the lookup of a sample above its cell, and lets an ascending ray leave once it is above its bin's suffix.
// Host + device: the kernels that fill the table (atmrt_kernels.hip, k_ceiling_cells / k_ceiling_suffix) and the stand-alone test
// program (tests/csrc/ceiling_host.cpp) run the same functions.
#pragma once

#include "atmrt_core.h"

namespace atmrt {

// One table entry: 8 B, one load per lane and step.
struct alignas(8) CeilEntry {
  float cell;   // >= terrain_elev_or_zero at the sample of this step, for every direction of the bin, + 1 m (rounded up; >= 1)
  float suffix; // max of `cell` over this step and every later one
};

// The bins: `n_bins` equal intervals of width `w` over the rays' directions RELATIVE to the frame's direction, from rel_lo on.
// A direction outside [rel_lo, rel_lo + n_bins w) — or NaN — has the bin n_bins, whose column of the table holds the mosaic's
// global numbers.  Row i of the table is entry[i * (n_bins + 1) + bin].
struct CeilLayout {
  double dir0;   // the frame's direction in radians
  double rel_lo; // lower edge of bin 0, relative to dir0, in [-pi, pi)
  double w;      // width of a bin in radians
  double inv_w;
  int32_t n_bins;
  int32_t _pad;
};
constexpr double CEIL_BIN_DEG = 0.15;  // width of a bin
constexpr int CEIL_MAX_BINS = 2400;    // the whole circle
constexpr double CEIL_PI = 3.14159265358979323846;

// direction - dir0 wrapped into [-pi, pi): a frame that looks along +-pi (yaw 180 degrees) has its rays on both sides of atan2's cut
ATMRT_HD double ceiling_rel(double dir0, double direction) {
  double rel = direction - dir0;
  rel -= 2.0 * CEIL_PI * dm_floor((rel + CEIL_PI) / (2.0 * CEIL_PI));
  return rel;
}
// The bin of a ray: a function of its direction alone (radians, as rect_ray_params returns it), so the same ray has the same bin in
// every launch shape, tile cut and march variant.
ATMRT_HD int ceiling_bin(const CeilLayout& L, double direction) {
  const double t = (ceiling_rel(L.dir0, direction) - L.rel_lo) * L.inv_w;
  return t >= 0.0 && t < (double)L.n_bins ? (int)t : L.n_bins; // NaN: neither comparison holds
}
// The directions (radians) that bound bin j, widened by far more than the rounding of ceiling_bin's arithmetic (1e-9 rad is
// 0.2 mm at 200 km): every direction with ceiling_bin == j lies between them.
ATMRT_HD void ceiling_bin_edges(const CeilLayout& L, int j, double& d_lo, double& d_hi) {
  d_lo = L.dir0 + L.rel_lo + (double)j * L.w - 1.0e-9;
  d_hi = L.dir0 + L.rel_lo + (double)(j + 1) * L.w + 1.0e-9;
}

// The bins of the frame's terrain ceiling table: the azimuth range of the shard's rays, from its border pixels (an image that
// holds the zenith or the nadir has rays outside that range: they take the table's last column, the mosaic's top).  Bin edges are
// whole multiples of the bin width relative to the frame's direction, so a column tile cuts the same bins as the whole frame and
// a ray's bin covers the same directions in both.
inline CeilLayout ceiling_layout(const atmrt_params_t& p, const Pinhole& ph, int c0, int wl, int h) {
  CeilLayout L{};
  L.dir0 = dm_to_radians(p.frame.direction);
  L.w = dm_to_radians(CEIL_BIN_DEG);
  L.inv_w = 1.0 / L.w;
  double lo = dm_inf(), hi = -dm_inf();
  auto see = [&](int x, int y) {
    double direction, elevation;
    rect_ray_params(p, ph, x, y, direction, elevation);
    const double rel = ceiling_rel(L.dir0, direction);
    if (rel == rel) lo = (rel < lo ? rel : lo), hi = (rel > hi ? rel : hi);
  };
  for (int x = c0; x < c0 + wl; x++) see(x, 0), see(x, h - 1);
  for (int y = 0; y < h; y++) see(c0, y), see(c0 + wl - 1, y);
  if (!(lo <= hi)) lo = hi = 0.0;
  const double k_lo = dm_floor(lo * L.inv_w) - 1.0, k_hi = dm_floor(hi * L.inv_w) + 2.0; // a bin to spare on both sides
  L.rel_lo = k_lo * L.w;
  L.n_bins = (int32_t)(k_hi - k_lo < (double)CEIL_MAX_BINS ? k_hi - k_lo : (double)CEIL_MAX_BINS);
  return L;
}


// A lookup that a bounding box cannot describe (it crosses the date line, comes close to a pole, holds a NaN or spans more than a
// degree per side): the caller uses the mosaic's top.
constexpr float CEIL_UNBOUNDED = -1.0f;

// THE COVER.  The samples of step i of the rays of one bin lie on an arc of the circle of radius `dist` (along the ground) around
// the observer, between the geodesic points (lat0, lon0) and (lat1, lon1) of the bin's two edge directions; the arc's angle is
// `w_arc`.  Returns max(0, every post whose bilinear square can hold a sample of the arc) + 1 m, rounded up to float:
//   * the arc stays within its sagitta dist (1 - cos(w_arc / 2)) of the chord between the end points, the chord within the end
//     points' lat/lon box up to the curvature of the lat/lon map over the chord's length ((dist w_arc)^2 / radius, times
//     1 + tan(lat)); both are converted to degrees (longitude: over cos of the box's highest latitude) and inflate the box;
//   * in every tile the box touches, in the tile's own index space (tiles of one mosaic may differ in resolution), the box is
//     widened by one post and rounded outwards to whole posts: a sample at fractional index f reads the posts floor(f) and
//     floor(f) + 1, both inside.  Every post taken lies within the box inflated by two posts;
//   * a missing tile and everything outside the mosaic is 0 m, which the maximum starts from.
ATMRT_HD float ceiling_cover(const TerrainView& tv, double radius, double lat0, double lon0, double lat1, double lon1, double dist, double w_arc) {
  if (!(lat0 == lat0 && lon0 == lon0 && lat1 == lat1 && lon1 == lon1)) return CEIL_UNBOUNDED;
  double la_lo = lat0 < lat1 ? lat0 : lat1, la_hi = lat0 < lat1 ? lat1 : lat0;
  double lo_lo = lon0 < lon1 ? lon0 : lon1, lo_hi = lon0 < lon1 ? lon1 : lon0;
  const double la_abs = dm_fabs(la_lo) > dm_fabs(la_hi) ? dm_fabs(la_lo) : dm_fabs(la_hi);
  if (la_abs > 88.0 || lo_hi - lo_lo > 1.0 || la_hi - la_lo > 1.0) return CEIL_UNBOUNDED;
  const double cl = dm_cos(dm_to_radians(la_abs + 1.0)); // the box's highest latitude after the inflation (checked below: < 1 degree)
  const double chord = dist * w_arc;
  const double metres = dist * (1.0 - dm_cos(0.5 * w_arc)) + chord * chord / radius * (1.0 + 1.0 / cl) + 1.0e-3;
  const double dlat = metres / (radius * (CEIL_PI / 180.0)) * 1.000001, dlon = dlat / cl;
  if (!(dlon < 1.0)) return CEIL_UNBOUNDED;
  la_lo -= dlat, la_hi += dlat, lo_lo -= dlon, lo_hi += dlon;
  int top = 0;
  // the tiles the box can touch: a post of margin is less than a degree (a tile has at least 2 posts per side), so one cell around
  const int ci_lo = sat_i16(dm_floor(la_lo)) - 1, ci_hi = sat_i16(dm_floor(la_hi)) + 1;
  const int cj_lo = sat_i16(dm_floor(lo_lo)) - 1, cj_hi = sat_i16(dm_floor(lo_hi)) + 1;
  for (int ci = ci_lo; ci <= ci_hi; ci++) {
    for (int cj = cj_lo; cj <= cj_hi; cj++) {
      const int ti = ci - tv.lat_min, tj = cj - tv.lon_min;
      if (ti < 0 || tj < 0 || ti >= tv.n_cells_lat || tj >= tv.n_cells_lon) continue;
      const int slot = tv.cell_tile[ti * tv.n_cells_lon + tj];
      if (slot < 0) continue;
      const TileDesc td = tv.tiles[slot];
      if (td.n_lat < 2 || td.n_lon < 2) return CEIL_UNBOUNDED;
      // the box in the tile's index space, one post wider, outwards to whole posts, cut to the tile
      const double fi_lo = dm_floor((la_lo - (double)ci) * (double)(td.n_lat - 1) - 1.0), fi_hi = -dm_floor(-((la_hi - (double)ci) * (double)(td.n_lat - 1) + 1.0));
      const double fj_lo = dm_floor((lo_lo - (double)cj) * (double)(td.n_lon - 1) - 1.0), fj_hi = -dm_floor(-((lo_hi - (double)cj) * (double)(td.n_lon - 1) + 1.0));
      if (fi_hi < 0.0 || fj_hi < 0.0 || fi_lo > (double)(td.n_lat - 1) || fj_lo > (double)(td.n_lon - 1)) continue;
      const int i_lo = fi_lo < 0.0 ? 0 : (int)fi_lo, i_hi = fi_hi > (double)(td.n_lat - 1) ? td.n_lat - 1 : (int)fi_hi;
      const int j_lo = fj_lo < 0.0 ? 0 : (int)fj_lo, j_hi = fj_hi > (double)(td.n_lon - 1) ? td.n_lon - 1 : (int)fj_hi;
      for (int i = i_lo; i <= i_hi; i++) {
        const int16_t* row = tv.posts + td.offset + (int64_t)i * td.n_lon;
        for (int j = j_lo; j <= j_hi; j++) top = row[j] > top ? row[j] : top;
      }
    }
  }
  return (float)(top + 1); // an int16 + 1 is a float exactly
}

// cell[i][j] from the geodesic points of the bin's two edge directions at step i (the caller computes them with the code the march
// runs: coords_at_step): the cover, or the mosaic's top where there is none; never above the top (tv.skip_above is the top + 1 m)
ATMRT_HD float ceiling_cell(const TerrainView& tv, const CeilLayout& L, double radius, double lat0, double lon0, double lat1, double lon1, double dist) {
  const float global = (float)tv.skip_above; // max(highest post, 0) + 1: exact
  const float c = ceiling_cover(tv, radius, lat0, lon0, lat1, lon1, dist, L.w + 2.0e-9);
  return c == CEIL_UNBOUNDED || c > global ? global : c;
}

// An ESTIMATE of the steps a ray of bin `bin` marches, for the order of the whole-frame work queue (Frame::ceil_order): a key
// that decides scheduling, never a result.  The ray's height is the closed form alt + x slope + x^2 / (2 R_eff) over the distance
// table (slope = tan of its elevation angle, R_eff the usual 7/6 earth radius, inv_2r = 1 / (2 R_eff)); the estimate is the first
// step at which it is ascending and above its bin's suffix (it would escape) or below its cell (it would meet terrain soon), else
// march_steps.  This is the test of one step, `ce` the bin's entry of the step's row and x its distance (k_march_length_estimate
// spreads the steps of a ray over lanes).
ATMRT_HD bool ceiling_estimate_ends(const CeilEntry& ce, double x, double alt, double slope, double inv_2r) {
  const double h = alt + x * slope + x * x * inv_2r;
  return (slope + 2.0 * x * inv_2r > 0.0 && h > (double)ce.suffix) || h < (double)ce.cell;
}

} // namespace atmrt
