// Test-only stand-alone program: find_normal with the record of its frame constants (atmrt_core.h NormalTrig, what the trace-point
// epilogue of the kernels reads) against find_normal as the reference has it, restated here from the primitives that stay
// (dircalc_new, coords_at_dist, world_directions, terrain_elev_or_zero): 64-bit patterns must be equal at every point, for all four
// calculators, both families of world_directions, both divisions and two radii.  And spherical_calc_from, the part factored out of
// dircalc_new, against dircalc_new.  Prints "cases C points P helper H failures F"; exit status 1 when F != 0.
#include "../../atm-raytracer_amd/csrc/atmrt_core.h"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace atmrt;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double uniform() { // xorshift64*, 53 bits
  rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
  return (double)((rng_state * 0x2545f4914f6cdd1dull) >> 11) / 9007199254740992.0;
}
static bool same(double a, double b) { return memcmp(&a, &b, 8) == 0; }
static bool same(const Vec3& a, const Vec3& b) { return same(a.x, b.x) && same(a.y, b.y) && same(a.z, b.z); }

// utils.rs:15-40 as atmrt_core.h had it before the record: two calculators, four geodesic points, world_directions
static Vec3 reference_normal(const Earth& e, const TerrainView& tv, double lat, double lon) {
  const double DIFF = 15.0;
  double diff_ns = 0.0, diff_ew = 0.0;
  for (int k = 0; k < 2; k++) {
    DirCalc c;
    dircalc_new(e, lat, lon, k == 0 ? 0.0 : 90.0, c);
    double plat, plon, mlat, mlon;
    coords_at_dist(e, c, DIFF, plat, plon);
    coords_at_dist(e, c, -DIFF, mlat, mlon);
    double d = terrain_elev_or_zero(tv, plat, plon) - terrain_elev_or_zero(tv, mlat, mlon);
    if (k == 0) diff_ns = d;
    else diff_ew = d;
  }
  Vec3 dn, de, du;
  world_directions(e, lat, lon, dn, de, du);
  Vec3 vec_ns = dn * (2.0 * DIFF) + du * diff_ns;
  Vec3 vec_ew = de * (2.0 * DIFF) + du * diff_ew;
  Vec3 normal = cross(vec_ew, vec_ns);
  double len = dm_sqrt(normal.x * normal.x + normal.y * normal.y + normal.z * normal.z);
  return normal / len;
}

// A mosaic of 2 x 2 one-degree cells, one of them without a tile, the three tiles of different sizes, with relief of a few hundred
// metres over a few hundred metres (so that +-15 m changes the height); placed with its south-west corner at (lat_min, lon_min).
struct Mosaic {
  std::vector<int16_t> posts;
  TileDesc tiles[3];
  int32_t cell_tile[4] = {0, 1, -1, 2};
  Mosaic() {
    const int n_lat[3] = {121, 61, 201}, n_lon[3] = {121, 91, 151};
    for (int t = 0; t < 3; t++) {
      tiles[t] = TileDesc{(int64_t)posts.size(), n_lat[t], n_lon[t]};
      for (int i = 0; i < n_lat[t]; i++)
        for (int j = 0; j < n_lon[t]; j++) {
          const double u = (double)i / (n_lat[t] - 1), v = (double)j / (n_lon[t] - 1);
          const unsigned h = (unsigned)(i * 7919 + j * 104729 + t * 13) * 2654435761u;
          posts.push_back((int16_t)(800.0 + 700.0 * u * (1.0 - v) + 300.0 * v * v + (double)(h >> 24) - 128.0 + (t == 1 ? -1500.0 : 0.0)));
        }
    }
  }
  TerrainView view(int lat_min, int lon_min) const { return TerrainView{posts.data(), tiles, cell_tile, lat_min, lon_min, 2, 2, 3000.0}; }
};

int main() {
  const Mosaic mosaic;
  // where the mosaic lies: mid-latitudes; across the equator and the prime meridian; at either pole's last degrees; at either end of
  // the longitudes
  const int place[6][2] = {{46, 8}, {-1, -1}, {88, 20}, {-90, -70}, {10, 178}, {-30, -180}};
  long cases = 0, points = 0, failures = 0, helper = 0;
  for (int pl = 0; pl < 6; pl++) {
    const int la0 = place[pl][0], lo0 = place[pl][1];
    const TerrainView tv = mosaic.view(la0, lo0);
    std::vector<double> lat, lon;
    // the named points (those outside this placement's mosaic read 0 m everywhere: the geodesic part alone)
    const double named_lat[] = {0.0, 89.9, -89.9, 46.5}, named_lon[] = {0.0, 179.999, -179.999, 8.5};
    for (double a : named_lat)
      for (double o : named_lon) lat.push_back(a), lon.push_back(o);
    // the corners of every cell, and points 10 m inside and 10 m outside each edge of the mosaic and of the cell without a tile: a
    // +-15 m neighbour leaves the terrain there and reads 0 m
    const double m = 10.0 / DEGREE_DISTANCE;
    for (int i = 0; i <= 2; i++)
      for (int j = 0; j <= 2; j++) lat.push_back(la0 + i), lon.push_back(lo0 + j);
    for (int i = 0; i <= 2; i++)
      for (double s : {-m, m})
        for (double t : {0.3, 1.0, 1.7}) {
          lat.push_back(la0 + i + s), lon.push_back(lo0 + t);
          lat.push_back(la0 + t), lon.push_back(lo0 + i + s / dm_cos(dm_to_radians((double)la0 + t < 89.0 ? la0 + t : 89.0)));
        }
    // seeded points: most inside the mosaic, some in a margin around it
    const size_t seeded = 1667 + (pl < 4 ? 1 : 0); // 10,000 over the six placements
    for (size_t k = 0; k < seeded; k++) {
      const bool margin = k % 8 == 0;
      double a = margin ? la0 - 0.01 + 2.02 * uniform() : la0 + 2.0 * uniform();
      double o = margin ? lo0 - 0.01 + 2.02 * uniform() : lo0 + 2.0 * uniform();
      if (a > 90.0) a = 90.0;
      if (a < -90.0) a = -90.0;
      lat.push_back(a), lon.push_back(o);
    }
    for (int calc = 0; calc < 4; calc++)
      for (int flat = 0; flat < 2; flat++)
        for (int fast = 0; fast < 2; fast++)
          for (int big = 0; big < 2; big++) {
            Earth e{};
            e.calc = calc;
            e.flat_dirs = (flat ? EARTH_FLAT_DIRS : 0) | (fast ? EARTH_FAST_DIV : 0);
            e.cart = calc == 2 ? 1 : calc == 3 ? 2 : 0;
            e.spherical = calc >= 2;
            e.calc_radius = e.cart_radius = e.shape_radius = big ? EARTH_R * (7.0 / 6.0) : EARTH_R;
            e.a = WGS84_A, e.b = WGS84_B;
            NormalTrig nt;
            normal_trig_fill(e, 46.6, 8.5, nt);
            cases++;
            for (size_t k = 0; k < lat.size(); k++) {
              const Vec3 want = reference_normal(e, tv, lat[k], lon[k]);
              const Vec3 got = find_normal(e, tv, lat[k], lon[k], &nt), plain = find_normal(e, tv, lat[k], lon[k]);
              points++;
              if (!same(got, want) || !same(plain, want)) {
                if (failures++ < 10)
                  printf("mismatch calc %d flat %d fast %d big %d at (%.17g, %.17g): want %.17g %.17g %.17g, record %.17g %.17g %.17g\n", calc, flat,
                         fast, big, lat[k], lon[k], want.x, want.y, want.z, got.x, got.y, got.z);
              }
            }
          }
  }
  // the factored calculator against dircalc_new: azimuths 0 and 90 with the record's sines and cosines, 1,000 seeded ones with dm_sincos
  Earth e{};
  e.calc = 2, e.cart = 1, e.spherical = 1, e.calc_radius = e.cart_radius = e.shape_radius = EARTH_R;
  NormalTrig nt;
  normal_trig_fill(e, 0.0, 0.0, nt);
  for (int k = 0; k < 1002; k++) {
    const double la = -90.0 + 180.0 * uniform(), lo = -180.0 + 360.0 * uniform();
    const double az = k == 0 ? 0.0 : k == 1 ? 90.0 : -360.0 + 1080.0 * uniform();
    DirCalc want, got;
    dircalc_new(e, la, lo, az, want);
    Vec3 dirn, dire, up;
    spherical_directions(la, lo, dirn, dire, up);
    double s, c;
    if (k == 0) s = nt.sin_az0, c = nt.cos_az0;
    else if (k == 1) s = nt.sin_az90, c = nt.cos_az90;
    else dm_sincos(dm_to_radians(az), &s, &c);
    spherical_calc_from(dirn, dire, up, s, c, got);
    helper++;
    if (!same(got.pos, want.pos) || !same(got.dir, want.dir)) {
      if (failures++ < 10) printf("helper mismatch at (%.17g, %.17g) azimuth %.17g\n", la, lo, az);
    }
  }
  // the observer's vectors of the record are spherical_directions of its position
  {
    NormalTrig o;
    normal_trig_fill(e, -33.25, 151.75, o);
    Vec3 dirn, dire, up;
    spherical_directions(-33.25, 151.75, dirn, dire, up);
    if (!same(o.obs_n, dirn) || !same(o.obs_e, dire) || !same(o.obs_up, up) || !(nt.cos_az90 > 6.0e-17 && nt.cos_az90 < 6.2e-17) || nt.sin_az0 != 0.0) failures++;
  }
  printf("cases %ld points %ld helper %ld failures %ld\n", cases, points, helper, failures);
  return failures ? 1 : 0;
}
