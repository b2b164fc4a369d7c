// Test-only stand-alone program: the second form of the Spherical geodesic point (atmrt_core.h coords_at_dist_sc, what the marching
// kernels call with sin / cos read from the per-step table) against coords_at_dist and against the arithmetic of
// SphericalCalc::coords_at_dist written out here (directional_calc.rs:72-85), on seeded (DirCalc, dist) pairs.
//   coords_sc_host N  ->  "N pairs, M with the shortcut division, 0 differ"; exit status 1 if any pair differs.
#include "../../atm-raytracer_amd/csrc/atmrt_core.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace atmrt;

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static double uniform() { // splitmix64 -> [0, 1)
  uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z ^= z >> 31;
  return (double)(z >> 11) * 0x1p-53;
}
static bool same(double a, double b) { return memcmp(&a, &b, sizeof a) == 0 || (a != a && b != b); }

int main(int argc, char** argv) {
  const long n = argc > 1 ? atol(argv[1]) : 100000;
  long fast = 0, bad = 0;
  for (long k = 0; k < n; k++) {
    atmrt_earth_model_t m{};
    m.kind = k % 3 == 0 ? ATMRT_EARTH_OBSERVER_AE : ATMRT_EARTH_SPHERICAL; // both take the Spherical calculator
    const int band = (int)(k % 7);
    m.radius = band == 5 ? 1.0e31 * (1.0 + uniform()) : band == 6 ? 1.0e-31 * (1.0 + uniform()) : 1.0e6 + 9.0e6 * uniform();
    Earth e;
    if (earth_resolve(m, e) || e.calc != 2) return 2;
    if (e.calc_radius >= 1.0e-30 && e.calc_radius <= 1.0e30) e.flat_dirs |= EARTH_FAST_DIV, fast++; // as atmrt_set_params sets it
    DirCalc c;
    dircalc_new(e, -90.0 + 180.0 * uniform(), -180.0 + 360.0 * uniform(), 360.0 * uniform(), c);
    // a stepper's distance: a multiple of a step, up to a quarter of the circumference and a little beyond
    const double step = 1.0e-3 + 500.0 * uniform(), dist = k % 11 == 0 ? 0.0 : step * (double)(long)(uniform() * 1.7 * e.calc_radius / step);
    double lat0, lon0, lat1, lon1, s, co;
    coords_at_dist(e, c, dist, lat0, lon0);
    dm_sincos(dist / e.calc_radius, &s, &co); // the host's dm_div is the IEEE division
    coords_at_dist_sc(e, c, s, co, lat1, lon1);
    const double fx = c.pos.x * co + c.dir.x * s, fy = c.pos.y * co + c.dir.y * s, fz = c.pos.z * co + c.dir.z * s;
    const double lat2 = dm_to_degrees(dm_asin(fz)), lon2 = dm_to_degrees(dm_atan2(fy, fx));
    double s2, c2;
    spherical_sincos(e, dist, s2, c2);
    if (!(same(lat0, lat1) && same(lon0, lon1) && same(lat0, lat2) && same(lon0, lon2) && same(s, s2) && same(co, c2))) {
      if (bad++ < 5) printf("pair %ld differs: radius %a dist %a: %a %a / %a %a / %a %a\n", k, e.calc_radius, dist, lat0, lon0, lat1, lon1, lat2, lon2);
    }
  }
  printf("%ld pairs, %ld with the shortcut division, %ld differ\n", n, fast, bad);
  return bad ? 1 : 0;
}
