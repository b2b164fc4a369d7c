// gen_host.cpp — the reference's `generator::generate` flow (src/generator/mod.rs:47-99, minus renderer and metadata)
// written against the C++ host mirror: Terrain::from_folder -> Params -> make_generator -> generate().
// Usage: gen_host TERRAIN_DIR GENERATOR(Fast|Rectilinear|InterpolatingRectilinear) WIDTH HEIGHT OUT.bin [DEVICES]
// DEVICES: comma-separated HIP device ordinals, e.g. 0,1,2,3,4,5,6,7 — the frame is then cut into pixel-column tiles inside the
// library (a device may be listed twice: "0,0" is two tiles on one GPU); the host code below is the same either way.
// Writes per pixel: azimuth, elevation_angle, n_trace_points, then the first trace point (lat lon distance elevation) or
// four NaNs, as float64 — tests/test_host_cpp.py compares the file with the oracle.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "atmrt_host.hpp"

using namespace atmrt_host;

int main(int argc, char** argv) {
  if (argc != 6 && argc != 7) {
    fprintf(stderr, "usage: %s TERRAIN_DIR GENERATOR WIDTH HEIGHT OUT.bin [DEVICES]\n", argv[0]);
    return 2;
  }
  try {
    std::vector<int> devices;
    if (argc == 7)
      for (const char* p = argv[6]; *p;) {
        devices.push_back((int)strtol(p, const_cast<char**>(&p), 10));
        if (*p == ',') p++;
      }
    Terrain terrain = devices.empty() ? Terrain::from_folder(argv[1]) : Terrain::from_folder(argv[1], devices);
    if (!devices.empty()) printf("%d devices\n", terrain.devices());
    printf("Detected %d terrain files\n", terrain.files()); // terrain/mod.rs:80
    Params params;
    params.position = Position{46.5, 8.5, Altitude{Altitude::Relative, 50.0}};
    params.frame = Frame{0.0, -2.0, 60.0, 60000.0};
    params.model = EarthModel::Spherical(6371000.0);
    params.simulation_step = 100.0;
    params.width = (uint16_t)atoi(argv[3]);
    params.height = (uint16_t)atoi(argv[4]);
    params.generator = !strcmp(argv[2], "Fast") ? GeneratorDef::Fast
                       : !strcmp(argv[2], "Rectilinear") ? GeneratorDef::Rectilinear : GeneratorDef::InterpolatingRectilinear;
    auto generator = make_generator(params, terrain);
    auto result = generator->generate();
    FILE* f = fopen(argv[5], "wb");
    if (!f) return 3;
    size_t hits = 0;
    for (const auto& row : result)
      for (const ResultPixel& px : row) {
        double rec[7] = {px.azimuth, px.elevation_angle, (double)px.trace_points.size(), NAN, NAN, NAN, NAN};
        if (!px.trace_points.empty()) {
          const TracePoint& tp = px.trace_points[0];
          rec[3] = tp.lat; rec[4] = tp.lon; rec[5] = tp.distance; rec[6] = tp.elevation;
          hits++;
        }
        fwrite(rec, sizeof rec, 1, f);
      }
    fclose(f);
    printf("%zux%zu pixels, %zu with a trace point, %llu ray-steps\n", result[0].size(), result.size(), hits,
           (unsigned long long)generator->last_ray_steps);
    if (devices.empty() && hits) { // where in the picture is this place?  (a multi-device context searches gathered planes instead)
      atmrt_landmark_t mark{};
      for (const auto& row : result)
        for (const ResultPixel& px : row)
          if (!px.trace_points.empty()) mark = landmark(px.trace_points[0].lat, px.trace_points[0].lon); // the last pixel that sees ground
      const LocatedLandmarks found = locate_landmarks(terrain, {mark}, 3.0 / 3600.0);
      const atmrt_landmark_hit_t& h = found.hits[0];
      printf("landmark %.6f %.6f: %u trace points within 3 arcseconds, the nearest in pixel (%u, %u) at %.1f m\n", mark.lat, mark.lon, h.n_within,
             h.x, h.y, h.distance);
      if (h.n_within == 0 || h.d2 != 0.0) return 4;
    }
    if (devices.empty()) { // which of the frame's points does a low western light reach?  (needs the frame: before the calls that follow)
      const uint32_t w = params.width, h = params.height;
      const ShadowMask sh = shadow_mask(terrain, atmrt_shadow_spec_t{260.0, 2.0, 20000.0, 0.0}, w, h);
      for (uint32_t y = 0; y < h; y++) {
        printf("shadow row %u ", y);
        for (uint32_t x = 0; x < w; x++) printf("%d:%u%s", sh.status[(size_t)y * w + x], sh.block[(size_t)y * w + x], x + 1 < w ? "," : "\n");
      }
      printf("shadow stats none %llu lit %llu shadowed %llu integrated_steps %llu escaped_rays %llu\n", (unsigned long long)sh.stats.none,
             (unsigned long long)sh.stats.lit, (unsigned long long)sh.stats.shadowed, (unsigned long long)sh.stats.integrated_steps,
             (unsigned long long)sh.stats.escaped_rays);
      // and the image with those shadows under the Shading method lit from the same direction: frame.direction + 180 - light_dir = 260
      const atmrt_params_t pod = params.pod(params.generator);
      atmrt_coloring_t coloring;
      if (atmrt_coloring_from_conf(&pod, ATMRT_COLORING_SHADING, 300.0, 0.3, 88.0, -80.0, ATMRT_PALETTE_IMPROVED, 0, 1.0, &coloring)) return 5;
      const std::vector<uint8_t> lit_image = draw_image_shadowed(terrain, coloring, ShadowMask{std::vector<uint8_t>(sh.status.size(), ATMRT_SHADOW_LIT), {}, {}}, w, h);
      const std::vector<uint8_t> image = draw_image_shadowed(terrain, coloring, sh, w, h);
      size_t darker = 0, other = 0;
      for (size_t p = 0; p < (size_t)w * h; p++) {
        const bool differs = memcmp(&image[3 * p], &lit_image[3 * p], 3) != 0;
        if (differs && sh.status[p] == ATMRT_SHADOW_SHADOWED) darker++;
        else if (differs) other++;
      }
      printf("shadow image darker %zu other %zu\n", darker, other);
      if (other) return 6;
      // the same light and one at 30 degrees in the south-east as world-frame vectors: every point marches in its own local direction
      const atmrt_position_t& at = pod.position;
      const std::vector<std::array<double, 3>> lights = {shadow_light_direction(pod.earth, at.latitude, at.longitude, 260.0, 2.0),
                                                         shadow_light_direction(pod.earth, at.latitude, at.longitude, 135.0, 30.0)};
      const std::pair<double, double> seen = shadow_local_direction(pod.earth, lights[0], at.latitude, at.longitude);
      if (std::fabs(seen.first + 100.0) > 1e-9 || std::fabs(seen.second - 2.0) > 1e-9) return 7; // atan2 returns -100 for 260
      const ShadowLights sl = shadow_lights(terrain, lights, 20000.0, 0.0, w, h, true, true);
      for (uint32_t y = 0; y < h; y++) {
        printf("lights row %u ", y);
        for (uint32_t x = 0; x < w; x++) {
          const size_t p = (size_t)y * w + x, q = (size_t)w * h + p;
          printf("%llu:%d:%u:%d:%u%s", (unsigned long long)sl.lit_mask[p], sl.status[p], sl.block[p], sl.status[q], sl.block[q], x + 1 < w ? "," : "\n");
        }
      }
      printf("lights stats none %llu lit %llu shadowed %llu integrated_steps %llu escaped_rays %llu\n", (unsigned long long)sl.stats.none,
             (unsigned long long)sl.stats.lit, (unsigned long long)sl.stats.shadowed, (unsigned long long)sl.stats.integrated_steps,
             (unsigned long long)sl.stats.escaped_rays);
    }
    if (devices.empty()) { // at which angle does the ground 23.7 km to the east appear, and the top of an 1800 m mast on it?  (no frame needed)
      const std::vector<atmrt_sight_t> sights = sight_lines(terrain, {{90.0, 23700.0, 0.0}, {90.0, 23700.0, 1800.0}}, -6.0, 6.0, 3);
      for (const atmrt_sight_t& s : sights)
        printf("sight status %d rounds %d m %d angle %.17g hidden %.17g ground %.17g resolution %.17g block %d %.17g %.17g\n", s.status, s.rounds_done,
               s.m, s.angle, s.hidden, s.ground, s.resolution, s.block_index, s.block_distance, s.block_elevation);
      // and the same question for the ground along three azimuths as far as 23.7 km: the viewshed, one line per cell of the last sample
      const Viewshed v = viewshed(terrain, atmrt_viewshed_spec_t{88.0, 2.0, 23700.0, 0.0, -6.0, 6.0, 3, 128});
      for (int32_t j = 0; j < v.n_az; j++) {
        const size_t o = (size_t)j * v.m + (v.m - 1);
        printf("viewshed azimuth %d m %d k_star %d status %d hidden %.17g ground %.17g block %d lat %.17g lon %.17g\n", j, v.m, v.k_star[o], v.status[o],
               v.hidden[o], v.ground[o], v.block_index[o], v.lat[o], v.lon[o]);
      }
      // the same viewshed as a raster over a map: four quarter-degree cells east of the observer, binned on the device
      const atmrt_geo_grid_t grid{46.25, 8.5, 0.25, 0.25, 2, 2};
      const ViewshedMap vmap = viewshed_map(terrain, atmrt_viewshed_spec_t{88.0, 2.0, 23700.0, 0.0, -6.0, 6.0, 3, 128}, grid);
      for (uint32_t cell = 0; cell < grid.n_lat * grid.n_lon; cell++)
        printf("viewshed_map cell %u n_samples %u n_seen %u min_hidden %.17g\n", cell, vmap.n_samples[cell], vmap.n_seen[cell], vmap.min_hidden[cell]);
      printf("viewshed_map stats n_samples %llu n_binned %llu n_outside %llu n_skipped %llu n_seen %llu\n", (unsigned long long)vmap.stats.n_samples,
             (unsigned long long)vmap.stats.n_binned, (unsigned long long)vmap.stats.n_outside, (unsigned long long)vmap.stats.n_skipped,
             (unsigned long long)vmap.stats.n_seen);
      // and where the skyline is along the same three azimuths, over the same fan (the same path table), narrowed twice
      const std::vector<atmrt_horizon_t> hz = horizon(terrain, atmrt_horizon_spec_t{88.0, 2.0, 23700.0, -6.0, 6.0, 3, 128, 3});
      for (size_t j = 0; j < hz.size(); j++)
        printf("horizon azimuth %zu status %d rounds %d k_star %d block %d clear %.17g blocked %.17g resolution %.17g distance %.17g lat %.17g lon %.17g "
               "elevation %.17g\n", j, hz[j].status, hz[j].rounds_done, hz[j].k_star, hz[j].block_index, hz[j].angle_clear, hz[j].angle_blocked,
               hz[j].resolution, hz[j].block_distance, hz[j].block_lat, hz[j].block_lon, hz[j].block_elevation);
    }
    if (auto e = terrain.get_elev(46.5, 8.5)) printf("elevation under the observer: %.3f m\n", *e);
  } catch (const Error& e) {
    fprintf(stderr, "ERROR: %s\n", e.what()); // main.rs:36-38
    return 1;
  }
  return 0;
}
