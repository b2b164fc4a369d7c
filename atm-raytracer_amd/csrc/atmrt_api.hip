// atmrt_api.hip — implementation of the C ABI in include/atmrt.h: context, terrain store (own DTED
// parser), frame set-up and the launch sequence of each generator.  The calls that read a finished frame are in
// atmrt_consumers.hip, the harness and debug probes in atmrt_probes.hip.  There is no CPU compute path:
// without a HIP device atmrt_ctx_create fails with ATMRT_ERR_NO_DEVICE.
#include <dirent.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "atmrt_ctx.h"
#include "atmrt_hostmem.h"
#include "atmrt_kernels.h"
#include "atmrt_multi.h"
#include "atmrt_tiff.h"

using namespace atmrt;

namespace {

std::mutex g_err_mutex;
std::string g_create_error = "";

} // namespace

// ---------------------------------------------------------------------------------------------
// DTED (MIL-PRF-89020B) — replaces crate dted 0.2's read_dted / read_dted_header (terrain/mod.rs:24,86)
// ---------------------------------------------------------------------------------------------
namespace {

constexpr long DTED_DATA_OFFSET = 3428; // UHL 80 + DSI 648 + ACC 2700

int parse_uint(const unsigned char* p, int n) {
  int v = 0;
  for (int i = 0; i < n; i++) {
    if (p[i] < '0' || p[i] > '9') return -1;
    v = v * 10 + (p[i] - '0');
  }
  return v;
}

bool parse_angle(const unsigned char* p, double* deg) { // DDDMMSSH
  int d = parse_uint(p, 3), m = parse_uint(p + 3, 2), s = parse_uint(p + 5, 2);
  if (d < 0 || m < 0 || s < 0) return false;
  double v = (double)d + (double)m / 60.0 + (double)s / 3600.0;
  if (p[7] == 'S' || p[7] == 'W') v = -v;
  else if (p[7] != 'N' && p[7] != 'E') return false;
  *deg = v;
  return true;
}

// returns 0, or a negative status with msg filled
int read_dted(const char* path, int* lat0, int* lon0, HostTile* tile, std::string* msg) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    *msg = std::string("cannot open ") + path;
    return ATMRT_ERR_IO;
  }
  unsigned char uhl[80];
  double olat = 0, olon = 0;
  int rc = ATMRT_ERR_FORMAT;
  std::vector<unsigned char> rec;
  do {
    if (fread(uhl, 1, 80, f) != 80 || memcmp(uhl, "UHL1", 4) != 0) break;
    if (!parse_angle(uhl + 4, &olon) || !parse_angle(uhl + 12, &olat)) break;
    int nlon = parse_uint(uhl + 47, 4), nlat = parse_uint(uhl + 51, 4);
    if (nlon < 2 || nlat < 2) break;
    size_t rec_size = 12 + 2 * (size_t)nlat;
    rec.resize(rec_size);
    tile->n_lat = nlat;
    tile->n_lon = nlon;
    tile->posts.assign((size_t)nlat * nlon, 0);
    if (fseek(f, DTED_DATA_OFFSET, SEEK_SET)) break;
    bool ok = true;
    for (int j = 0; j < nlon && ok; j++) {
      if (fread(rec.data(), 1, rec_size, f) != rec_size || rec[0] != 0xAA) {
        ok = false;
        break;
      }
      for (int i = 0; i < nlat; i++) {
        unsigned v = ((unsigned)rec[8 + 2 * i] << 8) | rec[9 + 2 * i];
        int e = (int)(v & 0x7fff);
        if (v & 0x8000) e = -e; // signed magnitude
        tile->posts[(size_t)i * nlon + j] = (int16_t)e;
      }
    }
    if (!ok) break;
    // `f64::from(header.origin_lat) as i16`: truncation (terrain/mod.rs:91-92)
    *lat0 = sat_i16(olat);
    *lon0 = sat_i16(olon);
    rc = 0;
  } while (0);
  fclose(f);
  if (rc) *msg = std::string("Could not buffer terrain file ") + path; // terrain/mod.rs:117
  return rc;
}

} // namespace

// ---------------------------------------------------------------------------------------------
// lifetime
// ---------------------------------------------------------------------------------------------
extern "C" int atmrt_abi_version(void) { return ATMRT_ABI_VERSION; }

#ifndef ATMRT_SOURCE_HASH
#define ATMRT_SOURCE_HASH "unknown"
#endif
#ifndef ATMRT_BUILD_FLAGS
#define ATMRT_BUILD_FLAGS "unknown"
#endif
extern "C" const char* atmrt_build_info(void) { return "source_hash: " ATMRT_SOURCE_HASH "; " ATMRT_BUILD_FLAGS; }

extern "C" size_t atmrt_abi_sizeof(int which) {
  switch (which) {
    case 0: return sizeof(atmrt_params_t);
    case 1: return sizeof(atmrt_atmosphere_t);
    case 2: return sizeof(atmrt_object_t);
    case 3: return sizeof(atmrt_result_t);
    case 4: return sizeof(atmrt_device_planes_t);
    case 5: return sizeof(atmrt_earth_model_t);
    case 6: return sizeof(atmrt_position_t);
    case 7: return sizeof(atmrt_frame_t);
    case 8: return sizeof(atmrt_frame_stats_t);
    case 9: return sizeof(atmrt_timings_t);
    case 10: return sizeof(atmrt_coloring_t);
    case 11: return sizeof(atmrt_device_hits_t);
    case 12: return sizeof(atmrt_comm_timings_t);
    case 13: return sizeof(atmrt_temp_function_t);
    case 14: return sizeof(atmrt_tick_t);
    case 15: return sizeof(atmrt_overlay_t);
    case 16: return sizeof(atmrt_drawn_tick_t);
    // 17 stays 0
    case 18: return sizeof(atmrt_geo_grid_t);
    case 19: return sizeof(atmrt_visibility_stats_t);
    case 20: return sizeof(atmrt_landmark_t);
    case 21: return sizeof(atmrt_landmark_hit_t);
    case 22: return sizeof(atmrt_landmark_stats_t);
    // 23 stays 0
    case 24: return sizeof(atmrt_sight_target_t);
    case 25: return sizeof(atmrt_sight_t);
    case 26: return sizeof(atmrt_sight_ray_t);
    case 28: return sizeof(atmrt_viewshed_spec_t);
    case 30: return sizeof(atmrt_horizon_spec_t);
    case 31: return sizeof(atmrt_horizon_t);
    // 32 stays 0
    case 33: return sizeof(atmrt_viewshed_map_stats_t);
    // 34 stays 0
    case 35: return sizeof(atmrt_shadow_spec_t);
    case 36: return sizeof(atmrt_shadow_stats_t);
    // 37 stays 0
    case 38: return sizeof(atmrt_shadow_lights_spec_t);
    // 39 stays 0
    case 40: return sizeof(atmrt_interp_lattice_t);
    // 41 stays 0
    case 42: return sizeof(atmrt_sky_spec_t);
    case 43: return sizeof(atmrt_sky_ray_t);
    case 44: return sizeof(atmrt_sky_stats_t);
    case 45: return sizeof(atmrt_sky_body_t);
    // 46 stays 0
    case 47: return sizeof(atmrt_sky_table_spec_t);
    // 48 stays 0
    case 49: return sizeof(atmrt_sky_light_spec_t);
    case 50: return sizeof(atmrt_sky_shade_t);
    default: return 0;
  }
}

extern "C" const char* atmrt_last_error(const atmrt_ctx* ctx) {
  if (ctx) return ctx->error.c_str();
  std::lock_guard<std::mutex> lk(g_err_mutex);
  static thread_local std::string copy;
  copy = g_create_error;
  return copy.c_str();
}

static int create_fail(int code, const std::string& msg) {
  std::lock_guard<std::mutex> lk(g_err_mutex);
  g_create_error = msg;
  return code;
}

int atmrt::api_create_fail(int code, const std::string& msg) { return create_fail(code, msg); }

extern "C" int atmrt_ctx_create(atmrt_ctx** out, int device_ordinal) { return api_create_plain(out, device_ordinal); }

int atmrt::api_create_plain(atmrt_ctx** out, int device_ordinal) {
  if (!out) return create_fail(ATMRT_ERR_INVALID_ARGUMENT, "out is NULL");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return create_fail(ATMRT_ERR_NO_DEVICE,
                       std::string("no HIP device available (") + hipGetErrorString(e) +
                           "); this library has no CPU path");
  if (device_ordinal < 0 || device_ordinal >= n)
    return create_fail(ATMRT_ERR_INVALID_ARGUMENT, "device ordinal out of range");
  if ((e = hipSetDevice(device_ordinal)) != hipSuccess)
    return create_fail(ATMRT_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
  atmrt_ctx* c = new atmrt_ctx();
  c->device = device_ordinal;
  if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming)) != hipSuccess ||
      (e = hipEventCreate(&c->ev_t0)) != hipSuccess || (e = hipEventCreate(&c->ev_t1)) != hipSuccess) {
    std::string msg = std::string("stream/event creation: ") + hipGetErrorString(e);
    atmrt_ctx_destroy(c);
    return create_fail(ATMRT_ERR_HIP, msg);
  }
  for (hipEvent_t& ev : c->ev_seg) {
    if ((e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) {
      std::string msg = std::string("hipEventCreate: ") + hipGetErrorString(e);
      atmrt_ctx_destroy(c);
      return create_fail(ATMRT_ERR_HIP, msg);
    }
  }
  for (hipEvent_t& ev : c->ev_scan) {
    if ((e = hipEventCreate(&ev)) != hipSuccess) {
      std::string msg = std::string("hipEventCreate: ") + hipGetErrorString(e);
      atmrt_ctx_destroy(c);
      return create_fail(ATMRT_ERR_HIP, msg);
    }
  }
  for (hipEvent_t& ev : c->ev) {
    if ((e = hipEventCreate(&ev)) != hipSuccess) {
      std::string msg = std::string("hipEventCreate: ") + hipGetErrorString(e);
      atmrt_ctx_destroy(c);
      return create_fail(ATMRT_ERR_HIP, msg);
    }
  }
  atmrt_params_default(&c->params);
  {
    atmrt_atmosphere_t us;
    atmrt_atmosphere_us76(&us);
    c->atm_def.assign(us);
  }
  *out = c;
  return ATMRT_OK;
}

extern "C" void atmrt_ctx_destroy(atmrt_ctx* c) {
  if (!c) return;
  if (c->multi) multi_destroy(c); // the children first, each on its own worker thread
  (void)hipSetDevice(c->device);
  if (c->comm) comm_destroy(c);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->stream2) (void)hipStreamSynchronize(c->stream2);
  for (hipEvent_t ev : c->ev)
    if (ev) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : c->ev_seg)
    if (ev) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : c->ev_scan)
    if (ev) (void)hipEventDestroy(ev);
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->ev_join) (void)hipEventDestroy(c->ev_join);
  if (c->ev_t0) (void)hipEventDestroy(c->ev_t0);
  if (c->ev_t1) (void)hipEventDestroy(c->ev_t1);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  if (c->stream2) (void)hipStreamDestroy(c->stream2);
  delete c; // its DevBufs free themselves, in no particular order: the streams are idle and this device is current
}

// ---------------------------------------------------------------------------------------------
// terrain
// ---------------------------------------------------------------------------------------------
extern "C" int atmrt_terrain_clear(atmrt_ctx* c) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  c->terrain->tiles.clear();
  c->terrain->generation++;
  return ATMRT_OK;
}

extern "C" int atmrt_terrain_add_tile(atmrt_ctx* c, int32_t lat0, int32_t lon0, int32_t n_lat, int32_t n_lon,
                                      const int16_t* posts) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (!posts || n_lat < 2 || n_lon < 2 || n_lat > 65536 || n_lon > 65536)
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "bad tile shape %d x %d", n_lat, n_lon);
  if (lat0 < -90 || lat0 > 89 || lon0 < -360 || lon0 > 359)
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "tile origin (%d, %d) out of range", lat0, lon0);
  HostTile& t = c->terrain->tiles[{lat0, lon0}]; // HashMap::insert replaces (terrain/mod.rs:93-96)
  t.n_lat = n_lat;
  t.n_lon = n_lon;
  t.posts.assign(posts, posts + (size_t)n_lat * n_lon);
  c->terrain->generation++;
  return ATMRT_OK;
}

// Terrain::from_folder, terrain/mod.rs:66-83
extern "C" int atmrt_terrain_load_dir(atmrt_ctx* c, const char* path, int32_t* n_files) {
  if (!c || !path) return ATMRT_ERR_INVALID_ARGUMENT;
  DIR* d = opendir(path);
  if (!d) return c->fail(ATMRT_ERR_IO, "Error opening the terrain data directory %s", path);
  int files = 0;
  while (struct dirent* ent = readdir(d)) {
    if (!strcmp(ent->d_name, ".") || !strcmp(ent->d_name, "..")) continue;
    std::string full = std::string(path) + "/" + ent->d_name;
    HostTile t;
    int lat0, lon0;
    std::string msg;
    int rc = read_dted(full.c_str(), &lat0, &lon0, &t, &msg);
    if (rc == ATMRT_ERR_FORMAT && atmrt_tiff::coords_from_name(ent->d_name, lat0, lon0)) {
      // not DTED, but named like a GeoTIFF tile (terrain/mod.rs:100-118 -> geotiff.rs).  The reference opens such a file lazily and
      // treats a failure as "no elevation here"; so does this loader: an undecodable file leaves its cell empty (0 m).
      std::string why;
      t = HostTile{};
      if (atmrt_tiff::read_dem(full, 3601, t.posts, why)) {
        t.n_lat = t.n_lon = 3601; // geotiff.rs:70-71: a 3600-interval grid per degree, file row = latitude index
        c->terrain->tiles[{lat0, lon0}] = std::move(t);
      } else {
        c->terrain->tiles.erase({lat0, lon0});
      }
      files++;
      continue;
    }
    if (rc) {
      closedir(d);
      c->terrain->generation++; // tiles read before the bad file are in the map: the mosaic must be rebuilt to match it
      return c->fail(rc, "%s", msg.c_str());
    }
    c->terrain->tiles[{lat0, lon0}] = std::move(t);
    files++;
  }
  closedir(d);
  c->terrain->generation++;
  if (n_files) *n_files = files;
  return ATMRT_OK;
}

// Upload the tile mosaic: all posts back to back + a dense (lat, lon) cell -> tile table.
static int upload_terrain(atmrt_ctx* c) {
  const TileStore& store = *c->terrain; // shared by the devices of a multi-device context: read-only while a frame is prepared
  if (c->terrain_uploaded == store.generation) return ATMRT_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  TerrainView tv{};
  if (store.tiles.empty()) {
    tv.lat_min = tv.lon_min = 0;
    tv.n_cells_lat = tv.n_cells_lon = 0;
    tv.skip_above = 1.0; // no tiles: every lookup is 0 m
    c->tv = tv;
    c->terrain_uploaded = store.generation;
    return ATMRT_OK;
  }
  int lat_min = 1 << 30, lat_max = -(1 << 30), lon_min = 1 << 30, lon_max = -(1 << 30);
  size_t total = 0;
  for (auto& kv : store.tiles) {
    lat_min = std::min(lat_min, kv.first.first);
    lat_max = std::max(lat_max, kv.first.first);
    lon_min = std::min(lon_min, kv.first.second);
    lon_max = std::max(lon_max, kv.first.second);
    total += kv.second.posts.size();
  }
  int ncl = lat_max - lat_min + 1, nco = lon_max - lon_min + 1;
  std::vector<int32_t> cells((size_t)ncl * nco, -1);
  std::vector<TileDesc> descs;
  std::vector<int16_t> mosaic;
  mosaic.reserve(total + 8);
  for (auto& kv : store.tiles) {
    TileDesc td;
    td.offset = (int64_t)mosaic.size();
    td.n_lat = kv.second.n_lat;
    td.n_lon = kv.second.n_lon;
    cells[(size_t)(kv.first.first - lat_min) * nco + (kv.first.second - lon_min)] = (int32_t)descs.size();
    descs.push_back(td);
    mosaic.insert(mosaic.end(), kv.second.posts.begin(), kv.second.posts.end());
  }
  HIP_TRY(c, c->d_posts.reserve(mosaic.size() * sizeof(int16_t)));
  HIP_TRY(c, c->d_tiles.reserve(descs.size() * sizeof(TileDesc)));
  HIP_TRY(c, c->d_cells.reserve(cells.size() * sizeof(int32_t)));
  HIP_TRY(c, hipMemcpy(c->d_posts.ptr, mosaic.data(), mosaic.size() * sizeof(int16_t), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(c->d_tiles.ptr, descs.data(), descs.size() * sizeof(TileDesc), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(c->d_cells.ptr, cells.data(), cells.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  tv.posts = c->d_posts.as<int16_t>();
  tv.tiles = c->d_tiles.as<TileDesc>();
  tv.cell_tile = c->d_cells.as<int32_t>();
  tv.lat_min = lat_min;
  tv.lon_min = lon_min;
  tv.n_cells_lat = ncl;
  tv.n_cells_lon = nco;
  int16_t top = 0;
  for (int16_t v : mosaic) top = std::max(top, v);
  tv.skip_above = (double)top + 1.0;
  c->tv = tv;
  c->terrain_uploaded = store.generation;
  return ATMRT_OK;
}

// ---------------------------------------------------------------------------------------------
// configuration
// ---------------------------------------------------------------------------------------------
extern "C" void atmrt_params_default(atmrt_params_t* p) { // Config::default, params.rs:481-494
  memset(p, 0, sizeof *p);
  p->position.latitude = 0.0;
  p->position.longitude = 0.0;
  p->position.altitude_kind = ATMRT_ALT_RELATIVE; // params.rs:42-44
  p->position.altitude = 1.0;
  p->frame.direction = 0.0;
  p->frame.tilt = 0.0;
  p->frame.fov = 30.0;              // params.rs:156-158
  p->frame.max_distance = 150000.0; // params.rs:160-162
  p->earth.kind = ATMRT_EARTH_SPHERICAL;
  p->earth.radius = 6371000.0; // params.rs:467-471
  p->wavelength = 530e-9;      // params.rs:477-479
  p->simulation_step = 50.0;   // params.rs:473-475
  p->terrain_alpha = 1.0;      // params.rs:76-78
  p->straight_rays = 0;
  p->generator = ATMRT_GEN_FAST; // params.rs:427-429
  p->width = 640;                // params.rs:419-425
  p->height = 480;
}

extern "C" void atmrt_atmosphere_us76(atmrt_atmosphere_t* a) {
  static const double alt[7] = {0.0, 11000.0, 20000.0, 32000.0, 47000.0, 51000.0, 71000.0};
  static const double lapse[7] = {-0.0065, 0.0, 0.001, 0.0028, 0.0, -0.0028, -0.002};
  static const struct Table {
    atmrt_temp_function_t fn[7];
    Table() {
      memset(fn, 0, sizeof fn);
      for (int k = 0; k < 7; k++) {
        fn[k].kind = ATMRT_TEMP_LINEAR;
        fn[k].altitude = alt[k];
        fn[k].gradient = lapse[k];
      }
    }
  } table;
  memset(a, 0, sizeof *a);
  a->pressure_altitude = 0.0;
  a->pressure = 101325.0;
  a->temperature_altitude = 0.0;
  a->temperature = 288.15;
  a->has_temperature_fixed_point = 1;
  a->n_functions = 7;
  a->functions = table.fn; // library-owned, immutable
}

// everything an atmosphere definition says, as one byte string (the struct's scalars, its functions, their spline points)
static std::vector<uint8_t> atm_def_image(const atmrt_atmosphere_t& a) {
  std::vector<uint8_t> out;
  auto put = [&](const void* p, size_t n) { out.insert(out.end(), (const uint8_t*)p, (const uint8_t*)p + n); };
  atmrt_atmosphere_t head = a;
  head.functions = nullptr;
  put(&head, sizeof head);
  for (int j = 0; j < a.n_functions && a.functions; j++) {
    atmrt_temp_function_t fn = a.functions[j];
    const double *xs = fn.point_altitude, *ys = fn.point_temperature;
    fn.point_altitude = fn.point_temperature = nullptr;
    put(&fn, sizeof fn);
    if (fn.kind == ATMRT_TEMP_SPLINE && fn.n_points > 0 && xs && ys) {
      put(xs, sizeof(double) * (size_t)fn.n_points);
      put(ys, sizeof(double) * (size_t)fn.n_points);
    }
  }
  return out;
}

extern "C" int atmrt_set_atmosphere(atmrt_ctx* c, const atmrt_atmosphere_t* a) {
  if (!c || !a) return ATMRT_ERR_INVALID_ARGUMENT;
  AtmTableBuf t;
  static const char* why[] = {"", "bad function count or kind", "function altitudes must increase",
                              "no temperature anchor: give temperature_fixed_point or a Spline", "bad spline points"};
  int rc = atm_compile(*a, c->params.wavelength, t);
  if (rc) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "invalid atmosphere definition: %s", why[-rc <= 4 ? -rc : 1]);
  if (!(a->pressure > 0.0)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "the pressure fixed point must be positive");
  // Nothing derived is validated: a profile that runs through 0 K, or whose hydrostatic pressure overflows, is marched like any
  // other (NaN and inf propagate as they do in the reference's f64 arithmetic); such segments get no certificate (atm_certify)
  // and are evaluated with IEEE operations.  Until round 2 they were rejected here.
  if (!c->atm_def_bytes.empty() && c->atm_def_bytes == atm_def_image(*a)) {
    // the same definition again (hosts set it before every frame): the compiled table of the last frame stands
  } else {
    c->atm_def.assign(*a);
    c->atm_def_bytes = atm_def_image(*a);
    c->atm_def_serial++;
  }
  if (c->multi) return multi_forward(c, [a](atmrt_ctx* k) { return atmrt_set_atmosphere(k, a); });
  return ATMRT_OK;
}

extern "C" int atmrt_set_params(atmrt_ctx* c, const atmrt_params_t* p) {
  if (!c || !p) return ATMRT_ERR_INVALID_ARGUMENT;
  Earth e;
  if (earth_resolve(p->earth, e)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "unknown earth model kind %d", p->earth.kind);
  if ((e.calc == 2 && !(e.calc_radius > 0.0)) || (e.calc == 3 && !(e.a > 0.0 && e.b > 0.0)))
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "earth model radius / axes must be positive");
  if (!(p->simulation_step > 0.0) || !std::isfinite(p->simulation_step))
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "simulation_step must be positive");
  if (!(p->frame.max_distance > 0.0) || !std::isfinite(p->frame.max_distance))
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "max_distance must be positive and finite");
  if (p->frame.max_distance / p->simulation_step > 4.0e6)
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "max_distance / simulation_step exceeds 4e6 samples per ray");
  if (p->width == 0 || p->height == 0 || p->width > 32767 || p->height > 32767) // i16 casts, fast.rs:116,122
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "width and height must be in 1..32767");
  if (!(p->col_begin == 0 && p->col_end == 0) && !(p->col_begin < p->col_end && p->col_end <= p->width))
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "column shard [%u, %u) outside width %u", p->col_begin, p->col_end, p->width);
  if (p->generator < 0 || p->generator > 2) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "unknown generator %d", p->generator);
  if (!(p->wavelength > 0.0)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "wavelength must be positive");
  // distances handed to SphericalCalc are sums of steps and interpolation points inside a step: 0 or >= ~1e-17 step
  if (e.calc_radius >= 1.0e-30 && e.calc_radius <= 1.0e30 && p->simulation_step >= 1.0e-10 && p->frame.max_distance <= 1.0e30)
    e.flat_dirs |= EARTH_FAST_DIV;
  if ((c->comm || c->multi) && !(p->col_begin == 0 && p->col_end == 0))
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "col_begin / col_end must be 0 on a context that shares its frame with other ranks or "
                                               "devices: the library assigns the pixel-column tiles itself");
  c->params = *p;
  c->earth = e;
  c->have_params = true;
  if (c->multi) return multi_forward(c, [p](atmrt_ctx* k) { return atmrt_set_params(k, p); });
  return ATMRT_OK;
}

extern "C" int atmrt_objects_set(atmrt_ctx* c, const atmrt_object_t* objects, size_t n) {
  if (!c || (n && !objects)) return ATMRT_ERR_INVALID_ARGUMENT;
  if (n > 1000000) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "too many objects");
  std::vector<ObjectDev> objs(n);
  std::vector<uint8_t> pool;
  for (size_t i = 0; i < n; i++) {
    const atmrt_object_t& s = objects[i];
    ObjectDev& o = objs[i];
    memset(&o, 0, sizeof o);
    if (s.kind != ATMRT_OBJ_FRUSTUM && s.kind != ATMRT_OBJ_BILLBOARD)
      return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "object %zu: unknown kind %d", i, s.kind);
    if (s.position.altitude_kind != ATMRT_ALT_ABSOLUTE && s.position.altitude_kind != ATMRT_ALT_RELATIVE)
      return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "object %zu: unknown altitude kind", i);
    o.kind = s.kind;
    o._pad = s.position.altitude_kind;
    o.lat = s.position.latitude;
    o.lon = s.position.longitude;
    o.elev = s.position.altitude;
    o.r1 = s.r1;
    o.r2 = s.r2;
    o.height = s.height;
    o.width = s.width;
    for (int k = 0; k < 4; k++) o.color[k] = s.color[k];
    if (s.kind == ATMRT_OBJ_BILLBOARD) {
      // Image::get_pixel clamps to (0, w - 2): f64::clamp panics for textures smaller than 2x2 (object/mod.rs:95,100)
      if (!s.texture_rgba || s.texture_width < 2 || s.texture_height < 2 || s.texture_width > 16384 || s.texture_height > 16384)
        return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "object %zu: a billboard needs an RGBA8 texture of at least 2x2", i);
      o.tex_w = (int32_t)s.texture_width;
      o.tex_h = (int32_t)s.texture_height;
      o.tex_offset = (int64_t)pool.size();
      size_t bytes = (size_t)s.texture_width * s.texture_height * 4;
      pool.insert(pool.end(), s.texture_rgba, s.texture_rgba + bytes);
    }
  }
  c->objects.swap(objs);
  c->textures.swap(pool);
  c->objects_serial++;
  if (c->multi) return multi_forward(c, [objects, n](atmrt_ctx* k) { return atmrt_objects_set(k, objects, n); });
  return ATMRT_OK;
}

// ---------------------------------------------------------------------------------------------
// escape certificate
// ---------------------------------------------------------------------------------------------
// The spherical stepper integrates r'' = r + (2 r'^2 n + (r^2 + r'^2) r n') / (r n) in phi.  Where r |n'| / n <= 1/2, r'' >= r / 2 +
// 3 r'^2 / (2 r) > 0 whatever r' is: a ray with r' > 0 stays ascending, and so does every RK4 stage of it (all four stage slopes are
// positive), so the sign test has nothing left to find once it is above the mosaic's top and the objects' bands.  The factor 2 is the
// margin for the central difference of n' (points 1 cm apart), the truncation of RK4 and the rounding of r'.
//
// Upper bound of (R + h) |n'(h)| / n(h) over [u, v], from segment k's closed form (u, v may lie a centimetre outside the segment: the
// stencil of the right-hand side): n - 1 = K pt / Z, pt = p / T and Z Ciddor's compressibility (ciddor_z).  pt and its derivative are
// monotone on a Linear or isothermal segment, and bounded through the coefficients on a Spline knot interval.  Where the temperature
// of a Linear segment is <= 0 the evaluations are NaN (dm_pow of a negative base) and a ray that gets there never crosses anything
// again: no constraint.  +inf: no bound.
static double escape_piece_bound(const AtmTable& t, int k, double u, double v, double radius) {
  const AtmSeg& s = t.seg(k);
  const double a0 = 1.58123e-6, a1 = 2.9331e-8, a2 = 1.1043e-10, zd = 1.83e-11; // |coefficients| of ciddor_z
  double pt_max, dpt_max, t_lo, t_hi, dt_max;
  if (s.cubic) {
    const double du = u - s.hb, dv = v - s.hb, m = std::max(std::fabs(du), std::fabs(dv));
    dt_max = std::fabs(s.lapse) + 2.0 * std::fabs(s.c2) * m + 3.0 * std::fabs(s.c3) * m * m;
    const double tu = seg_temperature(s.tb, s.lapse, s.c2, s.c3, du);
    t_lo = tu - dt_max * (v - u);
    t_hi = tu + dt_max * (v - u);
    if (!(t_lo > 1.0) || !(s.expo < 0.0)) return INFINITY;
    // p decreases with h (expo < 0, T > 0): its largest value is at u
    const double p_max = s.pb * seg_pressure_ratio(1, s.hb, s.tb, s.gtb, s.lapse, s.c2, s.c3, s.expo, u) * (1.0 + 1.0e-9);
    pt_max = p_max / t_lo;
    dpt_max = pt_max * (std::fabs(s.expo) + dt_max) / t_lo; // d(p/T)/dh = (p/T) (expo - T') / T
  } else if (s.lapse != 0.0) {
    const double xu = std::fma(s.gtb, u - s.hb, 1.0), xv = std::fma(s.gtb, v - s.hb, 1.0);
    double x_lo = std::min(xu, xv), x_hi = std::max(xu, xv);
    if (!(x_hi > 0.0)) return s.expo1 > 1.0 ? 0.0 : INFINITY; // T <= 0 throughout: NaN
    if (!(x_lo > 0.0)) {
      if (!(s.expo1 > 1.0)) return INFINITY; // pt' = ptb expo1 gtb x^(expo1 - 1) unbounded as T -> 0
      x_lo = 0.0;
    }
    // pt = ptb x^expo1, |pt'| = ptb |expo1 gtb| x^(expo1 - 1): both monotone in x
    pt_max = std::max(s.ptb * std::pow(x_lo, s.expo1), s.ptb * std::pow(x_hi, s.expo1));
    const double g = s.ptb * std::fabs(s.expo1 * s.gtb);
    dpt_max = std::max(g * std::pow(x_lo, s.expo1 - 1.0), g * std::pow(x_hi, s.expo1 - 1.0));
    t_lo = s.tb * x_lo;
    t_hi = s.tb * x_hi;
    dt_max = std::fabs(s.lapse);
  } else { // isothermal: pt = ptb exp(expo1 (h - hb))
    pt_max = std::max(s.ptb * std::exp(s.expo1 * (u - s.hb)), s.ptb * std::exp(s.expo1 * (v - s.hb)));
    dpt_max = std::fabs(s.expo1) * pt_max;
    t_lo = t_hi = s.tb;
    dt_max = 0.0;
  }
  pt_max *= 1.0 + 1.0e-9;
  dpt_max *= 1.0 + 1.0e-9;
  const double ta = std::max(std::fabs(t_lo - 273.15), std::fabs(t_hi - 273.15));
  const double a_max = a0 + a1 * ta + a2 * ta * ta;
  const double z_min = 1.0 - pt_max * a_max;
  if (!(z_min >= 0.5)) return INFINITY;
  // Z' = -pt' A - pt A'(t) T' + 2 pt pt' d;  n' = K (pt' / Z - pt Z' / Z^2);  n >= 1
  const double dz_max = dpt_max * (a_max + 2.0 * pt_max * zd) + pt_max * (a1 + 2.0 * a2 * ta) * dt_max;
  double dn_max = std::fabs(t.k_refr) * (dpt_max / z_min + pt_max * dz_max / (z_min * z_min));
  // What the stepper differences is the computed n: on a Linear segment pt = ptb x^(expo1) carries the rounding of x (2^-53) times
  // |expo1| (3e7 for a gradient of 1e-9 K/m) besides pow's own, and the central difference divides two such errors by 2 cm
  if (!s.cubic && s.lapse != 0.0) dn_max += 100.0 * std::fabs(t.k_refr) * pt_max / z_min * (std::fabs(s.expo1) + 4.0) * 0x1p-52;
  const double b = (radius + std::max(std::fabs(u), std::fabs(v))) * dn_max * (1.0 + 1.0e-6);
  return b >= 0.0 ? b : INFINITY;
}

constexpr double ESCAPE_BOUND = 0.5;
// The lowest altitude `from` >= lo such that (R + h) |n'| / n <= ESCAPE_BOUND for every h >= from, or +inf; *worst: the largest bound
// above `from`.  Sweeps every segment's part of [lo, 1e7 m) in pieces of 50 m growing by 2 % of the height above the segment's lower
// boundary (above 0 m in the first segment); a jump of n at a
// segment boundary enters the central difference of a stencil across it as 50 |jump|.  Above 1e7 m the last segment must make the
// bound decreasing: isothermal with expo1 (R + h) <= -1, Linear warming with expo1 < -1, or Linear cooling to T = 0 below 1e7 m.
static double escape_certified_from(const AtmTable& t, double radius, double lo, double* worst) {
  constexpr double H_END = 1.0e7, EPS = 0.01;
  double from = lo, w = 0.0;
  std::vector<double> pieces; // (top, bound) of every piece, bottom up
  auto jump = [&](int k) { // |n| jump at the lower boundary of segment k >= 1, + the rounding of the two values
    const double h = t.seg(k).from;
    const double d = std::fabs(refr_n_layer<true, false>(t.k_refr, t.seg(k), h) - refr_n_layer<true, false>(t.k_refr, t.seg(k - 1), h));
    return (d == d ? d : INFINITY) + 1.0e-15;
  };
  for (int k = 0; k < t.n; k++) {
    const double s_lo = k > 0 ? t.seg(k).from : -INFINITY, s_hi = k + 1 < t.n ? t.seg(k + 1).from : INFINITY;
    const double a = std::max(s_lo, lo - 2.0 * EPS), b = std::min(s_hi, H_END);
    // the pieces are a lattice of the segment, not of `lo` (anchored at its lower boundary; the first segment's at 0 m, in 50 m pieces
    // below), and a piece that reaches above `lo` counts whole: a higher `lo` sees a subset of the same pieces, so the floor never
    // comes down when the mosaic's top goes up
    const double anchor = k > 0 ? s_lo : 0.0;
    double u = anchor;
    if (k == 0 && a < 0.0) u = a > -1.0e6 ? -50.0 * std::ceil(-a / 50.0) : a;
    while (u < b) {
      const double v = std::min(b, u + 50.0 + 0.02 * std::max(u - anchor, 0.0));
      if (v > a) {
        double bound = escape_piece_bound(t, k, u - EPS, v + EPS, radius);
        if (k > 0 && u == s_lo) bound += (radius + u + EPS) * 50.0 * jump(k);
        if (k + 1 < t.n && v == s_hi) bound += (radius + v + EPS) * 50.0 * jump(k + 1);
        pieces.push_back(v);
        pieces.push_back(bound);
      }
      u = v;
    }
    if (k + 1 == t.n) { // the tail above H_END
      const AtmSeg& s = t.seg(k);
      bool ok;
      if (s.cubic) ok = false;
      else if (s.lapse == 0.0) ok = s.expo1 * (radius + std::max(a, H_END)) <= -1.0;
      else if (s.gtb > 0.0) ok = s.expo1 < -1.0;
      else ok = s.gtb < 0.0 && s.hb - 1.0 / s.gtb < H_END && s.expo1 > 1.0;
      pieces.push_back(INFINITY);
      pieces.push_back(ok ? 0.0 : INFINITY);
    }
  }
  for (size_t q = 0; q < pieces.size(); q += 2)
    if (!(pieces[q + 1] <= ESCAPE_BOUND)) from = pieces[q] + 2.0 * EPS; // a stencil centred here no longer reaches into the refused piece
  for (size_t q = 0; q < pieces.size(); q += 2)
    if (pieces[q] > from && pieces[q + 1] > w) w = pieces[q + 1];
  if (worst) *worst = w;
  return from;
}

// What the march gets: the floor above which an ascending ray may leave (Frame::esc_floor), +inf for none.  `top`: the mosaic's
// skip_above (every post is below it; lookups outside the mosaic are 0 m, and it is at least 1 m).
static double escape_floor(const AtmTable& t, bool spherical, double radius, bool straight, double top, double step, double* from_out,
                           double* worst) {
  if (worst) *worst = 0.0;
  if (from_out) *from_out = top - step;
  if (straight) return top;        // h(x) is linear (flat) or convex (spherical, while the ray's angle stays below 90 degrees)
  if (!spherical) return INFINITY; // flat earth, refracted: n' < 0 bends every ray down
  const double from = escape_certified_from(t, radius, top - step, worst);
  if (from_out) *from_out = from;
  return std::max(top, from + step); // the stages of a step reach no lower than its start; one step of margin below that
}

static bool escape_enabled() { return !env_off("ATMRT_ESCAPE"); }
// ATMRT_STEP_TRIG=off: no table of the geodesic's sin / cos (Frame::xs_sin), every sample computes them (A/B runs, tests/test_gpu_step_trig.py)
static bool step_trig_enabled() { return !env_off("ATMRT_STEP_TRIG"); }
// ATMRT_NORMAL_TRIG=off: no record of the epilogue's frame constants (Frame::normal_trig), every trace point computes them (A/B runs,
// tests/test_gpu_normal_trig.py).  Read at every frame.
static bool normal_trig_enabled() { return !env_off("ATMRT_NORMAL_TRIG"); }

// ATMRT_CEILING=off: no terrain ceiling table (Frame::ceil), the march runs on the mosaic's top alone; =rebuild: the table is built
// again in every frame, as for an observer that moves from frame to frame (A/B runs, tests/test_gpu_ceiling.py).  Read at every frame.
static int ceiling_mode() {
  const char* e = getenv("ATMRT_CEILING");
  return !e ? 1 : !strcmp(e, "off") ? 0 : !strcmp(e, "rebuild") ? 2 : 1;
}

// Frame::ceil for `f` (complete but for the three ceiling fields): the cached table, or a new one built on the frame's stream
static int prepare_ceiling(atmrt_ctx* c, Frame& f) {
  c->ceil_built = false; // for the frames that return before the table's refresh
  f.ceil = nullptr;
  f.ceil_layout = CeilLayout{};
  f.ceil_floor = INFINITY;
  f.ceil_order = f.ceil_order_steps = nullptr;
  const int mode = ceiling_mode();
  const atmrt_params_t& p = f.p;
  if (!mode || p.generator != ATMRT_GEN_RECTILINEAR || c->earth.calc != 2 || f.march_steps < 1 || f.wl < 1 || f.h < 1) return ATMRT_OK;
  (void)c->bins.refresh({bits(p.frame.direction), bits(p.frame.fov), bits(p.frame.tilt), (int32_t)p.width, (int32_t)p.height, f.c0, f.wl}, [&](CeilLayout& l) {
    l = ceiling_layout(p, f.ph, f.c0, f.wl, f.h);
    return 0;
  });
  f.ceil_layout = c->bins.value();
  const CeilKey key{c->terrain_uploaded, c->steps.serial(), bits(p.position.latitude), bits(p.position.longitude), key_of(c->earth), key_of(f.ceil_layout), f.xs_sin ? 1 : 0};
  const int rc = c->ceiling.refresh(key, [&](Nothing&) {
    HIP_TRY(c, c->d_ceil.reserve(((size_t)f.march_steps + 1) * (size_t)(f.ceil_layout.n_bins + 1) * sizeof(CeilEntry)));
    HIP_TRY(c, hipEventRecord(c->ev[EV_CEIL_BEGIN], c->stream));
    launch_ceiling(f, c->d_ceil.as<CeilEntry>(), c->stream);
    HIP_TRY(c, hipGetLastError());
    return 0;
  }, mode == 2, &c->ceil_built);
  if (rc) return rc;
  f.ceil = c->d_ceil.as<CeilEntry>();
  // The work queue of the whole-frame march, beside the table: built whenever the table is, and when what the table does not depend
  // on changes the rays (the image's rows and the observer's altitude; the bins' key holds the rest of the camera).  Its time is the
  // table's (EV_CEIL_BEGIN .. EV_CEIL_END, ceiling_ms).
  bool order_built = false;
  if (frame_march_plan(f, c->comm != nullptr).route == MarchRoute::Queue) {
    const OrderKey okey{c->ceiling.serial(), c->bins.serial(), f.h, p.position.altitude_kind, bits(p.position.altitude)};
    MarchOrder o{};
    const int orc = c->ceil_order.refresh(okey, [&](Nothing&) {
      HIP_TRY(c, reserve_carved(c->d_ceil_order, [&](Carve& k) { march_order_layout(f, k, o); }));
      if (!c->ceil_built) HIP_TRY(c, hipEventRecord(c->ev[EV_CEIL_BEGIN], c->stream));
      launch_march_order(f, o, c->stream);
      HIP_TRY(c, hipGetLastError());
      return 0;
    }, mode == 2, &order_built);
    if (orc) return orc;
    Carve carved(c->d_ceil_order.ptr); // the order's key holds what the layout depends on: the same carving as the build's
    march_order_layout(f, carved, o);
    f.ceil_order = o.order, f.ceil_order_steps = o.order_steps;
  }
  if (c->ceil_built || order_built) HIP_TRY(c, hipEventRecord(c->ev[EV_CEIL_END], c->stream));
  c->ceil_built = c->ceil_built || order_built;
  // the certificate's part of the escape floor (Frame::esc_floor is the same rule over the mosaic's top)
  if (escape_enabled()) {
    if (p.straight_rays) f.ceil_floor = -INFINITY;
    else if (c->earth.spherical) f.ceil_floor = c->atm.value().ceil_from + p.simulation_step;
  }
  return ATMRT_OK;
}

extern "C" int atmrt_escape_certificate(const atmrt_atmosphere_t* atmosphere, double wavelength, int32_t spherical, double radius,
                                        int32_t straight, double simulation_step, double top, double out[3]) {
  if (!atmosphere || !out) return ATMRT_ERR_INVALID_ARGUMENT;
  AtmTableBuf buf;
  if (atm_compile(*atmosphere, wavelength, buf)) return ATMRT_ERR_INVALID_ARGUMENT;
  double from = 0.0, worst = 0.0;
  out[0] = escape_floor(buf.table(), spherical != 0, radius, straight != 0, top, simulation_step, &from, &worst);
  out[1] = from;
  out[2] = worst;
  return ATMRT_OK;
}

// ---------------------------------------------------------------------------------------------
// frame set-up
// ---------------------------------------------------------------------------------------------
// The products a frame is set up from (atmrt_ctx.h), one function each; prepare_frame refreshes sources before their dependents.
// The distance table by repeated addition, exactly like `distance += step` (utils.rs:191-196) and the stepper's x;
// n_t = #{k: xs[k] < max}; the path cache gets one element more than the first k whose PREVIOUS x exceeds max (utils.rs:160-170)
static int refresh_steps(atmrt_ctx* c, const atmrt_params_t& p) {
  return c->steps.refresh({bits(p.simulation_step), bits(p.frame.max_distance)}, [&](Steps& t) {
    t.xs.clear();
    t.n_t = 0;
    for (double d = 0.0;; d += p.simulation_step) {
      t.xs.push_back(d);
      if (d < p.frame.max_distance) t.n_t++;
      const size_t k = t.xs.size() - 1; // index of d
      if (k >= 1 && t.xs[k - 1] > p.frame.max_distance) break;
      if (t.xs.size() > 5000000) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "distance table too long");
    }
    t.march_steps = 0;
    for (size_t k = 1; k < t.xs.size(); k++) // the march's own rule: step k is taken while x_k <= max_distance (rectilinear.rs:178)
      if (t.xs[k] <= p.frame.max_distance) t.march_steps = (int)k;
      else break;
    t.n_path_cap = (int)t.xs.size();
    HIP_TRY(c, c->d_xs.reserve(t.xs.size() * sizeof(double)));
    HIP_TRY(c, hipMemcpy(c->d_xs.ptr, t.xs.data(), t.xs.size() * sizeof(double), hipMemcpyHostToDevice));
    return 0;
  });
}

// The Spherical calculator's sin / cos of xs[k] / calc_radius, by the device code the samples would run (k_step_trig): like xs they
// depend on nothing of the ray or the observer and survive the frame.  The kernels of this frame follow on the same stream.
static int refresh_trig(atmrt_ctx* c) {
  const size_t n = (size_t)c->steps.value().march_steps + 1;
  return c->trig.refresh({c->steps.serial(), bits(c->earth.calc_radius), c->earth.flat_dirs & EARTH_FAST_DIV}, [&](Nothing&) {
    HIP_TRY(c, c->d_xs_trig.reserve(2 * n * sizeof(double)));
    launch_step_trig(c->earth, n, c->d_xs.as<double>(), c->d_xs_trig.as<double>(), c->d_xs_trig.as<double>() + n, c->stream);
    HIP_TRY(c, hipGetLastError());
    return 0;
  });
}

// The Spherical calculator's constants of the trace-point epilogue, by the device code a lane would run (k_normal_trig): the earth
// model is the same from call to call, the observer's position changes when the observer moves.  The kernels of this frame follow on
// the same stream.
static int refresh_normal_trig(atmrt_ctx* c, const atmrt_params_t& p) {
  return c->normal_trig.refresh({bits(c->earth.calc_radius), c->earth.flat_dirs & EARTH_FAST_DIV, bits(p.position.latitude), bits(p.position.longitude)}, [&](Nothing&) {
    HIP_TRY(c, c->d_normal_trig.reserve(sizeof(NormalTrig)));
    launch_normal_trig(c->earth, p.position.latitude, p.position.longitude, c->d_normal_trig.as<NormalTrig>(), c->stream);
    HIP_TRY(c, hipGetLastError());
    return 0;
  });
}

// The compiled table and its certificates: hosts set the same atmosphere before every frame (the Python mirror does), and the
// certificate's bisections are a quarter of a millisecond of host time — a twentieth of a Fast frame.
static int refresh_atm(atmrt_ctx* c, const atmrt_params_t& p) {
  return c->atm.refresh({c->atm_def_serial, bits(p.wavelength), bits(p.simulation_step), bits(c->earth.shape_radius), c->earth.spherical}, [&](Atm& a) {
    if (atm_compile(c->atm_def.pod, p.wavelength, a.table)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "invalid atmosphere");
    AtmTable& t = a.table.table();
    atm_certify(t, c->earth.spherical != 0, c->earth.shape_radius, p.simulation_step);
    if (getenv("ATMRT_NO_TIGHT")) // experiments: the voting path of dm_div3 on every segment (same bits, tests/test_gpu_march_variants.py)
      for (int k = 0; k < t.n; k++) {
        t.seg(k).flags &= ~ATM_SEG_TIGHT;
        t.seg(k).tight_lo = INFINITY, t.seg(k).tight_hi = -INFINITY;
      }
    // the escape certificate from the lowest value an entry of the terrain ceiling table can have (1 m) minus a step
    a.ceil_from = escape_certified_from(t, c->earth.shape_radius, 1.0 - p.simulation_step, nullptr);
    HIP_TRY(c, c->d_atm.reserve(a.table.bytes()));
    HIP_TRY(c, hipMemcpy(c->d_atm.ptr, &t, a.table.bytes(), hipMemcpyHostToDevice));
    return 0;
  });
}

// the escape certificate of the compiled table for the mosaic's top
static int refresh_escape(atmrt_ctx* c, const atmrt_params_t& p) {
  return c->escape.refresh({c->atm.serial(), bits(c->tv.skip_above)}, [&](Escape& e) {
    (void)escape_floor(c->atm.value().table.table(), true, c->earth.shape_radius, false, c->tv.skip_above, p.simulation_step, &e.from, &e.bound);
    return 0;
  });
}

// The scene: k_resolve rewrites the object table every frame (Altitude::abs depends on the terrain), the textures change with atmrt_objects_set
static int upload_objects(atmrt_ctx* c) {
  if (c->objects.empty()) return ATMRT_OK;
  HIP_TRY(c, c->d_objects.reserve(c->objects.size() * sizeof(ObjectDev)));
  HIP_TRY(c, hipMemcpy(c->d_objects.ptr, c->objects.data(), c->objects.size() * sizeof(ObjectDev), hipMemcpyHostToDevice));
  return c->textures_dev.refresh(c->objects_serial, [&](Nothing&) {
    if (c->textures.empty()) return 0;
    HIP_TRY(c, c->d_textures.reserve(c->textures.size()));
    HIP_TRY(c, hipMemcpy(c->d_textures.ptr, c->textures.data(), c->textures.size(), hipMemcpyHostToDevice));
    return 0;
  });
}

int atmrt::prepare_frame(atmrt_ctx* c, Frame* out) {
  if (!c->have_params) return c->fail(ATMRT_ERR_STATE, "atmrt_set_params has not been called");
  HIP_TRY(c, hipSetDevice(c->device));
  int rc = upload_terrain(c);
  if (rc) return rc;
  const atmrt_params_t& p = c->params;
  const bool trig = c->earth.calc == 2 && step_trig_enabled(); // off: a table of an earlier frame stays as it is
  const bool ntrig = c->earth.calc == 2 && normal_trig_enabled(); // off: a record of an earlier frame stays as it is
  if ((rc = refresh_steps(c, p)) || (trig && (rc = refresh_trig(c))) || (ntrig && (rc = refresh_normal_trig(c, p))) || (rc = refresh_atm(c, p)) || (rc = refresh_escape(c, p)) || (rc = upload_objects(c))) return rc;
  const Steps& steps = c->steps.value();
  Frame f{};
  f.p = p;
  f.earth = c->earth;
  f.inv_shape_radius = c->earth.spherical && c->earth.shape_radius != 0.0 ? 1.0 / c->earth.shape_radius : 0.0;
  f.atm = c->d_atm.as<AtmTable>();
  pinhole_init(p, f.ph);
  f.tv = c->tv;
  HIP_TRY(c, c->d_alt.reserve(sizeof(double)));
  f.alt = c->d_alt.as<double>();
  f.xs = c->d_xs.as<double>();
  f.xs_sin = trig ? c->d_xs_trig.as<double>() : nullptr;
  f.xs_cos = trig ? c->d_xs_trig.as<double>() + steps.march_steps + 1 : nullptr;
  f.normal_trig = ntrig ? c->d_normal_trig.as<NormalTrig>() : nullptr;
  f.objects = c->objects.empty() ? nullptr : c->d_objects.as<ObjectDev>();
  f.textures = c->d_textures.as<uint8_t>();
  f.n_objects = (int32_t)c->objects.size();
  f.n_t = steps.n_t;
  f.n_path_cap = steps.n_path_cap;
  f.march_steps = steps.march_steps;
  f.esc_floor = INFINITY;
  f.esc_ang_max = INFINITY;
  if (escape_enabled() && p.generator == ATMRT_GEN_RECTILINEAR) {
    if (p.straight_rays) {
      f.esc_floor = c->tv.skip_above;
      // spherical: h = r0 cos(ang) / cos(ang + x / R) - R is convex while ang + x / R stays below 90 degrees (then it turns negative
      // and the reference stops the ray at -1000 m): with 0.05 rad of margin for the rounding of the angle
      if (c->earth.spherical) f.esc_ang_max = 1.5207963267948966 - p.frame.max_distance * f.inv_shape_radius;
    } else if (c->earth.spherical) {
      f.esc_floor = std::max(c->tv.skip_above, c->escape.value().from + p.simulation_step);
    }
  }
  {
    int c0 = (p.col_begin == 0 && p.col_end == 0) ? 0 : p.col_begin;
    int c1 = (p.col_begin == 0 && p.col_end == 0) ? p.width : p.col_end;
    if (c->comm) comm_columns(c, p.width, &c0, &c1); // a rank / device of a shared frame: the library's own pixel-column tile
    if (c1 <= c0) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "image width %u leaves this rank without a pixel column", p.width);
    f.c0 = c0;
    f.wl = c1 - c0;
  }
  f.h = p.height;
  f.opaque = (p.terrain_alpha == 1.0 && c->objects.empty()) ? 1 : 0;
  f.lattice = 0;
  f.atm_cubic = atm_has_cubic(c->atm.value().table.table()) ? 1 : 0;
  f.di0 = f.ei0 = 0;
  f.dir_step = f.elev_step = 0.0;
  rc = prepare_ceiling(c, f);
  if (rc) return rc;
  *out = f;
  return ATMRT_OK;
}

// The scratch of frame `f`: the context's workspace allocation grown to workspace_layout(f) and carved by it, and the three arrays
// that outlive it (atmrt_ctx.h).  The allocation moves when it grows, so the rule is: NOTHING OF THIS FRAME IS LIVE IN IT WHEN IT IS
// RESERVED.  Every call comes before the frame's first launch, but for the one in interp_blend_tail: it prepares the frame
// that the entry point prepared already, so it cannot grow the allocation, and what the blend still needs of the lattice pass lies
// in buffers of its own.  No pointer into the allocation is kept in the context across frames.
static int prepare_workspace(atmrt_ctx* c, const Frame& f, Workspace* ws) {
  *ws = Workspace{};
  ws->march = frame_march_plan(f, c->comm != nullptr);
  if (f.p.generator == ATMRT_GEN_RECTILINEAR && !f.opaque) { // the counting passes' trace points beyond the slots
    static const long forced_cap = [] { // test hook: a tiny arena forces the second-pass route (tests/test_gpu_march_variants.py)
      const char* e = getenv("ATMRT_OVERFLOW_CAP");
      return e ? atol(e) : -1L;
    }();
    ws->overflow_cap = forced_cap >= 0 ? (size_t)forced_cap : std::max<size_t>(65536, (size_t)f.wl * f.h / 4);
  }
  HIP_TRY(c, reserve_carved(c->d_workspace, [&](Carve& k) { workspace_layout(f, k, *ws); }));
  HIP_TRY(c, reserve_into(c->d_alt, ws->alt, 1));
  HIP_TRY(c, reserve_into(c->d_hit_offset, ws->hit_offset, (size_t)f.wl * f.h));
  HIP_TRY(c, reserve_into(c->d_counters, ws->counters, N_COUNTERS));
  return ATMRT_OK;
}

// The frame's counter block on the host, after everything enqueued on `s` so far.
static hipError_t read_counters(const Workspace& ws, hipStream_t s, uint64_t (&cnt)[N_COUNTERS]) {
  const hipError_t e = hipMemcpyAsync(cnt, ws.counters, sizeof cnt, hipMemcpyDeviceToHost, s);
  return e == hipSuccess ? hipStreamSynchronize(s) : e;
}

// One frame of the Fast or Rectilinear generator into `dense` (device memory).  When `want_packed` (or whenever
// a pixel can hold several trace points) the packed trace points are left in c->d_packed and their offsets in
// ws.hit_offset.  Counters are NOT reset here.
static int run_core(atmrt_ctx* c, const Frame& f, Workspace& ws, const DensePlanes& dense, bool want_packed,
                    PackedHits* packed_out, uint64_t* n_hits_out) {
  hipStream_t s = c->stream;
  launch_resolve(f, ws, c->d_objects.as<ObjectDev>(), s);
  hipEvent_t* ev = c->ev;
  const bool fast = f.p.generator == ATMRT_GEN_FAST;
  const bool general = f.n_objects > 0; // scenes with objects: full get_single_pixel, count -> scan -> fill
  if (fast && general) {
    launch_fast_caches(f, ws, s, c->stream2, c->ev_fork, c->ev_join, ev);
    launch_close_count(f, ws, s);
    uint64_t cnt[N_COUNTERS];
    HIP_TRY(c, read_counters(ws, s, cnt));
    HIP_TRY(c, reserve_into(c->d_clist, ws.clist, cnt[CTR_CLOSE_TOTAL] + 1));
    launch_close_fill(f, ws, s);
    HIP_TRY(c, hipEventRecord(ev[EV_MARCH_BEGIN], s));
    launch_trace_count(f, ws, dense, s);
    HIP_TRY(c, hipEventRecord(ev[EV_MARCH_END], s));
    HIP_TRY(c, hipEventRecord(ev[EV_FINALIZE_END], s));
  } else if (general) {
    // Rectilinear with scene objects: the lean march first (it leaves the rays that can meet an object to the general tracer and
    // lists them), then the tracer over that list
    HIP_TRY(c, hipEventRecord(ev[EV_MARCH_BEGIN], s));
    c->last.march_route = launch_rect_trace_count(f, ws, dense, s);
    uint64_t cnt[N_COUNTERS];
    HIP_TRY(c, read_counters(ws, s, cnt));
    launch_rect_trace_objects(f, ws, dense, cnt[CTR_OBJECT_RAYS], s);
    HIP_TRY(c, hipEventRecord(ev[EV_MARCH_END], s));
    HIP_TRY(c, hipEventRecord(ev[EV_FINALIZE_END], s));
  } else if (fast) {
    c->scan_segments = launch_fast_pipeline(f, ws, dense, s, c->stream2, c->ev_fork, c->ev_seg, c->ev_scan, ev); // records EV_PROFILE_BEGIN .. EV_MARCH_BEGIN
    HIP_TRY(c, hipEventRecord(ev[EV_MARCH_END], s));
    if (f.opaque) launch_fast_finalize(f, ws, dense, s);
    HIP_TRY(c, hipEventRecord(ev[EV_FINALIZE_END], s));
  } else {
    HIP_TRY(c, hipEventRecord(ev[EV_MARCH_BEGIN], s));
    c->last.march_route = launch_rect_march(f, ws, dense, s, ev[EV_MARCH_END]);
    HIP_TRY(c, hipEventRecord(ev[EV_FINALIZE_END], s));
  }
  HIP_TRY(c, hipEventRecord(ev[EV_PACK_BEGIN], s));
  PackedHits packed{};
  if (want_packed || !f.opaque) {
    uint64_t counters[N_COUNTERS];
    launch_scan_counts(f, ws, dense.hit_count, s);
    HIP_TRY(c, read_counters(ws, s, counters));
    uint64_t n_hits = counters[CTR_HITS];
    const bool rect = f.p.generator == ATMRT_GEN_RECTILINEAR;
    if (rect && !f.opaque) {
      ws.n_overflow = counters[CTR_OVERFLOW_PIXELS]; // pixels whose points did not fit the slots: marched a second time if the arena overflowed too
      ws.n_overflow_records = counters[CTR_OVERFLOW_RECORDS];
      HIP_TRY(c, hipMemsetAsync(&ws.counters[CTR_OVERFLOW_CURSOR], 0, sizeof(uint64_t), s));
    }
    HIP_TRY(c, reserve_carved(c->d_hit_lists, [&](Carve& k) { // what the fill pass needs per trace point, now that their number is known
      // some step produced more trace points than StepHits keeps: the fill pass sorts those in place by `prop`
      if (counters[CTR_BIG_STEPS]) k(ws.step_prop, (n_hits + 1) * sizeof(double));
      if (f.opaque) return;
      k(ws.list_step, (n_hits + 1) * sizeof(uint32_t)), k(ws.list_pixel, (n_hits + 1) * sizeof(uint32_t));
      if (rect) k(ws.rect_rec, 4 * (n_hits + 1) * sizeof(double)), k(ws.overflow, (ws.n_overflow + 1) * sizeof(uint32_t));
    }));
    HIP_TRY(c, reserve_carved(c->d_packed, [&](Carve& k) { packed = carve_packed(k, n_hits); }));
    if (f.opaque) launch_pack_first_hits(f, ws, dense, packed, s);
    else launch_list_fill(f, ws, n_hits, dense, packed, s);
    if (n_hits_out) *n_hits_out = n_hits;
  }
  HIP_TRY(c, hipEventRecord(ev[EV_PACK_END], s));
  if (packed_out) *packed_out = packed;
  return ATMRT_OK;
}

// The last stage of InterpolatingRectilinearGenerator::generate, for the frame and for atmrt_debug_interp_blend alike: cache_coords
// (:186-204) of every pixel of `f` over the ray table in ib.elev / ib.dir, the bounding rectangle of the lattice points the pixels
// reference, the lattice itself — `lattice(ei0, di0, ne, nd, lr)` leaves the ne x nd points of that rectangle in HBM, names them in
// `lr` (all but lr.ne / lr.nd) and points ib.referenced at ne x nd zeroed flags — and the 4-corner blend (:395-418) into `dense` and
// c->d_packed: count -> scan -> arena -> scan -> fill -> finish.  ws is the workspace of `f`, its counters zeroed by the caller.
template <class Lattice>
static int interp_blend_tail(atmrt_ctx* c, const Frame& f, Workspace& ws, InterpBuffers& ib, double min_elev_step, double min_dir_step,
                             const DensePlanes& dense, Lattice&& lattice, PackedHits* packed_out, uint64_t* n_hits_out) {
  hipStream_t s = c->stream;
  int32_t bounds[4] = {INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN};
  HIP_TRY(c, hipMemcpyAsync(ib.bounds, bounds, sizeof bounds, hipMemcpyHostToDevice, s));
  launch_lattice_keys(f, ib, min_elev_step, min_dir_step, s);
  HIP_TRY(c, hipMemcpyAsync(bounds, ib.bounds, sizeof bounds, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  const int64_t ne = (int64_t)bounds[1] + 1 - bounds[0] + 1, nd = (int64_t)bounds[3] + 1 - bounds[2] + 1;
  if (ne <= 0 || nd <= 0 || ne > 60000 || nd > 2000000 || ne * nd > (int64_t)1 << 31)
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "InterpolatingRectilinear lattice of %lld x %lld points is out of range",
                   (long long)nd, (long long)ne);
  LatticeResult lr{};
  int rc = lattice(bounds[0], bounds[2], ne, nd, lr);
  if (rc) return rc;
  lr.nd = (int32_t)nd;
  lr.ne = (int32_t)ne;
  // blend: count -> scan -> fill
  if ((rc = prepare_workspace(c, f, &ws))) return rc;
  HIP_TRY(c, hipMemsetAsync(&ws.counters[CTR_RAY_STEPS], 0, sizeof(uint64_t), s)); // only referenced lattice pixels count
  PackedHits none{};
  Frame fb = f;
  fb.di0 = bounds[2];
  fb.ei0 = bounds[0];
  launch_interp_blend(fb, ws, ib, lr, false, dense, none, s);
  launch_scan_counts(f, ws, dense.hit_count, s);
  uint64_t counters[N_COUNTERS];
  HIP_TRY(c, read_counters(ws, s, counters));
  BlendArena arena{};
  if (counters[CTR_BIG_BLEND_PIXELS]) { // pixels whose four corners hold more points than the in-register member list: blended over an HBM arena
    const size_t n = (size_t)counters[CTR_BIG_BLEND_POINTS];
    HIP_TRY(c, reserve_carved(c->d_blend_arena, [&](Carve& k) {
      k(arena.k, n * 8), k(arena.dist, n * 8), k(arena.group, n * 4), k(arena.corner, n), k(arena.tag, n);
    }));
    launch_interp_blend_big(fb, ws, ib, lr, false, dense, none, arena, s);
    launch_scan_counts(f, ws, dense.hit_count, s); // again, now that every pixel has its count
    HIP_TRY(c, read_counters(ws, s, counters));
  }
  uint64_t n_hits = counters[CTR_HITS];
  PackedHits packed;
  HIP_TRY(c, reserve_carved(c->d_packed, [&](Carve& k) { packed = carve_packed(k, n_hits); }));
  launch_interp_blend(fb, ws, ib, lr, true, dense, packed, s);
  if (arena.k) launch_interp_blend_big(fb, ws, ib, lr, true, dense, packed, arena, s);
  launch_interp_finish(f, ws, ib, lr, dense, packed, s);
  if (packed_out) *packed_out = packed;
  if (n_hits_out) *n_hits_out = n_hits;
  return ATMRT_OK;
}

// InterpolatingRectilinearGenerator::generate (interpolating_rectilinear.rs:110-162): ray table -> lattice steps ->
// lattice frame through the Fast pipeline -> 4-corner blend (count -> scan -> fill).
static int run_interpolating(atmrt_ctx* c, const Frame& f, Workspace& ws, const DensePlanes& dense, PackedHits* packed_out,
                             uint64_t* n_hits_out) {
  hipStream_t s = c->stream;
  const size_t W = f.p.width, H = f.p.height, npx = (size_t)f.wl * f.h;
  // gen_fov_data :453-522
  InterpBuffers ib{};
  HIP_TRY(c, reserve_carved(c->d_interp, [&](Carve& k) {
    k(ib.dir, W * H * 8), k(ib.elev, W * H * 8), k(ib.colmin, W * 8), k(ib.rowmin, H * 8);
    k(ib.rem_e, npx * 8), k(ib.rem_d, npx * 8), k(ib.key_e, npx * 4), k(ib.key_d, npx * 4), k(ib.bounds, 16);
  }));
  launch_fov_table(f, ib, s);
  std::vector<double> mins(W + H);
  HIP_TRY(c, hipMemcpyAsync(mins.data(), ib.colmin, W * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(mins.data() + W, ib.rowmin, H * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  double min_elev_step = INFINITY, min_dir_step = INFINITY; // .reduce(|| INFINITY, f64::min) * SCALE
  for (size_t x = 0; x < W; x++) min_elev_step = std::fmin(min_elev_step, mins[x]);
  for (size_t y = 0; y < H; y++) min_dir_step = std::fmin(min_dir_step, mins[W + y]);
  min_elev_step *= 1.5;
  min_dir_step *= 1.5;
  if (!(min_elev_step > 0.0) || !(min_dir_step > 0.0) || !std::isfinite(min_elev_step) || !std::isfinite(min_dir_step))
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "degenerate field of view for InterpolatingRectilinear");
  // the lattice frame (Cache::get_pixel :80-107 for every lattice point of the bounding rectangle)
  return interp_blend_tail(c, f, ws, ib, min_elev_step, min_dir_step, dense, [&](int32_t ei0, int32_t di0, int64_t ne, int64_t nd, LatticeResult& lr) {
    Frame fl = f;
    fl.p.generator = ATMRT_GEN_FAST;
    fl.lattice = 1;
    fl.di0 = di0;
    fl.ei0 = ei0;
    fl.dir_step = min_dir_step;
    fl.elev_step = min_elev_step;
    fl.c0 = 0;
    fl.wl = (int32_t)nd;
    fl.h = (int32_t)ne;
    const size_t nlat = (size_t)nd * ne;
    // run_core leaves its trace points in d_packed / d_hit_offset, and so must this frame.  The two pairs of buffers trade places
    // twice per frame — here, before the lattice workspace takes their addresses, and after the lattice pass — so that each pair serves the same role (lattice / image) in every frame
    // and keeps its capacity: with one swap the roles alternated and the smaller buffer was reallocated in the second frame.
    std::swap(c->d_packed, c->d_lat_packed);
    std::swap(c->d_hit_offset, c->d_lat_offset);
    Workspace wsl{};
    int rc = prepare_workspace(c, fl, &wsl);
    if (rc) return rc;
    HIP_TRY(c, reserve_carved(c->d_px_steps, [&](Carve& k) { k(wsl.px_steps, nlat * sizeof(uint32_t)), k(ib.referenced, nlat); }));
    HIP_TRY(c, hipMemsetAsync(ib.referenced, 0, nlat, s));
    DensePlanes ldense;
    HIP_TRY(c, reserve_carved(c->d_lat_dense, [&](Carve& k) { ldense = carve_dense(k, nlat); }));
    PackedHits lpacked{};
    uint64_t lhits = 0;
    if ((rc = run_core(c, fl, wsl, ldense, true, &lpacked, &lhits))) return rc;
    std::swap(c->d_packed, c->d_lat_packed);   // keep the lattice result; the image gets the other pair
    std::swap(c->d_hit_offset, c->d_lat_offset);
    lr.hit_count = ldense.hit_count;
    lr.hit_offset = c->d_lat_offset.as<uint64_t>();
    lr.azimuth = ldense.azimuth;
    lr.elevation_angle = ldense.elevation_angle;
    lr.hits = lpacked;
    lr.px_steps = wsl.px_steps;
    return (int)ATMRT_OK;
  }, packed_out, n_hits_out);
}

// Runs the generator named in params.  `dense` must be device memory.  When `want_packed`, the
// packed trace points are left in c->d_packed (n_hits of them).  What the frame left where is c->last.
static int run_generator(atmrt_ctx* c, const Frame& f, Workspace& ws, const DensePlanes& dense, bool want_packed, uint64_t* n_hits_out,
                         uint64_t* ray_steps_out, double* ms_out) {
  hipStream_t s = c->stream;
  hipEvent_t* ev = c->ev;
  // the buffers of the previous frame are about to be reused (or reallocated): until this frame has succeeded there is nothing
  // atmrt_draw_image / atmrt_last_hits_device may touch
  c->last.valid = false;
  c->last.ceil_rows = 0;
  c->last.march_route = MarchRoute::None; // run_core sets it where it launches the Rectilinear march
  c->stats = atmrt_frame_stats_t{};
  HIP_TRY(c, hipEventRecord(c->ev_t0, s));
  c->scan_segments = 0;
  HIP_TRY(c, hipMemsetAsync(ws.counters, 0, N_COUNTERS * sizeof(uint64_t), s));
  PackedHits packed{};
  int rc;
  if (f.p.generator == ATMRT_GEN_INTERPOLATING_RECTILINEAR) rc = run_interpolating(c, f, ws, dense, &packed, n_hits_out);
  else rc = run_core(c, f, ws, dense, want_packed, &packed, n_hits_out);
  if (rc) return rc;
  if (c->inject_failure) { // test hook: the frame's kernels have run and its buffers have been rewritten; now fail
    c->inject_failure = false;
    (void)hipStreamSynchronize(s);
    return c->fail(ATMRT_ERR_HIP, "failure injected by atmrt_debug_fail_next_frame");
  }
  uint64_t counters[N_COUNTERS];
  HIP_TRY(c, hipEventRecord(c->ev_t1, s));
  HIP_TRY(c, read_counters(ws, s, counters));
  HIP_TRY(c, hipGetLastError());
  float ms = 0.f;
  HIP_TRY(c, hipEventElapsedTime(&ms, c->ev_t0, c->ev_t1));
  {
    atmrt_timings_t t{};
    float v = 0.f;
    t.total_ms = ms;
    if (f.p.generator != ATMRT_GEN_RECTILINEAR) {
      HIP_TRY(c, hipEventElapsedTime(&v, ev[EV_PROFILE_BEGIN], ev[EV_PROFILE_END]));
      t.profile_ms = v;
      HIP_TRY(c, hipEventElapsedTime(&v, ev[EV_PATHS_BEGIN], ev[EV_PATHS_END]));
      t.paths_ms = v;
      HIP_TRY(c, hipEventElapsedTime(&v, ev[EV_MARCH_BEGIN], ev[EV_MARCH_END]));
      t.intersect_ms = v;
      if (c->scan_segments) { // pipelined frame: the scan's own time, without the waits for the path segments
        t.intersect_ms = 0.0;
        for (int k = 0; k < c->scan_segments; k++) {
          HIP_TRY(c, hipEventElapsedTime(&v, c->ev_scan[2 * k], c->ev_scan[2 * k + 1]));
          t.intersect_ms += v;
        }
      }
    } else {
      HIP_TRY(c, hipEventElapsedTime(&v, ev[EV_MARCH_BEGIN], ev[EV_MARCH_END]));
      t.march_ms = v;
    }
    HIP_TRY(c, hipEventElapsedTime(&v, ev[EV_FINALIZE_BEGIN], ev[EV_FINALIZE_END]));
    t.finalize_ms = v;
    HIP_TRY(c, hipEventElapsedTime(&v, ev[EV_PACK_BEGIN], ev[EV_PACK_END]));
    t.pack_ms = v;
    t.ray_steps = counters[CTR_RAY_STEPS];
    t.n_hits = counters[CTR_HITS];
    if (c->ceil_built) {
      HIP_TRY(c, hipEventElapsedTime(&v, ev[EV_CEIL_BEGIN], ev[EV_CEIL_END]));
      t.ceiling_ms = v;
    }
    c->timings = t;
  }
  if (counters[CTR_SLICE_UNFINISHED])
    return c->fail(ATMRT_ERR_HIP, "the time-sliced march left %llu of its ray groups unfinished", (unsigned long long)counters[CTR_SLICE_UNFINISHED] - 1);
  c->stats.unlisted_rays = counters[CTR_UNLISTED_RAYS];
  c->stats.unlisted_columns = counters[CTR_UNLISTED_COLUMNS];
  c->stats.big_steps = counters[CTR_BIG_STEPS];
  c->stats.big_blend_pixels += counters[CTR_BIG_BLEND_PIXELS];
  c->stats.retraced_pixels += ws.n_overflow;
  c->stats.terrain_lookups = counters[CTR_TERRAIN_LOOKUPS];
  c->stats.object_rays = counters[CTR_OBJECT_RAYS];
  c->stats.object_steps = counters[CTR_OBJECT_STEPS];
  if (ms_out) *ms_out = ms;
  if (ray_steps_out) *ray_steps_out = counters[CTR_RAY_STEPS];
  LastFrame& l = c->last; // the frame has succeeded: everything of the record but march_route, which run_core has set
  l.valid = true;
  l.packed = want_packed || !f.opaque || f.p.generator == ATMRT_GEN_INTERPOLATING_RECTILINEAR;
  l.npx = (size_t)f.wl * f.h;
  l.wl = f.wl, l.h = f.h, l.c0 = f.c0;
  l.alpha = f.p.terrain_alpha;
  l.params = f.p;
  l.dense = dense, l.hits = packed, l.offset = ws.hit_offset;
  l.nhits = l.packed ? counters[CTR_HITS] : 0;
  l.ray_steps = counters[CTR_RAY_STEPS], l.escaped_steps = counters[CTR_ESCAPED_STEPS], l.escaped_rays = counters[CTR_ESCAPED_RAYS];
  l.ceil_rows = f.ceil ? f.march_steps + 1 : 0;
  l.ceil_layout = f.ceil_layout;
  l.ceil_serial = c->ceiling.serial();
  l.order_groups = f.ceil_order ? (uint32_t)(((size_t)f.wl * f.h + 63) / 64) : 0;
  l.order_serial = c->ceil_order.serial();
  return ATMRT_OK;
}

// ---------------------------------------------------------------------------------------------
// the path
// ---------------------------------------------------------------------------------------------
// Host memory of atmrt_result_t: ONE page-locked block per result (device-to-host copies run at PCIe speed into it; through
// pageable memory the 0.7 GB of a headline frame cost 55 ms, eight times the Fast generator's device time), carved into the
// arrays with 256-byte alignment.  Pinning is slow, so freed blocks are kept (at most two, process-wide) and reused by later
// frames of a similar size.  If pinned memory cannot be had the block is ordinary malloc memory.
namespace {
struct HostBlocks {
  std::mutex m;
  struct Blk {
    void* p;
    size_t cap;
    bool pinned;
  };
  std::vector<Blk> live, spare;
  void* take(size_t bytes) {
    std::lock_guard<std::mutex> g(m);
    for (size_t i = 0; i < spare.size(); i++)
      if (spare[i].cap >= bytes && spare[i].cap / 2 <= bytes) {
        Blk b = spare[i];
        spare.erase(spare.begin() + (long)i);
        live.push_back(b);
        return b.p;
      }
    Blk b{nullptr, bytes + bytes / 16, true};
    if (hipHostMalloc(&b.p, b.cap, hipHostMallocDefault) != hipSuccess || !b.p) {
      (void)hipGetLastError();
      b = Blk{malloc(bytes), bytes, false};
      if (!b.p) return nullptr;
    }
    live.push_back(b);
    return b.p;
  }
  void give(void* p) {
    std::lock_guard<std::mutex> g(m);
    for (size_t i = 0; i < live.size(); i++)
      if (live[i].p == p) {
        Blk b = live[i];
        live.erase(live.begin() + (long)i);
        if (!b.pinned) {
          free(b.p);
          return;
        }
        spare.push_back(b);
        if (spare.size() > 2) {
          (void)hipHostFree(spare.front().p);
          spare.erase(spare.begin());
        }
        return;
      }
  }
};
HostBlocks g_host_blocks;
} // namespace

extern "C" int atmrt_internal_result_alloc(atmrt_result_t* out, uint32_t width, uint32_t height, uint64_t n_hits) {
  memset(out, 0, sizeof *out);
  const size_t npx = (size_t)width * height;
  const size_t nh = n_hits ? n_hits : 1, np1 = npx ? npx : 1;
  auto layout = [&](Carve& k) { // azimuth first: atmrt_result_free returns the block by this pointer
    k(out->azimuth, np1 * 8), k(out->elevation_angle, np1 * 8), k(out->hit_offset, np1 * 8), k(out->hit_count, np1 * 4);
    packed_fields([&](size_t b, auto*& a) { k(a, nh * b); }, *out);
  };
  Carve size(nullptr);
  layout(size);
  Carve block(g_host_blocks.take(size.bytes));
  if (!block.base) return -1;
  layout(block);
  out->width = width;
  out->height = height;
  out->n_pixels = npx;
  out->n_hits = n_hits;
  return 0;
}

extern "C" void atmrt_result_free(atmrt_result_t* r) {
  if (!r) return;
  if (r->azimuth) g_host_blocks.give(r->azimuth); // the first array is the base of the block
  memset(r, 0, sizeof *r);
}

// One frame of this context's tile, everything left in HBM: the one generate sequence, of atmrt_generate, atmrt_generate_device and
// the multi-device paths alike.
int atmrt::api_generate_tile(atmrt_ctx* c, const DensePlanes* dense_in, bool want_packed, uint64_t* n_hits, uint64_t* ray_steps,
                             double* device_ms) {
  Frame f;
  int rc = prepare_frame(c, &f);
  if (rc) return rc;
  Workspace ws{};
  if ((rc = prepare_workspace(c, f, &ws))) return rc;
  DensePlanes dense;
  if (dense_in) {
    dense = *dense_in;
  } else {
    HIP_TRY(c, reserve_carved(c->d_dense, [&](Carve& k) { dense = carve_dense(k, (size_t)f.wl * f.h); }));
  }
  uint64_t nh = 0;
  rc = run_generator(c, f, ws, dense, want_packed, &nh, ray_steps, device_ms);
  if (n_hits) *n_hits = nh;
  return rc;
}

// The frame (or the probe's image) of wl x h pixels that `dense`, `hit_offset` and `packed` hold in HBM as a library-allocated
// atmrt_result_t.
static int result_to_host(atmrt_ctx* c, int wl, int h, const DensePlanes& dense, const uint64_t* hit_offset, const PackedHits& packed,
                          uint64_t n_hits, uint64_t steps, double ms, atmrt_result_t* out) {
  const size_t npx = (size_t)wl * h;
  if (atmrt_internal_result_alloc(out, (uint32_t)wl, (uint32_t)h, n_hits))
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "out of host memory for %zu pixels / %llu hits", npx, (unsigned long long)n_hits);
  out->ray_steps = steps;
  out->device_ms = ms;
  hipStream_t s = c->stream;
  auto d2h = [&](void* dst, const void* src, size_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s); };
  hipError_t e = d2h(out->azimuth, dense.azimuth, npx * 8);
  if (e == hipSuccess) e = d2h(out->elevation_angle, dense.elevation_angle, npx * 8);
  if (e == hipSuccess) e = d2h(out->hit_count, dense.hit_count, npx * 4);
  if (e == hipSuccess) e = d2h(out->hit_offset, hit_offset, npx * 8);
  if (e == hipSuccess) e = copy_packed(*out, packed, n_hits, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    atmrt_result_free(out);
    return c->fail(ATMRT_ERR_HIP, "copying the result to the host: %s", hipGetErrorString(e));
  }
  return ATMRT_OK;
}

extern "C" int atmrt_generate(atmrt_ctx* c, atmrt_result_t* out) {
  if (!c || !out) return ATMRT_ERR_INVALID_ARGUMENT;
  memset(out, 0, sizeof *out);
  if (c->multi) return multi_generate(c, out); // every device its pixel-column tile, straight into the one [H][W] block
  uint64_t n_hits = 0, steps = 0;
  double ms = 0;
  if (int rc = api_generate_tile(c, nullptr, true, &n_hits, &steps, &ms)) return rc;
  const LastFrame& l = c->last;
  return result_to_host(c, l.wl, l.h, l.dense, l.offset, l.hits, n_hits, steps, ms, out);
}

extern "C" int atmrt_generate_device(atmrt_ctx* c, const atmrt_device_planes_t* planes, uint64_t* ray_steps,
                                     double* device_ms) {
  if (!c || !planes) return ATMRT_ERR_INVALID_ARGUMENT;
  if (c->multi) return c->fail(ATMRT_ERR_STATE, "a multi-device context leaves its frame in HBM through atmrt_generate_image_device");
  DensePlanes dense;
  if (!planes_from_abi(*planes, &dense)) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "every plane pointer must be a device allocation");
  return api_generate_tile(c, &dense, false, nullptr, ray_steps, device_ms);
}

extern "C" int atmrt_last_hits_device(atmrt_ctx* c, const atmrt_device_hits_t* dst, uint64_t* n_hits) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (c->multi) return c->fail(ATMRT_ERR_STATE, "a multi-device context hands its lists over through atmrt_image_hits_device");
  if (!c->last.valid) return c->fail(ATMRT_ERR_STATE, "atmrt_last_hits_device needs a frame: call atmrt_generate_device first");
  if (!c->last.packed)
    return c->fail(ATMRT_ERR_STATE, "the last frame holds first-hit planes only (opaque scene through atmrt_generate_device): "
                                    "its trace points are the planes themselves");
  const uint64_t n = c->last.nhits;
  if (n_hits) *n_hits = n;
  if (!dst) return ATMRT_OK; // size query
  if (dst->capacity < n)
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "capacity %llu is less than the %llu trace points of the frame",
                   (unsigned long long)dst->capacity, (unsigned long long)n);
  PackedHits to;
  if (!hits_from_abi(*dst, &to) || !dst->hit_offset)
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "every array pointer must be a device allocation");
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  if (c->last.npx) HIP_TRY(c, hipMemcpyAsync(dst->hit_offset, c->last.offset, c->last.npx * 8, hipMemcpyDeviceToDevice, s));
  HIP_TRY(c, copy_packed(to, c->last.hits, n, hipMemcpyDeviceToDevice, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  return ATMRT_OK;
}

extern "C" int atmrt_last_timings(atmrt_ctx* c, atmrt_timings_t* out) {
  if (!c || !out) return ATMRT_ERR_INVALID_ARGUMENT;
  if (c->multi) return multi_last_timings(c, out);
  *out = c->timings;
  return ATMRT_OK;
}

extern "C" int atmrt_debug_fail_next_frame(atmrt_ctx* c) {
  if (!c) return ATMRT_ERR_INVALID_ARGUMENT;
  if (c->multi) return atmrt_debug_fail_next_frame(multi_child(c, multi_size(c) - 1));
  c->inject_failure = true;
  return ATMRT_OK;
}

extern "C" int atmrt_last_stats(atmrt_ctx* c, atmrt_frame_stats_t* out) {
  if (!c || !out) return ATMRT_ERR_INVALID_ARGUMENT;
  if (c->multi) return multi_last_stats(c, out);
  *out = c->stats;
  return ATMRT_OK;
}

extern "C" int atmrt_last_march_work(atmrt_ctx* c, uint64_t* integrated_steps, uint64_t* escaped_rays) {
  if (!c || !integrated_steps || !escaped_rays) return ATMRT_ERR_INVALID_ARGUMENT;
  if (c->multi) return multi_last_march_work(c, integrated_steps, escaped_rays);
  *integrated_steps = c->last.ray_steps - c->last.escaped_steps;
  *escaped_rays = c->last.escaped_rays;
  return ATMRT_OK;
}

extern "C" int atmrt_debug_interp_blend(atmrt_ctx* c, uint32_t width, uint32_t height, const double* elev, const double* dir,
                                        double min_elev_step, double min_dir_step, double simulation_step,
                                        const atmrt_interp_lattice_t* lat, atmrt_result_t* out) {
  if (!c || !out) return ATMRT_ERR_INVALID_ARGUMENT;
  memset(out, 0, sizeof *out);
  FORWARD_TO_FIRST_DEVICE(c, atmrt_debug_interp_blend(k_, width, height, elev, dir, min_elev_step, min_dir_step, simulation_step, lat, out));
  if (!elev || !dir || !lat) return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "atmrt_debug_interp_blend: a NULL ray table or lattice");
  if (!lat->hit_count || !lat->azimuth || !lat->elevation_angle || !lat->px_steps ||
      (lat->n_hits && (!lat->lat || !lat->lon || !lat->distance || !lat->elevation || !lat->path_length || !lat->normal || !lat->color_tag || !lat->rgba)))
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "atmrt_debug_interp_blend: a NULL lattice plane");
  const size_t npx = (size_t)width * height;
  if (!width || !height || width > 65535 || height > 65535 || npx > ((size_t)1 << 24)) // a frame's sides are u16
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "atmrt_debug_interp_blend: an image of %u x %u pixels", width, height);
  for (double step : {min_elev_step, min_dir_step, simulation_step})
    if (!(step > 0.0) || !std::isfinite(step))
      return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "atmrt_debug_interp_blend: a step of %g is not finite and positive", step);
  if (lat->ne <= 0 || lat->nd <= 0 || (int64_t)lat->ne * lat->nd > (int64_t)1 << 31)
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "atmrt_debug_interp_blend: a lattice of %d x %d points", lat->nd, lat->ne);
  const size_t nlat = (size_t)lat->ne * lat->nd;
  std::vector<uint64_t> offset(nlat); // what launch_scan_counts leaves of the lattice frame's hit_count
  uint64_t total = 0;
  for (size_t q = 0; q < nlat; q++) offset[q] = total, total += lat->hit_count[q];
  if (total != lat->n_hits)
    return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "atmrt_debug_interp_blend: hit_count sums to %llu, n_hits is %llu", (unsigned long long)total,
                   (unsigned long long)lat->n_hits);
  for (uint64_t k = 0; k < total; k++)
    if (lat->color_tag[k] != ATMRT_COLOR_TERRAIN && lat->color_tag[k] != ATMRT_COLOR_RGBA)
      return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "atmrt_debug_interp_blend: trace point %llu has the unknown colour tag %u", (unsigned long long)k,
                     lat->color_tag[k]);
  HIP_TRY(c, hipSetDevice(c->device));
  c->last.valid = false; // the buffers of the last frame are about to be rewritten
  hipStream_t s = c->stream;
  Frame f{}; // what the blend reads of a frame: the image, its shard (all of it) and the step; an opaque frame sizes the least scratch
  f.p.generator = ATMRT_GEN_INTERPOLATING_RECTILINEAR;
  f.p.width = (uint16_t)width;
  f.p.height = (uint16_t)height;
  f.p.simulation_step = simulation_step;
  f.wl = (int32_t)width;
  f.h = (int32_t)height;
  f.opaque = 1;
  Workspace ws{};
  int rc = prepare_workspace(c, f, &ws);
  if (rc) return rc;
  HIP_TRY(c, hipMemsetAsync(ws.counters, 0, N_COUNTERS * sizeof(uint64_t), s));
  DensePlanes dense;
  HIP_TRY(c, reserve_carved(c->d_dense, [&](Carve& k) { dense = carve_dense(k, npx); }));
  InterpBuffers ib{};
  HIP_TRY(c, reserve_carved(c->d_interp, [&](Carve& k) {
    k(ib.dir, npx * 8), k(ib.elev, npx * 8);
    k(ib.rem_e, npx * 8), k(ib.rem_d, npx * 8), k(ib.key_e, npx * 4), k(ib.key_d, npx * 4), k(ib.bounds, 16);
  }));
  HIP_TRY(c, hipMemcpyAsync(ib.elev, elev, npx * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipMemcpyAsync(ib.dir, dir, npx * 8, hipMemcpyHostToDevice, s));
  PackedHits packed{};
  uint64_t n_hits = 0;
  rc = interp_blend_tail(c, f, ws, ib, min_elev_step, min_dir_step, dense, [&](int32_t ei0, int32_t di0, int64_t ne, int64_t nd, LatticeResult& lr) {
    if (ne != lat->ne || nd != lat->nd)
      return c->fail(ATMRT_ERR_INVALID_ARGUMENT, "atmrt_debug_interp_blend: the rays reference %lld x %lld lattice points from (%d, %d), the lattice has %d x %d",
                     (long long)nd, (long long)ne, di0, ei0, lat->nd, lat->ne);
    // the caller's planes where the lattice pass of a frame leaves its own
    uint32_t* px_steps;
    HIP_TRY(c, reserve_carved(c->d_px_steps, [&](Carve& k) { k(px_steps, nlat * sizeof(uint32_t)), k(ib.referenced, nlat); }));
    HIP_TRY(c, hipMemsetAsync(ib.referenced, 0, nlat, s));
    DensePlanes ldense;
    HIP_TRY(c, reserve_carved(c->d_lat_dense, [&](Carve& k) { ldense = carve_dense(k, nlat); }));
    PackedHits lpacked{};
    HIP_TRY(c, reserve_carved(c->d_lat_packed, [&](Carve& k) { lpacked = carve_packed(k, total); }));
    uint64_t* loffset;
    HIP_TRY(c, reserve_into(c->d_lat_offset, loffset, nlat));
    auto h2d = [&](void* dst, const void* src, size_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s); };
    HIP_TRY(c, h2d(px_steps, lat->px_steps, nlat * 4));
    HIP_TRY(c, h2d(ldense.hit_count, lat->hit_count, nlat * 4));
    HIP_TRY(c, h2d(ldense.azimuth, lat->azimuth, nlat * 8));
    HIP_TRY(c, h2d(ldense.elevation_angle, lat->elevation_angle, nlat * 8));
    HIP_TRY(c, h2d(loffset, offset.data(), nlat * 8));
    hipError_t e = hipSuccess;
    if (total) packed_fields([&](size_t b, auto* to, auto* from) { if (e == hipSuccess) e = h2d(to, from, total * b); }, lpacked, *lat);
    HIP_TRY(c, e);
    HIP_TRY(c, hipStreamSynchronize(s)); // `offset` and the caller's arrays are pageable memory
    lr.hit_count = ldense.hit_count;
    lr.hit_offset = loffset;
    lr.azimuth = ldense.azimuth;
    lr.elevation_angle = ldense.elevation_angle;
    lr.hits = lpacked;
    lr.px_steps = px_steps;
    return (int)ATMRT_OK;
  }, &packed, &n_hits);
  if (rc) return rc;
  uint64_t counters[N_COUNTERS];
  HIP_TRY(c, read_counters(ws, s, counters));
  HIP_TRY(c, hipGetLastError());
  return result_to_host(c, f.wl, f.h, dense, ws.hit_offset, packed, n_hits, counters[CTR_RAY_STEPS], 0.0, out);
}
