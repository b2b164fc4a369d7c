/* atmrt.h — C ABI of the MI355X-native per-pixel ray-marching path of atm-raytracer.
 *
 * The reference has no FFI: its plug-in surface for this path is the Rust trait
 *     pub trait Generator { fn generate(&self) -> Vec<Vec<ResultPixel>>; }
 * (src/generator/generators/mod.rs:82-84), implemented by FastGenerator (fast.rs:21-108),
 * RectilinearGenerator (rectilinear.rs:23-76) and InterpolatingRectilinearGenerator
 * (interpolating_rectilinear.rs:110-162), each built from (&Params, &Terrain).  The entry points
 * below are what a Rust `impl Generator for HipGenerator` binds (INTEGRATION.md shows the stub):
 * plain pointers, sizes and #[repr(C)]-compatible PODs; all angles in DEGREES and all lengths in
 * METRES exactly as in the reference's `Params` (src/generator/params.rs:496-505).
 *
 * Error convention: every call returns 0 on success or a negative atmrt_status; the message is
 * available from atmrt_last_error().  The library never aborts the process (the reference
 * panics: terrain/mod.rs:45,71,117, params.rs:681-691; a shim may turn a non-zero status into
 * panic!/Err(String) to keep that behaviour).  A context is single-owner and not re-entrant.
 */
#ifndef ATMRT_H
#define ATMRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ATMRT_ABI_VERSION 5

typedef enum atmrt_status {
  ATMRT_OK = 0,
  ATMRT_ERR_INVALID_ARGUMENT = -1, /* bad pointer, size or enum value */
  ATMRT_ERR_NO_DEVICE = -2,        /* no gfx950 device / HIP runtime unavailable: never falls back to CPU */
  ATMRT_ERR_HIP = -3,              /* a HIP call or kernel failed (message carries hipGetErrorString) */
  ATMRT_ERR_IO = -4,               /* terrain directory or file unreadable (terrain/mod.rs:70-71) */
  ATMRT_ERR_FORMAT = -5,           /* a file in the terrain directory is not a DTED tile (terrain/mod.rs:113-118) */
  ATMRT_ERR_STATE = -6,            /* call order violated (e.g. generate before set_params) */
  ATMRT_ERR_UNSUPPORTED = -7       /* reserved; not returned since ABI 3: the fixed capacities of ABI 2 (12 trace points per step, 64
                                      corner points per interpolating pixel) now have unbounded routes */
} atmrt_status;

/* EarthModel, src/utils/earth_model/mod.rs:19-28 (same order as the Rust enum). */
typedef enum atmrt_earth_kind {
  ATMRT_EARTH_SIMPLE_SPHERE = 0,
  ATMRT_EARTH_SPHERICAL = 1,             /* uses .radius */
  ATMRT_EARTH_ELLIPSOID = 2,             /* uses .a, .b */
  ATMRT_EARTH_WGS84 = 3,
  ATMRT_EARTH_AZIMUTHAL_EQUIDISTANT = 4,
  ATMRT_EARTH_FLAT_DISTORTED = 5,
  ATMRT_EARTH_OBSERVER_AE = 6,           /* uses .radius as proj_radius */
  ATMRT_EARTH_SIMPLE_OBSERVER_AE = 7
} atmrt_earth_kind;

typedef struct atmrt_earth_model {
  int32_t kind; /* atmrt_earth_kind */
  int32_t _pad;
  double radius;
  double a;
  double b;
} atmrt_earth_model_t;

/* Altitude, params.rs:17-30. */
typedef enum atmrt_altitude_kind { ATMRT_ALT_ABSOLUTE = 0, ATMRT_ALT_RELATIVE = 1 } atmrt_altitude_kind;

/* Position, params.rs:32-40. */
typedef struct atmrt_position {
  double latitude;
  double longitude;
  int32_t altitude_kind; /* atmrt_altitude_kind */
  int32_t _pad;
  double altitude;
} atmrt_position_t;

/* Frame, params.rs:145-155. */
typedef struct atmrt_frame {
  double direction;
  double tilt;
  double fov;
  double max_distance;
} atmrt_frame_t;

/* GeneratorDef, params.rs:387-392 (same order). */
typedef enum atmrt_generator_kind {
  ATMRT_GEN_FAST = 0,
  ATMRT_GEN_INTERPOLATING_RECTILINEAR = 1,
  ATMRT_GEN_RECTILINEAR = 2
} atmrt_generator_kind;

/* The subset of `Params` (params.rs:496-505) that reaches the generators. */
typedef struct atmrt_params {
  atmrt_position_t position;   /* view.position */
  atmrt_frame_t frame;         /* view.frame */
  atmrt_earth_model_t earth;   /* model; env.shape is derived from it (earth_model/mod.rs:95-112) */
  double wavelength;           /* env.wavelength [m] */
  double simulation_step;      /* [m] */
  double terrain_alpha;        /* scene.terrain_alpha */
  int32_t straight_rays;       /* bool */
  int32_t generator;           /* atmrt_generator_kind, output.generator */
  uint16_t width;              /* output.width  (u16 as in params.rs:398-402) */
  uint16_t height;             /* output.height */
  uint16_t col_begin;          /* pixel-column shard [col_begin, col_end) computed by this context; 0,0 means the whole width. */
  uint16_t col_end;            /*   Leave 0,0 on a multi-device context / a rank context: the library assigns the tiles itself. */
} atmrt_params_t;

/* AtmosphereDef of crate atm-refraction 0.6 (schema: reference README.md:283-323): a pressure fixed point, a list of
 * temperature functions (the first from -inf, every next one from its `altitude` upwards), each either `Linear{gradient}`
 * or `Spline{boundary_condition, points}`, and — when every function is Linear — a temperature fixed point.  Both lists are
 * `Vec`s in the reference (params.rs:453-454) and unbounded here: pointer + count, borrowed for the duration of the call that
 * takes the definition (atmrt_set_atmosphere copies what it needs). */
typedef enum atmrt_temp_function_kind { ATMRT_TEMP_LINEAR = 0, ATMRT_TEMP_SPLINE = 1 } atmrt_temp_function_kind;
typedef enum atmrt_spline_boundary {
  ATMRT_SPLINE_NATURAL = 0,            /* second derivative 0 at both ends */
  ATMRT_SPLINE_DERIVATIVES = 1,        /* first derivatives bc[0], bc[1] at the ends */
  ATMRT_SPLINE_SECOND_DERIVATIVES = 2  /* second derivatives bc[0], bc[1] at the ends */
} atmrt_spline_boundary;
typedef struct atmrt_temp_function {
  int32_t kind;      /* atmrt_temp_function_kind */
  int32_t boundary;  /* enum atmrt_spline_boundary; Spline only */
  double altitude;   /* applies for h >= altitude; ignored for the first function */
  double gradient;   /* Linear: dT/dh [K/m] */
  double bc[2];      /* Spline boundary values */
  int32_t n_points;  /* Spline: >= 2, strictly increasing altitudes */
  int32_t _pad;
  const double* point_altitude;    /* [n_points] */
  const double* point_temperature; /* [n_points] */
} atmrt_temp_function_t;
typedef struct atmrt_atmosphere {
  double pressure_altitude;          /* pressure fixed point */
  double pressure;                   /* [Pa] */
  double temperature_altitude;       /* temperature_fixed_point (used only when has_temperature_fixed_point) */
  double temperature;                /* [K] */
  int32_t has_temperature_fixed_point;
  int32_t n_functions;               /* >= 1 */
  const atmrt_temp_function_t* functions; /* [n_functions] */
} atmrt_atmosphere_t;

/* Scene objects, src/object/mod.rs:19-75,119-131 after ConfShape::into_shape. */
typedef enum atmrt_object_kind { ATMRT_OBJ_FRUSTUM = 0, ATMRT_OBJ_BILLBOARD = 1 } atmrt_object_kind;
typedef struct atmrt_object {
  int32_t kind; /* atmrt_object_kind; Cylinder = Frustum{r1=r2}, Cone = Frustum{r2=0} (object/mod.rs:44-54) */
  int32_t _pad;
  atmrt_position_t position;
  double r1, r2;       /* frustum bottom / top radius */
  double height;       /* frustum or billboard height */
  double width;        /* billboard width */
  double color[4];     /* frustum RGBA in [0,1]; alpha defaults to 1.0 in the YAML (object/mod.rs:140-146) */
  const uint8_t* texture_rgba; /* billboard texture, row-major top row first, 4 bytes per texel; borrowed during the call */
  uint32_t texture_width;
  uint32_t texture_height;
} atmrt_object_t;

/* PixelColor tag of a trace point, generators/mod.rs:45-49. */
typedef enum atmrt_color_tag { ATMRT_COLOR_TERRAIN = 0, ATMRT_COLOR_RGBA = 1 } atmrt_color_tag;

/* Vec<Vec<ResultPixel>> (generators/mod.rs:13-30) flattened to structure-of-arrays.
 * Pixel p = y * width + (x - col_begin), row-major like result[y][x] (fast.rs:52-92).
 * Trace points of pixel p are hits [hit_offset[p], hit_offset[p] + hit_count[p]) in march order. */
typedef struct atmrt_result {
  uint32_t width;  /* columns in this shard */
  uint32_t height;
  uint64_t n_pixels;
  uint64_t n_hits;
  double* azimuth;         /* [n_pixels] degrees */
  double* elevation_angle; /* [n_pixels] degrees */
  uint32_t* hit_count;     /* [n_pixels] */
  uint64_t* hit_offset;    /* [n_pixels] */
  double* lat;             /* [n_hits] TracePoint.lat */
  double* lon;
  double* distance;
  double* elevation;
  double* path_length;
  double* normal;          /* [n_hits][3] */
  uint32_t* color_tag;     /* [n_hits] atmrt_color_tag */
  double* rgba;            /* [n_hits][4]; Terrain(alpha) -> {0,0,0,alpha} */
  uint64_t ray_steps;      /* sample pairs examined under the reference's termination rule (utils.rs:211-287) */
  double device_ms;        /* device time of the generate call, HIP events */
} atmrt_result_t;

/* Device-resident first-hit planes of one shard, written by atmrt_generate_device (caller-owned
 * device memory, e.g. torch tensors; the library only writes them).  Used by bench.py and by the
 * multi-GPU path so that results stay in HBM for the RCCL all-gather. */
typedef struct atmrt_device_planes {
  double* azimuth;         /* [H][Wshard] */
  double* elevation_angle;
  uint32_t* hit_count;     /* total trace points of the pixel */
  double* lat;             /* first trace point; NaN where hit_count == 0 */
  double* lon;
  double* distance;
  double* elevation;
  double* path_length;
  double* normal;          /* [3][H][Wshard] planar */
} atmrt_device_planes_t;

typedef struct atmrt_ctx atmrt_ctx;

/* ---- lifetime ---------------------------------------------------------------------------- */
int atmrt_abi_version(void);
/* "source_hash: <sha256/16 of csrc + Makefile + this header>; march_units: <flags>; calling_units: <flags>; all: <flags>; arch: gfx950":
 * what the library was built from and with which code-generation flags (the calling units must carry -enable-ipra=0). */
const char* atmrt_build_info(void);
/* device_ordinal: HIP device index (LOCAL_RANK under torchrun).  Fails with ATMRT_ERR_NO_DEVICE
 * when no GPU is present — there is no CPU path in this library. */
int atmrt_ctx_create(atmrt_ctx** out, int device_ordinal);
void atmrt_ctx_destroy(atmrt_ctx* ctx);
/* Message of the last failing call on ctx (or of the last failing atmrt_ctx_create when ctx == NULL). */
const char* atmrt_last_error(const atmrt_ctx* ctx);

/* ---- terrain: replaces Terrain::{from_folder,get_elev} (terrain/mod.rs:55-126) + crate dted 0.2 */
/* Scan a terrain directory (Terrain::from_folder, terrain/mod.rs:66-118): every entry must be a DTED file or be named like a
 * GeoTIFF tile ((N|S)dd(E|W)ddd, 16-bit single band, at least 3601 x 3601 samples); anything else fails as the reference
 * panics.  A GeoTIFF that cannot be decoded leaves its cell without terrain, like the reference's lazy load. */
int atmrt_terrain_load_dir(atmrt_ctx* ctx, const char* path, int32_t* n_files);
/* Register one 1-degree cell directly.  posts: n_lat rows (south to north) of n_lon posts (west to east). */
int atmrt_terrain_add_tile(atmrt_ctx* ctx, int32_t lat0, int32_t lon0, int32_t n_lat, int32_t n_lon,
                           const int16_t* posts);
int atmrt_terrain_clear(atmrt_ctx* ctx);
/* Batched Terrain::get_elev on the device: valid[i] = 0 where the reference returns None. */
int atmrt_terrain_get_elev(atmrt_ctx* ctx, size_t n, const double* lat, const double* lon, double* elev,
                           uint8_t* valid);

/* ---- configuration ------------------------------------------------------------------------ */
void atmrt_params_default(atmrt_params_t* p);         /* Config::default, params.rs:481-494 */
void atmrt_atmosphere_us76(atmrt_atmosphere_t* a);    /* AtmosphereDef::us_76; `functions` points at a table inside the library */
int atmrt_set_params(atmrt_ctx* ctx, const atmrt_params_t* p);
int atmrt_set_atmosphere(atmrt_ctx* ctx, const atmrt_atmosphere_t* a);
/* scene.objects, in order (object/mod.rs:156-190).  Billboard textures are copied during the call. */
int atmrt_objects_set(atmrt_ctx* ctx, const atmrt_object_t* objects, size_t n);

/* ---- the path ----------------------------------------------------------------------------- */
/* Generator::generate for the generator named in params (generators/mod.rs:82-84): Fast (fast.rs:22-98), Rectilinear
 * (rectilinear.rs:24-60) or InterpolatingRectilinear (interpolating_rectilinear.rs:110-162), with or without scene objects and
 * for any terrain_alpha.  The result is library-allocated host memory — one page-locked block the arrays point into, so the
 * device-to-host copy runs at PCIe speed; release it (as a whole) with atmrt_result_free, which keeps the block for the next frame. */
int atmrt_generate(atmrt_ctx* ctx, atmrt_result_t* out);
void atmrt_result_free(atmrt_result_t* r);
/* Same computation, results left in HBM in caller-provided planes; ray_steps/device_ms optional.  The planes must stay
 * allocated until the next generate call on ctx or until the last atmrt_draw_image* / atmrt_last_hits_device call for this
 * frame, whichever comes first: those read the first-hit planes of an opaque frame in place. */
int atmrt_generate_device(atmrt_ctx* ctx, const atmrt_device_planes_t* planes, uint64_t* ray_steps,
                          double* device_ms);

/* The complete trace-point lists of the frame atmrt_generate_device just produced (translucent terrain, scenes with objects,
 * InterpolatingRectilinear), copied device-to-device into caller-owned arrays laid out like the hit arrays of atmrt_result_t:
 * what a multi-GPU host gathers after the hit_count planes.  dst == NULL only queries *n_hits.  An opaque frame has
 * no list beyond its planes: ATMRT_ERR_STATE. */
typedef struct atmrt_device_hits {
  uint64_t capacity;     /* entries each hit array can hold */
  uint64_t* hit_offset;  /* [H][Wshard] index of each pixel's first trace point */
  double* lat;
  double* lon;
  double* distance;
  double* elevation;
  double* path_length;
  double* normal;        /* [n][3] */
  uint32_t* color_tag;
  double* rgba;          /* [n][4] */
} atmrt_device_hits_t;
int atmrt_last_hits_device(atmrt_ctx* ctx, const atmrt_device_hits_t* dst, uint64_t* n_hits);

/* Device time of each phase of the last atmrt_generate / atmrt_generate_device call, measured with HIP
 * events recorded on the library's own streams (a caller's events on another stream cannot see them). */
typedef struct atmrt_timings {
  double total_ms;     /* first launch to last launch of the call */
  double profile_ms;   /* Fast phase A: k_fast_columns + k_terrain_profile   (utils.rs:176-199) */
  double paths_ms;     /* Fast phase B: k_fast_paths, concurrent with phase A (utils.rs:136-174) */
  double intersect_ms; /* Fast phase C: k_fast_intersect, summed over its segments (they run while later path segments of phase B are integrated) (utils.rs:201-289) */
  double march_ms;     /* Rectilinear: k_rect_march                           (rectilinear.rs:161-185) */
  double finalize_ms;  /* trace-point epilogue: k_fast_finalize / k_rect_finalize */
  double pack_ms;      /* scan + packing / multi-hit fill, when requested */
  uint64_t ray_steps;
  uint64_t n_hits;
  double ceiling_ms;   /* Rectilinear, Spherical calculator: the terrain ceiling table, when this call had to build it (else 0); it is
                          built ahead of the frame's first launch and is not part of total_ms */
} atmrt_timings_t;
/* Environment switches read at every frame (A/B runs; results are the same bits either way):
 *   ATMRT_ESCAPE=off        no ray leaves the Rectilinear march early
 *   ATMRT_STEP_TRIG=off     no per-step sin / cos table of the Spherical geodesic
 *   ATMRT_NORMAL_TRIG=off   no record of the trace-point epilogue's frame constants: every trace point computes them
 *   ATMRT_CEILING=off       no terrain ceiling table: the march tests every sample against the mosaic's highest post
 *   ATMRT_CEILING=rebuild   the terrain ceiling table is built again in every frame (it is cached otherwise) */
int atmrt_last_timings(atmrt_ctx* ctx, atmrt_timings_t* out);

/* How often the last frame left the fast routes of the device path (results are the same either way; tests use this to
 * prove that a workload really exercises the fall-back routes). */
typedef struct atmrt_frame_stats {
  uint64_t unlisted_rays;     /* Rectilinear, scenes with objects: rays with more candidate objects than the per-ray list
                                 holds (24) — they test every object at every sample (is_close, frustum.rs:103-114) */
  uint64_t unlisted_columns;  /* Fast / InterpolatingRectilinear: columns with more candidates than the per-column list (64) */
  uint64_t retraced_pixels;   /* Rectilinear: pixels with more trace points than the 4 slots of the counting pass: their further
                                 points come out of an overflow arena (marched / traced a second time only when the arena is full or
                                 big_steps > 0) */
  uint64_t big_steps;         /* steps that produced more trace points than the in-register step list (12): sorted in HBM */
  uint64_t big_blend_pixels;  /* InterpolatingRectilinear: pixels whose four lattice corners hold more than 4 trace points together
                                 (blended over a member arena in HBM; any number of points) */
  uint64_t terrain_lookups;   /* Rectilinear march: Terrain::get_elev evaluations actually performed.  A sample whose ray is
                                 above the highest post of the mosaic (+ 1 m) is above the terrain for certain, so its geodesic
                                 point and lookup are not evaluated — every ODE step, sign test and result stays the same;
                                 ray_steps keeps counting every step */
  uint64_t object_rays;       /* Rectilinear, scenes with objects: rays left to the general tracer — since round 4 only those of
                                 wavefronts with more candidate objects than the wavefront's list holds (96), or of an earth model
                                 without the geometric pre-filter; every other ray stays with the lean march */
  uint64_t object_steps;      /* Rectilinear, scenes with objects: ray-steps the lean march handed to its out-of-line object step
                                 (the step lies inside a candidate object's distance interval and enters its height band) */
} atmrt_frame_stats_t;
int atmrt_last_stats(atmrt_ctx* ctx, atmrt_frame_stats_t* out);
/* The work of the last frame's Rectilinear march beside its ray_steps.  ray_steps counts every sample pair under the reference's
 * termination rule; a ray that is above the mosaic's top (and the objects' height bands) and provably ascending to max_distance
 * leaves the march early and is credited the steps it did not integrate (the escape certificate).
 * *integrated_steps = the steps actually integrated, *escaped_rays = the rays that left early.  ATMRT_ESCAPE=off in the environment
 * (read at every frame) turns the shortcut off: then *integrated_steps = ray_steps.  A multi-device context sums its devices. */
int atmrt_last_march_work(atmrt_ctx* ctx, uint64_t* integrated_steps, uint64_t* escaped_rays);
/* The escape certificate for an atmosphere, without a device: out[0] = the altitude above which an ascending Rectilinear ray leaves
 * the march (+inf: never), out[1] = the lowest altitude from which (R + h) |dn/dh| / n <= 1/2 holds everywhere above it (refracted
 * spherical stepper; +inf: nowhere), out[2] = the largest value of that bound above out[1].  `top` is the mosaic's top + 1 m. */
int atmrt_escape_certificate(const atmrt_atmosphere_t* atmosphere, double wavelength, int32_t spherical, double radius,
                             int32_t straight, double simulation_step, double top, double out[3]);
/* Fault injection for tests of the error paths: the next atmrt_generate / atmrt_generate_device on ctx runs its kernels and then
 * fails with ATMRT_ERR_HIP (once).  After ANY failed frame atmrt_draw_image* and atmrt_last_hits_device return ATMRT_ERR_STATE
 * until a frame succeeds: the failed frame has already reused the buffers of the one before it. */
int atmrt_debug_fail_next_frame(atmrt_ctx* ctx);
/* How the Rectilinear march of a frame (or column tile) of width x height pixels with `samples` terrain samples per ray
 * (ceil(max_distance / simulation_step)) is planned; no device needed.  out[0] = 1 when the time-sliced march is used (tiles of at
 * most 4 Mpixel without scene objects), out[1] = ray groups, out[2] = the FIFO's capacity in entries, out[3] = bytes
 * of slice state, out[4] = the bound on the slices a ray can need after the first, out[5] = steps per slice. */
int atmrt_debug_march_plan(int32_t width, int32_t height, int32_t samples, int32_t n_objects, uint64_t out[6]);

/* ---- renderer compositing + colouring on the device (src/renderer/mod.rs:367-414, src/coloring) -- */
typedef enum atmrt_coloring_kind { ATMRT_COLORING_SIMPLE = 0, ATMRT_COLORING_SHADING = 1 } atmrt_coloring_kind;
typedef enum atmrt_palette { ATMRT_PALETTE_LEGACY = 0, ATMRT_PALETTE_IMPROVED = 1 } atmrt_palette;
/* `Coloring` (params.rs:216-229) + view.fog_distance (params.rs:305). */
typedef struct atmrt_coloring {
  int32_t kind;          /* atmrt_coloring_kind */
  int32_t palette;       /* enum atmrt_palette; Shading only */
  double water_level;
  double max_distance;   /* Simple: frame.max_distance */
  double ambient_light;  /* Shading */
  double light_dir[3];   /* Shading: unit vector in the world frame */
  int32_t has_fog;       /* view.fog_distance.is_some() */
  int32_t _pad;
  double fog_distance;
} atmrt_coloring_t;
/* ConfColoring::into_coloring (params.rs:231-277): light_zenith_angle / light_dir in degrees, relative to view.frame.direction. */
int atmrt_coloring_from_conf(const atmrt_params_t* params, int32_t kind, double water_level, double ambient_light,
                             double light_zenith_angle, double light_dir, int32_t palette, int32_t has_fog,
                             double fog_distance, atmrt_coloring_t* out);
/* renderer::draw_image for the frame of the last atmrt_generate / atmrt_generate_device call on this context (its trace
 * points are still in HBM): rgb is host memory [height][width][3] of the shard, row-major like ImageBuffer. */
int atmrt_draw_image(atmrt_ctx* ctx, const atmrt_coloring_t* coloring, uint8_t* rgb);
/* Same, into caller-provided device memory (3 B per pixel instead of 88 B per pixel to gather across GPUs). */
int atmrt_draw_image_device(atmrt_ctx* ctx, const atmrt_coloring_t* coloring, uint8_t* rgb_device);

/* ---- the annotations of renderer::output_image (src/renderer/mod.rs:28-365, 416-431) on the device image: azimuth / elevation
 * ticks, the flat-Earth "horizon" line and the eye-level line, drawn over the RGB8 image of atmrt_draw_image*.  Tick labels are
 * text: the library resolves their strings and positions, the host rasterises them (anchors: renderer/mod.rs:292-321). */
typedef enum atmrt_tick_kind { ATMRT_TICK_SINGLE = 0, ATMRT_TICK_MULTIPLE = 1 } atmrt_tick_kind;
/* Tick / VerticalTick, params.rs:325-368. */
typedef struct atmrt_tick {
  int32_t kind;     /* atmrt_tick_kind */
  uint32_t size;    /* length of the tick line [px] */
  double angle;     /* Single: azimuth (ticks) or elevation (vertical_ticks) [deg] */
  double bias;      /* Multiple: ticks at bias + k step inside the frame */
  double step;      /* Multiple: > 0 and finite (the reference would never leave its loop otherwise) */
  int32_t labelled; /* bool */
  int32_t _pad;
} atmrt_tick_t;
/* output.ticks, output.vertical_ticks, output.show_eye_level, output.show_flat_horizon (params.rs:403-410); the arrays are
 * borrowed for the duration of the call. */
typedef struct atmrt_overlay {
  const atmrt_tick_t* ticks;          /* [n_ticks] */
  const atmrt_tick_t* vertical_ticks; /* [n_vertical_ticks] */
  uint32_t n_ticks;
  uint32_t n_vertical_ticks;
  int32_t show_eye_level;    /* bool: the line of elevation 0, colour [255,128,255] */
  int32_t show_flat_horizon; /* bool: drawn only on a flat earth shape with refraction (see atmrt_draw_overlay_device), [0,128,255] */
} atmrt_overlay_t;
#define ATMRT_TICK_LABEL_BYTES 32
/* One tick as it is drawn: a white line (pos, 0) -> (pos, size), or (0, pos) -> (size, pos) when vertical. */
typedef struct atmrt_drawn_tick {
  uint32_t pos;      /* x of a horizontal tick, y of a vertical one */
  uint32_t size;
  int32_t labelled;  /* the host draws `label` at (pos - 8, size + 5), a vertical tick's at (size + 5, pos - 7) */
  int32_t vertical;
  char label[ATMRT_TICK_LABEL_BYTES]; /* format!("{:.1$}", angle, decimals), NUL-terminated (cut to 31 bytes) */
} atmrt_drawn_tick_t;
/* gen_ticks (renderer/mod.rs:227-268) with into_draw_ticks[_vertical], azimuth_to_x, elevation_to_y and round_decimals: host
 * code, no device, ctx-free.  azimuth_row0 is row 0 of the azimuth plane, elevation_col0 column 0 of the elevation plane; their
 * lengths are the image's: params->height and params->width, or the width of the column shard when col_begin / col_end are set
 * — a shard is an image of its own to the overlay, while the ranges of `Multiple` ticks (and the aspect ratio of the vertical
 * ones) keep coming from params->frame and params->width / height.  drawn[0 .. *n_drawn) comes out sorted by (vertical, pos): two
 * definitions that land on one pixel leave the larger size, the earlier one when equal.  drawn == NULL only counts; capacity
 * < *n_drawn, an image narrower or lower than 2 pixels, a step that is not positive and finite, or more than 2^20 ticks of one
 * definition: ATMRT_ERR_INVALID_ARGUMENT. */
int atmrt_overlay_resolve_ticks(const atmrt_params_t* params, const atmrt_overlay_t* overlay, const double* azimuth_row0,
                                const double* elevation_col0, atmrt_drawn_tick_t* drawn, size_t capacity, size_t* n_drawn);
/* draw_ticks, then the flat horizon, then eye level (output_image, renderer/mod.rs:416-431; a later layer overwrites an earlier
 * one) onto rgb_device, [height][width][3] of the frame — or column shard — of the last atmrt_generate / atmrt_generate_device on
 * ctx, whose azimuth / elevation planes are still in HBM: same rules as atmrt_draw_image_device (ATMRT_ERR_STATE without a
 * frame or after a failed one).  Each line takes its row per column from find_elev (:325-343) and joins neighbouring columns with
 * Bresenham segments; pixels outside the image are skipped.  The flat horizon is drawn when show_flat_horizon is
 * set, the earth model's shape is flat (earth_model/mod.rs:95-112) and straight_rays is off, at the elevation
 * degrees(acos(1 / n(observer altitude))): *flat_horizon_deg returns it, NaN when the line is not drawn.  drawn / capacity /
 * n_drawn as above (all three optional).  An image narrower or lower than 2 pixels: ATMRT_ERR_INVALID_ARGUMENT. */
int atmrt_draw_overlay_device(atmrt_ctx* ctx, const atmrt_overlay_t* overlay, uint8_t* rgb_device, atmrt_drawn_tick_t* drawn,
                              size_t capacity, size_t* n_drawn, double* flat_horizon_deg);
/* The same onto a host image (in and out), staged through the context's device. */
int atmrt_draw_overlay(atmrt_ctx* ctx, const atmrt_overlay_t* overlay, uint8_t* rgb, atmrt_drawn_tick_t* drawn, size_t capacity,
                       size_t* n_drawn, double* flat_horizon_deg);
/* The same with explicit [height][width] device planes: the route of a gathered multi-device frame (every device holds the whole
 * planes after atmrt_generate_image_device; pass one device's planes and its image of atmrt_draw_image_gathered_device).  All
 * three pointers must be memory of one device of ctx.  Frame and position are those set on ctx. */
int atmrt_draw_overlay_planes_device(atmrt_ctx* ctx, const atmrt_overlay_t* overlay, const double* azimuth,
                                     const double* elevation_angle, uint32_t width, uint32_t height, uint8_t* rgb_device,
                                     atmrt_drawn_tick_t* drawn, size_t capacity, size_t* n_drawn, double* flat_horizon_deg);

/* ---- the visibility map: the frame's trace points binned over a latitude / longitude grid (no reference counterpart: the
 * reference's `view` window answers "what does this pixel see" one click at a time, viewer/app.rs:112-176; this is the inverse
 * picture — which ground is visible from here, and how far away it is).  One scatter pass over the frame where it lies in HBM. */
/* A regular grid in plain degrees.  Cell (i, j) covers [lat0 + i cell_lat, lat0 + (i + 1) cell_lat) x [lon0 + j cell_lon,
 * lon0 + (j + 1) cell_lon): the south and west edges belong to it, the north and east ones to its neighbour, so the top and right
 * edges of the grid are outside.  There is NO antimeridian handling: longitudes are binned as the plain numbers the generators
 * emit (a frame across +-180 degrees needs two grids). */
typedef struct atmrt_geo_grid {
  double lat0, lon0;          /* south-west corner [deg], finite */
  double cell_lat, cell_lon;  /* cell size [deg], finite and > 0 */
  uint32_t n_lat, n_lon;      /* rows south -> north, columns west -> east; both >= 1, n_lat * n_lon <= 2^31 */
} atmrt_geo_grid_t;
/* The binning rule, host code, ctx-free: fi = floor((lat - lat0) / cell_lat), fj = floor((lon - lon0) / cell_lon) in IEEE
 * arithmetic (numpy's np.floor((lat - lat0) / cell)); inside iff 0 <= fi < n_lat and 0 <= fj < n_lon, compared as doubles, so
 * NaN, infinities and huge values are outside; *cell = i * n_lon + j, or -1 outside.  The kernels run the same function.
 * A grid the rules above refuse: ATMRT_ERR_INVALID_ARGUMENT. */
int atmrt_geo_grid_cell(const atmrt_geo_grid_t* g, double lat, double lon, int64_t* cell);
typedef enum atmrt_visibility_mode {
  ATMRT_VIS_FIRST = 0, /* the first trace point of every pixel, from the dense planes: any frame */
  ATMRT_VIS_ALL = 1    /* every trace point of every pixel, from the packed lists where the frame has them, else as FIRST */
} atmrt_visibility_mode;
/* A trace point whose lat, lon or distance is NaN, or whose distance is negative, is skipped; every other one is looked up in
 * the grid and is either binned or outside: n_points = n_binned + n_outside + n_skipped.  n_updates counts the pairs of atomic
 * updates the kernel issued: within a wavefront (64 consecutive pixels p = y * width + x) a maximal run of consecutive lanes with
 * the same cell makes ONE update carrying the run's point count and smallest distance, and a lane without a binned point ends
 * a run.  ATMRT_VIS_AGGREGATE=off in the environment (read at every call) makes every lane update for itself: the same map,
 * n_updates = n_binned. */
typedef struct atmrt_visibility_stats {
  uint64_t n_points, n_binned, n_outside, n_skipped, n_updates;
} atmrt_visibility_stats_t;
/* Minimum and maximum of lat and lon over the trace points `mode` would look up in a grid (the ones not skipped) of the last
 * frame on ctx: out = {lat_min, lat_max, lon_min, lon_max}, all NaN when there is no such point.  State rules as below. */
int atmrt_frame_bounds(atmrt_ctx* ctx, int32_t mode, double out[4]);
/* The map of the last atmrt_generate / atmrt_generate_device frame on ctx (a column shard is a frame of its own), into
 * caller-owned device memory, overwritten: count [n_lat][n_lon] u32 = binned trace points of the cell, min_distance (may be
 * NULL) [n_lat][n_lon] f64 = the smallest TracePoint.distance among them (-0.0 counts as 0.0), +inf where count is 0.  Integer
 * atomics only, so the map is the same to the bit at every call.  Same rules as atmrt_draw_image_device: ATMRT_ERR_STATE
 * without a frame, after a failed one, and on a multi-device context (use atmrt_visibility_map_planes_device on the gathered
 * planes).  A grid that breaks the rules of atmrt_geo_grid_t, an unknown mode, a NULL count: ATMRT_ERR_INVALID_ARGUMENT. */
int atmrt_visibility_map_device(atmrt_ctx* ctx, const atmrt_geo_grid_t* grid, int32_t mode, uint32_t* count_device,
                                double* min_distance_device, atmrt_visibility_stats_t* stats /* may be NULL */);
/* The same into host arrays, staged through the context's device. */
int atmrt_visibility_map(atmrt_ctx* ctx, const atmrt_geo_grid_t* grid, int32_t mode, uint32_t* count, double* min_distance,
                         atmrt_visibility_stats_t* stats);
/* The same over explicit [height][width] device planes (the route of a gathered multi-device frame: one device's planes of
 * atmrt_generate_image_device), FIRST mode: pixel p has the point (lat[p], lon[p], distance[p]) when hit_count[p] != 0.  All
 * pointers must be memory of one device of ctx. */
int atmrt_visibility_map_planes_device(atmrt_ctx* ctx, const atmrt_geo_grid_t* grid, const double* lat, const double* lon,
                                       const double* distance, const uint32_t* hit_count, uint32_t width, uint32_t height,
                                       uint32_t* count_device, double* min_distance_device, atmrt_visibility_stats_t* stats);

/* ---- landmarks: the nearest trace point of each latitude / longitude (no reference counterpart: the reference's `view` window
 * answers "what does this pixel see" one click at a time, viewer/app.rs:112-176; this inverts it for points — where in the
 * picture is this peak, and is it there at all).  "Not found" does NOT say why: a landmark outside the field of view and one
 * hidden behind terrain both have no trace point near them; telling them apart is the refracted inverse problem, out of scope
 * HERE: the section "sight lines" below solves it, one target at a time, without a frame. */
typedef struct atmrt_landmark {
  double lat, lon;   /* degrees, finite */
  double lon_scale;  /* what a degree of longitude is worth against a degree of latitude at this place: the caller's number (the
                      * host mirrors fill in cos(lat)); finite, 1e-6 <= lon_scale <= 1 */
} atmrt_landmark_t;
/* The rule, host code, ctx-free — the same function the kernels run: dlat = lat - L.lat, dlon = (lon - L.lon) * L.lon_scale,
 * *d2 = dlat * dlat + dlon * dlon, every operation an IEEE operation rounded on its own (no FMA), numpy's expression.  No
 * trigonometry, no antimeridian handling (as the grid has none).  A trace point is WITHIN a landmark iff d2 <= r2, r2 =
 * radius_deg * radius_deg computed once on the host; a NaN d2 is never within.  NULL: ATMRT_ERR_INVALID_ARGUMENT. */
int atmrt_landmark_d2(const atmrt_landmark_t* landmark, double lat, double lon, double* d2);
/* Per landmark: the winner is the within-point with the smallest d2; ties go to the smallest flat pixel index p = y * width + x,
 * ties within a pixel to the smallest point index.  Equal landmarks get equal records, and the record does not depend on the
 * order the wavefronts arrive in (integer atomics only): two calls on one frame return the same bytes. */
typedef struct atmrt_landmark_hit {
  uint32_t n_within;          /* trace points within the radius */
  uint32_t x, y;              /* pixel of the winner in the frame's own coordinates (a column shard counts from its own first
                               * column, as its planes do); UINT32_MAX, UINT32_MAX when n_within == 0 */
  uint32_t point;             /* index of the winning trace point inside its pixel (0 in FIRST mode); 0 when none */
  double d2;                  /* of the winner; +inf when none */
  double distance, elevation; /* TracePoint.distance / .elevation of the winner, bits as the frame holds them; NaN when none */
} atmrt_landmark_hit_t;
/* n_points trace points were read, n_skipped of them skipped exactly as the visibility map skips them (lat, lon or distance NaN,
 * or distance < 0).  n_tested counts the (point, landmark) pairs on which the rule was evaluated: it depends on the filter (a
 * bucket index over the landmarks, built per call on the host; it only ever adds candidates), so only n_tested >= n_within is
 * promised.  n_within is the sum of the landmarks' n_within. */
typedef struct atmrt_landmark_stats {
  uint64_t n_points, n_skipped, n_tested, n_within;
} atmrt_landmark_stats_t;
/* Locates n landmarks (host array in, host array out; 1 <= n <= 2^20) in the last atmrt_generate / atmrt_generate_device frame on
 * ctx, mode as in atmrt_visibility_map (ALL reads the packed lists where the frame has them, else it is FIRST).  State rules of
 * atmrt_visibility_map: ATMRT_ERR_STATE without a frame, after a failed one, and on a multi-device context.  n == 0 or n > 2^20,
 * a NULL array, radius_deg not finite, <= 0 or > 1, a landmark that breaks the rules of atmrt_landmark_t, an unknown mode:
 * ATMRT_ERR_INVALID_ARGUMENT. */
int atmrt_locate_landmarks(atmrt_ctx* ctx, const atmrt_landmark_t* landmarks, size_t n, double radius_deg, int32_t mode,
                           atmrt_landmark_hit_t* hits, atmrt_landmark_stats_t* stats /* may be NULL */);
/* The same over explicit [height][width] device planes (the route of a gathered multi-device frame), FIRST mode: pixel p has the
 * point (lat[p], lon[p], distance[p], elevation[p]) when hit_count[p] != 0.  All planes must be memory of one device of ctx. */
int atmrt_locate_landmarks_planes_device(atmrt_ctx* ctx, const atmrt_landmark_t* landmarks, size_t n, double radius_deg,
                                         const double* lat, const double* lon, const double* distance, const double* elevation,
                                         const uint32_t* hit_count, uint32_t width, uint32_t height, atmrt_landmark_hit_t* hits,
                                         atmrt_landmark_stats_t* stats /* may be NULL */);
/* Where the time of the last atmrt_locate_landmarks* call on ctx went, in milliseconds (tools/measure_landmarks.py): out = {the
 * host's index build (host clock), upload of the index and reset, pass A (counts and smallest d2), pass B (the winner's key),
 * pass C (the records)}, the last four between events on the library's stream. */
int atmrt_last_landmark_timings(atmrt_ctx* ctx, double out[5]);
/* A diagnostic in the spirit of atmrt_math_probe, host only, ctx-free — not a CPU path for the product: builds the bucket index
 * exactly as the library would for a frame with bounds = {lat_min, lat_max, lon_min, lon_max} and returns, for n_points points, the
 * candidate landmarks the filter yields: items[offsets[i] .. offsets[i + 1]) are the indices of point i's candidates.  *n_items is
 * always set to the number of items needed; a capacity below it: ATMRT_ERR_INVALID_ARGUMENT and nothing else written. */
int atmrt_landmark_index_probe(const atmrt_landmark_t* landmarks, size_t n, double radius_deg, const double bounds[4],
                               const double* lat, const double* lon, size_t n_points, uint64_t* offsets /* n_points + 1 */,
                               uint32_t* items, size_t capacity, size_t* n_items);

/* ---- sight lines: at which elevation angle a target appears, and what terrain hides it (no reference counterpart: the refracted
 * inverse problem the landmark search leaves open).  The solve needs the context's parameters, atmosphere and terrain only; it
 * neither needs nor disturbs a generated frame.
 *
 * THE RULE (tests/sight_model.py restates it in numpy).  A target is {azimuth_deg, distance, height}; the setting is what
 * atmrt_set_params / atmrt_set_atmosphere / the terrain say now: observer position and resolved altitude alt (Altitude::abs,
 * params.rs:23-30), earth model, simulation_step, straight_rays.
 *   Sample lattice (the Fast generator's): d_0 = 0, d_i = d_{i-1} + step (repeated addition, utils.rs:191-196); (lat_i, lon_i) =
 *     coords_at_dist(d_i) from the observer along azimuth_deg; T_i = get_elev(lat_i, lon_i), 0 where the terrain has none; m = the
 *     first index with d_m >= distance (m > 65535: invalid argument).
 *   A ray at elevation angle e [deg, converted as atmrt_ray_paths converts]: H_0 = alt, H_i = the stepper's h after i steps of
 *     `step`; c_i = H_i - T_i.  The ray is BLOCKED AT i for the first 1 <= i <= m - 1 with c_{i-1} * c_i < 0.0 (the strict test of
 *     utils.rs:222) or with H_{i-1} < -1000 (utils.rs:167), whichever i is smaller.  Otherwise it ARRIVES:
 *     prop = (distance - d_{m-1}) / (d_m - d_{m-1}), arrival = H_{m-1} + prop * (H_m - H_{m-1}).
 *   Per target: ground = T_{m-1} + prop * (T_m - T_{m-1}), aim = ground + height.  Every operation of these formulas is an IEEE
 *     operation rounded on its own (no FMA).
 *   A FAN over [lo, hi] is 64 angles: delta = (hi - lo) / 63.0, e_k = lo + (double)k * delta (two rounded operations).  Ray k FAILS
 *     iff it is blocked or arrival < aim; a NaN arrival fails.  k* = one above the highest failing ray: 0 if none fails, 64 if
 *     ray 63 fails — an answer even where ducting makes rays cross.
 *   ROUNDS, 1 <= rounds <= 4: if k* is 0 or 64 the solve stops there; otherwise the next fan is [e_{k*-1}, e_{k*}], those very
 *     doubles.
 * Equal targets get equal records; two calls return the same bytes (every NaN of a record is the quiet NaN 0x7ff8000000000000). */
typedef struct atmrt_sight_target {
  double azimuth_deg; /* finite */
  double distance;    /* surface distance [m], finite, > 0 */
  double height;      /* metres above the ground at the target, finite, >= 0 */
} atmrt_sight_target_t;
typedef enum atmrt_sight_status {
  ATMRT_SIGHT_SEEN = 0,      /* the last round's ray k* - 1 arrived, merely low: the aimed point is visible at `angle` to within the last delta */
  ATMRT_SIGHT_HIDDEN = 1,    /* ray k* - 1 was blocked */
  ATMRT_SIGHT_ABOVE_FAN = 2, /* k* == 64: every angle of the fan is too low */
  ATMRT_SIGHT_BELOW_FAN = 3  /* k* == 0: the lowest angle of the fan already passes above the aimed point */
} atmrt_sight_status;
typedef struct atmrt_sight {
  int32_t status;        /* atmrt_sight_status */
  int32_t rounds_done;   /* rounds actually run */
  int32_t m;             /* as defined above */
  int32_t block_index;   /* HIDDEN: the i of ray k* - 1's blocking pair; else -1 */
  double angle;          /* e_{k*} of the last round [deg]; NaN for ABOVE_FAN */
  double arrival;        /* of ray k*; NaN for ABOVE_FAN */
  double ground;         /* as defined above */
  double hidden;         /* arrival - aim: about 0 for SEEN; for HIDDEN the metres above the aimed point that terrain still covers; NaN for ABOVE_FAN */
  double resolution;     /* the last round's delta [deg] */
  double block_distance, block_lat, block_lon, block_elevation; /* HIDDEN: d_i, lat_i, lon_i, T_i of that pair — which ridge; else NaN */
} atmrt_sight_t;
/* One ray of atmrt_sight_fan_probe.  The minimum runs over the c_i the ray has (i <= m - 1, and i <= block_index for a blocked
 * ray), smallest index first: a later c_i replaces it only when it is smaller. */
typedef struct atmrt_sight_ray {
  int32_t block_index;   /* -1: arrived */
  int32_t min_index;
  double arrival;        /* NaN for a blocked ray */
  double min_clearance;
} atmrt_sight_ray_t;
/* The two host halves of the rule, ctx-free — the same functions the kernel's rule is written from.  fan_angles: out[k] = e_k.
 * pick: fails[k] != 0 means ray k fails; *k_star as defined above.  NULL: ATMRT_ERR_INVALID_ARGUMENT. */
int atmrt_sight_fan_angles(double lo, double hi, double out[64]);
int atmrt_sight_pick(const uint8_t fails[64], int32_t* k_star);
/* Solves n targets (host arrays in and out, 1 <= n <= 65536) over the first fan [fan_lo_deg, fan_hi_deg].  One wavefront per
 * target, all rounds inside one kernel; targets are processed in batches so that the call's device scratch (an allocation of the
 * context's own, grown on demand, freed with the context) stays under 256 MB — ATMRT_SIGHT_SCRATCH_BYTES, read at call time,
 * lowers that limit (a test hook: the records do not depend on it).  ATMRT_ERR_INVALID_ARGUMENT: a NULL array, n out of range, a
 * fan that is not finite, not increasing or wider than 180 degrees, rounds outside [1, 4], a target that breaks its rules or lies
 * more than 65535 samples away.  ATMRT_ERR_STATE: before atmrt_set_params, and on a multi-device context. */
int atmrt_sight_lines(atmrt_ctx* ctx, const atmrt_sight_target_t* targets, size_t n, double fan_lo_deg, double fan_hi_deg,
                      int32_t rounds, atmrt_sight_t* out);
/* A diagnostic in the spirit of atmrt_math_probe: the rays of any list of 1 <= n_angles <= 4096 elevation angles against one
 * target, by the device functions the solve runs.  Arguments and states refused as above. */
int atmrt_sight_fan_probe(atmrt_ctx* ctx, const atmrt_sight_target_t* target, size_t n_angles, const double* angles_deg,
                          atmrt_sight_ray_t* rays);
/* Where the time of the last atmrt_sight_lines call on ctx went, in milliseconds between events on the library's stream, summed
 * over its batches: out = {profile pass (upload included), solve, download}. */
int atmrt_last_sight_timings(atmrt_ctx* ctx, double out[3]);
/* The number of batches that call took. */
int atmrt_last_sight_batches(atmrt_ctx* ctx, int32_t* batches);

/* ---- viewshed: for every cell of a polar lattice around the observer, whether a point `height` metres above the ground there is
 * seen, and how many metres are hidden (no reference counterpart).  Like the sight lines it needs the context's parameters,
 * atmosphere and terrain only; it neither needs nor disturbs a generated frame.
 *
 * THE RULE (tests/viewshed_model.py restates it in numpy): the viewshed is, by definition, the FIRST ROUND of the sight-line rule
 * evaluated at every lattice cell.  A call gives az_lo_deg, az_step_deg and 1 <= n_az <= 65536; reach [m], which gives m = the
 * first index with d_m >= reach, 1 <= m <= 65535; height [m] >= 0, the same for every cell; and a fan [fan_lo_deg, fan_hi_deg] of
 * K rays, K a multiple of 64 in [64, 4096].
 *   Azimuths: az_j = az_lo + (double)j * az_step (two rounded operations).
 *   Fan: delta = (hi - lo) / (double)(K - 1), e_k = lo + (double)k * delta; at K = 64 the very doubles of atmrt_sight_fan_angles.
 *   Lattice and profiles: d_i, (lat_{j,i}, lon_{j,i}) and T_{j,i} for 0 <= i <= m are exactly the sight lines' sample lattice for
 *     azimuth az_j (the same device functions produce them).
 *   Ray heights: H_{k,0} = alt, H_{k,i} = the stepper's h after i steps of simulation_step at angle e_k.  A ray is integrated for
 *     all m steps, whatever it meets.  The atmosphere is horizontally uniform: one table serves every azimuth.
 *   Blocking: c = H_{k,i} - T_{j,i}; ray k is blocked against azimuth j at the first i' >= 1 with c_{i'-1} * c_{i'} < 0.0 or
 *     H_{k,i'-1} < -1000.
 *   Cell (j, i), 1 <= i <= m, plays the target {az_j, d_i, height}, whose m is i and whose prop is 1.0; the expressions keep the
 *     sight rule's shape so that the bits agree: arrival_k = H_{k,i-1} + 1.0 * (H_{k,i} - H_{k,i-1}), ground = T_{j,i-1} + 1.0 *
 *     (T_{j,i} - T_{j,i-1}), aim = ground + height.  Ray k FAILS iff it is blocked at some i' <= i - 1 or !(arrival_k >= aim).
 *     k* = one above the highest failing ray: 0 if none fails, K if ray K - 1 fails — an answer even where ducting makes rays cross.
 *   status: ATMRT_SIGHT_ABOVE_FAN when k* = K, BELOW_FAN when k* = 0, HIDDEN when ray k* - 1 is blocked at some i' <= i - 1, SEEN
 *     otherwise.  hidden = arrival_{k*} - aim, NaN for ABOVE_FAN (every NaN is the quiet NaN the sight lines write).  block_index =
 *     the i' of ray k* - 1 when HIDDEN, -1 otherwise.
 * The outputs are planes indexed [j * m + (i - 1)].  Equal calls return equal bytes: the scan uses no atomics and does not depend
 * on the order in which wavefronts arrive. */
typedef struct atmrt_viewshed_spec {
  double az_lo_deg, az_step_deg; /* finite */
  double reach;                  /* [m], finite, > 0 */
  double height;                 /* metres above the ground at every cell, finite, >= 0 */
  double fan_lo_deg, fan_hi_deg; /* finite, increasing, at most 180 degrees apart */
  int32_t n_az;                  /* 1 .. 65536 */
  int32_t fan_rays;              /* K */
} atmrt_viewshed_spec_t;
/* The fan's host half, ctx-free — the same function the kernels run: out[k] = e_k for k < fan_rays.  NULL, a fan_rays that is
 * not a multiple of 64 in [64, 4096] or a bound that is not finite: ATMRT_ERR_INVALID_ARGUMENT. */
int atmrt_viewshed_fan_angles(double lo, double hi, int32_t fan_rays, double* out);
/* A diagnostic in the spirit of atmrt_debug_step_trig, NOT part of the stable surface: the shape of THIS BUILD's scan kernel, so
 * that tests can straddle it.  *az_per_load = the azimuths that share one load of a ray height, *step_tile = the steps between two
 * meetings of a block's wavefronts, *rays_per_lane = the rays a lane owns at fan_rays (0 for a fan_rays the call would refuse).  The
 * values may change with any build; no result of atmrt_viewshed depends on them.  Any pointer may be NULL. */
int atmrt_debug_viewshed_shape(int32_t fan_rays, int32_t* az_per_load, int32_t* step_tile, int32_t* rays_per_lane);
/* m for `reach` under the parameters now set on ctx: what sizes the planes.  Refuses what atmrt_viewshed refuses of reach and state. */
int atmrt_viewshed_steps(atmrt_ctx* ctx, double reach, int32_t* m);
/* The raster into host arrays of n_az * m entries each; block_index, ground, lat and lon are optional (NULL skips one).
 * Three passes: the path table H[i][k] (kept in the context with the key it was built from: atmosphere,
 * observer, terrain, fan, K, m, step, straight_rays, earth — a second call that changes only height or the azimuths does not
 * rebuild it), the azimuths' profiles, and the scan.  Azimuths are processed in batches so that the call's device scratch stays
 * under the sight lines' limit (ATMRT_SIGHT_SCRATCH_BYTES lowers it here too; the planes do not depend on it).
 * ATMRT_ERR_INVALID_ARGUMENT: a NULL spec or required plane, a number that is not finite, n_az, m or fan_rays out of range, a fan
 * that is not increasing or wider than 180 degrees, a negative height, a reach that is not positive, a path table of
 * (m + 1) * K * 8 bytes above the (unlowered) scratch limit of 200 MiB.  ATMRT_ERR_STATE: before atmrt_set_params, and on a
 * multi-device context. */
int atmrt_viewshed(atmrt_ctx* ctx, const atmrt_viewshed_spec_t* spec, uint16_t* k_star, uint8_t* status, double* hidden,
                   int32_t* block_index, double* ground, double* lat, double* lon);
/* The same with the planes written into caller-provided memory of the context's device: no download. */
int atmrt_viewshed_device(atmrt_ctx* ctx, const atmrt_viewshed_spec_t* spec, uint16_t* k_star, uint8_t* status, double* hidden,
                          int32_t* block_index, double* ground, double* lat, double* lon);
/* Where the time of the last viewshed call on ctx went, in milliseconds between events on the library's stream, the last three
 * summed over its batches: out = {path table (0 when it was not rebuilt), profiles (upload included), scan, download}. */
int atmrt_last_viewshed_timings(atmrt_ctx* ctx, double out[4]);
/* The batches that call took, and whether it rebuilt the path table (1) or found it (0). */
int atmrt_last_viewshed_work(atmrt_ctx* ctx, int32_t* batches, int32_t* table_rebuilt);

/* ---- viewshed map: the polar viewshed binned over a latitude / longitude grid on the device (no reference counterpart) — which
 * ground is seen from here, as a raster that lies over a map; accumulated over observers, from how many of them.
 *
 * THE RULE (tests/viewshed_map_model.py restates it in numpy).  A SAMPLE is one lattice cell (j, i) of a viewshed with its status,
 * hidden, lat and lon entries as atmrt_viewshed defines them; a grid is an atmrt_geo_grid_t under its own rules.
 *   The cell of a sample is atmrt_geo_grid_cell(grid, lat, lon): the kernel runs the same function.
 *   Every sample falls into exactly one class.  SKIPPED: lat or lon is NaN, or status > 3.  OUTSIDE: the grid function returns -1.
 *     BINNED: every other sample.  So n_samples = n_binned + n_outside + n_skipped.
 *   Planes, each [n_lat][n_lon], rows south to north:
 *     n_samples (u32): the binned samples of the cell.
 *     n_seen (u32): those of them whose status is ATMRT_SIGHT_SEEN or ATMRT_SIGHT_BELOW_FAN.
 *     min_hidden (f64, may be NULL): the smallest hidden among the cell's binned samples of status SEEN or HIDDEN whose hidden is
 *       not NaN and does not have its sign bit set (-0.0 does not take part); +inf where no sample takes part.  By the viewshed
 *       rule ray k* does not fail, so hidden = arrival - aim >= +0.0 for those statuses: the condition only matters for
 *       atmrt_viewshed_map_planes_device.  The minimum is a u64 minimum on the bit pattern, as the visibility map takes the
 *       minimum of distances.
 *   accumulate == 0: the three planes are overwritten.  accumulate != 0: they must already hold a map on the same grid; counts are
 *     added and the minimum is taken against what is there, so the map of observers A then B accumulated is the cell-wise sum and
 *     minimum of their separate maps.
 *   Integer atomics only (u32 add, u64 min): equal calls give equal bytes, however the call was batched.
 * stats (may be NULL) are of this call only, also under accumulate. */
typedef struct atmrt_viewshed_map_stats {
  uint64_t n_samples, n_binned, n_outside, n_skipped, n_seen;
} atmrt_viewshed_map_stats_t;
/* Any n samples (0 <= n <= (2^31 - 1) * 256) in memory of the context's device: what consumes the planes of atmrt_viewshed_device.
 * The three map planes are device memory too.  Refusals as below. */
int atmrt_viewshed_map_planes_device(atmrt_ctx* ctx, const atmrt_geo_grid_t* grid, size_t n, const uint8_t* status, const double* hidden,
                                     const double* lat, const double* lon, int32_t accumulate, uint32_t* n_samples, uint32_t* n_seen,
                                     double* min_hidden, atmrt_viewshed_map_stats_t* stats);
/* The fused call: the viewshed's three passes per batch of azimuths exactly as atmrt_viewshed batches them — the path table is
 * the same product of the context under the same key — with the scan writing only status, hidden, lat and lon (25 bytes per
 * cell, counted by the batch size) into the call's scratch, and every batch scattered into the map in place of a download.
 * atmrt_last_viewshed_work and atmrt_last_viewshed_timings report this call like a viewshed call; the last timing entry is the
 * scatter.  The map planes are memory of the context's device.
 * ATMRT_ERR_INVALID_ARGUMENT: everything atmrt_viewshed refuses in a spec, a grid atmrt_geo_grid_cell refuses, a NULL spec, grid,
 * n_samples or n_seen (and, for the planes route, a NULL sample plane or an n above its limit).  ATMRT_ERR_STATE: before
 * atmrt_set_params, and on a multi-device context (all three entry points).  A failed call leaves the context usable; with
 * accumulate == 0 it leaves no promise about the planes. */
int atmrt_viewshed_map_device(atmrt_ctx* ctx, const atmrt_viewshed_spec_t* spec, const atmrt_geo_grid_t* grid, int32_t accumulate,
                              uint32_t* n_samples, uint32_t* n_seen, double* min_hidden, atmrt_viewshed_map_stats_t* stats);
/* The same into host arrays, staged through the context's device (under accumulate the arrays are uploaded first). */
int atmrt_viewshed_map(atmrt_ctx* ctx, const atmrt_viewshed_spec_t* spec, const atmrt_geo_grid_t* grid, int32_t accumulate,
                       uint32_t* n_samples, uint32_t* n_seen, double* min_hidden, atmrt_viewshed_map_stats_t* stats);

/* ---- horizon: for every azimuth of a fan, the elevation angle at which terrain ends and sky begins, with refraction, and which
 * ridge forms it (no reference counterpart).  Like the viewshed it needs the context's parameters, atmosphere and terrain only; it
 * neither needs nor disturbs a generated frame.
 *
 * THE RULE (tests/horizon_model.py restates it in numpy).  A call gives az_lo_deg, az_step_deg and 1 <= n_az <= 65536; reach [m],
 * which gives m = the first index with d_m >= reach, 1 <= m <= 65535; a first fan [fan_lo_deg, fan_hi_deg] of K rays, K a multiple
 * of 64 in [64, 4096]; and 1 <= rounds <= 4.
 *   Shared with the viewshed, bit for bit (the same device functions produce them, and the same path table of the context holds the
 *     heights under the same key): the azimuths az_j, the first fan's angles e_k, the lattice d_i, the profiles (lat, lon, T)_{j,i}
 *     for 0 <= i <= m, and the ray heights H_{k,i}.
 *   Blocking: c = H_{k,i} - T_{j,i}; a ray is BLOCKED at the first 1 <= i' <= m with c_{i'-1} * c_{i'} < 0.0 or H_{k,i'-1} < -1000.
 *     i' = m is included (the sight lines' ray stops testing at m - 1).  A ray FAILS iff it is blocked or H_{k,m} is NaN.
 *   Round one, over the K rays of the table: k* = one above the highest failing ray: 0 if none fails, K if ray K - 1 fails — the
 *     highest failing ray, not the first clear one: an answer even where ducting makes rays cross.  k* = K: ATMRT_HORIZON_ABOVE_FAN;
 *     k* = 0: ATMRT_HORIZON_BELOW_FAN; either stops the solve.  Otherwise ATMRT_HORIZON_FOUND with the bracket [e_{k*-1}, e_{k*}].
 *   Rounds 2 to `rounds`: the fan is the sight lines' 64 angles over the bracket [lo, hi], delta = (hi - lo) / 63.0, e_k = lo +
 *     (double)k * delta (atmrt_sight_fan_angles); every ray is integrated by the serial stepper and k* is picked in the same way.
 *     0 < k* < 64: the bracket becomes [e_{k*-1}, e_{k*}].  k* = 0 or 64 (possible only through the last-bit difference between
 *     e_63 and hi): the round is discarded, the bracket stays, the failing ray of record is that round's ray 0 — the same angle as
 *     before, hence the same ray — and the solve stops.
 * Every NaN of a record is the quiet NaN the sight lines write.  Equal calls return equal bytes: the solve uses no atomics and does
 * not depend on the order in which wavefronts arrive. */
typedef enum atmrt_horizon_status {
  ATMRT_HORIZON_FOUND = 0,
  ATMRT_HORIZON_ABOVE_FAN = 2, /* every ray of the first fan fails: the skyline lies above it (ATMRT_SIGHT_ABOVE_FAN's value) */
  ATMRT_HORIZON_BELOW_FAN = 3  /* no ray of the first fan fails: the skyline lies below it (ATMRT_SIGHT_BELOW_FAN's value) */
} atmrt_horizon_status;
typedef struct atmrt_horizon_spec {
  double az_lo_deg, az_step_deg; /* finite */
  double reach;                  /* [m], finite, > 0 */
  double fan_lo_deg, fan_hi_deg; /* the first fan: finite, increasing, at most 180 degrees apart */
  int32_t n_az;                  /* 1 .. 65536 */
  int32_t fan_rays;              /* K */
  int32_t rounds;                /* 1 .. 4 */
} atmrt_horizon_spec_t; /* 56 bytes: four of padding at the end */
typedef struct atmrt_horizon {
  int32_t status;        /* atmrt_horizon_status */
  int32_t rounds_done;   /* rounds run, a discarded one included */
  int32_t k_star;        /* round one's k* */
  int32_t block_index;   /* the i' of the failing ray of record; -1 where it failed by NaN or where there is none */
  double angle_clear;    /* upper end of the last bracket [deg]; e_0 for BELOW_FAN; NaN for ABOVE_FAN */
  double angle_blocked;  /* lower end of the last bracket: the failing ray of record; e_{K-1} for ABOVE_FAN; NaN for BELOW_FAN */
  double resolution;     /* the delta of the round that produced the bracket [deg] */
  double block_distance, block_lat, block_lon, block_elevation; /* d, lat, lon, T at block_index — which ridge; NaN where it is -1 */
} atmrt_horizon_t;
/* A diagnostic like atmrt_debug_viewshed_shape, NOT part of the stable surface: the shape of THIS BUILD's round-one scan, so that
 * tests can straddle it.  *az_per_load = the azimuths that share one load of a ray height, *step_tile = the steps between two
 * looks at whether the wavefront may leave the step loop, *rays_per_lane = the rays a lane owns at fan_rays (0 for a fan_rays the
 * call would refuse).  No result of atmrt_horizon depends on them.  Any pointer may be NULL. */
int atmrt_debug_horizon_shape(int32_t fan_rays, int32_t* az_per_load, int32_t* step_tile, int32_t* rays_per_lane);
/* n_az records into a host array.  The path table H[i][k] is the viewshed's own product under the viewshed's key: a horizon call
 * after a viewshed call of the same fan, K, reach and setting does not rebuild it, nor the reverse.  Then per batch of azimuths
 * (batched as the viewshed batches them; ATMRT_SIGHT_SCRATCH_BYTES lowers the limit here too, and the records do not depend on
 * it): the profiles, the scan of the table (round one), and one wavefront per azimuth for the later rounds and the ridge.
 * ATMRT_ERR_INVALID_ARGUMENT: a NULL spec or array, a number that is not finite, n_az, m, fan_rays or rounds out of range, a fan
 * that is not increasing or wider than 180 degrees, a reach that is not positive, a path table of (m + 1) * K * 8 bytes above the
 * (unlowered) scratch limit of 200 MiB.  ATMRT_ERR_STATE: before atmrt_set_params, and on a multi-device context. */
int atmrt_horizon(atmrt_ctx* ctx, const atmrt_horizon_spec_t* spec, atmrt_horizon_t* out);
/* The same with the records written into caller-provided memory of the context's device: no download. */
int atmrt_horizon_device(atmrt_ctx* ctx, const atmrt_horizon_spec_t* spec, atmrt_horizon_t* out);
/* Where the time of the last horizon call on ctx went, in milliseconds between events on the library's stream, the last four
 * summed over its batches: out = {path table (0 when it was not rebuilt), profiles (upload included), scan, refine, download}. */
int atmrt_last_horizon_timings(atmrt_ctx* ctx, double out[5]);
/* The batches that call took, and whether it rebuilt the path table (1) or found it (0). */
int atmrt_last_horizon_work(atmrt_ctx* ctx, int32_t* batches, int32_t* table_rebuilt);

/* ---- cast shadows: which of a frame's first trace points the light reaches (no reference counterpart: Shading, coloring/shading.rs:
 * 108-112, darkens a slope by the angle between its normal and light_dir and knows nothing of the terrain between the point and
 * the light).  A second march, from every hit pixel toward the light, through the refracting stepper.
 *
 * THE RULE (tests/shadow_model.py restates it in numpy).  A spec is {azimuth_deg: the direction TOWARD the light, elevation_deg:
 * the launch elevation angle of the shadow ray, reach [m] > 0, lift [m] >= 0}; elevation_deg is finite and strictly between -90
 * and 90.  SIMPLIFICATION: azimuth_deg and elevation_deg are taken as the same in the local frame of every surface point.  The
 * true local direction of a light at infinity turns with the point's position by distance / R: up to 1.8 degrees over a frame of
 * 200 km.  The entry points of "shadow lights" below take the direction per point.  The setting is what the context holds NOW: earth model, simulation_step
 * (`step`), straight_rays, atmosphere, terrain.
 *   For pixel p of the last frame with hit_count[p] >= 1 take its FIRST trace point (lat_p, lon_p, elev_p): entry p of the planes,
 *   or entry hit_offset[p] of the lists — whatever the point is, terrain or object: objects receive shadows, they cast none.
 *   Lattice: d_0 = 0, d_i = d_{i-1} + step by repeated addition; m = the first index with d_m >= reach (m > 65535: invalid);
 *     (lat_i, lon_i) = coords_at_dist(d_i) from (lat_p, lon_p) along azimuth_deg, through a DirectionalCalc made at the point
 *     exactly as the reference makes one at the observer; T_i = get_elev(lat_i, lon_i), 0 where the terrain has none.
 *   Ray: H_0 = elev_p + lift (one rounded addition); H_i = the stepper's h after i steps of `step` from H_0 at elevation_deg, as
 *     atmrt_ray_paths returns it; with straight_rays the straight stepper.
 *   SHADOWED at i for the first 1 <= i <= m with H_i < T_i or H_{i-1} < -1000.0 (utils.rs:167), whichever i is smaller; otherwise
 *     LIT.  The point's own sample (i = 0) is deliberately not tested: a trace point is interpolated between two samples and may
 *     lie a hair under the bilinear surface.  A NaN compares false: it never shadows.
 *   Outputs per pixel: status u8 (atmrt_shadow_status), and optionally block u16 = that i for SHADOWED, else 0.
 * Equal calls return equal bytes.  The escape shortcut (ATMRT_SHADOW_ESCAPE=off, read at every call, disables it) only ends rays
 * that are LIT for good: the planes do not depend on it, atmrt_shadow_stats_t's last two counts do. */
typedef struct atmrt_shadow_spec {
  double azimuth_deg;   /* toward the light, finite */
  double elevation_deg; /* finite, in (-90, 90) */
  double reach;         /* [m], finite, > 0 */
  double lift;          /* [m], finite, >= 0 */
} atmrt_shadow_spec_t;
typedef enum atmrt_shadow_status {
  ATMRT_SHADOW_NONE = 0, /* the pixel has no trace point */
  ATMRT_SHADOW_LIT = 1,
  ATMRT_SHADOW_SHADOWED = 2
} atmrt_shadow_status;
/* none + lit + shadowed = the pixels; integrated_steps: the stepper steps taken (a SHADOWED ray its block index, a LIT ray m, or
 * the index at which it passed the escape test); escaped_rays: the LIT rays that passed it before m. */
typedef struct atmrt_shadow_stats {
  uint64_t none, lit, shadowed, integrated_steps, escaped_rays;
} atmrt_shadow_stats_t;
/* m for `reach` under the parameters now set on ctx.  ATMRT_ERR_INVALID_ARGUMENT: NULL, a reach that is not finite and positive,
 * m > 65535.  ATMRT_ERR_STATE: before atmrt_set_params. */
int atmrt_shadow_steps(atmrt_ctx* ctx, double reach, int32_t* m);
/* The status plane (and block, unless NULL) of the last frame of a single-device context, [height][width] as the frame's planes,
 * into memory of the context's device.  stats may be NULL.  The frame stays as it is.  ATMRT_ERR_INVALID_ARGUMENT: NULL, a
 * number that is not finite, elevation_deg outside (-90, 90), reach <= 0, lift < 0, m > 65535.  ATMRT_ERR_STATE: before
 * atmrt_set_params, without a frame, on a multi-device context. */
int atmrt_shadow_mask_device(atmrt_ctx* ctx, const atmrt_shadow_spec_t* spec, uint8_t* status_device, uint16_t* block_device,
                             atmrt_shadow_stats_t* stats);
/* The same into host arrays. */
int atmrt_shadow_mask(atmrt_ctx* ctx, const atmrt_shadow_spec_t* spec, uint8_t* status, uint16_t* block, atmrt_shadow_stats_t* stats);
/* The same over any planes of n_pixels entries in device memory (the first trace point of pixel p is entry p): what a gathered
 * multi-device frame uses, as atmrt_visibility_map_planes_device does; the setting is still the context's. */
int atmrt_shadow_mask_planes_device(atmrt_ctx* ctx, const atmrt_shadow_spec_t* spec, size_t n_pixels, const uint32_t* hit_count,
                                    const double* lat, const double* lon, const double* elev, uint8_t* status_device,
                                    uint16_t* block_device, atmrt_shadow_stats_t* stats);
/* renderer::draw_image exactly as atmrt_draw_image does it, with one exception: under ATMRT_COLORING_SHADING the first trace point
 * of a pixel whose status is ATMRT_SHADOW_SHADOWED takes light_dot = 0.0, so its brightness is exactly ambient_light; later
 * points of a translucent pixel are shaded as before.  Under ATMRT_COLORING_SIMPLE the status plane has no effect.  `status`:
 * [height][width] of the last frame, host memory (_device: memory of the context's device, like rgb_device). */
int atmrt_draw_image_shadowed(atmrt_ctx* ctx, const atmrt_coloring_t* coloring, const uint8_t* status, uint8_t* rgb);
int atmrt_draw_image_shadowed_device(atmrt_ctx* ctx, const atmrt_coloring_t* coloring, const uint8_t* status_device, uint8_t* rgb_device);
/* Where the time of the last shadow call on ctx went, in milliseconds between events on the library's stream:
 * out = {compaction (clear and upload included), march, download (statistics, and the planes of atmrt_shadow_mask)}. */
int atmrt_last_shadow_timings(atmrt_ctx* ctx, double out[3]);

/* ---- shadow lights: a direction per point and a list of lights per call (no reference counterpart) ----------------------------
 * The cast shadows above without their simplification, and for up to 64 lights in one call: a light is a WORLD-FRAME vector, every
 * surface point marches toward each light in that light's own local direction at the point, and the answer is a 64-bit mask per
 * pixel: which lights reach the point.  The atmrt_shadow_mask* calls and their rule stay as they are.
 *
 * THE RULE (tests/shadow_lights_model.py restates it in numpy).
 *   World frame: the frame of EarthModel::world_directions, in which atmrt_coloring_t.light_dir lives: a Shading configuration's
 *     light_dir can be passed as a light unchanged.
 *   A light: three doubles (x, y, z), a vector TOWARD the light, all finite; n2 = x*x + y*y + z*z (summed left to right, every
 *     operation rounded on its own) finite and > 0.  The library normalises once on the host: s = sqrt(n2), L = (x/s, y/s, z/s).
 *   Local direction at a point (lat, lon): (n, e, u) = world_directions(earth, lat, lon); a = dot(L, n), b = dot(L, e),
 *     c = dot(L, u) with dot(p, q) = p.x*q.x + p.y*q.y + p.z*q.z, every operation rounded on its own; c' = c > 1 ? 1 : (c < -1 ? -1 : c)
 *     (a NaN passes through); azimuth_deg = to_degrees(atan2(b, a)), elevation_deg = to_degrees(asin(c')), in the library's
 *     deterministic functions.  atmrt_shadow_local_direction below IS the function the kernel runs.
 *   Per (pixel p with hit_count[p] >= 1, light l), decided without a march, in this order: elevation_deg >= 90: LIT, block 0 (a
 *     height field has nothing straight above a point); otherwise elevation_deg <= -90: SHADOWED, block 1; otherwise elevation_deg
 *     not strictly inside (-90, 90), that is NaN: LIT, block 0.  Such a pair counts 0 integrated steps.
 *   Otherwise the rule of "cast shadows" verbatim with THIS point's azimuth_deg and elevation_deg in place of the spec's: the
 *     lattice d_i and m from reach, the DirectionalCalc at the point, H_0 = elev_p + lift, the stepper, SHADOWED at the first
 *     1 <= i <= m with H_i < T_i or H_{i-1} < -1000.0, otherwise LIT; the escape shortcut and ATMRT_SHADOW_ESCAPE=off as there
 *     (nothing in the certificate depends on the launch elevation), and the planes do not depend on it.
 *   Outputs for 1 <= n_lights <= 64: lit_mask u64 [n_pixels], bit l set iff light l is LIT at p, 0 for a pixel without a trace
 *     point; optionally status u8 [n_lights][n_pixels] (atmrt_shadow_status) and block u16 [n_lights][n_pixels].  At least one of
 *     lit_mask and status is required.
 *   atmrt_shadow_stats_t: none = the pixels without a trace point, counted once; lit + shadowed = hit pixels * n_lights;
 *     integrated_steps and escaped_rays summed over all pairs.
 * Equal calls return equal bytes: a lane owns its pixel's mask and writes it once, the counts are integer sums. */
typedef struct atmrt_shadow_lights_spec {
  const double* dir; /* [n_lights][3], host memory: vectors toward the lights, world frame, any positive length */
  uint32_t n_lights; /* 1 .. 64 */
  uint32_t _pad;
  double reach;      /* [m], finite, > 0 */
  double lift;       /* [m], finite, >= 0 */
} atmrt_shadow_lights_spec_t;
/* Host code, no context and no device.  A light given as the angles under which it is seen from (lat, lon): with (n, e, u) =
 * world_directions there, ce = cos(el), se = sin(el), ca = cos(az), sa = sin(az) of the angles in radians (deg * (pi / 180)),
 * dir[k] = (n[k] * (ce * ca) + e[k] * (ce * sa)) + u[k] * se, every operation rounded on its own.  ATMRT_ERR_INVALID_ARGUMENT: NULL,
 * an unknown earth model, an argument that is not finite, |elevation_deg| > 90. */
int atmrt_shadow_light_direction(const atmrt_earth_model_t* earth, double lat, double lon, double azimuth_deg, double elevation_deg,
                                 double dir[3]);
/* Host code, no context and no device: the light normalised, then the rule's local direction at (lat, lon) — the function the
 * kernel runs.  ATMRT_ERR_INVALID_ARGUMENT: NULL, an unknown earth model, a light the rule refuses. */
int atmrt_shadow_local_direction(const atmrt_earth_model_t* earth, const double dir[3], double lat, double lon, double* azimuth_deg,
                                 double* elevation_deg);
/* The planes of the last frame of a single-device context into memory of the context's device; lit_mask_device, status_device and
 * block_device may each be NULL, but not both of the first two; stats may be NULL.  The frame stays as it is.
 * ATMRT_ERR_INVALID_ARGUMENT: a NULL spec or dir, n_lights of 0 or above 64, a light the rule refuses, reach or lift as
 * atmrt_shadow_mask refuses them, m > 65535, neither lit_mask nor status given.  ATMRT_ERR_STATE: as atmrt_shadow_mask. */
int atmrt_shadow_lights_device(atmrt_ctx* ctx, const atmrt_shadow_lights_spec_t* spec, uint64_t* lit_mask_device, uint8_t* status_device,
                               uint16_t* block_device, atmrt_shadow_stats_t* stats);
/* The same into host arrays, staged through a device buffer of n_pixels * (8 + 3 * n_lights) bytes at most (less where a plane is
 * not asked for). */
int atmrt_shadow_lights(atmrt_ctx* ctx, const atmrt_shadow_lights_spec_t* spec, uint64_t* lit_mask, uint8_t* status, uint16_t* block,
                        atmrt_shadow_stats_t* stats);
/* The same over any planes of n_pixels entries in device memory, as atmrt_shadow_mask_planes_device: what a gathered multi-device
 * frame uses.  atmrt_last_shadow_timings reports all three calls. */
int atmrt_shadow_lights_planes_device(atmrt_ctx* ctx, const atmrt_shadow_lights_spec_t* spec, size_t n_pixels, const uint32_t* hit_count,
                                      const double* lat, const double* lon, const double* elev, uint64_t* lit_mask_device,
                                      uint8_t* status_device, uint16_t* block_device, atmrt_shadow_stats_t* stats);

/* ---- sky rays: the true direction of every sky pixel, sun and moon discs (no reference counterpart) --------------------------
 * A frame's elevation_angle plane holds the LAUNCH elevation of a pixel's ray at the observer.  For a pixel without a trace point
 * (hit_count == 0) this section gives the TRUE (astronomical) elevation: the direction of the ray once it has left the atmosphere,
 * relative to the observer's horizontal; launch - true is the astronomical refraction.  On top of it, discs ("bodies": a sun, a
 * moon) given by their true direction are found in the frame and drawn where the refracted rays meet them — lifted and flattened
 * near the horizon, cut by whatever terrain the frame holds.
 *
 * THE RULE (tests/sky_model.py restates it over the oracle's stepper).
 *   Setting: what the context holds NOW: of the earth model only to_shape (spherical or flat, shape_radius; no calculator, no
 *     geodesic), straight_rays, the atmosphere and the wavelength.  Terrain is not consulted.
 *   A spec is {step [m]: 0 means the context's simulation_step, otherwise finite and > 0; top [m] finite; floor [m] finite and
 *     below top; m: the step cap, 1 <= m <= 1 048 575}.
 *   Ray: stepper_init(h0, to_radians(elevation_deg)); h0 is the observer's altitude of the frame (after Altitude::abs) or the
 *     caller's.  For i = 1 .. m: st = stepper_next(step); the first of these that holds decides the ray, tested in this order:
 *       st.h is NaN: LOST at i;  st.h < floor: GROUND at i;  st.h >= top: EXIT at i.
 *     A ray that no i decides is INSIDE, and its steps is m.  An elevation_deg that is NaN or outside (-90, 90) is LOST at step 0,
 *     without a march.  (The stepper advances in GROUND distance: a ray at 89.9 degrees with a 1000 m step leaps 570 km up in one
 *     step and its height comes out NaN — that is LOST.)
 *   True elevation of an EXIT ray [deg], the stepper state s taken after step i:
 *       straight rays:                 elevation_deg itself, the same bits (the closed-form stepper does not maintain a and b);
 *       refracted rays on a sphere:    to_degrees(atan2(s.b, s.a) - s.x / radius), the division IEEE, every operation rounded once;
 *       refracted rays on a flat earth: to_degrees(atan2(s.b, 1.0)).
 *     Every other status gives NaN.
 *   What bends above `top` is neglected.  Over US-76 on a sphere of 6371 km from h0 = 1 m at step 100 m, the refraction of the
 *     0-degree ray is 0.551189 deg for a top of 60 km, 0.551214 for 84 km, 0.5512150 for 100 km and 0.5512150 for 120 km: 100 km
 *     is a sound default.  The step matters as little (0.551215 at 100 m, 0.551207 at 1000 m, 0.551199 at 5000 m), so the sky
 *     march may take a much longer step than the frame.
 *   Frame: pixel p with hit_count[p] == 0 is a ray of elevation_deg = elevation_angle[p]; a pixel with a trace point gets status
 *     NONE, true elevation NaN and steps 0.  Outputs per pixel: true_elevation f64, status u8 (atmrt_sky_status), optionally steps
 *     u32 (the deciding i; m for INSIDE; 0 for NONE and for LOST at step 0).
 *   Bodies: at most 32 per call, each {azimuth_deg, elevation_deg: TRUE, as seen from the observer with no atmosphere, both finite;
 *     radius_deg in (0, 90); rgb}.  For an EXIT pixel with a = its entry of the frame's azimuth plane and e = its true elevation:
 *     (se, ce) = sincos(to_radians(e)), (sa, ca) = sincos(to_radians(a)), d = (ce * ca, ce * sa, se); the body's u the same way
 *     from its two angles.  The pixel belongs to the FIRST body in list order with d.x * u.x + d.y * u.y + d.z * u.z (summed left
 *     to right, every operation rounded on its own) >= cos(to_radians(radius_deg)).  The body plane holds k + 1 for body k, 0 for
 *     no body and for a pixel that is not EXIT.  Drawing writes the body's rgb over exactly the pixels whose body is not 0; every
 *     other byte of the image stays.  Refraction acts in the vertical plane of the azimuth: the azimuth is the pixel's own.
 * Equal calls return equal bytes: a lane owns its pixel, the counts are integer sums.  The order in which the march takes the list
 * (from its end, where a frame's horizon rows lie: ATMRT_SKY_ORDER=forward, read at every call, takes it from the head) decides
 * scheduling only. */
typedef struct atmrt_sky_spec {
  double step;  /* [m]: 0 = the context's simulation_step, otherwise finite and > 0 */
  double top;   /* [m], finite */
  double floor; /* [m], finite, < top */
  int32_t m;    /* 1 .. 1 048 575 */
  int32_t _pad;
} atmrt_sky_spec_t;
typedef enum atmrt_sky_status {
  ATMRT_SKY_NONE = 0, /* the pixel has a trace point: not a sky pixel */
  ATMRT_SKY_EXIT = 1,
  ATMRT_SKY_GROUND = 2,
  ATMRT_SKY_INSIDE = 3,
  ATMRT_SKY_LOST = 4
} atmrt_sky_status;
typedef struct atmrt_sky_ray {
  int32_t status;        /* atmrt_sky_status */
  uint32_t steps;
  double true_elevation; /* [deg]; NaN unless status is ATMRT_SKY_EXIT */
} atmrt_sky_ray_t;
/* none + exit + ground + inside + lost = the pixels (the list call: none = 0); integrated_steps: the stepper steps taken. */
typedef struct atmrt_sky_stats {
  uint64_t none, exit, ground, inside, lost, integrated_steps;
} atmrt_sky_stats_t;
typedef struct atmrt_sky_body {
  double azimuth_deg;   /* finite */
  double elevation_deg; /* true elevation, finite */
  double radius_deg;    /* in (0, 90) */
  uint8_t rgb[3];
  uint8_t _pad[5];
} atmrt_sky_body_t;
/* Host code, no context and no device: one ray by the function the kernel's lanes run.  spec->step must be > 0 here (there is no
 * context to take it from).  ATMRT_ERR_INVALID_ARGUMENT: NULL, an invalid atmosphere, an unknown earth model, a spec or an h0 the
 * rule refuses.  An elevation_deg that is NaN or outside (-90, 90) is no error: it is LOST at step 0. */
int atmrt_sky_ray_host(const atmrt_atmosphere_t* atmosphere, double wavelength, const atmrt_earth_model_t* earth, int32_t straight_rays,
                       const atmrt_sky_spec_t* spec, double h0, double elevation_deg, atmrt_sky_ray_t* out);
/* Host code, no context and no device: the body rule for one direction.  *body = k + 1 for the first body k that holds the
 * direction, 0 for none.  ATMRT_ERR_INVALID_ARGUMENT: NULL, more than 32 bodies, a body the rule refuses. */
int atmrt_sky_body_host(const atmrt_sky_body_t* bodies, uint32_t n_bodies, double azimuth_deg, double true_elevation_deg, uint32_t* body);
/* The list call, on the device: n rays from h0 at elevation_deg[n] (host arrays, any n), one record each; it also serves as the
 * refraction table.  stats may be NULL.  ATMRT_ERR_INVALID_ARGUMENT: NULL (n > 0), a number of the spec or an h0 that is not
 * finite, step < 0, floor >= top, m outside its range.  ATMRT_ERR_STATE: before atmrt_set_params. */
int atmrt_sky_rays(atmrt_ctx* ctx, const atmrt_sky_spec_t* spec, double h0, size_t n, const double* elevation_deg, atmrt_sky_ray_t* records,
                   atmrt_sky_stats_t* stats);
/* The planes of the last frame of a single-device context, [height][width] as the frame's planes, into memory of the context's
 * device; steps_device and stats may be NULL.  The frame stays as it is.  Refusals as atmrt_sky_rays; ATMRT_ERR_STATE also without
 * a frame and on a multi-device context. */
int atmrt_sky_directions_device(atmrt_ctx* ctx, const atmrt_sky_spec_t* spec, double* true_elevation_device, uint8_t* status_device,
                                uint32_t* steps_device, atmrt_sky_stats_t* stats);
/* The same into host arrays. */
int atmrt_sky_directions(atmrt_ctx* ctx, const atmrt_sky_spec_t* spec, double* true_elevation, uint8_t* status, uint32_t* steps,
                         atmrt_sky_stats_t* stats);
/* The same over any hit_count and elevation_angle planes of n_pixels entries in device memory, from h0: what a gathered multi-device
 * frame uses; the setting is still the context's. */
int atmrt_sky_directions_planes_device(atmrt_ctx* ctx, const atmrt_sky_spec_t* spec, double h0, size_t n_pixels, const uint32_t* hit_count,
                                       const double* elevation_angle, double* true_elevation_device, uint8_t* status_device,
                                       uint32_t* steps_device, atmrt_sky_stats_t* stats);
/* The body plane of the last frame of a single-device context from the planes of atmrt_sky_directions_device and the frame's
 * azimuth plane, into memory of the context's device; rgb_device: NULL, or the [height][width][3] image the discs are drawn into
 * in place.  ATMRT_ERR_INVALID_ARGUMENT: NULL, more than 32 bodies, a number that is not finite, a radius outside (0, 90).
 * ATMRT_ERR_STATE: without a frame, on a multi-device context. */
int atmrt_sky_bodies_device(atmrt_ctx* ctx, const atmrt_sky_body_t* bodies, uint32_t n_bodies, const double* true_elevation_device,
                            const uint8_t* status_device, uint8_t* body_device, uint8_t* rgb_device);
/* The same from and into host arrays (rgb: NULL, or the image, updated in place). */
int atmrt_sky_bodies(atmrt_ctx* ctx, const atmrt_sky_body_t* bodies, uint32_t n_bodies, const double* true_elevation, const uint8_t* status,
                     uint8_t* body, uint8_t* rgb);
/* The same over the caller's planes of n_pixels entries in device memory, the azimuth plane included. */
int atmrt_sky_bodies_planes_device(atmrt_ctx* ctx, const atmrt_sky_body_t* bodies, uint32_t n_bodies, size_t n_pixels, const double* azimuth,
                                   const double* true_elevation_device, const uint8_t* status_device, uint8_t* body_device,
                                   uint8_t* rgb_device);
/* Where the time of the last atmrt_sky_rays / atmrt_sky_directions* call on ctx went, in milliseconds between events on the
 * library's stream: out = {compaction (clear and upload included), march, download (statistics and host planes)}. */
int atmrt_last_sky_timings(atmrt_ctx* ctx, double out[3]);

/* ---- sky light: air mass per sky ray, a reddened sun, a shaded sky (no reference counterpart) -----------------------------------
 * "Sky rays" say where a sky pixel's ray points; this section says how much air it crossed, and colours the sky and the bodies
 * by it.  The refractivity n(h) - 1 = K (p / T) / Z that the stepper differentiates is, for dry air at one wavelength, proportional
 * to density, so its integral along the refracted ray ("column") divided by the same integral taken vertically from a reference
 * altitude ("zenith column") is the relative air mass X.  No atmosphere quantity is needed that the context does not hold.
 *
 * THE RULE (tests/sky_light_model.py restates it over the oracle's stepper and oracle_n).
 *   March: marching, status, steps and true elevation are those of "sky rays", the same bits.  In addition q(h) = n(h) - 1 by the
 *     generic per-layer IEEE evaluation (the oracle's n(h)), for straight rays too.  Start with h_prev = h0, q_prev = q(h0), C = 0.
 *     After every step i whose height st.h is neither NaN nor below the floor (the step that EXITs included, whole):
 *       q_i = q(st.h);  w = (step / radius) * (0.5 * (h_prev + st.h) + radius) on a sphere, w = step on a flat earth;
 *       dh = st.h - h_prev;  C = C + 0.5 * (q_prev + q_i) * sqrt(w * w + dh * dh);  h_prev = st.h, q_prev = q_i
 *     — every operation IEEE and rounded on its own.  The output `column` [m] is C for an EXIT ray, NaN for every other status.
 *   Zenith column Z0(ref_alt, top, dz), host code: K = ceil((top - ref_alt) / dz); nodes ref_alt + k * dz for k < K, the last node
 *     `top` itself; Z0 = the trapezoid 0.5 * (q_prev + q) * (h - h_prev) over the actual node spacings, summed upward.  Refused:
 *     K > 1 048 575, a dz that is not finite and positive, ref_alt >= top, a number that is not finite.  Air mass X = column / Z0.
 *     A light spec is {sky: a spec of "sky rays"; ref_alt [m]; column_dz [m]: 0 means the step of the march}.
 *     US-76 from sea level to 100 km: Z0 = 2.34687220 m with 100 m nodes, 2.34684803 with 10 m, 2.3493 with 1000 m.
 *   Shade, EXIT pixels only (every other byte of the image stays): X = column / zenith_column; per channel c
 *       T_c = exp(-(tau_c * X)).
 *     The pixel's body is that of "sky rays" (the body plane equals atmrt_sky_bodies').  A pixel of body k, with d and u the unit
 *     vectors of the body rule:  chord2 = (d.x - u.x)^2 + (d.y - u.y)^2 + (d.z - u.z)^2, summed left to right;
 *       R2 = 4 * s * s, s = sin(0.5 * to_radians(radius_deg));  m = 1 - chord2 / R2;  mu = sqrt(m) if m > 0, otherwise 0;
 *       limb_c = 1 - u_c * (1 - mu);  v = rgb_c * T_c * limb_c.
 *     A pixel of no body, the airlight:  v = airlight_c * exposure * (1 - T_c).
 *     The byte is 255 if v >= 255, (uint8) v if 0 < v < 255, and 0 otherwise (a NaN too).
 *     Shade parameters {zenith_column finite and > 0; tau[3] finite and >= 0; limb[3] (the u_c) in [0, 1]; exposure finite and
 *     >= 0; airlight rgb}.  The Python and CLI defaults — tau (0.06, 0.11, 0.24), limb (0.5, 0.6, 0.75), exposure 4, a white
 *     airlight: a zenith of about (59, 106, 217), a horizon that saturates to white — are this project's choice.
 *   The airlight does not know where the sun is, and the stepper advances in GROUND distance: at a sky step of 1000 m an 80-degree
 *     ray climbs 5.7 km per step and its trapezoid overestimates the column (against the 100 m step: below 1e-5 up to 5 degrees,
 *     +0.03 % at 30, +0.28 % at 60, +3.2 % at 80; at 100 m the figures agree with Kasten and Young 1989 to 0.2 % from 0.5 to 80
 *     degrees and to 0.8 % at the horizon).  X is about 1 there and the tint hardly moves.
 * Equal calls return equal bytes; the list order of the march (ATMRT_SKY_ORDER) decides scheduling only. */
typedef struct atmrt_sky_light_spec {
  atmrt_sky_spec_t sky;
  double ref_alt;   /* [m] the altitude whose zenith is air mass 1; finite, < sky.top */
  double column_dz; /* [m] node spacing of the zenith column: 0 = the step of the march, otherwise finite and > 0 */
} atmrt_sky_light_spec_t;
typedef struct atmrt_sky_shade {
  double zenith_column; /* [m] Z0, as atmrt_sky_light* and atmrt_sky_zenith_column_host return it; finite, > 0 */
  double tau[3];        /* zenith optical depth per channel, finite, >= 0 */
  double limb[3];       /* limb-darkening coefficient per channel, in [0, 1] */
  double exposure;      /* finite, >= 0 */
  uint8_t airlight[3];
  uint8_t _pad[5];
} atmrt_sky_shade_t;
/* Host code, no context and no device: Z0 by the function the library runs.  ATMRT_ERR_INVALID_ARGUMENT: NULL, an invalid
 * atmosphere, arguments the rule refuses. */
int atmrt_sky_zenith_column_host(const atmrt_atmosphere_t* atmosphere, double wavelength, double ref_alt, double top, double dz, double* zenith_column);
/* Host code: one ray by the function the kernel's lanes run, the record of atmrt_sky_ray_host and the column.  Refusals as there. */
int atmrt_sky_light_ray_host(const atmrt_atmosphere_t* atmosphere, double wavelength, const atmrt_earth_model_t* earth, int32_t straight_rays,
                             const atmrt_sky_spec_t* spec, double h0, double elevation_deg, atmrt_sky_ray_t* out, double* column);
/* Host code: the shade of one EXIT pixel: *body as atmrt_sky_body_host, rgb[3] its bytes.  ATMRT_ERR_INVALID_ARGUMENT: NULL, shade
 * parameters or bodies the rule refuses. */
int atmrt_sky_shade_host(const atmrt_sky_shade_t* shade, const atmrt_sky_body_t* bodies, uint32_t n_bodies, double azimuth_deg,
                         double true_elevation_deg, double column, uint32_t* body, uint8_t* rgb);
/* The list call, on the device: atmrt_sky_rays with column[n] beside the records.  Refusals as there. */
int atmrt_sky_light_rays(atmrt_ctx* ctx, const atmrt_sky_spec_t* spec, double h0, size_t n, const double* elevation_deg, atmrt_sky_ray_t* records,
                         double* column, atmrt_sky_stats_t* stats);
/* atmrt_sky_directions_device with the column plane [height][width] f64 beside the others, and *zenith_column = Z0(spec->ref_alt,
 * spec->sky.top, spec->column_dz) of the context's atmosphere.  steps_device and stats may be NULL.  Refusals as
 * atmrt_sky_directions_device, and what the zenith column refuses. */
int atmrt_sky_light_device(atmrt_ctx* ctx, const atmrt_sky_light_spec_t* spec, double* true_elevation_device, uint8_t* status_device,
                           uint32_t* steps_device, double* column_device, atmrt_sky_stats_t* stats, double* zenith_column);
/* The same into host arrays. */
int atmrt_sky_light(atmrt_ctx* ctx, const atmrt_sky_light_spec_t* spec, double* true_elevation, uint8_t* status, uint32_t* steps, double* column,
                    atmrt_sky_stats_t* stats, double* zenith_column);
/* The same over any hit_count and elevation_angle planes of n_pixels entries in device memory, from h0 (a gathered multi-device frame). */
int atmrt_sky_light_planes_device(atmrt_ctx* ctx, const atmrt_sky_light_spec_t* spec, double h0, size_t n_pixels, const uint32_t* hit_count,
                                  const double* elevation_angle, double* true_elevation_device, uint8_t* status_device, uint32_t* steps_device,
                                  double* column_device, atmrt_sky_stats_t* stats, double* zenith_column);
/* The shade of the last frame of a single-device context: the body plane as atmrt_sky_bodies_device writes it, and the EXIT pixels
 * of the [height][width][3] image rgb_device (not NULL here) shaded in place.  ATMRT_ERR_INVALID_ARGUMENT: NULL, shade parameters
 * or bodies the rule refuses.  ATMRT_ERR_STATE: without a frame, on a multi-device context. */
int atmrt_sky_shade_device(atmrt_ctx* ctx, const atmrt_sky_shade_t* shade, const atmrt_sky_body_t* bodies, uint32_t n_bodies,
                           const double* true_elevation_device, const uint8_t* status_device, const double* column_device, uint8_t* body_device,
                           uint8_t* rgb_device);
/* The same from and into host arrays. */
int atmrt_sky_shade(atmrt_ctx* ctx, const atmrt_sky_shade_t* shade, const atmrt_sky_body_t* bodies, uint32_t n_bodies, const double* true_elevation,
                    const uint8_t* status, const double* column, uint8_t* body, uint8_t* rgb);
/* The same over the caller's planes of n_pixels entries in device memory, the azimuth plane included. */
int atmrt_sky_shade_planes_device(atmrt_ctx* ctx, const atmrt_sky_shade_t* shade, const atmrt_sky_body_t* bodies, uint32_t n_bodies, size_t n_pixels,
                                  const double* azimuth, const double* true_elevation_device, const uint8_t* status_device,
                                  const double* column_device, uint8_t* body_device, uint8_t* rgb_device);
/* atmrt_last_sky_timings reports the atmrt_sky_light* calls as it reports atmrt_sky_directions*.  The last atmrt_sky_shade* call on
 * ctx: *ms = the milliseconds of its kernel between events on the library's stream. */
int atmrt_last_sky_shade_timing(atmrt_ctx* ctx, double* ms);

/* ---- apparent elevation: the inverse of the sky march, and shadow lights given by their TRUE direction (no reference counterpart)
 * "Sky rays" turn a LAUNCH elevation into the TRUE elevation of the ray outside the atmosphere.  This section is the inverse: for a
 * point at altitude h and a body (a light) at local true elevation t, the launch elevation whose ray leaves the atmosphere at t —
 * where the body APPEARS.  It is read from a refraction table over (altitude x launch elevation) that the context builds once per
 * setting and keeps on the device.  With it the shadow lights can be given by their true (astronomical) direction, as the bodies of
 * "sky rays" are: atmrt_shadow_lights* launch a shadow ray at the light's geometric local elevation, and that ray leaves the
 * atmosphere up to 0.55 degrees BELOW the light; atmrt_shadow_lights_true* launch it at the apparent elevation.
 *
 * THE RULE (tests/sky_apparent_model.py restates it in Python floats, every operation rounded on its own, no fma).
 *   Table spec: {sky: a spec of "sky rays" (step 0 = the context's simulation_step); alt_lo < alt_hi [m]; -90 < el_lo < el_hi < 90
 *     [deg]; 2 <= n_alt <= 1024; 2 <= n_el <= 65536; n_alt * n_el <= 2^24}, all numbers finite.
 *   Lattice: dh = (alt_hi - alt_lo) / (n_alt - 1), h_j = alt_lo + j * dh; de = (el_hi - el_lo) / (n_el - 1), e_k = el_lo + k * de.
 *   S[j][k] and T[j][k]: status and true elevation of the "sky rays" rule for the ray (h0 = h_j, elevation_deg = e_k) in the
 *     context's setting; T is NaN unless S is EXIT.
 *   tail[j]: the smallest k0 such that every entry k0 .. n_el - 1 of row j is EXIT and T[j][k] < T[j][k + 1] for every
 *     k0 <= k <= n_el - 2; n_el when the row's last entry is not EXIT.  A row is USABLE iff tail[j] <= n_el - 2.
 *   The inverse uses the monotone tail only.  LIMITATION: under a duct the tail starts above the trapped (GROUND, INSIDE or
 *     non-monotone) rays; a light below T[j][tail[j]] is treated by the first arm below, as if the refraction of the lowest tail ray
 *     held for everything under it.  The non-monotone part of a ducted table is not inverted.
 *   row(j, t), with k0 = tail[j], L = n_el - 1:
 *       t is NaN:        NaN;
 *       t < T[j][k0]:    t + (e_k0 - T[j][k0])  (the refraction of the lowest tail ray held constant; the shadow march then decides,
 *                        as it does for a light under the horizon);
 *       t > T[j][L]:     t + (e_L - T[j][L]);
 *       otherwise:       k = the smallest index in (k0, L] with T[j][k] >= t (found by bisection: the tail is strictly increasing),
 *                        w = (t - T[j][k-1]) / (T[j][k] - T[j][k-1]) (IEEE division), row = e_{k-1} + w * (e_k - e_{k-1}).
 *   apparent(h, t): u = (h - alt_lo) / dh; a NaN u gives NaN; u clamped to [0, n_alt - 1]; j = min((int)floor(u), n_alt - 2);
 *     f = u - j; a = row(j, t), b = row(j + 1, t); apparent = a + f * (b - a).
 *   With straight_rays the apparent elevation is t itself, the same bits, and no table is consulted (atmrt_sky_apparent and the
 *     shadow calls; the table is still built, and every T[j][k] of it is e_k).
 *   Closure: over US-76 on the 6371 km sphere (sky step 1000 m, top 100 km), de = 0.02 deg and rows 281.25 m apart, the inverted
 *     elevation marched by the exact route leaves the atmosphere within 1.1e-4 deg of the target (has the
 *     measured figures); on a flat earth next to the lowest exiting ray the error reaches 1.1e-2 deg: no bound is given there.
 *   TRUE-DIRECTION SHADOW LIGHTS: the rule of "shadow lights" verbatim with one insertion after the local direction: when
 *     elevation_deg is strictly inside (-90, 90), elevation_deg := apparent(H_0, elevation_deg) with H_0 = elev_p + lift, the value
 *     the march starts from.  The three no-march tests then look at the new value; the lattice, the DirectionalCalc, the stepper at
 *     the context's simulation_step, the block rule and the escape shortcut are unchanged.  Outputs and stats are those of
 *     atmrt_shadow_lights.  A table with a row that is not usable is refused.
 * Equal calls return equal bytes. */
typedef struct atmrt_sky_table_spec {
  atmrt_sky_spec_t sky;
  double alt_lo, alt_hi; /* [m], finite, alt_lo < alt_hi */
  double el_lo, el_hi;   /* [deg], -90 < el_lo < el_hi < 90 */
  uint32_t n_alt;        /* 2 .. 1024 */
  uint32_t n_el;         /* 2 .. 65536; n_alt * n_el <= 2^24 */
} atmrt_sky_table_spec_t;
/* Builds the table of the context's setting NOW, or finds it: the table, its status plane and tail stay on the device under the key
 * of everything the rule reads (atmosphere, wavelength, earth shape and radius, straight_rays, the spec with its step resolved); a
 * later call with an equal key finds them, a changed key rebuilds them.  true_elevation [n_alt][n_el], status [n_alt][n_el],
 * tail [n_alt]: host arrays, each may be NULL; stats (of the march that built the table; none = 0) may be NULL.  It succeeds with
 * unusable rows, so that they can be looked at.  ATMRT_ERR_INVALID_ARGUMENT: NULL, a spec the rule refuses.  ATMRT_ERR_STATE: before
 * atmrt_set_params. */
int atmrt_sky_table(atmrt_ctx* ctx, const atmrt_sky_table_spec_t* spec, double* true_elevation, uint8_t* status, uint32_t* tail,
                    atmrt_sky_stats_t* stats);
/* Host code, no context and no device: tail[n_alt] of the caller's planes, by the function the kernel's rule states.
 * ATMRT_ERR_INVALID_ARGUMENT: NULL, a spec the rule refuses. */
int atmrt_sky_tail_host(const atmrt_sky_table_spec_t* spec, const double* true_elevation, const uint8_t* status, uint32_t* tail);
/* Host code, no context and no device: apparent(h, t) over the caller's table, by the function the kernels run.
 * ATMRT_ERR_INVALID_ARGUMENT: NULL, a spec the rule refuses, a tail entry that says its row is not usable (or lies above n_el). */
int atmrt_sky_apparent_host(const atmrt_sky_table_spec_t* spec, const double* true_elevation, const uint32_t* tail, double h, double t,
                            double* apparent);
/* The list call, on the device: where a body of true elevation t[i] appears from altitude h[i] (host arrays, any n); the table is
 * built or found as by atmrt_sky_table.  ATMRT_ERR_INVALID_ARGUMENT: NULL (n > 0), a spec the rule refuses, a table with an unusable
 * row (atmrt_last_error names the first).  ATMRT_ERR_STATE: before atmrt_set_params. */
int atmrt_sky_apparent(atmrt_ctx* ctx, const atmrt_sky_table_spec_t* spec, size_t n, const double* h, const double* t, double* apparent);
/* The three routes of atmrt_shadow_lights* under the true-direction rule: the same arguments and one more, the table's spec.
 * Refusals: those of atmrt_shadow_lights* and of atmrt_sky_apparent.  atmrt_last_shadow_timings reports them (the table's build is
 * not part of those: atmrt_last_sky_table_work has it). */
int atmrt_shadow_lights_true_device(atmrt_ctx* ctx, const atmrt_shadow_lights_spec_t* spec, const atmrt_sky_table_spec_t* table,
                                    uint64_t* lit_mask_device, uint8_t* status_device, uint16_t* block_device, atmrt_shadow_stats_t* stats);
int atmrt_shadow_lights_true(atmrt_ctx* ctx, const atmrt_shadow_lights_spec_t* spec, const atmrt_sky_table_spec_t* table, uint64_t* lit_mask,
                             uint8_t* status, uint16_t* block, atmrt_shadow_stats_t* stats);
int atmrt_shadow_lights_true_planes_device(atmrt_ctx* ctx, const atmrt_shadow_lights_spec_t* spec, const atmrt_sky_table_spec_t* table,
                                           size_t n_pixels, const uint32_t* hit_count, const double* lat, const double* lon, const double* elev,
                                           uint64_t* lit_mask_device, uint8_t* status_device, uint16_t* block_device, atmrt_shadow_stats_t* stats);
/* What the last call on ctx that needed the table did for it: *rebuilt = 1 when it built the table, 0 when it found it;
 * ms = {march, tail, download (the host arrays of atmrt_sky_table and the tail the library reads)} in milliseconds between events
 * on the library's stream; march and tail are 0 when the table was found. */
int atmrt_last_sky_table_work(atmrt_ctx* ctx, int32_t* rebuilt, double ms[3]);

/* ---- several GPUs of one node --------------------------------------------------------------------------------
 * The reference calls `generator.generate()` ONCE per frame (src/generator/mod.rs:72-86, trait at generators/mod.rs:82-84), so the
 * multi-GPU path lives BELOW this ABI: pixels are independent (rectilinear.rs:32-37), the image is cut into pixel-column tiles —
 * device / rank g of G computes columns [g W / G, (g + 1) W / G) of every row against its own copy of the terrain mosaic — and the
 * only exchange is the finished frame.  Two ways to get there, same code underneath:
 *
 *  (1) ONE PROCESS, SEVERAL DEVICES: atmrt_ctx_create_multi(devices, n) returns a context that every entry point of this header
 *      accepts.  Each device gets a sub-context and a host thread.  atmrt_generate returns the whole [H][W] frame in host memory:
 *      every device copies its tile straight into the one page-locked block (strided device-to-host copies over its own PCIe
 *      link; no collective, the consumer being the host).  atmrt_generate_image_device leaves the whole frame in the HBM of EVERY
 *      device: one ncclAllGather (RCCL over xGMI) of the tiles' planes + a permutation kernel into the [H][W] planes.
 *  (2) ONE PROCESS PER GPU (torchrun, MPI): every rank creates a plain context, rank 0 obtains atmrt_comm_unique_id and hands it to
 *      the others through whatever the launcher offers, every rank calls atmrt_ctx_comm_init_rank (which also runs the
 *      communicator's first collective, a probe with a time-out, so that a fabric that does not work is an error HERE, where the
 *      host can still take atmrt_ctx_comm_init_external*); atmrt_generate_image_device is then collective over the ranks.  atmrt_generate / atmrt_generate_device on such a context return the rank's own tile.
 *
 * Frames whose pixels hold several trace points (terrain_alpha < 1, scene objects, InterpolatingRectilinear) also exchange the
 * variable-length lists: atmrt_image_hits_device (count -> scan -> offset on the device, one all-gather of the lists).
 * RCCL is resolved with dlopen("librccl.so.1") on first use: a process that already carries one under that SONAME (PyTorch's
 * bundled librccl) shares it — one RCCL, one HIP runtime per process — any other finds ROCm's through the library's RUNPATH. */
#define ATMRT_COMM_ID_BYTES 128
/* ncclGetUniqueId: 128 opaque bytes for the other ranks' atmrt_ctx_comm_init_rank. */
int atmrt_comm_unique_id(uint8_t id[ATMRT_COMM_ID_BYTES]);
/* Joins this context (one device) to `world` ranks that share every frame from now on: ncclCommInitRank, collective over the
 * ranks.  Parameters keep describing the WHOLE image (col_begin = col_end = 0). */
int atmrt_ctx_comm_init_rank(atmrt_ctx* ctx, const uint8_t id[ATMRT_COMM_ID_BYTES], int32_t rank, int32_t world);
/* The same with the host's own transport in place of RCCL (an MPI all-gather without GPU awareness, a shared-memory ring, gloo,
 * a test double): the callback must deliver, on every rank, rank i's `bytes_per_rank` bytes at recv_host + i * bytes_per_rank and
 * return 0.  Both pointers are page-locked HOST memory owned by the library, which stages the tile out of and the gathered
 * tiles back into HBM around the call. */
typedef int (*atmrt_all_gather_fn)(void* user, const void* send_host, void* recv_host, size_t bytes_per_rank);
int atmrt_ctx_comm_init_external(atmrt_ctx* ctx, int32_t rank, int32_t world, atmrt_all_gather_fn all_gather, void* user);
/* The same for a transport that moves DEVICE memory itself (a GPU-aware MPI, another RCCL communicator the host already owns):
 * both pointers are in this context's HBM; the library's stream has drained when the callback is entered and the gathered bytes
 * must be in place when it returns. */
typedef int (*atmrt_all_gather_device_fn)(void* user, const void* send_device, void* recv_device, size_t bytes_per_rank);
int atmrt_ctx_comm_init_external_device(atmrt_ctx* ctx, int32_t rank, int32_t world, atmrt_all_gather_device_fn all_gather, void* user);
/* One context over n_devices HIP devices of this process (1): terrain, parameters, atmosphere and objects set on it reach every
 * device.  A device may be listed more than once (its tiles then are exchanged by device-to-device copies; RCCL needs distinct
 * devices).  ATMRT_GATHER=peer forces that route, ATMRT_GATHER=rccl makes a failure to set RCCL up an error instead of a fallback. */
int atmrt_ctx_create_multi(atmrt_ctx** out, const int32_t* devices, int32_t n_devices);
/* 1 for a plain context, n_devices for a multi-device one. */
int atmrt_ctx_device_count(const atmrt_ctx* ctx);
/* Generator::generate with the WHOLE frame left in HBM: `image` holds one set of [H][W] planes per device of the context (a plain
 * or rank context: one; a multi-device context: device_count sets, entry i in the memory of devices[i]; a set whose azimuth
 * pointer is NULL is skipped).  ray_steps: of this rank (rank context) / of all devices (multi-device context). */
int atmrt_generate_image_device(atmrt_ctx* ctx, const atmrt_device_planes_t* image, uint64_t* ray_steps, double* device_ms);
/* The complete trace-point lists of that frame in the image's pixel order p = y W + x — atmrt_last_hits_device for the whole
 * image — on every device: `dst` like `image` above (entry i on devices[i]; hit_offset is [H][W]).
 *   dst == NULL: only *n_hits, the image's total — every rank has known it since the frame's own collective (each tile's slab
 *     carries its count): no communication, any rank may ask at any time.
 *   dst != NULL: COLLECTIVE — every rank of the frame (every device of a multi-device context: one entry each) must make the
 *     call; ONE all-gather of the packed lists, then count -> scan -> offset on the device.  A rank (or device entry) that wants
 *     nothing for itself passes hit_offset == NULL and still takes part.  A rank's own mistake (capacity < *n_hits, a NULL array
 *     while the image has trace points, no image planes assembled on it) is reported to that rank AFTER it has taken part, so
 *     the others never wait for it.  An image without a single trace point has no collective at all: hit_offset is zero-filled,
 *     the list arrays are not touched and may be NULL.
 * Frames without lists (opaque terrain, no objects, not InterpolatingRectilinear): ATMRT_ERR_STATE on every rank. */
int atmrt_image_hits_device(atmrt_ctx* ctx, const atmrt_device_hits_t* dst, uint64_t* n_hits);
/* renderer::draw_image of every tile + an all-gather of the 3 B/pixel RGB8 tiles instead of the 84 B/pixel planes: rgb_device[i]
 * is [H][W][3] on devices[i] (NULL entries skipped). */
int atmrt_draw_image_gathered_device(atmrt_ctx* ctx, const atmrt_coloring_t* coloring, uint8_t* const* rgb_device);
/* What the exchange of the last atmrt_generate_image_device / atmrt_generate (multi-device) cost, from HIP events on the
 * library's streams (slowest device). */
typedef enum atmrt_gather_route {
  ATMRT_ROUTE_NONE = 0,     /* one device: nothing to exchange */
  ATMRT_ROUTE_RCCL = 1,     /* ncclAllGather over xGMI */
  ATMRT_ROUTE_PEER = 2,     /* device-to-device copies inside one process */
  ATMRT_ROUTE_EXTERNAL = 3, /* the host's transport (atmrt_ctx_comm_init_external) */
  ATMRT_ROUTE_HOST = 4,     /* atmrt_generate on a multi-device context: strided copies into the host block */
  ATMRT_ROUTE_EXTERNAL_DEVICE = 5 /* the host's device-memory transport (atmrt_ctx_comm_init_external_device) */
} atmrt_gather_route;
typedef struct atmrt_comm_timings {
  double gather_ms;         /* the collective (or the copies) */
  double assemble_ms;       /* permutation of the gathered tiles into the [H][W] planes (route HOST: the merge of the lists on the host threads, wall clock) */
  double tile_ms_max;       /* slowest device's generate time */
  double tile_ms_min;       /* fastest device's */
  uint64_t bytes_per_rank;  /* what each rank contributed to the collective */
  int32_t world;
  int32_t route;            /* atmrt_gather_route */
  int32_t collectives;      /* data-path collectives of the last frame (1 for an image, + 1 for its lists) */
  int32_t _pad;
} atmrt_comm_timings_t;
int atmrt_last_comm_timings(atmrt_ctx* ctx, atmrt_comm_timings_t* out);
/* 1 when RCCL can be loaded in this process (no device work, not collective): what every rank of a launcher checks — and agrees
 * on — BEFORE any of them enters the collective atmrt_ctx_comm_init_rank. */
int atmrt_comm_available(void);
/* The pixel columns [*col_begin, *col_end) of a tile: of the last frame that was exchanged, else of the next one.  A multi-device
 * context: of device `index`; a rank context: of rank `index` (index < 0: its own); a plain context: its whole width or shard.
 * Tiles start equal (rank g of G: [g W / G, (g + 1) W / G), inner boundaries on multiples of 64 columns when tiles are at least 128
 * wide) and are RE-CUT by the library after a frame whose slowest tile took
 * more than 1 % longer than the mean — every rank from the same gathered tile times, so all agree without a message
 * (ATMRT_TILE_BALANCE=0 keeps them equal; 1 forces re-cutting where it is off by default: devices listed twice, the host-buffer
 * transport). */
int atmrt_ctx_tile_columns(atmrt_ctx* ctx, int32_t index, int32_t* col_begin, int32_t* col_end);
/* The re-cutting rule itself, a pure function: cols (n_tiles + 1 ascending boundaries, 0 .. width) and each tile's time ->
 * boundaries that would have equalised the times had the cost per column been constant inside each tile, on multiples of 64 columns
 * (a wavefront of the marching kernels is 64 consecutive pixels: tiles whose width is not a multiple of 64 march 15 % slower) when
 * every tile is at least 128 wide; cols_out = cols when the re-cut would not shorten the slowest tile by 1 % under that model. */
int atmrt_tiles_rebalance(int32_t width, int32_t n_tiles, const int32_t* cols, const double* tile_ms, int32_t* cols_out);
/* Test hooks.  set_tiling: the next frames use exactly these n = world + 1 boundaries (NULL: back to the library's own); on a
 * rank context every rank must be given the same.  fail_next_collective: the nth data-path collective from now (1 = the next)
 * fails on device `index` of a multi-device context / on this rank — before it is enqueued, as a refused ncclAllGather would. */
int atmrt_debug_set_tiling(atmrt_ctx* ctx, const int32_t* cols, int32_t n);
int atmrt_debug_fail_next_collective(atmrt_ctx* ctx, int32_t index, int32_t nth);

/* ---- integrator / sampler harnesses (the reference's diagnostic subcommands) ---------------- */
/* output-ray-paths (src/ray_path.rs:65-103): for each elevation angle [deg] step the ray n_steps
 * times from height h0 with `step` metres; x and h are [n_angles][n_steps+1] including the start. */
int atmrt_ray_paths(atmrt_ctx* ctx, double h0, size_t n_angles, const double* angles_deg, int32_t straight,
                    double step, size_t n_steps, double* x, double* h);
/* output-atm (src/atm_printer.rs:37-46): T [K], p [Pa], refractive index n and dn/dh at altitudes. */
int atmrt_atmosphere_sample(atmrt_ctx* ctx, size_t n, const double* altitude, double* temperature,
                            double* pressure, double* n_index, double* dn_dh);
/* DirectionalCalc::coords_at_dist (directional_calc.rs:5-7) for the context's earth model. */
int atmrt_coords_at_dist(atmrt_ctx* ctx, double lat0, double lon0, double dir_deg, size_t n, const double* dist,
                         double* lat, double* lon);

/* ---- the metadata file (src/generator/mod.rs:20-45, read back by src/viewer/mod.rs:17-29) -------- */
/* bincode-1 encoding of `result: Vec<Vec<ResultPixel>>` exactly as serde derives it (generators/mod.rs:13-49): u64 lengths,
 * u32 enum tags, f64 little-endian; layout in csrc/atmrt_metadata.hip.  vector3_len_prefix != 0 writes nalgebra's Vector3 as a
 * sequence (u64 3 + 3 f64, what nalgebra 0.32's ArrayStorage serializer is believed to emit; crate absent, UNPINNED), 0 as
 * three bare f64.  Host-only functions (no device work, callable without a GPU).  dst == NULL queries *n_bytes. */
int atmrt_result_encode_bincode(const atmrt_result_t* r, int32_t vector3_len_prefix, uint8_t* dst, size_t capacity,
                                size_t* n_bytes);
/* The inverse: `out` is library-allocated (release with atmrt_result_free); *consumed = bytes read from src.  Rows of unequal
 * length, an unknown PixelColor tag or a truncated buffer give ATMRT_ERR_FORMAT. */
int atmrt_result_decode_bincode(const uint8_t* src, size_t n_bytes, int32_t vector3_len_prefix, atmrt_result_t* out,
                                size_t* consumed);

/* The deterministic elementary functions of the device path (csrc/detmath.h), element-wise on host arrays: the same
 * instruction sequences the marching kernels execute.  The bit-exactness claim of this library rests on them returning, on
 * gfx950, exactly what the host build of detmath.h returns (and, for DIV / DIV_R / SQRT_INRANGE, what IEEE division and square
 * root return inside their documented operand range); tests/test_gpu_detmath.py checks that on 1e7 operands per function.
 * b may be NULL for one-operand functions, out1 may be NULL unless op is SINCOS or POW3. */
typedef enum atmrt_math_probe_op {
  ATMRT_PROBE_DIV = 0,          /* dm_div(a, b): division without the range scaling / fix-up steps */
  ATMRT_PROBE_DIV_R = 1,        /* dm_div_r(a, b, RN(1/b)): division by a tabulated reciprocal */
  ATMRT_PROBE_SQRT_INRANGE = 2, /* dm_sqrt_inrange(a) */
  ATMRT_PROBE_EXP = 3,
  ATMRT_PROBE_LOG = 4,
  ATMRT_PROBE_POW = 5,          /* dm_pow(a, b) */
  ATMRT_PROBE_SINCOS = 6,       /* out0 = sin, out1 = cos */
  ATMRT_PROBE_ASIN = 7,
  ATMRT_PROBE_ATAN2 = 8,        /* dm_atan2(a, b) */
  ATMRT_PROBE_IEEE_DIV = 9,     /* the compiler's a / b */
  ATMRT_PROBE_IEEE_SQRT = 10,   /* the compiler's sqrt(a) */
  ATMRT_PROBE_ATAN = 11,
  ATMRT_PROBE_TAN = 12,
  ATMRT_PROBE_POW3 = 13,        /* out0 = dm_pow(a, b) through the three-point form of the stepping kernels; out1 = sum of
                                   the other two points (a * 0.99999981, a * 1.00000019) */
  ATMRT_PROBE_DIV3 = 14,        /* dm_div3: out0 = a / (b (1 - 2^-22)), out1 = a / (b (1 + 2^-21)), both with their reciprocal seeded
                                   from b's; the centre quotient a / b is ATMRT_PROBE_DIV's */
  ATMRT_PROBE_DIV3_SEEDED = 15, /* dm_div3_seeded without a seed for b (the p / T site of a tight atmosphere segment): the DIV3 outputs
                                   for divisors b (1 -+ 2^-22), no vote */
  ATMRT_PROBE_DIV3_SEED_Z = 16, /* dm_div3_seeded with b = Z close to 1 (|1 - Z| <= 2^-10.5) and 2 - Z as the seed of its reciprocal:
                                   out0 = a / b, out1 = a / (b (1 + 2^-22)) */
  ATMRT_PROBE_DIV_SEED_N = 17,  /* dm_div_seeded(a, 1 + b, 1 - b) for 0 <= b <= 2^-10.5: a / n with n = 1 + (n - 1) */
  ATMRT_PROBE_POW3_SHARED = 18  /* the three-point pow of a TIGHT segment (shared table rows, csrc/detmath.h): out0 = dm_pow(a, b),
                                   out1 = dm_pow(a (1 - 2^-22), b) + dm_pow(a (1 + 2^-22), b) */
} atmrt_math_probe_op;
int atmrt_math_probe(atmrt_ctx* ctx, int32_t op, size_t n, const double* a, const double* b, double* out0, double* out1);
/* The three-point forms of one ODE right-hand side with EVERY operand the caller's, so that a test can place the outer points at
 * the exact distance from the centre a certificate admits (atm_certify's TIGHT segments: 2^-21 (1 + 2^-35) relative) instead of the
 * fixed 1 -+ 2^-22 of the ops above.  out0 / out1 / out2 receive the three results apart; took[i] says which form the wavefront of
 * element i ran (the kernel is launched in blocks of 256: elements 64 w .. 64 w + 63 form one wavefront, and every branch is a
 * wave vote).  All pointers are required; a diagnostic like atmrt_math_probe, a multi-device context answers on its first device.
 * tests/test_gpu_detmath.py predicts took from the host and compares the results bit for bit with the plain operations. */
typedef enum atmrt_math_probe3_op {
  ATMRT_PROBE3_DIV3 = 0,        /* dm_div3(a, b0, a, b1, a, b2); took = 1: the outer reciprocals seeded from b0's (every lane's seed
                                   residual <= 2^-20), 0: dm_div for both */
  ATMRT_PROBE3_DIV3_SEEDED = 1, /* dm_div3_seeded(..., have_seed = 0): no vote, took = 1 */
  ATMRT_PROBE3_DIV3_SEED_Z = 2, /* dm_div3_seeded(..., 1, 2 - b0): b0 = Z close to 1 with 2 - Z seeding its reciprocal; took = 1 */
  ATMRT_PROBE3_POW3_TIGHT = 3,  /* pow3_tight(b0, b1, b2, y = a, thr): dm_pow(b_i, a) of a tight Linear segment with expo1 = a and the
                                   exp_thr atm_certify stores for it; took bit 0: the shared log row, bit 1: the shared exp entry */
  ATMRT_PROBE3_EXP3_TIGHT = 4   /* exp3_tight(a b0, a b1, a b2, thr): dm_exp_main(a * b_i) of a tight isothermal segment with expo1 = a
                                   and its exp_thr; took = 1: the shared exp entry */
} atmrt_math_probe3_op;
int atmrt_math_probe3(atmrt_ctx* ctx, int32_t op, size_t n, const double* a, const double* b0, const double* b1, const double* b2,
                      double* out0, double* out1, double* out2, int32_t* took);
/* The table the marching kernels read the Spherical geodesic's sin / cos from, for the parameters now set: *n = its entries
 * (max over k of the stepper distances xs[k] <= max_distance, plus one; 0: no table — another calculator, or ATMRT_STEP_TRIG=off),
 * and the first min(cap, *n) of xs[k], sin(xs[k] / radius), cos(xs[k] / radius).  tests/test_gpu_step_trig.py compares them with
 * atmrt_math_probe's division and SINCOS: an entry must be the bit pattern a lane computes for that distance. */
int atmrt_debug_step_trig(atmrt_ctx* ctx, size_t cap, double* xs, double* sin_out, double* cos_out, size_t* n);
/* A diagnostic like atmrt_debug_step_trig, NOT part of the stable surface: the record the trace-point epilogue of the Spherical
 * calculator reads its frame constants from, for the parameters now set.  *n = its doubles (17; 0: no
 * record — another calculator, or ATMRT_NORMAL_TRIG=off), and the first min(cap, *n) of them: sin, cos of +15 m / radius; sin, cos
 * of -15 m / radius; sin, cos of 0 degrees; sin, cos of 90 degrees; then the north, east and up vectors (x, y, z each) of the
 * observer's latitude and longitude.  tests/test_gpu_normal_trig.py compares them with atmrt_math_probe's division and SINCOS. */
int atmrt_debug_normal_trig(atmrt_ctx* ctx, size_t cap, double* out, size_t* n);
/* A diagnostic like atmrt_debug_step_trig, NOT part of the stable surface: the terrain ceiling table that
 * the context's LAST GENERATED FRAME marched with, as the device holds it.  *rows = its rows (the march's steps + 1) and *n_bins
 * its bins; layout = {dir0, rel_lo, w} of the bins in radians; cell and suffix receive the first min(cap, *rows x (*n_bins + 1))
 * floats of the two planes, row i at i x (*n_bins + 1), the last column being the one of the rays outside the bins.  *rows = 0
 * (and nothing written) when that frame had no table: ATMRT_CEILING=off, another generator than Rectilinear, another calculator
 * than the Spherical one, or no frame yet.  A multi-device context answers for its first device, whose table holds the bins of
 * that device's pixel-column tile.  ATMRT_ERR_STATE when a call after that frame (another set of parameters put through a
 * harness or a tool such as atmrt_viewshed) has built another table in its place.  tests/test_gpu_ceiling_table.py compares the
 * table with the one tests/csrc/ceiling_host.cpp builds on the host: every byte must be equal. */
int atmrt_debug_ceiling_table(atmrt_ctx* ctx, size_t cap, float* cell, float* suffix, int32_t* rows, int32_t* n_bins, double layout[3]);
/* A diagnostic of the same kind: the work queue the LAST GENERATED FRAME's whole-frame opaque march took its 64-pixel groups from
 * (DESIGN.md §7.9), longest estimated march first.  *n_groups = its entries, ceil(pixels / 64) (0, and nothing written: the
 * frame's plan — march_plan, csrc/atmrt_march_plan.h — did not route it to the queue: a small frame unless
 * ATMRT_MARCH_VARIANT=queue, translucent terrain, objects, a column tile, no ceiling table); order receives the first
 * min(cap, *n_groups) of them.  The order decides scheduling only, and entries of equal estimate may change places from build to
 * build; what must hold is that it is a permutation of 0 .. *n_groups - 1 (tests/test_gpu_march_queue.py).  ATMRT_ERR_STATE when a
 * later call has built another order in its place. */
int atmrt_debug_march_order(atmrt_ctx* ctx, size_t cap, uint32_t* order, uint32_t* n_groups);
/* Beside it, under the same rules (*n_groups = 0 without a queue, ATMRT_ERR_STATE once another order was built, the first device of
 * a multi-device context): the ESTIMATED STEPS the queue holds for every entry of that order — order_steps[i] is the estimate of
 * group order[i], the longest of the four rays k_march_length_estimate samples across the group's 64 pixels (pixels 0, 21, 42 and
 * 63, clamped to the image's last), each the first step >= 1 at which ceiling_estimate_ends (csrc/atmrt_ceiling.h) holds for the
 * ray's bin, else the march's steps.  Every value lies in 1 .. steps and the array is non-increasing: the queue sizes the chunks it
 * claims and sets its priorities by these numbers.  They decide scheduling only and change no bit of a frame, so
 * tests/test_gpu_march_queue_scenes.py compares them with a host restatement (tests/march_order_model.py). */
int atmrt_debug_march_order_steps(atmrt_ctx* ctx, size_t cap, uint32_t* order_steps, uint32_t* n_groups);
/* The route the LAST GENERATED FRAME's first-pass Rectilinear march was launched by (MarchRoute, csrc/atmrt_march_plan.h): 0 none
 * (another generator), 1 the plain grid, 2 the small-launch grid, 3 the time-sliced march, 4 the whole-frame work queue.  What was
 * launched, not what was planned: a queue that had to fall back reports its grid.  All routes give the same bits, so this is how a
 * test sees which one a frame took.  index: the device of a multi-device context, as in atmrt_ctx_tile_columns; a context of one
 * device takes -1 or 0.  ATMRT_ERR_STATE without a valid last frame. */
int atmrt_debug_last_march_route(atmrt_ctx* ctx, int32_t index, int32_t* route);
/* A lattice for atmrt_debug_interp_blend, host memory: ne rows (elevation keys, ascending) of nd points (direction keys, ascending),
 * each what Cache::get_pixel (interpolating_rectilinear.rs:80-107) would hold for it — its ResultPixel and the ray steps computing it
 * took.  The trace points of point q are hits [o(q), o(q) + hit_count[q]), o the running sum of hit_count in lattice order, laid out
 * like the hit arrays of atmrt_result_t; n_hits must be the sum of hit_count, every color_tag an atmrt_color_tag. */
typedef struct atmrt_interp_lattice {
  int32_t ne, nd;
  uint64_t n_hits;
  const uint32_t* hit_count;     /* [ne][nd] */
  const double* azimuth;         /* [ne][nd] */
  const double* elevation_angle; /* [ne][nd] */
  const uint32_t* px_steps;      /* [ne][nd] */
  const double* lat;             /* [n_hits] */
  const double* lon;
  const double* distance;
  const double* elevation;
  const double* path_length;
  const double* normal;          /* [n_hits][3] */
  const uint32_t* color_tag;     /* [n_hits] */
  const double* rgba;            /* [n_hits][4] */
} atmrt_interp_lattice_t;
/* A diagnostic in the spirit of atmrt_debug_step_trig, NOT part of the stable surface: the last stage of an InterpolatingRectilinear
 * frame — FovData::cache_coords (:186-204), collect_trace_points, match_sequence, interpolate_trace_points and the angle blend
 * (:213-418), the ray-step count of the referenced lattice points — run on a ray table and a lattice of the caller's, by the host
 * function and the kernels the frame itself runs (k_lattice_keys, k_interp_blend, k_interp_blend_big, k_lattice_steps).  elev and dir
 * are the rays of a width x height image, radians, row-major; min_elev_step, min_dir_step and simulation_step are what the frame
 * derives from its field of view and takes from its parameters.  The lattice must be exactly the rectangle the frame would trace:
 * rows floor(min elev / min_elev_step) .. floor(max elev / min_elev_step) + 1 and the columns likewise; the frame's own limits on it
 * (at most 60000 rows, 2000000 columns, 2^31 points) hold.  `out` is filled as atmrt_generate fills it (release it with
 * atmrt_result_free; device_ms stays 0).  Needs neither parameters nor terrain; a frame generated before is gone afterwards, as
 * after a failed frame.  ATMRT_ERR_INVALID_ARGUMENT: NULL, an empty image, a side above 65535 or more than 2^24 pixels, a step that is not finite and
 * positive, a lattice that is not that rectangle, an n_hits that is not the sum of hit_count, an unknown colour tag.  A multi-device
 * context answers with its first device.  tests/test_gpu_interp_blend.py compares the result with tests/interp_blend_model.py, a
 * model written from the reference's text: every bit must be equal. */
int atmrt_debug_interp_blend(atmrt_ctx* ctx, uint32_t width, uint32_t height, const double* elev, const double* dir,
                             double min_elev_step, double min_dir_step, double simulation_step,
                             const atmrt_interp_lattice_t* lattice, atmrt_result_t* out);

#ifdef __cplusplus
}
#endif
#endif /* ATMRT_H */
