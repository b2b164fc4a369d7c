// atmrt_kernels.h — launch interface between the C-ABI host code (atmrt_api.hip, atmrt_consumers.hip,
// atmrt_probes.hip) and the gfx950 kernels (atmrt_kernels.hip).  Internal; the public surface is include/atmrt.h.
#pragma once

#include <stdlib.h>
#include <string.h>

#include "atmrt_core.h"
#include "atmrt_ceiling.h"
#include "atmrt_march_queue.h"
#include "atmrt_march_plan.h"
#include "atmrt_objects.h"

namespace atmrt {

// Everything a kernel needs about the frame; passed by value (about 1.3 KB of kernel arguments).
struct Frame {
  atmrt_params_t p;
  Earth earth;
  const AtmTable* atm;      // layer table in global memory: wave-uniform indices become scalar loads
  Pinhole ph;
  TerrainView tv;
  const double* alt;        // device scalar: observer altitude after Altitude::abs (params.rs:23-30)
  const double* xs;         // xs[k] = 0 + step + ... + step (k additions): utils.rs:191-196 and the stepper's x
  const ObjectDev* objects;
  const uint8_t* textures;
  int32_t n_objects;
  int32_t n_t;              // terrain samples per column: #{k : xs[k] < max_distance}
  int32_t n_path_cap;       // path elements per row when the ray never drops below -1000 m
  int32_t c0, wl, h;        // pixel-column shard [c0, c0 + wl), image height
  int32_t opaque;           // terrain_alpha == 1.0 and no objects: at most one trace point per pixel
  // InterpolatingRectilinear: the frame is the angular lattice of Cache::get_pixel (interpolating_rectilinear.rs:80-107):
  // column x has azimuth (di0 + x) * dir_step, row y has elevation (ei0 + y) * elev_step (radians)
  int32_t lattice;
  int32_t atm_cubic;        // the atmosphere has Spline segments: launch the kernel variants that carry the quadrature path
  int32_t di0, ei0;
  double dir_step, elev_step;
  double inv_shape_radius;  // RN(1 / earth.shape_radius) (0 on a flat earth): calc_dist divides the step length by the radius (dm_div_r)
  // The escape certificate (atmrt_api.hip, escape_floor): a Rectilinear ray whose last sample lies above
  // esc_floor and which is ascending (refracted: the stepper's dr/dphi > 0; straight: the sample above the one before, and its
  // elevation angle below esc_ang_max) provably crosses neither the terrain nor an object of its wavefront's list again before
  // max_distance: the march credits the rest of its march_steps and leaves.  esc_floor = +inf: no certificate (ATMRT_ESCAPE=off,
  // flat-earth refraction, an atmosphere that can bend an ascending ray back down).
  double esc_floor;
  double esc_ang_max;
  int32_t march_steps;      // steps of a ray that marches to max_distance: #{k >= 1 : xs[k] <= max_distance}
  // Spherical calculator (earth.calc == 2): sin and cos of xs[k] / calc_radius, k = 0 .. march_steps, as spherical_sincos computes
  // them (k_step_trig) — the same for every ray of the frame, so a sample at the stepper's distance xs[k] reads them instead of
  // dividing and reducing again (coords_at_step).  Null for the other calculators and under ATMRT_STEP_TRIG=off.
  const double* xs_sin;
  const double* xs_cos;
  // The terrain ceiling table (atmrt_ceiling.h): rows 0 .. march_steps of ceil_layout.n_bins + 1 entries.  A sample
  // of the lean march above its cell skips its lookup; a ray above max(its suffix, ceil_floor) that is ascending leaves.
  // ceil_floor is the certificate's part of that floor: the lowest certified altitude + one step (refracted rays on a sphere),
  // -inf (straight rays) or +inf (no escape).  Null for the other calculators and generators and under ATMRT_CEILING=off: the march
  // then runs on skip_above and esc_floor alone.
  const CeilEntry* ceil;
  CeilLayout ceil_layout;
  double ceil_floor;
  // The work queue of the whole-frame opaque march (k_rect_march_queue): the frame's groups of 64 consecutive pixels, longest
  // estimated march first (k_march_length_estimate over the table above) — a permutation of 0 .. ceil(wl h / 64) - 1 that decides
  // scheduling only.  Set exactly when the frame's route is MarchRoute::Queue (frame_march_plan), else null.
  const uint32_t* ceil_order;
  const uint32_t* ceil_order_steps; // beside it: the estimated steps of every entry of ceil_order (descending): sizes the chunks claimed from its tail
  // Spherical calculator: the record of what the trace-point epilogue would compute again in every lane (NormalTrig, atmrt_core.h;
  // k_normal_trig): sin / cos of find_normal's two azimuths and of +-15 m / calc_radius, and the three vectors of the observer's
  // position.  Null for the other calculators and under ATMRT_NORMAL_TRIG=off: every lane then computes them, as the reference does.
  // The struct's last field: every other one keeps its place in the kernels' arguments.
  const NormalTrig* normal_trig;
};

// column azimuth / row elevation in degrees, as handed to gen_terrain_cache / gen_path_cache
ATMRT_HD double frame_col_dir(const Frame& f, int x) {
  return f.lattice ? dm_to_degrees((double)(f.di0 + x) * f.dir_step) : fast_ray_dir(f.p, f.c0 + x);
}
ATMRT_HD double frame_row_elev(const Frame& f, int y) {
  return f.lattice ? dm_to_degrees((double)(f.ei0 + y) * f.elev_step) : fast_ray_elev(f.p, y);
}
ATMRT_HD double frame_azimuth(const Frame& f, int x) { // a single wrap into [0, 360): fast.rs:67-72, interpolating_rectilinear.rs:93-98
  double azimuth = frame_col_dir(f, x);
  if (azimuth < 0.0) azimuth += 360.0;
  else if (azimuth >= 360.0) azimuth -= 360.0;
  return azimuth;
}

// Dense per-pixel outputs ([h][wl] row-major).  `normal` is planar [3][h][wl].
struct DensePlanes {
  double* azimuth;
  double* elevation_angle;
  uint32_t* hit_count;
  double* lat;
  double* lon;
  double* distance;
  double* elevation;
  double* path_length;
  double* normal;
};

// Packed trace points (generators/mod.rs:21-30), filled in pixel order.
struct PackedHits {
  double* lat;
  double* lon;
  double* distance;
  double* elevation;
  double* path_length;
  double* normal; // [n][3]
  uint32_t* color_tag;
  double* rgba;   // [n][4]
};

// The arrays of DensePlanes in carving order, with the bytes of one pixel's entry: f(bytes, s.array...) for each, over any number
// of structs that name them alike (atmrt_device_planes_t does).
template <class F, class... S>
ATMRT_HD void dense_fields(F&& f, S&... s) {
  f(8, s.azimuth...), f(8, s.elevation_angle...), f(8, s.lat...), f(8, s.lon...), f(8, s.distance...), f(8, s.elevation...);
  f(8, s.path_length...), f(24, s.normal...), f(4, s.hit_count...);
}
// The same for the arrays of PackedHits and one trace point's entry (atmrt_result_t and atmrt_device_hits_t name them alike).
template <class F, class... S>
ATMRT_HD void packed_fields(F&& f, S&... s) {
  f(8, s.lat...), f(8, s.lon...), f(8, s.distance...), f(8, s.elevation...), f(8, s.path_length...), f(24, s.normal...);
  f(32, s.rgba...), f(4, s.color_tag...);
}

// 256-byte-aligned bump allocation in one buffer: k(ptr, n) points `ptr` at the next free byte and moves on by n bytes rounded up
// to 256.  Over a null base every pointer is null and `bytes` ends as the size of the layout: sizing and carving are one code.
struct Carve {
  char* base;
  size_t bytes = 0;
  ATMRT_HD static size_t pad(size_t n) { return (n + 255) / 256 * 256; }
  ATMRT_HD Carve(void* b) : base(static_cast<char*>(b)) {}
  template <class T>
  ATMRT_HD void operator()(T*& ptr, size_t n) {
    ptr = base ? reinterpret_cast<T*>(base + bytes) : nullptr;
    bytes += pad(n);
  }
};
// `buf` reserved for what layout(Carve&) carves, then carved by it
template <class Buf, class Layout>
hipError_t reserve_carved(Buf& buf, Layout&& layout) {
  Carve size(nullptr);
  layout(size);
  const hipError_t e = buf.reserve(size.bytes);
  if (e != hipSuccess) return e;
  Carve k(buf.ptr);
  layout(k);
  return hipSuccess;
}
ATMRT_HD DensePlanes carve_dense(Carve& k, size_t npx) {
  DensePlanes d;
  dense_fields([&](size_t b, auto*& a) { k(a, npx * b); }, d);
  return d;
}
ATMRT_HD PackedHits carve_packed(Carve& k, size_t n) {
  PackedHits h;
  packed_fields([&](size_t b, auto*& a) { k(a, n * b); }, h);
  return h;
}
// The caller's device arrays as the library's views: false when one of them is missing.
static inline bool planes_from_abi(const atmrt_device_planes_t& p, DensePlanes* d) {
  bool all = true;
  dense_fields([&](size_t, auto*& to, auto* from) { to = from, all = all && from; }, *d, p);
  return all;
}
static inline bool hits_from_abi(const atmrt_device_hits_t& h, PackedHits* p) {
  bool all = true;
  packed_fields([&](size_t, auto*& to, auto* from) { to = from, all = all && from; }, *p, h);
  return all;
}
// n entries of every array of `src` to the same array of `dst` (any struct with PackedHits' names), enqueued on `s`
template <class D>
hipError_t copy_packed(D& dst, const PackedHits& src, uint64_t n, hipMemcpyKind kind, hipStream_t s) {
  hipError_t e = hipSuccess;
  if (n) packed_fields([&](size_t b, auto* to, auto* from) { if (e == hipSuccess) e = hipMemcpyAsync(to, from, n * b, kind, s); }, dst, src);
  return e;
}

// State of one row's path integration at a segment boundary (k_fast_paths runs in segments, see launch_fast_pipeline)
struct PathSegState {
  double x, a, b, px, ph, path_length;
  int32_t hint, n, done, n_final;
};

// Device counters of a frame (Workspace::counters), by slot.  Slot 3 has three uses: in a Fast frame with objects, the scan total
// of the close lists (launch_close_count; the host reads it at once); in a Rectilinear frame, first the pixels that overflowed
// their slots (counted by the counting passes), then, reset by the host once it has read that count, the cursor of the list of
// those pixels (k_gather_slots appends to it, atmrt_kernels.hip).
enum Counter : int {
  CTR_RAY_STEPS = 0,
  CTR_HITS = 1, // total of the last launch_scan_counts: trace points of the frame
  CTR_ESCAPED_RAYS = 2, // Rectilinear rays that left the march under the escape certificate (Frame::esc_floor)
  CTR_CLOSE_TOTAL = 3, // entries of the close lists
  CTR_OVERFLOW_PIXELS = 3, // pixels with more trace points than RECT_SLOTS
  CTR_OVERFLOW_CURSOR = 3, // cursor of the list of those pixels
  CTR_UNLISTED_RAYS = 4, // rays whose candidate list overflowed
  CTR_UNLISTED_COLUMNS = 5, // columns whose candidate list overflowed
  CTR_BIG_STEPS = 6, // steps with more trace points than StepHits holds
  CTR_BIG_BLEND_PIXELS = 7, // InterpolatingRectilinear pixels with more corner points than the in-register member list
  CTR_BIG_BLEND_POINTS = 8, // their corner points together (size of the member arena)
  CTR_BLEND_CURSOR = 9, // cursor of that arena
  CTR_TERRAIN_LOOKUPS = 10, // terrain lookups performed by the Rectilinear march
  CTR_OBJECT_RAYS = 11, // rays of a scene with objects that the lean march left to the general tracer
  CTR_SLICE_UNFINISHED = 12, // groups the time-sliced march left unfinished, + 1 (must be 0: atmrt_api.hip checks)
  CTR_OVERFLOW_RECORDS = 13, // records appended to the overflow arena
  CTR_OBJECT_STEPS = 14, // ray-steps handed to the lean march's out-of-line object step
  CTR_ESCAPED_STEPS = 15, // ray-steps those rays were credited without integrating them: CTR_RAY_STEPS - this = steps integrated
};
constexpr int N_COUNTERS = 16;

// crossings per pixel recorded by the counting march (4096x2048 headline at terrain_alpha 0.5: 99.3 % of the pixels have <= 4)
constexpr int RECT_SLOTS = 4;
// Where slot j of pixel p lies in the slot arena (Workspace::slot_step and the arrays beside it) of a frame of `plane` pixels.  Frames
// without objects keep it slot-major, [RECT_SLOTS][plane]: their counting passes (k_fast_intersect, the lean march in MODE 1) run
// one pixel per lane, so a wavefront's stores to one slot coalesce.  Scenes with objects keep it pixel-major, [plane][RECT_SLOTS]:
// the general tracers (k_fast_trace, k_rect_trace, the lean march's object step) emit the points of one step into consecutive
// entries (step_commit_count, atmrt_device.h: their one route into slots and overflow arena), and the counting passes around them
// (k_fast_intersect with slot_tag, the lean march in MODE 3) follow suit.
enum class SlotLayout { SlotMajor, PixelMajor };
template <SlotLayout LAYOUT>
ATMRT_HD size_t slot_index(size_t p, size_t j, size_t plane) {
  return LAYOUT == SlotLayout::PixelMajor ? p * RECT_SLOTS + j : j * plane + p;
}

// Trace points beyond a pixel's RECT_SLOTS slots (translucent terrain, scenes with objects): appended by the counting passes in any
// order, each with its pixel and its ordinal among the pixel's trace points; CTR_OVERFLOW_RECORDS counts them (more than `cap`: the
// arena is not used and the overflowing pixels are marched / traced a second time, as before round 3).  44 B per record, + a
// PackedHits entry (100 B) in scenes with objects, where a record is a complete object point or a terrain record with its tag.
// `lean_source`: set in the records of the lean march of an object scene — those of a ray the march later hands to the general
// tracer (hit_step[p] = 1 there) are void, the tracer appends that ray's points itself.
constexpr uint32_t OVERFLOW_LEAN = 0x80000000u;
struct OverflowArena {
  uint32_t *pixel, *ordinal, *step;
  double *re0, *pl0, *re1, *pl1;
  uint32_t* color_tag; // scenes with objects: the PackedHits arena's tags (the lean march writes TERRAIN), else null
  uint32_t cap;
};
constexpr size_t STEP_SINKS_MAX_BYTES = 1024; // StepSinks (atmrt_device.h) fits: what Workspace::step_ctx reserves behind the Frame
static inline size_t overflow_arena_bytes(size_t cap) { return cap * (3 * sizeof(uint32_t) + 4 * sizeof(double)); }
static inline OverflowArena carve_overflow(char* base, size_t cap) {
  OverflowArena a{};
  if (!base) return a;
  a.re0 = (double*)base;
  a.pl0 = a.re0 + cap;
  a.re1 = a.pl0 + cap;
  a.pl1 = a.re1 + cap;
  a.pixel = (uint32_t*)(a.pl1 + cap);
  a.ordinal = a.pixel + cap;
  a.step = a.ordinal + cap;
  a.color_tag = nullptr;
  a.cap = (uint32_t)cap;
  return a;
}

// ATMRT_MARCH_VARIANT (MarchOverride, atmrt_march_plan.h), read once per process.
static inline int march_variant_override() {
  static const int v = [] {
    const char* e = getenv("ATMRT_MARCH_VARIANT");
    return !e ? 0 : !strcmp(e, "plain") ? 1 : !strcmp(e, "small") ? 2 : !strcmp(e, "sliced") ? 3 : !strcmp(e, "queue") ? 4 : 0;
  }();
  return v;
}
// The plan of frame `f`'s first-pass march (march_plan), made where the frame is set up (prepare_ceiling: does it take the work
// queue?) and where its scratch is (prepare_workspace: Workspace::march, which the launchers go by) — one function of the same
// inputs, so that Frame::ceil_order is set exactly when the route is Queue.  `f` needs its ceiling fields but ceil_order;
// shared_frame: the context is a rank of a frame that several devices share.
static inline MarchPlan frame_march_plan(const Frame& f, bool shared_frame) {
  if (f.p.generator != ATMRT_GEN_RECTILINEAR) return MarchPlan{};
  MarchShape s{};
  s.n = (size_t)f.wl * f.h;
  s.n_t = f.n_t;
  s.mode = f.n_objects ? 3 : f.opaque ? 0 : 1;
  s.objects = f.n_objects != 0;
  s.queue_ok = f.opaque && f.ceil && !f.lattice && f.c0 == 0 && f.wl == (int32_t)f.p.width && !shared_frame;
  return march_plan(s, march_variant_override());
}
// Wavefronts per SIMD that claim from the head of the queue.  Measured on the headline frame (ATMRT_MARCH_QUEUE_LONG=1|2|3
// is the A/B switch): with 1 the heads are served too slowly for the 2,200 items of 250 steps and more (8.28 ms per frame against
// the grid's 8.75), with 2 the launch ends with its longest item (6.61 ms).  With priorities by item and chunks that shrink as the
// queue empties (below) 3 measured 0.12 ms below 2 on the headline frame in every run, which is less than three
// spreads (0.18 ms) and was measured on no other shape: 2 stays.
constexpr int MARCH_QUEUE_LONG = 2;
static inline int march_queue_long() {
  static const int v = [] {
    const char* e = getenv("ATMRT_MARCH_QUEUE_LONG");
    const int l = e ? atoi(e) : MARCH_QUEUE_LONG;
    return l < 1 ? 1 : l > 3 ? 3 : l;
  }();
  return v;
}
// What a long wavefront's priority goes by (ATMRT_MARCH_QUEUE_PRIO=role|item is the A/B switch, read once per
// process).  item: the estimate of the item it owns against the head's (queue_item_priority: 3, 2 or 1).  role: every long wavefront
// at 1, as before.
static inline bool march_queue_item_prio() {
  static const bool v = [] {
    const char* e = getenv("ATMRT_MARCH_QUEUE_PRIO");
    return !(e && !strcmp(e, "role"));
  }();
  return v;
}
// Chunks that shrink as the queue empties (queue_chunk_cap; ATMRT_MARCH_QUEUE_CHUNKS=steps|guided is the A/B switch): false — a
// chunk goes by the steps rule alone, as before.
static inline bool march_queue_guided() {
  static const bool v = [] {
    const char* e = getenv("ATMRT_MARCH_QUEUE_CHUNKS");
    return !(e && !strcmp(e, "steps"));
  }();
  return v;
}
// the queue's scratch beside the ceiling table: the order, and what the counting sort needs to build it
struct MarchOrder {
  uint32_t* order;     // [n_groups] groups by estimated length, descending
  uint32_t* order_steps; // [n_groups] the estimate of every entry of `order`
  uint32_t* estimate;  // [n_groups] estimated steps of each group (the longest of its sampled rays), 0 .. march_steps
  uint32_t* bin_count; // [march_steps + 1] groups per estimate, then the cursor of each estimate's run in `order`
};
static inline void march_order_layout(size_t n_groups, size_t march_steps, Carve& k, MarchOrder& o) {
  k(o.order, n_groups * sizeof(uint32_t));
  k(o.order_steps, n_groups * sizeof(uint32_t));
  k(o.estimate, n_groups * sizeof(uint32_t));
  k(o.bin_count, (march_steps + 1) * sizeof(uint32_t));
}
static inline void march_order_layout(const Frame& f, Carve& k, MarchOrder& o) {
  march_order_layout(((size_t)f.wl * f.h + 63) / 64, (size_t)f.march_steps, k, o);
}

// Scratch of one frame.  Three owners (atmrt_ctx.h): the context's one workspace allocation, carved by workspace_layout below (array
// shapes, conditions and sizes are stated there); buffers of their own that outlive the frame or a second preparation within it; and
// buffers sized by a count the host reads back in mid-frame.  A field nobody set is null / zero.
struct Workspace {
  MarchPlan march;        // Rectilinear: the route of the frame's first-pass march (prepare_workspace), which the layout and the launchers go by
  // --- carved by workspace_layout
  int32_t* hit_step;      // first hit: index of the older sample of the pair, or -1
  uint64_t* scan_tmp;     // block sums for the scan
  DirCalc* colcalc;       // Fast: per-column DirectionalCalc
  double* prof;           // Fast: terrain profile, sample-major so a wavefront reads 64 columns coalesced
  double* pelev;          // Fast: ray elevation per row
  double* plen;           // Fast: running path length per row
  int32_t* npath;
  PathSegState* path_seg; // Fast: integration state between path segments
  double* dprev;          // Fast: ray-minus-terrain difference at the last sample of the previous intersect segment
  // scenes with objects (Fast): geodesic point of every sample and the objects close to it (utils.rs:74-80)
  double* plat;
  double* plon;
  uint32_t* ccount;       // number of close objects
  uint64_t* coffset;      // exclusive scan of ccount
  double* pelev_t;        // pelev / plen sample-major for k_fast_trace (lanes = rows)
  double* plen_t;
  int32_t* col_cand;      // objects that can be close to any sample of the column (ascending), and ...
  int32_t* col_ncand;     // ... their number; -1 = no list, test every object
  double* col_lo;         // distances between which a sample of the column can be close to the candidate ...
  double* col_hi;
  uint8_t* traced;        // 1 = the pixel can have a step with an object (k_fast_flag_rows)
  // translucent terrain or objects: the counting passes keep the first RECT_SLOTS trace points of every pixel, so that only pixels
  // with more are visited a second time — the slot arena, entry slot_index(p, j) of each array (k_gather_slots moves it to the list)
  uint32_t* slot_step;
  double* slot_rec;       // Rectilinear
  uint32_t* slot_pixel;   // scenes with objects (written by step_emit, not read)
  PackedHits slot_packed; // scenes with objects: trace points of the slots
  char* overflow_arena;   // Rectilinear, translucent terrain or objects: trace points beyond the slots (OverflowArena), or null
  PackedHits overflow_packed; // scenes with objects: the arena's complete points
  size_t overflow_cap;    // its capacity in records (set before the layout runs: prepare_workspace)
  uint32_t* object_rays;  // Rectilinear, scenes with objects: pixels the lean march left to the general tracer
  char* step_ctx;         // Rectilinear, scenes with objects: Frame + StepSinks in HBM for the lean march's out-of-line object step
  char* slice_state;      // route Sliced (slice_state_layout): ray state between two slices + the FIFO of groups, or null
  unsigned long long* march_claim; // route Queue: the claim word, zeroed before the launch, or null
  // --- carved by workspace_layout in an opaque frame (the march's first hits, [4][h][wl]), else sized by the frame's trace points
  double* rect_rec;       // Rectilinear: [4][n] ray elevation / path length at the two bracketing samples
  // --- buffers of their own
  double* alt;            // [1]
  uint64_t* hit_offset;   // [h][wl] exclusive scan of hit_count
  uint64_t* counters;     // [N_COUNTERS], indexed by Counter
  uint32_t* px_steps;     // optional [h][wl]: ray-steps of each pixel (InterpolatingRectilinear counts referenced lattice pixels only)
  // --- sized by a count read back in mid-frame
  uint32_t* clist;        // Fast, scenes with objects: object indices, ascending per sample
  uint32_t* list_step;    // multi-hit: per trace point, the step index and ...
  uint32_t* list_pixel;   // ... its pixel
  uint32_t* overflow;     // pixels with more than RECT_SLOTS crossings
  double* step_prop;      // fill pass, frames with big steps only: `prop` of every listed trace point (big_step_sort)
  // --- host copies of counters, after the counting march
  uint64_t n_overflow;         // CTR_OVERFLOW_PIXELS
  uint64_t n_overflow_records; // CTR_OVERFLOW_RECORDS
};

// The context's workspace allocation: every array of Workspace whose size follows from the Frame before its first launch, each with
// its condition and its bytes, once.  Run over a null base it sizes the allocation (reserve_carved); an array it does not carve for
// this frame stays null, so no kernel can see what another frame left there.
static inline void workspace_layout(const Frame& f, Carve& k, Workspace& ws) {
  const bool rect = f.p.generator == ATMRT_GEN_RECTILINEAR, objects = f.n_objects > 0;
  const size_t wl = (size_t)f.wl, h = (size_t)f.h, npx = wl * h;
  const size_t path = h * (size_t)f.n_path_cap;                        // [h][n_path_cap], or transposed
  const size_t samples = !rect && objects ? (size_t)f.n_t * wl : 0;    // [n_t][wl]
  k(ws.hit_step, npx * sizeof(int32_t));                                // [h][wl]
  k(ws.scan_tmp, ((npx > samples ? npx : samples) / 2048 + 2) * sizeof(uint64_t));
  if (!rect) { // Fast, and both frames of InterpolatingRectilinear
    k(ws.colcalc, wl * sizeof(DirCalc));                                // [wl]
    k(ws.prof, (size_t)f.n_t * wl * sizeof(double));                    // [n_t][wl]
    k(ws.pelev, path * sizeof(double)), k(ws.plen, path * sizeof(double));
    k(ws.npath, h * sizeof(int32_t)), k(ws.path_seg, h * sizeof(PathSegState)); // [h]
    if (!objects) {
      k(ws.dprev, npx * sizeof(double));                                // [h][wl]
    } else { // the close lists of every terrain sample, the paths transposed, the columns' candidates
      k(ws.plat, samples * sizeof(double)), k(ws.plon, samples * sizeof(double));
      k(ws.ccount, samples * sizeof(uint32_t)), k(ws.coffset, samples * sizeof(uint64_t));
      k(ws.pelev_t, path * sizeof(double)), k(ws.plen_t, path * sizeof(double));
      k(ws.col_cand, wl * 64 * sizeof(int32_t)), k(ws.col_ncand, wl * sizeof(int32_t)); // [wl][64], [wl]
      k(ws.col_lo, wl * 64 * sizeof(double)), k(ws.col_hi, wl * 64 * sizeof(double));
      k(ws.traced, npx);                                                // [h][wl]
    }
  }
  // rect_rec of a frame with several trace points per pixel is sized by their number, after the scan (run_core): the counting march
  // writes the slots and only the fill pass writes rect_rec
  if (rect && f.opaque) k(ws.rect_rec, 4 * npx * sizeof(double));
  if (!f.opaque) {
    k(ws.slot_step, RECT_SLOTS * npx * sizeof(uint32_t));               // slot_index: [RECT_SLOTS][h][wl]; with objects [h][wl][RECT_SLOTS]
    if (rect) k(ws.slot_rec, 4 * RECT_SLOTS * npx * sizeof(double));    // [4][RECT_SLOTS][h][wl]
    if (objects) {
      k(ws.slot_pixel, RECT_SLOTS * npx * sizeof(uint32_t));            // [h][wl][RECT_SLOTS]
      ws.slot_packed = carve_packed(k, RECT_SLOTS * npx);
    }
    if (rect) {
      k(ws.overflow_arena, overflow_arena_bytes(ws.overflow_cap));
      if (objects) ws.overflow_packed = carve_packed(k, ws.overflow_cap);
    }
  }
  if (rect && objects) {
    k(ws.object_rays, npx * sizeof(uint32_t));
    k(ws.step_ctx, Carve::pad(sizeof(Frame)) + STEP_SINKS_MAX_BYTES); // launch_rect_trace_count carves the two out of it
  }
  if (ws.march.route == MarchRoute::Sliced) k(ws.slice_state, ws.march.slices.bytes); // a small Rectilinear launch: the time-sliced march
  if (ws.march.route == MarchRoute::Queue) k(ws.march_claim, sizeof(unsigned long long)); // the whole-frame work queue
}

// InterpolatingRectilinear scratch
struct InterpBuffers {
  double* dir;        // [H][W] ray_params_table.direction (radians), full image
  double* elev;       // [H][W]
  double* colmin;     // [W]
  double* rowmin;     // [H]
  int32_t* key_e;     // [h][wl] elev_index of the pixel's first lattice corner
  int32_t* key_d;     // [h][wl]
  double* rem_e;      // [h][wl]
  double* rem_d;      // [h][wl]
  int32_t* bounds;    // [4] min/max of elev_index and dir_index over the shard
  uint8_t* referenced;// [ne][nd]
};
struct LatticeResult { // the lattice frame's packed result
  const uint32_t* hit_count;
  const uint64_t* hit_offset;
  const double* azimuth;
  const double* elevation_angle;
  PackedHits hits;
  const uint32_t* px_steps;
  int32_t nd, ne;
};
struct BlendArena { // member lists of the pixels k_interp_blend_big blends (more than 4 corner points together)
  uint64_t* k;
  double* dist;
  uint32_t* group;
  uint8_t* corner;
  uint8_t* tag;
};
void launch_interp_blend_big(const Frame& f, Workspace& ws, const InterpBuffers& ib, const LatticeResult& lr, bool fill,
                             const DensePlanes& dense, const PackedHits& packed, const BlendArena& arena, hipStream_t stream);
void launch_fov_table(const Frame& f, const InterpBuffers& ib, hipStream_t stream);
void launch_lattice_keys(const Frame& f, const InterpBuffers& ib, double min_elev_step, double min_dir_step, hipStream_t stream);
void launch_interp_blend(const Frame& f, Workspace& ws, const InterpBuffers& ib, const LatticeResult& lr, bool fill,
                         const DensePlanes& dense, const PackedHits& packed, hipStream_t stream);
void launch_interp_finish(const Frame& f, Workspace& ws, const InterpBuffers& ib, const LatticeResult& lr,
                          const DensePlanes& dense, const PackedHits& packed, hipStream_t stream);

// All launches go to `stream`; none of them synchronises or allocates.
void launch_resolve(const Frame& f, Workspace& ws, ObjectDev* objects_mut, hipStream_t stream);
// scenes with objects / translucent terrain + objects: general tracer (count -> scan -> fill)
void launch_close_count(const Frame& f, Workspace& ws, hipStream_t stream);
void launch_close_fill(const Frame& f, Workspace& ws, hipStream_t stream);
// exclusive scan of in[0, n) into out; the grand total into *total (and nothing else)
void launch_scan_u32(const uint32_t* in, size_t n, uint64_t* tmp, uint64_t* out, unsigned long long* total, hipStream_t stream);
void launch_trace_count(const Frame& f, Workspace& ws, const DensePlanes& out, hipStream_t stream); // Fast (Rectilinear: launch_rect_trace_count)
void launch_fast_paths(const Frame& f, Workspace& ws, hipStream_t stream, int i_begin, int i_end); // atmrt_paths.hip
// The phase events of a context (atmrt_ctx::ev; `timing` below): an interval of atmrt_timings_t lies between two of them.  Between
// frames atmrt_sight_lines, atmrt_locate_landmarks* and atmrt_shadow_mask* time their own consecutive intervals with the same events, under names of their own.
enum PhaseEvent {
  EV_PROFILE_BEGIN, EV_PROFILE_END, // Fast: the terrain profile
  EV_PATHS_BEGIN, EV_PATHS_END,     // Fast: the ray paths (second stream)
  EV_MARCH_BEGIN, EV_MARCH_END,     // the intersect scan (Fast) or the march (Rectilinear)
  EV_FINALIZE_END,                  // finalize begins where the scan or march ends
  EV_PACK_BEGIN, EV_PACK_END,
  EV_CEIL_BEGIN, EV_CEIL_END,       // the build of the terrain ceiling table (timings.ceiling_ms)
  EV_COUNT,
  EV_FINALIZE_BEGIN = EV_MARCH_END,
  EV_SIGHT_BEGIN = 0, EV_SIGHT_PROFILED, EV_SIGHT_SOLVED, EV_SIGHT_END,
  EV_VS_BEGIN = 0, EV_VS_PATHS, EV_VS_BATCH, EV_VS_PROFILED, EV_VS_SCANNED, EV_VS_END,
  EV_HZ_BATCH = EV_VS_BATCH, EV_HZ_PROFILED, EV_HZ_SCANNED, EV_HZ_REFINED, EV_HZ_END, // after EV_VS_BEGIN and EV_VS_PATHS: the table is the viewshed's
  EV_LM_BEGIN = 0, EV_LM_UPLOADED, EV_LM_FIRST_PASS, EV_LM_SECOND_PASS, EV_LM_END,
  EV_SH_BEGIN = 0, EV_SH_COMPACTED, EV_SH_MARCHED, EV_SH_END,
  EV_SKY_BEGIN = 0, EV_SKY_COMPACTED, EV_SKY_MARCHED, EV_SKY_END,
};
static_assert(EV_SIGHT_END < EV_COUNT && EV_VS_END < EV_COUNT && EV_HZ_END < EV_COUNT && EV_LM_END < EV_COUNT && EV_SH_END < EV_COUNT && EV_SKY_END < EV_COUNT, "the borrowed events exist");
#ifndef ATMRT_FAST_SEGMENTS
#define ATMRT_FAST_SEGMENTS 4
#endif
constexpr int FAST_SEGMENTS = ATMRT_FAST_SEGMENTS;
int launch_fast_pipeline(const Frame& f, Workspace& ws, const DensePlanes& out, hipStream_t stream, hipStream_t stream2,
                         hipEvent_t ev_fork, hipEvent_t* ev_seg, hipEvent_t* ev_scan, hipEvent_t* timing); // returns the number of segments; records EV_PROFILE_BEGIN .. EV_MARCH_BEGIN
void launch_fast_caches(const Frame& f, Workspace& ws, hipStream_t stream, hipStream_t stream2, hipEvent_t ev,
                        hipEvent_t ev_join, hipEvent_t* timing /* EV_PROFILE_*: phase A, EV_PATHS_*: phase B */);
void launch_fast_intersect(const Frame& f, Workspace& ws, const DensePlanes& out, hipStream_t stream);
void launch_fast_finalize(const Frame& f, Workspace& ws, const DensePlanes& out, hipStream_t stream);
MarchRoute launch_rect_march(const Frame& f, Workspace& ws, const DensePlanes& out, hipStream_t stream, hipEvent_t ev_marched); // the route it launched
void launch_scan_counts(const Frame& f, Workspace& ws, const uint32_t* hit_count, hipStream_t stream);
void launch_pack_first_hits(const Frame& f, Workspace& ws, const DensePlanes& dense, const PackedHits& packed,
                            hipStream_t stream);
// several trace points per pixel (terrain_alpha < 1, scenes with objects), count -> scan -> fill: the fill of every route — what the
// counting pass recorded to the pixel-ordered list, a second pass over the pixels that did not cover, the points completed
void launch_list_fill(const Frame& f, Workspace& ws, uint64_t n_hits, const DensePlanes& dense, const PackedHits& packed,
                      hipStream_t stream);
// its Rectilinear parts (atmrt_march_linear.hip): all the points of the ws.n_overflow pixels listed in ws.overflow — a second lean
// march, in scenes with objects the general tracer — and the terrain points of the list completed from their records
void launch_rect_second_pass(const Frame& f, Workspace& ws, uint64_t n_hits, const DensePlanes& dense, const PackedHits& packed,
                             hipStream_t stream);
void launch_rect_finalize_list(const Frame& f, Workspace& ws, uint64_t n_hits, const PackedHits& packed, hipStream_t stream);

void launch_draw_image(size_t n_pixels, const atmrt_coloring_t& col, double terrain_alpha, bool packed_valid,
                       const uint32_t* hit_count, const uint64_t* hit_offset, const PackedHits& hits, const DensePlanes& dense,
                       uint8_t* rgb, hipStream_t stream);
// the same with the cast-shadow status plane (include/atmrt.h, "cast shadows"): the first trace point of a SHADOWED pixel takes light_dot = 0
void launch_draw_image_shadowed(size_t n_pixels, const atmrt_coloring_t& col, double terrain_alpha, bool packed_valid,
                                const uint32_t* hit_count, const uint64_t* hit_offset, const PackedHits& hits, const DensePlanes& dense,
                                const uint8_t* status, uint8_t* rgb, hipStream_t stream);

// The annotations of renderer::output_image (kernels in atmrt_overlay.h).  find_elev for every column of the [h][w] plane `elev` and
// the targets t0, t1 in one pass over `bands` row bands (overlay_bands; workspace of overlay_workspace_bytes): *y_of_x points at
// [2][w] rows, -1 = None.  Ticks: an array of {u32 pos, u32 size, i32 vertical, i32 pad}.
int overlay_bands(int w, int h, int n_cu);
size_t overlay_workspace_bytes(int w, int bands);
void launch_overlay_find_elev(const double* elev, int w, int h, int bands, double t0, double t1, void* workspace, int32_t** y_of_x,
                              hipStream_t stream);
void launch_overlay_lines(const int32_t* y_of_x, int w, int h, uint8_t* rgb, const uint8_t color[3], hipStream_t stream);
void launch_overlay_ticks(const void* ticks, int n, int w, int h, uint8_t* rgb, hipStream_t stream);

// Where a frame's trace points are, for the kernels that read a finished frame (atmrt_vismap.h, atmrt_landmarks.h): pixel p of
// n_pixels holds entry p of the planes lat / lon / dist / elev where hit_count[p] != 0 (hit_offset null), or entries [hit_offset[p],
// + hit_count[p]) of the lists.  `width` turns a flat pixel index into (x, y).  The visibility map reads neither `width` nor `elev`:
// a caller without an elevation plane leaves it null.
struct TracePoints {
  size_t n_pixels;
  uint32_t width;
  const uint32_t* hit_count;
  const uint64_t* hit_offset; // null: the planes
  const double *lat, *lon, *dist, *elev;
};

// The visibility map (kernels in atmrt_vismap.h).  `block` is the call's device block of vis_block_bytes(): launch_vis_reset
// initialises it, the scatter adds its statistics and the bounds kernel its keys, vis_block_decode reads a host copy of it.
// min_distance may be null.
size_t vis_block_bytes();
void vis_block_decode(const void* block_host, atmrt_visibility_stats_t* stats, double bounds[4]);
void launch_vis_reset(void* block, hipStream_t stream);
void launch_vis_map(const TracePoints& src, const atmrt_geo_grid_t& grid, bool aggregate, uint32_t* count, double* min_distance, void* block,
                    hipStream_t stream);
void launch_vis_bounds(const TracePoints& src, void* block, hipStream_t stream);

// The landmark search (kernels in atmrt_landmarks.h).  LmIndex: the call's bucket index in device memory — cell c of `grid` lists
// the landmarks items[cell_start[c] .. cell_start[c + 1]), indices into lm.  LmState: per landmark the count, the smallest d2 (its
// bits) and the winner's key p << 32 | point index, and the statistics block (LM_N u64).
struct LmIndex {
  atmrt_geo_grid_t grid;
  const uint32_t* cell_start; // [n_cells + 1]
  const uint32_t* items;
  const atmrt_landmark_t* lm;
  double r2;
};
enum LmSlot : int { LM_POINTS = 0, LM_SKIPPED = 1, LM_TESTED = 2, LM_WITHIN = 3 };
constexpr int LM_N = 4;
struct LmState {
  uint32_t* count;
  unsigned long long *d2min, *key, *ctr;
};
// the call's kernels in order: reset, pass A (pass_b false), pass B, pass C; hits is device memory for n records
void launch_lm_reset(size_t n, const LmState& state, hipStream_t stream);
void launch_lm_pass(bool pass_b, const TracePoints& src, const LmIndex& index, const LmState& state, hipStream_t stream);
void launch_lm_finish(size_t n, const TracePoints& src, const LmState& state, atmrt_landmark_hit_t* hits, hipStream_t stream);

MarchRoute launch_rect_trace_count(const Frame& f, Workspace& ws, const DensePlanes& out, hipStream_t stream); // the route it launched
void launch_rect_trace_objects(const Frame& f, Workspace& ws, const DensePlanes& out, uint64_t n_rays, hipStream_t stream);
void launch_dense_from_packed(const Frame& f, Workspace& ws, const PackedHits& packed, const DensePlanes& dense, int fast_angles,
                              hipStream_t stream);

// harness kernels (diagnostic subcommands of the reference)
void launch_get_elev(const Frame& f, size_t n, const double* lat, const double* lon, double* elev, uint8_t* valid,
                     hipStream_t stream);
void launch_ray_paths(const Frame& f, double h0, size_t n_angles, const double* angles_deg, int straight, double step,
                      size_t n_steps, double* x, double* h, hipStream_t stream);
void launch_atm_sample(const Frame& f, size_t n, const double* alt, double* t, double* p, double* nidx, double* dn,
                       hipStream_t stream);
void launch_step_trig(const Earth& e, size_t n, const double* xs, double* s, double* c, hipStream_t stream);
void launch_normal_trig(const Earth& e, double obs_lat, double obs_lon, NormalTrig* out, hipStream_t stream);
// fills f.ceil (rows 0 .. f.march_steps) for f.ceil_layout: the cells, then every bin's suffix maxima
void launch_ceiling(const Frame& f, CeilEntry* table, hipStream_t stream);
// Frame::ceil_order from the table (f.ceil set): estimate, histogram, scan, scatter
void launch_march_order(const Frame& f, const MarchOrder& o, hipStream_t stream);
void launch_math_probe(int op, size_t n, const double* a, const double* b, double* out0, double* out1, hipStream_t stream);
void launch_math_probe3(int op, size_t n, const double* a, const double* b0, const double* b1, const double* b2, double* out0, double* out1,
                        double* out2, int32_t* took, hipStream_t stream);
void launch_coords_at_dist(const Frame& f, double lat0, double lon0, double dir, size_t n, const double* dist,
                           double* lat, double* lon, hipStream_t stream);

} // namespace atmrt
