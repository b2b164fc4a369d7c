// atmrt_march_plan.h — which way the first-pass Rectilinear march of a frame is launched, and the scratch the time-sliced way needs.
// The route is a pure function of the launch's shape and of ATMRT_MARCH_VARIANT (march_plan); one plan is made per frame
// (frame_march_plan, atmrt_kernels.h) and everything else reads it.  Plain C++ with nothing of HIP in it but atmrt_core.h's DirCalc:
// tests/csrc/march_plan_host.cpp compiles it alone.
#pragma once

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "atmrt_core.h"

namespace atmrt {

// Grid: k_rect_march over every pixel.  GridDrain: its small-launch variant (wave priorities that fall with progress against the
// drain at the end of the launch, object steps out of line; atmrt_march_impl.h).  Sliced: k_rect_march_first / _cont, ray state
// through HBM between slices of MARCH_SLICE_STEPS steps.  Queue: k_rect_march_queue, the whole-frame work queue.  None: the frame is
// not a Rectilinear one.
enum class MarchRoute : int32_t { None = 0, Grid = 1, GridDrain = 2, Sliced = 3, Queue = 4 };

// ATMRT_MARCH_VARIANT=plain|small|sliced forces one variant for every launch (test hook: the random sweeps run small frames over the
// kernel the full-size frames use, and the other way round; same results every way).  =queue forces the whole-frame work queue on
// the frames that can take it at any size and leaves every other launch to the choice by size.  All four are swept: the variant
// sweeps of tests/test_gpu_ceiling.py, _ceiling_table.py, _step_trig.py and _escape.py list queue beside the other three, and
// tests/test_gpu_march_queue_scenes.py runs a family of queue-eligible frames (tests/queue_cases.py) through it against the oracle.
enum MarchOverride : int { MARCH_BY_SIZE = 0, MARCH_FORCE_PLAIN = 1, MARCH_FORCE_SMALL = 2, MARCH_FORCE_SLICED = 3, MARCH_FORCE_QUEUE = 4 };

// A launch of at most MARCH_SMALL_MAX_BLOCKS 256-thread blocks is "small" (a few resident sets: column shards of a frame, test
// frames).  In a launch of many resident sets the drain is 1 % and the priorities against it cost about as much (the headline frame
// 269.4 -> 271.6 ms), so only launches of at most that many workgroups (16 resident sets) use them.
constexpr unsigned MARCH_SMALL_MAX_BLOCKS = 16384u;
constexpr int MARCH_SLICE_STEPS = 128;
// Since the plain march runs 5 wavefronts per SIMD too (round 4) the small-launch variant only pays where the drain is a large part
// of the launch: measured on the tiles of the headline (profiles/r04/march_occupancy_and_slices.json), translucent terrain (mode 1)
// plain / small at 16384 blocks 195 / 199 ms, at 8192 203 / 208, at 4096 235 / 218; scenes with objects (mode 3, where the variant also
// does the object steps out of line) 251 / 258, 295 / 267, 384 / 274.
constexpr unsigned march_drain_max_blocks(int mode) { return mode == 1 ? 6144u : mode == 3 ? 12288u : MARCH_SMALL_MAX_BLOCKS; }

// What the route depends on, and nothing else.
struct MarchShape {
  size_t n;        // pixels of the launch (the column shard's width x the image height)
  int32_t n_t;     // terrain samples per column: a ray marches at most n_t + 1 steps
  int32_t mode;    // k_rect_march's MODE: 0 opaque terrain, 1 translucent terrain, 3 scenes with objects
  bool objects;    // the scene has objects: a sliced group's candidate list travels with its state
  // The whole-frame work queue is for the launches the plain grid would run: opaque terrain without objects, a ceiling table to
  // estimate from, not the lattice frame of InterpolatingRectilinear, the whole image in one launch (c0 == 0, wl == width) and a
  // context that is no rank of a shared frame (the column tiles of a multi-GPU frame stay on the sliced march).
  bool queue_ok;
};

struct SliceLayout {
  uint32_t n_groups;     // groups of 64 consecutive pixels
  size_t n_pad;          // pixels rounded up to whole groups
  size_t slices_after;   // an upper bound on the slices a ray can need after the first
  size_t cap;            // FIFO entries: n_groups x slices_after
  size_t bytes;          // of Workspace::slice_state (slice_state_layout)
};

struct MarchPlan {
  MarchRoute route = MarchRoute::None;
  SliceLayout slices{};           // route == Sliced: what the slices need; else zero
  int override = MARCH_BY_SIZE;   // what the plan was made under: the frame's grid launches beside it go by the same (march_grid_drain)
};

constexpr int WAVE_CAND = 96; // entries of a wavefront's candidate list (scenes with objects); more: every ray of the wavefront is left to the tracer
// a group's list between two slices: lo, hi, vlo, vhi (f64) and the object index (i32) of every entry, the number of entries and
// the next wake distance
constexpr size_t SLICE_GROUP_LIST_BYTES = (size_t)WAVE_CAND * (4 * sizeof(double) + sizeof(int32_t)) + 2 * sizeof(double);

// The state of the time-sliced march in Workspace::slice_state (atmrt_march_impl.h, "Time-sliced march"): of every ray what it
// carries from slice to slice, the FIFO of groups and its three counters.  A kernel argument: the fields keep their order.
struct SliceState {
  double *x, *a, *b, *sh, *pl, *diff0, *ang; // [n_pad]
  int32_t *step, *hint;                      // [n_pad]; step < 0: the ray has finished
  uint32_t* count;                           // [n_pad] MODE 1: crossings so far
  DirCalc* calc;                             // [n_pad] the ray's geodesic calculator
  uint32_t* queue;                           // [cap], 0xffffffff = not written yet
  unsigned long long* ctl;                   // [4] in the 64 bytes reserved: entries claimed by readers, entries written, groups finished
  uint32_t cap;
  char* glist;                               // MODE 3: [n_groups] candidate lists of SLICE_GROUP_LIST_BYTES each, or null
};
// The one layout of that block: calc, x, a, b, sh, pl, diff0, ang, step, hint, count, ctl, queue and, for scenes with objects, the
// group lists at the next multiple of 256.  Returns its bytes; over a null base every pointer of `st` is null, over the block they
// are the arrays: sizing and carving are one code.
inline size_t slice_state_layout(char* base, const SliceLayout& L, bool objects, SliceState& st) {
  size_t off = 0;
  const auto take = [&](auto*& array, size_t count) {
    array = base ? reinterpret_cast<std::remove_reference_t<decltype(array)>>(base + off) : nullptr;
    off += count * sizeof(*array);
  };
  take(st.calc, L.n_pad);
  take(st.x, L.n_pad), take(st.a, L.n_pad), take(st.b, L.n_pad), take(st.sh, L.n_pad), take(st.pl, L.n_pad);
  take(st.diff0, L.n_pad), take(st.ang, L.n_pad);
  take(st.step, L.n_pad), take(st.hint, L.n_pad), take(st.count, L.n_pad);
  take(st.ctl, 8);
  take(st.queue, L.cap);
  st.cap = (uint32_t)L.cap;
  st.glist = nullptr;
  if (objects) { // every group's candidate list (what a wavefront of k_rect_march<3> keeps in LDS) travels with its state
    off = (off + 255) / 256 * 256;
    take(st.glist, (size_t)L.n_groups * SLICE_GROUP_LIST_BYTES);
  }
  return off;
}
// a group's candidate list in HBM (MODE 3): the arrays of one record
struct GroupList {
  double *lo, *hi, *vlo, *vhi;
  int32_t* obj;
  double* n_and_wake; // [0] number of entries (as a double), [1] x_wake
};
ATMRT_HD GroupList group_list(char* base, uint32_t group) {
  char* q = base + (size_t)group * SLICE_GROUP_LIST_BYTES;
  GroupList g;
  g.n_and_wake = (double*)q;
  g.lo = g.n_and_wake + 2;
  g.hi = g.lo + WAVE_CAND;
  g.vlo = g.hi + WAVE_CAND;
  g.vhi = g.vlo + WAVE_CAND;
  g.obj = (int32_t*)(g.vhi + WAVE_CAND);
  return g;
}

// false: a launch of this shape cannot be sliced — no pixels, rays one slice long, or a FIFO of more than 2^31 entries (such a frame
// is marched whole)
inline bool slice_layout_of(const MarchShape& s, SliceLayout& L) {
  if (s.n == 0 || (int64_t)s.n_t + 2 <= MARCH_SLICE_STEPS) return false;
  L.n_groups = (uint32_t)((s.n + 63) / 64);
  L.n_pad = (size_t)L.n_groups * 64;
  L.slices_after = ((size_t)s.n_t + 2 + MARCH_SLICE_STEPS - 1) / MARCH_SLICE_STEPS;
  L.cap = (size_t)L.n_groups * L.slices_after;
  if (L.cap > 0x7fffffffull) return false;
  SliceState sized;
  L.bytes = slice_state_layout(nullptr, L, s.objects, sized);
  return true;
}

// A launch that is a grid whatever else the frame does — the second march over the overflow list (mode 2), the fall-back of a queue
// that cannot be launched — and the last choice of march_plan: true = the small-launch variant.
inline bool march_grid_drain(int mode, size_t n, int override) {
  if (override == MARCH_FORCE_PLAIN) return false;
  if (override == MARCH_FORCE_SMALL || override == MARCH_FORCE_SLICED) return true;
  return (n + 255) / 256 <= march_drain_max_blocks(mode);
}

// The route of a Rectilinear frame's first-pass march.
inline MarchPlan march_plan(const MarchShape& s, int override) {
  MarchPlan plan;
  plan.override = override;
  const bool by_size = override == MARCH_BY_SIZE || override == MARCH_FORCE_QUEUE;
  const bool small = (s.n + 255) / 256 <= MARCH_SMALL_MAX_BLOCKS;
  // The queue: forced, or a grid above MARCH_SMALL_MAX_BLOCKS.  It and the slices exclude one another here, in one place.
  if (s.mode == 0 && s.queue_ok && (override == MARCH_FORCE_QUEUE || (override == MARCH_BY_SIZE && !small))) {
    plan.route = MarchRoute::Queue;
    return plan;
  }
  // The slices are for small launches over opaque terrain.
  // Scenes with objects CAN be sliced (round 4: a group's candidate list travels with its state, the object steps are done out of
  // line inside the slices; bit-identical, tests/test_gpu_march_variants.py) but are not by default: config 5's tiles at 8 GPUs
  // take 8 x 43.8 ms sliced against 8 x 42.3 ms through the small-launch variant of k_rect_march<3> (the slices that contain object
  // steps run long and put their groups out of step) — ATMRT_MARCH_VARIANT=sliced forces it.
  // Translucent terrain likewise (round 4, after the march went to 5 wavefronts per SIMD; tiles of the headline at alpha 0.5, sum of the
  // tile times): 2 tiles sliced 210 ms / plain 195 / small-launch 199, 4 tiles 211 / 203 / 208, 8 tiles 224 / 235 / 218 — rays that do
  // not stop at the terrain are of near-uniform length, which is what the slices were there to even out; those launches pick between
  // the plain and the small-launch variant by the size of the grid (march_drain_max_blocks).
  const bool want_slices = override == MARCH_FORCE_SLICED || (by_size && s.mode == 0 && small);
  if (want_slices && slice_layout_of(s, plan.slices)) {
    plan.route = MarchRoute::Sliced;
    return plan;
  }
  plan.slices = SliceLayout{};
  plan.route = march_grid_drain(s.mode, s.n, override) ? MarchRoute::GridDrain : MarchRoute::Grid;
  return plan;
}

} // namespace atmrt
