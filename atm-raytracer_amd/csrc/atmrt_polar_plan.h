// atmrt_polar_plan.h — the host arithmetic of the calls that march targets along azimuths from the observer (sight lines, viewshed,
// viewshed map, horizon) and of the cast shadows' lattice: how many samples a reach takes, and how a call's targets are split into
// the batches that share the scratch buffer.  Plain C++ with nothing of HIP in it: tests/csrc/polar_plan_host.cpp compiles it alone.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>

namespace atmrt {

// The sample lattice: d_0 = 0, d_{i+1} = d_i + step (utils.rs:191-196).  The first index i with d_i >= reach, or -1 where that is
// more than m_max samples away.
inline int32_t lattice_steps(double step, double reach, int32_t m_max) {
  int32_t i = 0;
  for (double d = 0.0; d < reach;) {
    d += step;
    if (++i > m_max) return -1;
  }
  return i;
}

struct SightMeta {
  uint64_t off; // first entry of the target's profile in SightBatch::T / lat / lon
  int32_t m;
  int32_t _pad;
};
inline size_t sight_target_bytes(int m) { return 3 * sizeof(double) * ((size_t)m + 1) + 1024; } // what a target's profile adds to a batch

struct PolarPlan {
  std::vector<SightMeta> meta;     // per target; off counts from the start of the target's batch
  std::vector<size_t> batch_begin; // first target of every batch, and n at the end
  size_t entries_max = 0;          // profile entries of the largest batch
};

// Targets in their order, as many to a batch as stay under `limit` at sight_target_bytes(m) + extra each; a batch holds at least one.
// With layout_bytes (the calls whose targets all have one m): no batch holds more than the first does, and then as many fewer as it
// takes for layout_bytes(targets of a batch) — the whole carve, distance table and every array's padding included — to stay under
// the limit.
inline PolarPlan polar_plan(const std::vector<int32_t>& m, size_t limit, size_t extra, const std::function<size_t(size_t)>& layout_bytes = nullptr) {
  const size_t n = m.size();
  size_t cap = n;
  if (layout_bytes && n) {
    cap = std::min(n, std::max<size_t>(1, limit / (sight_target_bytes(m[0]) + extra)));
    while (cap > 1 && layout_bytes(cap) > limit) cap--;
  }
  PolarPlan plan;
  plan.meta.resize(n);
  plan.batch_begin.assign(1, 0);
  size_t bytes = 0, entries = 0;
  for (size_t t = 0; t < n; t++) {
    const size_t add = sight_target_bytes(m[t]) + extra;
    if (bytes && (bytes + add > limit || t - plan.batch_begin.back() == cap)) {
      plan.batch_begin.push_back(t);
      bytes = entries = 0;
    }
    plan.meta[t] = SightMeta{entries, m[t], 0};
    bytes += add, entries += (size_t)m[t] + 1;
    plan.entries_max = std::max(plan.entries_max, entries);
  }
  plan.batch_begin.push_back(n);
  return plan;
}

} // namespace atmrt
