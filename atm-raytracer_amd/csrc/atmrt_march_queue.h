// atmrt_march_queue.h — the claim arithmetic of the whole-frame work queue (k_rect_march_queue, atmrt_march_impl.h).  Nothing of
// HIP: the kernel and the stand-alone host test (tests/csrc/claim_host.cpp, std::thread + ThreadSanitizer) run the same functions.
//
// n items 0 .. n-1 are handed out from ONE 64-bit word `head | tail << 32`, zero before the launch, by fetch-and-add alone:
//   * a LONG claimer adds 1 and owns item h, the head it saw;
//   * a SHORT claimer adds C << 32 and owns the C items n-1-t, n-2-t, ... below the tail t it saw (every claim may choose its own C);
// in both cases only where h + t < n (h items are gone from the front and t from the back: something is left), and a chunk is
// clipped to the n - h - t items that are left.  The word is the whole protocol: every value (h, t) it passes through is seen by
// exactly one claimer, h only grows by claims that own item h, t only by claims that own the items behind it, so every item is
// owned exactly once whatever the interleaving, and once h + t >= n every later claim of either kind owns nothing.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define ATMRT_QUEUE_HD __host__ __device__ inline
#else
#define ATMRT_QUEUE_HD inline
#endif

namespace atmrt {

constexpr uint32_t MARCH_QUEUE_CHUNK = 16; // C at most: sky and ground items last microseconds, one word saturates near 88 claims per microsecond
// A chunk is one wavefront's serial work, and towards the middle of the queue the items at the tail are no longer short: a claimer
// sizes its chunk by the estimated steps of the item at the tail it last saw, so that a chunk stays near MARCH_QUEUE_CHUNK_STEPS.
constexpr uint32_t MARCH_QUEUE_CHUNK_STEPS = 128;
ATMRT_QUEUE_HD uint32_t queue_chunk_for(uint32_t estimated_steps) {
  const uint32_t c = MARCH_QUEUE_CHUNK_STEPS / (estimated_steps ? estimated_steps : 1u);
  return c < 1u ? 1u : c > MARCH_QUEUE_CHUNK ? MARCH_QUEUE_CHUNK : c;
}
// Towards the end of the queue a chunk is also the length of the drain: the wavefronts that still own several items while every
// other claimer finds nothing.  So a chunk shrinks with what is left: besides the steps rule, at most left / (k x claimers) items,
// `left` = n - h - t of the word the claimer looked at (the look it sizes its chunk by anyway) and `claimers` the wavefronts of
// the launch — a k-th of an even share — and 1 once left <= k x claimers, so that the drain is one item long.  claimers 0: no cap.
// k = 1 by measurement (with 4,096 wavefronts k = 1/2 and k = 2 cost the headline frame 0.1 ms, k = 4 0.3 ms).
constexpr uint32_t MARCH_QUEUE_GUIDE_K = 1;
ATMRT_QUEUE_HD uint32_t queue_chunk_cap(uint32_t left, uint32_t claimers) {
  if (!claimers) return MARCH_QUEUE_CHUNK;
  const unsigned long long c = (unsigned long long)left / ((unsigned long long)MARCH_QUEUE_GUIDE_K * claimers);
  return c < 1u ? 1u : c > MARCH_QUEUE_CHUNK ? MARCH_QUEUE_CHUNK : (uint32_t)c;
}
ATMRT_QUEUE_HD uint32_t queue_chunk_for(uint32_t estimated_steps, uint32_t left, uint32_t claimers) {
  const uint32_t c = queue_chunk_for(estimated_steps), cap = queue_chunk_cap(left, claimers);
  return c < cap ? c : cap;
}
// the items left in the queue at the word `seen` (0 once it has run empty)
ATMRT_QUEUE_HD uint32_t queue_items_left(unsigned long long seen, uint32_t n) {
  const unsigned long long h = seen & 0xffffffffull, t = seen >> 32;
  return h + t >= (unsigned long long)n ? 0u : (uint32_t)((unsigned long long)n - h - t);
}

// The priority of a long claimer, by the estimate of the item it now owns against the head's (the longest estimate of the frame):
// 3 from half of it on, 2 from an eighth, 1 below.  (Short claimers run at 0.)
ATMRT_QUEUE_HD int queue_item_priority(uint32_t estimated_steps, uint32_t head_steps) {
  return estimated_steps >= (head_steps + 1u) / 2u ? 3 : estimated_steps >= (head_steps + 7u) / 8u ? 2 : 1;
}

// what a claimer adds to the word
ATMRT_QUEUE_HD unsigned long long queue_claim_increment(bool is_long, uint32_t chunk) {
  return is_long ? 1ull : (unsigned long long)chunk << 32;
}
// What the claimer that saw `seen` (the word before its own addition) owns: `count` items, first, first + dir, ...  (dir = +1 for a
// long claim, whose count is at most 1, and -1 for a chunk); 0: nothing is left, for this claimer and every later one.
ATMRT_QUEUE_HD uint32_t queue_claim_items(unsigned long long seen, bool is_long, uint32_t chunk, uint32_t n, uint32_t& first) {
  const unsigned long long h = seen & 0xffffffffull, t = seen >> 32;
  first = 0;
  if (h + t >= (unsigned long long)n) return 0;
  const unsigned long long left = (unsigned long long)n - h - t;
  if (is_long) {
    first = (uint32_t)h;
    return 1;
  }
  first = (uint32_t)((unsigned long long)n - 1 - t);
  return (uint32_t)(left < chunk ? left : chunk);
}

} // namespace atmrt
