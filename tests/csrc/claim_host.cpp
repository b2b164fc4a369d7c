// claim_host.cpp — stand-alone test of the whole-frame work queue's claim arithmetic (csrc/atmrt_march_queue.h), the functions
// k_rect_march_queue runs: THREADS std::threads, long and short claimers mixed, hammer one word with fetch-and-add until each
// owns nothing more; every item must have been owned exactly once and no claim may name an item outside 0 .. n-1.
// Built by tests/test_claim_protocol.py, plain and with -fsanitize=thread.  Prints "failures N".
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <thread>
#include <vector>

#include "../../atm-raytracer_amd/csrc/atmrt_march_queue.h"

using namespace atmrt;

static int failures = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      failures++;                   \
      std::printf("FAIL " __VA_ARGS__); \
      std::printf("\n");            \
    }                               \
  } while (0)

// one launch: `threads` claimers, the first `n_long` of every four long (the roles of the 16 wavefronts of a workgroup)
static void run(uint32_t n, uint32_t max_chunk, int threads, int n_long, int round) {
  std::atomic<unsigned long long> word{0};
  std::unique_ptr<std::atomic<uint32_t>[]> owned(new std::atomic<uint32_t>[n + 1]);
  for (uint32_t i = 0; i <= n; i++) owned[i].store(0, std::memory_order_relaxed);
  std::atomic<uint32_t> out_of_range{0}, claims_after_empty{0};
  std::atomic<int> go{0};
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; t++) {
    pool.emplace_back([&, t] {
      const bool is_long = t % 4 < n_long;
      while (!go.load(std::memory_order_acquire)) std::this_thread::yield();
      for (uint32_t it = 0;; it++) {
        // every claim chooses its own chunk, as the kernel does (queue_chunk_for of the item at the tail it looked at): here by
        // the tail it sees in a look of its own, between 1 and `max_chunk`
        const uint32_t chunk = is_long ? 1u : 1u + (uint32_t)((word.load(std::memory_order_relaxed) >> 32) + it * 7u + (uint32_t)t) % max_chunk;
        const unsigned long long inc = queue_claim_increment(is_long, chunk);
        const unsigned long long seen = word.fetch_add(inc, std::memory_order_relaxed);
        uint32_t first = 0;
        const uint32_t count = queue_claim_items(seen, is_long, chunk, n, first);
        if (!count) {
          // nothing is left for anybody: a second claim of the same kind owns nothing either
          uint32_t f2 = 0;
          if (queue_claim_items(word.fetch_add(inc, std::memory_order_relaxed), is_long, chunk, n, f2)) claims_after_empty.fetch_add(1);
          break;
        }
        if (count > (is_long ? 1u : chunk)) out_of_range.fetch_add(1);
        for (uint32_t k = 0; k < count; k++) {
          const uint64_t item = is_long ? (uint64_t)first : (uint64_t)first - k; // (first - k wraps if first < k: caught below)
          if (first < k || item >= n) out_of_range.fetch_add(1);
          else owned[item].fetch_add(1, std::memory_order_relaxed);
        }
      }
    });
  }
  go.store(1, std::memory_order_release);
  for (auto& th : pool) th.join();
  uint32_t missed = 0, twice = 0;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t c = owned[i].load(std::memory_order_relaxed);
    missed += c == 0, twice += c > 1;
  }
  CHECK(missed == 0 && twice == 0 && out_of_range.load() == 0 && claims_after_empty.load() == 0,
        "n %u chunk <= %u threads %d long %d round %d: missed %u twice %u out of range %u claims after empty %u", n, max_chunk, threads, n_long,
        round, missed, twice, out_of_range.load(), claims_after_empty.load());
}

// the same arithmetic by hand: every interleaving of one long and one short claimer over a small queue, step by step
static void sequential() {
  for (uint32_t n = 0; n <= 40; n++)
    for (uint32_t chunk : {1u, 3u, 16u})
      for (uint32_t pattern = 0; pattern < 64; pattern++) { // bit k: claim k is long
        unsigned long long word = 0;
        std::vector<int> owned(n, 0);
        bool bad = false;
        for (int k = 0; k < 6 + (int)n * 2; k++) {
          const bool is_long = k < 6 ? (pattern >> k) & 1 : k & 1;
          uint32_t first = 0;
          const uint32_t count = queue_claim_items(word, is_long, chunk, n, first);
          word += queue_claim_increment(is_long, chunk);
          for (uint32_t q = 0; q < count; q++) {
            const uint32_t item = is_long ? first : first - q;
            if (item >= n) bad = true;
            else owned[item]++;
          }
        }
        for (uint32_t i = 0; i < n; i++) bad = bad || owned[i] != 1;
        CHECK(!bad, "sequential n %u chunk %u pattern %u", n, chunk, pattern);
      }
}

int main() {
  sequential();
  for (uint32_t est = 0; est < 5000; est++) { // a chunk is 1 .. MARCH_QUEUE_CHUNK items, fewer the longer they are
    const uint32_t c = queue_chunk_for(est);
    CHECK(c >= 1 && c <= MARCH_QUEUE_CHUNK && (est == 0 || c <= queue_chunk_for(est - 1)) && (est < MARCH_QUEUE_CHUNK_STEPS || c == 1),
          "queue_chunk_for(%u) = %u", est, c);
  }
  for (int round = 0; round < 4; round++)
    for (uint32_t n : {0u, 1u, 15u, 16u, 17u, 1000u})
      for (uint32_t chunk : {1u, 16u})
        for (int threads : {8, 16})
          for (int n_long : {1, 2}) run(n, chunk, threads, n_long, round);
  run(100000, 16, 16, 1, 0); // long enough for the claimers to overlap in earnest
  std::printf("failures %d\n", failures);
  return failures ? 1 : 0;
}
