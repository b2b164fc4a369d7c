// claim_guided_host.cpp — stand-alone test of the work queue's guided chunks (csrc/atmrt_march_queue.h: queue_chunk_for with the
// items left and the launch's claimers, queue_chunk_cap, queue_items_left), the functions k_rect_march_queue runs: std::threads of
// both kinds claim from one word as the kernel's wavefronts do — a short claimer looks at the word, sizes its chunk by the estimate
// of the item at the tail it saw and by what is left, then claims with one fetch-and-add.  Every item must be owned exactly once;
// a chunk is never 0, never above MARCH_QUEUE_CHUNK, never above what the cap allows for the look it was sized by, and 1 once
// left <= k x claimers.  Also the priority rule of the long claimers (queue_item_priority) over its whole domain.
// Built by tests/test_claim_guided.py, plain and with -fsanitize=thread.  Prints "failures N".
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

// the estimates of an order: descending, a few long items at the head and a long run of short ones at the tail
static std::vector<uint32_t> estimates(uint32_t n) {
  std::vector<uint32_t> e(n);
  for (uint32_t i = 0; i < n; i++) e[i] = i < n / 50 + 1 ? 1500u - i % 700u : i < n / 4 ? 200u : i < n / 2 ? 40u : 3u;
  for (uint32_t i = 1; i < n; i++)
    if (e[i] > e[i - 1]) e[i] = e[i - 1];
  return e;
}

// one launch: `threads` claimers, the first `n_long` of every four long; `claimers` is what the launcher passes (0: unguided)
static void run(uint32_t n, int threads, int n_long, uint32_t claimers, int round) {
  const std::vector<uint32_t> est = estimates(n);
  std::atomic<unsigned long long> word{0};
  std::unique_ptr<std::atomic<uint32_t>[]> owned(new std::atomic<uint32_t>[n + 1]);
  for (uint32_t i = 0; i <= n; i++) owned[i].store(0, std::memory_order_relaxed);
  std::atomic<uint32_t> out_of_range{0}, bad_chunk{0}, not_one{0};
  std::atomic<int> go{0};
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; t++) {
    pool.emplace_back([&, t] {
      const bool is_long = t % 4 < n_long;
      while (!go.load(std::memory_order_acquire)) std::this_thread::yield();
      for (;;) {
        uint32_t chunk = 1;
        if (!is_long) { // the kernel's look: the tail as it is now, and what is left
          const unsigned long long now = word.load(std::memory_order_relaxed);
          const unsigned long long tail = now >> 32;
          const uint32_t left = queue_items_left(now, n);
          if (tail < n) {
            chunk = queue_chunk_for(est[n - 1u - (uint32_t)tail], left, claimers);
            const uint32_t cap = claimers ? left / (MARCH_QUEUE_GUIDE_K * claimers) : MARCH_QUEUE_CHUNK;
            if (chunk == 0 || chunk > MARCH_QUEUE_CHUNK || chunk > queue_chunk_for(est[n - 1u - (uint32_t)tail]) || chunk > (cap < 1u ? 1u : cap))
              bad_chunk.fetch_add(1);
            if (claimers && (unsigned long long)left <= (unsigned long long)MARCH_QUEUE_GUIDE_K * claimers && chunk != 1) not_one.fetch_add(1);
          }
        }
        const unsigned long long seen = word.fetch_add(queue_claim_increment(is_long, chunk), std::memory_order_relaxed);
        uint32_t first = 0;
        const uint32_t count = queue_claim_items(seen, is_long, chunk, n, first);
        if (!count) break;
        if (count > chunk) out_of_range.fetch_add(1);
        for (uint32_t k = 0; k < count; k++) {
          const uint64_t item = is_long ? (uint64_t)first : (uint64_t)first - k;
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
  CHECK(missed == 0 && twice == 0 && out_of_range.load() == 0 && bad_chunk.load() == 0 && not_one.load() == 0,
        "n %u threads %d long %d claimers %u round %d: missed %u twice %u out of range %u bad chunks %u chunks not 1 at the end %u", n, threads,
        n_long, claimers, round, missed, twice, out_of_range.load(), bad_chunk.load(), not_one.load());
}

// the sizing functions over their domain
static void arithmetic() {
  for (uint32_t claimers : {0u, 1u, 7u, 16u, 4096u})
    for (uint32_t left : {0u, 1u, 2u, 13u, 14u, 15u, 31u, 32u, 33u, 511u, 512u, 8191u, 8192u, 8193u, 16384u, 131072u, 0xffffffffu}) {
      const uint32_t cap = queue_chunk_cap(left, claimers);
      const unsigned long long share = claimers ? (unsigned long long)left / ((unsigned long long)MARCH_QUEUE_GUIDE_K * claimers) : MARCH_QUEUE_CHUNK;
      CHECK(cap >= 1 && cap <= MARCH_QUEUE_CHUNK && (cap == 1 || cap <= share), "queue_chunk_cap(%u, %u) = %u", left, claimers, cap);
      CHECK(!claimers || (unsigned long long)left > (unsigned long long)MARCH_QUEUE_GUIDE_K * claimers || cap == 1, "cap(%u, %u) = %u, not 1", left, claimers, cap);
      for (uint32_t est : {0u, 1u, 8u, 9u, 64u, 127u, 128u, 129u, 2000u}) {
        const uint32_t c = queue_chunk_for(est, left, claimers);
        CHECK(c >= 1 && c <= cap && c <= queue_chunk_for(est) && (c == cap || c == queue_chunk_for(est)), "queue_chunk_for(%u, %u, %u) = %u", est,
              left, claimers, c);
        CHECK(claimers || c == queue_chunk_for(est), "unguided queue_chunk_for(%u, %u, 0) = %u", est, left, c);
      }
    }
  for (uint32_t n : {0u, 1u, 100u})
    for (unsigned long long h = 0; h <= 101; h += 50)
      for (unsigned long long t = 0; t <= 101; t += 25) {
        const uint32_t left = queue_items_left(h | t << 32, n);
        CHECK(left == (h + t >= n ? 0u : (uint32_t)(n - h - t)), "queue_items_left(%llu | %llu << 32, %u) = %u", h, t, n, left);
      }
  for (uint32_t head : {0u, 1u, 7u, 8u, 9u, 1000u, 2001u})
    for (uint32_t est = 0; est <= head; est++) {
      const int prio = queue_item_priority(est, head);
      CHECK(prio >= 1 && prio <= 3 && (est == 0 || prio >= queue_item_priority(est - 1, head)), "queue_item_priority(%u, %u) = %d", est, head, prio);
      CHECK((prio == 3) == (2ull * est >= head) && (prio >= 2) == (8ull * est >= head), "queue_item_priority(%u, %u) = %d against 1/2 and 1/8", est, head, prio);
    }
  CHECK(queue_item_priority(5, 5) == 3 && queue_item_priority(0, 0) == 3, "the head is its own reference estimate: priority 3");
}

int main() {
  arithmetic();
  for (int round = 0; round < 3; round++)
    for (uint32_t n : {0u, 1u, 15u, 17u, 240u, 1000u})
      for (int threads : {8, 16})
        for (int n_long : {1, 2})
          for (uint32_t claimers : {0u, (uint32_t)threads, 4096u}) run(n, threads, n_long, claimers, round);
  run(100000, 16, 2, 16, 0); // long enough for the claimers to overlap in earnest, and for the cap to fall from 16 to 1
  std::printf("failures %d\n", failures);
  return failures ? 1 : 0;
}
