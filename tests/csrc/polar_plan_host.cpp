// polar_plan_host.cpp — csrc/atmrt_polar_plan.h alone on the host (tests/test_polar_plan_host.py).  Reads one case per line from the
// standard input and prints one line of integers per case:
//   S step reach m_max            ->  lattice_steps (-1: refused)
//   G limit extra n m_0 .. m_n-1  ->  the plan of n targets under the greedy rule
//   U limit n m k s_0 .. s_k-1    ->  the plan of n targets of m samples each with a layout_bytes: the sight lines' arrays and k more
//                                     of s_j bytes per target, each padded to 256 bytes as Carve pads (extra = the sum of s_j)
// A plan's line: the number of batch_begin entries, the entries, entries_max, n, then off and m of every target.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "../../atm-raytracer_amd/csrc/atmrt_polar_plan.h"

using namespace atmrt;

static size_t pad(size_t n) { return (n + 255) / 256 * 256; }

static void print_plan(const PolarPlan& p) {
  printf("%zu", p.batch_begin.size());
  for (size_t b : p.batch_begin) printf(" %zu", b);
  printf(" %zu %zu", p.entries_max, p.meta.size());
  for (const SightMeta& m : p.meta) printf(" %llu %d", (unsigned long long)m.off, m.m);
  printf("\n");
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string kind;
    if (!(in >> kind)) continue;
    if (kind == "S") {
      std::string step, reach;
      int m_max;
      in >> step >> reach >> m_max;
      printf("%d\n", lattice_steps(strtod(step.c_str(), nullptr), strtod(reach.c_str(), nullptr), m_max));
    } else if (kind == "G") {
      size_t limit, extra, n;
      in >> limit >> extra >> n;
      std::vector<int32_t> m(n);
      for (int32_t& v : m) in >> v;
      print_plan(polar_plan(m, limit, extra));
    } else if (kind == "U") {
      size_t limit, n, k, extra = 0;
      int32_t m;
      in >> limit >> n >> m >> k;
      std::vector<size_t> more(k);
      for (size_t& v : more) in >> v, extra += v;
      const auto layout_bytes = [&](size_t nb) { // a target of 24 bytes, its SightMeta of 16 and its DirCalc of 128
        size_t bytes = pad(8 * ((size_t)m + 1)) + pad(8) + pad(24 * nb) + pad(16 * nb) + pad(128 * nb) + 3 * pad(8 * nb * ((size_t)m + 1));
        for (size_t s : more) bytes += pad(nb * s);
        return bytes;
      };
      print_plan(polar_plan(std::vector<int32_t>(n, m), limit, extra, layout_bytes));
    } else {
      fprintf(stderr, "unknown case: %s\n", line.c_str());
      return 2;
    }
    if (!in) {
      fprintf(stderr, "short case: %s\n", line.c_str());
      return 2;
    }
  }
  return 0;
}
