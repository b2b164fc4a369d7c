// march_plan_host.cpp — csrc/atmrt_march_plan.h alone on the host (tests/test_march_plan_host.py).  Reads one case per line from the
// standard input and prints one line of integers per case:
//   P n n_t mode objects queue_ok override  ->  march_plan: route n_groups n_pad slices_after cap bytes (zeros unless Sliced)
//   G mode n override                       ->  march_grid_drain as a route: 2 the small-launch grid, 1 the plain one
//   L n n_t objects                         ->  the plan of that launch forced to the slices, its state carved from a real block of
//                                               `bytes` bytes: bytes, then offset, bytes, element size and alignment of every array
//                                               (calc x a b sh pl diff0 ang step hint count ctl queue glist; offset -1: null).  The
//                                               first and the last byte of every array are written.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "../../atm-raytracer_amd/csrc/atmrt_march_plan.h"

using namespace atmrt;

template <class T>
static void print_array(char* base, T* array, size_t count) {
  if (!array) {
    printf(" -1 0 %zu %zu", sizeof(T), alignof(T));
    return;
  }
  char* first = reinterpret_cast<char*>(array);
  if (count) first[0] = 1, first[count * sizeof(T) - 1] = 1;
  printf(" %td %zu %zu %zu", first - base, count * sizeof(T), sizeof(T), alignof(T));
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string kind;
    if (!(in >> kind)) continue;
    if (kind == "P") {
      MarchShape s{};
      int objects, queue_ok, override;
      in >> s.n >> s.n_t >> s.mode >> objects >> queue_ok >> override;
      s.objects = objects != 0, s.queue_ok = queue_ok != 0;
      const MarchPlan p = march_plan(s, override);
      printf("%d %u %zu %zu %zu %zu\n", (int)p.route, p.slices.n_groups, p.slices.n_pad, p.slices.slices_after, p.slices.cap, p.slices.bytes);
    } else if (kind == "G") {
      int mode, override;
      size_t n;
      in >> mode >> n >> override;
      printf("%d\n", (int)(march_grid_drain(mode, n, override) ? MarchRoute::GridDrain : MarchRoute::Grid));
    } else if (kind == "L") {
      MarchShape s{};
      int objects;
      in >> s.n >> s.n_t >> objects;
      s.objects = objects != 0, s.mode = objects ? 3 : 0;
      const MarchPlan p = march_plan(s, MARCH_FORCE_SLICED);
      if (p.route != MarchRoute::Sliced) {
        fprintf(stderr, "not sliced: %s\n", line.c_str());
        return 2;
      }
      const SliceLayout& L = p.slices;
      char* block = static_cast<char*>(aligned_alloc(256, (L.bytes + 255) / 256 * 256)); // as the workspace hands it out: on 256 bytes
      if (!block) return 3;
      memset(block, 0, L.bytes);
      SliceState st;
      const size_t bytes = slice_state_layout(block, L, s.objects, st);
      printf("%zu", bytes);
      print_array(block, st.calc, L.n_pad), print_array(block, st.x, L.n_pad), print_array(block, st.a, L.n_pad);
      print_array(block, st.b, L.n_pad), print_array(block, st.sh, L.n_pad), print_array(block, st.pl, L.n_pad);
      print_array(block, st.diff0, L.n_pad), print_array(block, st.ang, L.n_pad), print_array(block, st.step, L.n_pad);
      print_array(block, st.hint, L.n_pad), print_array(block, st.count, L.n_pad), print_array(block, st.ctl, 8);
      print_array(block, st.queue, L.cap);
      if (st.glist) { // a list's arrays through group_list: the last group's last index is the block's last word
        const GroupList g = group_list(st.glist, L.n_groups - 1);
        g.n_and_wake[0] = 1.0, g.obj[WAVE_CAND - 1] = 1;
        printf(" %td %zu 1 %zu\n", st.glist - block, (size_t)L.n_groups * SLICE_GROUP_LIST_BYTES, alignof(double));
      } else {
        printf(" -1 0 1 %zu\n", alignof(double));
      }
      if (st.cap != L.cap || bytes != L.bytes) {
        fprintf(stderr, "the carve disagrees with the plan: %s\n", line.c_str());
        return 2;
      }
      free(block);
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
