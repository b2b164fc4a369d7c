// The cache rule of csrc/atmrt_cached.h on the host, stand-alone: a product with a counting build function, driven by
// tests/test_cached_host.py.  Prints one line per failed expectation; exit status 0 when there is none.
#include "../../atm-raytracer_amd/csrc/atmrt_cached.h"
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

using atmrt::Cached;
using atmrt::bits;

static int failures = 0;
#define EXPECT(...) /* variadic: braces do not shield a comma from the preprocessor */ \
  do {                                                                                \
    if (!(__VA_ARGS__)) {                                                             \
      printf("%s:%d: expected %s\n", __FILE__, __LINE__, #__VA_ARGS__);               \
      failures++;                                                                     \
    }                                                                                 \
  } while (0)

struct Key {
  double x;
  int n;
  bool operator==(const Key& o) const { return bits(x) == bits(o.x) && n == o.n; }
};
struct Value {
  std::vector<double> table; // something a sanitizer can watch
  double x = 0.0;
};
struct DepKey {
  uint64_t source;
  int m;
  bool operator==(const DepKey& o) const { return source == o.source && m == o.m; }
};

int main() {
  int builds = 0, status = 0; // what the next build returns
  auto build = [&](const Key& k) {
    return [&builds, &status, k](Value& v) {
      builds++;
      v.table.assign(16 + builds, k.x); // overwritten before the status is known, as a device buffer would be
      v.x = k.x;
      return status;
    };
  };
  const Key A{1.5, 3}, B{2.5, 3};
  Cached<Key, Value> c;
  bool built = true;
  EXPECT(c.serial() == 0);

  // the first refresh builds; the same key does not
  EXPECT(c.refresh(A, build(A), false, &built) == 0 && built && builds == 1 && c.serial() == 1 && c.value().x == 1.5);
  EXPECT(c.refresh(A, build(A), false, &built) == 0 && !built && builds == 1 && c.serial() == 1);
  EXPECT(c.refresh(A, build(A)) == 0 && builds == 1);

  // a changed key builds and the serial grows; A -> B -> A builds three times
  EXPECT(c.refresh(B, build(B), false, &built) == 0 && built && builds == 2 && c.serial() == 2 && c.value().x == 2.5);
  EXPECT(c.refresh(A, build(A), false, &built) == 0 && built && builds == 3 && c.serial() == 3 && c.value().x == 1.5);
  EXPECT(c.refresh({1.5, 4}, build({1.5, 4})) == 0 && builds == 4 && c.serial() == 4); // every field counts
  EXPECT(c.refresh(A, build(A)) == 0 && builds == 5 && c.serial() == 5);

  // force builds with an equal key
  EXPECT(c.refresh(A, build(A), true, &built) == 0 && built && builds == 6 && c.serial() == 6);
  EXPECT(c.refresh(A, build(A), false, &built) == 0 && !built && builds == 6);

  // a failed build returns its status and leaves the product empty; the serial reads 0 while building
  uint64_t seen_while_building = 99;
  EXPECT(c.refresh(B, [&](Value&) { seen_while_building = c.serial(); return 7; }, false, &built) == 7 && !built);
  EXPECT(seen_while_building == 0 && c.serial() == 0);
  // ... the OLD key builds again: the value of before the failure is never served
  EXPECT(c.refresh(A, build(A), false, &built) == 0 && built && builds == 7 && c.serial() == 7 && c.value().x == 1.5);
  // ... and so does the NEW key after another failure
  status = -3;
  EXPECT(c.refresh(B, build(B), false, &built) == -3 && !built && builds == 8 && c.serial() == 0);
  EXPECT(c.refresh(B, build(B), false, &built) == -3 && !built && builds == 9 && c.serial() == 0); // it keeps failing, it keeps building
  status = 0;
  EXPECT(c.refresh(B, build(B), false, &built) == 0 && built && builds == 10 && c.serial() == 8 && c.value().x == 2.5);
  // a failed forced build of an equal key empties the product too
  status = 1;
  EXPECT(c.refresh(B, build(B), true) == 1 && c.serial() == 0);
  status = 0;
  EXPECT(c.refresh(B, build(B), false, &built) == 0 && built && c.serial() == 9); // serials never repeat

  // drop
  c.drop();
  EXPECT(c.serial() == 0);
  EXPECT(c.refresh(B, build(B), false, &built) == 0 && built && c.serial() == 10);

  // a dependent names its source's serial in its key
  {
    Cached<Key, Value> src;
    Cached<DepKey> dep;
    int dep_builds = 0;
    auto refresh_dep = [&](int m) { return dep.refresh({src.serial(), m}, [&](atmrt::Nothing&) { dep_builds++; return 0; }); };
    builds = 0;
    EXPECT(src.refresh(A, build(A)) == 0 && refresh_dep(1) == 0 && dep_builds == 1);
    EXPECT(src.refresh(A, build(A)) == 0 && refresh_dep(1) == 0 && dep_builds == 1 && builds == 1); // nothing changed: nothing built
    EXPECT(refresh_dep(2) == 0 && dep_builds == 2 && refresh_dep(2) == 0 && dep_builds == 2);       // its own input changed
    // the source fails, then is built again from an EQUAL key: the dependent follows
    status = 5;
    EXPECT(src.refresh(B, build(B)) == 5 && src.serial() == 0);
    status = 0;
    EXPECT(src.refresh(A, build(A)) == 0 && builds == 3);
    EXPECT(refresh_dep(2) == 0 && dep_builds == 3);
    EXPECT(refresh_dep(2) == 0 && dep_builds == 3);
    // a forced rebuild of the source rebuilds the dependent
    EXPECT(src.refresh(A, build(A), true) == 0 && refresh_dep(2) == 0 && dep_builds == 4);
  }

  // doubles compare by their bits
  {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    EXPECT(!(Key{0.0, 1} == Key{-0.0, 1}) && 0.0 == -0.0);
    EXPECT(Key{nan, 1} == Key{nan, 1} && nan != nan);
    EXPECT(!(Key{nan, 1} == Key{-nan, 1}));
    Cached<Key, Value> z;
    builds = 0;
    EXPECT(z.refresh({0.0, 1}, build({0.0, 1})) == 0 && z.refresh({-0.0, 1}, build({-0.0, 1})) == 0 && builds == 2);
    EXPECT(z.refresh({nan, 1}, build({nan, 1})) == 0 && z.refresh({nan, 1}, build({nan, 1})) == 0 && builds == 3);
  }

  printf("failures %d\n", failures);
  return failures ? 1 : 0;
}
