// The order key of csrc/walk_types.h (order_key / order_key_value and the band keys built on
// it), compiled for the host: round trip by bits, order, and the band keys' rules.
// Prints one line per failed check; exit status 0 when there is none.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "walk_types.h"

static uint64_t bits(double v) {
  uint64_t b;
  std::memcpy(&b, &v, 8);
  return b;
}

int main() {
  const double inf = std::numeric_limits<double>::infinity();
  const double den = std::numeric_limits<double>::denorm_min();
  // ascending, -0.0 below +0.0
  const double ordered[] = {-inf, -DBL_MAX, -1.0, -den, -0.0, 0.0, den, 1.0, DBL_MAX, inf};
  const int n = (int)(sizeof(ordered) / sizeof(ordered[0]));
  int bad = 0;
  auto check = [&](bool ok, const char *what, double a, double b) {
    if (!ok) {
      std::printf("FAIL %s: %a %a\n", what, a, b);
      ++bad;
    }
  };
  auto one = [&](double v) {
    const uint64_t k = fr::order_key(v);
    check(bits(fr::order_key_value(k)) == bits(v), "round trip", v, fr::order_key_value(k));
    check(fr::band_key(v, false) == k, "band_key max", v, 0.0);
    check(fr::band_key(v, true) == ~k, "band_key min", v, 0.0);
  };
  for (int i = 0; i < n; ++i) one(ordered[i]);
  one(std::numeric_limits<double>::quiet_NaN());
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j)
      check((i < j) == (fr::order_key(ordered[i]) < fr::order_key(ordered[j])), "order", ordered[i],
            ordered[j]);
  check(bits(fr::band_key_value(0, false)) == bits(0.0), "empty max band", 0.0, 0.0);
  check(bits(fr::band_key_value(~0ull, true)) == bits(0.0), "empty min band", 0.0, 0.0);
  std::printf("%d checks failed\n", bad);
  return bad != 0;
}
