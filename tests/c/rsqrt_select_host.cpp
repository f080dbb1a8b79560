// tog_rsqrt_select against tog_rsqrt (include/tog_math.h), bit for bit, on the host (tests/test_rsqrt_select.py
// builds this with -fsanitize=address,undefined): every input class, then 2^20 seeded normals across the exponent
// range. Prints the number of values compared and "ok", or the first mismatch.
//
// Two units from this one file. The reference's seed subtracts in signed arithmetic, which overflows for -0.0 and
// the small negative y (the result is then dropped by its class test); with -DRSQRT_REFERENCE_UNIT the file is just
// that call, built without the signed-overflow check, so that those inputs can reach it. The form under test is
// built with every check.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "tog_math.h"

extern "C" double rsqrt_reference(double y);

#ifdef RSQRT_REFERENCE_UNIT
extern "C" double rsqrt_reference(double y) { return tog_rsqrt(y); }
#else
static uint64_t bits(double v) {
  uint64_t b;
  std::memcpy(&b, &v, sizeof(b));
  return b;
}

static double from_bits(uint64_t b) {
  double v;
  std::memcpy(&v, &b, sizeof(v));
  return v;
}

static long checked = 0;

static bool same(double y) {
  const double a = rsqrt_reference(y), b = tog_rsqrt_select(y);
  checked++;
  if (bits(a) == bits(b)) return true;
  std::printf("mismatch at y = %a (0x%016llx): tog_rsqrt 0x%016llx, tog_rsqrt_select 0x%016llx\n", y,
              (unsigned long long)bits(y), (unsigned long long)bits(a), (unsigned long long)bits(b));
  return false;
}

int main() {
  const double classes[] = {0.0,     from_bits(1), from_bits(0x0008000000000000ull), DBL_MIN, 1.0, DBL_MAX,
                            INFINITY, -0.0,        -1.0,                             NAN,     -DBL_MIN, -0.125,
                            -INFINITY, from_bits(0xfff8000000000000ull)};
  for (double y : classes)
    if (!same(y)) return 1;
  // the classes' values, not only their agreement
  if (!(tog_rsqrt_select(0.0) == INFINITY && tog_rsqrt_select(-0.0) == INFINITY && tog_rsqrt_select(INFINITY) == 0.0 &&
        tog_rsqrt_select(1.0) == 1.0 && std::isnan(tog_rsqrt_select(-1.0)) && std::isnan(tog_rsqrt_select(NAN)))) {
    std::printf("class values\n");
    return 1;
  }
  // 2^20 normals: a 64-bit LCG (Knuth's MMIX constants) gives the mantissa and an exponent over the whole
  // normal range [1, 2046]
  uint64_t s = 0x9E3779B97F4A7C15ull;
  for (int i = 0; i < (1 << 20); i++) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    const uint64_t mant = (s >> 12) & 0x000FFFFFFFFFFFFFull;
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    const uint64_t expo = 1 + (s >> 33) % 2046;
    if (!same(from_bits((expo << 52) | mant))) return 1;
  }
  std::printf("%ld\nok\n", checked);
  return 0;
}
#endif
