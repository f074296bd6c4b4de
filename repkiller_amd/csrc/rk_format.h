// rk_format.h -- number formatting of the reference's output rows
// (commonFunctions.cpp:101-104: ofstream << uint64_t, << float).
//
// ostream << float widens to double and prints "%.*g" with precision 6.
// put_float reproduces that exactly without snprintf for the range the
// output actually holds (similarity and identity percentages): positive
// finite floats in [1e-3, 1e6).  There the float is m * 2^k with m < 2^24 and
// -34 <= k <= 0... and v * 10^(5-e) (e = the decimal exponent) is an exact
// rational num / 2^s with num < 2^63, so the 6-significant-digit integer is
// rounded to nearest-even on the exact binary value, as glibc's printf does.
// Everything else (-0, negatives, NaN/inf, tiny or huge values) goes to
// snprintf; +0 prints as "0" either way.  tests/test_format.py compares both paths over every value the
// generator can write and millions of random floats.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "rk_csv_row.h"

namespace rk {

inline char *put_u64(char *o, uint64_t v) {
  char t[24];
  int k = 0;
  do {
    t[k++] = (char)('0' + v % 10);
    v /= 10;
  } while (v);
  while (k) *o++ = t[--k];
  return o;
}

inline char *put_float_slow(char *o, float f) {
  return o + std::snprintf(o, 40, "%.6g", (double)f);
}

// the integer path lives in rk_csv_row.h (row_put_float), where the device
// egress compiles it too; what it refuses goes to snprintf
inline char *put_float(char *o, float f) {
  const uint32_t n = row_put_float(o, f);
  return n ? o + n : put_float_slow(o, f);
}

// The common spelling of the similarity column ("93.45": optional leading
// blanks and sign, digits, an optional '.' and digits, nothing after) with at
// most 7 significant digits: the decimal mantissa m < 2^24 and 10^k (k <= 10)
// are exact floats, so m / 10^k in float arithmetic is the correctly rounded
// value strtof returns (Clinger's fast path).  Anything else returns false
// and the caller uses strtof (tests/cpp/stof_check.cpp compares the two).
inline bool fast_stof(const char *p, const char *e, float *out) {
  while (p < e && (*p == ' ' || (*p >= '\t' && *p <= '\r'))) ++p;
  bool neg = false;
  if (p < e && (*p == '+' || *p == '-')) neg = *p++ == '-';
  uint32_t m = 0;
  int digits = 0, frac = 0;
  bool any = false, dot = false;
  for (; p < e; ++p) {
    const char c = *p;
    if (c >= '0' && c <= '9') {
      any = true;
      if (m == 0 && c == '0') {  // leading zeros add no significant digit
        if (dot) ++frac;
        continue;
      }
      if (++digits > 7) return false;
      m = m * 10 + (uint32_t)(c - '0');
      if (dot) ++frac;
    } else if (c == '.' && !dot) {
      dot = true;
    } else {
      return false;
    }
  }
  if (!any || frac > 10) return false;
  static const float p10[] = {1e0f, 1e1f, 1e2f, 1e3f, 1e4f, 1e5f, 1e6f, 1e7f, 1e8f, 1e9f, 1e10f};
  const float v = (float)m / p10[frac];
  *out = neg ? -v : v;
  return true;
}

}  // namespace rk
