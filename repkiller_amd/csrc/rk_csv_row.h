// rk_csv_row.h -- one output row of the result CSV -> its bytes, for the host
// and the device alike.
//
// A restatement of rk_host.cpp's format_row (store_frag,
// commonFunctions.cpp:101-104) that compiles as __host__ __device__:
//   Frag,xStart,yStart,xEnd,yEnd,strand,gid,length,score,ident,similarity,
//   identity,0,rep\n
// with identity = (float)ident * 100 / (float)length: one f32 multiply and ONE
// correctly rounded f32 divide -- the translation unit that compiles this for
// the device is built with -fhip-fp32-correctly-rounded-divide-sqrt and
// -ffp-contract=off (csrc/Makefile).  Nothing goes through f64.
//
// ostream << float prints "%.6g".  row_put_float is the integer path of
// rk::put_float (rk_format.h, which now calls it): exact for +0 and for the
// floats in [1e-3, 1e6) whose six significant digits do not round up to
// 1000000.  What this function never does is imitate snprintf: for any other
// value in either float column (-0, negatives, NaN / inf, denormals, values
// below 1e-3 or at and above 1e6, the floats just below 1e6 that print as
// 1e+06) it refuses, the row's status is ROW_HOST, and the caller hands the row
// to the host's own formatter (rk::db_format_row).  The predicate is exact:
// tests/cpp/csv_row_check.cpp checks it as a two-way classification.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RK_HD __host__ __device__
#else
#define RK_HD
#endif

namespace rk {

enum : uint8_t { ROW_DEVICE = 1, ROW_HOST = 2 };

// "Frag," + ten integer fields of at most 20 digits and a comma + two floats
// of at most 15 bytes and a comma + "f," "0," and the newline (the bound
// rk_host.cpp's writer sizes its buffers with): a row's length fits one byte
constexpr uint32_t ROW_MAX = 5 + 10 * 21 + 2 * 16 + 4;
static_assert(ROW_MAX < 256, "a row's length must fit one byte");

struct OutRow {
  uint64_t xs, ys, xe, ye, len, score, ident;
  float sim;
  uint8_t strand;
};

RK_HD inline uint32_t row_float_bits(float f) {
  union {
    float f;
    uint32_t u;
  } c;
  c.f = f;
  return c.u;
}

RK_HD inline uint32_t row_u64_digits(uint64_t v) {
  uint32_t k = 1;
  uint64_t p = 10;
  while (v >= p) {
    ++k;
    if (k == 20) break;  // 10^20 does not fit; v < 2^64 has at most 20 digits
    p *= 10;
  }
  return k;
}

// the decimal digits of v at o (o null: nothing is written); returns their count
RK_HD inline uint32_t row_put_u64(char *o, uint64_t v) {
  const uint32_t k = row_u64_digits(v);
  if (o)
    for (uint32_t i = k; i-- > 0;) {
      o[i] = (char)('0' + (uint32_t)(v % 10));
      v /= 10;
    }
  return k;
}

// "%.6g" of f at o (o null: the length alone), at most 10 bytes; 0 when f is
// not one of the values this path prints exactly (see the file comment)
RK_HD inline uint32_t row_put_float(char *o, float f) {
  const uint32_t bits = row_float_bits(f);
  if (bits == 0) {  // +0.0
    if (o) o[0] = '0';
    return 1;
  }
  if (!(f >= 1e-3f && f < 1e6f)) return 0;
  const int ebin = (int)((bits >> 23) & 0xFF);
  const uint64_t m = (bits & 0x7FFFFFu) | 0x800000u;  // normal: f >= 1e-3
  const int k = ebin - 150;                            // f = m * 2^k
  // decimal exponent e (f in [10^e, 10^(e+1))), e in [-3, 5]
  const float p10[10] = {1e-3f, 1e-2f, 1e-1f, 1e0f, 1e1f, 1e2f, 1e3f, 1e4f, 1e5f, 1e6f};
  int e = -3;
  while (e < 5 && f >= p10[e + 4]) ++e;
  const int q = 5 - e;  // 0..8: N = round(f * 10^q), 6 digits
  uint64_t t10 = 1;
  for (int i = 0; i < q; ++i) t10 *= 10;
  // f * 10^q = m * 10^q * 2^k; k < 0 here unless f >= 2^23 (not in range)
  const uint64_t num = m * t10;
  uint64_t N;
  if (k >= 0) {
    N = num << k;
  } else {
    const int s = -k;
    if (s >= 64) return 0;
    N = num >> s;
    const uint64_t rem = num & ((1ull << s) - 1ull), half = 1ull << (s - 1);
    if (rem > half || (rem == half && (N & 1ull))) ++N;
  }
  if (N >= 1000000ull) {  // rounded up to the next decade
    N /= 10;              // exact: N == 1000000
    ++e;
    if (e >= 6) return 0;  // prints as 1e+06
  }
  // %g: fixed notation for -4 <= e < 6 with 6 significant digits, trailing
  // zeros (and a trailing point) removed
  uint32_t d[6];
  uint32_t n32 = (uint32_t)N;
  for (int i = 5; i >= 0; --i) d[i] = n32 % 10, n32 /= 10;
  int last = 5;
  while (last > 0 && d[last] == 0) --last;
  uint32_t n = 0;
  auto put = [&](char c) {
    if (o) o[n] = c;
    ++n;
  };
  if (e >= 0) {
    for (int i = 0; i <= e; ++i) put((char)('0' + d[i]));
    if (last > e) {
      put('.');
      for (int i = e + 1; i <= last; ++i) put((char)('0' + d[i]));
    }
  } else {
    put('0');
    put('.');
    for (int i = 0; i < -e - 1; ++i) put('0');
    for (int i = 0; i <= last; ++i) put((char)('0' + d[i]));
  }
  return n;
}

RK_HD inline float row_identity(uint64_t ident, uint64_t length) {
  return (float)ident * 100 / (float)length;
}

// One row.  o null: the status and the length alone.  *len and the bytes at o
// are complete only for ROW_DEVICE (at most ROW_MAX bytes).
RK_HD inline uint8_t csv_row(const OutRow &r, uint64_t gid, unsigned rep, char *o, uint32_t *len) {
  const float identity = row_identity(r.ident, r.len);
  if (!row_put_float(nullptr, r.sim) || !row_put_float(nullptr, identity)) return ROW_HOST;
  uint32_t n = 0;
  auto lit = [&](char c) {
    if (o) o[n] = c;
    ++n;
  };
  auto num = [&](uint64_t v) {
    n += row_put_u64(o ? o + n : nullptr, v);
    lit(',');
  };
  lit('F'), lit('r'), lit('a'), lit('g'), lit(',');
  num(r.xs), num(r.ys), num(r.xe), num(r.ye);
  lit((char)r.strand), lit(',');
  num(gid), num(r.len), num(r.score), num(r.ident);
  n += row_put_float(o ? o + n : nullptr, r.sim);
  lit(',');
  n += row_put_float(o ? o + n : nullptr, identity);
  lit(','), lit('0'), lit(',');
  n += row_put_u64(o ? o + n : nullptr, rep);
  lit('\n');
  *len = n;
  return ROW_DEVICE;
}

}  // namespace rk
