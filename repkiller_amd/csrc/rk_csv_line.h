// rk_csv_line.h -- one body line of a fragment CSV -> one row, for the host and
// the device alike.
//
// A restatement of rk_host.cpp's parse_line (FragmentsDatabase.cpp:17-48) that
// compiles as __host__ __device__ and takes the same decisions byte for byte:
// the line is split on ',' into 14 fields; an empty field rejects it; a line
// with fewer than 14 fields repeats its last field; field 0 must be exactly
// "Frag"; the integer fields are atoll (leading white space, sign, saturation,
// stop at the first non-digit); the strand is the first byte of field 5;
// similarity follows rk::fast_stof's rules and ident is (uint64_t)similarity
// as the x86-64 reference evaluates it.
//
// What this function never does is guess a strtof result.  When every field
// rule passes but field 10 is not on Clinger's fast path (an exponent, more
// than 7 significant digits, nan / inf, a hex float, trailing garbage, an
// ERANGE candidate) the status is CSV_HOST and the caller hands the line to
// the host's own parse_line.  A line longer than RK_CSV_MAX_LINE whose field
// rules pass is CSV_HOST too; the device row kernel does not even walk such a
// line (it reports CSV_HOST from the length alone), so a lane's walk is
// bounded by RK_CSV_MAX_LINE bytes.
//
// The fast path's (float)m / 10^frac must be ONE correctly rounded f32 divide:
// the translation unit that compiles this for the device is built with
// -fhip-fp32-correctly-rounded-divide-sqrt (csrc/Makefile).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RK_HD __host__ __device__
#else
#define RK_HD
#endif

#define RK_CSV_MAX_LINE 4096u

namespace rk {

enum : uint8_t { CSV_REJECT = 0, CSV_ACCEPT = 1, CSV_HOST = 2 };

struct CsvRow {
  uint64_t xs, ys, xe, ye, len, score, ident;
  float sim;
  uint8_t strand;
};

RK_HD inline bool csv_isspace(unsigned char c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

// atoll on the field: strtoll(s, NULL, 10) semantics, see rk_host.cpp
RK_HD inline uint64_t csv_atoll(const char *p, const char *e) {
  while (p < e && csv_isspace((unsigned char)*p)) ++p;
  bool neg = false;
  if (p < e && (*p == '+' || *p == '-')) neg = *p++ == '-';
  const unsigned long long llmax = 0x7FFFFFFFFFFFFFFFull;
  unsigned long long acc = 0;
  bool over = false;
  const unsigned long long lim = neg ? llmax + 1ull : llmax;
  for (; p < e && *p >= '0' && *p <= '9'; ++p) {
    const unsigned d = (unsigned)(*p - '0');
    if (!over && acc > (lim - d) / 10) over = true;
    if (!over) acc = acc * 10 + d;
  }
  if (over) acc = lim;
  return neg ? 0ull - acc : acc;
}

// rk::fast_stof (rk_format.h), same answers and the same refusals
RK_HD inline bool csv_fast_stof(const char *p, const char *e, float *out) {
  while (p < e && csv_isspace((unsigned char)*p)) ++p;
  bool neg = false;
  if (p < e && (*p == '+' || *p == '-')) neg = *p++ == '-';
  uint32_t m = 0;
  int digits = 0, frac = 0;
  bool any = false, dot = false;
  for (; p < e; ++p) {
    const char c = *p;
    if (c >= '0' && c <= '9') {
      any = true;
      if (m == 0 && c == '0') {
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
  const float p10[11] = {1e0f, 1e1f, 1e2f, 1e3f, 1e4f, 1e5f, 1e6f, 1e7f, 1e8f, 1e9f, 1e10f};
  const float v = (float)m / p10[frac];
  *out = neg ? -v : v;
  return true;
}

// (uint64_t)float as the x86-64 reference binary evaluates it (rk_host.cpp)
RK_HD inline uint64_t csv_cvtt_si64(float x) {
  if (x != x || x >= 9223372036854775808.0f || x < -9223372036854775808.0f)
    return 0x8000000000000000ull;
  return (uint64_t)(int64_t)x;
}
RK_HD inline uint64_t csv_float_to_u64_x86(float x) {
  if (!(x >= 9223372036854775808.0f)) return csv_cvtt_si64(x);
  return csv_cvtt_si64(x - 9223372036854775808.0f) ^ 0x8000000000000000ull;
}

// The field rules alone: the 14 field bounds, or false when readFragment
// would reject the line before it looks at a number.
RK_HD inline bool csv_fields(const char *b, const char *e, const char **fb, const char **fe) {
  const char *p = b;
  int k = 0;
  bool at_eof = false;
  while (k < 14) {
    if (at_eof) {  // the previous field stays in the string
      fb[k] = fb[k - 1];
      fe[k] = fe[k - 1];
      ++k;
      continue;
    }
    const char *c = p;
    while (c < e && *c != ',') ++c;
    fb[k] = p;
    fe[k] = c;
    if (c < e) {
      p = c + 1;
    } else {
      p = e;
      at_eof = true;
    }
    if (fe[k] == fb[k]) return false;
    ++k;
  }
  return fe[0] - fb[0] == 4 && fb[0][0] == 'F' && fb[0][1] == 'r' && fb[0][2] == 'a' &&
         fb[0][3] == 'g';
}

// One body line [b, e) (no '\n').  *r is complete only for CSV_ACCEPT.
RK_HD inline uint8_t csv_line(const char *b, const char *e, CsvRow *r) {
  const char *fb[14], *fe[14];
  if (!csv_fields(b, e, fb, fe)) return CSV_REJECT;
  if ((uint64_t)(e - b) > RK_CSV_MAX_LINE) return CSV_HOST;
  float sim;
  if (!csv_fast_stof(fb[10], fe[10], &sim)) return CSV_HOST;
  r->xs = csv_atoll(fb[1], fe[1]);
  r->ys = csv_atoll(fb[2], fe[2]);
  r->xe = csv_atoll(fb[3], fe[3]);
  r->ye = csv_atoll(fb[4], fe[4]);
  r->strand = (uint8_t)fb[5][0];
  r->len = csv_atoll(fb[7], fe[7]);
  r->score = csv_atoll(fb[8], fe[8]);
  r->ident = csv_float_to_u64_x86(sim);
  r->sim = sim;
  return CSV_ACCEPT;
}

}  // namespace rk
