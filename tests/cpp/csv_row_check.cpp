// csv_row_check -- the shared row function (rk_csv_row.h), compiled for the
// host, against the host formatter (rk::db_format_row) and snprintf, row by row.
//
//   csv_row_check full  <workdir> <out.csv>...   (linked with librepkiller_amd)
//   csv_row_check check <workdir>                (stand-alone; -DRK_NO_LIB)
//
// full: every body row of every <out.csv> (its columns read back from the text)
// plus 300k rows of a seeded grammar are put into an rk_db, formatted with
// rk::db_format_row, and dumped: the rows to <workdir>/rows.bin, the host's
// text to <workdir>/host.bin; then the check runs.
// check: the same check from the two dumps alone, so a sanitized build never
// loads the HIP library.
//
// Per row the check evaluates for itself, with snprintf,
//   exact(f) = f is +0, or f is in [1e-3f, 1e6f) and "%.6g" of it is not "1e+06"
// and requires csv_row to return ROW_DEVICE iff exact(similarity) and
// exact(identity), ROW_HOST otherwise -- a two-way classification, nothing left
// out.  A ROW_DEVICE row must have the host's length and bytes, from the
// length-only call too, written into a buffer of exactly that size.  Every
// row's host text must be the row rebuilt here with snprintf.  Then the float
// function alone: 2 M random bit patterns, 2 M uniform and 1 M log-uniform
// values of [1e-3, 1e6), and the edges, against snprintf; rk::put_float
// (rk_format.h) must print every one of them as snprintf does.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "rk_csv_row.h"
#include "rk_format.h"
#ifndef RK_NO_LIB
#include "rk_db.h"
#endif

namespace {

#pragma pack(push, 1)
struct Rec {
  uint64_t v[7];  // xs ys xe ye len score ident
  uint32_t sim;   // bits
  uint8_t strand;
  uint64_t gid;
  uint32_t rep;
};
#pragma pack(pop)

struct Rng {
  uint64_t s;
  uint64_t next() {
    s ^= s << 13, s ^= s >> 7, s ^= s << 17;
    return s;
  }
  uint64_t below(uint64_t n) { return next() % n; }
  double unit() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
};

float from_bits(uint32_t b) {
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}
uint32_t to_bits(float f) {
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return b;
}

std::string slurp(const std::string &path) {
  std::ifstream f(path, std::ios::binary);
  std::stringstream ss;
  ss << f.rdbuf();
  return ss.str();
}

uint64_t pow10u(int k) {
  uint64_t p = 1;
  while (k-- > 0) p *= 10;
  return p;
}

// 0, 9, 10, every power of ten +- 1 up to 10^19, 2^64 - 1, or any digit count
uint64_t edge_u64(Rng &r) {
  switch (r.below(8)) {
    case 0: return r.below(3) == 0 ? 0 : r.below(2) ? 9 : 10;
    case 1: return pow10u(1 + (int)r.below(19)) - 1;
    case 2: return pow10u(1 + (int)r.below(19));
    case 3: return pow10u(1 + (int)r.below(19)) + 1;
    case 4: return ~0ull;
    default: {
      const int d = 1 + (int)r.below(20);  // digit count 1..20
      if (d == 20) return pow10u(19) + r.next() % (~0ull - pow10u(19));
      const uint64_t lo = d == 1 ? 0 : pow10u(d - 1);
      return lo + r.next() % (pow10u(d) - lo);
    }
  }
}

const float kEdges[] = {1e-3f, 1e6f, 999999.94f, 999999.9f, 999999.5f, 99999.95f, 9999.995f,
                        0.00099999f, 0.5f, 1.0f, 100.0f, 99.99995f, 0.001f, 123456.5f,
                        0.0f, -0.0f, -1.5f, -1e-3f, 1e-45f, 1e-40f, 1.17549421e-38f, 1e7f, 3e38f,
                        0.000999999f, 1000000.06f, 16777216.0f, 8388608.0f, 0.0999999f};

float edge_float(Rng &r) {
  switch (r.below(12)) {
    case 0: return from_bits((uint32_t)r.next());
    case 1: return std::nextafterf(1e-3f, r.below(2) ? 0.0f : 1.0f);
    case 2: return std::nextafterf(1e6f, r.below(2) ? 0.0f : 1e7f);
    case 3: return r.below(2) ? INFINITY : -INFINITY;
    case 4: return from_bits(r.below(2) ? 0x7FC00000u : 0xFFC00000u | (uint32_t)r.below(1000));
    case 5: return from_bits((uint32_t)r.below(0x800000u) | (r.below(2) ? 0x80000000u : 0u));
    case 6: return -(float)(r.unit() * 100.0);
    case 7: return kEdges[r.below(sizeof kEdges / sizeof *kEdges)];
    default: return (float)(1e-3 + r.unit() * 100.0);  // the column's usual values
  }
}

Rec gen_rec(Rng &r) {
  Rec q;
  const bool plain = r.below(2) == 0;
  for (int k = 0; k < 7; ++k) q.v[k] = plain ? r.below(pow10u(1 + (int)r.below(9))) : edge_u64(r);
  q.sim = to_bits(plain ? (float)(r.unit() * 100.0) : edge_float(r));
  q.strand = plain ? (r.below(2) ? 'f' : 'r') : (uint8_t)r.below(256);
  q.gid = r.below(3) ? r.below(1000000) : r.below(2) ? 4294967295ull : r.next() & 0xFFFFFFFFull;
  q.rep = (uint32_t)r.below(3);
  // identity pairs: v[4] = length, v[6] = ident
  switch (r.below(10)) {
    case 0: q.v[4] = 0, q.v[6] = r.below(2) ? 0 : 1 + r.below(100); break;
    case 1: q.v[6] = 0, q.v[4] = 1 + r.below(100000); break;
    case 2: q.v[4] = 1 + r.below(1000), q.v[6] = q.v[4] + 1 + r.below(1000000); break;
    case 3: q.v[4] = (1ull << 24) + r.below(1ull << 40), q.v[6] = (1ull << 24) + r.below(1ull << 40); break;
    case 4: break;  // whatever the columns drew
    default: q.v[4] = 1 + r.below(100000), q.v[6] = r.below(q.v[4] + 1); break;
  }
  return q;
}

std::string fmt_g(float f) {
  char b[48];
  std::snprintf(b, sizeof b, "%.6g", (double)f);
  return b;
}

bool exact(float f) {
  if (to_bits(f) == 0) return true;
  return f >= 1e-3f && f < 1e6f && fmt_g(f) != "1e+06";
}

float identity_of(const Rec &q) { return (float)q.v[6] * 100 / (float)q.v[4]; }

std::string snprintf_row(const Rec &q) {
  char b[512];
  const int n = std::snprintf(
      b, sizeof b,
      "Frag,%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%c,%" PRIu64 ",%" PRIu64 ",%" PRIu64
      ",%" PRIu64 ",",
      q.v[0], q.v[1], q.v[2], q.v[3], (char)q.strand, q.gid, q.v[4], q.v[5], q.v[6]);
  // (%c writes a NUL strand byte as a byte too: n counts it)
  std::string s(b, (size_t)n);
  s += fmt_g(from_bits(q.sim)) + "," + fmt_g(identity_of(q)) + ",0," + std::to_string(q.rep) + "\n";
  return s;
}

rk::OutRow as_row(const Rec &q) {
  rk::OutRow r;
  r.xs = q.v[0], r.ys = q.v[1], r.xe = q.v[2], r.ye = q.v[3], r.len = q.v[4], r.score = q.v[5];
  r.ident = q.v[6], r.sim = from_bits(q.sim), r.strand = q.strand;
  return r;
}

size_t g_bad = 0;
void fail(const char *what, const std::string &detail) {
  if (++g_bad <= 20) std::printf("%s: [%s]\n", what, detail.c_str());
}

void check_rows(const std::vector<Rec> &recs, const std::string &host, size_t *n_dev,
                size_t *n_host) {
  size_t at = 0;
  for (size_t i = 0; i < recs.size(); ++i) {
    const Rec &q = recs[i];
    if (at >= host.size()) {
      fail("host dump too short", std::to_string(i));
      return;
    }
    const size_t hl = (unsigned char)host[at];
    const std::string htext = host.substr(at + 1, hl);
    at += 1 + hl;
    const std::string want_text = snprintf_row(q);
    if (htext != want_text) fail("host formatter differs from snprintf", want_text);
    const bool dev = exact(from_bits(q.sim)) && exact(identity_of(q));
    const rk::OutRow row = as_row(q);
    uint32_t len0 = 0xFFFFFFFFu, len1 = 0xFFFFFFFFu;
    const uint8_t st0 = rk::csv_row(row, q.gid, q.rep, nullptr, &len0);
    if (st0 != (dev ? rk::ROW_DEVICE : rk::ROW_HOST)) {
      fail(st0 == rk::ROW_DEVICE ? "DEVICE unexpected" : "HOST unexpected", want_text);
      continue;
    }
    if (!dev) {
      ++*n_host;
      continue;
    }
    ++*n_dev;
    if (len0 != want_text.size() || len0 > rk::ROW_MAX) {
      fail("DEVICE with another length", want_text);
      continue;
    }
    std::vector<char> out(len0);  // exactly the row: a sanitized build sees one byte more
    const uint8_t st1 = rk::csv_row(row, q.gid, q.rep, out.data(), &len1);
    if (st1 != rk::ROW_DEVICE || len1 != len0 ||
        std::memcmp(out.data(), want_text.data(), len0) != 0)
      fail("DEVICE with other bytes", want_text);
  }
  if (at != host.size()) fail("host dump too long", std::to_string(at));
}

void check_float(float f, size_t *n_exact, size_t *n_refused) {
  const std::string want = fmt_g(f);
  char b[64];
  std::memset(b, '#', sizeof b);
  const uint32_t n = rk::row_put_float(b, f);
  const uint32_t n0 = rk::row_put_float(nullptr, f);
  if (n != n0 || (n != 0) != exact(f) || n > 10 || b[n ? n : 0] != '#')
    fail("row_put_float: predicate or length", want);
  else if (n && std::string(b, n) != want)
    fail("row_put_float: bytes", want);
  if (n) ++*n_exact;
  else ++*n_refused;
  char c[64];
  char *e = rk::put_float(c, f);
  if (std::string(c, (size_t)(e - c)) != want) fail("put_float differs from snprintf", want);
}

void check_floats(size_t *n_exact, size_t *n_refused) {
  Rng r{0xD1B54A32D192ED03ull};
  for (int i = 0; i < 2000000; ++i) check_float(from_bits((uint32_t)r.next()), n_exact, n_refused);
  for (int i = 0; i < 2000000; ++i) {
    float f = (float)(1e-3 + r.unit() * (1e6 - 1e-3));
    if (!(f < 1e6f)) f = std::nextafterf(1e6f, 0.0f);
    check_float(f, n_exact, n_refused);
  }
  for (int i = 0; i < 1000000; ++i) {
    float f = (float)std::pow(10.0, -3.0 + 9.0 * r.unit());
    if (!(f < 1e6f)) f = std::nextafterf(1e6f, 0.0f);
    if (!(f >= 1e-3f)) f = 1e-3f;
    check_float(f, n_exact, n_refused);
  }
  for (float f : kEdges) check_float(f, n_exact, n_refused);
  // 1e-3f, 1e6f and every decade between, with 64 neighbours on both sides
  for (int d = -3; d <= 6; ++d) {
    float up = (float)std::pow(10.0, d), dn = up;
    for (int k = 0; k < 64; ++k) {
      check_float(up, n_exact, n_refused), check_float(dn, n_exact, n_refused);
      up = std::nextafterf(up, INFINITY), dn = std::nextafterf(dn, 0.0f);
    }
  }
  for (uint32_t b : {0x00000001u, 0x007FFFFFu, 0x00800000u, 0x80000001u, 0x7F800000u, 0xFF800000u,
                     0x7FC00000u, 0xFFC00000u, 0x7F800001u, 0x80000000u, 0x7F7FFFFFu})
    check_float(from_bits(b), n_exact, n_refused);
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  const std::string mode = argv[1], dir = argv[2];
  const std::string rows_path = dir + "/rows.bin", host_path = dir + "/host.bin";
#ifndef RK_NO_LIB
  if (mode == "full") {
    std::vector<Rec> recs;
    size_t fixture_bad = 0;
    std::vector<std::string> fixture_lines;
    for (int a = 3; a < argc; ++a) {
      const std::string text = slurp(argv[a]);
      size_t p = 0;
      while (p < text.size()) {
        size_t nl = text.find('\n', p);
        if (nl == std::string::npos) nl = text.size();
        const std::string line = text.substr(p, nl - p);
        p = nl + 1;
        if (line.compare(0, 5, "Frag,") != 0) continue;
        std::vector<std::string> f;
        std::stringstream ss(line);
        for (std::string s; std::getline(ss, s, ',');) f.push_back(s);
        if (f.size() != 14 || f[5].size() != 1) {
          ++fixture_bad;
          continue;
        }
        Rec q;
        static const int col[7] = {1, 2, 3, 4, 7, 8, 9};
        for (int k = 0; k < 7; ++k) q.v[k] = std::strtoull(f[(size_t)col[k]].c_str(), nullptr, 10);
        q.sim = to_bits(std::strtof(f[10].c_str(), nullptr));
        q.strand = (uint8_t)f[5][0];
        q.gid = std::strtoull(f[6].c_str(), nullptr, 10);
        q.rep = (uint32_t)std::strtoul(f[13].c_str(), nullptr, 10);
        recs.push_back(q);
        fixture_lines.push_back(line + "\n");
      }
    }
    if (fixture_bad || recs.empty()) {
      std::printf("fixture rows not understood: %zu (read %zu)\n", fixture_bad, recs.size());
      return 1;
    }
    const size_t n_fix = recs.size();
    Rng rng{0x9E3779B97F4A7C15ull};
    for (int i = 0; i < 300000; ++i) recs.push_back(gen_rec(rng));
    rk_db db;
    for (const Rec &q : recs) {
      db.x_start.push_back(q.v[0]), db.y_start.push_back(q.v[1]), db.x_end.push_back(q.v[2]);
      db.y_end.push_back(q.v[3]), db.length.push_back(q.v[4]), db.score.push_back(q.v[5]);
      db.ident.push_back(q.v[6]), db.similarity.push_back(from_bits(q.sim));
      db.strand.push_back(q.strand);
    }
    std::string host;
    for (size_t i = 0; i < recs.size(); ++i) {
      char row[256];
      const char *e = rk::db_format_row(&db, (uint32_t)i, recs[i].gid, recs[i].rep, row);
      host.push_back((char)(unsigned char)(e - row));
      host.append(row, (size_t)(e - row));
      // a fixture row read back from its text formats to that text again
      if (i < n_fix && std::string(row, (size_t)(e - row)) != fixture_lines[i])
        fail("fixture row does not format back to its line", fixture_lines[i]);
    }
    std::ofstream(rows_path, std::ios::binary)
        .write((const char *)recs.data(), (std::streamsize)(recs.size() * sizeof(Rec)));
    std::ofstream(host_path, std::ios::binary).write(host.data(), (std::streamsize)host.size());
  } else
#endif
      if (mode != "check") {
    return 2;
  }
  const std::string raw = slurp(rows_path), host = slurp(host_path);
  if (raw.empty() || raw.size() % sizeof(Rec)) {
    std::printf("no rows in %s\n", rows_path.c_str());
    return 1;
  }
  std::vector<Rec> recs(raw.size() / sizeof(Rec));
  std::memcpy(recs.data(), raw.data(), raw.size());
  size_t n_dev = 0, n_host = 0, n_exact = 0, n_refused = 0;
  check_rows(recs, host, &n_dev, &n_host);
  check_floats(&n_exact, &n_refused);
  std::printf("rows %zu device %zu host %zu floats_exact %zu floats_refused %zu mismatches %zu\n",
              recs.size(), n_dev, n_host, n_exact, n_refused, g_bad);
  return g_bad ? 1 : 0;
}
