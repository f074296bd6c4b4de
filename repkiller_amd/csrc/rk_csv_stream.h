// rk_csv_stream.h -- host pieces read as ONE byte stream: the bodies of a
// batch's files as rk_dbset_load_csv_device parses them (rk_csv.hip) and as
// the staging ring gathers them (rk_io.hip).  Host code only, no HIP; the
// offset arithmetic is checked on its own by tests/cpp/csv_stream_check.cpp.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace rk {

// Piece k is bytes [off[k], off[k] + len(k)) of the stream and, where nl[k] is
// set, one '\n' right after them; off has n + 1 entries,
// off[k + 1] - off[k] = len(k) + nl[k]
struct IoStream {
  const char *const *p;
  const uint64_t *off;
  const uint8_t *nl;
  size_t n;
};

// stream bytes [lo, hi) to dst (hi <= off[n]): the pieces in turn, the appended
// '\n' where nl says
inline void stream_fill(const IoStream &s, char *dst, uint64_t lo, uint64_t hi) {
  size_t k = (size_t)(std::upper_bound(s.off, s.off + s.n + 1, lo) - s.off) - 1;
  while (lo < hi && k < s.n) {
    const uint64_t plen = s.off[k + 1] - s.off[k] - s.nl[k], r = lo - s.off[k];
    if (r < plen) {
      const uint64_t c = std::min(hi - lo, plen - r);
      std::memcpy(dst, s.p[k] + r, (size_t)c);
      dst += c, lo += c;
    }
    if (lo < hi && s.nl[k] && lo == s.off[k] + plen) *dst++ = '\n', ++lo;
    ++k;
  }
}

// The bytes a load parses: the body of one mapped file (one piece, nothing
// appended), or the bodies of a batch's files, where every non-empty body that
// does not end in a newline gets one, so a line lies in one piece.
struct CsvStream {
  std::vector<const char *> p;
  std::vector<uint64_t> off{0};  // pieces + 1
  std::vector<uint8_t> nl;
  void add(const char *body, uint64_t len, bool newline) {
    p.push_back(body);
    nl.push_back(newline ? 1 : 0);
    off.push_back(off.back() + len + (newline ? 1 : 0));
  }
  uint64_t size() const { return off.back(); }
  IoStream io() const { return IoStream{p.data(), off.data(), nl.data(), p.size()}; }
  // the piece that holds stream byte at (< size()); empty pieces hold none
  size_t piece_of(uint64_t at) const {
    return (size_t)(std::upper_bound(off.begin(), off.end(), at) - off.begin()) - 1;
  }
  uint64_t plen(size_t k) const { return off[k + 1] - off[k] - nl[k]; }
  char at(uint64_t a) const {
    const size_t k = piece_of(a);
    return a - off[k] < plen(k) ? p[k][a - off[k]] : '\n';
  }
  // bytes [a, a + len) where they lie in one piece's own bytes, else null (an
  // empty range is never null)
  const char *span(uint64_t a, uint64_t len) const {
    if (!len) return "";
    if (a >= size()) return nullptr;
    const size_t k = piece_of(a);
    return a - off[k] + len <= plen(k) ? p[k] + (a - off[k]) : nullptr;
  }
  // the last '\n' in [a, b) (a < b <= size()); ~0 when there is none
  uint64_t last_nl(uint64_t a, uint64_t b) const {
    for (size_t k = piece_of(b - 1) + 1; k-- > 0 && off[k + 1] > a;) {
      const uint64_t e = off[k] + plen(k);
      if (nl[k] && e >= a && e < b) return e;
      const uint64_t lo = std::max(a, off[k]), hi = std::min(b, e);
      if (lo < hi) {
        const void *q = memrchr(p[k] + (lo - off[k]), '\n', (size_t)(hi - lo));
        if (q) return off[k] + (uint64_t)((const char *)q - p[k]);
      }
    }
    return ~0ull;
  }
  // the first '\n' in [a, size()) (a < size()); ~0 when there is none
  uint64_t next_nl(uint64_t a) const {
    for (size_t k = piece_of(a); k < p.size(); ++k) {
      const uint64_t e = off[k] + plen(k), lo = std::max(a, off[k]);
      if (lo < e) {
        const void *q = std::memchr(p[k] + (lo - off[k]), '\n', (size_t)(e - lo));
        if (q) return off[k] + (uint64_t)((const char *)q - p[k]);
      }
      if (nl[k] && e >= a) return e;
    }
    return ~0ull;
  }
};

}  // namespace rk
