// csv_stream_check -- the offset arithmetic of rk_csv_stream.h against a plain
// concatenation.  Random piece lists (empty pieces, pieces with and without a
// final newline, the batch's rule for the appended newline) are held in heap
// buffers of their exact size, so a read past a piece is a sanitizer error when
// this is built with -fsanitize=address,undefined.  Checked against the
// concatenated string: stream_fill over ranges that start and end inside
// pieces, on the appended newlines and on piece seams; at(); span(); last_nl();
// next_nl(); piece_of().
//
//   csv_stream_check [rounds]      prints "mismatches N", exit 0 when N == 0
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "rk_csv_stream.h"

namespace {

uint64_t bad = 0;

void expect(bool ok, const char *what, uint64_t a, uint64_t b) {
  if (ok) return;
  if (++bad <= 20) std::fprintf(stderr, "mismatch: %s (%llu, %llu)\n", what,
                                (unsigned long long)a, (unsigned long long)b);
}

void round_of(std::mt19937_64 &rnd, bool batch_rule) {
  const size_t pieces = batch_rule ? 1 + rnd() % 40 : 1;
  std::vector<std::unique_ptr<char[]>> mem;
  rk::CsvStream s;
  std::string all;
  for (size_t k = 0; k < pieces; ++k) {
    // lengths around the seams of the copy loop: 0, 1, 2, and a spread
    const uint64_t pick = rnd() % 8;
    const uint64_t len = pick == 0 ? 0 : pick == 1 ? 1 : pick == 2 ? 2 : rnd() % 300;
    mem.emplace_back(new char[len ? len : 1]);
    char *p = mem.back().get();
    for (uint64_t i = 0; i < len; ++i) p[i] = rnd() % 9 == 0 ? '\n' : (char)('a' + rnd() % 26);
    // the batch's rule: a non-empty body that does not end in '\n' gets one;
    // a single file's body gets nothing
    const bool nl = batch_rule && len && p[len - 1] != '\n';
    s.add(p, len, nl);
    all.append(p, len);
    if (nl) all.push_back('\n');
  }
  const uint64_t n = s.size();
  expect(n == all.size(), "size", n, all.size());
  if (!n) return;
  const rk::IoStream io = s.io();
  for (int t = 0; t < 200; ++t) {
    uint64_t a = rnd() % n, b = a + 1 + rnd() % (n - a);
    if (t == 0) a = 0, b = n;
    if (t % 7 == 1) {  // a range that starts and ends on piece seams
      a = s.off[rnd() % pieces];
      b = s.off[1 + rnd() % pieces];
      if (a >= b) continue;
    }
    std::unique_ptr<char[]> out(new char[b - a]);
    rk::stream_fill(io, out.get(), a, b);
    expect(all.compare(a, b - a, out.get(), b - a) == 0, "stream_fill", a, b);
    const size_t lr = all.rfind('\n', b - 1);
    const uint64_t want_last = lr == std::string::npos || lr < a ? ~0ull : lr;
    expect(s.last_nl(a, b) == want_last, "last_nl", a, b);
    const size_t nf = all.find('\n', a);
    expect(s.next_nl(a) == (nf == std::string::npos ? ~0ull : nf), "next_nl", a, 0);
    expect(s.at(a) == all[a], "at", a, 0);
    const size_t k = s.piece_of(a);
    expect(k < pieces && s.off[k] <= a && a < s.off[k + 1], "piece_of", a, k);
    // a span inside one piece's own bytes is that piece's memory; one that
    // takes an appended newline or crosses a seam is refused
    const uint64_t len = b - a;
    const char *sp = s.span(a, len);
    const bool inside = a - s.off[k] + len <= s.plen(k);
    expect((sp != nullptr) == inside, "span null", a, len);
    if (sp && inside) expect(all.compare(a, len, sp, len) == 0, "span bytes", a, len);
    expect(s.span(a, 0) != nullptr, "empty span", a, 0);
  }
  expect(s.span(n, 0) != nullptr && s.span(n, 1) == nullptr, "span at the end", n, 0);
  if (batch_rule) expect(all.back() == '\n', "a batch's stream ends in a newline", n, 0);
}

}  // namespace

int main(int argc, char **argv) {
  const int rounds = argc > 1 ? std::atoi(argv[1]) : 2000;
  std::mt19937_64 rnd(20240611);
  for (int r = 0; r < rounds; ++r) round_of(rnd, r % 5 != 0);
  std::printf("rounds %d mismatches %llu\n", rounds, (unsigned long long)bad);
  return bad ? 1 : 0;
}
