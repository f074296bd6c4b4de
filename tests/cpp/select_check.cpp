// select_check -- the host selection of rk_select.h against a naive loop, over
// seeded batch layouts (every other one with its first set starting above slot
// 0).  A stand-alone host program (tests/test_select_host.py
// builds it with the address and undefined-behaviour sanitizers): every array
// is sized exactly, so a read of an unused slot's neighbour past the end or a
// write past a set's kept rows is caught.
//
//   select_check <rounds>     prints "mismatches N"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rk_select.h"

namespace {

uint64_t state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
  state ^= state << 13, state ^= state >> 7, state ^= state << 17;
  return (uint32_t)(state >> 32);
}

constexpr uint32_t S32 = 0xDEADBEEFu;
constexpr uint8_t S8 = 0xA5;

}  // namespace

int main(int argc, char **argv) {
  const long rounds = argc > 1 ? std::atol(argv[1]) : 500;
  unsigned long long mismatches = 0, checked = 0;
  for (long r = 0; r < rounds; ++r) {
    // windows: empty ones (runs of them too), short ones around the group of
    // 16, now and then a long one; n_out below the window for about half
    const uint32_t ns = 1 + rnd() % 12;
    std::vector<uint64_t> off(ns + 1, 0), n_out(ns);
    off[0] = (r & 1) ? rnd() % 40 : 0;  // slots before it belong to no set
    for (uint32_t k = 0; k < ns; ++k) {
      const uint32_t kind = rnd() % 8;
      const uint64_t w = kind < 2 ? 0 : kind < 6 ? rnd() % 40 : kind < 7 ? 15 + rnd() % 3 : rnd() % 700;
      off[k + 1] = off[k] + w;
      n_out[k] = (rnd() & 1) ? w : (w ? rnd() % (w + 1) : 0);
    }
    const uint64_t n = off[ns];
    std::vector<uint32_t> order(n), gid(n);
    std::vector<uint8_t> rep(n);
    static const uint8_t flags[] = {0, 1, 2, 2, 2, 3, 255};
    for (uint64_t p = 0; p < n; ++p) order[p] = rnd(), gid[p] = rnd(), rep[p] = flags[rnd() % 7];
    for (uint64_t p = 0; p < off[0]; ++p) rep[p] = 1, order[p] = 0xFFFFFFFFu;
    for (uint32_t k = 0; k < ns; ++k)  // unused slots read as kept rows if read at all
      for (uint64_t p = off[k] + n_out[k]; p < off[k + 1]; ++p) rep[p] = 1, order[p] = 0xFFFFFFFFu;
    for (uint32_t keep = 1; keep <= 7; ++keep) {
      std::vector<uint32_t> oo(n, S32), og(n, S32), wo(n, S32), wg(n, S32);
      std::vector<uint8_t> orp(n, S8), wr(n, S8);
      std::vector<uint64_t> kept(ns, 99), want(ns, 0);
      uint64_t by[4], wby[4] = {0, 0, 0, 0};
      rk::select_host(rk::SelTab{off.data(), n_out.data(), ns}, order.data(), gid.data(),
                      rep.data(), keep, oo.data(), og.data(), orp.data(), kept.data(), by);
      for (uint32_t k = 0; k < ns; ++k)
        for (uint64_t p = off[k]; p < off[k] + n_out[k]; ++p) {
          const uint8_t f = rep[p];
          ++wby[f < 3 ? f : 3];
          if (f > 2 || !((keep >> f) & 1u)) continue;
          const uint64_t d = off[k] + want[k]++;
          wo[d] = order[p], wg[d] = gid[p], wr[d] = f;
        }
      bool ok = oo == wo && og == wg && orp == wr && kept == want;
      for (int i = 0; i < 4; ++i) ok = ok && by[i] == wby[i];
      mismatches += !ok;
      ++checked;
    }
    // the pieces on their own
    for (uint64_t p = off[0]; p < n; ++p) {
      const uint32_t s = rk::sel_set_of(rk::SelTab{off.data(), n_out.data(), ns}, 0, p);
      mismatches += !(off[s] <= p && p < off[s + 1]);
    }
  }
  for (uint32_t f = 0; f < 256; ++f)
    for (uint32_t keep = 0; keep <= 7; ++keep)
      mismatches += rk::sel_keep(f, keep) != (f <= 2 && ((keep >> f) & 1u));
  std::printf("selections %llu mismatches %llu\n", checked, mismatches);
  return mismatches ? 1 : 0;
}
