// rk_select.h -- selection of result rows by repeat flag, for the host and the
// device alike (rk_select.hip compiles it for both; tests/cpp/select_check.cpp
// for the host alone).
//
// The flag is chosen when a group is saved (save_frags_from_group,
// commonFunctions.cpp:106-115): 0 singleton, 1 representative, 2 repeated; the
// result arrays are in output order (commonFunctions.cpp:126-128).  A stable
// selection of their entries is therefore the reference's file with the
// unwanted Frag lines deleted.
//
// The arrays are in rk_batch_result layout: set s owns slots
// [off[s], off[s + 1]); the first n_out[s] of them are USED, the rest hold
// anything.  A used slot is kept when its flag f <= 2 and bit f of `keep` is
// set; a kept slot goes to off[s] + (its rank among its set's kept slots).
// One result is the batch of one set, off = {0, n_out}.  off[0] may be above
// zero (as rk_classify_batch's set_off): slots before it belong to no set and
// are neither read nor written.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RK_HD __host__ __device__
#else
#define RK_HD
#endif

namespace rk {

constexpr uint32_t SEL_GROUP = 16;  // slots a lane takes at once: one 16-B word of flags

struct SelTab {
  const uint64_t *off;    // nsets + 1, non-decreasing
  const uint64_t *n_out;  // nsets, n_out[s] <= off[s + 1] - off[s]
  uint32_t ns;
};

RK_HD inline bool sel_keep(uint32_t flag, uint32_t keep) {
  return flag <= 2u && ((keep >> flag) & 1u);
}

// the set of slot p < off[ns]: the last s with off[s] <= p (an empty set shares
// its offset with the next one and is never the answer); lo: a set known to
// start at or before p
RK_HD inline uint32_t sel_set_of(const SelTab &t, uint32_t lo, uint64_t p) {
  uint32_t hi = t.ns;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (t.off[mid] <= p) lo = mid;
    else hi = mid;
  }
  return lo;
}

// where the kept slot whose exclusive kept-prefix (over all slots) is `prefix`
// goes: its set starts at off_s and the prefix at off_s is base_s
RK_HD inline uint64_t sel_dst(uint64_t off_s, uint64_t base_s, uint64_t prefix) {
  return off_s + (prefix - base_s);
}

// A position in the set table, moved forward only.
struct SelCur {
  uint32_t s;
  uint64_t lo, end, used_end;  // off[s], off[s + 1], off[s] + n_out[s]
};

RK_HD inline void sel_load(const SelTab &t, SelCur &c, uint32_t s) {
  c.s = s;
  c.lo = t.off[s];
  c.end = t.off[s + 1];
  c.used_end = c.lo + t.n_out[s];
}

// the cursor at slot p (>= the cursor's own set's start, < off[ns])
RK_HD inline void sel_seek(const SelTab &t, SelCur &c, uint64_t p) {
  if (p >= c.end) sel_load(t, c, sel_set_of(t, c.s, p));
}

// flag j of a 16-B word of flags held as four little-endian dwords
RK_HD inline uint32_t sel_flag(const uint32_t w[4], uint32_t j) {
  return (w[j >> 2] >> (8u * (j & 3u))) & 0xFFu;
}

// Kept bits of the slots [p0, p0 + cnt), cnt <= SEL_GROUP, whose flags are w;
// c is at or before p0 and ends at the last slot's set.  *by gains, in four
// 8-bit fields, the used slots with flag 0, 1, 2 and anything else.
RK_HD inline uint32_t sel_mask(const SelTab &t, SelCur &c, uint64_t p0, uint32_t cnt,
                               const uint32_t w[4], uint32_t keep, uint32_t *by) {
  uint32_t m = 0, b = 0;
#if defined(__clang__)
#pragma unroll
#endif
  for (uint32_t j = 0; j < SEL_GROUP; ++j) {
    if (j < cnt) {
      const uint64_t p = p0 + j;
      sel_seek(t, c, p);
      if (p < c.used_end) {
        const uint32_t f = sel_flag(w, j);
        b += 1u << (8u * (f < 3u ? f : 3u));
        if (sel_keep(f, keep)) m |= 1u << j;
      }
    }
  }
  *by += b;
  return m;
}

// The host selection: the same walk in groups of SEL_GROUP slots from off[0]
// on, one cursor.
// kept[s] = rows of set s written from off[s] on; entries of `out` past them
// are not written.  by_flag[4]: used slots by flag (0, 1, 2, other).
inline void select_host(const SelTab &t, const uint32_t *order, const uint32_t *gid,
                        const uint8_t *rep, uint32_t keep, uint32_t *out_order, uint32_t *out_gid,
                        uint8_t *out_rep, uint64_t *kept, uint64_t by_flag[4]) {
  for (int i = 0; i < 4; ++i) by_flag[i] = 0;
  for (uint32_t s = 0; s < t.ns; ++s) kept[s] = 0;
  if (!t.ns || t.off[t.ns] == t.off[0]) return;
  const uint64_t first = t.off[0], n = t.off[t.ns];
  SelCur c;
  sel_load(t, c, sel_set_of(t, 0, first));
  uint64_t prefix = 0, base = 0;  // kept before the slot / before the cursor's set
  uint32_t at = c.s;
  for (uint64_t p0 = first; p0 < n; p0 += SEL_GROUP) {
    const uint32_t cnt = (uint32_t)(n - p0 < SEL_GROUP ? n - p0 : SEL_GROUP);
    uint32_t w[4] = {0, 0, 0, 0};
    for (uint32_t j = 0; j < cnt; ++j) w[j >> 2] |= (uint32_t)rep[p0 + j] << (8u * (j & 3u));
    SelCur walk = c;
    uint32_t by = 0;
    const uint32_t m = sel_mask(t, c, p0, cnt, w, keep, &by);
    for (int i = 0; i < 4; ++i) by_flag[i] += (by >> (8 * i)) & 0xFFu;
    for (uint32_t j = 0; j < cnt; ++j) {
      if (!((m >> j) & 1u)) continue;
      sel_seek(t, walk, p0 + j);
      if (walk.s != at) at = walk.s, base = prefix;
      const uint64_t d = sel_dst(walk.lo, base, prefix);
      out_order[d] = order[p0 + j], out_gid[d] = gid[p0 + j], out_rep[d] = rep[p0 + j];
      ++kept[at];
      ++prefix;
    }
  }
}

}  // namespace rk
