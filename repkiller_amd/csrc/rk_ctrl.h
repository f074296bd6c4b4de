// rk_ctrl.h -- the 32-bit control words through which the drivers talk to
// their kernels, the spans the host reads back, and the pinned buffer they
// land in.  This file is the one description of these layouts: kernels, call
// sites and message layouts use its names.  Every value is fixed -- the
// sharded words travel between ranks inside the gathered messages.
#pragma once
#include <stdint.h>

namespace rk {

// words of one occupancy-sweep counter block (their sum: the waves / runs
// still pending after the sweep)
constexpr uint32_t PEND_WORDS = 64;

// ---- the single-device blocks: Work::ctrl (generic pipeline) and
// NWork::ctrl (record pipeline), rk_api.hip ---------------------------------
enum : uint32_t {
  CW_ERR = 0,           // error bits (ERRB_*)
  CW_KEPT = 1,          // kept rows
  CW_SWEEP_COUNT = 2,   // the sweep scratch's device count (build_runs' long runs)
  CW_NOPACK = 3,        // some row does not pack into a 16-B record
  CW_MAXLEN = 4,        // longest kept length
  CW_JUMP = 5,          // a pointer-jumping round changed a parent
  CW_WIDE_KEYS = 6,     // some in-group sort key needs more than 32 bits
  CW_FWD_KEPT = 8,      // forward-strand kept rows (counted; the host does not read it)
  CW_OPEN_X = 10,       // the queued sweeps left the X axis open (RK_ROOTS_FUSED=0)
  CW_OPEN_Y = 11,       // ... the Y axis
  CW_CHAINS = 12,       // parent chains listed for k_nw_assign_rest
  CW_CHAIN_OPEN = 13,   // a chain stayed open after 4128 steps
  CW_GROUPS = 32,       // group count G
  CW_HEAPS = 33,        // depth-limit heap segments left to the caller (one pair)
  CW_PEND_X = 64,                       // the X axis' pending counters (generic: either axis')
  CW_PEND_Y = CW_PEND_X + PEND_WORDS,   // the Y axis' pending counters
  CW_PEND_JUNK = CW_PEND_Y + PEND_WORDS,  // counted into by the queued sweeps before an
                                          // axis' last; never read, never cleared
  CW_GENERIC_WORDS = CW_PEND_Y,                  // Work::ctrl
  CW_CLEARED_WORDS = CW_PEND_JUNK,               // what a record-pipeline call clears first
  CW_RECORD_WORDS = CW_PEND_JUNK + PEND_WORDS,   // NWork::ctrl
};

// Readbacks of these blocks: RB_x the first word, RB_x_N the count; the host
// then finds word W at ctx->host[W - RB_x].
enum : uint32_t {
  RB_ORDER = CW_ERR, RB_ORDER_N = CW_FWD_KEPT + 1 - RB_ORDER,  // after the order histogram
  RB_PREP = CW_ERR, RB_PREP_N = CW_KEPT + 1 - RB_PREP,         // generic: after prep_keys
  // the fused roots: wide-key flag, G and both axes' pending counters
  RB_ROOTS = CW_JUMP, RB_ROOTS_N = CW_PEND_JUNK - RB_ROOTS,
  // a jumping round of the record pipeline: + wide-key flag, open flags, G
  RB_ROUND = CW_JUMP, RB_ROUND_N = CW_GROUPS + 1 - RB_ROUND,
  // a jumping round of the generic pipeline: + wide-key flag
  RB_GROUND = CW_JUMP, RB_GROUND_N = CW_WIDE_KEYS + 1 - RB_GROUND,
  // the call's end: error bits and the open-chain flag; one pair: + the heap count
  RB_END = CW_ERR, RB_END_N = CW_CHAIN_OPEN + 1 - RB_END, RB_END1_N = CW_HEAPS + 1 - RB_END,
};

// ---- the sharded block: Shard::ctrl (rk_shard.hip, rk_shard_nw.h,
// rk_shard_fast.h), cleared at a call's start and before a repeat on another
// driver.  Words [0, 32) in this numbering are also the u32[32] at GA_WORDS of
// the fast path's first message (k_sh_rows writes them there directly).
enum : uint32_t {
  SC_ERR = 0,          // error bits (ERRB_*)
  SC_KEPT = 1,         // generic driver: kept rows (prep_keys)
  SC_MISMATCH = 2,     // halo entries whose states disagree (X, later Y: read back in between)
  SC_JUMP = 3,         // a jumping round changed a parent / a listed chain stayed open
  SC_SWEEP_COUNT = 4,  // the sweep scratch's device count
  SC_WIDE_KEYS = 6,    // some in-group sort key needs more than 32 bits
  SC_EXPECT = 7,       // k_part_scatter's overflow flag when no expect flag is bound
  // two roles in two drivers, which never run on one clearing of the block
  // (a fallback to the generic driver clears it first):
  SC_MAXLEN64 = 10,    // generic driver: longest length, 64 bits ([10..11], k_row_keys)
  SC_CHAINS = 10,      // fast record driver: jump_listed's listed-chain count
  SC_LOWER = 12,       // generic driver: k_lower_bound's result (lead-in suffix)
  SC_NOPACK = 20,      // some kept row does not pack (k_sh_rows)
  SC_MAXLEN = 21,      // longest kept length
  SC_LEAD_IN = 22,     // record drivers: k_lower_bound16's result (lead-in suffix)
  SC_XLINK = 23,       // this rank has a cross-slice parent link
  SC_REC_KEPT = 25,    // kept rows (k_sh_rows)
  SC_ONE = 32,         // world size 1: k_nw_order_hist's words, CW_* numbering from here
  SC_ONE_WORDS = 16,
  SC_PEND = 64,        // the sweeps' pending counters (PEND_WORDS)
  SC_TOTALS = 128,     // a partition plan's totals, MAXP + 1 words (rk_shard.hip)
  // the fast path's words, SC_FAST_CLEARED of them cleared per call; the first
  // GW_HALF ride in every GC / GD / GE message
  SC_FAST = 200,
  SC_F_RETRY = SC_FAST,         // RETRY_* bits
  SC_F_MISM_X = SC_FAST + 1,    // X halo mismatches
  SC_F_MISM_Y = SC_FAST + 2,    // Y halo mismatches
  SC_F_OPEN_X = SC_FAST + 3,    // the queued sweeps left the X axis open
  SC_F_OPEN_Y = SC_FAST + 4,    // ... the Y axis
  SC_F_HEAPS = SC_FAST + 5,     // depth-limit heap segments left to the caller
  SC_FAST_CLEARED = 16,
  SC_WORDS = 256,
  // the careful record driver's first readback, from SC_ERR: up to the kept
  // count, or (world size 1) through the one-route copy's RB_ORDER span
  RB_SH_ROWS_N = SC_REC_KEPT + 1, RB_SH_ROWS_ONE_N = SC_ONE + RB_ORDER_N,
};
// head of the GC / GD / GE messages (k_msg_head), u32[2 * GW_HALF]: the
// block's first GW_HALF words, then the first GW_HALF fast words; gw_head(w):
// the place of one of those words in it
constexpr uint32_t GW_HALF = 8;
constexpr uint32_t gw_head(uint32_t w) { return w < SC_FAST ? w : GW_HALF + w - SC_FAST; }

// ---- the pinned host buffer (rk_ctx::host) ---------------------------------
// A readback may fill all of it.  The upper half is also lent as scratch words
// to build_runs, sort_groups_exact / sort_groups_heap_deferred and
// rk_std_sort_segments, which use them within the call only: nothing there
// has to survive a readback.
constexpr uint32_t HOST_WORDS = 256;
constexpr uint32_t HOST_SCRATCH = 128;                         // first scratch word
constexpr uint32_t HOST_SCRATCH_WORDS = HOST_WORDS - HOST_SCRATCH;
constexpr uint32_t GS_HOST_WORDS = 16;  // what sort_groups_exact asks of host_words

// ---- checks ----------------------------------------------------------------
namespace ctrl_check {
template <uint32_t... W>
constexpr bool distinct() {
  const uint32_t w[] = {W...};
  for (unsigned i = 0; i < sizeof...(W); ++i)
    for (unsigned j = i + 1; j < sizeof...(W); ++j)
      if (w[i] == w[j]) return false;
  return true;
}
// a readback of n words from `first` holds every word listed
template <uint32_t first, uint32_t n, uint32_t... W>
constexpr bool covers() {
  const uint32_t w[] = {W...};
  for (uint32_t x : w)
    if (x < first || x >= first + n) return false;
  return true;
}
// single-device: names distinct; words and counter blocks inside the blocks
static_assert(distinct<CW_ERR, CW_KEPT, CW_SWEEP_COUNT, CW_NOPACK, CW_MAXLEN, CW_JUMP,
                       CW_WIDE_KEYS, CW_FWD_KEPT, CW_OPEN_X, CW_OPEN_Y, CW_CHAINS, CW_CHAIN_OPEN,
                       CW_GROUPS, CW_HEAPS>(), "single-device control words overlap");
static_assert(CW_HEAPS < CW_PEND_X, "a named word inside the pending counters");
static_assert(CW_OPEN_Y == CW_OPEN_X + 1, "the open flags are cleared and passed as a pair");
static_assert(CW_GENERIC_WORDS == 64 + PEND_WORDS && CW_CLEARED_WORDS == 64 + 2 * PEND_WORDS &&
              CW_RECORD_WORDS == 64 + 3 * PEND_WORDS, "block sizes are fixed");
static_assert(CW_PEND_X + PEND_WORDS <= CW_GENERIC_WORDS && CW_WIDE_KEYS < CW_PEND_X,
              "the generic block holds its words");
static_assert(CW_PEND_JUNK + PEND_WORDS <= CW_RECORD_WORDS, "the record block holds its counters");
// the readbacks: today's spans, every word the host reads from each, inside
// the block, inside the pinned buffer
static_assert(RB_ORDER_N == 9 && RB_PREP_N == 2 && RB_ROOTS_N == 187 && RB_ROUND_N == 28 &&
              RB_GROUND_N == 2 && RB_END_N == 14 && RB_END1_N == 34, "readback spans are fixed");
static_assert(covers<RB_ORDER, RB_ORDER_N, CW_ERR, CW_KEPT, CW_NOPACK, CW_MAXLEN>(), "RB_ORDER");
static_assert(covers<RB_PREP, RB_PREP_N, CW_ERR, CW_KEPT>(), "RB_PREP");
static_assert(covers<RB_ROOTS, RB_ROOTS_N, CW_WIDE_KEYS, CW_GROUPS, CW_PEND_X,
                     CW_PEND_Y + PEND_WORDS - 1>(), "RB_ROOTS");
static_assert(covers<RB_ROUND, RB_ROUND_N, CW_JUMP, CW_WIDE_KEYS, CW_OPEN_X, CW_OPEN_Y,
                     CW_GROUPS>(), "RB_ROUND");
static_assert(covers<RB_GROUND, RB_GROUND_N, CW_JUMP, CW_WIDE_KEYS>(), "RB_GROUND");
static_assert(covers<RB_END, RB_END_N, CW_ERR, CW_CHAIN_OPEN>(), "RB_END");
static_assert(covers<RB_END, RB_END1_N, CW_ERR, CW_CHAIN_OPEN, CW_HEAPS>(), "RB_END (one pair)");
static_assert(RB_ORDER + RB_ORDER_N <= CW_RECORD_WORDS &&
                  RB_ROOTS + RB_ROOTS_N <= CW_RECORD_WORDS &&
                  RB_ROUND + RB_ROUND_N <= CW_RECORD_WORDS && RB_END + RB_END1_N <= CW_RECORD_WORDS,
              "a record-pipeline readback leaves its block");
static_assert(RB_PREP + RB_PREP_N <= CW_GENERIC_WORDS &&
                  RB_GROUND + RB_GROUND_N <= CW_GENERIC_WORDS,
              "a generic-pipeline readback leaves its block");
static_assert(RB_ROOTS_N <= HOST_WORDS && PEND_WORDS <= HOST_WORDS,
              "the largest readback fits the pinned buffer");
static_assert(GS_HOST_WORDS <= HOST_SCRATCH_WORDS, "the scratch half holds its users' words");
// sharded: names distinct (SC_MAXLEN64 / SC_CHAINS share a word, see there)
static_assert(distinct<SC_ERR, SC_KEPT, SC_MISMATCH, SC_JUMP, SC_SWEEP_COUNT, SC_WIDE_KEYS,
                       SC_EXPECT, SC_MAXLEN64, SC_MAXLEN64 + 1, SC_LOWER, SC_NOPACK, SC_MAXLEN,
                       SC_LEAD_IN, SC_XLINK, SC_REC_KEPT>(), "sharded control words overlap");
static_assert(SC_REC_KEPT < SC_ONE && SC_REC_KEPT < 32, "the GA message carries words [0, 32)");
static_assert(SC_ONE_WORDS >= RB_ORDER_N && SC_ONE + SC_ONE_WORDS <= SC_PEND,
              "the one-route copy holds the order words and stops before the sweep counters");
static_assert(SC_PEND + PEND_WORDS <= SC_TOTALS, "the sweep counters stop before the totals");
static_assert(GW_HALF <= SC_FAST_CLEARED && SC_FAST + SC_FAST_CLEARED <= SC_WORDS &&
              SC_F_HEAPS < SC_FAST + GW_HALF, "the fast words: in the block, in the message");
static_assert(SC_EXPECT < GW_HALF, "the message head carries the low flag words");
static_assert(RB_SH_ROWS_N == 26 && RB_SH_ROWS_ONE_N == 41 && RB_SH_ROWS_ONE_N <= SC_WORDS,
              "the record driver's first readback is fixed");
static_assert(covers<SC_ERR, RB_SH_ROWS_N, SC_ERR, SC_NOPACK, SC_MAXLEN, SC_REC_KEPT>() &&
              covers<SC_ERR, RB_SH_ROWS_ONE_N, SC_ONE + CW_ERR, SC_ONE + CW_KEPT,
                     SC_ONE + CW_NOPACK, SC_ONE + CW_MAXLEN>(), "RB_SH_ROWS");
// kernels of the single-device pipelines that the sharded drivers run on
// their own block (jump rounds, nw_x_chunks, sort_keys) write these
static_assert(uint32_t(SC_ERR) == uint32_t(CW_ERR) &&
              uint32_t(SC_WIDE_KEYS) == uint32_t(CW_WIDE_KEYS), "shared kernels, one numbering");
}  // namespace ctrl_check

}  // namespace rk
