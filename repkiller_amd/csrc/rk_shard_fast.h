// rk_shard_fast.h -- the record driver with its exchange sizes agreed up
// front (part of rk_shard.hip's translation unit, after rk_shard_nw.h).
//
// The careful record driver (rk_shard_nw.h) sizes every all-to-all by a
// device count read back to the host and all-gathered right before it, and
// reads back the occupancy sweeps' pending counts and every pointer-jumping
// round: ~20 host waits and ~21-24 all-gathers per call at 2-4 ranks.  Over
// RCCL an all-gather is itself a wait, so at 8 ranks (~1.2 ms of device work
// per rank at cfg3) the round trips would decide the time.  This driver makes
// the same exchanges, in the same order, with the same kernels -- it calls the
// careful driver's stage functions (rk_shard_nw.h, rk_shard.hip), binding
// their exchange policy to FastExchange, their resolver to the queued sweeps
// and their chain compression to jump_listed; its own are the messages
// below, the fingerprints, k_sh_counts, the single-shot halo comparisons, the
// retry decisions and plan_to_msg -- but learns
// their sizes from a few messages assembled ON THE DEVICE (histograms, count
// matrices, flags written by the kernels that produce them) and gathered in
// one collective with one wait each:
//   GA  every rank's row count, error / pack bits, longest length, the
//       xStart/10 histogram and the Y-centre bucket histogram of its rows
//       -> the slice bounds AND the Y-range bounds (the same multiset of
//       rows, so the same bounds the careful driver finds after its Y sort);
//   GB  one pass over the source rows counts, per (slice, destination), the
//       Y records (halos included), the X lead-in records and the rows in
//       every Y range's first / last bucket -> the sizes of the row, Y, halo,
//       X-state, X-hit and Y-state exchanges;
//   GC  after both axes: the verification mismatches, whether a queued sweep
//       left an axis open, the wide-key flag, and per slice the parents this
//       Y owner sends, its roots and its cross-slice links -> the parent
//       exchange, the gid offsets and the first request round;
//   GD  after each request round: the next round's request counts, the
//       pointer-jumping flag and the (speculative) gid histogram -> the
//       member exchange (its bounds lie on the histogram's bins);
//   GE  the error bits and the deferred heap segments.
// Five gathers and five waits per call when one request round settles the
// roots (two ranks), one more per further round.  A halo disagreement or an
// axis still open after its queued sweeps (the careful driver's rare
// re-resolution) makes every rank repeat the call on the careful driver.
//
// Receive buffers: a stage whose gathered counts (and so every size it takes)
// equal those of the last call that completed on this path runs without
// agreement points -- no rank can need a larger buffer; otherwise its
// exchanges go through Shard::exchange, whose count gather agrees on any
// growth before data moves (the first call, or a new input).
#pragma once

constexpr int RK_SHARD_RETRY = 1 << 21;  // not a status: repeat on the careful driver

// bits of the fast path's retry word (SC_F_RETRY; the fast words: rk_ctrl.h)
enum : uint32_t { RETRY_EXPECT = 1u, RETRY_PARENT = 2u };

// message layouts (byte offsets into the payload)
constexpr size_t GA_HOST = 0;     // u64 rows of this rank, u64 fingerprints[8]
constexpr size_t GA_WORDS = 128;  // u32[32]: SC_ERR, SC_NOPACK, SC_MAXLEN, SC_REC_KEPT
constexpr size_t GA_XH = 256, GA_YH = GA_XH + NBINS * 4, GA_END = GA_YH + NBINS * 4;
static_assert(GA_END <= GMAX, "GA message");
constexpr size_t GW_END = 2 * GW_HALF * 4;  // GC / GD / GE: the head (k_msg_head; gw_head(SC_*))
static_assert(GW_END == 64, "the message head is fixed");
static_assert(GW_END + (2 * MAXP + MAXP * MAXP + 2) * 4 <= GMAX, "GC message");
static_assert(GW_END + 256 + NBINS * 4 <= GMAX, "GD message");

inline uint64_t hmix(uint64_t h, uint64_t v) {
  uint64_t z = h + 0x9e3779b97f4a7c15ull + v;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
inline uint64_t hbytes(uint64_t h, const void *p, size_t n) {
  const uint8_t *b = (const uint8_t *)p;
  size_t i = 0;
  for (; i + 8 <= n; i += 8) {
    uint64_t v;
    std::memcpy(&v, b + i, 8);
    h = hmix(h, v);
  }
  uint64_t t = 0;
  for (size_t k = 0; i < n; ++i, ++k) t |= (uint64_t)b[i] << (8 * k);
  return hmix(h, t ^ n);
}

// ---- kernels ----------------------------------------------------------------
// the one-route's order-histogram words (k_nw_order_hist's, CW_*) in
// k_sh_rows' layout (SC_*)
__global__ void k_sh_one_words(const uint32_t *c, uint32_t *w) {
  if (threadIdx.x == 0) {
    w[SC_ERR] = c[CW_ERR];
    w[SC_NOPACK] = c[CW_NOPACK];
    w[SC_MAXLEN] = c[CW_MAXLEN];
    w[SC_REC_KEPT] = c[CW_KEPT];
  }
}

// head of the GC / GD / GE messages: the error / flag words and the fast words
__global__ void k_msg_head(const uint32_t *ctrl, uint32_t *w) {
  const uint32_t t = threadIdx.x;
  if (t < GW_HALF) w[t] = ctrl[t];
  else if (t < 2 * GW_HALF) w[t] = ctrl[SC_FAST + t - GW_HALF];
}

// per source row, with the bounds of every slice, Y range and lead-in: the Y
// records each slice sends to each Y owner (YOp12's masks), the lead-in
// records each slice sends to each later slice (GhostOp16's), and the rows in
// every Y range's first / last bucket (YStateOp's selections)
struct ShCountArgs {
  Frags f;
  uint32_t drop, P;
  Bounds sk;
  int64_t ylo[MAXP], yhi[MAXP];
  uint64_t thr[MAXP];
  uint64_t fb[MAXP], lb[MAXP];  // ~0: an empty range
  uint32_t *out;                // [P * P] Y, [P * P] lead-in, [P] first, [P] last
};
__global__ void __launch_bounds__(256) k_sh_counts(ShCountArgs a) {
  __shared__ uint32_t c[2 * MAXP * MAXP + 2 * MAXP];
  const uint32_t P = a.P, W = 2 * P * P + 2 * P;
  for (uint32_t j = threadIdx.x; j < W; j += 256) c[j] = 0;
  __syncthreads();
  uint32_t *ym = c, *hm = c + P * P, *fc = c + 2 * P * P, *lc = fc + P;
  GRID_STRIDE(i, a.f.n) {
    const uint64_t xs = a.f.x[i];
    const uint64_t pk = div10_sh(xs);
    if (pk >= a.drop) continue;  // (the never-iterated last bucket: no record)
    const uint64_t ys = a.f.y[i];
    const uint32_t len = (uint32_t)(a.f.len[i] & 0xFFFFFFu);  // every row packs here
    const uint32_t s = owner_of(a.sk, pk);
    const uint64_t yb = (ys + len / 2) / 100, xb = (xs + len / 2) / 100;
    for (uint32_t q = 0; q < P; ++q) {
      if ((int64_t)yb >= a.ylo[q] && (int64_t)yb < a.yhi[q]) atomicAdd(&ym[s * P + q], 1u);
      if (yb == a.fb[q]) atomicAdd(&fc[q], 1u);
      if (yb == a.lb[q]) atomicAdd(&lc[q], 1u);
    }
    for (uint32_t g = s + 1; g < P; ++g)
      if (xb >= a.thr[g]) atomicAdd(&hm[s * P + g], 1u);
  }
  __syncthreads();
  for (uint32_t j = threadIdx.x; j < W; j += 256)
    if (c[j]) atomicAdd(&a.out[j], c[j]);
}

// k_sh_x_own, counting the own X hits whose winner sits in an earlier slice
// (a cross-slice link per entry: lk[me * P + owner of the winner])
__global__ void k_sh_x_own_fast(const uint32_t *par, const uint4 *halo, uint32_t G, uint32_t m,
                                uint32_t poff, uint32_t *xg, uint8_t *used, Bounds slices,
                                uint32_t me, uint32_t *lk) {
  __shared__ uint32_t c[MAXP];
  const uint32_t P = slices.P;
  if (threadIdx.x < MAXP) c[threadIdx.x] = 0;
  __syncthreads();
  GRID_STRIDE(k, G + m) {
    const uint32_t w = par[k];
    const bool hit = w != k;  // (k_sh_x_own)
    if (k < G) {
      used[k] = hit ? 0 : 1;
      continue;
    }
    uint32_t g = NONE;
    if (hit) {
      if (w < G) {
        g = halo[w].y;
        atomicAdd(&c[owner_of(slices, g)], 1u);
      } else {
        g = poff + (w - G);
      }
    }
    xg[k - G] = g;
  }
  __syncthreads();
  if (threadIdx.x < P && c[threadIdx.x]) atomicAdd(&lk[me * P + threadIdx.x], c[threadIdx.x]);
}

// lanes with `on` add one to cnt[key]: one LDS atomic per distinct key in
// the wavefront (every lane of the wavefront must call it)
__device__ __forceinline__ void wave_count(bool on, uint32_t key, uint32_t *cnt) {
  uint64_t act = __ballot(on);
  while (act) {
    const int lead = __builtin_ctzll(act);
    const uint32_t k0 = (uint32_t)__shfl((int)key, lead);
    const uint64_t b = __ballot(on && key == k0);
    if ((int)(threadIdx.x & 63) == lead) atomicAdd(&cnt[k0], (uint32_t)__popcll(b));
    act &= ~b;
  }
}

// k_sh_y_results, counting per slice (the slice of the record's processing
// index) the parents this Y owner sends (X misses of its own range whose slice
// is another rank's), the roots (Y misses among them) and the cross-slice
// links (Y winner in another slice).  A winner outside the held records (an
// axis left open: the call is repeated) is not followed.
__global__ void __launch_bounds__(256) k_sh_y_results_fast(
    const uint3 *yr, const uint8_t *code, uint32_t c, const uint32_t *par, uint8_t *ystate,
    uint32_t *ywin, uint32_t poff, uint32_t m, uint32_t *xpar, Bounds slices, uint32_t me,
    uint32_t *pc, uint32_t *rc, uint32_t *lk, uint32_t *flag) {
  __shared__ uint32_t cnt[2 * MAXP + MAXP * MAXP];
  const uint32_t P = slices.P, lane = threadIdx.x & 63;
  for (uint32_t j = threadIdx.x; j < 2 * P + P * P; j += blockDim.x) cnt[j] = 0;
  __syncthreads();
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r - lane < c;
       r += gridDim.x * blockDim.x) {
    bool par_on = false, root_on = false, link_on = false;
    uint32_t s = 0, b = 0;
    if (r < c) {
      const uint8_t cr = code[r];
      if (cr & YC_XHIT) {
        ystate[r] = 1;
        ywin[r] = NONE;
      } else {
        uint32_t p = par[r];
        if (p >= c) {
          atomicOr(flag, RETRY_PARENT);
          p = r;
        }
        ystate[r] = p == r ? 1 : 0;
        const uint32_t w = yr[p].y, self = yr[r].y;
        ywin[r] = w;
        if (!(cr & 3)) {  // (a halo record: its owner decides it)
          const uint32_t own = self - poff;
          if (own < m) xpar[own] = w;
          s = owner_of(slices, self);
          par_on = s != me;
          if (p == r) {
            root_on = true;
          } else {
            b = owner_of(slices, w);
            link_on = b != s;
          }
        }
      }
    }
    wave_count(par_on, s, cnt);
    wave_count(root_on, P + s, cnt);
    wave_count(link_on, 2 * P + s * P + b, cnt);
  }
  __syncthreads();
  for (uint32_t j = threadIdx.x; j < 2 * P + P * P; j += blockDim.x) {
    const uint32_t v = cnt[j];
    if (!v) continue;
    if (j < P) atomicAdd(&pc[j], v);
    else if (j < 2 * P) atomicAdd(&rc[j - P], v);
    else atomicAdd(&lk[j - 2 * P], v);
  }
}

// the root count of this slice against the one the Y owners counted
__global__ void k_expect1(const uint32_t *v, uint32_t want, uint32_t *flag, uint32_t bit) {
  if (threadIdx.x == 0 && *v != want) atomicOr(flag, bit);
}
__global__ void k_copy_word(const uint32_t *src, uint32_t *dst) {
  if (threadIdx.x == 0) *dst = *src;
}

// k_final_gid without the error bit: after a request round that may not be
// the last, the labels can still be open (the next gather says)
__global__ void k_final_gid_spec(const uint32_t *lpar, const uint32_t *lab, uint32_t m,
                                 uint32_t *gid) {
  GRID_STRIDE(k, m) {
    const uint32_t g = lab[lpar[k]];
    gid[k] = g == NONE ? 0u : g;
  }
}

// ---- host helpers --------------------------------------------------------------
// an exchange whose per-peer counts every rank knows: straight to the
// all-to-all (known: the stage's sizes match the last completed call, no rank
// grows a buffer), or through Shard::exchange's count gather and agreement
template <class T>
T *xchg(Shard &S, bool known, const void *send, const PartPlan &pp, const uint64_t *rcnt,
        int slot, uint32_t *nrecv) {
  const uint32_t P = S.P;
  if (P == 1) {  // one rank: the send block is the receive block
    *nrecv = (uint32_t)pp.total;
    return const_cast<T *>(reinterpret_cast<const T *>(send));
  }
  if (!known) {
    uint32_t n = 0;
    T *r = S.exchange<T>(send, pp, slot, &n);
    uint64_t want = 0;
    for (uint32_t q = 0; q < P; ++q) want += rcnt[q];
    if (n != want) {
      S.ctx->err = "fast path: exchange size differs from the agreed counts";
      throw RK_E_INTERNAL;
    }
    *nrecv = n;
    return r;
  }
  uint64_t sb[MAXP], rb[MAXP], tot = 0;
  for (uint32_t q = 0; q < P; ++q) {
    sb[q] = pp.cnt[q] * sizeof(T);
    rb[q] = rcnt[q] * sizeof(T);
    tot += rcnt[q];
  }
  T *recv = S.take<T>(slot, tot + 1);
  S.run_a2a(send, sb, recv, rb);
  ++S.n_agree_skipped;
  *nrecv = (uint32_t)tot;
  return recv;
}

// a plan whose per-destination counts come back in a message (the next
// request round): the counts and the scan on the device, the totals into the
// payload (k_totals' cumulative offsets), no readback
template <class Op>
void plan_to_msg(Shard &S, const Op &op, uint32_t n, PartPlan &pp, uint32_t *tot) {
  pp.n = n;
  pp.nblk = n ? (n + PART_TILE - 1) / PART_TILE : 1;
  const size_t len = (size_t)S.P * pp.nblk + 1;
  uint32_t *cnt = S.take<uint32_t>(SL_PCNT, len);
  pp.off = S.take<uint32_t>(SL_POFF, len);
  S.zero(cnt + len - 1, 4);
  kt_begin(S.st, KID_PART);
  k_part_count<<<pp.nblk, 256, 0, S.st>>>(op, n, S.P, pp.nblk, cnt, pp.mcache, pp.mread);
  kt_end(S.st, KID_PART, 0.0);
  S.launched("k_part_count");
  exclusive_scan_u32(cnt, pp.off, len, S.scan_scratch(SL_PSCAN, len), S.st);
  k_totals<<<1, 64, 0, S.st>>>(pp.off, pp.nblk, S.P, tot);
  S.launched("k_totals");
}

// the stages' exchange policy of this driver: the per-peer counts rcnt are
// agreed, `known` is the stage's flag (see xchg)
struct FastExchange {
  Shard &S;
  bool known;
  const uint64_t *rcnt;
  template <class T>
  T *operator()(const T *send, const PartPlan &pp, int slot, uint32_t *nrecv) const {
    return xchg<T>(S, known, send, pp, rcnt, slot, nrecv);
  }
};

// ---- the driver ------------------------------------------------------------------
// Returns RK_OK, an error, RK_SHARD_FALLBACK (a row does not pack: the generic
// driver) or RK_SHARD_RETRY (the careful driver).  *N_out / *row_base_out:
// every rank's rows / this rank's first global row.
int classify_sharded_fast(Shard &S, const Geom &geo, const rk_frags_soa *in, const rk_params &p,
                          bool one_on, rk_shard_result *out, int pre, uint64_t *N_out,
                          uint64_t *row_base_out) {
  rk_ctx *ctx = S.ctx;
  rk_shard_stats &ss = ctx->shard_stats;
  const uint32_t P = S.P, me = S.me;
  hipStream_t st = S.st;
  if (pre) {  // this rank cannot run: its status in the peers' first gather (GA)
    (void)S.status_gather(pre, nullptr, nullptr, 0);
    throw pre;
  }
  S.expect_flag = S.ctrl + SC_F_RETRY;
  S.expect_bit = RETRY_EXPECT;
  ss.fast_path = 1;
  const bool solo = P == 1;
  auto tphase = std::chrono::steady_clock::now();
  // the sweeps queued, as many as the last careful call took; an axis left
  // open sets SC_F_OPEN_X / SC_F_OPEN_Y
  const auto resolve = [&](const Axis &a, const SweepScratch &sc, int axis) {
    S.check(resolve_axis_queued(ctx, a, sc, ctx->sh_blind[axis],
                                S.ctrl + (axis ? SC_F_OPEN_Y : SC_F_OPEN_X)));
  };

  // ---- GA: rows, checks, the slice and Y-range histograms ---------------------
  RecState R = rec_state(S, geo, in, p, one_on, false);
  const uint32_t nl = R.nl, shift = R.shift, nby = R.nby;
  uint8_t *pay = S.msg_begin(P > 1 ? GA_END : GA_XH);
  uint32_t *wa = reinterpret_cast<uint32_t *>(pay + GA_WORDS);
  S.zero(S.ctrl + SC_FAST, SC_FAST_CLEARED * 4);
  source_rows(S, R, wa, P > 1 ? reinterpret_cast<uint32_t *>(pay + GA_XH) : nullptr,
              P > 1 ? reinterpret_cast<uint32_t *>(pay + GA_YH) : nullptr);
  if (R.one && nl) {
    k_sh_one_words<<<1, 64, 0, st>>>(S.ctrl + SC_ONE, wa);
    S.launched("k_sh_one_words");
  }
  {
    uint64_t hostp[9];
    hostp[0] = in->n;
    for (int k = 0; k < 8; ++k) hostp[1 + k] = ctx->sh_fp[k];
    if (S.msg_gather(0, hostp, sizeof hostp)) throw (int)RK_E_PEER;
  }
  uint64_t N = 0, row_base = 0;
  std::vector<uint64_t> nall(P), kept(P), fps((size_t)P * 8);
  uint32_t anyerr = 0, nopack = 0;
  std::vector<uint64_t> gh(NBINS, 0), gy(NBINS, 0);
  std::vector<uint32_t> hx_all(P > 1 ? (size_t)P * NBINS : 0);  // every rank's own row bins
  uint64_t fp = hmix(0x5eedull, P);
  fp = hmix(hmix(hmix(fp, R.H), p.len_x_hdr + 1), p.len_y_hdr + 1);
  for (uint32_t q = 0; q < P; ++q) {
    const uint8_t *mq = S.msg_of(q);
    std::memcpy(&nall[q], mq + GA_HOST, 8);
    std::memcpy(&fps[(size_t)q * 8], mq + GA_HOST + 8, 64);
    const uint32_t *w = reinterpret_cast<const uint32_t *>(mq + GA_WORDS);
    N += nall[q];
    row_base += q < me ? nall[q] : 0;
    anyerr |= w[SC_ERR];
    nopack |= w[SC_NOPACK];
    R.maxlen = w[SC_MAXLEN] > R.maxlen ? w[SC_MAXLEN] : R.maxlen;
    kept[q] = w[SC_REC_KEPT];
    fp = hmix(hmix(hmix(fp, nall[q]), kept[q]), w[SC_MAXLEN]);
    if (P > 1) {
      const uint32_t *hx = reinterpret_cast<const uint32_t *>(mq + GA_XH);
      const uint32_t *hy = reinterpret_cast<const uint32_t *>(mq + GA_YH);
      std::memcpy(&hx_all[(size_t)q * NBINS], hx, NBINS * 4);
      for (uint32_t b = 0; b < NBINS; ++b) gh[b] += hx[b], gy[b] += hy[b];
      fp = hbytes(hbytes(fp, hx, NBINS * 4), hy, NBINS * 4);
    }
  }
  *N_out = N;
  *row_base_out = R.row_base = row_base;
  if (N >= 0xFFFFFFFFull) return RK_E_TOO_MANY;  // every rank sees the same N
  ss.n_in = nl;
  ss.n_total = N;
  S.check(err_status(ctx, anyerr & ~(uint32_t)ERRB_WIDE_LENGTH));
  if (nopack) return RK_SHARD_FALLBACK;
  // the fingerprints every rank holds for each stage (a stage runs without
  // agreement points when every rank holds the same one and it matches)
  const auto fp_known = [&](int k, uint64_t want) {
    for (uint32_t q = 0; q < P; ++q)
      if (fps[(size_t)q * 8 + k] != want || !want) return false;
    return true;
  };
  uint64_t new_fp[8] = {};
  uint64_t kept_all = 0;
  for (uint32_t q = 0; q < P; ++q) kept_all += kept[q];
  R.kept = kept[me];
  R.slice_keys = split_bounds(gh, shift, R.drop, P);
  if (slice_max_rows(gh, R.slice_keys, shift, P, kept_all) >= (1ull << 30))
    return RK_SHARD_FALLBACK;
  std::vector<uint64_t> mall(P, 0);  // every slice: the global histogram's bins between its bounds
  for (uint32_t q = 0; q < P; ++q)
    mall[q] = P == 1 ? kept_all : bins_in(gh.data(), R.slice_keys, q, shift);
  set_slices(S, R, mall);
  const uint32_t m = R.m, poff = R.poff;
  R.yb = split_bounds(gy, R.yshift, nby, P);
  const Bounds &slices = R.slices, &yb = R.yb;
  uint64_t thr[MAXP];
  lead_in_thresholds(thr, R.mall, R.slice_keys, R.H);
  uint64_t fbk[MAXP], lbk[MAXP];  // every Y range's first and last bucket
  for (uint32_t q = 0; q < MAXP; ++q) {
    const bool ne = q < P && yb.b[q] < yb.b[q + 1];
    fbk[q] = ne ? yb.b[q] : ~0ull;
    lbk[q] = ne ? yb.b[q + 1] - 1 : ~0ull;
  }

  // ---- GB: the exchange sizes, counted over the source rows -------------------
  std::vector<uint64_t> Ym((size_t)P * P, 0), Hm((size_t)P * P, 0), Fc(P, 0), Lc(P, 0);
  if (P > 1) {
    pay = S.msg_begin((size_t)(2 * P * P + 2 * P) * 4);
    if (nl) {
      ShCountArgs ca{};
      ca.f = R.f;
      ca.drop = R.drop;
      ca.P = P;
      ca.sk = R.slice_keys;
      y_halo_ranges(yb, P, R.H, ca.ylo, ca.yhi);
      for (uint32_t q = 0; q < MAXP; ++q) {
        ca.thr[q] = thr[q];
        ca.fb[q] = fbk[q];
        ca.lb[q] = lbk[q];
      }
      ca.out = reinterpret_cast<uint32_t *>(pay);
      kt_begin(st, KID_SHARD_AUX);
      k_sh_counts<<<grid_for(nl, 256, 1024), 256, 0, st>>>(ca);
      kt_end(st, KID_SHARD_AUX, 25.0 * nl);
      S.launched("k_sh_counts");
    }
    if (S.msg_gather(0)) throw (int)RK_E_PEER;
    for (uint32_t q = 0; q < P; ++q) {
      const uint32_t *w = reinterpret_cast<const uint32_t *>(S.msg_of(q));
      for (size_t j = 0; j < (size_t)P * P; ++j) Ym[j] += w[j], Hm[j] += w[P * P + j];
      for (uint32_t k = 0; k < P; ++k) Fc[k] += w[2 * P * P + k], Lc[k] += w[2 * P * P + P + k];
    }
  }
  const auto Yat = [&](uint32_t s, uint32_t q) { return Ym[(size_t)s * P + q]; };
  const auto Hat = [&](uint32_t s, uint32_t g) { return Hm[(size_t)s * P + g]; };
  // the Y-state counts owner q -> rank r: YStateOp sends q's first-bucket
  // entries to every rank whose range ends at q's start, its last-bucket ones
  // to every rank whose range starts at q's end (once to a rank in both)
  std::vector<uint64_t> Ys((size_t)P * P, 0);
  for (uint32_t q = 0; q < P; ++q)
    for (uint32_t r = 0; r < P; ++r) {
      if (r == q) continue;
      const bool fm = yb.b[r + 1] == yb.b[q], lm = yb.b[r] == yb.b[q + 1];
      uint64_t c = (fm ? Fc[q] : 0) + (lm ? Lc[q] : 0);
      if (fm && lm && fbk[q] == lbk[q] && fbk[q] != ~0ull) c -= Fc[q];
      Ys[(size_t)q * P + r] = c;
    }
  uint64_t ny64 = P == 1 ? m : 0, G64 = 0;
  for (uint32_t s = 0; P > 1 && s < P; ++s) ny64 += Yat(s, me), G64 += Hat(s, me);
  for (uint32_t r = 0; P > 1 && r < P; ++r) {  // every rank's Y range under the 30-bit bound
    uint64_t c = 0;
    for (uint32_t s = 0; s < P; ++s) c += Yat(s, r);
    if (c >= (1ull << 30)) {
      ctx->err = "a Y range of 2^30 or more records";
      throw RK_E_TOO_MANY;
    }
  }
  fp = hbytes(hbytes(fp, Ym.data(), Ym.size() * 8), Hm.data(), Hm.size() * 8);
  fp = hbytes(hbytes(fp, Fc.data(), Fc.size() * 8), Lc.data(), Lc.size() * 8);
  new_fp[0] = fp;
  const bool knownA = P > 1 && fp_known(0, fp);
  S.alloc_locked = knownA;
  ss.fast_stages |= knownA ? 1u : 0u;
  // the GC message collects the axes' flags and counts from here on
  uint32_t *gc = reinterpret_cast<uint32_t *>(S.msg_begin(GW_END + (size_t)(2 * P + P * P) * 4));
  uint32_t *gc_pc = gc + GW_END / 4, *gc_rc = gc_pc + P, *gc_lk = gc_rc + P;
  ss.ms_ingress = ms_since(tphase);

  // ---- 2: rows -> slice owners as 16-B records ----------------------------------
  tphase = std::chrono::steady_clock::now();
  uint64_t rfrom[MAXP] = {};
  for (uint32_t q = 0; q < P; ++q)
    rfrom[q] = P == 1 ? R.kept : bins_in(&hx_all[(size_t)q * NBINS], R.slice_keys, me, shift);
  uint32_t mrecv = 0;
  const uint4 *rin = rows_to_owners(S, R, P > 1 ? &hx_all[(size_t)me * NBINS] : nullptr,
                                    FastExchange{S, knownA, rfrom}, &mrecv);
  if (mrecv != m) {
    ctx->err = "fast path: slice size differs from the histogram's";
    throw RK_E_INTERNAL;
  }

  // ---- 3: the slice's processing order, its Y records ---------------------------
  slice_order(S, R, rin);

  // ---- 4: Y records -> Y-range owners (+ halos) ----------------------------------
  YOp12 yop = y_op(R, P);
  PartPlan ypp;
  uint64_t ysend[MAXP] = {}, yfrom[MAXP] = {};
  for (uint32_t q = 0; q < P; ++q) ysend[q] = Yat(me, q), yfrom[q] = P == 1 ? m : Yat(q, me);
  y_to_owners(S, R, yop, ypp, ysend, FastExchange{S, knownA, yfrom});
  const uint32_t ny = R.ny;
  if (ny != ny64) {
    ctx->err = "fast path: Y range size differs from the counts";
    throw RK_E_INTERNAL;
  }
  y_buffers(S, R);
  const uint64_t ylo = R.ylo, yhi = R.yhi;
  // (one rank: no halo classes, no verification, no parents to send)
  y_beside_x(S, R, !solo);
  ss.ms_y = ms_since(tphase);

  // ---- 5: X lead-in halo from earlier slices -------------------------------------
  tphase = std::chrono::steady_clock::now();
  GhostOp16 gop{};
  gop.R = R.Ra;
  gop.P = P;
  gop.me = me;
  gop.poff = poff;
  gop.base = 0;
  for (uint32_t g = 0; g < MAXP; ++g) gop.thr[g] = thr[g];
  uint64_t hsend[MAXP] = {}, hfrom[MAXP] = {};
  uint64_t hsend_tot = 0;
  for (uint32_t q = 0; q < P; ++q) {
    hsend[q] = P > 1 ? Hat(me, q) : 0;
    hfrom[q] = P > 1 ? Hat(q, me) : 0;
    hsend_tot += hsend[q];
  }
  PartPlan hpp;
  if (hsend_tot && m) {
    // the suffix starts on the device (no readback): entries before it select
    // nothing
    lead_in_suffix(S, R, thr);
    gop.dbase = S.ctrl + SC_LEAD_IN;
    S.plan_counts(gop, m, hpp, hsend);
  } else {
    S.zero_plan(0, hpp);
  }
  gop.out = S.take<uint4>(SN_SHALO, hpp.total + 1);
  if (hpp.n) S.emit(gop, hpp);
  const FastExchange ex_halo{S, knownA, hfrom};
  uint32_t G = 0;
  const uint4 *hx = ex_halo(gop.out, hpp, SN_HX, &G);
  if (G != G64) {
    ctx->err = "fast path: lead-in size differs from the counts";
    throw RK_E_INTERNAL;
  }
  ss.x_ghosts = G;

  // ---- 6: X axis over [halo ; own], its sweeps queued -----------------------------
  x_buffers(S, R, G);
  uint32_t *xg = R.xg;
  // one rank: entry ids are processing indices, and both axes write their
  // decisions straight into the parent words (as on one device); the X hits
  // become the Y sort's bitmask (k_nw_x_bits, from those parent words)
  solve_x(S, R, hx, G, solo ? xg : nullptr, resolve,
          [&](const uint32_t *par, uint32_t mx) {
            if (solo) {
              nw_x_bits(par, m, R.ybits, st);
              S.launched("k_nw_x_bits");
            } else {
              kt_begin(st, KID_SH_XOWN);
              k_sh_x_own_fast<<<grid_for(mx, 256, 4096), 256, 0, st>>>(
                  par, hx, G, m, poff, xg, R.xused, slices, me, gc_lk);
              kt_end(st, KID_SH_XOWN, 0.0);
              S.launched("k_sh_x_own_fast");
            }
          });
  // the owners' final states of the lead-in (the same selection as the records)
  if (P > 1) {
    GhostOp16 sop = gop;
    sop.out = nullptr;
    sop.xg = xg;
    PartPlan spp;
    if (hpp.n) S.plan_counts(sop, m, spp, hsend);
    else S.zero_plan(0, spp);
    sop.sout = S.take<uint8_t>(SL_SEND, spp.total + 1);
    if (spp.n) S.emit(sop, spp);
    uint32_t G2 = 0;
    const uint8_t *xown = ex_halo(sop.sout, spp, SL_XOWN, &G2);
    if (G) {
      k_cmp_x16<<<grid_for(G, 256, 1024), 256, 0, st>>>(hx, G, relevant_from(R, me), R.xused, xown,
                                                        S.ctrl + SC_F_MISM_X);
      S.launched("k_cmp_x16");
    }
    ss.x_rounds = 1;
  }
  ss.ms_x = ms_since(tphase);

  // ---- 7: X-hit bytes after the Y records, the Y sort, its sweeps ----------------
  tphase = std::chrono::steady_clock::now();
  if (solo) S.hip(hipStreamWaitEvent(st, ctx->join, 0), "join wait");
  else xhits_follow_y(S, R, yop, ypp, FastExchange{S, knownA, yfrom});
  if (ny) {
    nw_y_sort_after_x(R.yB, R.yA, ny, R.yd, R.yhist, R.ystat, R.cy, nby, R.max_y, R.ybits, st,
                      reinterpret_cast<const uint4 *>(R.yr));
    S.launched("Y sort");
  }
  sweep_y(S, R, ny, solo ? xg : R.par_l, resolve);
  if (ny && !solo) {
    kt_begin(st, KID_SH_YRES);
    // (a grid of at most 2048 blocks: each block adds its counts with global
    // atomics on a few shared words, and 65536 blocks serialised them there)
    k_sh_y_results_fast<<<grid_for(ny, 256, 2048), 256, 0, st>>>(
        R.yr, R.ycode, ny, R.par_l, R.ystate, R.ywin, poff, m, xg, slices, me, gc_pc, gc_rc, gc_lk,
        S.ctrl + SC_F_RETRY);
    kt_end(st, KID_SH_YRES, 0.0);
    S.launched("k_sh_y_results_fast");
  }
  // the owners' states of the relevant Y halo entries
  if (P > 1) {
    RelOp relop{R.ycode, ylo ? owner_of_host(yb, ylo - 1) : 0u,
                yhi < nby ? owner_of_host(yb, yhi) : 0u, nullptr};
    uint64_t ysts[MAXP] = {}, ystr[MAXP] = {};
    for (uint32_t q = 0; q < P; ++q) {
      ysts[q] = Ys[(size_t)me * P + q];
      ystr[q] = Ys[(size_t)q * P + me];
    }
    const bool lonely = ylo == 0 && yhi == yb.b[P];
    PartPlan rp;
    if (lonely) S.zero_plan(ny, rp);
    else S.plan_counts(relop, ny, rp, ystr);
    const uint32_t nrel = (uint32_t)rp.total;
    uint32_t *relidx = S.take<uint32_t>(SL_RELIDX, nrel + 1);
    relop.out = relidx;
    if (!lonely) S.emit(relop, rp);
    if (nrel) {
      k_set_used<<<grid_for(nrel, 256), 256, 0, st>>>(relidx, nrel, nullptr, R.ystate, R.yused);
      S.launched("k_set_used");
    }
    YStateOp yso{};
    yso.code = R.ycode;
    yso.ystate = R.ystate;
    for (uint32_t q = 0; q < P; ++q) {
      if (q == me) continue;
      if (yb.b[q + 1] == ylo) yso.first_mask |= 1u << q;
      if (yb.b[q] == yhi) yso.last_mask |= 1u << q;
    }
    const bool none = !yso.first_mask && !yso.last_mask;
    PartPlan sp;
    if (none) S.zero_plan(ny, sp);
    else S.plan_counts(yso, ny, sp, ysts);
    yso.out = S.take<uint8_t>(SL_SEND, sp.total + 1);
    if (!none) S.emit(yso, sp);
    uint32_t n2 = 0;
    const uint8_t *rys = xchg<uint8_t>(S, knownA, yso.out, sp, ystr, SL_RYS, &n2);
    if (n2 != nrel) {
      ctx->err = "fast path: Y halo state count mismatch";
      throw RK_E_INTERNAL;
    }
    if (nrel) {
      k_cmp_y<<<grid_for(nrel, 256, 1024), 256, 0, st>>>(relidx, nrel, R.yused, rys,
                                                         S.ctrl + SC_F_MISM_Y);
      S.launched("k_cmp_y");
    }
    ss.y_rounds = 1;
  }
  ss.ms_y += ms_since(tphase);

  // ---- 8: roots -------------------------------------------------------------------
  tphase = std::chrono::steady_clock::now();
  const RootBufs rb = root_buffers(S, m);
  uint32_t *lpar = rb.lpar, *lrank = rb.lrank, *lab = rb.lab, *cur = rb.cur;
  // local parents (X winners; the X misses' Y winners of this rank's slice
  // are in place, the other ranks' arrive with the parent exchange), chains
  // compressed inside the slice by a jumping pass and a pass over the chains
  // it left open (no readback between them; a chain still open after both is
  // a crafted input: its flag, checked with the next gather, repeats the call
  // the careful way)
  const auto roots = [&](const ParRec *prr, uint32_t npar) {
    local_roots(S, rb, xg, prr, npar, m, poff, [&](Proc jp, uint32_t *isnew) {
      S.zero(S.ctrl + SC_JUMP, 4);
      jump_listed(jp, m, isnew, S.ctrl, S.take<uint32_t>(SL_JLIST, m + 1), S.ctrl + SC_CHAINS,
                  S.ctrl + SC_JUMP, st);
      S.launched("jump_listed");
    });
  };
  if (P == 1) {
    roots(nullptr, 0);
    if (m) {  // the slice's roots: its new groups
      k_copy_word<<<1, 64, 0, st>>>(lrank + m, gc_rc);
      S.launched("k_copy_word");
    }
  }
  k_msg_head<<<1, 64, 0, st>>>(S.ctrl, gc);
  S.launched("k_msg_head");
  if (S.msg_gather(S.sticky)) throw S.sticky ? S.sticky : (int)RK_E_PEER;
  uint32_t anyerr2 = 0, retry = 0, wide = 0;
  std::vector<uint64_t> Pm((size_t)P * P, 0), Rt(P, 0), Lm((size_t)P * P, 0);
  for (uint32_t q = 0; q < P; ++q) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(S.msg_of(q));
    anyerr2 |= w[gw_head(SC_ERR)];
    wide |= w[gw_head(SC_WIDE_KEYS)];
    retry |= w[gw_head(SC_F_RETRY)] | w[gw_head(SC_F_MISM_X)] | w[gw_head(SC_F_MISM_Y)] |
             w[gw_head(SC_F_OPEN_X)] | w[gw_head(SC_F_OPEN_Y)] |
             (P == 1 ? w[gw_head(SC_JUMP)] : 0u);
    const uint32_t *pc = w + GW_END / 4, *rc = pc + P, *lk = rc + P;
    for (uint32_t s = 0; s < P; ++s) {
      Pm[(size_t)q * P + s] = pc[s];
      Rt[s] += rc[s];
    }
    for (size_t j = 0; j < (size_t)P * P; ++j) Lm[j] += lk[j];
    fp = hbytes(fp, w, GW_END + (size_t)(2 * P + P * P) * 4);
  }
  if (retry) return RK_SHARD_RETRY;
  S.check(err_status(ctx, anyerr2 & ~(uint32_t)ERRB_WIDE_LENGTH));
  const bool narrow = wide == 0;  // every in-group sort key fits 32 bits
  uint64_t Gtot = 0, goff = 0;
  for (uint32_t q = 0; q < P; ++q) Gtot += Rt[q], goff += q < me ? Rt[q] : 0;
  bool links = false;
  for (uint64_t v : Lm) links |= v != 0;
  new_fp[1] = fp;
  const bool knownB = knownA && fp_known(1, fp);
  S.alloc_locked = knownB;
  ss.fast_stages |= knownB ? 2u : 0u;

  uint32_t *gid_own = rb.junk;
  const uint2 *erk = nullptr;
  MemOpNw mop = member_op(S, R, gid_own, Gtot, &erk);
  const uint32_t gshift = mop.shift;
  mop.narrow = narrow;
  bool knownC = knownB;
  std::vector<uint32_t> ghist_all;  // every rank's gid histogram (the last GD)
  if (P > 1) {
    // the parent exchange: the sizes every Y owner counted
    ParOp12 pop{R.yr, R.ycode, slices, R.ywin, me, nullptr};
    uint64_t psend[MAXP] = {}, pfrom[MAXP] = {};
    for (uint32_t q = 0; q < P; ++q) {
      psend[q] = Pm[(size_t)me * P + q];
      pfrom[q] = Pm[(size_t)q * P + me];
    }
    PartPlan ppp;
    S.plan_counts(pop, ny, ppp, psend);
    pop.out = S.take<ParRec>(SL_SEND, ppp.total + 1);
    S.emit(pop, ppp);
    uint32_t npar = 0;
    const ParRec *prr = xchg<ParRec>(S, knownB, pop.out, ppp, pfrom, SL_PR, &npar);
    roots(prr, npar);
    if (m) {
      k_expect1<<<1, 64, 0, st>>>(lrank + m, (uint32_t)Rt[me], S.ctrl + SC_F_RETRY,
                                  RETRY_EXPECT);
      S.launched("k_expect1");
    }
    // cross-slice links: request rounds, the first sized by the links the Y
    // owners and the X lead-in counted, each later one by the last GD message
    uint64_t rq_send[MAXP] = {}, rq_recv[MAXP] = {};
    for (uint32_t q = 0; q < P; ++q) {
      rq_send[q] = Lm[(size_t)me * P + q];
      rq_recv[q] = Lm[(size_t)q * P + me];
    }
    if (links && m) {
      kt_begin(st, KID_SHARD_AUX);
      k_init_labels<<<grid_for(m, 256), 256, 0, st>>>(lpar, rb.ext, lrank, (uint32_t)goff, m, lab,
                                                      cur);
      kt_end(st, KID_SHARD_AUX, 0.0);
      S.launched("k_init_labels");
    }
    const ReqOp rq{lpar, lab, cur, slices, nullptr, nullptr};
    PartPlan rpp;
    bool planned = false;  // rpp already planned on the device (a later round)
    for (uint32_t round = 0;; ++round) {
      if (round > 64) {
        ctx->err = "cross-slice root resolution did not converge";
        throw RK_E_INTERNAL;
      }
      if (links) {
        ++ss.root_rounds;
        if (!planned) S.plan_counts(rq, m, rpp, rq_send);
        request_round(S, rb, slices, m, poff, rpp, FastExchange{S, knownC, rq_recv}, rq_recv,
                      [&](int rrc) {
                        if (!knownC) {
                          S.agree(rrc);  // the response buffers were sized by skewed counts
                        } else if (rrc) {
                          S.sticky = rrc;  // (no agreement point here: reported by the next gather)
                          ctx->err = "a local failure before the response exchange";
                        }
                      },
                      false);
      }
      // GD: the next round's request counts, the jumping flag, the gid histogram
      uint32_t *gd = reinterpret_cast<uint32_t *>(S.msg_begin(GW_END + 256 + NBINS * 4));
      uint32_t *gd_tot = gd + GW_END / 4, *gd_hist = gd + (GW_END + 256) / 4;
      if (links) {
        plan_to_msg(S, rq, m, rpp, gd_tot);
        if (m) {
          k_final_gid_spec<<<grid_for(m, 256), 256, 0, st>>>(lpar, lab, m, gid_own);
          S.launched("k_final_gid_spec");
        }
      } else if (m) {
        kt_begin(st, KID_SHARD_AUX);
        k_final_gid_local<<<grid_for(m, 256), 256, 0, st>>>(lpar, lrank, (uint32_t)goff, m,
                                                            gid_own);
        kt_end(st, KID_SHARD_AUX, 12.0 * m);
        S.launched("k_final_gid_local");
      }
      if (m) {
        k_hist<<<grid_for(m, 256, 512), 256, 0, st>>>(mop, m, gd_hist);
        S.launched("k_hist");
      }
      k_msg_head<<<1, 64, 0, st>>>(S.ctrl, gd);
      S.launched("k_msg_head");
      if (S.msg_gather(S.sticky)) throw S.sticky ? S.sticky : (int)RK_E_PEER;
      uint32_t anyerr3 = 0, jflag = 0, rflag = 0;
      bool more = false;
      std::vector<uint64_t> C((size_t)P * P, 0);
      for (uint32_t q = 0; q < P; ++q) {
        const uint32_t *w = reinterpret_cast<const uint32_t *>(S.msg_of(q));
        anyerr3 |= w[gw_head(SC_ERR)];
        jflag |= w[gw_head(SC_JUMP)];
        rflag |= w[gw_head(SC_F_RETRY)];
        if (links) {
          const uint32_t *t = w + GW_END / 4;
          for (uint32_t d = 0; d < P; ++d) {
            C[(size_t)q * P + d] = t[d + 1] - t[d];
            more |= C[(size_t)q * P + d] != 0;
          }
        }
        fp = hbytes(fp, w, GW_END + 256);
      }
      if (jflag || rflag) return RK_SHARD_RETRY;  // a chain longer than two jumping rounds
      S.check(err_status(ctx, anyerr3 & ~(uint32_t)ERRB_WIDE_LENGTH));
      if (!more) {  // every label is final: the histogram stands
        ghist_all.resize((size_t)P * NBINS);
        for (uint32_t q = 0; q < P; ++q) {
          std::memcpy(&ghist_all[(size_t)q * NBINS], S.msg_of(q) + GW_END + 256, NBINS * 4);
          fp = hbytes(fp, &ghist_all[(size_t)q * NBINS], NBINS * 4);
        }
      }
      if (round + 2 < 8) {
        new_fp[2 + round] = fp;
        knownC = knownC && fp_known(2 + round, fp);
      } else {
        knownC = false;
      }
      S.alloc_locked = knownC;
      if (!more) break;
      for (uint32_t q = 0; q < P; ++q) {
        rq_send[q] = C[(size_t)me * P + q];
        rq_recv[q] = C[(size_t)q * P + me];
      }
      uint64_t tot = 0;
      for (uint32_t q = 0; q < MAXP; ++q) {
        rpp.cnt[q] = q < P ? rq_send[q] : 0;
        tot += rpp.cnt[q];
      }
      rpp.total = tot;
      rpp.cap = (uint32_t)tot;
      planned = true;
    }
  } else {
    // one rank: gid = the root's rank (every chain ends in the slice)
    if (m) {
      kt_begin(st, KID_SHARD_AUX);
      k_final_gid_local<<<grid_for(m, 256), 256, 0, st>>>(lpar, lrank, 0u, m, gid_own);
      kt_end(st, KID_SHARD_AUX, 12.0 * m);
      S.launched("k_final_gid_local");
    }
  }
  S.alloc_locked = knownC;
  ss.fast_stages |= knownC ? 4u : 0u;
  ss.ms_roots = ms_since(tphase);

  // ---- 9: members -> gid-range owners; exact in-group order; emit -----------------
  tphase = std::chrono::steady_clock::now();
  Bounds gb{};
  std::vector<uint64_t> mr_all(P, 0);
  uint64_t msend[MAXP] = {}, mfrom[MAXP] = {};
  if (P > 1) {
    std::vector<uint64_t> gsum(NBINS, 0);
    for (uint32_t q = 0; q < P; ++q)
      for (uint32_t b = 0; b < NBINS; ++b) gsum[b] += ghist_all[(size_t)q * NBINS + b];
    gb = split_bounds(gsum, gshift, Gtot, P);
    for (uint32_t q = 0; q < P; ++q) {
      msend[q] = bins_in(&ghist_all[(size_t)me * NBINS], gb, q, gshift);
      mfrom[q] = bins_in(&ghist_all[(size_t)q * NBINS], gb, me, gshift);
      for (uint32_t r = 0; r < P; ++r) mr_all[r] += bins_in(&ghist_all[(size_t)q * NBINS], gb, r, gshift);
    }
  } else {
    gb.P = 1;
    gb.b[0] = 0;
    for (uint32_t q = 1; q <= MAXP; ++q) gb.b[q] = Gtot;
    mr_all[0] = m;
  }
  for (uint32_t r = 0; r < P; ++r)
    if (mr_all[r] >= (1ull << 30)) {
      ctx->err = "a gid range of 2^30 or more members";
      throw RK_E_TOO_MANY;
    }
  mop.B = gb;
  // one rank, no halo: the X chunk's member arrays are the rows, read in place
  uint32_t mr = 0;
  const void *mem = nullptr;
  if (P == 1) {
    mr = m;
  } else {
    PartPlan mpp;
    S.plan_counts(mop, m, mpp, msend);
    mop.out = S.take<uint8_t>(SN_SMEM, (mpp.total + 1) * (narrow ? 12 : 16));
    S.emit(mop, mpp);
    const FastExchange ex{S, knownC, mfrom};
    mem = narrow ? (const void *)ex((const uint3 *)mop.out, mpp, SL_MEM, &mr)
                 : (const void *)ex((const uint4 *)mop.out, mpp, SL_MEM, &mr);
  }
  // (the depth-limit heap segments -- crafted inputs only -- are counted into
  // SC_F_HEAPS and sorted after GE)
  member_order(S, R, mem, mr, gb, narrow, erk, gid_own, S.ctrl + SC_F_HEAPS);
  S.alloc_locked = false;

  // ---- GE: the error bits and the heap segments ---------------------------------
  uint32_t *ge = reinterpret_cast<uint32_t *>(S.msg_begin(GW_END));
  k_msg_head<<<1, 64, 0, st>>>(S.ctrl, ge);
  S.launched("k_msg_head");
  if (S.msg_gather(S.sticky)) throw S.sticky ? S.sticky : (int)RK_E_PEER;
  uint32_t anyerr4 = 0, heap_me = 0, retry4 = 0;
  bool heap_any = false;
  for (uint32_t q = 0; q < P; ++q) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(S.msg_of(q));
    anyerr4 |= w[gw_head(SC_ERR)];
    retry4 |= w[gw_head(SC_F_RETRY)];  // a member plan whose device counts disagreed
    heap_any |= w[gw_head(SC_F_HEAPS)] != 0;
    if (q == me) heap_me = w[gw_head(SC_F_HEAPS)];
  }
  if (retry4) return RK_SHARD_RETRY;
  S.check(err_status(ctx, anyerr4 & ~(uint32_t)ERRB_WIDE_LENGTH));
  int hrc = RK_OK;
  if (heap_me && mr) {  // sorted now, then the result again
    hrc = sort_groups_heap_deferred(R.Gl, mr, R.reckey, R.tag, R.otag, R.gsort, heap_me,
                                    ctx->host + HOST_SCRATCH, st);
    if (!hrc) {
      emit_members(S, R);
      if (hipGetLastError() != hipSuccess) hrc = RK_E_HIP;
    } else {
      ctx->err = "depth-limit heap segments: buffer allocation failed";
    }
  }
  if (heap_any) {  // every rank agrees on the heap segments' outcome
    if (!hrc && hipStreamSynchronize(st) != hipSuccess) hrc = RK_E_HIP;
    S.agree(hrc);
    S.agree_errors();
  }
  ss.ms_members = ms_since(tphase);
  set_result(out, R.oord, R.ogid, R.orep, mr, mr_all, me, Gtot);
  for (int k = 0; k < 8; ++k) ctx->sh_fp[k] = new_fp[k];
  return RK_OK;
}
