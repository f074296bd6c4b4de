// rk_shard_nw.h -- rk_classify_sharded on the record pipeline's internals.
// Part of rk_shard.hip's translation unit (included inside namespace rk {
// namespace { ... } } after the driver infrastructure: Shard, the partition
// plans, Bounds, the Y-halo codes and the root kernels).
//
// The same stages as the generic sharded driver (rk_shard.hip's header
// comment), with the single-device record pipeline (rk_narrow.hip) inside
// each stage instead of 32-B rows, pair sorts and gathers:
//   ingress   rows leave their rank as 16-B processing-order records {xStart/10,
//             global file row, yStart lo, length | strand | yStart hi |
//             xStart % 10}; the slice owner sorts them with the one-sweep
//             passes (the last pass also writes the 12-B Y records with GLOBAL
//             processing indices);
//   X axis    the lead-in halo arrives as the same 16-B records (the row word
//             replaced by the global processing index) and sits AHEAD of the
//             own records: the X-chunk kernel builds the axis straight from
//             [halo ; own], no sort;
//   Y axis    12-B Y records go to their Y-range owners and are sorted there
//             (the first pass numbers them by arrival: arrival order = global
//             processing order); the X-hit bits follow in the same order, as
//             one byte per record, and become the tail pass' state bitmask;
//   members   12-B {gid, global row, sort key} records (16 B when a sort key
//             needs more than 32 bits) go to gid-range owners and are sorted
//             by local gid with the one-sweep passes into the group sort.
// Every row has to pack into a record (length < 2^24, yStart < 2^35, as in
// the single-device record pipeline); otherwise every rank agrees to run the
// generic driver.  At world size 1 an exchange hands the send block over
// without a copy.
//
// Layout: the kernels and partition ops; the stages of both record drivers
// (source_rows, rows_to_owners, slice_order, y_to_owners / y_buffers /
// y_beside_x, lead_in_suffix, solve_x, xhits_follow_y, sweep_y, member_order;
// local_roots, request_round and the small host helpers sit in rk_shard.hip,
// where the generic driver uses them too); then the careful driver,
// classify_sharded_nw, which reads as the sequence of the stages plus what is
// its own: the readbacks and gathers that size every exchange, and the halo
// verification loops with their re-resolutions.
#pragma once

constexpr int RK_SHARD_FALLBACK = 1 << 20;  // not a status: run the generic driver

// largest bucket index get_associated_group touches for centre c
// (SequenceOcupationList.cpp:47-89; the same bound as rk_narrow.hip's)
__device__ __forceinline__ uint64_t probe_max_bucket_sh(uint64_t c, uint64_t max_index) {
  if (c < (1ull << 32) - 2 && max_index != 0 && max_index < (1ull << 32)) {
    // the same in 32 bits (no wrap of c + 2 or max_index - 1 here)
    const uint32_t c32 = (uint32_t)c, m32 = (uint32_t)max_index;
    uint32_t b = c32 / 100u;
    if (c32 < m32 && (c32 + 1) / 100u > b) b = (c32 + 1) / 100u;
    if (c32 < m32 - 1 && (c32 + 2) / 100u > b) b = (c32 + 2) / 100u;
    return b;
  }
  uint64_t b = c / 100;
  if (c < max_index && (c + 1) / 100 > b) b = (c + 1) / 100;
  if (c < max_index - 1 && (c + 2) / 100 > b) b = (c + 2) / 100;
  return b;
}

// 16-B record fields (rk_narrow.hip's layout)
__device__ __forceinline__ uint64_t nwr_x(const uint4 &r) { return (uint64_t)r.x * 10 + (r.w >> 28); }
__device__ __forceinline__ uint32_t nwr_len(const uint4 &r) { return r.w & 0xFFFFFFu; }
__device__ __forceinline__ uint64_t nwr_xbucket(const uint4 &r) {
  return (nwr_x(r) + nwr_len(r) / 2) / 100;
}
// 12-B Y record: {strand * nby + bucket, id, length | centre % 100 << 24}
__device__ __forceinline__ uint32_t nwy_bucket(const uint3 &r, uint32_t nby) {
  return r.x >= nby ? r.x - nby : r.x;
}

// ---- source side: processing keys, the checks, the slice histogram --------
// ctrl: SC_ERR, SC_NOPACK, SC_MAXLEN, SC_REC_KEPT (the sharded block, or the
// fast path's GA message words)
struct ShRowsArgs {
  Frags f;
  uint64_t vsize, max_x, max_y;
  uint32_t shift;
  uint32_t *hist, *ctrl;  // hist null: one rank owns everything, no bounds to find
  uint32_t *yhist = nullptr;  // (fast path) the Y-centre bucket histogram, bins >> yshift
  uint32_t yshift = 0;
};
__device__ __forceinline__ uint64_t div10_sh(uint64_t v) {  // 32-bit when it fits
  return v < (1ull << 32) ? (uint64_t)((uint32_t)v / 10u) : v / 10;
}
__global__ void __launch_bounds__(256) k_sh_rows(ShRowsArgs a) {
  __shared__ uint32_t h[NBINS], hy[NBINS];
  __shared__ uint32_t red[3];
  for (uint32_t b = threadIdx.x; b < NBINS; b += 256) h[b] = hy[b] = 0;
  if (threadIdx.x < 3) red[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t drop = a.vsize - 1;
  uint32_t maxlen = 0, kept = 0;
  bool ub = false, ubc = false, wide = false;
  GRID_STRIDE(i, a.f.n) {
    const uint64_t xs = a.f.x[i], ys = a.f.y[i], L0 = a.f.len[i];
    const uint64_t pk = div10_sh(xs);
    ub |= pk >= a.vsize;
    if (pk >= drop) continue;  // the never-iterated last bucket (or out of bounds)
    ++kept;
    wide |= L0 >= (1ull << 24) || ys >= (1ull << 35);
    const uint32_t len = (uint32_t)(L0 & 0xFFFFFFu);  // exact whenever the row packs
    maxlen = len > maxlen ? len : maxlen;
    const uint64_t hl = len / 2;
    ubc |= probe_max_bucket_sh(xs + hl, a.max_x) > a.max_x ||
           probe_max_bucket_sh(ys + hl, a.max_y) > a.max_y;
    if (a.hist) atomicAdd(&h[(uint32_t)pk >> a.shift], 1u);
    if (a.yhist) {  // the Y record's bucket (rk_narrow.hip DstProc): centre yStart + len / 2
      const uint64_t yb = ((ys + hl) / 100) >> a.yshift;
      if (yb < NBINS) atomicAdd(&hy[yb], 1u);
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t o = __shfl_xor(maxlen, off);
    maxlen = o > maxlen ? o : maxlen;
    kept += __shfl_xor(kept, off);
  }
  const uint64_t bub = __ballot(ub), bubc = __ballot(ubc), bwide = __ballot(wide);
  if ((threadIdx.x & 63) == 0) {
    atomicMax(&red[0], maxlen);
    atomicOr(&red[1], (bub ? 1u : 0u) | (bubc ? 2u : 0u) | (bwide ? 4u : 0u));
    atomicAdd(&red[2], kept);
  }
  __syncthreads();
  if (a.hist)
    for (uint32_t b = threadIdx.x; b < NBINS; b += 256)
      if (h[b]) atomicAdd(&a.hist[b], h[b]);
  if (a.yhist)
    for (uint32_t b = threadIdx.x; b < NBINS; b += 256)
      if (hy[b]) atomicAdd(&a.yhist[b], hy[b]);
  if (threadIdx.x == 0) {
    if (red[2]) atomicAdd(&a.ctrl[SC_REC_KEPT], red[2]);
    if (red[0]) atomicMax(&a.ctrl[SC_MAXLEN], red[0]);
    if (red[1] & 1u) atomicOr(&a.ctrl[SC_ERR], ERRB_UB_BUCKET);
    if (red[1] & 2u) atomicOr(&a.ctrl[SC_ERR], ERRB_UB_CENTER);
    if (red[1] & 4u) atomicOr(&a.ctrl[SC_NOPACK], 1u);
  }
}

// ---- partition ops ----------------------------------------------------------
struct RowOp16 {  // kept rows -> slice owners, as processing-order records
  Frags f;
  Bounds B;
  uint32_t drop, row_base;
  uint4 *out;
  __device__ uint32_t key(uint32_t i) const {
    const uint64_t pk = div10_sh(f.x[i]);
    return pk < drop ? (uint32_t)pk : drop;
  }
  __device__ uint32_t mask(uint32_t i) const {
    const uint32_t k = key(i);
    return k < drop ? 1u << owner_of(B, k) : 0u;
  }
  __device__ void emit(uint32_t i, uint32_t, uint32_t pos) const {
    const uint64_t xs = f.x[i], ys = f.y[i], L = f.len[i];
    const uint32_t s = f.strand[i] != 'f' ? 1u : 0u;
    const uint64_t pk = div10_sh(xs);
    out[pos] = make_uint4((uint32_t)pk, row_base + i, (uint32_t)ys,
                          (uint32_t)(L & 0xFFFFFFu) | s << 24 | (uint32_t)((ys >> 32) & 7u) << 25 |
                              (uint32_t)(xs - pk * 10) << 28);
  }
};

// own records (processing order, suffix from `base`) -> later slices whose
// lead-in they fall in; the row word carries the global processing index
struct GhostOp16 {
  const uint4 *R;
  uint64_t thr[MAXP];  // lead-in start bucket of every slice (~0: none)
  uint32_t P, me, poff, base;
  uint4 *out;          // records, or
  uint8_t *sout;       // the entries' X states (1 = ACTIVE), same order
  const uint32_t *xg;
  // (fast path) the suffix start on the device: the op runs over all m
  // entries, those before *dbase select nothing (base is then 0)
  const uint32_t *dbase = nullptr;
  __device__ uint32_t mask(uint32_t i) const {
    if (dbase && i < *dbase) return 0u;
    const uint64_t bk = nwr_xbucket(R[base + i]);
    uint32_t m = 0;
    for (uint32_t g = me + 1; g < P; ++g)
      if (bk >= thr[g]) m |= 1u << g;
    return m;
  }
  __device__ void emit(uint32_t i, uint32_t, uint32_t pos) const {
    const uint32_t k = base + i;
    if (sout) {
      sout[pos] = xg[k] == NONE ? 1 : 0;
      return;
    }
    uint4 r = R[k];
    r.y = poff + k;
    out[pos] = r;
  }
};

struct SelXOp16 {  // relevant halo entries the owner calls ACTIVE (fixed-halo X problem)
  const uint4 *gh;
  const uint8_t *owner_state;
  uint64_t rel;
  uint4 *out;
  __device__ uint32_t mask(uint32_t j) const {
    return nwr_xbucket(gh[j]) >= rel && owner_state[j] ? 1u : 0u;
  }
  __device__ void emit(uint32_t j, uint32_t, uint32_t pos) const { out[pos] = gh[j]; }
};

struct YOp12 {  // own Y records -> Y-range owners (+ their halos), processing order
  const uint3 *yrec;
  uint32_t nby, P, shift;
  int64_t lo[MAXP], hi[MAXP];  // halo-extended ranges
  const uint32_t *xg;          // with xout: the X results, sent after X in the same order
  uint3 *out;
  uint8_t *xout;
  __device__ uint32_t bin(uint32_t k) const { return nwy_bucket(yrec[k], nby) >> shift; }
  __device__ uint32_t mask(uint32_t k) const {
    const int64_t b = nwy_bucket(yrec[k], nby);
    uint32_t m = 0;
    for (uint32_t q = 0; q < P; ++q)
      if (b >= lo[q] && b < hi[q]) m |= 1u << q;
    return m;
  }
  __device__ void emit(uint32_t k, uint32_t, uint32_t pos) const {
    if (xout) xout[pos] = xg[k] != NONE ? 1 : 0;
    else out[pos] = yrec[k];
  }
};

struct ParOp12 {  // Y decisions of own X misses -> slice owners (other ranks)
  const uint3 *yr;
  const uint8_t *code;
  Bounds slices;
  const uint32_t *ywin;
  uint32_t me;
  ParRec *out;
  __device__ uint32_t mask(uint32_t r) const {
    const uint8_t c = code[r];
    if ((c & 3) || (c & YC_XHIT)) return 0u;
    const uint32_t q = owner_of(slices, yr[r].y);
    return q == me ? 0u : 1u << q;  // this rank's own slice: written in place
  }
  __device__ void emit(uint32_t r, uint32_t, uint32_t pos) const {
    out[pos] = ParRec{yr[r].y, ywin[r]};
  }
};

struct MemOpNw {  // {gid, global row, sort key} -> gid-range owners
  const uint32_t *gid;
  const uint2 *erk;     // {global row, sort key low 32} of own row k
  const uint32_t *ehi;  // sort key high 32
  Bounds B;
  uint32_t shift;
  bool narrow;
  void *out;
  __device__ uint32_t bin(uint32_t k) const { return gid[k] >> shift; }
  __device__ uint32_t mask(uint32_t k) const { return 1u << owner_of(B, gid[k]); }
  __device__ void emit(uint32_t k, uint32_t, uint32_t pos) const {
    const uint2 e = erk[k];
    if (narrow) reinterpret_cast<uint3 *>(out)[pos] = make_uint3(gid[k], e.x, e.y);
    else reinterpret_cast<uint4 *>(out)[pos] = make_uint4(gid[k], e.x, e.y, ehi[k]);
  }
};

// ---- small kernels ------------------------------------------------------------
// first k with R[k].x >= v (keys ascending)
__global__ void k_lower_bound16(const uint4 *R, uint32_t m, uint64_t v, uint32_t *out) {
  uint32_t lo = 0, hi = m;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (R[mid].x < v) lo = mid + 1;
    else hi = mid;
  }
  *out = lo;
}

// own X results -> global winner ids (NONE: X miss); the halo entries' local
// decisions (1 = in the X list).  The X axis over [halo ; own] runs with
// Axis::xres == nullptr, so once it is closed every entry of the local CSR,
// halo entries included, has par[k] = its winner (a hit) or k (in the list):
// hit = par[k] != k, as in k_nw_x_bits.  (An axis the fast path's queued
// sweeps left open makes the call repeat; a stale word then gives an arbitrary
// xg, which is only compared with NONE until k_local_par bounds it.)
__global__ void k_sh_x_own(const uint32_t *par, const uint4 *halo, uint32_t G, uint32_t m,
                           uint32_t poff, uint32_t *xg, uint8_t *used) {
  GRID_STRIDE(k, G + m) {
    const uint32_t w = par[k];
    const bool hit = w != k;
    if (k < G) {
      used[k] = hit ? 0 : 1;
      continue;
    }
    xg[k - G] = !hit ? NONE : w < G ? halo[w].y : poff + (w - G);
  }
}

__global__ void k_cmp_x16(const uint4 *gh, uint32_t G, uint64_t rel, const uint8_t *used,
                          const uint8_t *owner, uint32_t *mism) {
  for (uint32_t base = blockIdx.x * blockDim.x; base < G; base += gridDim.x * blockDim.x) {
    const uint32_t j = base + threadIdx.x;
    count_flag(j < G && nwr_xbucket(gh[j]) >= rel && used[j] != owner[j], mism);
  }
}

__global__ void k_sh_ycode(const uint3 *yr, uint32_t n, uint32_t nby, uint64_t lo, uint64_t hi,
                           uint8_t *code) {
  GRID_STRIDE(r, n) code[r] = y_code(nwy_bucket(yr[r], nby), lo, hi);
}

// the X-hit bytes (arrival order) -> code bits and the Y states' bitmask
__global__ void k_sh_xhit_bits(const uint8_t *xh, uint32_t n, uint8_t *code, uint32_t *bits) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r - lane < n;
       r += gridDim.x * blockDim.x) {
    const bool hit = r < n && xh[r] != 0;
    if (hit) code[r] |= YC_XHIT;
    const uint64_t b = __ballot(hit);
    if (lane == 0) bits[r >> 5] = (uint32_t)b;
    if (lane == 32 && r < n) bits[r >> 5] = (uint32_t)(b >> 32);
  }
}

// a fixed-halo Y problem's records (the selection ymap, in arrival order) and
// their X-hit bitmask
__global__ void k_sh_ysel(const uint3 *yr, const uint8_t *code, const uint32_t *ymap, uint32_t c,
                          uint3 *ysel, uint32_t *bits) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k - lane < c;
       k += gridDim.x * blockDim.x) {
    bool hit = false;
    if (k < c) {
      const uint32_t r = ymap[k];
      ysel[k] = yr[r];
      hit = (code[r] & YC_XHIT) != 0;
    }
    const uint64_t b = __ballot(hit);
    if (lane == 0) bits[k >> 5] = (uint32_t)b;
    if (lane == 32 && k < c) bits[k >> 5] = (uint32_t)(b >> 32);
  }
}

// (the Y winner of an X miss of this rank's own slice -- processing index in
// [poff, poff + m) -- goes straight into its parent word xpar)
__global__ void k_sh_y_results(const uint3 *yr, const uint8_t *code, const uint32_t *ymap,
                               uint32_t c, const uint32_t *par, uint8_t *ystate, uint32_t *ywin,
                               uint32_t poff, uint32_t m, uint32_t *xpar) {
  GRID_STRIDE(k, c) {
    const uint32_t r = ymap ? ymap[k] : k;
    const uint8_t cr = code[r];
    if (cr & YC_XHIT) {
      ystate[r] = 1;
      ywin[r] = NONE;
    } else {
      const uint32_t p = par[k];
      ystate[r] = p == k ? 1 : 0;
      const uint32_t w = yr[ymap ? ymap[p] : p].y;
      ywin[r] = w;
      if (!(cr & 3)) {
        const uint32_t own = yr[r].y - poff;
        if (own < m) xpar[own] = w;
      }
    }
  }
}

// ---- the stages of both record drivers ------------------------------------------
// classify_sharded_nw (below) and classify_sharded_fast (rk_shard_fast.h) are
// sequences of these; RecState (rk_shard.hip) carries what one stage leaves
// for the next.  A stage that exchanges takes the driver's exchange policy
// `ex(send, plan, receive slot, &count)`: CarefulExchange here, FastExchange
// there.
enum SlotNw : int {
  SN_HIST = SL_COUNT, SN_SROWS, SN_RIN, SN_RA, SN_RB, SN_YOWN, SN_STAT, SN_YSTAT, SN_SHALO, SN_HX,
  SN_HSEL, SN_SY, SN_YR, SN_YA, SN_YB, SN_XCNT, SN_XOFF, SN_XKEY, SN_XENT, SN_XPK, SN_XNBD,
  SN_XSTATE, SN_EREC, SN_PAR, SN_XGUSED, SN_YKEY, SN_YENT, SN_YPK, SN_YNBD, SN_YST,
  SN_XBITS, SN_PARL, SN_SMEM, SN_T0, SN_T1, SN_SGID, SN_MROW, SN_KEY, SN_TAG, SN_GOFF, SN_YSEL,
  SN_SXH, SN_CHIST, SN_COFF, SN_XCNT0, SN_COUNT
};
static_assert(SN_COUNT <= kPoolSlots, "rk_shard.hip kPoolSlots");

// Every record exchange has its own send slot, so a block that is handed over
// without a copy at world size 1 is never overwritten by a later exchange.
template <class T>
T *exchange_nw(Shard &S, const T *send, const PartPlan &pp, int recv_slot, uint32_t *nrecv,
               uint64_t *from = nullptr) {
  if (S.P == 1) {
    S.agree(RK_OK);  // the same collective sequence as with peers
    *nrecv = (uint32_t)pp.total;
    S.last_recv[0] = pp.total;
    if (from) from[0] = pp.total;
    return const_cast<T *>(send);
  }
  return S.exchange<T>(send, pp, recv_slot, nrecv, from);
}
struct CarefulExchange {  // sizes by a count gather; an agreement point at every world size
  Shard &S;
  template <class T>
  T *operator()(const T *send, const PartPlan &pp, int slot, uint32_t *nrecv) const {
    return exchange_nw<T>(S, send, pp, slot, nrecv);
  }
};

// A fresh state: the inputs, the digit plans, the route at one rank, and the
// order / Y / member digit histograms' buffer.
RecState rec_state(Shard &S, const Geom &geo, const rk_frags_soa *in, const rk_params &p,
                   bool one_on, bool y_early) {
  RecState R{};
  static_cast<Geom &>(R) = geo;
  R.p = p;
  R.in = in;
  R.nl = (uint32_t)in->n;
  R.f = Frags{in->x_start, in->y_start, in->length, in->strand, R.nl};
  R.one = one_on && S.P == 1;
  R.y_early = y_early;
  R.ad = nw_plan(bit_length(R.vsize - 1));
  R.yd = nw_plan(bit_length(2ull * R.nby - 1), 9);
  R.op1 = R.one ? nw_order_split_range(R.nl, 0, R.drop) : NwOrderPlan{};
  R.ahist = S.take<uint32_t>(SN_HIST, 3 * 4096);
  R.yhist = R.ahist + 4096, R.ehist = R.ahist + 2 * 4096;
  return R;
}

// the largest slice's row count: at one rank the kept rows, else the global
// histogram's bins between each pair of slice bounds
static uint64_t slice_max_rows(const std::vector<uint64_t> &gh, const Bounds &sk, uint32_t shift,
                               uint32_t P, uint64_t kept) {
  if (P == 1) return kept;
  uint64_t most = 0;
  for (uint32_t q = 0; q < P; ++q) {
    const uint64_t c = bins_in(gh.data(), sk, q, shift);
    most = c > most ? c : most;
  }
  return most;
}

// Source rows: keys, checks and histograms.  World size 1 (R.one, rows
// numbered from 0): the rows are read once, as on one device --
// k_nw_order_hist takes the checks, the kept count and the order and Y digit
// histograms (into ahist / yhist) in the place of k_sh_rows, its words (CW_*)
// from SC_ONE on.  Else
// k_sh_rows: its words into `words` (ShRowsArgs' layout), the xStart/10 and
// Y-centre bucket histograms into xhist / yhist (null: not needed).
void source_rows(Shard &S, const RecState &R, uint32_t *words, uint32_t *xhist, uint32_t *yhist) {
  if (R.one) {
    S.zero(R.ahist, 3 * 4096 * 4);
    S.zero(S.ctrl + SC_ONE, SC_ONE_WORDS * 4);
    if (R.nl)
      nw_order_hist(*R.in, R.vsize, R.max_x, R.max_y, R.nby, R.op1.nseg ? R.op1.coarse : R.ad,
                    R.yd, R.ahist, R.yhist, S.ctrl + SC_ONE, S.st);
  } else if (R.nl) {
    ShRowsArgs ra{R.f, R.vsize, R.max_x, R.max_y, R.shift, xhist, words};
    if (yhist) ra.yhist = yhist, ra.yshift = R.yshift;
    // more blocks when there is no slice histogram to flush (one rank)
    kt_begin(S.st, KID_SH_ROWKEYS);
    k_sh_rows<<<grid_for(R.nl, 256, S.P > 1 ? 1024 : 4096), 256, 0, S.st>>>(ra);
    kt_end(S.st, KID_SH_ROWKEYS, 25.0 * R.nl);
  }
  S.launched("source rows");
}

// every rank's slice size -> the slices' processing-index bounds, this rank's
// slice
void set_slices(Shard &S, RecState &R, std::vector<uint64_t> mall) {
  R.mall = std::move(mall);
  R.slices = slice_offsets(R.mall);
  R.m = (uint32_t)R.mall[S.me];
  R.poff = (uint32_t)R.slices.b[S.me];
  S.ctx->shard_stats.n_slice = R.m;
}

// Rows -> slice owners as 16-B records (arrival order = file order).  The
// bounds lie on histogram bins (or at the end), so this rank's count per owner
// is a sum of its own bins `mine` (one rank: the kept rows) -- the plan needs
// no readback.  One rank, no row dropped: the records in row order, or
// (R.in_place) none at all -- the order sort reads the rows, and the send
// block is the fine kernel's scratch.
template <class Ex>
const uint4 *rows_to_owners(Shard &S, RecState &R, const uint32_t *mine, const Ex &ex,
                            uint32_t *nrecv) {
  const uint32_t P = S.P, nl = R.nl;
  RowOp16 rop{R.f, R.slice_keys, R.drop, (uint32_t)R.row_base, nullptr};
  PartPlan pp;
  rop.out = R.srows = S.take<uint4>(SN_SROWS, (size_t)nl + 1);  // room for every row (see plan_counts)
  R.in_place = R.one && R.kept == nl;
  if (R.in_place) {
    S.identity_plan(nl, pp);
  } else if (P == 1 && R.kept == nl) {
    S.emit_identity(rop, nl, pp);
  } else {
    uint64_t cnt[MAXP] = {};
    for (uint32_t q = 0; q < P; ++q)
      cnt[q] = P == 1 ? R.kept : bins_in(mine, R.slice_keys, q, R.shift);
    S.plan_counts(rop, nl, pp, cnt);
    S.emit(rop, pp);
  }
  return ex(rop.out, pp, SN_RIN, nrecv);
}

// The slice's processing order (one-sweep passes) and its Y records.  The
// two-stage order sort (coarse passes, per-segment LDS sort) when the slice's
// key density suits it: the slice holds m rows over its own key span, and the
// coarse digits are slice-relative, (key - kbase) >> F, so the segment table
// covers that span only.  The X axis' chunk width (solve_x) comes from the
// slice's own rows: the fine kernel then counts the slice's X-chunk entries
// as it writes the order, and solve_x adds the halo's (when its width comes
// out the same).
void slice_order(Shard &S, RecState &R, const uint4 *rin) {
  const uint32_t m = R.m, me = S.me;
  hipStream_t st = S.st;
  // (in place: the order and Y histograms are in, ehist zero; the head-first
  // Y schedule counts the Y keys itself)
  if (!R.in_place) S.zero(R.ahist, 3 * 4096 * 4);
  else if (R.y_early) S.zero(R.yhist, 4096 * 4);
  uint32_t *astat = S.take<uint32_t>(SN_STAT, nw_status_words(m + 1));
  uint4 *Ra = R.Ra = S.take<uint4>(SN_RA, m + 1), *Rb = S.take<uint4>(SN_RB, m + 1);
  uint4 *yown = R.yown = S.take<uint4>(SN_YOWN, (size_t)m * 3 / 4 + 2);  // 12-B records
  const NwOrderPlan op = R.in_place
                             ? R.op1
                             : nw_order_split_range(m, R.slice_keys.b[me], R.slice_keys.b[me + 1]);
  S.ctx->shard_stats.order_split = op.nseg ? 1u : 0u;
  R.span = (R.slice_keys.b[me + 1] - R.slice_keys.b[me]) / 10 + 2;
  NwChunkCounts &own_cc = R.own_cc;
  own_cc.W = nw_chunk_width(m, (uint32_t)(R.span < R.nbx ? R.span : R.nbx));
  while ((1u << own_cc.lgW) < own_cc.W) ++own_cc.lgW;
  own_cc.nch = nw_chunks(R.nbx, own_cc.W);
  if (m && op.nseg) {
    uint32_t *chist = S.take<uint32_t>(SN_CHIST, nw_seg_words(m));
    uint32_t *coff = S.take<uint32_t>(SN_COFF, nw_seg_words(m));
    own_cc.cnts = S.take<uint32_t>(SN_XCNT0, (size_t)3 * own_cc.nch + 2);
    if (R.in_place) {  // the rows themselves (op == op1, whose histogram is in)
      nw_order_sort_split_coarse(*R.in, op, R.ahist, astat, Ra, Rb, chist,
                                 ZeroRegion{own_cc.cnts, ((size_t)3 * own_cc.nch + 1) * 4},
                                 R.vsize, st, nullptr);
      nw_order_sort_split_fine(R.nl, m, R.nby, op, Ra, Rb, yown, R.srows, chist, coff,
                               S.scan_scratch(SL_PSCAN, (size_t)op.nseg + 1), &own_cc, st);
    } else {
      nw_rec_hist(rin, 16, m, op.kbase, op.coarse, R.ahist, st);
      // rin is read by the first coarse pass only: the fine kernel's scratch
      nw_order_sort_recs_split(rin, m, R.nby, R.poff, op, R.ahist, astat, Ra, Rb, yown,
                               const_cast<uint4 *>(rin), chist, coff,
                               S.scan_scratch(SL_PSCAN, (size_t)op.nseg + 1), &own_cc, st);
    }
    R.own_counts = true;
    S.launched("order sort");
  } else if (m) {
    if (R.in_place) {
      nw_order_sort(*R.in, R.vsize, R.nby, R.ad, R.ahist, astat, Ra, Rb, yown, st);
    } else {
      nw_rec_hist(rin, 16, m, 0, R.ad, R.ahist, st);
      nw_order_sort_recs(rin, m, R.nby, R.poff, R.ad, R.ahist, astat, Ra, Rb, yown, st);
    }
    S.launched("order sort");
  }
}

// ---- Y records -> Y-range owners (+ halos)
YOp12 y_op(const RecState &R, uint32_t P) {
  YOp12 yop{};
  yop.yrec = reinterpret_cast<const uint3 *>(R.yown);
  yop.nby = R.nby;
  yop.P = P;
  yop.shift = R.yshift;
  return yop;
}
void y_halo_ranges(const Bounds &yb, uint32_t P, uint64_t H, int64_t lo[MAXP], int64_t hi[MAXP]) {
  for (uint32_t q = 0; q < MAXP; ++q) {
    lo[q] = q < P ? (int64_t)yb.b[q] - 1 - (int64_t)H : 0;
    hi[q] = q < P ? (int64_t)yb.b[q + 1] + 1 + (int64_t)H : 0;
  }
}
// the records to the owners of R.yb's ranges; cnt: the per-owner counts (null:
// counted on the device and read back).  The masks stay cached for the X-hit
// bytes (xhits_follow_y).
template <class Ex>
void y_to_owners(Shard &S, RecState &R, YOp12 &yop, PartPlan &ypp, const uint64_t *cnt,
                 const Ex &ex) {
  const uint32_t m = R.m;
  y_halo_ranges(R.yb, S.P, R.H, yop.lo, yop.hi);
  if (S.P == 1) {  // one Y range, halos included: every record stays, in order
    S.identity_plan(m, ypp);
  } else {
    ypp.mcache = S.take<uint32_t>(SL_YMASK, m + 1);
    if (cnt) S.plan_counts(yop, m, ypp, cnt);
    else S.plan(yop, m, ypp);
  }
  // every own record stays here, once: the send layout is the records themselves
  const bool y_self = ypp.total == m && ypp.cnt[S.me] == m;
  if (!y_self) {
    yop.out = S.take<uint3>(SN_SY, ypp.total + 1);
    S.emit(yop, ypp);
  }
  R.yr = ex(y_self ? yop.yrec : yop.out, ypp, SN_YR, &R.ny);
  S.ctx->shard_stats.y_entries = R.ny;
}
// the Y range's buffers (ny records received)
void y_buffers(Shard &S, RecState &R) {
  const uint32_t ny = R.ny;
  R.ylo = R.yb.b[S.me], R.yhi = R.yb.b[S.me + 1];
  R.ycode = S.take<uint8_t>(SL_YCODE, ny + 1);
  R.ystate = S.take<uint8_t>(SL_YSTATE, ny + 1);
  R.ywin = S.take<uint32_t>(SL_YWIN, ny + 1);
  R.yused = S.take<uint8_t>(SL_YUSED, ny + 1);
  R.par_l = S.take<uint32_t>(SN_PARL, ny + 1);
  R.ystat = S.take<uint32_t>(SN_YSTAT, nw_status_words(ny + 1));
  R.yA = S.take<uint4>(SN_YA, (size_t)ny * 3 / 4 + 2);
  R.yB = S.take<uint4>(SN_YB, (size_t)ny * 3 / 4 + 2);
  R.cy.key = S.take<uint32_t>(SN_YKEY, ny + 1);
  R.cy.ent = S.take<uint32_t>(SN_YENT, ny + 1);
  R.cy.pk = S.take<uint2>(SN_YPK, ny + 1);
  R.cy.nbd = S.take<uint8_t>(SN_YNBD, ny + 1);
  R.cy.state = S.take<uint8_t>(SN_YST, ny + 1);
  R.ybits = S.take<uint32_t>(SN_XBITS, ny / 32 + 2);
}
// the Y sort's passes read the received records (first pass: arrival
// numbering) and ping-pong through yA / yB; the received array stays whole for
// the winners' global ids
void y_sort(Shard &S, const RecState &R, const uint3 *src, uint32_t n, const uint32_t *bits,
            hipStream_t s, bool head, bool tail) {
  if (!n) return;
  if (head) {
    nw_rec_hist(src, 12, n, 0, R.yd, R.yhist, s);
    nw_y_sort_head(R.yB, R.yA, n, R.yd, R.yhist, R.ystat, s, true,
                   reinterpret_cast<const uint4 *>(src));
  }
  if (tail)
    nw_y_sort_tail(R.yB, R.yA, n, R.yd, R.yhist, R.ystat, R.cy, R.nby, R.max_y, bits, s, true,
                   reinterpret_cast<const uint4 *>(src));
}
// Beside X on the second stream: the Y codes (codes) and the Y key histogram
// (in place: counted by k_nw_order_hist over the same rows).  The Y sort runs
// after X, as on one device (nw_y_sort_after_x): its first pass carries the
// X-hit bit in the records, so no pass shares the device with the X axis and
// the last one needs no lookup.  R.y_early: the round-3 schedule (the head
// passes beside X, the tail looking the bits up).
void y_beside_x(Shard &S, const RecState &R, bool codes) {
  rk_ctx *ctx = S.ctx;
  const uint32_t ny = R.ny;
  S.hip(hipEventRecord(ctx->fork, S.st), "fork");
  S.hip(hipStreamWaitEvent(S.st2, ctx->fork, 0), "fork wait");
  if (ny && codes) {
    k_sh_ycode<<<grid_for(ny, 256), 256, 0, S.st2>>>(R.yr, ny, R.nby, R.ylo, R.yhi, R.ycode);
    S.launched("k_sh_ycode");
  }
  if (R.y_early) {
    y_sort(S, R, R.yr, ny, nullptr, S.st2, true, false);
    S.launched("Y sort head");
  } else if (ny && !R.in_place) {
    nw_rec_hist(R.yr, 12, ny, 0, R.yd, R.yhist, S.st2);
  }
  S.hip(hipEventRecord(ctx->join, S.st2), "join");
}

// ---- X lead-in halo
// The start of the slice's suffix whose centres can reach a later slice's
// lead-in, into SC_LEAD_IN (false: no later slice has one, or the slice is empty)
bool lead_in_suffix(Shard &S, const RecState &R, const uint64_t *thr) {
  uint64_t thr_min = ~0ull;
  for (uint32_t g = S.me + 1; g < S.P; ++g) thr_min = thr[g] < thr_min ? thr[g] : thr_min;
  if (thr_min == ~0ull || !R.m) return false;
  const uint64_t reach = thr_min * 100;  // centre >= reach is needed
  const uint64_t half = R.maxlen / 2;
  const uint64_t key0 = reach > half + 10 ? (reach - half) / 10 - 1 : 0;
  k_lower_bound16<<<1, 1, 0, S.st>>>(R.Ra, R.m, key0, S.ctrl + SC_LEAD_IN);
  S.launched("k_lower_bound16");
  return true;
}
// halo entries from this bucket on are relevant: probed by own queries
uint64_t relevant_from(const RecState &R, uint32_t me) {
  const uint64_t bmin_me = R.slice_keys.b[me] / 10;
  return bmin_me >= 1 ? bmin_me - 1 : 0;
}

// ---- X axis over [halo ; own] (the X-chunk kernel, no sort)
void x_buffers(Shard &S, RecState &R, uint32_t G) {
  R.xg = S.take<uint32_t>(SL_XG, R.m + 1);
  R.xused = S.take<uint8_t>(SN_XGUSED, G + 1);
  S.zero(S.ctrl + SC_WIDE_KEYS, 4);
}
// resolve(axis, scratch, 0): the sweeps, with readbacks (resolve_axis) or
// queued (resolve_axis_queued); own(par, mx): the own results from the
// resolved axis' parent words (k_sh_x_own, k_sh_x_own_fast, or nw_x_bits at
// one rank).  par: the parent words (null: a buffer of their own).
template <class Resolve, class Own>
void solve_x(Shard &S, RecState &R, const uint4 *halo, uint32_t Gc, uint32_t *par,
             Resolve &&resolve, Own &&own) {
  hipStream_t st = S.st;
  const uint32_t mx = Gc + R.m, nbx = R.nbx;
  R.Gfin = Gc;  // (the member records sit behind the halo's)
  R.mx = mx;
  if (!mx) return;
  NwChunkCounts cc{};
  cc.W = nw_chunk_width(mx, (uint32_t)(R.span < nbx ? R.span : nbx));
  while ((1u << cc.lgW) < cc.W) ++cc.lgW;
  cc.nch = nw_chunks(nbx, cc.W);
  cc.cnts = S.take<uint32_t>(SN_XCNT, (size_t)3 * cc.nch + 2);
  uint32_t *xoff = S.take<uint32_t>(SN_XOFF, (size_t)3 * cc.nch + 2);
  if (R.own_counts && cc.W == R.own_cc.W) {
    S.hip(hipMemcpyAsync(cc.cnts, R.own_cc.cnts, ((size_t)3 * cc.nch + 1) * 4,
                         hipMemcpyDeviceToDevice, st), "counts copy");
    nw_x_count_add(halo, Gc, cc, st);
  } else {
    nw_x_count(R.Ra, mx, cc, st, halo, Gc);
  }
  exclusive_scan_u32(cc.cnts, xoff, (size_t)3 * cc.nch + 1,
                     S.scan_scratch(SL_PSCAN, (size_t)3 * cc.nch + 1), st);
  Csr cx{};
  cx.key = S.take<uint32_t>(SN_XKEY, mx + 1);
  cx.ent = S.take<uint32_t>(SN_XENT, mx + 1);
  cx.pk = S.take<uint2>(SN_XPK, mx + 1);
  cx.nbd = S.take<uint8_t>(SN_XNBD, mx + 1);
  cx.state = S.take<uint8_t>(SN_XSTATE, mx + 1);
  uint4 *erec = S.take<uint4>(SN_EREC, (size_t)mx * 3 / 4 + 2);
  if (!par) par = S.take<uint32_t>(SN_PAR, mx + 1);
  nw_x_chunks(R.Ra, mx, nbx, R.max_x, R.maxlen, xoff, cx, erec, S.ctrl, cc.W, st, halo, Gc);
  S.launched("X chunks");
  Axis ax{cx.key, cx.ent, nullptr, nullptr, cx.state, nullptr, par, cx.pk, cx.nbd,
          S.take<uint32_t>(SL_RLEN, mx), S.take<uint32_t>(SL_RBEG, mx), mx, R.max_x,
          R.p.len_ratio, R.p.pos_ratio};
  SweepScratch sc{S.take<uint32_t>(SL_RUNS, runs_scratch_words(mx)),
                  S.take<uint8_t>(SL_WPEND, mx / 64 + 1), S.take<uint8_t>(SL_RPEND, mx),
                  S.ctrl + SC_PEND, S.ctrl + SC_SWEEP_COUNT};
  resolve(ax, sc, 0);
  own(par, mx);
}

// ---- Y axis
// The X-hit bytes follow the Y records (the same plan, the same order) and
// become the code bits and the Y sort's bitmask.
template <class Ex>
void xhits_follow_y(Shard &S, const RecState &R, const YOp12 &yop, const PartPlan &ypp,
                    const Ex &ex) {
  YOp12 xop = yop;
  xop.xg = R.xg;
  PartPlan xpp;
  xop.xout = S.take<uint8_t>(SN_SXH, (size_t)ypp.total + 1);
  if (S.P == 1) {
    S.emit_identity(xop, R.m, xpp);
  } else {
    xpp.mcache = ypp.mcache;
    xpp.mread = true;
    S.plan_same(xop, R.m, xpp, ypp);  // the Y records' own selection: counts known
    S.emit(xop, xpp);
  }
  uint32_t n2 = 0;
  const uint8_t *xh = ex(xop.xout, xpp, SL_YXH, &n2);
  if (n2 != R.ny) {
    S.ctx->err = "Y X-hit count mismatch";
    throw RK_E_INTERNAL;
  }
  S.hip(hipStreamWaitEvent(S.st, S.ctx->join, 0), "join wait");
  if (R.ny) {
    kt_begin(S.st, KID_SH_MERGE);
    k_sh_xhit_bits<<<grid_for(R.ny, 256), 256, 0, S.st>>>(xh, R.ny, R.ycode, R.ybits);
    kt_end(S.st, KID_SH_MERGE, 0.0);
    S.launched("k_sh_xhit_bits");
  }
}
// the sweeps over the first n entries of the sorted Y axis (resolve as in
// solve_x, axis 1); par: the parent words
template <class Resolve>
void sweep_y(Shard &S, const RecState &R, uint32_t n, uint32_t *par, Resolve &&resolve) {
  if (!n) return;
  const Csr &cy = R.cy;
  Axis ay{cy.key, cy.ent, nullptr, nullptr, cy.state, nullptr, par, cy.pk, cy.nbd,
          S.take<uint32_t>(SL_RLEN, n), S.take<uint32_t>(SL_RBEG, n), n, R.max_y, R.p.len_ratio,
          R.p.pos_ratio};
  ay.par_dev = true;
  SweepScratch sc{S.take<uint32_t>(SL_RUNS, runs_scratch_words(n)),
                  S.take<uint8_t>(SL_WPEND, n / 64 + 1), S.take<uint8_t>(SL_RPEND, n),
                  S.ctrl + SC_PEND, S.ctrl + SC_SWEEP_COUNT};
  resolve(ay, sc, 1);
}

// ---- members
// the member op over the own rows' gids: the X chunk kernel wrote the member
// records behind the last solve's halo's
MemOpNw member_op(Shard &S, const RecState &R, const uint32_t *gid_own, uint64_t Gtot,
                  const uint2 **erk_out) {
  const uint2 *erk =
      reinterpret_cast<const uint2 *>(S.take<uint4>(SN_EREC, (size_t)R.mx * 3 / 4 + 2));
  *erk_out = erk;
  return MemOpNw{gid_own, erk + R.Gfin, reinterpret_cast<const uint32_t *>(erk + R.mx) + R.Gfin,
                 {}, bin_shift(Gtot), true, nullptr};
}
void emit_members(Shard &S, const RecState &R) {
  emit_result(R.otag, R.sgid, R.goffs, R.mrow, R.mr, R.ogid, R.orep, R.oord, S.st);
  if (R.g0) k_add_u32<<<grid_for(R.mr, 256), 256, 0, S.st>>>(R.ogid, R.mr, R.g0);
}
// Member order: the gid range gb[me]'s mr members -- received as records
// (mem), or at one rank without a halo read in place from the X chunk's member
// arrays erk and the gids (mem null) -- sorted by local gid, then exactly
// inside every group, and the result.  heap_count: the depth-limit heap
// segments are counted there and sorted later by the caller (null: here).
void member_order(Shard &S, RecState &R, const void *mem, uint32_t mr, const Bounds &gb,
                  bool narrow, const uint2 *erk, const uint32_t *gid_own, uint32_t *heap_count) {
  rk_ctx *ctx = S.ctx;
  hipStream_t st = S.st, st2 = S.st2;
  const uint32_t g0 = R.g0 = (uint32_t)gb.b[S.me];
  const uint32_t Gl = R.Gl = (uint32_t)(gb.b[S.me + 1] - gb.b[S.me]);
  R.mr = mr;
  R.ogid = S.take<uint32_t>(SL_OGID, mr + 1);
  R.orep = S.take<uint8_t>(SL_OREP, mr + 1);
  R.oord = S.take<uint32_t>(SL_OORD, mr + 1);
  if (!mr) return;
  const NwDigits ed = nw_plan(bit_length(Gl ? Gl - 1 : 0), narrow ? 9 : 8);
  R.sgid = S.take<uint32_t>(SN_SGID, mr + 1);
  R.mrow = S.take<uint32_t>(SN_MROW, mr + 1);
  R.reckey = S.take<uint64_t>(SN_KEY, mr + 1);
  R.tag = S.take<uint32_t>(SN_TAG, mr + 1);
  R.otag = S.take<uint32_t>(SL_OTAG, mr + 1);
  R.goffs = S.take<uint32_t>(SN_GOFF, (size_t)Gl + 2);
  uint4 *t0 = S.take<uint4>(SN_T0, mr + 1), *t1 = S.take<uint4>(SN_T1, mr + 1);
  uint32_t *mstat = S.take<uint32_t>(SN_STAT, nw_status_words(mr + 1));
  R.gsort = S.take<uint8_t>(SL_GSORT, groupsort_scratch_bytes(mr));
  S.zero(R.ehist, 4096 * 4);
  if (!mem) {
    nw_rec_hist(gid_own, 4, mr, g0, ed, R.ehist, st);
    nw_member_sort(reinterpret_cast<const uint4 *>(erk), gid_own, t0, t1, mr, ed, R.ehist, mstat,
                   R.sgid, R.reckey, R.tag, R.mrow, narrow, st);
  } else {
    nw_rec_hist(mem, narrow ? 12 : 16, mr, g0, ed, R.ehist, st);
    nw_member_sort_recv(mem, narrow, mr, g0, ed, R.ehist, mstat, t0, t1, R.sgid, R.reckey, R.tag,
                        R.mrow, st);
  }
  group_offsets(R.sgid, mr, Gl, R.goffs, st);
  // the group-sort tiers on both streams, as in the single-device path
  const int rc = sort_groups_exact(R.sgid, R.goffs, Gl, mr, R.reckey, R.tag, R.otag, R.gsort,
                                   S.scan_scratch(SL_SCAN, mr + Gl + 2), ctx->host + HOST_SCRATCH,
                                   narrow, st, st2 != st ? st2 : nullptr, ctx->fork, ctx->join,
                                   heap_count);
  if (!heap_count) S.check(rc);
  emit_members(S, R);
  S.launched("member order");
}

// ---- the careful driver -----------------------------------------------------------
// Every exchange is sized by a device count read back and gathered right
// before it, the sweeps and the jumping rounds are read back, and a halo that
// disagrees with its owners is re-resolved.  Returns RK_OK, an error, or
// RK_SHARD_FALLBACK.
int classify_sharded_nw(Shard &S, const Geom &geo, const rk_frags_soa *in, const rk_params &p,
                        bool one_on, bool y_early, uint64_t row_base, rk_shard_result *out,
                        std::chrono::steady_clock::time_point t0) {
  rk_ctx *ctx = S.ctx;
  rk_shard_stats &ss = ctx->shard_stats;
  const uint32_t P = S.P, me = S.me;
  hipStream_t st = S.st;
  RecState R = rec_state(S, geo, in, p, one_on, y_early);
  R.row_base = row_base;
  const CarefulExchange ex{S};
  const auto resolve = [&](const Axis &a, const SweepScratch &sc, int axis) {
    uint32_t sweeps = 0;
    S.check(resolve_axis(ctx, a, sc, true, &sweeps));
    S.max_sweeps[axis] = sweeps > S.max_sweeps[axis] ? sweeps : S.max_sweeps[axis];
  };

  // ---- 1: keys, checks and the slice histogram at the source; every rank
  // agrees on the record layout (or all run the generic driver)
  S.zero(R.ahist, NBINS * 4);  // (the slice histogram; later the sorts' digit histograms)
  S.zero(S.ctrl + SC_REC_KEPT, 4);
  source_rows(S, R, S.ctrl, P > 1 ? R.ahist : nullptr, nullptr);
  // the error bits, the pack flag and the longest length, the kept count and
  // the slice histogram in one readback, and the first three with the
  // histogram in one all-gather
  std::vector<uint32_t> flags(RB_SH_ROWS_ONE_N);
  const uint32_t MW = 2 + (P > 1 ? NBINS : 0);  // message words
  std::vector<uint32_t> msg(MW);
  S.hip(hipMemcpyAsync(flags.data(), S.ctrl + SC_ERR,
                       (R.one ? RB_SH_ROWS_ONE_N : RB_SH_ROWS_N) * 4, hipMemcpyDeviceToHost, st),
        "d2h");
  if (P > 1)
    S.hip(hipMemcpyAsync(msg.data() + 2, R.ahist, NBINS * 4, hipMemcpyDeviceToHost, st), "d2h");
  ++S.n_syncs;
  S.hip(hipStreamSynchronize(st), "d2h sync");
  if (R.one) {  // k_nw_order_hist's words in k_sh_rows' layout
    flags[SC_ERR] = flags[SC_ONE + CW_ERR];
    flags[SC_REC_KEPT] = flags[SC_ONE + CW_KEPT];
    flags[SC_NOPACK] = flags[SC_ONE + CW_NOPACK];
    flags[SC_MAXLEN] = flags[SC_ONE + CW_MAXLEN];
  }
  msg[0] = flags[SC_ERR];
  msg[1] = flags[SC_NOPACK] | (flags[SC_MAXLEN] << 1);
  std::vector<uint32_t> allm((size_t)P * MW);
  S.allgather(msg.data(), allm.data(), MW * 4);
  uint32_t anyerr = 0, nopack = 0;
  std::vector<uint64_t> gh(NBINS, 0);
  for (uint32_t q = 0; q < P; ++q) {
    const uint32_t *mq = allm.data() + (size_t)q * MW;
    anyerr |= mq[0];
    nopack |= mq[1] & 1u;
    R.maxlen = (mq[1] >> 1) > R.maxlen ? (mq[1] >> 1) : R.maxlen;
    if (P > 1)
      for (uint32_t b = 0; b < NBINS; ++b) gh[b] += mq[2 + b];
  }
  S.check(err_status(ctx, anyerr & ~(uint32_t)ERRB_WIDE_LENGTH));
  if (nopack) return RK_SHARD_FALLBACK;
  R.kept = flags[SC_REC_KEPT];
  R.slice_keys = split_bounds(gh, R.shift, R.drop, P);
  // the one-sweep passes' status words carry a 30-bit count (SW_VAL,
  // rk_onesweep.h), as the single-device record pipeline's bound n < 2^30
  // (record_eligible): a slice of 2^30 or more rows takes the generic driver.
  // Every rank sees the same global histogram (the kept count at one rank), so
  // the decision is agreed
  if (slice_max_rows(gh, R.slice_keys, R.shift, P, R.kept) >= (1ull << 30))
    return RK_SHARD_FALLBACK;

  // ---- 2: rows -> slice owners; every rank's slice size is known from the
  // exchange's count all-gather
  uint32_t m = 0;
  const uint4 *rin = rows_to_owners(S, R, msg.data() + 2, ex, &m);
  set_slices(S, R, std::vector<uint64_t>(S.last_recv, S.last_recv + P));

  // ---- 3: the slice's processing order, its Y records
  slice_order(S, R, rin);
  ss.ms_ingress = ms_since(t0);

  // ---- 4: Y records -> Y-range owners (+ halos), their ranges from the
  // global histogram of the records' buckets; beside X on the second stream:
  // the Y codes and the Y key histogram (or the Y sort's head passes)
  const auto ty = std::chrono::steady_clock::now();
  YOp12 yop = y_op(R, P);
  R.yb = split_bounds(P > 1 ? global_hist(S, yop, m) : std::vector<uint64_t>(NBINS, 0), R.yshift,
                      R.nby, P);
  PartPlan ypp;
  y_to_owners(S, R, yop, ypp, nullptr, ex);
  // the Y ranges (+ halos) received: the same 30-bit bound on every rank's
  // sort (every rank knows every rank's count from the exchange)
  S.check_recv_below(1u << 30, RK_E_TOO_MANY, "a Y range of 2^30 or more records");
  y_buffers(S, R);
  const uint32_t ny = R.ny;
  y_beside_x(S, R, true);
  ss.ms_y = ms_since(ty);

  // ---- 5: X lead-in halo from earlier slices (16-B records, global ids)
  const auto tx = std::chrono::steady_clock::now();
  GhostOp16 gop{};
  gop.R = R.Ra;
  gop.P = P;
  gop.me = me;
  gop.poff = R.poff;
  lead_in_thresholds(gop.thr, R.mall, R.slice_keys, R.H);
  gop.base = lead_in_suffix(S, R, gop.thr) ? S.read1(S.ctrl + SC_LEAD_IN) : m;
  const uint32_t nsuf = m - gop.base;
  PartPlan pp;
  if (nsuf) S.plan(gop, nsuf, pp);
  else S.zero_plan(0, pp);  // no row can reach a later slice: nothing to send
  gop.out = S.take<uint4>(SN_SHALO, pp.total + 1);
  if (nsuf) S.emit(gop, pp);
  uint32_t G = 0;
  const uint4 *hx = ex(gop.out, pp, SN_HX, &G);
  ss.x_ghosts = G;

  // ---- 6: X axis over [halo ; own]
  x_buffers(S, R, G);
  uint32_t *xg = R.xg;
  const auto x_own = [&](const uint4 *halo, uint32_t Gc) {
    return [&, halo, Gc](const uint32_t *par, uint32_t mx) {
      kt_begin(st, KID_SH_XOWN);
      k_sh_x_own<<<grid_for(mx, 256), 256, 0, st>>>(par, halo, Gc, m, R.poff, xg, R.xused);
      kt_end(st, KID_SH_XOWN, 0.0);
      S.launched("k_sh_x_own");
    };
  };
  solve_x(S, R, hx, G, nullptr, resolve, x_own(hx, G));
  // verify the relevant halo against its owners' decisions (one rank: there
  // are no later slices, so no halo was sent or received)
  const uint64_t rel_x = relevant_from(R, me);
  for (; P > 1;) {
    ++ss.x_rounds;
    if (ss.x_rounds > P + 2) {
      ctx->err = "X halo verification did not converge";
      throw RK_E_INTERNAL;
    }
    GhostOp16 sop = gop;
    sop.out = nullptr;
    sop.xg = xg;
    S.plan(sop, nsuf, pp);
    sop.sout = S.take<uint8_t>(SL_SEND, pp.total + 1);
    S.emit(sop, pp);
    uint32_t G2 = 0;
    uint8_t *xown = S.exchange<uint8_t>(sop.sout, pp, SL_XOWN, &G2);
    if (G2 != G) {
      ctx->err = "X halo state count mismatch";
      throw RK_E_INTERNAL;
    }
    S.zero(S.ctrl + SC_MISMATCH, 4);
    if (G) {
      k_cmp_x16<<<grid_for(G, 256, 1024), 256, 0, st>>>(hx, G, rel_x, R.xused, xown,
                                                        S.ctrl + SC_MISMATCH);
      S.launched("k_cmp_x16");
    }
    const uint32_t mism = S.read1(S.ctrl + SC_MISMATCH);
    if (S.sum_any(mism) == 0) break;
    if (mism) {  // re-resolve with the halo fixed to the owners' states
      ++ss.x_reruns;
      SelXOp16 sel{hx, xown, rel_x, nullptr};
      PartPlan sp;
      Shard S1 = S;
      S1.P = 1;
      S1.me = 0;
      S1.plan(sel, G, sp);
      sel.out = S.take<uint4>(SN_HSEL, sp.total + 1);
      S1.emit(sel, sp);
      solve_x(S, R, sel.out, (uint32_t)sp.total, nullptr, resolve,
              x_own(sel.out, (uint32_t)sp.total));
      S.hip(hipMemcpyAsync(R.xused, xown, G, hipMemcpyDeviceToDevice, st), "xused copy");
    }
  }
  ss.ms_x = ms_since(tx);

  // ---- 7: the X-hit bytes follow the Y records; the Y sort's last pass
  // writes the CSR with the states
  const auto ty2 = std::chrono::steady_clock::now();
  xhits_follow_y(S, R, yop, ypp, ex);
  const auto y_results = [&](const uint32_t *ymap, uint32_t c) {
    if (!c) return;
    kt_begin(st, KID_SH_YRES);
    k_sh_y_results<<<grid_for(c, 256), 256, 0, st>>>(R.yr, R.ycode, ymap, c, R.par_l, R.ystate,
                                                      R.ywin, R.poff, m, xg);
    kt_end(st, KID_SH_YRES, 0.0);
    S.launched("k_sh_y_results");
  };
  if (R.y_early) {
    y_sort(S, R, R.yr, ny, R.ybits, st, false, true);
  } else if (ny) {
    nw_y_sort_after_x(R.yB, R.yA, ny, R.yd, R.yhist, R.ystat, R.cy, R.nby, R.max_y, R.ybits, st,
                      reinterpret_cast<const uint4 *>(R.yr));
  }
  S.launched("Y sort");
  sweep_y(S, R, ny, R.par_l, resolve);
  y_results(nullptr, ny);
  // a fixed-halo re-resolution: the selected records sorted again on stream 1
  const auto solve_y = [&](const uint32_t *ymap, uint32_t c) {
    if (!c) return;
    uint3 *ysel = S.take<uint3>(SN_YSEL, c + 1);
    k_sh_ysel<<<grid_for(c, 256), 256, 0, st>>>(R.yr, R.ycode, ymap, c, ysel, R.ybits);
    S.launched("k_sh_ysel");
    S.zero(R.yhist, 4096 * 4);
    y_sort(S, R, ysel, c, R.ybits, st, true, true);
    sweep_y(S, R, c, R.par_l, resolve);
    y_results(ymap, c);
  };
  const RelOp relop{R.ycode, R.ylo ? owner_of_host(R.yb, R.ylo - 1) : 0u,
                    R.yhi < R.nby ? owner_of_host(R.yb, R.yhi) : 0u, nullptr};
  verify_y_halo(S, relop, R.ycode, R.ystate, R.yused, R.yb, ny, solve_y);
  ss.ms_y += ms_since(ty2);

  // ---- 8: parents back to the slice owners; roots; gids
  const auto tr = std::chrono::steady_clock::now();
  ParOp12 pop{R.yr, R.ycode, R.slices, R.ywin, me, nullptr};
  if (P == 1) S.zero_plan(ny, pp);  // every parent is local (written by k_sh_y_results)
  else S.plan(pop, ny, pp);
  pop.out = S.take<ParRec>(SL_SEND, pp.total + 1);
  if (P > 1) S.emit(pop, pp);
  uint32_t npar = 0;
  const ParRec *prr = S.exchange<ParRec>(pop.out, pp, SL_PR, &npar);
  uint64_t Gtot = 0;
  const uint32_t *gid_own = resolve_roots(S, xg, prr, npar, m, R.poff, R.slices, &Gtot);
  ss.ms_roots = ms_since(tr);

  // ---- 9: members -> gid-range owners; exact in-group order; emit
  const auto tm = std::chrono::steady_clock::now();
  const uint2 *erk = nullptr;
  MemOpNw mop = member_op(S, R, gid_own, Gtot, &erk);
  // the gid histogram and the wide-key flags (the X-chunk kernel's) in one
  // readback and one all-gather
  std::vector<uint32_t> wide;
  std::vector<uint64_t> ghist(NBINS, 0);
  if (P > 1) ghist = global_hist(S, mop, m, {S.ctrl + SC_WIDE_KEYS}, &wide);
  else wide = S.gather1<uint32_t>(S.read1(S.ctrl + SC_WIDE_KEYS));
  bool narrow = true;  // every sort key fits 32 bits
  for (uint32_t w : wide) narrow &= w == 0;
  mop.narrow = narrow;
  const Bounds gb = split_bounds(ghist, mop.shift, Gtot, P);
  mop.B = gb;
  // one rank: every member stays here and the X chunk's member arrays are
  // exactly the own rows (no halo): the member sort reads them in place, as on
  // one device (no plan needed)
  const bool m_self = P == 1 && R.Gfin == 0;
  uint32_t mr = 0;
  const void *mem = nullptr;
  if (m_self) {
    S.agree(RK_OK);  // the exchange's agreement point
    mr = m;
    S.last_recv[0] = mr;
  } else {
    S.plan(mop, m, pp);
    mop.out = S.take<uint8_t>(SN_SMEM, (pp.total + 1) * (narrow ? 12 : 16));
    S.emit(mop, pp);
    mem = narrow ? (const void *)ex((const uint3 *)mop.out, pp, SL_MEM, &mr)
                 : (const void *)ex((const uint4 *)mop.out, pp, SL_MEM, &mr);
  }
  // the gid range's members: the same 30-bit bound on the member sort
  S.check_recv_below(1u << 30, RK_E_TOO_MANY, "a gid range of 2^30 or more members");
  member_order(S, R, mem, mr, gb, narrow, erk, gid_own, nullptr);
  // every rank's share of the output: its received members
  const std::vector<uint64_t> oall(S.last_recv, S.last_recv + P);
  S.hip(hipStreamSynchronize(st), "final sync");
  S.agree_errors();
  ss.ms_members = ms_since(tm);
  set_result(out, R.oord, R.ogid, R.orep, mr, oall, me, Gtot);
  return RK_OK;
}
