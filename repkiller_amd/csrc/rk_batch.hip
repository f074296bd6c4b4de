// rk_batch.hip -- many fragment sets in one classification (gfx950).
//
// rk_classify_device_batch runs a whole batch of sets through the record
// pipeline (rk_narrow.hip) at the cost of ONE call:
//
//   1 k_batch_pack   every set's rows are translated into the set's own window
//                    of one combined coordinate space (rk_batch_layout: bases
//                    are multiples of 100, so every xStart/10 and centre/100
//                    bucket relation inside a set is kept; deviations and
//                    in-group sort keys depend on differences only).  Rows of
//                    a set's never-iterated last xStart/10 bucket go to the
//                    combined set's own last bucket, which the pipeline drops
//                    before any check.  The per-set checks rk_classify would
//                    make (xStart/10 >= vsize, probes past an occupancy array)
//                    happen here, before the translation.
//   2 the combined set is classified by rk_classify_device.  Sets sit in
//     increasing windows, so their rows are processed -- and their groups
//     created -- one set after the other: every set's output rows and gids
//     are one contiguous range.
//   3 k_batch_nbd    (called by the pipeline once per axis) the only thing
//                    that does not translate: the upward-probe guards compare
//                    a centre with the SET's bucket count
//                    (SequenceOcupationList.cpp:58,80); the CSR's one byte per
//                    entry is rewritten for centres of remainder 98 / 99.
//   4 k_batch_split  the combined result back into per-set results with local
//                    rows and gids.
//
// Sets are packed greedily, in order, into sub-batches that fit the record
// pipeline's limits; a sub-batch it cannot take (a row that does not pack, a
// context on the generic pipeline) is classified set by set.
#include <cstdio>
#include <cstdlib>
#include <new>
#include <string>
#include <vector>

#include "rk_ctx.h"

namespace rk {

struct BatchState {
  void *dev = nullptr;  // translated rows + combined result + tables + words
  size_t dev_cap = 0;
  char *host = nullptr;  // pinned: tables up, words back
  size_t host_cap = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

void batch_destroy(rk_ctx *ctx) {
  BatchState *b = ctx->batch;
  if (!b) return;
  if (b->dev) (void)hipFree(b->dev);
  if (b->host) (void)hipHostFree(b->host);
  if (b->ev0) (void)hipEventDestroy(b->ev0);
  if (b->ev1) (void)hipEventDestroy(b->ev1);
  delete b;
  ctx->batch = nullptr;
}

namespace {

constexpr uint32_t BW_ERR = 0, BW_NOPACK = 1, BW_INTERNAL = 2, BW_HEAD = 4;

// the set k with t[k] <= v < t[k + 1] (t non-decreasing, t[0] <= v < t[n])
__device__ __forceinline__ uint32_t find_set(const uint32_t *__restrict__ t, uint32_t n,
                                             uint32_t v) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (t[mid] <= v) lo = mid;
    else hi = mid;
  }
  return lo;
}

// largest bucket get_associated_group touches for centre c
// (SequenceOcupationList.cpp:40-93; max_index - 1 wraps as there)
__device__ __forceinline__ uint64_t probe_max_bucket_b(uint64_t c, uint64_t max_index) {
  uint64_t b = c / 100;
  if (c < max_index && (c + 1) / 100 > b) b = (c + 1) / 100;
  if (c < max_index - 1 && (c + 2) / 100 > b) b = (c + 2) / 100;
  return b;
}

struct PackArgs {
  const uint64_t *x, *y, *len;
  const uint8_t *s;
  uint32_t n, nsets;
  const uint32_t *roff;      // nsets + 1: the sets' first rows
  const uint64_t *bx, *by;   // nsets + 1: window starts (coordinates)
  const uint64_t *vsize;     // nsets
  const uint32_t *mix, *miy; // nsets
  uint64_t *ox, *oy, *ol;
  uint8_t *os;
  uint32_t *words;  // BW_HEAD flag words, then err[nsets], kept[nsets]
};

// One pass over the concatenated rows, a run of consecutive rows per wave, 64
// at a time.  While the 64 rows belong to one set (every step of a large set)
// the wave keeps the set's kept count and error bits in registers, until its
// set changes: one atomic per wave and set, not per row.
__global__ void __launch_bounds__(256) k_batch_pack(const PackArgs a) {
  uint32_t *const err = a.words + BW_HEAD, *const kept = err + a.nsets;
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t trash_x = a.bx[a.nsets];
  uint32_t acc_k = 0xFFFFFFFFu, acc_n = 0, acc_e = 0;
  bool nopack = false, anyerr = false;
  // (consecutive rows per wave: its set changes as rarely as the rows allow)
  const uint32_t waves = gridDim.x * (blockDim.x >> 6);
  const uint32_t per = ((a.n + waves - 1) / waves + 63u) & ~63u;
  const uint64_t w0 = (uint64_t)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * per;
  const uint32_t end = w0 + per < a.n ? (uint32_t)(w0 + per) : a.n;
  for (uint32_t b = w0 < a.n ? (uint32_t)w0 : a.n; b < end; b += 64) {
    const uint32_t i = b + lane;
    const bool live = i < end;
    uint32_t k = 0, e = 0;
    bool keep = false;
    if (live) {
      k = find_set(a.roff, a.nsets, i);
      const uint64_t xs = a.x[i], ys = a.y[i], L0 = a.len[i];
      const uint64_t vs = a.vsize[k], pk = xs / 10;
      if (pk >= vs) e |= ERRB_UB_BUCKET;
      // (vs - 1: the never-iterated last bucket, FragmentsDatabase.h:29-31)
      if (pk < vs - 1) {
        const uint64_t h = L0 / 2, mx = a.mix[k], my = a.miy[k];
        if (probe_max_bucket_b(xs + h, mx) > mx || probe_max_bucket_b(ys + h, my) > my)
          e |= ERRB_UB_CENTER;
        else
          keep = true;
      }
      const uint64_t ty = ys + a.by[k];
      nopack |= keep && (L0 >= (1ull << 24) || ys >= (1ull << 35) || ty >= (1ull << 35));
      a.ox[i] = keep ? xs + a.bx[k] : trash_x;
      a.oy[i] = keep ? ty : 0;
      a.ol[i] = keep ? L0 : 0;
      a.os[i] = a.s[i];
    }
    anyerr |= e != 0;
    const uint32_t k0 = __shfl(k, 0);  // (lane 0 is live: b < end)
    if (__all(!live || k == k0)) {
      if (k0 != acc_k) {
        if (lane == 0 && acc_k != 0xFFFFFFFFu) {
          if (acc_n) atomicAdd(&kept[acc_k], acc_n);
          if (acc_e) atomicOr(&err[acc_k], acc_e);
        }
        acc_k = k0, acc_n = 0, acc_e = 0;
      }
      acc_n += __popcll(__ballot(keep));
      acc_e |= (__ballot(e & ERRB_UB_BUCKET) ? ERRB_UB_BUCKET : 0u) |
               (__ballot(e & ERRB_UB_CENTER) ? ERRB_UB_CENTER : 0u);
    } else if (live) {
      if (keep) atomicAdd(&kept[k], 1u);
      if (e) atomicOr(&err[k], e);
    }
  }
  if (lane == 0 && acc_k != 0xFFFFFFFFu) {
    if (acc_n) atomicAdd(&kept[acc_k], acc_n);
    if (acc_e) atomicOr(&err[acc_k], acc_e);
  }
  const uint64_t be = __ballot(anyerr), bn = __ballot(nopack);
  if (lane == 0) {
    if (be) atomicOr(&a.words[BW_ERR], 1u);
    if (bn) atomicOr(&a.words[BW_NOPACK], 1u);
  }
}

// start[k] = kept rows of the sets before k (nsets + 1 entries), one block
__global__ void __launch_bounds__(1024) k_batch_scan(const uint32_t *__restrict__ kept,
                                                     uint32_t nsets,
                                                     uint32_t *__restrict__ start) {
  __shared__ uint32_t sh[1024];
  __shared__ uint32_t carry;
  const uint32_t t = threadIdx.x;
  if (t == 0) carry = 0;
  __syncthreads();
  for (uint32_t b = 0; b < nsets + 1; b += 1024) {
    const uint32_t k = b + t;
    const uint32_t v = k < nsets ? kept[k] : 0u;
    sh[t] = v;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) {
      const uint32_t o = t >= off ? sh[t - off] : 0u;
      __syncthreads();
      sh[t] += o;
      __syncthreads();
    }
    const uint32_t base = carry;
    if (k < nsets + 1) start[k] = base + sh[t] - v;
    __syncthreads();
    if (t == 1023) carry = base + sh[t];
    __syncthreads();
  }
}

// entries whose centre has remainder 98 / 99: the upward probe as the entry's
// own set decides it (neighbour_dir with the local centre and the set's
// max_index; max_index - 1 wraps as there).  Other entries are left alone.
__global__ void __launch_bounds__(256) k_batch_nbd(const uint32_t *__restrict__ key,
                                                   const uint2 *__restrict__ pk,
                                                   uint8_t *__restrict__ nbd, uint32_t m,
                                                   uint32_t nb, const uint32_t *__restrict__ bkt,
                                                   const uint32_t *__restrict__ mi,
                                                   uint32_t nsets) {
  for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < m; q += gridDim.x * blockDim.x) {
    const uint32_t kq = key[q], b = kq >= nb ? kq - nb : kq;
    const uint32_t rem = pk[q].x - b * 100u;  // (the low 32 bits of the centre suffice)
    if (rem != 98u && rem != 99u) continue;
    // (a bucket outside every window cannot hold an entry; clamped all the same)
    const uint32_t bc = b < bkt[nsets] ? b : bkt[nsets] - 1;
    const uint32_t k = find_set(bkt, nsets, bc);
    const uint64_t c = (uint64_t)(bc - bkt[k]) * 100 + rem, mx = mi[k];
    nbd[q] = (rem == 99u && c < mx) || (rem == 98u && c < mx - 1) ? 2 : 0;
  }
}

struct SplitArgs {
  const uint32_t *order, *gid;
  const uint8_t *rep;
  uint32_t m, n, nsets;
  const uint32_t *roff, *start;
  uint32_t *out_order, *out_gid;
  uint8_t *out_rep;
  uint32_t *gbase;  // nsets: the gid at the set's first output position
  uint32_t *words;
};

// combined output position p belongs to the set of its row; the set's rows
// are positions [start[k], start[k + 1])
__global__ void __launch_bounds__(256) k_batch_split(const SplitArgs a) {
  bool bad = false;
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < a.m; p += gridDim.x * blockDim.x) {
    const uint32_t row = a.order[p];
    if (row >= a.n) {
      bad = true;
      continue;
    }
    const uint32_t k = find_set(a.roff, a.nsets, row);
    const uint32_t s0 = a.start[k], r0 = a.roff[k];
    if (p < s0 || p >= a.start[k + 1] || p - s0 >= a.roff[k + 1] - r0) {
      bad = true;
      continue;
    }
    const uint32_t g0 = a.gid[s0], g = a.gid[p], dst = r0 + (p - s0);
    bad |= g < g0;
    a.out_order[dst] = row - r0;
    a.out_gid[dst] = g - g0;
    a.out_rep[dst] = a.rep[p];
    if (p == s0) a.gbase[k] = g0;
  }
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&a.words[BW_INTERNAL], 1u);
}

// ---------------------------------------------------------------------------
// host side

struct SetGeom {
  uint64_t vsize, mi_x, mi_y, wx, wy;
  bool ok;  // the window sizes did not overflow
};

SetGeom set_geom(uint64_t hx, uint64_t hy) {
  SetGeom g{};
  const uint64_t len_x = hx + 1, len_y = hy + 1;  // FragmentsDatabase.cpp:62,65 (wraps as there)
  g.vsize = 1 + len_x / 10;
  g.mi_x = len_x / 100;
  g.mi_y = len_y / 100;
  // X: every admissible xStart (xStart/10 < vsize), centre buckets 0..mi_x and
  // one empty bucket; Y: centre buckets 0..mi_y and one empty bucket
  const uint64_t top = (10 * g.vsize - 1) / 100;
  const uint64_t bx = (g.mi_x > top ? g.mi_x : top) + 2, by = g.mi_y + 2;
  g.ok = bx < (1ull << 56) && by < (1ull << 56);
  g.wx = 100 * bx;
  g.wy = 100 * by;
  return g;
}

uint64_t env_u64(const char *name, uint64_t dflt) {
  const char *e = std::getenv(name);
  if (!e || !*e) return dflt;
  char *end = nullptr;
  const unsigned long long v = std::strtoull(e, &end, 10);
  return end == e || v == 0 ? dflt : (uint64_t)v;
}

// does a combined set of `rows` rows and extents X, Y take the record pipeline?
bool fits(uint64_t rows, uint64_t X, uint64_t Y, uint64_t max_rows, uint64_t max_span) {
  if (rows >= (1ull << 30) || rows > max_rows) return false;
  if (X > max_span || Y > max_span) return false;
  if (Y >= (1ull << 35)) return false;
  // classify_device's own limits with len_x = X, len_y = Y
  if (X / 10 >= 0xFFFFFFF0ull || 2 * (X / 100 + 1) >= 0xFFFFFFF0ull ||
      2 * (Y / 100 + 1) >= 0xFFFFFFF0ull)
    return false;
  return true;
}

bool record_pipeline_on(const rk_ctx *ctx) {
  const char *e = std::getenv("RK_RECORD_PIPELINE");
  return ctx->pipeline == RK_PIPELINE_AUTO && !(e && e[0] == '0');
}

int ensure_state(rk_ctx *ctx, size_t dev_bytes, size_t host_bytes) {
  if (!ctx->batch) {
    ctx->batch = new (std::nothrow) BatchState;
    if (!ctx->batch) return RK_E_NOMEM;
    HIPCHK(ctx, hipEventCreate(&ctx->batch->ev0));
    HIPCHK(ctx, hipEventCreate(&ctx->batch->ev1));
  }
  BatchState *b = ctx->batch;
  if (dev_bytes > b->dev_cap) {
    if (b->dev) (void)hipFree(b->dev);
    b->dev = nullptr;
    b->dev_cap = 0;
    const hipError_t e = hipMalloc(&b->dev, dev_bytes);
    if (e != hipSuccess) {
      ctx->err = std::string("batch scratch hipMalloc(") + std::to_string(dev_bytes) +
                 "): " + hipGetErrorString(e);
      return e == hipErrorOutOfMemory ? RK_E_NOMEM : RK_E_HIP;
    }
    b->dev_cap = dev_bytes;
  }
  if (host_bytes > b->host_cap) {
    if (b->host) (void)hipHostFree(b->host);
    b->host = nullptr;
    b->host_cap = 0;
    HIPCHK(ctx, hipHostMalloc((void **)&b->host, host_bytes, hipHostMallocDefault));
    b->host_cap = host_bytes;
  }
  return RK_OK;
}

struct BatchCall {
  const rk_frags_soa *in;
  const rk_batch_params *p;
  rk_batch_result *out;
};

void name_set(rk_ctx *ctx, uint64_t k) {
  ctx->err = "set " + std::to_string(k) + ": " + ctx->err;
}

// sets [s0, s1) one by one through the single-set path
int classify_looped(rk_ctx *ctx, const BatchCall &c, uint32_t s0, uint32_t s1) {
  for (uint32_t k = s0; k < s1; ++k) {
    const uint64_t r0 = c.p->set_off[k], nk = c.p->set_off[k + 1] - r0;
    const rk_frags_soa sub{nk ? c.in->x_start + r0 : nullptr, nk ? c.in->y_start + r0 : nullptr,
                           nk ? c.in->length + r0 : nullptr, nk ? c.in->strand + r0 : nullptr, nk};
    const rk_params prm{c.p->len_x_hdr[k], c.p->len_y_hdr[k], c.p->len_ratio, c.p->pos_ratio};
    rk_result res{nk ? c.out->out_order + r0 : nullptr, nk ? c.out->gid + r0 : nullptr,
                  nk ? c.out->repval + r0 : nullptr, 0, 0};
    const int rc = rk_classify_device(ctx, &sub, &prm, &res);
    if (rc) {
      name_set(ctx, k);
      return rc;
    }
    c.out->n_out[k] = res.n_out;
    c.out->n_groups[k] = res.n_groups;
    ctx->batch_stats.device_ms += ctx->stats.device_ms;
    ++ctx->batch_stats.looped_sets;
  }
  return RK_OK;
}

// sets [s0, s1) (at least two, within fits()) as one combined set; *looped:
// the record pipeline cannot take it
int classify_combined(rk_ctx *ctx, const BatchCall &c, uint32_t s0, uint32_t s1,
                      const std::vector<SetGeom> &geom, bool *looped) {
  *looped = false;
  const uint32_t ns = s1 - s0;
  const uint64_t r0 = c.p->set_off[s0];
  const uint32_t n = (uint32_t)(c.p->set_off[s1] - r0);
  // device: translated rows, combined result, tables, words
  Carve probe{nullptr};
  auto carve = [&](Carve &cv, uint64_t *&ox, uint64_t *&oy, uint64_t *&ol, uint8_t *&os,
                   uint32_t *&cord, uint32_t *&cgid, uint8_t *&crep, char *&tab,
                   uint32_t *&words) {
    ox = cv.take<uint64_t>(n);
    oy = cv.take<uint64_t>(n);
    ol = cv.take<uint64_t>(n);
    os = cv.take<uint8_t>(n);
    cord = cv.take<uint32_t>(n);
    cgid = cv.take<uint32_t>(n);
    crep = cv.take<uint8_t>(n);
    tab = cv.take<char>((size_t)(ns + 1) * (3 * 8 + 5 * 4));
    words = cv.take<uint32_t>(BW_HEAD + (size_t)4 * (ns + 1));
  };
  uint64_t *ox, *oy, *ol;
  uint8_t *os, *crep;
  uint32_t *cord, *cgid, *words;
  char *tab;
  carve(probe, ox, oy, ol, os, cord, cgid, crep, tab, words);
  const size_t tab_bytes = (size_t)(ns + 1) * (3 * 8 + 5 * 4);
  const size_t back_words = BW_HEAD + (size_t)3 * ns;
  int rc = ensure_state(ctx, probe.off, tab_bytes > back_words * 4 ? tab_bytes : back_words * 4);
  if (rc) return rc;
  BatchState *bs = ctx->batch;
  Carve real{(char *)bs->dev};
  carve(real, ox, oy, ol, os, cord, cgid, crep, tab, words);

  // the tables, one upload: u64 bx, by, vsize; u32 roff, bkt_x, bkt_y, mi_x, mi_y
  const size_t e1 = ns + 1;
  uint64_t *h_bx = reinterpret_cast<uint64_t *>(bs->host), *h_by = h_bx + e1, *h_vs = h_by + e1;
  uint32_t *h_roff = reinterpret_cast<uint32_t *>(h_vs + e1), *h_kx = h_roff + e1,
           *h_ky = h_kx + e1, *h_mx = h_ky + e1, *h_my = h_mx + e1;
  uint64_t X = 0, Y = 0;
  for (uint32_t j = 0; j <= ns; ++j) {
    h_bx[j] = X;
    h_by[j] = Y;
    h_kx[j] = (uint32_t)(X / 100);
    h_ky[j] = (uint32_t)(Y / 100);
    h_roff[j] = (uint32_t)(c.p->set_off[s0 + j] - r0);
    const SetGeom &g = geom[s0 + (j < ns ? j : ns - 1)];
    h_vs[j] = j < ns ? g.vsize : 0;
    h_mx[j] = j < ns ? (uint32_t)g.mi_x : 0;
    h_my[j] = j < ns ? (uint32_t)g.mi_y : 0;
    if (j < ns) X += g.wx, Y += g.wy;
  }
  uint64_t *d_bx = reinterpret_cast<uint64_t *>(tab), *d_by = d_bx + e1, *d_vs = d_by + e1;
  uint32_t *d_roff = reinterpret_cast<uint32_t *>(d_vs + e1), *d_kx = d_roff + e1,
           *d_ky = d_kx + e1, *d_mx = d_ky + e1, *d_my = d_mx + e1;
  uint32_t *d_err = words + BW_HEAD, *d_kept = d_err + ns, *d_gbase = d_kept + ns,
           *d_start = d_gbase + ns;
  (void)d_err;

  hipStream_t st = ctx->stream;
  HIPCHK(ctx, hipEventRecord(bs->ev0, st));
  HIPCHK(ctx, hipMemcpyAsync(tab, bs->host, tab_bytes, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemsetAsync(words, 0, (BW_HEAD + (size_t)4 * (ns + 1)) * sizeof(uint32_t), st));
  const PackArgs pa{c.in->x_start + r0, c.in->y_start + r0, c.in->length + r0, c.in->strand + r0,
                    n, ns, d_roff, d_bx, d_by, d_vs, d_mx, d_my, ox, oy, ol, os, words};
  k_batch_pack<<<grid_for(n, 256, 4096), 256, 0, st>>>(pa);
  k_batch_scan<<<1, 1024, 0, st>>>(d_kept, ns, d_start);
  HIPCHK(ctx, hipGetLastError());
  // (the tables are uploaded: the pinned buffer is free for the words)
  if ((rc = readback(ctx, words, BW_HEAD))) return rc;
  if (ctx->host[BW_NOPACK]) {  // a row that fits no record: set by set
    *looped = true;
    return RK_OK;
  }
  if (ctx->host[BW_ERR]) {
    HIPCHK(ctx, hipMemcpyAsync(bs->host, words, back_words * sizeof(uint32_t),
                               hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const uint32_t *h_err = reinterpret_cast<const uint32_t *>(bs->host) + BW_HEAD;
    for (uint32_t j = 0; j < ns; ++j)
      if (h_err[j]) {
        rc = err_status(ctx, h_err[j]);
        name_set(ctx, s0 + j);
        return rc;
      }
    ctx->err = "batch: error flag without a set";
    return RK_E_INTERNAL;
  }

  // the combined set: headers X - 1, Y - 1 make its own last xStart/10 bucket
  // exactly X / 10, where the dropped rows were sent
  const rk_frags_soa cin{ox, oy, ol, os, n};
  const rk_params prm{X - 1, Y - 1, c.p->len_ratio, c.p->pos_ratio};
  rk_result res{cord, cgid, crep, 0, 0};
  const BatchTables bt{ns, d_kx, d_ky, d_mx, d_my};
  ctx->batch_tables = &bt;
  rc = rk_classify_device(ctx, &cin, &prm, &res);
  ctx->batch_tables = nullptr;
  if (rc) {
    ctx->err = "batch (sets " + std::to_string(s0) + ".." + std::to_string(s1 - 1) +
               " combined): " + ctx->err;
    return rc;
  }
  if (res.n_out && ctx->stats.pipeline != 1) {  // (the pack check above mirrors the pipeline's)
    *looped = true;
    return RK_OK;
  }
  const uint32_t m = (uint32_t)res.n_out;
  const SplitArgs sa{cord, cgid, crep, m, n, ns, d_roff, d_start,
                     c.out->out_order + r0, c.out->gid + r0, c.out->repval + r0, d_gbase, words};
  if (m) k_batch_split<<<grid_for(m, 256, 4096), 256, 0, st>>>(sa);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(bs->host, words, back_words * sizeof(uint32_t),
                             hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipEventRecord(bs->ev1, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  const uint32_t *hw = reinterpret_cast<const uint32_t *>(bs->host);
  const uint32_t *h_kept = hw + BW_HEAD + ns, *h_gbase = h_kept + ns;
  uint64_t total = 0;
  for (uint32_t j = 0; j < ns; ++j) total += h_kept[j];
  if (hw[BW_INTERNAL] || total != m) {
    ctx->err = "batch: the combined result does not split into the sets' ranges";
    return RK_E_INTERNAL;
  }
  // groups per set from consecutive bases and the total
  uint64_t next = res.n_groups;
  for (uint32_t j = ns; j-- > 0;) {
    c.out->n_out[s0 + j] = h_kept[j];
    if (h_kept[j]) {
      c.out->n_groups[s0 + j] = next - h_gbase[j];
      next = h_gbase[j];
    } else {
      c.out->n_groups[s0 + j] = 0;
    }
  }
  float ms = 0;
  HIPCHK(ctx, hipEventElapsedTime(&ms, bs->ev0, bs->ev1));
  ctx->batch_stats.device_ms += ms;
  ++ctx->batch_stats.sub_batches;
  ctx->batch_stats.batched_sets += ns;
  return RK_OK;
}

int check_args(rk_ctx *ctx, const rk_frags_soa *in, const rk_batch_params *p,
               const rk_batch_result *out, bool *empty) {
  *empty = false;
  if (!ctx || !in || !p || !out) return RK_E_ARG;
  ctx->err.clear();
  ctx->batch_stats = rk_batch_stats{};
  if (p->nsets == 0) {
    *empty = true;
    return RK_OK;
  }
  if (p->len_ratio <= 0 || p->pos_ratio <= 0) {  // NaN passes, as in the reference
    ctx->err = "ratios must be greater than zero (commonFunctions.cpp:26-27)";
    return RK_E_ARG;
  }
  if (!p->set_off || !p->len_x_hdr || !p->len_y_hdr || !out->n_out || !out->n_groups) {
    ctx->err = "batch: null per-set array";
    return RK_E_ARG;
  }
  for (uint32_t k = 0; k < p->nsets; ++k)
    if (p->set_off[k + 1] < p->set_off[k]) {
      ctx->err = "batch: set_off decreases at set " + std::to_string(k);
      return RK_E_ARG;
    }
  if (p->set_off[p->nsets] > in->n) {
    ctx->err = "batch: set_off ends past the rows";
    return RK_E_ARG;
  }
  if (p->set_off[p->nsets] > p->set_off[0] &&
      (!in->x_start || !in->y_start || !in->length || !in->strand || !out->out_order ||
       !out->gid || !out->repval)) {
    ctx->err = "batch: null row or result array with rows present";
    return RK_E_ARG;
  }
  return RK_OK;
}

int classify_batch_device(rk_ctx *ctx, const rk_frags_soa *in, const rk_batch_params *p,
                          rk_batch_result *out) {
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const BatchCall c{in, p, out};
  // read on every call: a test forces several sub-batches at tiny sizes
  const uint64_t max_rows = env_u64("RK_BATCH_MAX_ROWS", ~0ull);
  const uint64_t max_span = env_u64("RK_BATCH_MAX_SPAN", ~0ull);
  const bool record = record_pipeline_on(ctx);
  std::vector<SetGeom> geom(p->nsets);
  for (uint32_t k = 0; k < p->nsets; ++k) geom[k] = set_geom(p->len_x_hdr[k], p->len_y_hdr[k]);
  uint32_t s0 = 0;
  while (s0 < p->nsets) {
    // greedily, in order: the longest run of sets that fits one combined set
    uint32_t s1 = s0;
    uint64_t X = 0, Y = 0;
    while (s1 < p->nsets && geom[s1].ok &&
           fits(p->set_off[s1 + 1] - p->set_off[s0], X + geom[s1].wx, Y + geom[s1].wy, max_rows,
                max_span)) {
      X += geom[s1].wx;
      Y += geom[s1].wy;
      ++s1;
    }
    int rc;
    bool looped = true;
    if (s1 - s0 >= 2 && record && p->set_off[s1] > p->set_off[s0]) {
      if ((rc = classify_combined(ctx, c, s0, s1, geom, &looped))) return rc;
    } else if (s1 == s0) {
      s1 = s0 + 1;  // a set that fits no combined set goes alone
    }
    if (looped && (rc = classify_looped(ctx, c, s0, s1))) return rc;
    s0 = s1;
  }
  return RK_OK;
}

}  // namespace

void batch_nbd(const BatchTables &t, bool y_axis, const Csr &c, uint32_t m, uint32_t nb,
               hipStream_t st) {
  if (!m) return;
  k_batch_nbd<<<grid_for(m, 256, 4096), 256, 0, st>>>(c.key, c.pk, c.nbd, m, nb,
                                                      y_axis ? t.bkt_y : t.bkt_x,
                                                      y_axis ? t.mi_y : t.mi_x, t.nsets);
}

}  // namespace rk

extern "C" int rk_batch_layout(uint32_t nsets, const uint64_t *len_x_hdr,
                               const uint64_t *len_y_hdr, uint64_t *base_x, uint64_t *base_y) {
  if (!base_x || !base_y || (nsets && (!len_x_hdr || !len_y_hdr))) return RK_E_ARG;
  uint64_t X = 0, Y = 0;
  base_x[0] = base_y[0] = 0;
  for (uint32_t k = 0; k < nsets; ++k) {
    const rk::SetGeom g = rk::set_geom(len_x_hdr[k], len_y_hdr[k]);
    if (!g.ok || __builtin_add_overflow(X, g.wx, &X) || __builtin_add_overflow(Y, g.wy, &Y))
      return RK_E_ARG;
    base_x[k + 1] = X;
    base_y[k + 1] = Y;
  }
  return RK_OK;
}

extern "C" int rk_get_batch_stats(const rk_ctx *ctx, rk_batch_stats *st) {
  if (!ctx || !st) return RK_E_ARG;
  *st = ctx->batch_stats;
  return RK_OK;
}

extern "C" int rk_classify_device_batch(rk_ctx *ctx, const rk_frags_soa *in_dev,
                                        const rk_batch_params *p, rk_batch_result *out) {
  bool empty = false;
  int rc = rk::check_args(ctx, in_dev, p, out, &empty);
  if (rc || empty) return rc;
  try {
    rc = rk::classify_batch_device(ctx, in_dev, p, out);
  } catch (...) {
    ctx->err = "unexpected C++ exception";
    rc = RK_E_INTERNAL;
  }
  ctx->batch_tables = nullptr;
  return rc;
}

// Host rows in, host results out: the plain SoA goes up (25 B per row), the
// result arrays come down whole (entries past a set's n_out are zero).
extern "C" int rk_classify_batch(rk_ctx *ctx, const rk_frags_soa *in, const rk_batch_params *p,
                                 rk_batch_result *out) {
  bool empty = false;
  int rc = rk::check_args(ctx, in, p, out, &empty);
  if (rc || empty) return rc;
  const size_t n = p->set_off[p->nsets];
  if (n >= 0xFFFFFFFFull) return RK_E_TOO_MANY;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t need = rk::align_up(n * 8 + 16) * 3 + rk::align_up(n + 16) * 2 +
                      rk::align_up(n * 4 + 16) * 2;
  if (need > ctx->io_cap) {
    if (ctx->io) (void)hipFree(ctx->io);
    ctx->io = nullptr;
    ctx->io_cap = 0;
    HIPCHK(ctx, hipMalloc(&ctx->io, need));
    ctx->io_cap = need;
  }
  rk::Carve c{(char *)ctx->io};
  uint64_t *dx = c.take<uint64_t>(n), *dy = c.take<uint64_t>(n), *dl = c.take<uint64_t>(n);
  uint8_t *ds = c.take<uint8_t>(n), *drep = c.take<uint8_t>(n);
  uint32_t *dgid = c.take<uint32_t>(n), *dord = c.take<uint32_t>(n);
  if (n) {
    rc = rk::io_h2d(ctx, {{(void *)in->x_start, dx, n * 8},
                          {(void *)in->y_start, dy, n * 8},
                          {(void *)in->length, dl, n * 8},
                          {(void *)in->strand, ds, n}});
    if (rc) return rc;
    HIPCHK(ctx, hipMemsetAsync(drep, 0, n, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(dgid, 0, n * 4, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(dord, 0, n * 4, ctx->stream));
  }
  const rk_frags_soa din{dx, dy, dl, ds, n};
  rk_batch_result dres{dord, dgid, drep, out->n_out, out->n_groups};
  try {
    rc = rk::classify_batch_device(ctx, &din, p, &dres);
  } catch (...) {
    ctx->err = "unexpected C++ exception";
    rc = RK_E_INTERNAL;
  }
  ctx->batch_tables = nullptr;
  if (rc) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (n)
    rc = rk::io_d2h(ctx, {{out->out_order, dord, n * 4}, {out->gid, dgid, n * 4},
                          {out->repval, drep, n}});
  return rc;
}
