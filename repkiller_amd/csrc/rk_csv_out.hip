// rk_csv_out.hip -- device egress: the result CSV formatted on the GPU
// (rk_db_write_csv_device), beside the host writer of rk_host.cpp.
//
// save_all_frag_pairs (commonFunctions.cpp:101-146) echoes the header and
// writes one line per member in output order.  Here the header is written by
// the host, and the body is formatted from the nine columns a database loaded
// with RK_DB_KEEP_ROWS keeps in HBM, in chunks of RK_CSV_OUT_ROWS output rows.
// Per chunk:
//   1. length pass: one lane per output row k gathers input row out_order[k]
//      and runs csv_row (rk_csv_row.h) for the length alone: a length byte, a
//      ROW_HOST flag, the block's byte total; the chunk's host-row count, byte
//      total and error bits come back in one readback;
//   2. host fix-up (only when rows are ROW_HOST: a float the device does not
//      print exactly): the rows are listed, formatted by the host's own
//      rk::db_format_row, uploaded packed, and a small kernel patches their
//      lengths in;
//   3. scan of the block totals to chunk-local u32 offsets (rk_csv_scan.h);
//   4. put pass: a 128-row block formats its rows into LDS at their block-local
//      offsets (host rows are copied from the patch bytes), then copies its
//      contiguous byte range to the chunk's text buffer, consecutive lanes on
//      consecutive 16-B words; the unaligned head and tail go byte-wise.
// Two context-owned text buffers alternate: chunk c + 1 is formatted on
// ctx->stream while chunk c comes down on the copy stream through the pinned
// staging slots, each of which is pwritten from where the DMA left it
// (rk::io_d2h_sink).  Scratch comes from ctx->ws; uploaded result arrays from
// ctx->io.
//
// One driver (write_chunks) runs this loop for both routes.  FileRoute: the
// n_out output rows, pwritten behind the header of one file.  SetRoute, a batch
// of sets (rk_dbset_write_csv_device): the slots of an rk_batch_result.
// k_outb_len takes the place of the length pass (it finds each slot's set, turns
// a used slot into its combined row, gives an unused one length 0), the other
// passes run unchanged on the combined rows, and k_outb_cuts gives the text
// offset at which every set of the chunk starts.  The writers split each pinned
// slot at those cuts and pwrite every piece into its own set's file (SetFiles).
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdlib>
#include <mutex>
#include <new>

#include "rk_csv_row.h"
#include "rk_csv_scan.h"
#include "rk_ctx.h"
#include "rk_db.h"

namespace {

// rows of a block.  The put pass holds a block's text in LDS, worst case
// ROW_MAX bytes per row: 128 rows are 32 KB, five blocks per CU (DESIGN.md,
// "Device egress")
constexpr uint32_t OB = 128;
constexpr uint32_t LDS_TEXT = OB * rk::ROW_MAX + 16;
constexpr uint32_t DEFAULT_ROWS = 1u << 22;
constexpr uint32_t MAX_ROWS = 1u << 24;  // x ROW_MAX < 2^32: chunk-local offsets are u32
static_assert((uint64_t)MAX_ROWS * rk::ROW_MAX < (1ull << 32), "chunk text offsets are u32");

enum : uint32_t { OERR_ORDER = 1, OERR_BOUNDS = 2 };

struct OCols {
  const uint64_t *xs, *ys, *xe, *ye, *len, *score, *ident;
  const float *sim;
  const uint8_t *strand;
};

// a result's arrays: device memory in the kernels, which only read them; not
// const, since carve_result's callers fill them; host memory only as the source
// of upload_result
struct Res {
  uint32_t *order, *gid;
  uint8_t *rep;
};

// counters of a chunk
struct Ctr {
  unsigned long long host_rows, bytes, slot;
  uint32_t err, pad;
};

__device__ inline rk::OutRow gather(const OCols &c, uint32_t i) {
  rk::OutRow r;
  r.xs = c.xs[i], r.ys = c.ys[i], r.xe = c.xe[i], r.ye = c.ye[i];
  r.len = c.len[i], r.score = c.score[i], r.ident = c.ident[i];
  r.sim = c.sim[i], r.strand = c.strand[i];
  return r;
}

// The two length kernels share their body.  row_len: the text length of input
// row i as output row k of the chunk's slice r; a ROW_HOST row has length 0 until
// the fix-up patches it.
__device__ __forceinline__ uint32_t row_len(const OCols &c, uint32_t i, const Res &r, uint32_t k,
                                            bool *host) {
  const rk::OutRow row = gather(c, i);
  uint32_t len = 0;
  *host = rk::csv_row(row, r.gid[k], r.rep[k], nullptr, &len) == rk::ROW_HOST;
  return *host ? 0 : len;
}

// len_tail: row k's length byte and ROW_HOST flag, the block's byte total, and
// the block's share of the chunk's counters (every thread of the block calls it)
__device__ __forceinline__ void len_tail(uint32_t k, uint32_t cnt, uint32_t len, bool host,
                                         uint8_t *len8, uint8_t *hst, uint32_t *blk_tot,
                                         Ctr *ctr) {
  __shared__ uint32_t lds[OB];
  if (k < cnt) {
    len8[k] = (uint8_t)len;
    hst[k] = host ? 1 : 0;
  }
  uint32_t total;
  (void)rk::block_excl_scan<OB>(len, lds, &total);
  const int nh = __syncthreads_count(host);
  if (threadIdx.x == 0) {
    blk_tot[blockIdx.x] = total;
    if (total) atomicAdd(&ctr->bytes, (unsigned long long)total);
    if (nh) atomicAdd(&ctr->host_rows, (unsigned long long)nh);
  }
}

// rows [0, cnt) of the chunk (r is the chunk's slice of the result arrays)
__global__ __launch_bounds__(OB) void k_out_len(OCols c, uint64_t n, Res r, uint32_t cnt,
                                               uint8_t *len8, uint8_t *hst, uint32_t *blk_tot,
                                               Ctr *ctr) {
  const uint32_t k = blockIdx.x * OB + threadIdx.x;
  uint32_t len = 0;
  bool host = false;
  if (k < cnt) {
    const uint32_t i = r.order[k];
    if (i >= n) atomicOr(&ctr->err, OERR_ORDER);
    else len = row_len(c, i, r, k, &host);
  }
  len_tail(k, cnt, len, host, len8, hst, blk_tot, ctr);
}

// ---- a batch of sets (rk_dbset_write_csv_device): the result is in
// rk_batch_result layout, set s owning slots [off[s], off[s] + n_out[s]) with
// out_order local to the set; the slots up to off[s + 1] are unused (the rows
// of the set's dropped last xStart/10 bucket)
struct SetTab {
  const uint64_t *off;    // nsets + 1
  const uint64_t *n_out;  // nsets
  uint32_t ns;
};

// the set of slot p < off[ns]: the last s with off[s] <= p (an empty set shares
// its offset with the next one and is never the answer); lo: a set known to
// start at or before p
__device__ inline uint32_t set_of(const SetTab &s, uint32_t lo, uint64_t p) {
  uint32_t hi = s.ns;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (s.off[mid] <= p) lo = mid;
    else hi = mid;
  }
  return lo;
}

// k_out_len for slots [k0, k0 + cnt) of a batch (r is the chunk's slice of the
// result arrays).  A used slot becomes the combined row off[s] + out_order[p],
// kept in crow[] for the passes that follow (k_out_hostlist, k_out_put take it
// as their order array); an unused slot has length 0.  The wave's first slot is
// searched at a wave-uniform address; a lane searches on only when its slot
// lies past that set's end.
__global__ __launch_bounds__(OB) void k_outb_len(OCols c, SetTab s, Res r, uint64_t k0,
                                                uint32_t cnt, uint32_t *crow, uint8_t *len8,
                                                uint8_t *hst, uint32_t *blk_tot, Ctr *ctr) {
  const uint32_t k = blockIdx.x * OB + threadIdx.x;
  uint32_t len = 0;
  bool host = false;
  if (k < cnt) {
    const uint64_t p = k0 + k;
    uint32_t set = set_of(s, 0, k0 + (k & ~63u));
    if (p >= s.off[set + 1]) set = set_of(s, set, p);
    const uint64_t base = s.off[set], local = p - base;
    uint32_t i = 0;
    if (local < s.n_out[set]) {
      const uint64_t o = r.order[k];
      if (o >= s.off[set + 1] - base) {
        atomicOr(&ctr->err, OERR_ORDER);
      } else {
        i = (uint32_t)(base + o);
        len = row_len(c, i, r, k, &host);
      }
    }
    crow[k] = i;
  }
  len_tail(k, cnt, len, host, len8, hst, blk_tot, ctr);
}

// cuts[j] = chunk-local text offset of the first slot of set ks + j, for the m
// sets whose slots start in the chunk (or at its end, for the last chunk's
// trailing empty sets): its block's offset plus the lengths before the slot in
// its 128-row block.  One lane per set; the host splits the text at the cuts.
__global__ __launch_bounds__(OB) void k_outb_cuts(const uint64_t *off, uint32_t ks, uint32_t m,
                                                 uint64_t k0, uint32_t cnt, const uint8_t *len8,
                                                 const uint32_t *blk_off, uint32_t *cuts) {
  const uint32_t j = blockIdx.x * OB + threadIdx.x;
  if (j >= m) return;
  const uint64_t q = off[ks + j] - k0;
  const uint32_t p = q < cnt ? (uint32_t)q : cnt;  // (blk_off has the chunk's total at its end)
  uint32_t at = blk_off[p / OB];
  for (uint32_t i = p - p % OB; i < p; ++i) at += len8[i];
  cuts[j] = at;
}

// the ROW_HOST rows as (k, i, gid, rep); any order, cap entries at most
__global__ __launch_bounds__(OB) void k_out_hostlist(const uint8_t *hst, Res r, uint32_t cnt,
                                                    Ctr *ctr, uint32_t cap, uint32_t *list) {
  const uint32_t k = blockIdx.x * OB + threadIdx.x;
  if (k >= cnt || !hst[k]) return;
  const unsigned long long e = atomicAdd(&ctr->slot, 1ull);
  if (e >= cap) return;
  list[4 * e] = k, list[4 * e + 1] = r.order[k], list[4 * e + 2] = r.gid[k];
  list[4 * e + 3] = r.rep[k];
}

// host row e is row pk[e] of the chunk, its bytes [pofs[e], pofs[e + 1]) of the patch text
__global__ __launch_bounds__(OB) void k_out_patch(const uint32_t *pk, const uint32_t *pofs,
                                                 uint32_t nhost, uint32_t cnt, uint8_t *len8,
                                                 uint32_t *poff, uint32_t *blk_tot) {
  const uint32_t e = blockIdx.x * OB + threadIdx.x;
  if (e >= nhost) return;
  const uint32_t k = pk[e];
  if (k >= cnt) return;
  const uint32_t len = pofs[e + 1] - pofs[e];
  len8[k] = (uint8_t)len;
  poff[k] = pofs[e];
  atomicAdd(&blk_tot[k / OB], len);
}

// The block's text is laid out in LDS from byte (base & 15) on, so an LDS
// 16-B word and the global word it goes to share their alignment.
__global__ __launch_bounds__(OB) void k_out_put(OCols c, Res r, uint32_t cnt, const uint8_t *len8,
                                               const uint8_t *hst, const uint32_t *poff,
                                               const char *ptext, const uint32_t *blk_off,
                                               char *txt, uint64_t cap, uint32_t *perr) {
  __shared__ __attribute__((aligned(16))) char buf[LDS_TEXT];
  __shared__ uint32_t lds[OB];
  const uint32_t t = threadIdx.x, k = blockIdx.x * OB + t;
  const bool live = k < cnt;
  const uint32_t len = live ? len8[k] : 0u;
  uint32_t total;
  const uint32_t excl = rk::block_excl_scan<OB>(len, lds, &total);
  const uint32_t base = blk_off[blockIdx.x], skew = base & 15u;
  // (a block's lengths sum to at most OB * 255 on a damaged length array: the
  // LDS image and the text buffer are both guarded)
  if (total > OB * rk::ROW_MAX || (uint64_t)base + total > cap) {
    if (t == 0) atomicOr(perr, OERR_BOUNDS);
    return;
  }
  if (live && len) {
    char *o = buf + skew + excl;
    if (hst[k]) {
      const char *p = ptext + poff[k];
      for (uint32_t j = 0; j < len; ++j) o[j] = p[j];
    } else {
      const rk::OutRow row = gather(c, r.order[k]);
      uint32_t l2;
      (void)rk::csv_row(row, r.gid[k], r.rep[k], o, &l2);
    }
  }
  __syncthreads();
  char *dst = txt + base;  // txt is 16-B aligned: dst + j is aligned where skew + j is
  const uint32_t head = min(total, (16u - skew) & 15u);
  for (uint32_t j = t; j < head; j += OB) dst[j] = buf[skew + j];
  const uint32_t nvec = (total - head) / 16u;
  const uint4 *src4 = reinterpret_cast<const uint4 *>(buf + skew + head);
  uint4 *dst4 = reinterpret_cast<uint4 *>(dst + head);
  for (uint32_t v = t; v < nvec; v += OB) dst4[v] = src4[v];
  for (uint32_t j = head + nvec * 16u + t; j < total; j += OB) dst[j] = buf[skew + j];
}

// ------------------------------------------------------------------ host --

struct Events {
  hipEvent_t e[6] = {};
  ~Events() {
    for (auto &x : e)
      if (x) (void)hipEventDestroy(x);
  }
};

// device buffers of one chunk's host fix-up; they live until the chunk's put
// pass has run
struct Patch {
  void *pk = nullptr, *pofs = nullptr, *text = nullptr;
  void release() {
    for (void **p : {&pk, &pofs, &text}) {
      if (*p) (void)hipFree(*p);
      *p = nullptr;
    }
  }
  ~Patch() { release(); }
};

struct FdCloser {
  int fd;
  ~FdCloser() {
    if (fd >= 0) ::close(fd);
  }
};

uint32_t chunk_rows() {
  const char *e = std::getenv("RK_CSV_OUT_ROWS");
  if (e && *e) {
    char *end = nullptr;
    const unsigned long long v = std::strtoull(e, &end, 10);
    if (end != e) return (uint32_t)std::min<unsigned long long>(std::max(v, 1ull), MAX_ROWS);
  }
  return DEFAULT_ROWS;
}

bool pwrite_all(int fd, const char *p, size_t len, uint64_t at) {
  while (len) {
    const ssize_t w = ::pwrite(fd, p, len, (off_t)at);
    if (w <= 0) {
      if (w < 0 && errno == EINTR) continue;
      return false;
    }
    p += w, len -= (size_t)w, at += (uint64_t)w;
  }
  return true;
}

struct Chunk {
  uint32_t cnt = 0;
  uint64_t bytes = 0;
  uint32_t ks = 0, m = 0;  // a batch: the sets ks .. ks + m - 1 start in the chunk
};

struct Save {
  rk_ctx *ctx;
  const rk_db *db;
  OCols cols;
  uint64_t n;
  Res res;  // device arrays, n_out entries
  rk_egress_stats *st;
  Events ev;  // 0,1: the synchronous passes; 2,3 / 4,5: the put pass of an even / odd chunk
  Patch patch[2];
  // scratch of a chunk (ctx->ws), carved for R rows
  uint8_t *len8, *hst;
  uint32_t *poff, *blk_tot, *blk_off;
  Ctr *ctr;
  uint32_t *perr;  // the put passes' error bits: cleared once, read once at the end

  void carve(rk::Carve &c, uint32_t R) {
    const uint32_t nb = (R + OB - 1) / OB;
    len8 = c.take<uint8_t>(R), hst = c.take<uint8_t>(R), poff = c.take<uint32_t>(R);
    blk_tot = c.take<uint32_t>(nb), blk_off = c.take<uint32_t>(nb + 1);
    ctr = c.take<Ctr>(1), perr = c.take<uint32_t>(1);
  }
  // the result entries of the chunk that starts at k0
  Res slice(uint64_t k0) const { return Res{res.order + k0, res.gid + k0, res.rep + k0}; }

  // host rows of the chunk's cnt rows r: list, format, upload, patch the lengths
  int fix_up(const Res &r, uint32_t cnt, uint32_t nhost, int par, uint64_t *added) {
    hipStream_t s = ctx->stream;
    const uint32_t nb = (cnt + OB - 1) / OB;
    Patch &p = patch[par];
    p.release();
    void *list = nullptr;
    int rc;
    if ((rc = rk::dev_alloc(ctx, &list, (size_t)nhost * 16, "csv host rows"))) return rc;
    struct Free {
      void *p;
      ~Free() { (void)hipFree(p); }
    } free_list{list};
    k_out_hostlist<<<nb, OB, 0, s>>>(hst, r, cnt, ctr, nhost, (uint32_t *)list);
    std::vector<uint32_t> hl((size_t)nhost * 4);
    HIPCHK(ctx, hipMemcpyAsync(hl.data(), list, (size_t)nhost * 16, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    // (a database whose lengths are all zero sends every row here: the list is
    // formatted by up to 16 threads, each into a text of its own)
    const unsigned nt = nhost < (1u << 14)
                            ? 1u
                            : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<std::vector<char>> part(nt);
    std::vector<uint32_t> pk(nhost), pofs((size_t)nhost + 1);
    std::atomic<bool> outside{false};
    const uint64_t n_rows = n;
    auto format = [&](unsigned w) {
      const uint32_t e0 = (uint32_t)((uint64_t)nhost * w / nt);
      const uint32_t e1 = (uint32_t)((uint64_t)nhost * (w + 1) / nt);
      std::vector<char> &out = part[w];
      out.reserve((size_t)(e1 - e0) * 96);
      char row[256];
      for (uint32_t e = e0; e < e1; ++e) {
        const uint32_t k = hl[4 * (size_t)e], i = hl[4 * (size_t)e + 1];
        pk[e] = k;
        pofs[e + 1] = 0;
        if (k >= cnt || i >= n_rows) {
          outside = true;
          continue;
        }
        const char *end = rk::db_format_row(db, i, hl[4 * (size_t)e + 2], hl[4 * (size_t)e + 3], row);
        pofs[e + 1] = (uint32_t)(end - row);  // the length, for now
        out.insert(out.end(), (const char *)row, end);
      }
    };
    {
      std::vector<std::thread> th;
      for (unsigned w = 1; w < nt; ++w) {
        try {
          th.emplace_back(format, w);
        } catch (...) {  // no thread to be had: this one takes the share
          format(w);
        }
      }
      format(0);
      for (auto &x : th) x.join();
    }
    if (outside) {
      ctx->err = "csv host rows: entry outside the chunk";
      return RK_E_INTERNAL;
    }
    pofs[0] = 0;
    for (uint32_t e = 0; e < nhost; ++e) pofs[e + 1] += pofs[e];
    const uint64_t tbytes = pofs[nhost];
    std::vector<char> text;
    text.reserve(tbytes);
    for (auto &v : part) text.insert(text.end(), v.begin(), v.end());
    if (text.size() != tbytes) {
      ctx->err = "csv host rows: packed text and offsets disagree";
      return RK_E_INTERNAL;
    }
    if ((rc = rk::dev_alloc(ctx, &p.pk, (size_t)nhost * 4, "csv host rows"))) return rc;
    if ((rc = rk::dev_alloc(ctx, &p.pofs, ((size_t)nhost + 1) * 4, "csv host rows"))) return rc;
    if ((rc = rk::dev_alloc(ctx, &p.text, tbytes, "csv host rows"))) return rc;
    if ((rc = rk::io_h2d(ctx, {{pk.data(), p.pk, (size_t)nhost * 4},
                               {pofs.data(), p.pofs, ((size_t)nhost + 1) * 4},
                               {text.data(), p.text, (size_t)tbytes}})))
      return rc;
    k_out_patch<<<(nhost + OB - 1) / OB, OB, 0, s>>>((const uint32_t *)p.pk,
                                                     (const uint32_t *)p.pofs, nhost, cnt, len8,
                                                     poff, blk_tot);
    *added = tbytes;
    return RK_OK;
  }

  // passes 1-4 of chunk c = rows [k0, k0 + cnt); returns with the put pass queued.
  // The route launches its length pass and names the rows the other passes read;
  // after the scan it may queue work of its own (a batch: the sets' cuts).
  template <class Route>
  int format_chunk(Route &rt, uint64_t c, uint64_t k0, uint32_t cnt, Chunk *out) {
    hipStream_t s = ctx->stream;
    const int par = (int)(c & 1);
    const uint32_t nb = (cnt + OB - 1) / OB;
    HIPCHK(ctx, hipEventRecord(ev.e[0], s));
    HIPCHK(ctx, hipMemsetAsync(ctr, 0, sizeof(Ctr), s));
    const Res r = rt.len_pass(*this, k0, cnt, nb);
    HIPCHK(ctx, hipMemcpyAsync(ctx->host, ctr, sizeof(Ctr), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipEventRecord(ev.e[1], s));
    HIPCHK(ctx, hipEventSynchronize(ev.e[1]));
    float ms = 0;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    st->device_ms += ms;
    HIPCHK(ctx, hipGetLastError());
    Ctr got;
    std::memcpy(&got, ctx->host, sizeof got);
    if (got.err & OERR_ORDER) return RK_E_ARG;  // an out_order entry >= n, as the host route
    if (got.host_rows > cnt || got.bytes > (uint64_t)cnt * rk::ROW_MAX) {
      ctx->err = "csv length pass: counts exceed the chunk";
      return RK_E_INTERNAL;
    }
    uint64_t bytes = got.bytes;
    if (got.host_rows) {
      const double t = rk::wall_ms();
      uint64_t added = 0;
      const int rc = fix_up(r, cnt, (uint32_t)got.host_rows, par, &added);
      if (rc) return rc;
      bytes += added;
      st->host_rows += got.host_rows;
      st->host_fix_ms += rk::wall_ms() - t;
    }
    int rc = rk::grow(ctx, &ctx->txt[par], &ctx->txt_cap[par], rk::align_up(bytes + 16),
                      "csv text");
    if (rc) return rc;
    HIPCHK(ctx, hipEventRecord(ev.e[2 + 2 * par], s));
    rk::k_csv_scan<uint32_t><<<1, 1024, 0, s>>>(blk_tot, nb, blk_off);
    if ((rc = rt.after_scan(*this, par, k0, cnt, out))) return rc;
    k_out_put<<<nb, OB, 0, s>>>(cols, r, cnt, len8, hst, poff, (const char *)patch[par].text,
                                blk_off, (char *)ctx->txt[par], bytes, perr);
    HIPCHK(ctx, hipEventRecord(ev.e[3 + 2 * par], s));
    HIPCHK(ctx, hipGetLastError());
    out->cnt = cnt;
    out->bytes = bytes;
    return RK_OK;
  }
};

// n entries of a result (u32 order, u32 gid, u8 rep) in one of the context's
// grow-only buffers
int carve_result(rk_ctx *ctx, void **buf, size_t *cap, size_t n, const char *what, Res *out) {
  rk::Carve pc{nullptr};
  pc.take<uint32_t>(n), pc.take<uint32_t>(n), pc.take<uint8_t>(n);
  const int rc = rk::grow(ctx, buf, cap, pc.off, what);
  if (rc) return rc;
  rk::Carve c{(char *)*buf};
  out->order = c.take<uint32_t>(n), out->gid = c.take<uint32_t>(n), out->rep = c.take<uint8_t>(n);
  return RK_OK;
}

// the n entries of a host result uploaded to ctx->io
int upload_result(rk_ctx *ctx, const Res &host, size_t n, Res *dev) {
  const double t = rk::wall_ms();
  int rc = carve_result(ctx, &ctx->io, &ctx->io_cap, n, "result upload", dev);
  if (rc) return rc;
  if ((rc = rk::io_h2d(ctx, {{host.order, dev->order, n * 4},
                             {host.gid, dev->gid, n * 4},
                             {host.rep, dev->rep, n}})))
    return rc;
  ctx->egress.upload_ms = rk::wall_ms() - t;
  return RK_OK;
}

// The chunk driver of both routes.  in: the result's `entries` entries, device
// arrays with RK_RES_DEVICE, host arrays otherwise.  The route (FileRoute,
// SetRoute) has: open, the checks and files before any device work (*work: there
// is text to format); total, the rows or slots the chunks are cut over; set_up,
// its own state behind the driver's in ctx->ws, called twice as a Carve is
// (sizes first; then pointers, pinned memory and uploads); len_pass and
// after_scan (format_chunk); begin_chunk, sink, end_chunk around a chunk's way
// down; stop, a file failed; done, after the last chunk alone, which finish
// cannot tell from a failure; finish, the call's code.
template <class Route>
int write_chunks(rk_ctx *ctx, const rk_db *db, Route &rt, const Res &in, uint64_t entries,
                 uint32_t flags) {
  const double t0 = rk::wall_ms();
  rk_egress_stats &st = ctx->egress;
  st = rk_egress_stats{};
  bool work = false;
  int rc = rt.open(ctx, &work);
  if (rc) return rc;
  auto finish = [&](int code) {
    code = rt.finish(ctx, code);
    st.total_ms = rk::wall_ms() - t0;
    return code;
  };
  if (!work) return finish(RK_OK);

  HIPCHK(ctx, hipSetDevice(ctx->device));
  Save S{ctx, db};
  S.cols = OCols{db->dev_x,     db->dev_y,     db->dev_xe,  db->dev_ye,    db->dev_len,
                 db->dev_score, db->dev_ident, db->dev_sim, db->dev_strand};
  S.n = db->x_start.size();
  S.st = &st;
  for (auto &e : S.ev.e) HIPCHK(ctx, hipEventCreate(&e));
  S.res = in;
  if (!(flags & RK_RES_DEVICE) && (rc = upload_result(ctx, in, entries, &S.res))) return rc;
  const uint64_t total = rt.total;
  const uint32_t R = (uint32_t)std::min<uint64_t>(chunk_rows(), total);
  rk::Carve ps{nullptr};
  S.carve(ps, R), (void)rt.set_up(ctx, ps, R);
  if ((rc = rk::grow(ctx, &ctx->ws, &ctx->ws_cap, ps.off, "csv rows out"))) return rc;
  rk::Carve cs{(char *)ctx->ws};
  S.carve(cs, R);
  if ((rc = rt.set_up(ctx, cs, R))) return rc;

  hipStream_t s = ctx->stream;
  HIPCHK(ctx, hipMemsetAsync(S.perr, 0, 4, s));
  const uint64_t nchunks = (total + R - 1) / R;
  auto rows_of = [&](uint64_t c) { return (uint32_t)std::min<uint64_t>(R, total - c * R); };
  // on any failure below the stream is drained before the patch buffers go
  auto fail = [&](int code) {
    (void)hipStreamSynchronize(s);
    return finish(code);
  };
  Chunk cur, next;
  if ((rc = S.format_chunk(rt, 0, 0, rows_of(0), &cur))) return fail(rc);
  for (uint64_t c = 0; c < nchunks; ++c) {
    const int par = (int)(c & 1);
    // chunk c + 1 is formatted (the other text buffer) before chunk c's
    // download starts to wait: its put pass runs beside the copies and writes
    if (c + 1 < nchunks &&
        (rc = S.format_chunk(rt, c + 1, (c + 1) * R, rows_of(c + 1), &next)))
      return fail(rc);
    const double t = rk::wall_ms();
    hipEvent_t put = S.ev.e[3 + 2 * par];
    if ((rc = rt.begin_chunk(ctx, c * R, cur, par, put))) return fail(rc);
    rc = rk::io_d2h_sink(ctx, ctx->txt[par], (size_t)cur.bytes, put,
                         [&](const char *p, size_t len, size_t o) { return rt.sink(p, len, o); });
    rt.end_chunk(cur, rc, &st);
    st.d2h_write_ms += rk::wall_ms() - t;
    if (rc != 1 && rc) return fail(rc);  // (1: a sink call failed; the route knows)
    // the put pass of chunk c is complete (the copy stream waited for it)
    float ms = 0;
    HIPCHK(ctx, hipEventElapsedTime(&ms, S.ev.e[2 + 2 * par], put));
    st.device_ms += ms;
    S.patch[par].release();
    st.bytes += cur.bytes;
    ++st.chunks;
    cur = next;
    if (rt.stop()) return fail(RK_OK);
  }
  rt.done(&st);
  HIPCHK(ctx, hipMemcpyAsync(ctx->host, S.perr, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  if (*ctx->host) {  // (the put pass' own error word, not a control block's)
    ctx->err = "csv put pass: a block's text does not fit its place";
    return finish(RK_E_INTERNAL);
  }
  return finish(RK_OK);
}

// One file: the rows' text follows the header.
struct FileRoute {
  const rk_db *db;
  const char *path;
  uint64_t total;  // n_out
  FdCloser f{-1};
  uint64_t at = 0;  // the file offset of the chunk's text
  bool ok = true;

  int open(rk_ctx *, bool *work) {
    // the file first, as the host route: an open failure does nothing else
    f.fd = ::open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (f.fd < 0) return RK_E_IO;
    if (total > 0xFFFFFFFFull || (total && db->x_start.empty())) return RK_E_ARG;
    ok = pwrite_all(f.fd, db->header.data(), db->header.size(), 0);
    at = db->header.size();
    *work = total && ok;
    return RK_OK;
  }
  int set_up(rk_ctx *, rk::Carve &, uint32_t) { return RK_OK; }
  Res len_pass(Save &S, uint64_t k0, uint32_t cnt, uint32_t nb) {
    const Res r = S.slice(k0);
    k_out_len<<<nb, OB, 0, S.ctx->stream>>>(S.cols, S.n, r, cnt, S.len8, S.hst, S.blk_tot, S.ctr);
    return r;
  }
  int after_scan(Save &, int, uint64_t, uint32_t, Chunk *) { return RK_OK; }
  int begin_chunk(rk_ctx *, uint64_t, const Chunk &, int, hipEvent_t) { return RK_OK; }
  bool sink(const char *p, size_t len, size_t off) { return pwrite_all(f.fd, p, len, at + off); }
  void end_chunk(const Chunk &c, int rc, rk_egress_stats *st) {
    if (rc == 1) ok = false;  // a pwrite failed
    else if (rc) return;
    at += c.bytes;
    st->rows += c.cnt;
  }
  bool stop() const { return !ok; }
  void done(rk_egress_stats *) {}
  int finish(rk_ctx *, int rc) {
    const int fd = f.fd;
    f.fd = -1;
    if (::close(fd) != 0) ok = false;
    return rc ? rc : ok ? RK_OK : RK_E_IO;
  }
};

int write_device(rk_ctx *ctx, const rk_db *db, const char *path, const rk_result *res,
                 uint32_t flags) {
  FileRoute rt{db, path, res->n_out};
  return write_chunks(ctx, db, rt, Res{res->out_order, res->gid, res->repval}, res->n_out, flags);
}

int check_args(rk_ctx *ctx, const rk_db *db, const char *what) {
  if (!db->dev_rows) {
    ctx->err = std::string(what) + ": the database was not loaded with RK_DB_KEEP_ROWS";
    return RK_E_ARG;
  }
  if (db->dev_device != ctx->device) {
    ctx->err = std::string(what) + ": the database's columns are on another device";
    return RK_E_ARG;
  }
  return RK_OK;
}

// ---- a batch of sets: one text stream, split into the sets' files ----------

// A set's part of a chunk's text: bytes [t0, t1) go to its file at base + (x - t0).
struct Seg {
  uint32_t set;
  uint64_t t0, t1, base;
  int fd;
  uint64_t left;  // bytes of [t0, t1) not yet written
  bool ends;      // the set's last slot lies in this chunk: close when left is 0
};

// The output files of a batch.  The writers of io_d2h_sink split every pinned
// slot at the chunk's cuts and pwrite each piece at its file's offset (header
// length plus the bytes earlier chunks wrote for the set).  A file is opened
// by the first writer that reaches it, which also writes its header, and
// closed by the one that writes its last byte, so the descriptors open at once
// are bounded by the slots in flight, not by the sets.  A path that cannot be
// opened does not stop the others: the lowest such set is kept in `bad`, sets
// from it on are skipped, and every lower-numbered file is complete when the
// chunk is.
struct SetFiles {
  const rk_dbset *dbs;
  const char *const *paths;
  std::mutex mu[32];      // segment i's descriptor and byte count: mu[i % 32]
  std::vector<Seg> segs;  // the chunk's, in text order
  std::atomic<uint32_t> bad{~0u};
  std::atomic<bool> io_bad{false};
  // the set whose text runs on into the next chunk, its descriptor, its bytes so far
  uint32_t open_set = ~0u;
  int open_fd = -1;
  uint64_t open_bytes = 0;

  ~SetFiles() {
    for (Seg &g : segs)
      if (g.fd >= 0) ::close(g.fd);
    if (open_fd >= 0) ::close(open_fd);
  }
  // under the segment's mutex (or on the calling thread between chunks)
  int open_file(uint32_t k) {
    if (k >= bad) return -1;
    const int fd = ::open(paths[k], O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) {
      for (uint32_t b = bad; k < b && !bad.compare_exchange_weak(b, k);) {
      }
      return -1;
    }
    if (!pwrite_all(fd, dbs->header[k].data(), dbs->header[k].size(), 0)) io_bad = true;
    return fd;
  }
  void close_file(int fd) {
    if (::close(fd) != 0) io_bad = true;
  }
  // a set without output rows: its header alone
  void header_only(uint32_t k) {
    const int fd = open_file(k);
    if (fd >= 0) close_file(fd);
  }

  // the segments of chunk [k0, k0 + cnt): the set running on from the last
  // chunk, then the m sets that start here at cuts[0 .. m); header-only files
  // of the latter are written here
  bool begin_chunk(const uint64_t *off, const uint64_t *n_out, uint64_t k0, uint32_t cnt,
                   uint32_t ks, uint32_t m, const uint32_t *cuts, uint64_t bytes) {
    segs.clear();
    for (uint32_t j = 0; j < m; ++j)
      if (cuts[j] > bytes || (j && cuts[j] < cuts[j - 1])) return false;
    const uint64_t end = k0 + cnt;
    if (ks > 0 && (ks == dbs->header.size() || off[ks] > k0) && n_out[ks - 1]) {
      const uint32_t k = ks - 1;
      const bool mine = open_set == k;
      const uint64_t t1 = m ? cuts[0] : bytes;
      segs.push_back(Seg{k, 0, t1, dbs->header[k].size() + (mine ? open_bytes : 0),
                         mine ? open_fd : -1, t1, off[k + 1] <= end});
    } else if (open_fd >= 0) {
      close_file(open_fd);
    }
    open_set = ~0u, open_fd = -1;
    for (uint32_t j = 0; j < m; ++j) {
      const uint32_t k = ks + j;
      const uint64_t t0 = cuts[j], t1 = j + 1 < m ? cuts[j + 1] : bytes;
      if (!n_out[k]) {
        header_only(k);
        continue;
      }
      segs.push_back(Seg{k, t0, t1, dbs->header[k].size(), -1, t1 - t0, off[k + 1] <= end});
    }
    return true;
  }

  // a writer's slot: bytes [off, off + len) of the chunk's text
  bool sink(const char *p, size_t len, size_t off) {
    const uint64_t lo = off, hi = off + len;
    size_t i = (size_t)(std::partition_point(segs.begin(), segs.end(),
                                             [&](const Seg &g) { return g.t1 <= lo; }) -
                        segs.begin());
    for (; i < segs.size() && segs[i].t0 < hi; ++i) {
      Seg &g = segs[i];
      const uint64_t a = std::max(lo, g.t0), b = std::min(hi, g.t1);
      if (a >= b) continue;
      int fd;
      {
        std::lock_guard<std::mutex> lk(mu[i % 32]);
        if (g.fd < 0) g.fd = open_file(g.set);
        fd = g.fd;
      }
      if (fd >= 0 && !pwrite_all(fd, p + (a - lo), (size_t)(b - a), g.base + (a - g.t0)))
        io_bad = true;
      std::lock_guard<std::mutex> lk(mu[i % 32]);
      g.left -= b - a;
      if (g.left == 0 && g.ends && g.fd >= 0) {
        close_file(g.fd);
        g.fd = -1;
      }
    }
    return !io_bad;
  }

  // after the chunk's last sink call: a set that ended here without text in
  // this chunk is closed; the one that runs on keeps its descriptor
  void end_chunk() {
    for (size_t i = 0; i < segs.size(); ++i) {
      Seg &g = segs[i];
      if (g.ends || g.set >= bad) {
        if (g.fd >= 0) close_file(g.fd);
      } else {  // (only the last segment can run on)
        open_set = g.set, open_fd = g.fd;
        open_bytes = g.base - dbs->header[g.set].size() + (g.t1 - g.t0);
      }
      g.fd = -1;
    }
    segs.clear();
  }
};

struct PinnedFree {
  void *p = nullptr;
  ~PinnedFree() {
    if (p) (void)hipHostFree(p);
  }
};

int set_io_error(rk_ctx *ctx, const SetFiles &f) {
  const uint32_t k = f.bad;
  if (k != ~0u) ctx->err = "set " + std::to_string(k) + ": cannot open " + f.paths[k];
  return RK_E_IO;
}

// A batch of sets: the chunks run over the slots of an rk_batch_result, and
// every chunk's text is split at the sets' cuts into their files.
struct SetRoute {
  const rk_dbset *dbs;
  const rk_batch_result *res;
  SetFiles files;
  uint32_t ns;
  const uint64_t *off;  // the host's set_off
  uint64_t total;       // off[ns]: slots = rows
  uint64_t rows = 0;    // the sum of n_out
  // device: the set tables, the chunk's combined rows, per text buffer the cuts
  SetTab tab{};
  uint32_t *crow = nullptr, *cuts[2] = {};
  PinnedFree pin;
  uint32_t *hcuts[2] = {};  // pinned

  SetRoute(const rk_dbset *d, const char *const *paths, const rk_batch_result *r)
      : dbs(d), res(r), files{d, paths}, ns((uint32_t)d->header.size()),
        off(d->set_off.data()), total(off[ns]) {}

  int open(rk_ctx *ctx, bool *work) {
    for (uint32_t k = 0; k < ns; ++k) {
      if (res->n_out[k] > off[k + 1] - off[k]) {
        ctx->err = "set " + std::to_string(k) + ": n_out exceeds the set's rows";
        return RK_E_ARG;
      }
      rows += res->n_out[k];
    }
    if (!rows)  // no text at all: every file is its header
      for (uint32_t k = 0; k < ns && files.bad == ~0u; ++k) files.header_only(k);
    *work = rows != 0;
    return RK_OK;
  }
  int set_up(rk_ctx *ctx, rk::Carve &c, uint32_t R) {
    crow = c.take<uint32_t>(R);
    cuts[0] = c.take<uint32_t>(ns), cuts[1] = c.take<uint32_t>(ns);
    tab.off = c.take<uint64_t>((size_t)ns + 1), tab.n_out = c.take<uint64_t>(ns);
    tab.ns = ns;
    if (!c.base) return RK_OK;  // the sizing pass ends here
    // placed: the pinned cuts, and the set tables up to the device
    hipStream_t s = ctx->stream;
    HIPCHK(ctx, hipHostMalloc(&pin.p, (size_t)ns * 8, hipHostMallocDefault));
    hcuts[0] = (uint32_t *)pin.p, hcuts[1] = hcuts[0] + ns;
    HIPCHK(ctx, hipMemcpyAsync((void *)tab.off, off, ((size_t)ns + 1) * 8, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync((void *)tab.n_out, res->n_out, (size_t)ns * 8,
                               hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipStreamSynchronize(s));  // (the tables are pageable host memory)
    return RK_OK;
  }
  Res len_pass(Save &S, uint64_t k0, uint32_t cnt, uint32_t nb) {
    const Res r = S.slice(k0);
    k_outb_len<<<nb, OB, 0, S.ctx->stream>>>(S.cols, tab, r, k0, cnt, crow, S.len8, S.hst,
                                             S.blk_tot, S.ctr);
    return Res{crow, r.gid, r.rep};
  }
  // the sets whose first slot lies in the chunk, and their cuts on the way down;
  // the last chunk also takes the empty sets at the very end
  int after_scan(Save &S, int par, uint64_t k0, uint32_t cnt, Chunk *out) {
    hipStream_t s = S.ctx->stream;
    const uint64_t *b = off, *e = off + ns;
    out->ks = (uint32_t)(std::lower_bound(b, e, k0) - b);
    out->m = (k0 + cnt >= total ? ns : (uint32_t)(std::lower_bound(b, e, k0 + cnt) - b)) - out->ks;
    if (!out->m) return RK_OK;
    k_outb_cuts<<<(out->m + OB - 1) / OB, OB, 0, s>>>(tab.off, out->ks, out->m, k0, cnt, S.len8,
                                                      S.blk_off, cuts[par]);
    HIPCHK(S.ctx, hipMemcpyAsync(hcuts[par], cuts[par], (size_t)out->m * 4,
                                 hipMemcpyDeviceToHost, s));
    return RK_OK;
  }
  int begin_chunk(rk_ctx *ctx, uint64_t k0, const Chunk &c, int par, hipEvent_t put) {
    // the chunk's cuts are down once its put pass is (all but the last chunk's
    // already is: the next chunk's length pass ran behind it)
    HIPCHK(ctx, hipEventSynchronize(put));
    if (files.begin_chunk(off, res->n_out, k0, c.cnt, c.ks, c.m, hcuts[par], c.bytes))
      return RK_OK;
    ctx->err = "csv cuts: the sets' text offsets do not lie in the chunk in order";
    return RK_E_INTERNAL;
  }
  bool sink(const char *p, size_t len, size_t o) { return files.sink(p, len, o); }
  void end_chunk(const Chunk &, int, rk_egress_stats *) { files.end_chunk(); }  // (io_bad says so)
  bool stop() const { return files.bad != ~0u || files.io_bad; }
  void done(rk_egress_stats *st) {
    st->rows = rows;
    if (files.open_fd >= 0) files.close_file(files.open_fd), files.open_fd = -1;
  }
  int finish(rk_ctx *ctx, int rc) { return rc ? rc : stop() ? set_io_error(ctx, files) : RK_OK; }
};

int write_set_device(rk_ctx *ctx, const rk_dbset *dbs, const char *const *paths,
                     const rk_batch_result *res, uint32_t flags) {
  SetRoute rt(dbs, paths, res);
  return write_chunks(ctx, dbs->db, rt, Res{res->out_order, res->gid, res->repval}, rt.total,
                      flags);
}

// rk_classify_device_batch on the set's resident columns into DEVICE result
// arrays carved from ctx->io (zeroed first, as rk_classify_batch's are);
// returns with the stream idle
int dbset_classify_resident(rk_ctx *ctx, const rk_dbset *dbs, double len_ratio, double pos_ratio,
                            rk_batch_result *dres) {
  rk_frags_soa dv;
  if (rk_db_device_view(dbs->db, &dv)) return RK_E_ARG;
  const uint32_t ns = (uint32_t)dbs->header.size();
  const size_t n = dv.n;
  if (n >= 0xFFFFFFFFull) return RK_E_TOO_MANY;
  Res r;
  int rc = carve_result(ctx, &ctx->io, &ctx->io_cap, n, "result staging", &r);
  if (rc) return rc;
  dres->out_order = r.order, dres->gid = r.gid, dres->repval = r.rep;
  if (n) {
    HIPCHK(ctx, hipMemsetAsync(dres->out_order, 0, n * 4, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(dres->gid, 0, n * 4, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(dres->repval, 0, n, ctx->stream));
  }
  const rk_batch_params bp{ns, dbs->set_off.data(), dbs->len_x_hdr.data(), dbs->len_y_hdr.data(),
                           len_ratio, pos_ratio};
  if ((rc = rk_classify_device_batch(ctx, &dv, &bp, dres))) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return RK_OK;
}

int check_set_args(rk_ctx *ctx, const rk_dbset *dbs, bool rows, const char *what) {
  if (!dbs->db->dev_free || (rows && !dbs->db->dev_rows)) {
    ctx->err = std::string(what) + ": the set was not loaded with " +
               (rows ? "RK_DB_KEEP_ROWS" : "RK_DB_KEEP_DEVICE");
    return RK_E_ARG;
  }
  if (dbs->db->dev_device != ctx->device) {
    ctx->err = std::string(what) + ": the set's columns are on another device";
    return RK_E_ARG;
  }
  return RK_OK;
}

// The selection by repeat flag between a classification and its save
// (rk_select.hip): the kept rows of device arrays in rk_batch_result layout go to
// ctx->sel in the same layout, kept[k] rows for set k.
int selected(rk_ctx *ctx, uint32_t ns, const uint64_t *off, const uint64_t *n_out, Res in,
             uint32_t keep, Res *out, uint64_t *kept) {
  const size_t n = ns ? off[ns] : 0;
  const int rc = carve_result(ctx, &ctx->sel, &ctx->sel_cap, n, "selected result", out);
  if (rc) return rc;
  return rk::select_device(ctx, ns, off, n_out, in.order, in.gid, in.rep, keep, out->order,
                           out->gid, out->rep, kept);
}

template <class F>
int guarded(rk_ctx *ctx, const char *what, F &&body) {
  try {
    return body();
  } catch (const std::bad_alloc &) {
    (void)hipStreamSynchronize(ctx->stream);
    ctx->err = std::string(what) + ": out of host memory";
    return RK_E_NOMEM;
  } catch (...) {
    (void)hipStreamSynchronize(ctx->stream);
    ctx->err = "unexpected C++ exception";
    return RK_E_INTERNAL;
  }
}

}  // namespace

extern "C" int rk_classify_dbset(rk_ctx *ctx, const rk_dbset *dbs, double len_ratio,
                                 double pos_ratio, rk_batch_result *out) {
  if (!ctx || !dbs || !out) return RK_E_ARG;
  const uint32_t ns = (uint32_t)dbs->header.size();
  const size_t n = dbs->set_off[ns];
  if (ns && (!out->n_out || !out->n_groups)) return RK_E_ARG;
  if (n && (!out->out_order || !out->gid || !out->repval)) return RK_E_ARG;
  ctx->err.clear();
  int rc = check_set_args(ctx, dbs, false, "rk_classify_dbset");
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return guarded(ctx, "rk_classify_dbset", [&]() -> int {
    rk_batch_result dres{nullptr, nullptr, nullptr, out->n_out, out->n_groups};
    int rc2 = dbset_classify_resident(ctx, dbs, len_ratio, pos_ratio, &dres);
    if (rc2 || !n) return rc2;
    return rk::io_d2h(ctx, {{out->out_order, dres.out_order, n * 4},
                            {out->gid, dres.gid, n * 4},
                            {out->repval, dres.repval, n}});
  });
}

extern "C" int rk_dbset_write_csv_device(rk_ctx *ctx, const rk_dbset *dbs,
                                         const char *const *paths, const rk_batch_result *res,
                                         uint32_t flags) {
  if (!ctx || !dbs || !res || (flags & ~(uint32_t)RK_RES_DEVICE)) return RK_E_ARG;
  const uint32_t ns = (uint32_t)dbs->header.size();
  if (ns && (!paths || !res->n_out)) return RK_E_ARG;
  for (uint32_t k = 0; k < ns; ++k)
    if (!paths[k]) return RK_E_ARG;
  if (dbs->set_off[ns] && (!res->out_order || !res->gid || !res->repval)) {
    bool any = false;
    for (uint32_t k = 0; k < ns; ++k) any |= res->n_out[k] != 0;
    if (any) return RK_E_ARG;
  }
  ctx->err.clear();
  int rc = check_set_args(ctx, dbs, true, "rk_dbset_write_csv_device");
  if (rc) return rc;
  return guarded(ctx, "rk_dbset_write_csv_device",
                 [&] { return write_set_device(ctx, dbs, paths, res, flags); });
}

extern "C" int rk_classify_dbset_to_csv_keep(rk_ctx *ctx, const rk_dbset *dbs, double len_ratio,
                                             double pos_ratio, const char *const *paths,
                                             uint32_t keep, uint64_t *n_out, uint64_t *n_groups,
                                             uint64_t *n_kept) {
  if (!ctx || !dbs || keep == 0 || keep > (uint32_t)RK_KEEP_ALL) return RK_E_ARG;
  const uint32_t ns = (uint32_t)dbs->header.size();
  if (ns && !paths) return RK_E_ARG;
  for (uint32_t k = 0; k < ns; ++k)
    if (!paths[k]) return RK_E_ARG;
  ctx->err.clear();
  int rc = check_set_args(ctx, dbs, true, "rk_classify_dbset_to_csv");
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return guarded(ctx, "rk_classify_dbset_to_csv", [&]() -> int {
    std::vector<uint64_t> no(ns), ng(ns), nk(ns);
    rk_batch_result dres{nullptr, nullptr, nullptr, no.data(), ng.data()};
    int rc2 = dbset_classify_resident(ctx, dbs, len_ratio, pos_ratio, &dres);
    if (rc2) return rc2;
    for (uint32_t k = 0; k < ns; ++k) {
      if (n_out) n_out[k] = no[k];
      if (n_groups) n_groups[k] = ng[k];
    }
    if (keep != (uint32_t)RK_KEEP_ALL) {
      // the kept rows of every set, at the set's own offset (the layout the save reads)
      Res sel;
      if ((rc2 = selected(ctx, ns, dbs->set_off.data(), no.data(),
                          Res{dres.out_order, dres.gid, dres.repval}, keep, &sel, nk.data())))
        return rc2;
      dres = rk_batch_result{sel.order, sel.gid, sel.rep, nk.data(), ng.data()};
    } else {
      nk = no;
    }
    for (uint32_t k = 0; k < ns; ++k)
      if (n_kept) n_kept[k] = nk[k];
    return write_set_device(ctx, dbs, paths, &dres, RK_RES_DEVICE);
  });
}

extern "C" int rk_classify_dbset_to_csv(rk_ctx *ctx, const rk_dbset *dbs, double len_ratio,
                                        double pos_ratio, const char *const *paths,
                                        uint64_t *n_out, uint64_t *n_groups) {
  return rk_classify_dbset_to_csv_keep(ctx, dbs, len_ratio, pos_ratio, paths, RK_KEEP_ALL, n_out,
                                       n_groups, nullptr);
}

extern "C" int rk_db_write_csv_device(rk_ctx *ctx, const rk_db *db, const char *path,
                                      const rk_result *res, uint32_t flags) {
  if (!ctx || !db || !path || !res || (flags & ~(uint32_t)RK_RES_DEVICE) ||
      (res->n_out && (!res->gid || !res->repval || !res->out_order)))
    return RK_E_ARG;
  ctx->err.clear();
  int rc = check_args(ctx, db, "rk_db_write_csv_device");
  if (rc) return rc;
  return guarded(ctx, "rk_db_write_csv_device",
                 [&] { return write_device(ctx, db, path, res, flags); });
}

extern "C" int rk_classify_db_pairs_to_csv_keep(rk_ctx *ctx, const rk_db *db,
                                                const double *len_ratio, const double *pos_ratio,
                                                uint32_t npairs, const char *const *paths,
                                                uint32_t keep, uint64_t *n_out,
                                                uint64_t *n_groups, uint64_t *n_kept) {
  if (!ctx || !db || !len_ratio || !pos_ratio || !paths || npairs == 0 || keep == 0 ||
      keep > (uint32_t)RK_KEEP_ALL)
    return RK_E_ARG;
  for (uint32_t q = 0; q < npairs; ++q)
    if (!paths[q]) return RK_E_ARG;
  ctx->err.clear();
  int rc = check_args(ctx, db, "rk_classify_db_pairs_to_csv");
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return guarded(ctx, "rk_classify_db_pairs_to_csv", [&]() -> int {
    std::vector<rk_result> dres;
    if ((rc = rk::db_classify_resident(ctx, db, len_ratio, pos_ratio, npairs, dres))) return rc;
    for (uint32_t q = 0; q < npairs; ++q) {
      if (n_out) n_out[q] = dres[q].n_out;
      if (n_groups) n_groups[q] = dres[q].n_groups;
    }
    for (uint32_t q = 0; q < npairs; ++q) {
      rk_result r = dres[q];
      if (keep != (uint32_t)RK_KEEP_ALL) {
        const uint64_t off[2] = {0, r.n_out};
        Res sel;
        uint64_t kept = 0;
        if ((rc = selected(ctx, 1, off, &r.n_out, Res{r.out_order, r.gid, r.repval}, keep, &sel,
                           &kept)))
          return rc;
        r = rk_result{sel.order, sel.gid, sel.rep, kept, r.n_groups};
      }
      if (n_kept) n_kept[q] = r.n_out;
      if ((rc = write_device(ctx, db, paths[q], &r, RK_RES_DEVICE))) return rc;
    }
    return RK_OK;
  });
}

extern "C" int rk_classify_db_pairs_to_csv(rk_ctx *ctx, const rk_db *db, const double *len_ratio,
                                           const double *pos_ratio, uint32_t npairs,
                                           const char *const *paths, uint64_t *n_out,
                                           uint64_t *n_groups) {
  return rk_classify_db_pairs_to_csv_keep(ctx, db, len_ratio, pos_ratio, npairs, paths,
                                          RK_KEEP_ALL, n_out, n_groups, nullptr);
}

extern "C" int rk_get_egress_stats(const rk_ctx *ctx, rk_egress_stats *st) {
  if (!ctx || !st) return RK_E_ARG;
  *st = ctx->egress;
  return RK_OK;
}
