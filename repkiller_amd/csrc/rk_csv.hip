// rk_csv.hip -- device ingress: a fragment CSV parsed on the GPU
// (rk_db_load_csv_device), beside the host parser of rk_host.cpp.
//
// FragmentsDatabase.cpp:17-101 reads 16 header lines and then one fragment per
// body line.  Here the header is read on the host exactly as rk_db_load_csv
// reads it, and the body goes to the device as raw bytes through the copy
// stream's staging ring (rk_io.hip).  Per window of the body:
//   1. line index: every 2-KB tile counts its '\n' (16-B loads), the tile
//      counts are scanned, and every line's start offset is written as u64
//      (a last line without '\n' is a line; an empty line is a line);
//   2. row kernel: one lane per line runs csv_line (rk_csv_line.h) straight
//      from global memory and writes nine staged column values and a status
//      byte at the line's index;
//   3. host fix-up: lines whose status is CSV_HOST (the similarity field needs
//      strtof, or the line is longer than RK_CSV_MAX_LINE) are listed, parsed
//      by the host's own parse_line from the mapped file, and patched in;
//   4. stable compaction: the accept flags are scanned and the accepted rows
//      scattered, in file order, into the database's final device columns.
// The nine columns then come down into the rk_db's vectors (io_d2h); with
// RK_DB_KEEP_DEVICE the four classification columns also stay in HBM, owned by
// the database.  Scratch comes from the context's grow-only buffers (ctx->io
// for the raw bytes and the tile index, ctx->ws for the per-line arrays); the
// resident columns are an allocation of the database's own, so no later
// rk_classify* on the context can alias them.
//
// A batch of files (rk_dbset_load_csv_device) runs the same four steps over
// ONE byte stream: every file is mapped, its header read on the host, and the
// bodies are gathered piece by piece into the staging slots (io_h2d_gather), a
// body without a final newline getting one, so no line joins the next file's
// first.  Windows cut the stream as they cut one body, inside a set or at a set
// boundary.  After each window's compaction one lane per set whose body starts
// in the window finds the set's first row (k_csv_setoff); the per-set count
// check (FragmentsDatabase.cpp:99) runs on those offsets before the columns
// come down into the one combined rk_db of the rk_dbset.
//
// The load is synchronous: it returns when the host columns are complete.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <functional>
#include <memory>
#include <new>

#include "rk_csv_line.h"
#include "rk_csv_scan.h"
#include "rk_ctx.h"
#include "rk_db.h"

namespace rk {

int dev_alloc(rk_ctx *ctx, void **p, size_t bytes, const char *what) {
  const hipError_t e = hipMalloc(p, bytes ? bytes : 16);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    *p = nullptr;
    ctx->err = std::string(what) + " hipMalloc(" + std::to_string(bytes) + "): " +
               hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? RK_E_NOMEM : RK_E_HIP;
  }
  return RK_OK;
}

// one of the context's grow-only buffers, at least `need` bytes
int grow(rk_ctx *ctx, void **buf, size_t *cap, size_t need, const char *what) {
  if (need <= *cap) return RK_OK;
  if (*buf) (void)hipFree(*buf);
  *buf = nullptr;
  *cap = 0;
  const int rc = dev_alloc(ctx, buf, need, what);
  if (rc) return rc;
  *cap = need;
  return RK_OK;
}

}  // namespace rk

namespace {

using rk::dev_alloc;
using rk::block_excl_scan;
using rk::grow;

// bytes of one line-index block: 128 lanes x 16 B.  Half of RK_CSV_MAX_LINE, so
// a line the device parses can span three tiles.
constexpr uint32_t TILE = 2048;
constexpr uint32_t TI = TILE / 16;  // threads of a line-index block
constexpr uint32_t TB = 256;        // threads (= lines) of a row block
constexpr uint64_t DEFAULT_WINDOW = 8ull << 30;

struct Cols {
  uint64_t *xs, *ys, *xe, *ye, *len, *score, *ident;
  float *sim;
  uint8_t *strand;
};

struct PatchRow {
  uint64_t line;
  uint64_t xs, ys, xe, ye, len, score, ident;
  float sim;
  uint8_t strand, status;
};

// bit j: byte off + j of the window is '\n' (off a multiple of 16; the buffer is
// readable up to the next multiple of 16 past W, bytes past W are masked)
__device__ inline uint32_t nl_mask(const char *buf, uint64_t off, uint64_t W) {
  if (off >= W) return 0;
  const uint4 v = *reinterpret_cast<const uint4 *>(buf + off);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t m = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (((w[k] >> (8 * j)) & 0xFFu) == 0x0Au) m |= 1u << (4 * k + j);
  const uint64_t left = W - off;
  if (left < 16) m &= (1u << (uint32_t)left) - 1u;
  return m;
}

__global__ __launch_bounds__(TI) void k_csv_nl_count(const char *buf, uint64_t W,
                                                    uint32_t *tile_cnt) {
  const uint64_t off = (uint64_t)blockIdx.x * TILE + threadIdx.x * 16u;
  // (a count of the lanes that hold a newline, summed over their 16 bytes)
  __shared__ uint32_t lds[TI];
  uint32_t sum;
  (void)block_excl_scan<TI>((uint32_t)__popc(nl_mask(buf, off, W)), lds, &sum);
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = sum;
}

// start[k] = body offset of line k; the '\n' that ends line k writes
// start[k + 1], so with a final newline start[lines] = wbase + W; without one
// the sentinel start[lines] = wbase + W + 1 keeps "end = start[k + 1] - 1"
__global__ __launch_bounds__(TI) void k_csv_index(const char *buf, uint64_t W, uint64_t wbase,
                                                 const uint64_t *tile_pre, uint64_t lines,
                                                 uint32_t tail, uint64_t *start) {
  __shared__ uint32_t lds[TI];
  const uint64_t off = (uint64_t)blockIdx.x * TILE + threadIdx.x * 16u;
  uint32_t m = nl_mask(buf, off, W);
  uint32_t sum;
  const uint32_t excl = block_excl_scan<TI>((uint32_t)__popc(m), lds, &sum);
  uint64_t k = tile_pre[blockIdx.x] + excl + 1;
  while (m) {
    const uint32_t j = (uint32_t)__ffs((int)m) - 1u;
    m &= m - 1u;
    if (k <= lines) start[k] = wbase + off + j + 1;
    ++k;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    start[0] = wbase;
    if (tail) start[lines] = wbase + W + 1;
  }
}

// cnt[0] += accepted lines, cnt[1] += host lines
__global__ __launch_bounds__(TB) void k_csv_rows(const char *buf, uint64_t wbase,
                                                const uint64_t *start, uint64_t lines, Cols c,
                                                uint8_t *status, unsigned long long *cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  uint8_t st = rk::CSV_REJECT;
  const bool live = i < lines;
  if (live) {
    const uint64_t b = start[i] - wbase, e = start[i + 1] - 1 - wbase;
    if (e - b > RK_CSV_MAX_LINE) {
      st = rk::CSV_HOST;
    } else {
      rk::CsvRow r;
      st = rk::csv_line(buf + b, buf + e, &r);
      if (st == rk::CSV_ACCEPT) {
        c.xs[i] = r.xs, c.ys[i] = r.ys, c.xe[i] = r.xe, c.ye[i] = r.ye;
        c.len[i] = r.len, c.score[i] = r.score, c.ident[i] = r.ident;
        c.sim[i] = r.sim, c.strand[i] = r.strand;
      }
    }
    status[i] = st;
  }
  const int na = __syncthreads_count(live && st == rk::CSV_ACCEPT);
  const int nh = __syncthreads_count(live && st == rk::CSV_HOST);
  if (threadIdx.x == 0) {
    if (na) atomicAdd(&cnt[0], (unsigned long long)na);
    if (nh) atomicAdd(&cnt[1], (unsigned long long)nh);
  }
}

// the CSV_HOST lines as (line, offset, length); any order, cap entries at most
__global__ __launch_bounds__(TB) void k_csv_hostlist(const uint8_t *status, const uint64_t *start,
                                                    uint64_t lines, unsigned long long *slot,
                                                    uint64_t cap, uint64_t *list) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= lines || status[i] != rk::CSV_HOST) return;
  const uint64_t k = atomicAdd(slot, 1ull);
  if (k >= cap) return;
  list[3 * k] = i;
  list[3 * k + 1] = start[i];
  list[3 * k + 2] = start[i + 1] - 1 - start[i];
}

__global__ __launch_bounds__(TB) void k_csv_patch(const PatchRow *rows, uint64_t n, uint64_t lines,
                                                 Cols c, uint8_t *status) {
  const uint64_t k = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (k >= n) return;
  const PatchRow r = rows[k];
  const uint64_t i = r.line;
  if (i >= lines) return;
  status[i] = r.status;
  if (r.status != rk::CSV_ACCEPT) return;
  c.xs[i] = r.xs, c.ys[i] = r.ys, c.xe[i] = r.xe, c.ye[i] = r.ye;
  c.len[i] = r.len, c.score[i] = r.score, c.ident[i] = r.ident;
  c.sim[i] = r.sim, c.strand[i] = r.strand;
}

__global__ __launch_bounds__(TB) void k_csv_flagcount(const uint8_t *status, uint64_t lines,
                                                     uint32_t *blk_cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  const int n = __syncthreads_count(i < lines && status[i] == rk::CSV_ACCEPT);
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = (uint32_t)n;
}

// accepted rows, in line order, to rows [out_base, out_base + accepted) of the
// final columns (dst < out_cap is the host's count check, kept here as a guard)
__global__ __launch_bounds__(TB) void k_csv_scatter(const uint8_t *status, uint64_t lines,
                                                   const uint64_t *blk_pre, uint64_t out_base,
                                                   uint64_t out_cap, Cols s, Cols d) {
  __shared__ uint32_t lds[TB];
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  const bool take = i < lines && status[i] == rk::CSV_ACCEPT;
  uint32_t sum;
  const uint32_t excl = block_excl_scan<TB>(take ? 1u : 0u, lds, &sum);
  if (!take) return;
  const uint64_t o = out_base + blk_pre[blockIdx.x] + excl;
  if (o >= out_cap) return;
  d.xs[o] = s.xs[i], d.ys[o] = s.ys[i], d.xe[o] = s.xe[i], d.ye[o] = s.ye[i];
  d.len[o] = s.len[i], d.score[o] = s.score[i], d.ident[o] = s.ident[i];
  d.sim[o] = s.sim[i], d.strand[o] = s.strand[i];
}

// A batch of files: set k's first row in the combined columns.  Lane k takes a
// set whose body starts in this window at stream offset first[k] (a line start:
// every body ends in a newline there).  It lower-bounds that offset in start[],
// then adds the line's block prefix and the accepted lines before it in its
// 256-line block: no atomics, and the work scales with the sets, not the lines.
__global__ __launch_bounds__(TB) void k_csv_setoff(const uint64_t *first, uint32_t ns,
                                                  const uint64_t *start, uint64_t lines,
                                                  const uint8_t *status, const uint64_t *blk_pre,
                                                  uint64_t out_base, uint64_t *set_off) {
  const uint32_t k = blockIdx.x * TB + threadIdx.x;
  if (k >= ns) return;
  const uint64_t f = first[k];
  // (the host passes only sets with wbase <= f < wbase + W, and f is the start
  // of one of the window's lines, so the search ends at lo < lines)
  uint64_t lo = 0, hi = lines;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (start[mid] < f) lo = mid + 1;
    else hi = mid;
  }
  uint64_t rows = blk_pre[lo / TB];
  for (uint64_t i = lo - lo % TB; i < lo; ++i) rows += status[i] == rk::CSV_ACCEPT;
  set_off[k] = out_base + rows;
}

// ------------------------------------------------------------------ host --

using Stream = rk::CsvStream;  // rk_csv_stream.h

// the sets of a batch: where each body starts in the stream, and its first row
struct SetIndex {
  std::vector<uint64_t> first;    // nsets: stream offset of set k's body
  std::vector<uint64_t> host_off; // nsets: first row where the host decided it (~0: not)
  std::vector<uint64_t> total;    // nsets: the header totals
  uint64_t *d_first = nullptr, *d_off = nullptr;  // device: first[], first rows (~0: not set)
};

struct Mapped {
  const char *p = nullptr;
  size_t n = 0;
  int fd = -1;
  ~Mapped() {
    if (p && n) munmap((void *)p, n);
    if (fd >= 0) close(fd);
  }
};

struct DevBuf {
  void *p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

struct Events {
  hipEvent_t a = nullptr, b = nullptr;
  ~Events() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

void free_dev_block(void *block, int device) {
  if (device >= 0) (void)hipSetDevice(device);
  (void)hipFree(block);
}

Cols carve_cols(rk::Carve &c, uint64_t n) {
  Cols k;
  k.xs = c.take<uint64_t>(n), k.ys = c.take<uint64_t>(n), k.xe = c.take<uint64_t>(n);
  k.ye = c.take<uint64_t>(n), k.len = c.take<uint64_t>(n), k.score = c.take<uint64_t>(n);
  k.ident = c.take<uint64_t>(n), k.sim = c.take<float>(n), k.strand = c.take<uint8_t>(n);
  return k;
}

uint64_t window_bytes() {
  const char *e = std::getenv("RK_CSV_WINDOW");
  if (e && *e) {
    char *end = nullptr;
    const unsigned long long v = std::strtoull(e, &end, 10);
    if (end != e && v > 0) return std::min<unsigned long long>(v, 64ull << 30);
  }
  return DEFAULT_WINDOW;
}

uint32_t grid_for(uint64_t n) { return (uint32_t)((n + TB - 1) / TB); }

// The nine host columns at n rows.  The first touch of 61 B per row is the
// larger part of what the download costs, so a large column is sized (and
// zero-filled) by a thread of its own; a thread that cannot start leaves its
// column to the caller's.
int size_columns(rk_db *db, uint64_t n) {
  const std::function<void()> col[9] = {
      [&] { db->x_start.resize(n); }, [&] { db->y_start.resize(n); },
      [&] { db->x_end.resize(n); },   [&] { db->y_end.resize(n); },
      [&] { db->length.resize(n); },  [&] { db->score.resize(n); },
      [&] { db->ident.resize(n); },   [&] { db->similarity.resize(n); },
      [&] { db->strand.resize(n); }};
  std::atomic<bool> ok{true};
  auto run = [&](int k) {
    try {
      col[k]();
    } catch (...) {
      ok = false;
    }
  };
  std::vector<std::thread> th;
  for (int k = 0; k < 9; ++k) {
    bool started = false;
    if (n >= (1u << 16) && k < 8) {
      try {
        th.emplace_back(run, k);
        started = true;
      } catch (...) {
      }
    }
    if (!started) run(k);
  }
  for (auto &t : th) t.join();
  return ok ? RK_OK : RK_E_NOMEM;
}

struct Load {
  rk_ctx *ctx;
  const Stream *body;  // the body bytes; offsets below are relative to the stream
  Cols fin;          // final device columns, out_cap rows
  uint64_t out_cap, total_hdr;
  uint64_t out_n = 0;  // rows in the final columns so far
  rk_ingress_stats *st;
  SetIndex *sets = nullptr;  // a batch of files: per-set first rows are kept
  bool overflow = false;     // a batch: more rows than out_cap (some set exceeds its total)
  Events ev;

  int timed_begin() {
    HIPCHK(ctx, hipEventRecord(ev.a, ctx->stream));
    return RK_OK;
  }
  // waits for the stream; adds the kernels' time since timed_begin()
  int timed_end() {
    HIPCHK(ctx, hipEventRecord(ev.b, ctx->stream));
    HIPCHK(ctx, hipEventSynchronize(ev.b));
    float ms = 0;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ev.a, ev.b));
    st->device_ms += ms;
    HIPCHK(ctx, hipGetLastError());
    return RK_OK;
  }

  // rows the host parsed on its own (lines longer than a window), in file
  // order, appended to the final columns
  int flush_rows(std::vector<rk::DbRow> &rows) {
    const uint64_t k = rows.size();
    if (!k) return RK_OK;
    if (out_n + k > total_hdr) return RK_E_COUNT;
    if (sets && out_n + k > out_cap) {  // the per-set count check names the set
      overflow = true;
      out_n += k;
      rows.clear();
      return RK_OK;
    }
    std::vector<uint64_t> u(k);
    std::vector<float> f(k);
    std::vector<uint8_t> b(k);
    auto put64 = [&](uint64_t *dst, uint64_t rk::DbRow::*m) -> int {
      for (uint64_t i = 0; i < k; ++i) u[i] = rows[i].*m;
      HIPCHK(ctx, hipMemcpy(dst + out_n, u.data(), k * 8, hipMemcpyHostToDevice));
      return RK_OK;
    };
    int rc;
    if ((rc = put64(fin.xs, &rk::DbRow::xs)) || (rc = put64(fin.ys, &rk::DbRow::ys)) ||
        (rc = put64(fin.xe, &rk::DbRow::xe)) || (rc = put64(fin.ye, &rk::DbRow::ye)) ||
        (rc = put64(fin.len, &rk::DbRow::len)) || (rc = put64(fin.score, &rk::DbRow::score)) ||
        (rc = put64(fin.ident, &rk::DbRow::ident)))
      return rc;
    for (uint64_t i = 0; i < k; ++i) f[i] = rows[i].sim, b[i] = rows[i].strand;
    HIPCHK(ctx, hipMemcpy(fin.sim + out_n, f.data(), k * 4, hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(fin.strand + out_n, b.data(), k, hipMemcpyHostToDevice));
    out_n += k;
    rows.clear();
    return RK_OK;
  }

  // one window [wbase, wbase + W) of the body through the device
  int window(uint64_t wbase, uint64_t W) {
    hipStream_t s = ctx->stream;
    const uint64_t ntiles = (W + TILE - 1) / TILE;
    // stage A: raw bytes, tile counts and their scan, counters
    rk::Carve pa{nullptr};
    auto carve_a = [&](rk::Carve &c, char **raw, uint32_t **tc, uint64_t **tp,
                       unsigned long long **cnt) {
      *raw = c.take<char>(W + 16);
      *tc = c.take<uint32_t>(ntiles);
      *tp = c.take<uint64_t>(ntiles + 1);
      *cnt = c.take<unsigned long long>(8);
    };
    char *raw;
    uint32_t *tile_cnt;
    uint64_t *tile_pre;
    unsigned long long *cnt;
    carve_a(pa, &raw, &tile_cnt, &tile_pre, &cnt);
    int rc = grow(ctx, &ctx->io, &ctx->io_cap, pa.off, "csv window");
    if (rc) return rc;
    rk::Carve ra{(char *)ctx->io};
    carve_a(ra, &raw, &tile_cnt, &tile_pre, &cnt);

    double t = rk::wall_ms();
    // (one piece with nothing appended is its own bytes: the plain upload.  A
    // one-file batch whose body got a newline is a stream like any other: its
    // last byte is not in the file)
    if (body->p.size() == 1 && !body->nl[0])
      rc = rk::io_h2d(ctx, {{(void *)(body->p[0] + wbase), raw, (size_t)W}});
    else
      rc = rk::io_h2d_gather(ctx, body->io(), wbase, W, raw);
    if (rc) return rc;
    st->h2d_ms += rk::wall_ms() - t;

    if ((rc = timed_begin())) return rc;
    HIPCHK(ctx, hipMemsetAsync(cnt, 0, 8 * sizeof(unsigned long long), s));
    k_csv_nl_count<<<(uint32_t)ntiles, TI, 0, s>>>(raw, W, tile_cnt);
    rk::k_csv_scan<uint64_t><<<1, 1024, 0, s>>>(tile_cnt, ntiles, tile_pre);
    uint64_t newlines = 0;
    HIPCHK(ctx, hipMemcpyAsync(ctx->host, tile_pre + ntiles, 8, hipMemcpyDeviceToHost, s));
    if ((rc = timed_end())) return rc;
    std::memcpy(&newlines, ctx->host, 8);
    const uint32_t tail = body->at(wbase + W - 1) != '\n';
    const uint64_t lines = newlines + tail;
    if (newlines > W) {
      ctx->err = "csv line index: more newlines than bytes";
      return RK_E_INTERNAL;
    }

    // stage B: the per-line arrays
    const uint64_t nblk = (lines + TB - 1) / TB;
    auto carve_b = [&](rk::Carve &c, uint64_t **start, Cols *stg, uint8_t **status,
                       uint32_t **bc, uint64_t **bp) {
      *start = c.take<uint64_t>(lines + 2);
      *stg = carve_cols(c, lines);
      *status = c.take<uint8_t>(lines);
      *bc = c.take<uint32_t>(nblk);
      *bp = c.take<uint64_t>(nblk + 1);
    };
    uint64_t *start, *blk_pre;
    Cols stg;
    uint8_t *status;
    uint32_t *blk_cnt;
    rk::Carve pb{nullptr};
    carve_b(pb, &start, &stg, &status, &blk_cnt, &blk_pre);
    if ((rc = grow(ctx, &ctx->ws, &ctx->ws_cap, pb.off, "csv rows"))) return rc;
    rk::Carve rb{(char *)ctx->ws};
    carve_b(rb, &start, &stg, &status, &blk_cnt, &blk_pre);

    if ((rc = timed_begin())) return rc;
    k_csv_index<<<(uint32_t)ntiles, TI, 0, s>>>(raw, W, wbase, tile_pre, lines, tail, start);
    k_csv_rows<<<grid_for(lines), TB, 0, s>>>(raw, wbase, start, lines, stg, status, cnt);
    HIPCHK(ctx, hipMemcpyAsync(ctx->host, cnt, 16, hipMemcpyDeviceToHost, s));
    if ((rc = timed_end())) return rc;
    uint64_t got[2];
    std::memcpy(got, ctx->host, 16);
    uint64_t accepted = got[0];
    const uint64_t nhost = got[1];
    if (accepted + nhost > lines) {
      ctx->err = "csv row kernel: counts exceed the line count";
      return RK_E_INTERNAL;
    }
    st->lines += lines;
    st->host_lines += nhost;

    // host fix-up: the lines the device does not decide
    if (nhost) {
      t = rk::wall_ms();
      DevBuf list, patch;
      if ((rc = dev_alloc(ctx, &list.p, nhost * 24, "csv host list"))) return rc;
      if ((rc = dev_alloc(ctx, &patch.p, nhost * sizeof(PatchRow), "csv host rows"))) return rc;
      k_csv_hostlist<<<grid_for(lines), TB, 0, s>>>(status, start, lines, cnt + 2, nhost,
                                                    (uint64_t *)list.p);
      std::vector<uint64_t> hl(nhost * 3);
      HIPCHK(ctx, hipMemcpyAsync(hl.data(), list.p, nhost * 24, hipMemcpyDeviceToHost, s));
      HIPCHK(ctx, hipStreamSynchronize(s));
      std::vector<PatchRow> pr(nhost);
      // (a file whose similarity column is all exponents sends every line
      // here: the list is parsed by up to 16 threads, like rk_db_load_csv)
      std::atomic<uint64_t> kept{0};
      std::atomic<bool> outside{false};
      auto parse = [&](uint64_t k0, uint64_t k1) {
        uint64_t mine = 0;
        for (uint64_t k = k0; k < k1; ++k) {
          const uint64_t line = hl[3 * k], off = hl[3 * k + 1], len = hl[3 * k + 2];
          PatchRow &q = pr[k];
          std::memset(&q, 0, sizeof q);
          q.line = line;
          q.status = rk::CSV_REJECT;
          if (line >= lines || off < wbase || len > W || off + len > wbase + W) {
            outside = true;
            continue;
          }
          const char *text = body->span(off, len);
          if (!text) {
            outside = true;
            continue;
          }
          rk::DbRow r;
          if (rk::db_parse_line(text, text + len, &r)) {
            q.xs = r.xs, q.ys = r.ys, q.xe = r.xe, q.ye = r.ye, q.len = r.len, q.score = r.score;
            q.ident = r.ident, q.sim = r.sim, q.strand = r.strand;
            q.status = rk::CSV_ACCEPT;
            ++mine;
          }
        }
        kept += mine;
      };
      const unsigned nt = nhost < (1u << 14)
                              ? 1u
                              : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
      {
        std::vector<std::thread> th;
        for (unsigned w = 1; w < nt; ++w) {
          const uint64_t k0 = nhost * w / nt, k1 = nhost * (w + 1) / nt;
          try {
            th.emplace_back(parse, k0, k1);
          } catch (...) {  // no thread to be had: this one takes the share
            parse(k0, k1);
          }
        }
        parse(0, nhost / nt);
        for (auto &x : th) x.join();
      }
      if (outside) {
        ctx->err = "csv host list: entry outside the window";
        return RK_E_INTERNAL;
      }
      accepted += kept;
      HIPCHK(ctx, hipMemcpyAsync(patch.p, pr.data(), nhost * sizeof(PatchRow),
                                 hipMemcpyHostToDevice, s));
      k_csv_patch<<<grid_for(nhost), TB, 0, s>>>((const PatchRow *)patch.p, nhost, lines, stg,
                                                 status);
      HIPCHK(ctx, hipStreamSynchronize(s));
      st->host_fix_ms += rk::wall_ms() - t;
    }

    // count check (FragmentsDatabase.cpp:99), then the stable compaction
    if (out_n + accepted > total_hdr) return RK_E_COUNT;
    if (out_n + accepted > out_cap) {
      if (!sets) {
        ctx->err = "csv compaction: more rows than the bound on accepted lines";
        return RK_E_INTERNAL;
      }
      overflow = true;  // (the scatter stops at out_cap; the per-set check names the set)
    }
    if (lines) {
      if ((rc = timed_begin())) return rc;
      k_csv_flagcount<<<(uint32_t)nblk, TB, 0, s>>>(status, lines, blk_cnt);
      rk::k_csv_scan<uint64_t><<<1, 1024, 0, s>>>(blk_cnt, nblk, blk_pre);
      k_csv_scatter<<<(uint32_t)nblk, TB, 0, s>>>(status, lines, blk_pre, out_n, out_cap, stg,
                                                  fin);
      if (sets) {  // the sets whose bodies start in this window
        const auto &f = sets->first;
        const size_t k0 = (size_t)(std::lower_bound(f.begin(), f.end(), wbase) - f.begin());
        const size_t k1 = (size_t)(std::lower_bound(f.begin(), f.end(), wbase + W) - f.begin());
        if (k1 > k0)
          k_csv_setoff<<<grid_for(k1 - k0), TB, 0, s>>>(sets->d_first + k0, (uint32_t)(k1 - k0),
                                                        start, lines, status, blk_pre, out_n,
                                                        sets->d_off + k0);
      }
      if ((rc = timed_end())) return rc;
    }
    out_n += accepted;
    ++st->windows;
    return RK_OK;
  }
};

int map_file(const char *path, Mapped *m) {
  m->fd = open(path, O_RDONLY);
  if (m->fd < 0) return RK_E_IO;
  struct stat sb;
  if (fstat(m->fd, &sb) != 0) return RK_E_IO;
  m->n = (size_t)sb.st_size;
  if (m->n) {
    void *q = mmap(nullptr, m->n, PROT_READ, MAP_PRIVATE, m->fd, 0);
    if (q == MAP_FAILED) return RK_E_IO;
    m->p = (const char *)q;
  }
  return RK_OK;
}

// The body bytes through the device into db's nine host columns and, where
// flags keep them, its resident ones.  total_hdr: the bound of the count check
// on the rows as a whole (a batch checks per set afterwards: ~0); row_bound: a
// bound on the rows the final columns must hold.  sets: a batch's set index,
// whose per-set first rows come back in sets->host_off (every entry set) after
// the per-set count check.
int load_body(rk_ctx *ctx, const Stream &body, uint32_t flags, rk_db *db, uint64_t total_hdr,
              uint64_t row_bound, SetIndex *sets) {
  rk_ingress_stats &st = ctx->ingress;
  const uint64_t body_bytes = body.size();
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const bool keep = flags & RK_DB_KEEP_DEVICE;
  const bool keep_rows = flags == RK_DB_KEEP_ROWS;
  if (keep) {
    db->dev_free = free_dev_block;
    db->dev_device = ctx->device;
    db->dev_rows = keep_rows;
  }
  uint64_t n = 0;
  if (body_bytes) {
    // an accepted line holds at least "Frag,1": 6 bytes and its newline
    const uint64_t cap = std::min<uint64_t>(row_bound, body_bytes / 7 + 1);
    const size_t ns = sets ? sets->first.size() : 0;
    DevBuf set_tab;
    if (sets) {
      int rc0 = dev_alloc(ctx, &set_tab.p, ns * 16, "csv set index");
      if (rc0) return rc0;
      sets->d_first = (uint64_t *)set_tab.p, sets->d_off = sets->d_first + ns;
      HIPCHK(ctx, hipMemcpyAsync(sets->d_first, sets->first.data(), ns * 8, hipMemcpyHostToDevice,
                                 ctx->stream));
      HIPCHK(ctx, hipMemsetAsync(sets->d_off, 0xFF, ns * 8, ctx->stream));
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    // the database's own columns: x_start, y_start, length, strand (kept with
    // RK_DB_KEEP_DEVICE) and the five others
    // (with RK_DB_KEEP_ROWS one allocation holds both blocks, the five others
    // behind the four: the database's one dev_free hook releases all nine)
    DevBuf kept, rest;
    rk::Carve pk{nullptr}, pr{nullptr};
    pk.take<uint64_t>(cap), pk.take<uint64_t>(cap), pk.take<uint64_t>(cap), pk.take<uint8_t>(cap);
    pr.take<uint64_t>(cap), pr.take<uint64_t>(cap), pr.take<uint64_t>(cap), pr.take<uint64_t>(cap);
    pr.take<float>(cap);
    int rc;
    if ((rc = dev_alloc(ctx, &kept.p, pk.off + (keep_rows ? pr.off : 0), "csv columns"))) return rc;
    if (!keep_rows && (rc = dev_alloc(ctx, &rest.p, pr.off, "csv columns"))) return rc;
    rk::Carve ck{(char *)kept.p}, cr{keep_rows ? (char *)kept.p + pk.off : (char *)rest.p};
    Load L{ctx, &body};
    L.sets = sets;
    L.fin.xs = ck.take<uint64_t>(cap), L.fin.ys = ck.take<uint64_t>(cap);
    L.fin.len = ck.take<uint64_t>(cap), L.fin.strand = ck.take<uint8_t>(cap);
    L.fin.xe = cr.take<uint64_t>(cap), L.fin.ye = cr.take<uint64_t>(cap);
    L.fin.score = cr.take<uint64_t>(cap), L.fin.ident = cr.take<uint64_t>(cap);
    L.fin.sim = cr.take<float>(cap);
    L.out_cap = cap;
    L.total_hdr = total_hdr;
    L.st = &st;
    HIPCHK(ctx, hipEventCreate(&L.ev.a));
    HIPCHK(ctx, hipEventCreate(&L.ev.b));

    // windows of at most RK_CSV_WINDOW bytes, cut after a '\n'; a line that
    // does not fit a window is a host line
    const uint64_t wmax = window_bytes();
    std::vector<rk::DbRow> pending;
    uint64_t pos = 0;
    while (pos < body_bytes) {
      uint64_t wend = body_bytes;
      if (body_bytes - pos > wmax) {
        const uint64_t nl = body.last_nl(pos, pos + wmax);
        wend = nl != ~0ull ? nl + 1 : pos;
      }
      if (wend > pos) {
        if ((rc = L.flush_rows(pending))) return rc;
        if ((rc = L.window(pos, wend - pos))) return rc;
        pos = wend;
        continue;
      }
      const double t = rk::wall_ms();
      if (sets)  // the sets whose bodies start with this line: the host knows their first row
        for (size_t k = (size_t)(std::lower_bound(sets->first.begin(), sets->first.end(), pos) -
                                 sets->first.begin());
             k < ns && sets->first[k] == pos; ++k)
          sets->host_off[k] = L.out_n + pending.size();
      const uint64_t nl = body.next_nl(pos);
      const uint64_t le = nl != ~0ull ? nl : body_bytes;
      const char *text = body.span(pos, le - pos);
      if (!text) {
        ctx->err = "csv host line: a line crosses two files' bodies";
        return RK_E_INTERNAL;
      }
      rk::DbRow r;
      if (rk::db_parse_line(text, text + (le - pos), &r)) pending.push_back(r);
      ++st.lines;
      ++st.host_lines;
      pos = nl != ~0ull ? le + 1 : body_bytes;
      st.host_fix_ms += rk::wall_ms() - t;
      if (L.out_n + pending.size() > total_hdr) return RK_E_COUNT;
    }
    if ((rc = L.flush_rows(pending))) return rc;
    n = L.out_n;
    if (sets) {
      // first rows: the device's where a window held the body's start, the
      // host's where a host line did, the row count for bodies at the stream's end
      std::vector<uint64_t> got(ns);
      HIPCHK(ctx, hipMemcpy(got.data(), sets->d_off, ns * 8, hipMemcpyDeviceToHost));
      for (size_t k = 0; k < ns; ++k)
        if (sets->host_off[k] == ~0ull) sets->host_off[k] = got[k] != ~0ull ? got[k] : n;
      sets->d_first = sets->d_off = nullptr;
      // the count check (FragmentsDatabase.cpp:99), per file, before any row is
      // promised to anyone
      for (size_t k = 0; k < ns; ++k) {
        const uint64_t a = sets->host_off[k], b = k + 1 < ns ? sets->host_off[k + 1] : n;
        if (a > b) {
          ctx->err = "csv set index: first rows decrease at set " + std::to_string(k);
          return RK_E_INTERNAL;
        }
        if (b - a > sets->total[k]) {
          ctx->err = "set " + std::to_string(k) + ": more fragments than the header total";
          return RK_E_COUNT;
        }
      }
      if (L.overflow) {
        ctx->err = "csv compaction: more rows than the sets' header totals allow";
        return RK_E_INTERNAL;
      }
      if (n >= 0xFFFFFFFFull) return RK_E_TOO_MANY;
    }

    // the nine columns into the database's vectors
    const double t = rk::wall_ms();
    if ((rc = size_columns(db, n))) return rc;
    if ((rc = rk::io_d2h(ctx, {{db->x_start.data(), L.fin.xs, n * 8},
                               {db->y_start.data(), L.fin.ys, n * 8},
                               {db->x_end.data(), L.fin.xe, n * 8},
                               {db->y_end.data(), L.fin.ye, n * 8},
                               {db->length.data(), L.fin.len, n * 8},
                               {db->score.data(), L.fin.score, n * 8},
                               {db->ident.data(), L.fin.ident, n * 8},
                               {db->similarity.data(), L.fin.sim, n * 4},
                               {db->strand.data(), L.fin.strand, n}})))
      return rc;
    st.d2h_ms = rk::wall_ms() - t;
    if (keep) {
      db->dev_block = kept.p;
      kept.p = nullptr;
      db->dev_x = L.fin.xs, db->dev_y = L.fin.ys, db->dev_len = L.fin.len;
      db->dev_strand = L.fin.strand;
      if (keep_rows) {
        db->dev_xe = L.fin.xe, db->dev_ye = L.fin.ye, db->dev_score = L.fin.score;
        db->dev_ident = L.fin.ident, db->dev_sim = L.fin.sim;
      }
    }
  }
  st.accepted = n;
  return RK_OK;
}

int load_device(rk_ctx *ctx, const char *path, uint32_t flags, rk_db **out) {
  const double t0 = rk::wall_ms();
  rk_ingress_stats &st = ctx->ingress;
  st = rk_ingress_stats{};
  Mapped m;
  int rc = map_file(path, &m);
  if (rc) return rc;
  std::unique_ptr<rk_db, void (*)(rk_db *)> db(new (std::nothrow) rk_db, rk_db_free);
  if (!db) return RK_E_NOMEM;
  const char *end = m.p + m.n;
  bool eof = false;
  const char *p = rk::db_read_header(db.get(), m.p, end, &eof);
  const uint64_t body_bytes = (!eof && p < end) ? (uint64_t)(end - p) : 0;
  st.body_bytes = body_bytes;
  Stream body;
  body.add(p, body_bytes, false);
  if ((rc = load_body(ctx, body, flags, db.get(), db->total_hdr, db->total_hdr, nullptr)))
    return rc;
  st.total_ms = rk::wall_ms() - t0;
  *out = db.release();
  return RK_OK;
}

// Every listed file mapped (descriptors closed as the work goes: a mapping does
// not need its own), its header read on the host, and the bodies parsed as one
// stream into one combined database.
int load_set(rk_ctx *ctx, const char *const *paths, uint32_t nsets, uint32_t flags,
             rk_dbset **out) {
  const double t0 = rk::wall_ms();
  rk_ingress_stats &st = ctx->ingress;
  st = rk_ingress_stats{};
  std::unique_ptr<rk_dbset, void (*)(rk_dbset *)> dbs(new (std::nothrow) rk_dbset,
                                                      rk_dbset_free);
  if (!dbs) return RK_E_NOMEM;
  dbs->db = new rk_db;
  std::vector<Mapped> maps(nsets);
  Stream body;
  SetIndex sets;
  dbs->set_off.assign((size_t)nsets + 1, 0);
  dbs->len_x_hdr.resize(nsets), dbs->len_y_hdr.resize(nsets), dbs->total_hdr.resize(nsets);
  dbs->header.resize(nsets);
  uint64_t bound = 0;
  for (uint32_t k = 0; k < nsets; ++k) {
    Mapped &m = maps[k];
    const int rc = map_file(paths[k], &m);
    if (m.fd >= 0) close(m.fd);
    m.fd = -1;
    if (rc) {
      ctx->err = "set " + std::to_string(k) + ": cannot open or map " + paths[k];
      return rc;
    }
    rk_db hdr;
    bool eof = false;
    const char *end = m.p + m.n;
    const char *p = rk::db_read_header(&hdr, m.p, end, &eof);
    const uint64_t len = (!eof && p < end) ? (uint64_t)(end - p) : 0;
    dbs->header[k].swap(hdr.header);
    dbs->len_x_hdr[k] = hdr.len_x_hdr, dbs->len_y_hdr[k] = hdr.len_y_hdr;
    dbs->total_hdr[k] = hdr.total_hdr;
    if (__builtin_add_overflow(bound, hdr.total_hdr, &bound)) bound = ~0ull;
    sets.first.push_back(body.size());
    // (a body that does not end in a newline gets one: getline yields the same
    // lines, and its last line cannot join the next file's first)
    body.add(p, len, len && p[len - 1] != '\n');
    st.body_bytes += len;
  }
  sets.host_off.assign(nsets, ~0ull);
  sets.total = dbs->total_hdr;
  // (one row of slack: a set over its total must reach the per-set check, not
  // the bound of the columns)
  if (bound != ~0ull) ++bound;
  const int rc = load_body(ctx, body, flags, dbs->db, ~0ull, bound, nsets ? &sets : nullptr);
  if (rc) return rc;
  const uint64_t n = dbs->db->x_start.size();
  for (uint32_t k = 0; k < nsets; ++k) dbs->set_off[k] = body.size() ? sets.host_off[k] : 0;
  dbs->set_off[nsets] = n;
  st.total_ms = rk::wall_ms() - t0;
  *out = dbs.release();
  return RK_OK;
}

}  // namespace

extern "C" int rk_db_load_csv_device(rk_ctx *ctx, const char *path, uint32_t flags, rk_db **out) {
  // flags: 0, RK_DB_KEEP_DEVICE or RK_DB_KEEP_ROWS (bit 1 alone keeps nothing to classify)
  if (!ctx || !path || !out || (flags & ~(uint32_t)RK_DB_KEEP_ROWS) || flags == 2) return RK_E_ARG;
  *out = nullptr;
  ctx->err.clear();
  try {
    return load_device(ctx, path, flags, out);
  } catch (const std::bad_alloc &) {
    ctx->err = "rk_db_load_csv_device: out of host memory";
    return RK_E_NOMEM;
  } catch (...) {
    ctx->err = "unexpected C++ exception";
    return RK_E_INTERNAL;
  }
}

extern "C" int rk_dbset_load_csv_device(rk_ctx *ctx, const char *const *paths, uint32_t nsets,
                                        uint32_t flags, rk_dbset **out) {
  if (!ctx || !out || (nsets && !paths) || (flags & ~(uint32_t)RK_DB_KEEP_ROWS) || flags == 2)
    return RK_E_ARG;
  for (uint32_t k = 0; k < nsets; ++k)
    if (!paths[k]) return RK_E_ARG;
  *out = nullptr;
  ctx->err.clear();
  try {
    return load_set(ctx, paths, nsets, flags, out);
  } catch (const std::bad_alloc &) {
    ctx->err = "rk_dbset_load_csv_device: out of host memory";
    return RK_E_NOMEM;
  } catch (...) {
    ctx->err = "unexpected C++ exception";
    return RK_E_INTERNAL;
  }
}

extern "C" void rk_dbset_free(rk_dbset *dbs) {
  if (!dbs) return;
  rk_db_free(dbs->db);
  delete dbs;
}

extern "C" int rk_dbset_view(const rk_dbset *dbs, uint32_t *nsets, const uint64_t **set_off,
                             const uint64_t **len_x_hdr, const uint64_t **len_y_hdr,
                             const uint64_t **total_hdr, rk_frags_soa *host, rk_frags_soa *dev) {
  if (!dbs) return RK_E_ARG;
  if (dev && rk_db_device_view(dbs->db, dev)) return RK_E_ARG;
  if (nsets) *nsets = (uint32_t)dbs->header.size();
  if (set_off) *set_off = dbs->set_off.data();
  if (len_x_hdr) *len_x_hdr = dbs->len_x_hdr.data();
  if (len_y_hdr) *len_y_hdr = dbs->len_y_hdr.data();
  if (total_hdr) *total_hdr = dbs->total_hdr.data();
  if (host) (void)rk_db_view(dbs->db, host, nullptr, nullptr, nullptr);
  return RK_OK;
}

extern "C" int rk_get_ingress_stats(const rk_ctx *ctx, rk_ingress_stats *st) {
  if (!ctx || !st) return RK_E_ARG;
  *st = ctx->ingress;
  return RK_OK;
}

extern "C" uint32_t rk_csv_max_line(void) { return RK_CSV_MAX_LINE; }
extern "C" uint32_t rk_csv_tile(void) { return TILE; }

// Classify `db` from its resident columns; dres[q] are DEVICE arrays carved
// from ctx->io (valid until the context's next call that stages through it).
// Returns with the stream idle.
int rk::db_classify_resident(rk_ctx *ctx, const rk_db *db, const double *len_ratio,
                             const double *pos_ratio, uint32_t npairs,
                             std::vector<rk_result> &dres) {
  rk_frags_soa dv;
  if (rk_db_device_view(db, &dv)) return RK_E_ARG;
  const size_t n = dv.n;
  if (n >= 0xFFFFFFFFull) return RK_E_TOO_MANY;
  // per pair gid, order (u32), rep (u8) out, as rk_classify_pairs stages them
  const size_t need = (size_t)npairs * (rk::align_up(n + 16) + rk::align_up(n * 4 + 16) * 2);
  int rc = grow(ctx, &ctx->io, &ctx->io_cap, need, "result staging");
  if (rc) return rc;
  rk::Carve c{(char *)ctx->io};
  dres.assign(npairs, rk_result{});
  std::vector<rk_params> ps(npairs);
  for (uint32_t q = 0; q < npairs; ++q) {
    uint8_t *drep = c.take<uint8_t>(n);
    uint32_t *dgid = c.take<uint32_t>(n), *dord = c.take<uint32_t>(n);
    dres[q] = rk_result{dord, dgid, drep, 0, 0};
    ps[q] = rk_params{db->len_x_hdr, db->len_y_hdr, len_ratio[q], pos_ratio[q]};
  }
  rc = rk_classify_device_pairs(ctx, &dv, ps.data(), npairs, dres.data());
  if (rc) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return RK_OK;
}

extern "C" int rk_classify_db_pairs(rk_ctx *ctx, const rk_db *db, const double *len_ratio,
                                    const double *pos_ratio, uint32_t npairs, rk_result *out) {
  if (!ctx || !db || !len_ratio || !pos_ratio || !out || npairs == 0) return RK_E_ARG;
  rk_frags_soa dv;
  if (rk_db_device_view(db, &dv)) return RK_E_ARG;
  ctx->err.clear();
  const size_t n = dv.n;
  if (n >= 0xFFFFFFFFull) return RK_E_TOO_MANY;
  for (uint32_t q = 0; q < npairs; ++q)
    if (n && (!out[q].gid || !out[q].repval || !out[q].out_order)) return RK_E_ARG;
  if (db->dev_device != ctx->device) {
    ctx->err = "rk_classify_db_pairs: the database's columns are on another device";
    return RK_E_ARG;
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  try {
    std::vector<rk_result> dres;
    int rc = rk::db_classify_resident(ctx, db, len_ratio, pos_ratio, npairs, dres);
    if (rc) return rc;
    const double t2 = rk::wall_ms();
    std::vector<rk::IoPiece> down;
    for (uint32_t q = 0; q < npairs; ++q) {
      out[q].n_out = dres[q].n_out;
      out[q].n_groups = dres[q].n_groups;
      const size_t k = n ? dres[q].n_out : 0;
      down.push_back({out[q].out_order, dres[q].out_order, k * 4});
      down.push_back({out[q].gid, dres[q].gid, k * 4});
      down.push_back({out[q].repval, dres[q].repval, k});
    }
    if ((rc = rk::io_d2h(ctx, down))) return rc;
    ctx->stats.h2d_ms = 0;
    ctx->stats.d2h_ms = rk::wall_ms() - t2;
    return RK_OK;
  } catch (...) {
    ctx->err = "unexpected C++ exception";
    return RK_E_INTERNAL;
  }
}
