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
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdlib>
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

struct Res {
  const uint32_t *order, *gid;
  const uint8_t *rep;
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

// rows [0, cnt) of the chunk (r is the chunk's slice of the result arrays)
__global__ __launch_bounds__(OB) void k_out_len(OCols c, uint64_t n, Res r, uint32_t cnt,
                                               uint8_t *len8, uint8_t *hst, uint32_t *blk_tot,
                                               Ctr *ctr) {
  __shared__ uint32_t lds[OB];
  const uint32_t k = blockIdx.x * OB + threadIdx.x;
  uint32_t len = 0;
  bool host = false;
  if (k < cnt) {
    const uint32_t i = r.order[k];
    if (i >= n) {
      atomicOr(&ctr->err, OERR_ORDER);
    } else {
      const rk::OutRow row = gather(c, i);
      host = rk::csv_row(row, r.gid[k], r.rep[k], nullptr, &len) == rk::ROW_HOST;
      if (host) len = 0;
    }
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

  // host rows of chunk [k0, k0 + cnt): list, format, upload, patch the lengths
  int fix_up(uint64_t k0, uint32_t cnt, uint32_t nhost, int par, uint64_t *added) {
    hipStream_t s = ctx->stream;
    const uint32_t nb = (cnt + OB - 1) / OB;
    const Res r{res.order + k0, res.gid + k0, res.rep + k0};
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

  // passes 1-4 of chunk c = rows [k0, k0 + cnt); returns with the put pass queued
  int format_chunk(uint64_t c, uint64_t k0, uint32_t cnt, Chunk *out) {
    hipStream_t s = ctx->stream;
    const int par = (int)(c & 1);
    const uint32_t nb = (cnt + OB - 1) / OB;
    const Res r{res.order + k0, res.gid + k0, res.rep + k0};
    HIPCHK(ctx, hipEventRecord(ev.e[0], s));
    HIPCHK(ctx, hipMemsetAsync(ctr, 0, sizeof(Ctr), s));
    k_out_len<<<nb, OB, 0, s>>>(cols, n, r, cnt, len8, hst, blk_tot, ctr);
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
      const int rc = fix_up(k0, cnt, (uint32_t)got.host_rows, par, &added);
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
    k_out_put<<<nb, OB, 0, s>>>(cols, r, cnt, len8, hst, poff, (const char *)patch[par].text,
                                blk_off, (char *)ctx->txt[par], bytes, perr);
    HIPCHK(ctx, hipEventRecord(ev.e[3 + 2 * par], s));
    HIPCHK(ctx, hipGetLastError());
    out->cnt = cnt;
    out->bytes = bytes;
    return RK_OK;
  }
};

int write_device(rk_ctx *ctx, const rk_db *db, const char *path, const rk_result *res,
                 uint32_t flags) {
  const double t0 = rk::wall_ms();
  rk_egress_stats &st = ctx->egress;
  st = rk_egress_stats{};
  // the file first, as the host route: an open failure does nothing else
  FdCloser f{::open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644)};
  if (f.fd < 0) return RK_E_IO;
  const uint64_t n = db->x_start.size(), n_out = res->n_out;
  if (n_out > 0xFFFFFFFFull || (n_out && n == 0)) return RK_E_ARG;
  bool ok = pwrite_all(f.fd, db->header.data(), db->header.size(), 0);
  uint64_t file_off = db->header.size();
  auto finish = [&](int rc) {
    const int fd = f.fd;
    f.fd = -1;
    if (::close(fd) != 0) ok = false;
    st.total_ms = rk::wall_ms() - t0;
    return rc ? rc : ok ? RK_OK : RK_E_IO;
  };
  if (!n_out || !ok) return finish(RK_OK);

  HIPCHK(ctx, hipSetDevice(ctx->device));
  Save S{ctx, db};
  S.cols = OCols{db->dev_x,     db->dev_y,     db->dev_xe,  db->dev_ye,    db->dev_len,
                 db->dev_score, db->dev_ident, db->dev_sim, db->dev_strand};
  S.n = n;
  S.st = &st;
  for (auto &e : S.ev.e) HIPCHK(ctx, hipEventCreate(&e));
  int rc;
  if (flags & RK_RES_DEVICE) {
    S.res = Res{res->out_order, res->gid, res->repval};
  } else {
    const double t = rk::wall_ms();
    rk::Carve pc{nullptr};
    pc.take<uint32_t>(n_out), pc.take<uint32_t>(n_out), pc.take<uint8_t>(n_out);
    if ((rc = rk::grow(ctx, &ctx->io, &ctx->io_cap, pc.off, "result upload"))) return rc;
    rk::Carve c{(char *)ctx->io};
    uint32_t *dord = c.take<uint32_t>(n_out), *dgid = c.take<uint32_t>(n_out);
    uint8_t *drep = c.take<uint8_t>(n_out);
    if ((rc = rk::io_h2d(ctx, {{res->out_order, dord, (size_t)n_out * 4},
                               {res->gid, dgid, (size_t)n_out * 4},
                               {res->repval, drep, (size_t)n_out}})))
      return rc;
    S.res = Res{dord, dgid, drep};
    st.upload_ms = rk::wall_ms() - t;
  }
  const uint32_t R = (uint32_t)std::min<uint64_t>(chunk_rows(), n_out);
  rk::Carve ps{nullptr};
  S.carve(ps, R);
  if ((rc = rk::grow(ctx, &ctx->ws, &ctx->ws_cap, ps.off, "csv rows out"))) return rc;
  rk::Carve cs{(char *)ctx->ws};
  S.carve(cs, R);

  const uint64_t nchunks = (n_out + R - 1) / R;
  auto rows_of = [&](uint64_t c) { return (uint32_t)std::min<uint64_t>(R, n_out - c * R); };
  hipStream_t s = ctx->stream;
  // on any failure below the stream is drained before the patch buffers go
  auto fail = [&](int code) {
    (void)hipStreamSynchronize(s);
    return finish(code);
  };
  HIPCHK(ctx, hipMemsetAsync(S.perr, 0, 4, s));
  Chunk cur, next;
  if ((rc = S.format_chunk(0, 0, rows_of(0), &cur))) return fail(rc);
  for (uint64_t c = 0; c < nchunks; ++c) {
    const int par = (int)(c & 1);
    // chunk c + 1 is formatted (the other text buffer) before chunk c's
    // download starts to wait: its put pass runs beside the copies and writes
    if (c + 1 < nchunks && (rc = S.format_chunk(c + 1, (c + 1) * R, rows_of(c + 1), &next)))
      return fail(rc);
    const double t = rk::wall_ms();
    const uint64_t at = file_off;
    rc = rk::io_d2h_sink(ctx, ctx->txt[par], (size_t)cur.bytes, S.ev.e[3 + 2 * par],
                         [&](const char *p, size_t len, size_t off) {
                           return pwrite_all(f.fd, p, len, at + off);
                         });
    st.d2h_write_ms += rk::wall_ms() - t;
    if (rc == 1) ok = false, rc = RK_OK;
    if (rc) return fail(rc);
    // the put pass of chunk c is complete (the copy stream waited for it)
    float ms = 0;
    HIPCHK(ctx, hipEventElapsedTime(&ms, S.ev.e[2 + 2 * par], S.ev.e[3 + 2 * par]));
    st.device_ms += ms;
    S.patch[par].release();
    file_off += cur.bytes;
    st.rows += cur.cnt;
    st.bytes += cur.bytes;
    ++st.chunks;
    cur = next;
    if (!ok) return fail(RK_OK);
  }
  HIPCHK(ctx, hipMemcpyAsync(ctx->host, S.perr, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  if (*ctx->host) {  // (the put pass' own error word, not a control block's)
    ctx->err = "csv put pass: a block's text does not fit its place";
    return finish(RK_E_INTERNAL);
  }
  return finish(RK_OK);
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

}  // namespace

extern "C" int rk_db_write_csv_device(rk_ctx *ctx, const rk_db *db, const char *path,
                                      const rk_result *res, uint32_t flags) {
  if (!ctx || !db || !path || !res || (flags & ~(uint32_t)RK_RES_DEVICE) ||
      (res->n_out && (!res->gid || !res->repval || !res->out_order)))
    return RK_E_ARG;
  ctx->err.clear();
  int rc = check_args(ctx, db, "rk_db_write_csv_device");
  if (rc) return rc;
  try {
    return write_device(ctx, db, path, res, flags);
  } catch (const std::bad_alloc &) {
    (void)hipStreamSynchronize(ctx->stream);
    ctx->err = "rk_db_write_csv_device: out of host memory";
    return RK_E_NOMEM;
  } catch (...) {
    (void)hipStreamSynchronize(ctx->stream);
    ctx->err = "unexpected C++ exception";
    return RK_E_INTERNAL;
  }
}

extern "C" int rk_classify_db_pairs_to_csv(rk_ctx *ctx, const rk_db *db, const double *len_ratio,
                                           const double *pos_ratio, uint32_t npairs,
                                           const char *const *paths, uint64_t *n_out,
                                           uint64_t *n_groups) {
  if (!ctx || !db || !len_ratio || !pos_ratio || !paths || npairs == 0) return RK_E_ARG;
  for (uint32_t q = 0; q < npairs; ++q)
    if (!paths[q]) return RK_E_ARG;
  ctx->err.clear();
  int rc = check_args(ctx, db, "rk_classify_db_pairs_to_csv");
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  try {
    std::vector<rk_result> dres;
    if ((rc = rk::db_classify_resident(ctx, db, len_ratio, pos_ratio, npairs, dres))) return rc;
    for (uint32_t q = 0; q < npairs; ++q) {
      if (n_out) n_out[q] = dres[q].n_out;
      if (n_groups) n_groups[q] = dres[q].n_groups;
    }
    for (uint32_t q = 0; q < npairs; ++q)
      if ((rc = write_device(ctx, db, paths[q], &dres[q], RK_RES_DEVICE))) return rc;
    return RK_OK;
  } catch (const std::bad_alloc &) {
    (void)hipStreamSynchronize(ctx->stream);
    ctx->err = "rk_classify_db_pairs_to_csv: out of host memory";
    return RK_E_NOMEM;
  } catch (...) {
    (void)hipStreamSynchronize(ctx->stream);
    ctx->err = "unexpected C++ exception";
    return RK_E_INTERNAL;
  }
}

extern "C" int rk_get_egress_stats(const rk_ctx *ctx, rk_egress_stats *st) {
  if (!ctx || !st) return RK_E_ARG;
  *st = ctx->egress;
  return RK_OK;
}
