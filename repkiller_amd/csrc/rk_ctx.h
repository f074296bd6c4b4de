// rk_ctx.h -- the context object behind the C ABI and the host-side helpers
// shared by the single-device driver (rk_api.hip) and the sharded driver
// (rk_shard.hip).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "../../include/repkiller_amd.h"
#include "rk_csv_stream.h"
#include "rk_internal.h"

namespace rk {
struct IoEngine;  // rk_io.hip: copy stream, pinned staging ring, host copy threads
struct BatchState;  // rk_batch.hip: tables, scratch and events of rk_classify*_batch
// Device tables of the sub-batch being classified combined (rk_batch.hip): the
// record pipeline corrects the upward-probe codes of both axes with them
struct BatchTables {
  uint32_t nsets;
  const uint32_t *bkt_x, *bkt_y;  // window starts in 100-bp buckets, nsets + 1 each
  const uint32_t *mi_x, *mi_y;    // every set's own max_index (seq_size / 100)
};
}

// Grow-only device buffers of the sharded driver, one per slot (the exchange
// sizes are only known mid-call, so they cannot share the single carve).
struct rk_pool {
  std::vector<void *> ptr;
  std::vector<size_t> cap;
};

struct rk_ctx {
  int device = -1;
  bool nw_fell_back = false;  // the last record-pipeline call handed over to the generic one
  uint64_t readbacks = 0;     // readback() calls over the context's life (host waits)
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;             // Y-axis sort, overlapped with the X sweeps
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  hipEvent_t aux = nullptr;  // sharded driver: the X bucket order is ready (stream 2)
  void *ws = nullptr;  // device workspace
  size_t ws_cap = 0;
  void *ws_wide = nullptr;  // 64-bit length columns, only when a length is >= 2^31
  size_t ws_wide_cap = 0;
  int pipeline = RK_PIPELINE_AUTO;
  void *ws_nw = nullptr;  // workspace of the record pipeline (rk_narrow.hip)
  size_t ws_nw_cap = 0;
  void *nw_small = nullptr;  // its control words + digit histograms: allocated once, so
                             // the pack check runs before the workspace is sized
  uint32_t *host = nullptr;  // pinned readback words (HOST_WORDS, rk_ctrl.h)
  // device copies for rk_classify (host-buffer entry point)
  void *io = nullptr;
  size_t io_cap = 0;
  rk::IoEngine *ioe = nullptr;
  rk_pool pool;  // rk_classify_sharded buffers
  rk::BatchState *batch = nullptr;  // rk_classify*_batch buffers
  // non-null only while a batch's combined set is being classified
  const rk::BatchTables *batch_tables = nullptr;
  rk_batch_stats batch_stats{};
  rk_ingress_stats ingress{};  // the last rk_db_load_csv_device (rk_csv.hip)
  rk_egress_stats egress{};    // the last rk_db_write_csv_device (rk_csv_out.hip)
  void *txt[2] = {};           // its two chunk text buffers, grow-only
  size_t txt_cap[2] = {};
  rk_select_stats select{};    // the last rk_*_select (rk_select.hip)
  void *sel = nullptr;         // the selected result of the *_to_csv_keep routes, grow-only
  size_t sel_cap = 0;
  // the sharded driver's fast path (rk_shard_fast.h): its all-gather messages
  // (pinned, every rank's), the stage fingerprints of the last call that
  // completed on it (a stage whose gathered counts match needs no agreement
  // before its exchanges: every buffer it takes already has its size), and the
  // sweeps it queues per axis before one deferred pending check
  char *sh_msg = nullptr;
  size_t sh_msg_cap = 0;
  uint64_t sh_fp[8] = {};
  uint32_t sh_blind[2] = {3, 3};
  rk_stats stats{};
  rk_shard_stats shard_stats{};
  std::string err;
  // phase profiling (rk_set_profiling): one event per phase boundary, on the
  // context stream, accumulated over calls until rk_reset_phases
  bool profiling = false;
  hipEvent_t pev[RK_N_PHASES + 1] = {};
  bool pev_used[RK_N_PHASES + 1] = {};
  double phase_ms[RK_N_PHASES] = {};
  uint32_t phase_calls[RK_N_PHASES] = {};
  rk::KernelTimer kt{};   // timed launches of the current call
  double kt_ms[rk::KID_COUNT] = {}, kt_bytes[rk::KID_COUNT] = {};
  uint64_t kt_launches[rk::KID_COUNT] = {};
};

struct rk_db;

namespace rk {

// rk_csv.hip: the body of rk_classify_db_pairs up to the download
int db_classify_resident(rk_ctx *ctx, const rk_db *db, const double *len_ratio,
                         const double *pos_ratio, uint32_t npairs, std::vector<rk_result> &dres);

// rk_select.hip: the stable selection by repeat flag of device arrays in
// rk_batch_result layout (set k owns slots [off[k], off[k] + n_out[k]), off and
// n_out HOST arrays); kept[k] (HOST) = rows of set k written to `out` from
// off[k] on.  Returns with the stream idle.
int select_device(rk_ctx *ctx, uint32_t nsets, const uint64_t *off, const uint64_t *n_out,
                  const uint32_t *order, const uint32_t *gid, const uint8_t *rep, uint32_t keep,
                  uint32_t *out_order, uint32_t *out_gid, uint8_t *out_rep, uint64_t *kept);

#define HIPCHK(ctx, call)                                                          \
  do {                                                                             \
    hipError_t e_ = (call);                                                        \
    if (e_ != hipSuccess) {                                                        \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);              \
      return RK_E_HIP;                                                             \
    }                                                                              \
  } while (0)

constexpr size_t ALIGN = 256;
inline size_t align_up(size_t v) { return (v + ALIGN - 1) & ~(ALIGN - 1); }

// bump allocator over a workspace (sizes first with a null base, then pointers)
struct Carve {
  char *base;
  size_t off = 0;
  template <class T>
  T *take(size_t count) {
    T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
    off += align_up(count * sizeof(T) + 16);  // +16: uint4 tails of the scan
    return p;
  }
};

// rk_io.hip: host <-> device pieces of rk_classify on the copy stream
// (pinned host buffers by DMA, pageable ones through the staging ring);
// both return when the transfer is complete
struct IoPiece {
  void *host;
  void *dev;
  size_t bytes;
};
int io_h2d(rk_ctx *ctx, const std::vector<IoPiece> &pieces);
int io_d2h(rk_ctx *ctx, const std::vector<IoPiece> &pieces);
// (rk_csv_stream.h: host pieces read as one byte stream)
// stream bytes [a, a + bytes) to dev: the host threads gather every staging
// slot from however many pieces it spans, so thousands of small pieces cost
// one DMA per slot, not one each; returns when the last byte has landed
int io_h2d_gather(rk_ctx *ctx, const IoStream &s, uint64_t a, uint64_t bytes, void *dev);
// device -> consumer: `bytes` bytes at dev come down through the pinned slots
// and each filled slot goes to sink(data, len, off) (off: the slot's offset in
// the piece) on a writer pool of at most 4 threads; a slot is issued again only
// after its sink call has returned.  Before the first copy the copy stream
// waits for `ready` (null: nothing to wait for).  Returns when every sink call
// has; 1 when a sink call returned false (the rest are then skipped).
int io_d2h_sink(rk_ctx *ctx, const void *dev, size_t bytes, hipEvent_t ready,
                const std::function<bool(const char *, size_t, size_t)> &sink);
// the rows of a host SoA as 12-B wire records {xStart lo, yStart lo, length
// (24) | reverse (1) | yStart >> 32 (3) | xStart >> 32 (4)} at `dev`, packed by
// the host threads into the staging ring; 1 when some row does not fit
// (length >= 2^24, yStart >= 2^35 or xStart >= 2^36)
int io_h2d_rows(rk_ctx *ctx, const rk_frags_soa &in, void *dev);
// gid[k] = (rows j <= k with flag[j] != 2) - 1: a new group starts at every
// row whose repeat flag is not 2; on `threads` threads of its own, started
// now and joined by job.wait(), so it runs beside a transfer that keeps the
// host pool busy
struct GidJob {
  std::vector<std::thread> th;
  void wait() {
    for (auto &t : th) t.join();
    th.clear();
  }
  ~GidJob() { wait(); }
};
void gids_from_flags_async(const uint8_t *flag, size_t n, uint32_t *gid, int threads, GidJob &job);
void io_destroy(rk_ctx *ctx);
// the NUMA nodes of the last upload (rk_stats numa_*)
void io_numa_stats(const rk_ctx *ctx, rk_stats *st);
// a call without an upload of its own: every NUMA field unknown (-1)
inline void stats_numa_unknown(rk_stats *st) {
  st->numa_input = st->numa_threads = st->numa_staging = st->numa_gpu = -1;
}
bool host_pinned(const void *p);
// rk_csv.hip: hipMalloc with the failure put in ctx->err (RK_E_NOMEM / RK_E_HIP),
// and one of the context's grow-only buffers brought to at least `need` bytes
int dev_alloc(rk_ctx *ctx, void **p, size_t bytes, const char *what);
int grow(rk_ctx *ctx, void **buf, size_t *cap, size_t need, const char *what);
double wall_ms();

// copy `count` (<= HOST_WORDS) device words into ctx->host and wait
int readback(rk_ctx *ctx, const uint32_t *dev, uint32_t count);
// fold the launches timed during the current call into the per-kernel totals
void collect_kernel_timing(rk_ctx *ctx);
// device error bits (ERRB_*) -> status + message
int err_status(rk_ctx *ctx, uint32_t bits);

// rk_batch.hip: the per-set upward-probe guards of a combined set's axis
// (c < max_index, c < max_index - 1 compare a position with the SET's bucket
// count, SequenceOcupationList.cpp:58,80), rewritten into the CSR's nbd bytes
void batch_nbd(const BatchTables &t, bool y_axis, const Csr &c, uint32_t m, uint32_t nb,
               hipStream_t st);
void batch_destroy(rk_ctx *ctx);

// Device scratch of the occupancy sweeps for an axis of up to m entries.
struct SweepScratch {
  uint32_t *runs;      // runs_scratch_words(m)
  uint8_t *wpend;      // m / 64 + 1
  uint8_t *rpend;      // m
  uint32_t *counters;  // PEND_WORDS
  uint32_t *dev_count; // 1
};
// run sweeps on one axis until no bucket has undecided entries
int resolve_axis(rk_ctx *ctx, const Axis &ax, SweepScratch sc, bool fast32, uint32_t *sweeps);
// `sweeps` sweeps of a 32-bit axis with no host round trip; *pend = 1 (device,
// when pend is given) when entries are still undecided after them.  junk:
// PEND_WORDS words the sweeps before the last count into, sc.counters then
// already zero (no clear per sweep); null: every sweep clears sc.counters
int resolve_axis_queued(rk_ctx *ctx, const Axis &ax, SweepScratch sc, uint32_t sweeps,
                        uint32_t *pend, uint32_t *junk = nullptr);

}  // namespace rk
