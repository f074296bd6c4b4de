// rk_repkiller -- command-line driver with the reference's interface
// (/root/reference/src/repkiller.cpp:26-97, commonFunctions.cpp:3-30):
//
//   rk_repkiller <input.csv> <output.csv> <len_ratio> <pos_ratio> [<len_ratio> <pos_ratio>]...
//
// Loads the CSV once (FragmentsDatabase), classifies every (len_ratio,
// pos_ratio) pair on the GPU and hands each result to the SaverQueue writer.
// Like the reference, every pair writes the same output path; here the pairs
// run in order, so the LAST pair's result is the file left behind (the
// reference's 3-thread pool makes that nondeterministic).
// Differences kept deliberately: an odd number of ratio arguments is a usage
// error (the reference throws std::out_of_range and aborts), and every failure
// exits non-zero with a message instead of std::terminate.
//
// Options (before the positional arguments): --device N, --timing (phase
// times as one JSON line on stderr), --gpus P (one fragment set sharded over
// P GPUs, devices N..N+P-1, one thread each: rk_classify_sharded over RCCL),
// --same-device (all P ranks on device N -- a rehearsal of the sharded path
// on one GPU), --comm rccl|local (collectives: RCCL, or in-process device
// copies; default rccl, local with --same-device), --save-soa PATH (after the
// parse, keep the database as a binary SoA cache), --soa (the input is such a
// cache: no parse at all), --device-parse (the CSV body is
// parsed on the GPU, rk_db_load_csv_device, and every pair is classified from
// the columns that stay resident there: no second upload; --timing then adds
// the ingress legs; not with --soa or --gpus above 1; with --batch see below), --device-save
// (only with --device-parse: all nine columns stay resident, RK_DB_KEEP_ROWS,
// and every pair's output is formatted on the GPU and written from its staging
// slots, rk_classify_db_pairs_to_csv: the result arrays never reach the host;
// an output path that cannot be opened falls back to represults-<k>.csv as the
// saver thread does; --timing then adds the egress legs).
//
//   rk_repkiller --batch <list> <len_ratio> <pos_ratio>
//
// <list> holds one "input.csv<TAB>output.csv" per line: the inputs are loaded
// (at most 16 threads), classified together by ONE rk_classify_batch call and
// each output written as a run of its own would write it.
//
//   rk_repkiller --batch <list> --device-parse [--device-save] [--timing] <len_ratio> <pos_ratio>
//
// The listed CSVs are parsed on the GPU as one byte stream into one combined
// resident database (rk_dbset_load_csv_device) and classified from there
// (rk_classify_dbset, then the host save per file); with --device-save the
// outputs are formatted on the GPU too and every set's text goes to its own
// file (rk_classify_dbset_to_csv).  --timing prints the ingress, batch and
// egress stats as one JSON line on stderr.
//
// --keep all|unique|repeated|groups|<1..7> (every route that writes a CSV):
// only the rows whose repeat flag is in the mask are written (bit 0 singletons,
// bit 1 representatives, bit 2 repeated rows; unique = 3 is the repeat-free
// set, one row per group; groups = 6; all = 7, the default).  The header is
// echoed unchanged and group ids are not renumbered.  The host routes select
// on the host between the classification and the writer (rk_result_select);
// --device-save selects on the GPU (the *_to_csv_keep entry points).  --timing
// then adds the select stats.
#include <atomic>
#include <chrono>
#include <fstream>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "repkiller_amd.h"

static void print_help() {
  std::printf("Repkiller (MI355X) v0.9.b-compatible\n");
  std::printf("Usage: ./rk_repkiller [--device N] [--gpus P [--same-device] [--comm rccl|local]] "
              "[--timing] [--keep all|unique|repeated|groups|<1..7>] [--save-soa cache.soa | --soa | --device-parse [--device-save]] <input_file_path> <output_file_path> "
              "<length_ratio> <position_ratio> [<length_ratio> <position_ratio>]...\n");
  std::printf("       ./rk_repkiller [--device N] [--keep MASK] --batch <list of input<TAB>output lines> "
              "[--device-parse [--device-save] [--timing]] <length_ratio> <position_ratio>\n");
  std::fflush(stdout);
}

static double now_s() {
  using namespace std::chrono;
  return duration<double>(steady_clock::now().time_since_epoch()).count();
}

static bool parse_keep(const char *s, uint32_t *keep) {
  if (!std::strcmp(s, "all")) return *keep = RK_KEEP_ALL, true;
  if (!std::strcmp(s, "unique")) return *keep = RK_KEEP_UNIQUE, true;
  if (!std::strcmp(s, "repeated")) return *keep = RK_KEEP_REPEATED, true;
  if (!std::strcmp(s, "groups")) return *keep = RK_KEEP_REPRESENTATIVE | RK_KEEP_REPEATED, true;
  char *end = nullptr;
  const unsigned long v = std::strtoul(s, &end, 10);
  if (end == s || *end || v < 1 || v > RK_KEEP_ALL || s[0] < '0' || s[0] > '9') return false;
  *keep = (uint32_t)v;
  return true;
}

// the select stats of a run: summed over its selections
struct SelectTotals {
  rk_select_stats st{};
  // a host selection of `in` (host arrays) that kept `kept` rows: the rows by
  // flag are counted here, with or without a context
  void add(const rk_result &in, uint64_t kept) {
    st.rows_in += in.n_out, st.kept += kept, st.sets += 1;
    for (uint64_t k = 0; k < in.n_out; ++k) ++st.by_flag[in.repval[k] < 3 ? in.repval[k] : 3];
  }
  void from(const rk_ctx *ctx) { rk_get_select_stats(ctx, &st); }
  void print(const char *open, const char *close) const {
    std::fprintf(stderr,
                 "%s\"select\": {\"rows_in\": %llu, \"by_flag\": [%llu, %llu, %llu, %llu], "
                 "\"kept\": %llu, \"sets\": %u, \"device_ms\": %.3f}%s",
                 open, (unsigned long long)st.rows_in, (unsigned long long)st.by_flag[0],
                 (unsigned long long)st.by_flag[1], (unsigned long long)st.by_flag[2],
                 (unsigned long long)st.by_flag[3], (unsigned long long)st.kept, st.sets,
                 st.device_ms, close);
  }
};

// the host selection of one result: *r becomes the kept rows, held in `own`,
// which must outlive it (keep all: r is left as it is)
struct Selected {
  std::vector<uint32_t> order, gid;
  std::vector<uint8_t> rep;
};
static int select_host_result(rk_ctx *ctx, uint32_t keep, rk_result *r, Selected *own,
                              SelectTotals *tot) {
  if (keep == RK_KEEP_ALL) return RK_OK;
  own->order.resize(r->n_out), own->gid.resize(r->n_out), own->rep.resize(r->n_out);
  rk_result out{own->order.data(), own->gid.data(), own->rep.data(), 0, 0};
  const int rc = rk_result_select(ctx, r, keep, 0, &out);
  if (rc) return rc;
  tot->add(*r, out.n_out);
  *r = out;
  return RK_OK;
}

static bool parse_ratio(const char *s, double *v) {
  char *end = nullptr;
  *v = std::strtod(s, &end);
  return end != s;
}

// One fragment set over `gpus` ranks, one thread each; every pair in turn.
// The ranks hold consecutive blocks of rows; each copies its output share into
// the full result arrays at its offset.
static int classify_sharded_threads(const rk_frags_soa &soa, int device, int gpus,
                                    bool same_device, bool local, const std::vector<rk_params> &ps,
                                    std::vector<rk_result> &rs, std::string &err) {
  std::vector<rk_comm *> comms(gpus, nullptr);
  uint8_t id[RK_COMM_ID_BYTES];
  if (local) {
    if (rk_comm_create_local(gpus, comms.data())) {
      err = "rk_comm_create_local failed";
      return 1;
    }
  } else if (rk_comm_rccl_id(id)) {
    err = "RCCL is not available";
    return 1;
  }
  std::vector<int> status(gpus, 0);
  std::vector<std::string> msgs(gpus);
  std::vector<std::thread> th;
  for (int r = 0; r < gpus; ++r)
    th.emplace_back([&, r] {
      const int dev = same_device ? device : device + r;
      if (!local && rk_comm_create_rccl(r, gpus, dev, id, &comms[r])) {
        status[r] = RK_E_HIP;
        msgs[r] = "rk_comm_create_rccl failed";
        return;
      }
      rk_ctx *ctx = nullptr;
      if ((status[r] = rk_create(&ctx, dev))) {
        msgs[r] = "no usable gfx950 device " + std::to_string(dev);
        // the peers' first pair waits for this rank: release them
        (void)rk_comm_abandon(comms[r], status[r]);
        return;
      }
      const uint64_t a = soa.n * (uint64_t)r / gpus, b = soa.n * (uint64_t)(r + 1) / gpus;
      const rk_frags_soa mine{soa.x_start + a, soa.y_start + a, soa.length + a,
                              soa.strand + a, b - a};
      for (size_t i = 0; i < ps.size() && !status[r]; ++i) {
        rk_shard_result res;
        status[r] = rk_classify_sharded_host(ctx, comms[r], &mine, &ps[i], -1, &res);
        if (!status[r])
          status[r] = rk_shard_copy_result(ctx, &res, rs[i].out_order + res.out_offset,
                                           rs[i].gid + res.out_offset,
                                           rs[i].repval + res.out_offset);
        if (status[r]) msgs[r] = rk_last_error(ctx);
        if (r == 0 && !status[r]) rs[i].n_out = res.n_out_total, rs[i].n_groups = res.n_groups;
      }
      rk_destroy(ctx);
    });
  for (auto &t : th) t.join();
  for (rk_comm *c : comms) rk_comm_destroy(c);
  for (int r = 0; r < gpus; ++r)
    if (status[r]) {
      err = "rank " + std::to_string(r) + ": " + msgs[r] + " (" + std::to_string(status[r]) + ")";
      return status[r];
    }
  return 0;
}

static bool read_batch_list(const char *list_path, std::vector<std::string> &ins,
                            std::vector<std::string> &outs) {
  std::ifstream lf(list_path);
  if (!lf) {
    std::fprintf(stderr, "Could not open batch list %s.\n", list_path);
    return false;
  }
  for (std::string line; std::getline(lf, line);) {
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.empty()) continue;
    const size_t tab = line.find('\t');
    if (tab == std::string::npos || tab == 0 || tab + 1 == line.size()) {
      std::fprintf(stderr, "Batch list line without input<TAB>output: %s\n", line.c_str());
      return false;
    }
    ins.push_back(line.substr(0, tab));
    outs.push_back(line.substr(tab + 1));
  }
  return true;
}

// --batch --device-parse [--device-save]: the listed CSVs parsed on the GPU into
// one combined resident database, classified from there; the outputs written by
// the host per file, or formatted on the GPU too
static int run_batch_device(const char *list_path, double lr, double pr, int device,
                            bool device_save, bool timing, uint32_t keep) {
  std::vector<std::string> ins, outs;
  if (!read_batch_list(list_path, ins, outs)) return 1;
  const size_t ns = ins.size();
  std::printf("--- Running REPKILLER (MI355X), %zu fragment sets ---\n\n", ns);
  std::fflush(stdout);
  rk_ctx *ctx = nullptr;
  int rc = rk_create(&ctx, device);
  if (rc) {
    std::fprintf(stderr, "no usable gfx950 device %d (%d)\n", device, rc);
    return 1;
  }
  std::vector<const char *> ip(ns), op(ns);
  for (size_t k = 0; k < ns; ++k) ip[k] = ins[k].c_str(), op[k] = outs[k].c_str();
  rk_dbset *dbs = nullptr;
  const double t0 = now_s();
  rc = rk_dbset_load_csv_device(ctx, ip.data(), (uint32_t)ns,
                                device_save ? (uint32_t)RK_DB_KEEP_ROWS
                                            : (uint32_t)RK_DB_KEEP_DEVICE,
                                &dbs);
  const double t1 = now_s();
  auto fail = [&](const char *what) {
    std::fprintf(stderr, "%s failed (%d): %s\n", what, rc, rk_last_error(ctx));
    rk_dbset_free(dbs);
    rk_destroy(ctx);
    return 1;
  };
  if (rc == RK_E_COUNT) std::fprintf(stderr, "Unexpected number of fragments\n");
  if (rc) return fail("device parse");
  uint32_t nsets = 0;
  const uint64_t *off = nullptr;
  rk_dbset_view(dbs, &nsets, &off, nullptr, nullptr, nullptr, nullptr, nullptr);
  const uint64_t n = off[nsets];
  std::vector<uint64_t> n_out(ns + 1), n_groups(ns + 1);
  SelectTotals sel;
  double t2;
  if (device_save) {
    rc = rk_classify_dbset_to_csv_keep(ctx, dbs, lr, pr, op.data(), keep, n_out.data(),
                                       n_groups.data(), nullptr);
    t2 = now_s();
    if (rc) return fail("classification or device save");
    if (keep != RK_KEEP_ALL) sel.from(ctx);
  } else {
    std::vector<uint32_t> gid(n), order(n);
    std::vector<uint8_t> rep(n);
    rk_batch_result br{order.data(), gid.data(), rep.data(), n_out.data(), n_groups.data()};
    rc = rk_classify_dbset(ctx, dbs, lr, pr, &br);
    if (rc) return fail("classification");
    std::vector<uint32_t> sgid, sorder;
    std::vector<uint8_t> srep;
    std::vector<uint64_t> kept(ns + 1);
    if (keep != RK_KEEP_ALL) {
      sgid.resize(n), sorder.resize(n), srep.resize(n);
      rk_batch_result sb{sorder.data(), sgid.data(), srep.data(), kept.data(), nullptr};
      rc = rk_batch_result_select(ctx, nsets, off, &br, keep, 0, &sb);
      if (rc) return fail("selection");
      sel.from(ctx);
      order.swap(sorder), gid.swap(sgid), rep.swap(srep), n_out.swap(kept);
    }
    for (size_t k = 0; k < ns && !rc; ++k) {
      const rk_result r{order.data() + off[k], gid.data() + off[k], rep.data() + off[k], n_out[k],
                        n_groups[k]};
      if ((rc = rk_dbset_write_csv(dbs, (uint32_t)k, outs[k].c_str(), &r)))
        std::fprintf(stderr, "writing %s failed (%d)\n", outs[k].c_str(), rc);
    }
    t2 = now_s();
    if (rc) return fail("host save");
  }
  if (timing) {
    rk_ingress_stats ing{};
    rk_get_ingress_stats(ctx, &ing);
    rk_batch_stats bs{};
    rk_get_batch_stats(ctx, &bs);
    rk_egress_stats eg{};
    rk_get_egress_stats(ctx, &eg);
    std::fprintf(stderr,
                 "{\"sets\": %zu, \"frags\": %llu, \"load_s\": %.6f, \"classify_save_s\": %.6f, "
                 "\"ingress\": {\"body_bytes\": %llu, \"lines\": %llu, \"accepted\": %llu, "
                 "\"host_lines\": %llu, \"windows\": %u, \"h2d_ms\": %.3f, \"device_ms\": %.3f, "
                 "\"host_fix_ms\": %.3f, \"d2h_ms\": %.3f, \"total_ms\": %.3f}, "
                 "\"batch\": {\"sub_batches\": %u, \"looped_sets\": %u, \"batched_sets\": %u, "
                 "\"device_ms\": %.3f}, "
                 "\"egress\": {\"rows\": %llu, \"bytes\": %llu, \"host_rows\": %llu, "
                 "\"chunks\": %u, \"upload_ms\": %.3f, \"device_ms\": %.3f, "
                 "\"host_fix_ms\": %.3f, \"d2h_write_ms\": %.3f, \"total_ms\": %.3f}",
                 ns, (unsigned long long)n, t1 - t0, t2 - t1, (unsigned long long)ing.body_bytes,
                 (unsigned long long)ing.lines, (unsigned long long)ing.accepted,
                 (unsigned long long)ing.host_lines, ing.windows, ing.h2d_ms, ing.device_ms,
                 ing.host_fix_ms, ing.d2h_ms, ing.total_ms, bs.sub_batches, bs.looped_sets,
                 bs.batched_sets, bs.device_ms, (unsigned long long)eg.rows,
                 (unsigned long long)eg.bytes, (unsigned long long)eg.host_rows, eg.chunks,
                 eg.upload_ms, eg.device_ms, eg.host_fix_ms, eg.d2h_write_ms, eg.total_ms);
    if (keep != RK_KEEP_ALL) sel.print(", ", "}\n");
    else std::fprintf(stderr, "}\n");
  }
  rk_dbset_free(dbs);
  rk_destroy(ctx);
  std::printf("Repkiller finished with no errors\n");
  return 0;
}

// --batch: every listed CSV through one batched classification
static int run_batch(const char *list_path, double lr, double pr, int device, uint32_t keep) {
  std::vector<std::string> ins, outs;
  if (!read_batch_list(list_path, ins, outs)) return 1;
  const size_t ns = ins.size();
  std::printf("--- Running REPKILLER (MI355X), %zu fragment sets ---\n\n", ns);
  std::fflush(stdout);
  std::vector<rk_db *> dbs(ns, nullptr);
  std::vector<int> lrc(ns, 0);
  {
    std::atomic<size_t> next{0};
    std::vector<std::thread> th;
    const size_t nt = ns < 16 ? ns : 16;
    for (size_t t = 0; t < nt; ++t)
      th.emplace_back([&] {
        for (size_t k; (k = next++) < ns;) lrc[k] = rk_db_load_csv(ins[k].c_str(), &dbs[k]);
      });
    for (auto &t : th) t.join();
  }
  auto free_all = [&] {
    for (rk_db *d : dbs) rk_db_free(d);
  };
  for (size_t k = 0; k < ns; ++k)
    if (lrc[k]) {
      if (lrc[k] == RK_E_IO) std::fprintf(stderr, "Could not open input file %s.\n", ins[k].c_str());
      else if (lrc[k] == RK_E_COUNT) std::fprintf(stderr, "Unexpected number of fragments\n");
      else std::fprintf(stderr, "loading %s failed (%d)\n", ins[k].c_str(), lrc[k]);
      free_all();
      return 1;
    }
  std::vector<uint64_t> off(ns + 1, 0), hx(ns), hy(ns), n_out(ns), n_groups(ns);
  std::vector<rk_frags_soa> views(ns);
  for (size_t k = 0; k < ns; ++k) {
    uint64_t total;
    rk_db_view(dbs[k], &views[k], &hx[k], &hy[k], &total);
    off[k + 1] = off[k] + views[k].n;
  }
  const uint64_t n = off[ns];
  std::vector<uint64_t> x(n), y(n), len(n);
  std::vector<uint8_t> strand(n), rep(n);
  std::vector<uint32_t> gid(n), order(n);
  for (size_t k = 0; k < ns; ++k)
    if (views[k].n) {
      std::memcpy(x.data() + off[k], views[k].x_start, views[k].n * 8);
      std::memcpy(y.data() + off[k], views[k].y_start, views[k].n * 8);
      std::memcpy(len.data() + off[k], views[k].length, views[k].n * 8);
      std::memcpy(strand.data() + off[k], views[k].strand, views[k].n);
    }
  rk_ctx *ctx = nullptr;
  int rc = rk_create(&ctx, device);
  if (rc) {
    std::fprintf(stderr, "no usable gfx950 device %d (%d)\n", device, rc);
    free_all();
    return 1;
  }
  const rk_frags_soa soa{x.data(), y.data(), len.data(), strand.data(), n};
  const rk_batch_params bp{(uint32_t)ns, off.data(), hx.data(), hy.data(), lr, pr};
  rk_batch_result br{order.data(), gid.data(), rep.data(), n_out.data(), n_groups.data()};
  rc = rk_classify_batch(ctx, &soa, &bp, &br);
  if (rc) {
    std::fprintf(stderr, "classification failed (%d): %s\n", rc, rk_last_error(ctx));
    rk_destroy(ctx);
    free_all();
    return 1;
  }
  rk_destroy(ctx);
  SelectTotals sel;
  for (size_t k = 0; k < ns && !rc; ++k) {
    rk_result r{order.data() + off[k], gid.data() + off[k], rep.data() + off[k], n_out[k],
                n_groups[k]};
    Selected own;
    if ((rc = select_host_result(nullptr, keep, &r, &own, &sel))) {
      std::fprintf(stderr, "selection failed (%d)\n", rc);
      break;
    }
    if ((rc = rk_db_write_csv(dbs[k], outs[k].c_str(), &r)))
      std::fprintf(stderr, "writing %s failed (%d)\n", outs[k].c_str(), rc);
  }
  free_all();
  if (rc) return 1;
  std::printf("Repkiller finished with no errors\n");
  return 0;
}

int main(int argc, char **argv) {
  int device = 0, gpus = 1;
  bool timing = false, same_device = false, soa_in = false, device_parse = false;
  bool device_save = false;
  const char *comm_kind = nullptr, *save_soa = nullptr, *batch_list = nullptr;
  const char *keep_arg = nullptr;
  uint32_t keep = RK_KEEP_ALL;
  std::vector<const char *> pos;
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--device") && i + 1 < argc) device = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--gpus") && i + 1 < argc) gpus = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--comm") && i + 1 < argc) comm_kind = argv[++i];
    else if (!std::strcmp(argv[i], "--same-device")) same_device = true;
    else if (!std::strcmp(argv[i], "--timing")) timing = true;
    else if (!std::strcmp(argv[i], "--soa")) soa_in = true;
    else if (!std::strcmp(argv[i], "--device-parse")) device_parse = true;
    else if (!std::strcmp(argv[i], "--device-save")) device_save = true;
    else if (!std::strcmp(argv[i], "--save-soa") && i + 1 < argc) save_soa = argv[++i];
    else if (!std::strcmp(argv[i], "--batch") && i + 1 < argc) batch_list = argv[++i];
    else if (!std::strcmp(argv[i], "--keep") && i + 1 < argc) keep_arg = argv[++i];
    else pos.push_back(argv[i]);
  }
  if (keep_arg && !parse_keep(keep_arg, &keep)) {
    std::fprintf(stderr, "Invalid --keep value %s.\n", keep_arg);
    print_help();
    return 1;
  }
  if (gpus < 1 || gpus > 32 ||
      (comm_kind && std::strcmp(comm_kind, "rccl") && std::strcmp(comm_kind, "local"))) {
    std::fprintf(stderr, "Invalid --gpus / --comm.\n");
    print_help();
    return 1;
  }
  if (device_parse && (soa_in || gpus != 1)) {
    std::fprintf(stderr, "--device-parse does not combine with --soa or --gpus.\n");
    print_help();
    return 1;
  }
  if (device_save && !device_parse) {
    std::fprintf(stderr, "--device-save needs --device-parse.\n");
    print_help();
    return 1;
  }
  if (batch_list) {
    double lr, pr;
    if (pos.size() != 2 || !parse_ratio(pos[0], &lr) || !parse_ratio(pos[1], &pr) || lr <= 0 ||
        pr <= 0 || gpus != 1) {
      std::fprintf(stderr, "--batch takes a list file and one positive ratio pair.\n");
      print_help();
      return 1;
    }
    if (device_parse)
      return run_batch_device(batch_list, lr, pr, device, device_save, timing, keep);
    return run_batch(batch_list, lr, pr, device, keep);
  }
  const bool local = comm_kind ? !std::strcmp(comm_kind, "local") : same_device;
  // init_args (commonFunctions.cpp:14-29)
  if (pos.size() < 4 || (pos.size() - 2) % 2 != 0) {
    std::fprintf(stderr, "Invalid number of arguments.\n");
    print_help();
    return 1;
  }
  std::vector<std::pair<double, double>> params;
  for (size_t i = 2; i + 1 < pos.size(); i += 2) {
    double lr, pr;
    if (!parse_ratio(pos[i], &lr) || !parse_ratio(pos[i + 1], &pr)) {
      std::fprintf(stderr, "Invalid ratio argument.\n");
      print_help();
      return 1;
    }
    if (lr <= 0) {
      std::fprintf(stderr, "Ratio between length and position must be greater than zero\n");
      print_help();
      return 1;
    }
    if (pr <= 0) {
      std::fprintf(stderr, "Position proximity must be greater than zero\n");
      print_help();
      return 1;
    }
    params.emplace_back(lr, pr);
  }
  const std::string out_path = pos[1];
  if (out_path.empty()) {
    std::fprintf(stderr, "Output file name is missing\n");
    return 1;
  }

  std::printf("--- Running REPKILLER (MI355X) ---\n\n");
  std::fflush(stdout);
  double t0 = now_s();
  rk_db *db = nullptr;
  rk_ctx *ctx = nullptr;
  int rc;
  if (device_parse) {
    rc = rk_create(&ctx, device);
    if (rc) {
      std::fprintf(stderr, "no usable gfx950 device %d (%d)\n", device, rc);
      return 1;
    }
    const uint32_t keep = device_save ? (uint32_t)RK_DB_KEEP_ROWS : (uint32_t)RK_DB_KEEP_DEVICE;
    rc = rk_db_load_csv_device(ctx, pos[0], keep, &db);
    if (rc && rc != RK_E_IO && rc != RK_E_COUNT)
      std::fprintf(stderr, "device parse: %s\n", rk_last_error(ctx));
    if (rc) rk_destroy(ctx);
  } else {
    rc = soa_in ? rk_db_load_soa(pos[0], &db) : rk_db_load_csv(pos[0], &db);
  }
  if (rc == RK_E_ARG && soa_in) {
    std::fprintf(stderr, "%s is not a complete SoA cache file.\n", pos[0]);
    return 1;
  }
  if (rc == RK_E_IO) {
    std::fprintf(stderr, "Could not open input file %s.\n", pos[0]);
    return 1;
  }
  if (rc == RK_E_COUNT) {
    std::fprintf(stderr, "Unexpected number of fragments\n");
    return 1;
  }
  if (rc) {
    std::fprintf(stderr, "loading %s failed (%d)\n", pos[0], rc);
    return 1;
  }
  if (save_soa && (rc = rk_db_save_soa(db, save_soa))) {
    std::fprintf(stderr, "writing the SoA cache %s failed (%d)\n", save_soa, rc);
    rk_destroy(ctx);
    rk_db_free(db);
    return 1;
  }
  double t1 = now_s();
  rk_frags_soa soa;
  uint64_t lx, ly, total;
  rk_db_view(db, &soa, &lx, &ly, &total);

  if (gpus == 1 && !ctx) {
    rc = rk_create(&ctx, device);
    if (rc) {
      std::fprintf(stderr, "no usable gfx950 device %d (%d)\n", device, rc);
      rk_db_free(db);
      return 1;
    }
  }
  if (device_save) {
    // classification and egress in one call per run; the file left behind is the
    // last pair's, as below
    const size_t q = params.size();
    std::vector<double> lrs(q), prs(q);
    std::vector<const char *> paths(q, out_path.c_str());
    for (size_t i = 0; i < q; ++i) lrs[i] = params[i].first, prs[i] = params[i].second;
    const double a = now_s();
    rc = rk_classify_db_pairs_to_csv_keep(ctx, db, lrs.data(), prs.data(), (uint32_t)q,
                                          paths.data(), keep, nullptr, nullptr, nullptr);
    if (rc == RK_E_IO) {
      // the saver thread's rule, pair by pair (SaverQueue.cpp:16-20)
      size_t fallback_count = 0;
      rc = RK_OK;
      for (size_t i = 0; i < q && !rc; ++i) {
        const char *one = out_path.c_str();
        rc = rk_classify_db_pairs_to_csv_keep(ctx, db, &lrs[i], &prs[i], 1, &one, keep, nullptr,
                                              nullptr, nullptr);
        if (rc != RK_E_IO) continue;
        const std::string alt = "represults-" + std::to_string(++fallback_count) + ".csv";
        std::fprintf(stderr, "Couldn't access %s, saving into %s\n", out_path.c_str(),
                     alt.c_str());
        one = alt.c_str();
        rc = rk_classify_db_pairs_to_csv_keep(ctx, db, &lrs[i], &prs[i], 1, &one, keep, nullptr,
                                              nullptr, nullptr);
      }
    }
    const double t_all = now_s() - a;
    if (rc) {
      std::fprintf(stderr, "classification or device save failed (%d): %s\n", rc,
                   rk_last_error(ctx));
      rk_destroy(ctx);
      rk_db_free(db);
      return 1;
    }
    rk_stats stt{};
    rk_get_stats(ctx, &stt);
    rk_ingress_stats ing{};
    rk_get_ingress_stats(ctx, &ing);
    rk_egress_stats eg{};
    rk_get_egress_stats(ctx, &eg);
    SelectTotals sel;
    sel.from(ctx);  // the last pair's, as the egress stats
    rk_destroy(ctx);
    if (timing && keep != RK_KEEP_ALL) sel.print("{", "}\n");
    if (timing) {
      std::fprintf(stderr,
                   "{\"ingress\": {\"body_bytes\": %llu, \"lines\": %llu, \"accepted\": %llu, "
                   "\"host_lines\": %llu, \"windows\": %u, \"h2d_ms\": %.3f, \"device_ms\": %.3f, "
                   "\"host_fix_ms\": %.3f, \"d2h_ms\": %.3f, \"total_ms\": %.3f}}\n",
                   (unsigned long long)ing.body_bytes, (unsigned long long)ing.lines,
                   (unsigned long long)ing.accepted, (unsigned long long)ing.host_lines,
                   ing.windows, ing.h2d_ms, ing.device_ms, ing.host_fix_ms, ing.d2h_ms,
                   ing.total_ms);
      std::fprintf(stderr,
                   "{\"egress\": {\"rows\": %llu, \"bytes\": %llu, \"host_rows\": %llu, "
                   "\"chunks\": %u, \"upload_ms\": %.3f, \"device_ms\": %.3f, "
                   "\"host_fix_ms\": %.3f, \"d2h_write_ms\": %.3f, \"total_ms\": %.3f}}\n",
                   (unsigned long long)eg.rows, (unsigned long long)eg.bytes,
                   (unsigned long long)eg.host_rows, eg.chunks, eg.upload_ms, eg.device_ms,
                   eg.host_fix_ms, eg.d2h_write_ms, eg.total_ms);
      std::fprintf(stderr,
                   "{\"frags\": %llu, \"pairs\": %zu, \"load_s\": %.6f, "
                   "\"classify_save_s\": %.6f, \"device_ms\": %.3f, \"gpus\": %d}\n",
                   (unsigned long long)soa.n, params.size(), t1 - t0, t_all, stt.device_ms, gpus);
    }
    rk_db_free(db);
    std::printf("Repkiller finished with no errors\n");
    return 0;
  }
  rk_saver *sq = nullptr;
  rk_saver_start(db, &sq);
  // every pair over the one fragment set in one call: the ratio-independent
  // work (processing order, occupancy axes, sort keys) is shared
  const size_t q = params.size();
  std::vector<uint32_t> gid(q * soa.n), order(q * soa.n);
  std::vector<uint8_t> rep(q * soa.n);
  std::vector<rk_params> ps(q);
  std::vector<rk_result> rs(q);
  for (size_t i = 0; i < q; ++i) {
    ps[i] = rk_params{lx, ly, params[i].first, params[i].second};
    rs[i] = rk_result{order.data() + i * soa.n, gid.data() + i * soa.n, rep.data() + i * soa.n,
                      0, 0};
  }
  double a = now_s();
  std::string err;
  if (device_parse) {
    std::vector<double> lrs(q), prs(q);
    for (size_t i = 0; i < q; ++i) lrs[i] = params[i].first, prs[i] = params[i].second;
    rc = rk_classify_db_pairs(ctx, db, lrs.data(), prs.data(), (uint32_t)q, rs.data());
    if (rc) err = rk_last_error(ctx);
  } else if (gpus == 1) {
    rc = rk_classify_pairs(ctx, &soa, ps.data(), (uint32_t)q, rs.data());
    if (rc) err = rk_last_error(ctx);
  } else {
    rc = classify_sharded_threads(soa, device, gpus, same_device, local, ps, rs, err);
  }
  const double t_class = now_s() - a;
  if (rc) {
    std::fprintf(stderr, "classification failed (%d): %s\n", rc, err.c_str());
    rk_saver_stop(sq);
    rk_destroy(ctx);
    rk_db_free(db);
    return 1;
  }
  rk_stats stt{};
  if (ctx) rk_get_stats(ctx, &stt);
  const double dev_ms = stt.device_ms;
  // the selection of every pair's result on the host, then the saver thread as
  // it is (its fall-back file included)
  SelectTotals sel;
  for (size_t i = 0; i < q && !rc; ++i) {
    Selected own;
    rk_result r = rs[i];
    if ((rc = select_host_result(ctx, keep, &r, &own, &sel))) break;
    rk_saver_add(sq, out_path.c_str(), &r, soa.n);
  }
  if (rc) {
    std::fprintf(stderr, "selection failed (%d)\n", rc);
    rk_saver_stop(sq);
    rk_destroy(ctx);
    rk_db_free(db);
    return 1;
  }
  double t2 = now_s();
  rc = rk_saver_stop(sq);
  double t3 = now_s();
  rk_ingress_stats ing{};
  if (device_parse) rk_get_ingress_stats(ctx, &ing);
  rk_destroy(ctx);
  if (timing && device_parse)
    std::fprintf(stderr,
                 "{\"ingress\": {\"body_bytes\": %llu, \"lines\": %llu, \"accepted\": %llu, "
                 "\"host_lines\": %llu, \"windows\": %u, \"h2d_ms\": %.3f, \"device_ms\": %.3f, "
                 "\"host_fix_ms\": %.3f, \"d2h_ms\": %.3f, \"total_ms\": %.3f}}\n",
                 (unsigned long long)ing.body_bytes, (unsigned long long)ing.lines,
                 (unsigned long long)ing.accepted, (unsigned long long)ing.host_lines, ing.windows,
                 ing.h2d_ms, ing.device_ms, ing.host_fix_ms, ing.d2h_ms, ing.total_ms);
  if (timing && keep != RK_KEEP_ALL) sel.print("{", "}\n");
  if (timing)
    std::fprintf(stderr,
                 "{\"frags\": %llu, \"pairs\": %zu, \"load_s\": %.6f, \"classify_s\": %.6f, "
                 "\"device_ms\": %.3f, \"save_s\": %.6f, \"gpus\": %d}\n",
                 (unsigned long long)soa.n, params.size(), t1 - t0, t_class, dev_ms, t3 - t2, gpus);
  rk_db_free(db);
  if (rc) {
    std::fprintf(stderr, "writing output failed (%d)\n", rc);
    return 1;
  }
  std::printf("Repkiller finished with no errors\n");
  return 0;
}
