// rk_db.h -- the parsed database behind rk_db_*, shared by the host ingress
// (rk_host.cpp, built without HIP) and the device ingress (rk_csv.hip).  Not
// part of the public ABI.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

struct rk_db {
  std::vector<uint64_t> x_start, y_start, x_end, y_end, length, score, ident;
  std::vector<float> similarity;
  std::vector<uint8_t> strand;
  std::string header;
  uint64_t len_x_hdr = 0, len_y_hdr = 0, total_hdr = 0;
  // rk_db_load_csv_device with RK_DB_KEEP_DEVICE: x_start, y_start, length and
  // strand also stay in HBM (one allocation the database owns).  rk_host.cpp
  // cannot call HIP, so the device side leaves the function that frees it.
  void *dev_block = nullptr;
  const uint64_t *dev_x = nullptr, *dev_y = nullptr, *dev_len = nullptr;
  const uint8_t *dev_strand = nullptr;
  // with RK_DB_KEEP_ROWS the other five columns stay too (a second carve of the
  // same allocation, so the one dev_free hook releases all nine); null otherwise
  const uint64_t *dev_xe = nullptr, *dev_ye = nullptr, *dev_score = nullptr, *dev_ident = nullptr;
  const float *dev_sim = nullptr;
  bool dev_rows = false;  // loaded with RK_DB_KEEP_ROWS (also when it has no rows)
  int dev_device = -1;
  void (*dev_free)(void *block, int device) = nullptr;
};

// rk_dbset_load_csv_device: one database per listed file, held as one combined
// database (its header text and header numbers are unused) plus what differs
// per set.  Set k's rows are rows [set_off[k], set_off[k + 1]) of db's columns.
struct rk_dbset {
  rk_db *db = nullptr;
  std::vector<uint64_t> set_off;  // nsets + 1
  std::vector<uint64_t> len_x_hdr, len_y_hdr, total_hdr;
  std::vector<std::string> header;
};

namespace rk {

struct DbRow {
  uint64_t xs, ys, xe, ye, len, score, ident;
  float sim;
  uint8_t strand;
};

// rk_host.cpp: one body line -> row, or false where readFragment returns false
bool db_parse_line(const char *b, const char *e, DbRow *r);
// rk_host.cpp: the 16 header lines of the file [p, end) into db->header and the
// three header numbers (std::getline semantics); returns where the body starts,
// *eof set when the file ended inside the header
const char *db_read_header(rk_db *db, const char *p, const char *end, bool *eof);
// rk_host.cpp: output row of input row i (store_frag, commonFunctions.cpp:101-104)
// at o, at most 255 bytes; returns the end.  The device egress (rk_csv_out.hip)
// formats with it the rows its own row function refuses.
char *db_format_row(const rk_db *db, uint32_t i, uint64_t gid, unsigned rep, char *o);

}  // namespace rk
