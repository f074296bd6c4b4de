// csv_line_check -- the shared line function (rk_csv_line.h), compiled for the
// host, against the host parser of rk_db_load_csv, line by line.
//
//   csv_line_check full  <workdir> <csv>...   (linked with librepkiller_amd)
//   csv_line_check check <workdir>            (stand-alone; -DRK_NO_LIB)
//
// full: the body lines of every <csv> plus ~100k lines of a seeded grammar of
// hostile fields are written under a valid header to <workdir>/lines.csv; the
// file is loaded with rk_db_load_csv and saved as a SoA cache, whose nine
// columns are dumped as text to <workdir>/rows.txt; then the check runs.
// check: the same check from lines.csv and rows.txt alone, so a sanitized
// build never loads the HIP library.
//
// The check walks the lines in file order.  Per line it evaluates for itself
//   rules = the 14-field split, no empty field, field 0 == "Frag"
//   slow  = rk::fast_stof(field 10) fails, or the line is longer than the cap
// and requires csv_line to return REJECT iff !rules, HOST iff rules && slow,
// ACCEPT otherwise.  An ACCEPT line must be the host's next row, all nine
// values bit-equal.  A HOST line is the host's next row iff strtof converts
// its field 10 (std::stof's rule); the host's row count must come out exactly,
// so REJECT stands exactly where the host dropped a line.
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "rk_csv_line.h"
#include "rk_format.h"
#ifndef RK_NO_LIB
#include "repkiller_amd.h"
#endif

namespace {

struct HostRow {
  uint64_t v[7];  // xs ys xe ye len score ident
  uint32_t sim;
  unsigned strand;
};

std::string slurp(const std::string &path) {
  std::ifstream f(path, std::ios::binary);
  std::stringstream ss;
  ss << f.rdbuf();
  return ss.str();
}

// the body of a fragment CSV: what follows 16 getline calls
std::vector<std::string> body_lines(const std::string &text) {
  size_t p = 0;
  for (int k = 0; k < 16; ++k) {
    const size_t nl = text.find('\n', p);
    if (nl == std::string::npos) return {};
    p = nl + 1;
  }
  std::vector<std::string> out;
  while (p < text.size()) {
    const size_t nl = text.find('\n', p);
    if (nl == std::string::npos) {
      out.push_back(text.substr(p));
      break;
    }
    out.push_back(text.substr(p, nl - p));
    p = nl + 1;
  }
  return out;
}

struct Rng {
  uint64_t s;
  uint64_t next() {
    s ^= s << 13, s ^= s >> 7, s ^= s << 17;
    return s;
  }
  uint64_t below(uint64_t n) { return next() % n; }
};

std::string digits(Rng &r, int n) {
  std::string s;
  for (int i = 0; i < n; ++i) s.push_back((char)('0' + (i == 0 ? 1 + r.below(9) : r.below(10))));
  return s;
}

std::string fast_float(Rng &r) {
  std::string s;
  if (r.below(8) == 0) s += r.below(2) ? "-" : "+";
  if (r.below(16) == 0) s += " ";
  for (uint64_t z = r.below(3); z; --z) s += "0";
  const int sig = 1 + (int)r.below(7), frac = (int)r.below(11);
  std::string d = digits(r, sig);
  if (frac == 0) return s + d + (r.below(4) ? "" : ".");
  if (frac >= sig) return s + "0." + std::string((size_t)(frac - sig), '0') + d;
  return s + d.substr(0, (size_t)(sig - frac)) + "." + d.substr((size_t)(sig - frac));
}

std::string slow_float(Rng &r) {
  static const char *k[] = {"1e3",      "9.5E-2",   "12345678", "0.123456789", "nan",  "-nan",
                            "inf",      "-inf",     "0x1p3",    "1e50",        "1e-50", "93.4x",
                            " 1e2",     "abc",      ".",        "+",           "-",    "1.2.3",
                            "infinity", "1e",       "0x",       "1e-46",       "3.4028236e38",
                            "0.00000000001", "16777217", "1e400", "\t12.5e0"};
  return k[r.below(sizeof k / sizeof *k)];
}

std::string hostile_int(Rng &r) {
  switch (r.below(9)) {
    case 0: return " " + digits(r, 5);
    case 1: return "\t +" + digits(r, 4);
    case 2: return "-" + digits(r, 6);
    case 3: return digits(r, 19 + (int)r.below(7));
    case 4: return "-" + digits(r, 19 + (int)r.below(7));
    case 5: return digits(r, 3) + "a" + digits(r, 2);
    case 6: return std::string("12") + '\0' + "34";
    case 7: return "9223372036854775807";
    default: return "-9223372036854775808";
  }
}

std::string gen_line(Rng &r) {
  std::vector<std::string> f = {"Frag", digits(r, 1 + (int)r.below(9)), digits(r, 1 + (int)r.below(9)),
                                digits(r, 1 + (int)r.below(9)), digits(r, 1 + (int)r.below(9)),
                                r.below(2) ? "f" : "r", "0", digits(r, 1 + (int)r.below(5)),
                                digits(r, 1 + (int)r.below(5)), digits(r, 1 + (int)r.below(5)),
                                fast_float(r), fast_float(r), "0", "1"};
  const uint64_t cls = r.below(16);
  bool crlf = false, trailing = false;
  switch (cls) {
    case 0: crlf = true; break;
    case 1: return "";
    case 2: {  // 1..13 or 15..18 fields
      const size_t k = r.below(2) ? 1 + r.below(13) : 15 + r.below(4);
      while (f.size() > k) f.pop_back();
      while (f.size() < k) f.push_back(digits(r, 2));
      if (r.below(3) == 0 && f.size() > 1) f.back() = r.below(2) ? fast_float(r) : slow_float(r);
      break;
    }
    case 3: trailing = true; break;
    case 4: {
      static const char *t[] = {"frag", "Frag ", "Fra", "Fragx", " Frag", "FRAG", "F"};
      f[0] = t[r.below(7)];
      break;
    }
    case 5: case 6: {
      static const int at[] = {1, 2, 3, 4, 7, 8, 9};
      f[(size_t)at[r.below(7)]] = hostile_int(r);
      break;
    }
    case 7: f[10] = slow_float(r); break;
    case 8: f[10] = slow_float(r), f[1] = hostile_int(r); break;
    case 9: f[1 + r.below(13)] = ""; break;
    case 10: f[5] = std::string(1, (char)r.below(256) == ',' ? 'x' : (char)r.below(256)); break;
    case 11:
      if (r.below(8) == 0) f[2] = std::string(3000 + r.below(3000), ' ') + f[2];
      break;
    case 12: f[10] = std::string("9") + '\0' + "3"; break;
    default: break;
  }
  for (auto &s : f)
    for (auto &c : s)
      if (c == '\n') c = 'n';
  if (cls == 10 && (f[5].empty() || f[5][0] == ',')) f[5] = "f";
  std::string line;
  for (size_t i = 0; i < f.size(); ++i) line += (i ? "," : "") + f[i];
  if (trailing) line += ",";
  if (crlf) line += "\r";
  return line;
}

// std::stof's rule on the field's c_str(), as rk_host.cpp's parse_stof
bool strtof_converts(const char *b, const char *e) {
  const std::string s(b, (size_t)(e - b));
  char *end = nullptr;
  errno = 0;
  (void)std::strtof(s.c_str(), &end);
  return end != s.c_str() && errno != ERANGE;
}

int check(const std::vector<std::string> &lines, const std::vector<HostRow> &rows) {
  size_t next = 0, bad = 0, n_acc = 0, n_host = 0, n_rej = 0;
  auto fail = [&](size_t i, const char *what) {
    if (++bad <= 20) std::printf("line %zu: %s: [%s]\n", i, what, lines[i].c_str());
  };
  for (size_t i = 0; i < lines.size(); ++i) {
    const std::string &s = lines[i];
    const char *b = s.data(), *e = b + s.size();
    // the predicate, evaluated here with std::string splitting
    std::vector<std::string> f;
    bool rules = true;
    {
      size_t p = 0;
      bool eof = false;
      while (f.size() < 14 && rules) {
        if (eof) {
          f.push_back(f.back());
          continue;
        }
        const size_t c = s.find(',', p);
        if (c == std::string::npos) {
          f.push_back(s.substr(p));
          eof = true;
        } else {
          f.push_back(s.substr(p, c - p));
          p = c + 1;
        }
        if (f.back().empty()) rules = false;
      }
      if (rules && f[0] != "Frag") rules = false;
    }
    float fsim = 0;
    const bool slow = rules && (!rk::fast_stof(f[10].data(), f[10].data() + f[10].size(), &fsim) ||
                                s.size() > RK_CSV_MAX_LINE);
    const uint8_t want = !rules ? rk::CSV_REJECT : slow ? rk::CSV_HOST : rk::CSV_ACCEPT;
    rk::CsvRow r;
    std::memset(&r, 0, sizeof r);
    const uint8_t got = rk::csv_line(b, e, &r);
    if (got != want) {
      fail(i, got == rk::CSV_REJECT ? "REJECT unexpected"
                                    : got == rk::CSV_HOST ? "HOST unexpected" : "ACCEPT unexpected");
      // keep the row cursor in step with the host where that is still possible
      if (rules && strtof_converts(f[10].data(), f[10].data() + f[10].size())) ++next;
      continue;
    }
    if (got == rk::CSV_REJECT) {
      ++n_rej;
    } else if (got == rk::CSV_HOST) {
      ++n_host;
      if (strtof_converts(f[10].data(), f[10].data() + f[10].size())) ++next;
    } else {
      ++n_acc;
      if (next >= rows.size()) {
        fail(i, "ACCEPT but the host has no more rows");
        continue;
      }
      const HostRow &h = rows[next++];
      uint32_t bits;
      std::memcpy(&bits, &r.sim, 4);
      const uint64_t v[7] = {r.xs, r.ys, r.xe, r.ye, r.len, r.score, r.ident};
      if (std::memcmp(v, h.v, sizeof v) != 0 || bits != h.sim || r.strand != h.strand)
        fail(i, "ACCEPT with values that differ from the host's row");
    }
  }
  if (next != rows.size()) {
    std::printf("host rows %zu, lines that should be rows %zu\n", rows.size(), next);
    ++bad;
  }
  std::printf("lines %zu accept %zu host %zu reject %zu host_rows %zu mismatches %zu\n",
              lines.size(), n_acc, n_host, n_rej, rows.size(), bad);
  return bad ? 1 : 0;
}

std::vector<HostRow> read_rows(const std::string &path) {
  std::vector<HostRow> rows;
  FILE *f = std::fopen(path.c_str(), "r");
  if (!f) return rows;
  HostRow h;
  unsigned long long v[7];
  while (std::fscanf(f, "%llu %llu %llu %llu %llu %llu %llu %u %u", &v[0], &v[1], &v[2], &v[3],
                     &v[4], &v[5], &v[6], &h.sim, &h.strand) == 9) {
    for (int k = 0; k < 7; ++k) h.v[k] = v[k];
    rows.push_back(h);
  }
  std::fclose(f);
  return rows;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  const std::string mode = argv[1], dir = argv[2];
  const std::string csv = dir + "/lines.csv", txt = dir + "/rows.txt";
#ifndef RK_NO_LIB
  if (mode == "full") {
    std::vector<std::string> lines;
    for (int a = 3; a < argc; ++a) {
      const auto b = body_lines(slurp(argv[a]));
      lines.insert(lines.end(), b.begin(), b.end());
    }
    Rng rng{0x9E3779B97F4A7C15ull};
    for (int i = 0; i < 100000; ++i) lines.push_back(gen_line(rng));
    {
      std::ofstream o(csv, std::ios::binary);
      for (int k = 1; k <= 16; ++k) {
        if (k == 7) o << "SeqX length : 1000000000\n";
        else if (k == 8) o << "SeqY length : 1000000000\n";
        else if (k == 13) o << "Total fragments : " << lines.size() << "\n";
        else o << "header line " << k << "\n";
      }
      for (const auto &l : lines) o << l << "\n";
    }
    rk_db *db = nullptr;
    int rc = rk_db_load_csv(csv.c_str(), &db);
    if (rc) {
      std::printf("rk_db_load_csv: %d\n", rc);
      return 1;
    }
    const std::string soa = dir + "/host.soa";
    if ((rc = rk_db_save_soa(db, soa.c_str()))) {
      std::printf("rk_db_save_soa: %d\n", rc);
      return 1;
    }
    rk_db_free(db);
    // the cache layout (rk_host.cpp): magic, n, 3 header numbers, header bytes,
    // header text, then each column on a 4-KB boundary
    const std::string c = slurp(soa);
    uint64_t fixed[5];
    std::memcpy(fixed, c.data() + 8, 40);
    const uint64_t n = fixed[0];
    auto up = [](size_t v) { return (v + 4095) & ~(size_t)4095; };
    size_t off[9], o = up(48 + fixed[4]);
    const size_t width[9] = {8, 8, 8, 8, 8, 8, 8, 4, 1};
    for (int k = 0; k < 9; ++k) off[k] = o, o = up(o + n * width[k]);
    FILE *f = std::fopen(txt.c_str(), "w");
    for (uint64_t i = 0; i < n; ++i) {
      for (int k = 0; k < 7; ++k) {
        uint64_t v;
        std::memcpy(&v, c.data() + off[k] + i * 8, 8);
        std::fprintf(f, "%llu ", (unsigned long long)v);
      }
      uint32_t sim;
      std::memcpy(&sim, c.data() + off[7] + i * 4, 4);
      std::fprintf(f, "%u %u\n", sim, (unsigned)(uint8_t)c[off[8] + i]);
    }
    std::fclose(f);
  } else
#endif
      if (mode != "check") {
    return 2;
  }
  const auto lines = body_lines(slurp(csv));
  const auto rows = read_rows(txt);
  if (lines.empty()) {
    std::printf("no lines in %s\n", csv.c_str());
    return 1;
  }
  return check(lines, rows);
}
