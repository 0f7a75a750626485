// psis_host_main.cpp -- drives the host side of the pointwise tail select alone,
// on the CPU: pbh_trace_host.cpp's tail_key / tail_key_value, tail_pick,
// tail_finish and the select's scratch layout.  tests/test_psis_host.py builds
// it with the address and undefined-behaviour sanitizers and -ffp-contract=off.
// Reads requests from the file named on the command line, one per line, and
// answers each with one line.  A double and a key travel as 16 hex digits;
// every other number in decimal.
//   key v                  -> the key of the double v
//   value key              -> the double of a key
//   pick bits prefix rank below under h[0] .. h[2^bits - 1]
//       -> "prefix rank below under" after tail_pick (prefix in hex)
//   finish k done prefix rank below under n_keys key.. n_rows (m s)..
//       -> the k doubles of the tail, then rest_lse
//   layout tiles capacity  -> "npad prefix cursor hist list words"
//   batch capacity         -> tail_batch_tiles, then tail_default_capacity of
//                             the same number, then kTailMaxCapacity
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../probayes_amd/csrc/pbh_trace_host.h"

namespace {

double as_double(uint64_t bits) {
  double x;
  std::memcpy(&x, &bits, 8);
  return x;
}

std::string hex(uint64_t bits) {
  char buf[20];
  snprintf(buf, sizeof buf, "%016llx", (unsigned long long)bits);
  return buf;
}

std::string hex(double x) {
  uint64_t bits;
  std::memcpy(&bits, &x, 8);
  return hex(bits);
}

bool word(std::istream &in, uint64_t *v) {
  std::string w;
  if (!(in >> w)) return false;
  *v = std::stoull(w, nullptr, 16);
  return true;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  if (!in) return 2;
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string cmd;
    ls >> cmd;
    if (cmd == "key") {
      uint64_t v;
      if (!word(ls, &v)) return 3;
      std::cout << hex(pbh::tail_key(as_double(v))) << "\n";
    } else if (cmd == "value") {
      uint64_t v;
      if (!word(ls, &v)) return 3;
      std::cout << hex(pbh::tail_key_value(v)) << "\n";
    } else if (cmd == "pick") {
      int bits;
      pbh::TailState s;
      if (!(ls >> bits) || bits < 1 || bits > pbh::kTailDigit || !word(ls, &s.prefix) ||
          !(ls >> s.rank >> s.below >> s.under))
        return 3;
      std::vector<uint64_t> h((size_t)1 << bits);
      for (uint64_t &v : h)
        if (!(ls >> v)) return 3;
      pbh::tail_pick(h.data(), bits, &s);
      std::cout << hex(s.prefix) << ' ' << s.rank << ' ' << s.below << ' ' << s.under << "\n";
    } else if (cmd == "finish") {
      int64_t k, n_keys, n_rows;
      int done;
      pbh::TailState s;
      if (!(ls >> k >> done) || k < 1 || !word(ls, &s.prefix) ||
          !(ls >> s.rank >> s.below >> s.under >> n_keys) || n_keys < 0)
        return 3;
      std::vector<uint64_t> keys((size_t)n_keys);
      for (uint64_t &v : keys)
        if (!word(ls, &v)) return 3;
      if (!(ls >> n_rows) || n_rows < 0) return 3;
      std::vector<pbh::LsePair> rows((size_t)n_rows);
      for (pbh::LsePair &r : rows) {
        uint64_t m, sum;
        if (!word(ls, &m) || !word(ls, &sum)) return 3;
        r = pbh::LsePair{as_double(m), as_double(sum)};
      }
      std::vector<double> tail((size_t)k);
      double rest;
      pbh::tail_finish(keys.data(), n_keys, k, done, s, rows.data(), n_rows, tail.data(), &rest);
      for (double v : tail) std::cout << hex(v) << ' ';
      std::cout << hex(rest) << "\n";
    } else if (cmd == "layout") {
      int64_t tiles, capacity;
      if (!(ls >> tiles >> capacity)) return 3;
      const pbh::TailLayout l = pbh::tail_layout(tiles, capacity);
      std::cout << l.npad << ' ' << l.prefix << ' ' << l.cursor << ' ' << l.hist << ' ' << l.list
                << ' ' << l.words << "\n";
    } else if (cmd == "batch") {
      int64_t v;
      if (!(ls >> v) || v < 1) return 3;
      std::cout << pbh::tail_batch_tiles(v) << ' ' << pbh::tail_default_capacity(v) << ' '
                << pbh::kTailMaxCapacity << "\n";
    } else {
      return 3;
    }
  }
  return 0;
}
