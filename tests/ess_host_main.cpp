// ess_host_main.cpp -- drives the host stage of the bulk- and tail-ESS across
// chains alone, on the CPU: pbh_trace_host.cpp's multi_chain_ess and
// ess_layout (with rank_layout, behind whose bytes the ESS regions lie).
// tests/test_ess_rank_host.py builds it with the address and undefined-
// behaviour sanitizers and -ffp-contract=off.  Reads requests from the file
// named on the command line, one per line, and answers each with one line.  A
// double travels as the 16 hex digits of its bits.
//   ess C h m0 .. m(C-1) A0 .. A(h-1)
//                           -> "<ess as hex> <k*>" (C, h in decimal)
//   layout n count d bulk select_words
//                           -> "bad rank" (bulk = 1 and rank_layout refuses),
//                              "bad" (ess_layout refuses), or "ok base h pairs
//                              run groups select thr part acov means stats
//                              bytes", base = RankLayout.bytes with bulk = 1,
//                              else 0
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

std::string hex(double x) {
  uint64_t bits;
  std::memcpy(&bits, &x, 8);
  char buf[20];
  snprintf(buf, sizeof buf, "%016llx", (unsigned long long)bits);
  return buf;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  if (!in) return 2;
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string what;
    if (!(ls >> what)) continue;
    if (what == "ess") {
      int64_t C, h;
      if (!(ls >> C >> h) || C < 2 || h < 2) return 2;
      // (heap copies of exactly C and h doubles: a read outside ends the program)
      std::vector<double> m, A;
      std::string w;
      while (ls >> w) {
        const double x = as_double(std::stoull(w, nullptr, 16));
        if ((int64_t)m.size() < C) m.push_back(x);
        else A.push_back(x);
      }
      if ((int64_t)m.size() != C || (int64_t)A.size() != h) return 2;
      int64_t ks = -7;
      const double ess = pbh::multi_chain_ess(m.data(), A.data(), C, h, &ks);
      std::cout << hex(ess) << ' ' << ks << '\n';
    } else if (what == "layout") {
      int64_t n, count, sel;
      int32_t d, bulk;
      if (!(ls >> n >> count >> d >> bulk >> sel)) return 2;
      pbh::RankLayout rl;
      int64_t base = 0;
      if (bulk) {
        if (!pbh::rank_layout(n, count, d, 0, false, &rl)) {
          std::cout << "bad rank\n";
          continue;
        }
        base = rl.bytes;
      }
      pbh::EssLayout l;
      if (!pbh::ess_layout(n, count, d, base, sel, &l)) {
        std::cout << "bad\n";
        continue;
      }
      std::cout << "ok " << base << ' ' << l.h << ' ' << l.pairs << ' ' << l.run << ' '
                << l.groups << ' ' << l.select << ' ' << l.thr << ' ' << l.part << ' ' << l.acov
                << ' ' << l.means << ' ' << l.stats << ' ' << l.bytes << '\n';
    } else {
      return 2;
    }
  }
  return 0;
}
