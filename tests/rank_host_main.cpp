// rank_host_main.cpp -- drives the host side of the pooled ranks alone, on the
// CPU: probayes_amd/csrc/pbh_rank_impl.h (the normal score and the run search,
// the very header the device kernels include) and pbh_trace_host.cpp's
// rank_layout.  tests/test_rank_host.py builds it with the address and
// undefined-behaviour sanitizers and -ffp-contract=off.  Reads requests from
// the file named on the command line, one per line, and answers each with one
// line.  A double or a key travels as the 16 hex digits of its bits.
//   ndtri p0 p1 ..          -> normal_quantile of each
//   score M r0 r1 ..        -> normal_score(r, M) of each (M in decimal)
//   run k0 k1 ..            -> "lo0 hi0 lo1 hi1 .." (equal_run at every position
//                              of the ascending keys) and, after "ranks", the
//                              average_rank of each run as hex doubles
//   layout n count d select_words want_ranks
//                           -> "bad", or "ok M tiles chunk_tiles chunks select
//                              med res state chunk hist stats key0 key1 idx0
//                              idx1 z r bytes"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../probayes_amd/csrc/pbh_rank_impl.h"
#include "../probayes_amd/csrc/pbh_trace_host.h"

namespace {

std::vector<uint64_t> words(std::istream &in) {
  std::vector<uint64_t> v;
  std::string w;
  while (in >> w) v.push_back(std::stoull(w, nullptr, 16));
  return v;
}

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
    if (what == "ndtri") {
      const char *sep = "";
      for (uint64_t w : words(ls)) {
        std::cout << sep << hex(pbh::normal_quantile(as_double(w)));
        sep = " ";
      }
      std::cout << '\n';
    } else if (what == "score") {
      int64_t M;
      if (!(ls >> M)) return 2;
      const char *sep = "";
      for (uint64_t w : words(ls)) {
        std::cout << sep << hex(pbh::normal_score(as_double(w), (double)M));
        sep = " ";
      }
      std::cout << '\n';
    } else if (what == "run") {
      // (a heap copy of exactly M keys: a read outside it ends the program)
      const std::vector<uint64_t> keys = words(ls);
      const int64_t M = (int64_t)keys.size();
      if (M < 1) return 2;
      std::ostringstream ranks;
      for (int64_t p = 0; p < M; ++p) {
        int64_t lo = -7, hi = -7;
        pbh::equal_run(keys.data(), M, p, &lo, &hi);
        std::cout << lo << ' ' << hi << ' ';
        ranks << ' ' << hex(pbh::average_rank(lo, hi));
      }
      std::cout << "ranks" << ranks.str() << '\n';
    } else if (what == "layout") {
      int64_t n, count, sel;
      int32_t d, want;
      if (!(ls >> n >> count >> d >> sel >> want)) return 2;
      pbh::RankLayout l;
      if (!pbh::rank_layout(n, count, d, sel, want != 0, &l)) {
        std::cout << "bad\n";
        continue;
      }
      std::cout << "ok " << l.M << ' ' << l.tiles << ' ' << l.chunk_tiles << ' ' << l.chunks
                << ' ' << l.select << ' ' << l.med << ' ' << l.res << ' ' << l.state << ' '
                << l.chunk << ' ' << l.hist << ' ' << l.stats << ' ' << l.key[0] << ' '
                << l.key[1] << ' ' << l.idx[0] << ' ' << l.idx[1] << ' ' << l.z << ' ' << l.r
                << ' ' << l.bytes << '\n';
    } else {
      return 2;
    }
  }
  return 0;
}
