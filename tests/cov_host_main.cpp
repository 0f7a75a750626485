// cov_host_main.cpp -- drives the host side of the pooled covariance alone, on
// the CPU: pbh_trace_host.cpp's cov_layout and cov_finish.  tests/
// test_cov_host.py builds it with the address and undefined-behaviour
// sanitizers and -ffp-contract=off.  Reads requests from the file named on the
// command line, one per line, and answers each with one line.  A double
// travels as 16 hex digits; every other number in decimal.
//   layout n count d
//       -> "ok pairs chain_blocks slices slice_len rows cols K part res bytes",
//          or "refused"
//   tri a b d             -> cov_tri
//   finish d M K[d] S[d] P[d (d + 1) / 2]
//       -> mean [d], cov [d][d], corr [d][d]
//   finish_cov d M K[d] S[d] P[..]   -> cov [d][d] alone (the others null)
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

std::string hex(double x) {
  uint64_t bits;
  std::memcpy(&bits, &x, 8);
  char buf[20];
  snprintf(buf, sizeof buf, "%016llx", (unsigned long long)bits);
  return buf;
}

bool number(std::istream &in, double *x) {
  std::string w;
  if (!(in >> w)) return false;
  const uint64_t bits = std::stoull(w, nullptr, 16);
  std::memcpy(x, &bits, 8);
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
    if (cmd == "layout") {
      int64_t n, count;
      int32_t d;
      if (!(ls >> n >> count >> d)) return 3;
      pbh::CovLayout l;
      std::memset(&l, 0x5a, sizeof l);
      if (!pbh::cov_layout(n, count, d, &l)) {
        // a refusal leaves `out` untouched
        const unsigned char *p = reinterpret_cast<const unsigned char *>(&l);
        for (size_t i = 0; i < sizeof l; ++i)
          if (p[i] != 0x5a) return 4;
        std::cout << "refused\n";
        continue;
      }
      std::cout << "ok " << l.pairs << ' ' << l.chain_blocks << ' ' << l.slices << ' '
                << l.slice_len << ' ' << l.rows << ' ' << l.cols << ' ' << l.K << ' ' << l.part
                << ' ' << l.res << ' ' << l.bytes << "\n";
    } else if (cmd == "tri") {
      int64_t a, b, d;
      if (!(ls >> a >> b >> d)) return 3;
      std::cout << pbh::cov_tri(a, b, d) << "\n";
    } else if (cmd == "finish" || cmd == "finish_cov") {
      int32_t d;
      int64_t M;
      if (!(ls >> d >> M) || d < 1 || d > 32) return 3;
      std::vector<double> K((size_t)d), S((size_t)d), P((size_t)(d * (d + 1) / 2));
      for (std::vector<double> *v : {&K, &S, &P})
        for (double &x : *v)
          if (!number(ls, &x)) return 3;
      std::vector<double> mean((size_t)d), cov((size_t)(d * d)), corr((size_t)(d * d));
      const bool all = cmd == "finish";
      pbh::cov_finish(K.data(), S.data(), P.data(), M, d, all ? mean.data() : nullptr, cov.data(),
                      all ? corr.data() : nullptr);
      const char *sep = "";
      if (all)
        for (double x : mean) std::cout << sep << hex(x), sep = " ";
      for (double x : cov) std::cout << sep << hex(x), sep = " ";
      if (all)
        for (double x : corr) std::cout << sep << hex(x), sep = " ";
      std::cout << "\n";
    } else {
      return 3;
    }
  }
  return 0;
}
