// trace_host_main.cpp -- drives probayes_amd/csrc/pbh_trace_host.cpp alone, on
// the CPU (tests/test_trace_host.py builds it with the address and
// undefined-behaviour sanitizers).  Reads requests from the file named on the
// command line, one per line, and answers each with one line.  A double
// travels as the 16 hex digits of its bits, both ways.
//   window rec first count min_count
//     -> "ok end" or "bad end" (trace_window_ok, trace_window_end)
//   qerr nq n q0 .. q(n-1)
//     -> "ok", or quantile_list_error's text
//   plan M nq q0 ..
//     -> "plan lo0 hi0 frac0 lo1 .. ranks r0 r1 .." (pooled_plan)
//   interp M d nq q0 .. s0 ..        (s: [d][nt], nt as plan gives it)
//     -> "interp out.. stats .."     (pooled_interpolate: [nq][d], [nq][2][d])
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

bool doubles(std::istream &in, std::vector<double> &v) {
  for (double &x : v) {
    std::string w;
    if (!(in >> w)) return false;
    const uint64_t bits = std::stoull(w, nullptr, 16);
    std::memcpy(&x, &bits, 8);
  }
  return true;
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
    if (what == "window") {
      int64_t rec, first, count, least;
      if (!(ls >> rec >> first >> count >> least)) return 2;
      std::cout << (pbh::trace_window_ok(rec, first, count, least) ? "ok " : "bad ")
                << pbh::trace_window_end(first, count) << '\n';
    } else if (what == "qerr") {
      int32_t nq, n;
      if (!(ls >> nq >> n) || n < 1) return 2;
      std::vector<double> q(n);
      if (!doubles(ls, q)) return 2;
      const std::string bad = pbh::quantile_list_error(nq, q.data());
      std::cout << (bad.empty() ? "ok" : bad) << '\n';
    } else if (what == "plan" || what == "interp") {
      int64_t M, d = 0;
      int32_t nq;
      if (!(ls >> M)) return 2;
      if (what == "interp" && !(ls >> d)) return 2;
      if (!(ls >> nq) || nq < 1) return 2;
      std::vector<double> q(nq);
      if (!doubles(ls, q)) return 2;
      const pbh::PooledPlan p = pbh::pooled_plan(M, nq, q.data());
      if (what == "plan") {
        std::cout << "plan";
        for (int32_t j = 0; j < nq; ++j)
          std::cout << ' ' << p.lo[j] << ' ' << p.hi[j] << ' ' << hex(p.frac[j]);
        std::cout << " ranks";
        for (uint64_t r : p.ranks) std::cout << ' ' << r;
        std::cout << '\n';
        continue;
      }
      std::vector<double> s((size_t)d * p.ranks.size()), out((size_t)nq * d),
          stats((size_t)nq * 2 * d);
      if (!doubles(ls, s)) return 2;
      pbh::pooled_interpolate(p, d, s.data(), out.data(), stats.data());
      // without order statistics the quantiles are the same
      std::vector<double> only(out.size());
      pbh::pooled_interpolate(p, d, s.data(), only.data(), nullptr);
      if (std::memcmp(only.data(), out.data(), out.size() * 8) != 0) return 3;
      std::cout << "interp";
      for (double v : out) std::cout << ' ' << hex(v);
      std::cout << " stats";
      for (double v : stats) std::cout << ' ' << hex(v);
      std::cout << '\n';
    } else {
      return 2;
    }
  }
  return 0;
}
