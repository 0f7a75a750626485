// trace_host_main.cpp -- drives the host side of the trace reductions alone, on
// the CPU: probayes_amd/csrc/pbh_trace_host.cpp (the window and quantile-list
// checks, the pooled-quantile steps, rank_layout, ess_layout, multi_chain_ess)
// and pbh_rank_impl.h (the normal score and the run search, the very header
// the device kernels include).  tests/host_program.py builds it with the
// address and undefined-behaviour sanitizers and -ffp-contract=off, for
// test_trace_host.py, test_rank_host.py and test_ess_rank_host.py.  Reads
// requests from the file named on the command line, one per line, and answers
// each with one line.  A double or a key travels as the 16 hex digits of its
// bits, both ways; every other number in decimal.
//   window rec first count min_count
//     -> "ok end" or "bad end" (trace_window_ok, trace_window_end)
//   qerr nq n q0 .. q(n-1)
//     -> "ok", or quantile_list_error's text
//   plan M nq q0 ..
//     -> "plan lo0 hi0 frac0 lo1 .. ranks r0 r1 .." (pooled_plan)
//   interp M d nq q0 .. s0 ..        (s: [d][nt], nt as plan gives it)
//     -> "interp out.. stats .."     (pooled_interpolate: [nq][d], [nq][2][d])
//   ndtri p0 p1 ..          -> normal_quantile of each
//   score M r0 r1 ..        -> normal_score(r, M) of each
//   run k0 k1 ..            -> "lo0 hi0 lo1 hi1 .." (equal_run at every position
//                              of the ascending keys) and, after "ranks", the
//                              average_rank of each run as hex doubles
//   rank_layout n count d select_words want_ranks
//                           -> "bad", or "ok M tiles chunk_tiles chunks select
//                              med res state chunk hist stats key0 key1 idx0
//                              idx1 z r bytes"
//   ess C h m0 .. m(C-1) A0 .. A(h-1)
//                           -> "<ess as hex> <k*>" (multi_chain_ess)
//   ess_layout n count d bulk select_words
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

#include "../probayes_amd/csrc/pbh_rank_impl.h"
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

// the rest of the line, as keys
std::vector<uint64_t> words(std::istream &in) {
  std::vector<uint64_t> v;
  std::string w;
  while (in >> w) v.push_back(std::stoull(w, nullptr, 16));
  return v;
}

// the next v.size() words, as doubles
bool doubles(std::istream &in, std::vector<double> &v) {
  for (double &x : v) {
    std::string w;
    if (!(in >> w)) return false;
    x = as_double(std::stoull(w, nullptr, 16));
  }
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
    } else if (what == "ndtri") {
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
    } else if (what == "rank_layout") {
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
    } else if (what == "ess") {
      int64_t C, h;
      if (!(ls >> C >> h) || C < 2 || h < 2) return 2;
      // (heap copies of exactly C and h doubles: a read outside ends the program)
      std::vector<double> m((size_t)C), A((size_t)h);
      std::string more;
      if (!doubles(ls, m) || !doubles(ls, A) || (ls >> more)) return 2;
      int64_t ks = -7;
      const double ess = pbh::multi_chain_ess(m.data(), A.data(), C, h, &ks);
      std::cout << hex(ess) << ' ' << ks << '\n';
    } else if (what == "ess_layout") {
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
