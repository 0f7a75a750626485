// hist_host_main.cpp -- drives the host side of the pooled histograms alone, on
// the CPU: pbh_trace_host.cpp's hist_check_edges, hist2d_check_pairs,
// hist_layout, hist2d_layout, hist_guess_ok, hist_dim_plan and hist_fill_table,
// and the lookup of pbh_hist_bin.h, the very functions the kernels run.  tests/
// test_hist_host.py builds it with the address and undefined-behaviour
// sanitizers and -ffp-contract=off.  Reads requests from the file named on the
// command line, one per line, and answers each with one line.  A double
// travels as 16 hex digits; every other number in decimal.
//   check d n_bins[d] edges..          -> "ok", or what is wrong
//   pairs d n_bins[d] n_pairs pairs..  -> "ok", or what is wrong
//   layout n count d n_bins[d]
//       -> "ok dims groups lds_bytes chain_blocks slices slice_len n_tab n_ctr
//          tables counts bytes", then per listed dim "dim tab ctr", then per
//          group "first tab_off tab_len ctr_off ctr_len"; or "refused"
//   layout2d n count d n_bins[d] n_pairs pairs..
//       -> "ok lds_bytes chain_blocks slices slice_len n_tab n_ctr tables pairs
//          counts bytes", then tab_off [d], then out [n_pairs]; or "refused"
//   guess_ok B edges[B + 1]            -> 1 or 0
//   bins how B edges[B + 1] N x[N]     -> "mode" and the N bins; how = search
//       (the search at the dim's depth), guess ("refused" unless hist_guess_ok),
//       plan (what hist_dim_plan picks)
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

bool number(std::istream &in, double *x) {
  std::string w;
  if (!(in >> w)) return false;
  const uint64_t bits = std::stoull(w, nullptr, 16);
  std::memcpy(x, &bits, 8);
  return true;
}

bool bins_of(std::istream &in, int32_t d, std::vector<int32_t> *n_bins) {
  n_bins->resize((size_t)d);
  for (int32_t &b : *n_bins)
    if (!(in >> b)) return false;
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
    if (cmd == "check") {
      int32_t d;
      std::vector<int32_t> n_bins;
      if (!(ls >> d) || d < 1 || d > 32 || !bins_of(ls, d, &n_bins)) return 3;
      // (as many edges as the request holds: a refused n_bins reads none)
      std::vector<double> edges;
      double x;
      while (number(ls, &x)) edges.push_back(x);
      edges.push_back(0.);
      const std::string bad = pbh::hist_check_edges(d, n_bins.data(), edges.data());
      std::cout << (bad.empty() ? "ok" : bad) << "\n";
    } else if (cmd == "pairs") {
      int32_t d, n_pairs;
      std::vector<int32_t> n_bins;
      if (!(ls >> d) || d < 1 || d > 32 || !bins_of(ls, d, &n_bins) || !(ls >> n_pairs)) return 3;
      std::vector<int32_t> pairs((size_t)(n_pairs > 0 ? 2 * n_pairs : 0) + 2);
      // (as many as the request holds: a refused n_pairs reads none)
      for (int32_t i = 0; i < 2 * n_pairs; ++i)
        if (!(ls >> pairs[(size_t)i])) break;
      const std::string bad = pbh::hist2d_check_pairs(d, n_bins.data(), n_pairs, pairs.data());
      std::cout << (bad.empty() ? "ok" : bad) << "\n";
    } else if (cmd == "layout") {
      int64_t n, count;
      int32_t d;
      if (!(ls >> n >> count >> d)) return 3;
      std::vector<int32_t> n_bins;
      if (d >= 1 && d <= 32 && !bins_of(ls, d, &n_bins)) return 3;
      n_bins.resize(33);
      pbh::HistLayout l;
      std::memset(&l, 0x5a, sizeof l);
      if (!pbh::hist_layout(n, count, d, n_bins.data(), &l)) {
        // a refusal leaves `out` untouched
        const unsigned char *p = reinterpret_cast<const unsigned char *>(&l);
        for (size_t i = 0; i < sizeof l; ++i)
          if (p[i] != 0x5a) return 4;
        std::cout << "refused\n";
        continue;
      }
      std::cout << "ok " << l.dims << ' ' << l.groups << ' ' << l.lds_bytes << ' '
                << l.chain_blocks << ' ' << l.slices << ' ' << l.slice_len << ' ' << l.n_tab << ' '
                << l.n_ctr << ' ' << l.tables << ' ' << l.counts << ' ' << l.bytes;
      for (int j = 0; j < l.dims; ++j)
        std::cout << ' ' << l.dim[j] << ' ' << l.tab[j] << ' ' << l.ctr[j];
      for (int g = 0; g < l.groups; ++g)
        std::cout << ' ' << l.group_first[g] << ' ' << l.tab_off[g] << ' ' << l.tab_len[g] << ' '
                  << l.ctr_off[g] << ' ' << l.ctr_len[g];
      if (l.group_first[l.groups] != l.dims) return 4;
      std::cout << "\n";
    } else if (cmd == "layout2d") {
      int64_t n, count;
      int32_t d, n_pairs;
      std::vector<int32_t> n_bins;
      if (!(ls >> n >> count >> d) || d < 1 || d > 32 || !bins_of(ls, d, &n_bins) ||
          !(ls >> n_pairs))
        return 3;
      std::vector<int32_t> pairs((size_t)(n_pairs > 0 ? 2 * n_pairs : 0) + 2);
      // (as many as the request holds: a refused n_pairs reads none)
      for (int32_t i = 0; i < 2 * n_pairs; ++i)
        if (!(ls >> pairs[(size_t)i])) break;
      pbh::Hist2dLayout l;
      l.n_pairs = -7;
      if (!pbh::hist2d_layout(n, count, d, n_bins.data(), n_pairs, pairs.data(), &l)) {
        if (l.n_pairs != -7 || !l.out.empty()) return 4;
        std::cout << "refused\n";
        continue;
      }
      if ((int32_t)l.out.size() != n_pairs || l.n_pairs != n_pairs) return 4;
      std::cout << "ok " << l.lds_bytes << ' ' << l.chain_blocks << ' ' << l.slices << ' '
                << l.slice_len << ' ' << l.n_tab << ' ' << l.n_ctr << ' ' << l.tables << ' '
                << l.pairs << ' ' << l.counts << ' ' << l.bytes;
      for (int k = 0; k < d; ++k) std::cout << ' ' << l.tab_off[k];
      for (int64_t at : l.out) std::cout << ' ' << at;
      std::cout << "\n";
    } else if (cmd == "guess_ok" || cmd == "bins") {
      std::string how;
      if (cmd == "bins" && !(ls >> how)) return 3;
      int32_t B;
      if (!(ls >> B) || B < 1 || B > 4096) return 3;
      std::vector<double> e((size_t)B + 1);
      for (double &x : e)
        if (!number(ls, &x)) return 3;
      const bool ok = pbh::hist_guess_ok(e.data(), B);
      if (cmd == "guess_ok") {
        std::cout << (ok ? 1 : 0) << "\n";
        continue;
      }
      int64_t N;
      if (!(ls >> N) || N < 0) return 3;
      pbh::HistDimPlan p = pbh::hist_dim_plan(e.data(), B);
      if (p.bins != B || p.e0 != e[0] || p.eB != e[(size_t)B]) return 4;
      if ((p.mode == pbh::kHistGuess) != ok) return 4;
      if (how == "search") {
        p.mode = pbh::hist_depth(B);
      } else if (how == "guess") {
        if (!ok) {
          std::cout << "refused\n";
          continue;
        }
      } else if (how != "plan") {
        return 3;
      }
      // exactly the table's length: the sanitizer sees a read past it
      std::vector<double> t((size_t)pbh::hist_table_len(B));
      pbh::hist_fill_table(e.data(), p, t.data());
      std::cout << p.mode;
      for (int64_t i = 0; i < N; ++i) {
        double x;
        if (!number(ls, &x)) return 3;
        std::cout << ' ' << pbh::hist_bin_any(p.mode, t.data(), B, p.e0, p.eB, p.s, x);
      }
      std::cout << "\n";
    } else {
      return 3;
    }
  }
  return 0;
}
