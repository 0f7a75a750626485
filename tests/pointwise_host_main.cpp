// pointwise_host_main.cpp -- drives the host side of the pointwise reduction
// alone, on the CPU: pbh_trace_host.cpp's pointwise_layout, pointwise_combine
// and pointwise_finish, pbh_pointwise_merge.h (the very merges the kernels
// run) and pbh_expr_host.cpp's expr_check / expr_pointwise_error.
// tests/test_pointwise_host.py builds it with the address and
// undefined-behaviour sanitizers and -ffp-contract=off.  Reads requests from
// the file named on the command line, one per line, and answers each with one
// line.  A double travels as the 16 hex digits of its bits, both ways; every
// other number in decimal.
//   layout n count n_obs select_words prog_doubles
//       -> "bad untouched" / "bad touched" (a refusal, and whether `out` kept
//          the pattern it was filled with), or "ok chain_blocks tiles npad
//          slices slice_len rows select prog part res bytes"
//   shape d depth n_consts n_cols n_obs w0 w1 ..      (the code words)
//       -> "ok loop_pc", "check <pc> <text>" (expr_check refuses) or "shape
//          <text>" (expr_pointwise_error refuses)
//   lse ma sa mb sb         -> "m s" of lse_merge, then lse_value of it
//   mom na ka ma qa nb kb mb qb
//                           -> "n k mean m2" of moments_merge, then moments_mean
//   reduce rows live len v..
//       -> "lse mean var": one observation's terms v [rows][live][len] folded
//          as the device folds them -- per row (a workgroup) the lanes < live
//          push their len terms in order (lse_push, moments_push), the other
//          lanes of the 256 hold the identity, pointwise_combine merges the
//          lanes, and pointwise_finish merges the rows
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../probayes_amd/csrc/pbh_expr_host.h"
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
    std::string cmd;
    ls >> cmd;
    if (cmd == "layout") {
      int64_t n, count, n_obs, sel, prog;
      if (!(ls >> n >> count >> n_obs >> sel >> prog)) return 3;
      pbh::PointwiseLayout l, pattern;
      std::memset(&pattern, 0x5a, sizeof pattern);
      l = pattern;
      if (!pbh::pointwise_layout(n, count, (int32_t)n_obs, sel, prog, &l)) {
        std::cout << (std::memcmp(&l, &pattern, sizeof l) ? "bad touched" : "bad untouched")
                  << "\n";
        continue;
      }
      std::cout << "ok " << l.chain_blocks << ' ' << l.tiles << ' ' << l.npad << ' ' << l.slices
                << ' ' << l.slice_len << ' ' << l.rows << ' ' << l.select << ' ' << l.prog << ' '
                << l.part << ' ' << l.res << ' ' << l.bytes << "\n";
    } else if (cmd == "shape") {
      pbh::ExprProgram p;
      if (!(ls >> p.d >> p.depth >> p.n_consts >> p.n_cols >> p.n_obs)) return 3;
      std::vector<int32_t> code;
      long long w;
      while (ls >> w) code.push_back((int32_t)w);
      std::vector<double> consts((size_t)(p.n_consts > 0 ? p.n_consts : 1), 1.);
      std::vector<double> data((size_t)(p.n_cols > 0 && p.n_obs > 0 ? p.n_cols * p.n_obs : 1), 0.);
      p.code = code.data();
      p.n_code = (int32_t)code.size();
      p.consts = consts.data();
      p.data = p.n_cols ? data.data() : nullptr;
      int pc = -1;
      if (const char *bad = pbh::expr_check(p, &pc)) {
        std::cout << "check " << pc << ' ' << bad << "\n";
        continue;
      }
      int loop_pc = -1;
      if (const char *bad = pbh::expr_pointwise_error(p, &loop_pc)) {
        std::cout << "shape " << bad << "\n";
        continue;
      }
      std::cout << "ok " << loop_pc << "\n";
    } else if (cmd == "lse") {
      std::vector<double> v(4);
      if (!doubles(ls, v)) return 3;
      const pbh::LsePair r = pbh::lse_merge(pbh::LsePair{v[0], v[1]}, pbh::LsePair{v[2], v[3]});
      std::cout << hex(r.m) << ' ' << hex(r.s) << ' ' << hex(pbh::lse_value(r)) << "\n";
    } else if (cmd == "mom") {
      std::vector<double> v(8);
      if (!doubles(ls, v)) return 3;
      const pbh::Moments r = pbh::moments_merge(pbh::Moments{v[0], v[1], v[2], v[3]},
                                                pbh::Moments{v[4], v[5], v[6], v[7]});
      std::cout << hex(r.n) << ' ' << hex(r.k) << ' ' << hex(r.mean) << ' ' << hex(r.m2) << ' '
                << hex(pbh::moments_mean(r)) << "\n";
    } else if (cmd == "reduce") {
      int64_t rows, live, len;
      if (!(ls >> rows >> live >> len)) return 3;
      if (rows < 1 || live < 0 || live > pbh::kPointwiseLanes || len < 1) return 3;
      std::vector<double> v((size_t)(rows * live * len));
      if (!doubles(ls, v)) return 3;
      std::vector<pbh::LsePair> rl((size_t)rows);
      std::vector<pbh::Moments> rm((size_t)rows);
      for (int64_t r = 0; r < rows; ++r) {
        pbh::LsePair ll[pbh::kPointwiseLanes];
        pbh::Moments lm[pbh::kPointwiseLanes];
        for (int64_t c = 0; c < pbh::kPointwiseLanes; ++c) {
          ll[c] = pbh::lse_identity();
          lm[c] = pbh::moments_identity();
          for (int64_t i = 0; c < live && i < len; ++i) {
            const double t = v[(size_t)((r * live + c) * len + i)];
            ll[c] = pbh::lse_push(ll[c], t);
            lm[c] = pbh::moments_push(lm[c], t, 1. / (double)(i + 1));
          }
        }
        pbh::pointwise_combine(ll, lm, &rl[(size_t)r], &rm[(size_t)r]);
      }
      double lse, mean, var;
      pbh::pointwise_finish(rl.data(), rm.data(), rows, &lse, &mean, &var);
      std::cout << hex(lse) << ' ' << hex(mean) << ' ' << hex(var) << "\n";
    } else {
      return 3;
    }
  }
  return 0;
}
