// expr_host_main.cpp -- drives probayes_amd/csrc/pbh_expr_host.cpp alone, on
// the CPU (tests/test_expr_host.py builds it with the address and
// undefined-behaviour sanitizers).  Reads requests from the file named on the
// command line, one per line, and answers each with one line:
//   check d depth n_consts n_cols n_obs n_code w0 w1 ...
//     -> "ok nleaf", or "bad pc message"; an accepted program is also packed
//        as the engine packs it (the constants and the data are zeros)
//   leaves n_obs
//     -> "leaves deepest w0 w1 ..." (expr_leaf_word)
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../probayes_amd/csrc/pbh_expr_host.h"

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  if (!in) return 2;
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string what;
    if (!(ls >> what)) continue;
    if (what == "leaves") {
      int n_obs = 0;
      ls >> n_obs;
      std::vector<uint32_t> leaves;
      const int deepest = pbh::expr_leaves(leaves, n_obs);
      std::cout << "leaves " << deepest;
      for (uint32_t lw : leaves) {
        // the decode helpers give back what the encoder took
        if (pbh::expr_leaf_word(pbh::expr_leaf_start(lw), pbh::expr_leaf_terms(lw),
                                pbh::expr_leaf_pops(lw)) != lw)
          return 3;
        std::cout << ' ' << lw;
      }
      std::cout << '\n';
    } else if (what == "check") {
      pbh::ExprProgram p;
      ls >> p.d >> p.depth >> p.n_consts >> p.n_cols >> p.n_obs >> p.n_code;
      if (!ls || p.n_code < 0 || p.n_consts < 0 || p.n_cols < 0 || p.n_obs < 0) return 2;
      std::vector<int32_t> code(p.n_code);
      for (int32_t &w : code) ls >> w;
      if (!ls) return 2;
      const std::vector<double> consts(p.n_consts, 0.);
      const std::vector<double> data((size_t)p.n_cols * p.n_obs, 0.);
      p.code = code.data();
      p.consts = p.n_consts ? consts.data() : nullptr;
      p.data = p.n_cols ? data.data() : nullptr;
      int pc = -1;
      if (const char *why = pbh::expr_check(p, &pc)) {
        std::cout << "bad " << pc << ' ' << why << '\n';
        continue;
      }
      std::vector<double> blk(3, 1.);   // the program does not start the block
      const pbh::ExprLayout lay = pbh::expr_pack(blk, p);
      if (lay.oconst != 3 || lay.ocode != 3 + pbh::kExprConstPad || lay.n_code != p.n_code ||
          (p.data && (lay.odata % 8 || lay.npad % 8 || lay.npad < p.n_obs ||
                      lay.oleaf + (lay.nleaf + 1) / 2 != blk.size())))
        return 3;
      std::cout << "ok " << lay.nleaf << '\n';
    } else {
      return 2;
    }
  }
  return 0;
}
