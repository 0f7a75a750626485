// pbh_expr_host.h -- the host side of a PBH_TARGET_EXPR program: the check
// that lets the interpreter trust it, the leaves of its sums and its layout in the
// uploaded block.  No HIP: a host compiler alone builds it (tests/expr_host_main.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "pbh_expr_words.h"

namespace pbh {

// A program as the C-ABI passes it (pbh_model.expr_*, pbh_eval_expr*): a view,
// nothing is owned.  data / n_cols / n_obs are null / 0 / 0 without regions.
struct ExprProgram {
  int32_t d = 0;
  const int32_t *code = nullptr;
  int32_t n_code = 0;
  const double *consts = nullptr;
  int32_t n_consts = 0, depth = 0;
  const double *data = nullptr;   // [n_cols][n_obs]
  int32_t n_cols = 0, n_obs = 0;
};

// Every opcode, every operand's index for its kind, reads only after writes,
// the regions, the limits (pbhip.h).  nullptr, or what is wrong (*pc: where).
const char *expr_check(const ExprProgram &p, int *pc);
// Whether a program that passed expr_check has the pointwise shape
// (pbh_trace_pointwise): exactly one LOOP, and the region's SUM the last word.
// nullptr and *loop_pc = where the LOOP word stands, or what is wrong.
const char *expr_pointwise_error(const ExprProgram &p, int *loop_pc);
// The leaves of np.sum over n_obs contiguous terms, in order (expr_leaf_word): NumPy's
// pairwise sum of each buffer of 8192 terms, the buffers added one after another.
// Returns the deepest stack of pending sums (<= kExprLeafStack to PBH_EXPR_MAX_OBS).
int expr_leaves(std::vector<uint32_t> &out, int n_obs);
// Where expr_pack put a program in the block, in doubles from its start
// (n_code 0: no program, n_obs 0: no regions).
struct ExprLayout {
  size_t oconst = 0, ocode = 0, odata = 0, oleaf = 0;
  int32_t n_code = 0, n_obs = 0, npad = 0, nleaf = 0;
};
// Appends a checked program to the block: kExprConstPad constants (zero-padded),
// PBH_EXPR_MAX_CODE code words (padded with MOV words), and with regions the
// columns, each zero-padded to npad = a multiple of 8 observations, from a
// multiple of 8 doubles (64 bytes: the block is 256-byte aligned), then the leaves.
ExprLayout expr_pack(std::vector<double> &blk, const ExprProgram &p);
// KArgs econst .. enleaf for the block at `base` on the device (a default
// layout clears them); a template so that this header needs no HIP type.
template <class Args>
void expr_bind(Args &a, const double *base, const ExprLayout &l) {
  a.econst = l.n_code ? base + l.oconst : nullptr;
  a.ecode = l.n_code ? reinterpret_cast<const int32_t *>(base + l.ocode) : nullptr;
  a.en = l.n_code;
  a.edata = l.n_obs ? base + l.odata : nullptr;
  a.eleaf = l.n_obs ? reinterpret_cast<const int32_t *>(base + l.oleaf) : nullptr;
  a.enobs = l.n_obs;
  a.enpad = l.npad;
  a.enleaf = l.nleaf;
}

}  // namespace pbh
