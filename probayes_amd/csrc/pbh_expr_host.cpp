// pbh_expr_host.cpp -- see pbh_expr_host.h; no HIP (tests/test_expr_host.py).
#include "pbh_expr_host.h"

#include <cassert>
#include <cstring>

namespace pbh {

const char *expr_check(const ExprProgram &p, int *pc_out) {
  *pc_out = -1;
  if (p.d < 1 || p.d > PBH_EXPR_MAX_DIM) return "dim outside 1..16";
  if (!p.code || p.n_code < 1 || p.n_code > PBH_EXPR_MAX_CODE) return "code words outside 1..256";
  if (p.n_consts < 0 || p.n_consts > PBH_EXPR_MAX_CONSTS || (p.n_consts && !p.consts))
    return "constants outside 0..128 (or missing)";
  if (p.depth < 0 || p.depth > PBH_EXPR_MAX_SLOTS) return "depth outside 0..16";
  if (p.data || p.n_cols || p.n_obs) {
    if (!p.data) return "data columns missing";
    if (p.n_cols < 1 || p.n_cols > PBH_EXPR_MAX_COLS) return "data columns outside 1..8";
    if (p.n_obs < 1 || p.n_obs > PBH_EXPR_MAX_OBS) return "observations outside 1..65536";
  }
  uint32_t written = 0, temps = 0;
  int end = -1, first = 0;   // the open region's SUM word (-1: none), its first word
  for (int pc = 0; pc < p.n_code; ++pc) {
    *pc_out = pc;
    if (p.code[pc] < 0) return "code word with bit 31 set";
    const uint32_t w = (uint32_t)p.code[pc], op = expr_op(w);
    if (op == PBH_EXPR_LOOP) {
      if (end >= 0) return "nested loop region";
      if (!p.data) return "loop region in a program without data";
      const int len = expr_loop_len(w);
      end = pc + len + 1;
      if (len < 1 || end >= p.n_code || p.code[end] < 0 ||
          expr_op((uint32_t)p.code[end]) != PBH_EXPR_SUM)
        return "loop region does not end in SUM";
      first = pc + 1;
      temps = 0;
      continue;
    }
    const bool sum = op == PBH_EXPR_SUM;
    if (sum) {
      if (pc != end || expr_a_kind(w) != PBH_EXPR_ACC) return "SUM outside a loop region";
      end = -1;
    } else if (op >= PBH_EXPR_N_OPS) {
      return "unknown opcode";
    }
    const bool body = end >= 0;
    const bool binary = !sum && expr_binary(op);
    for (int j = 0; j < (binary ? 2 : 1); ++j) {
      const uint32_t kind = j ? expr_b_kind(w) : expr_a_kind(w);
      const uint32_t idx = j ? expr_b_idx(w) : expr_a_idx(w);
      if (body && idx >= PBH_EXPR_BODY_BASE && kind == PBH_EXPR_SLOT) {
        const uint32_t t = idx - PBH_EXPR_BODY_BASE;
        if (!(t < PBH_EXPR_MAX_TEMPS && ((temps >> t) & 1u)))
          return "body temporary read before the body wrote it (or outside the 4)";
        continue;
      }
      if (body && idx >= PBH_EXPR_BODY_BASE && kind == PBH_EXPR_VAR) {
        if (idx - PBH_EXPR_BODY_BASE >= (uint32_t)p.n_cols) return "data column out of range";
        continue;
      }
      if (kind == PBH_EXPR_SLOT && !(idx < (uint32_t)p.depth && ((written >> idx) & 1u)))
        return "slot read before it is written (or outside the depth)";
      if (kind == PBH_EXPR_VAR && idx >= (uint32_t)p.d) return "variable index outside the dims";
      if (kind == PBH_EXPR_CONST && idx >= (uint32_t)p.n_consts)
        return "constant index out of range";
      if (kind == PBH_EXPR_ACC && pc == (body ? first : 0))
        return body ? "accumulator read by a body's first word"
                    : "accumulator read by the first instruction";
    }
    if (expr_store(w)) {
      const uint32_t dst = expr_dst(w);
      if (body) {   // the store field names a body temporary: no outer slot is written
        if (dst >= PBH_EXPR_MAX_TEMPS) return "body stores outside its 4 temporaries";
        temps |= 1u << dst;
      } else {
        if (dst >= (uint32_t)p.depth) return "stored slot outside the depth";
        written |= 1u << dst;
      }
    }
  }
  return nullptr;
}

const char *expr_pointwise_error(const ExprProgram &p, int *loop_pc) {
  int loops = 0;
  *loop_pc = -1;
  for (int pc = 0; pc < p.n_code; ++pc)
    if (expr_op((uint32_t)p.code[pc]) == PBH_EXPR_LOOP) {
      if (loops++ == 0) *loop_pc = pc;
      pc += expr_loop_len((uint32_t)p.code[pc]);   // a body word may look like anything
    }
  if (loops == 0) return "a pointwise program needs a loop region (it has none)";
  if (loops > 1) return "a pointwise program has one loop region (it has several)";
  if (*loop_pc + expr_loop_len((uint32_t)p.code[*loop_pc]) + 1 != p.n_code - 1)
    return "a pointwise program ends in its region's SUM (words follow it)";
  return nullptr;
}

// NumPy's pairwise_sum over the terms [s, s + m) (loops_utils.h: at most 128
// terms are a leaf, else the left half rounded down to a multiple of 8, then
// the rest); `pops`: the ancestors this subtree is the right child of.
static int leaves_of(std::vector<uint32_t> &out, int s, int m, int pops, int pending) {
  if (m <= 128) {
    out.push_back(expr_leaf_word(s, m, pops));
    return pending + 1;
  }
  int m2 = m / 2;
  m2 -= m2 % 8;
  const int dl = leaves_of(out, s, m2, 0, pending);
  const int dr = leaves_of(out, s + m2, m - m2, pops + 1, pending + 1);
  return dl > dr ? dl : dr;
}

// np.sum adds the pairwise sums of its buffers of 8192 elements one after
// another: every chunk after the first is a right child of the total so far.
int expr_leaves(std::vector<uint32_t> &out, int n_obs) {
  constexpr int kChunk = 8192;   // NumPy's default buffer size, in elements
  int deepest = 0;
  for (int s = 0; s < n_obs; s += kChunk) {
    const int m = n_obs - s < kChunk ? n_obs - s : kChunk;
    const int d = leaves_of(out, s, m, s ? 1 : 0, s ? 1 : 0);
    if (d > deepest) deepest = d;
  }
  return deepest;
}

ExprLayout expr_pack(std::vector<double> &blk, const ExprProgram &p) {
  ExprLayout o;
  o.n_code = p.n_code;
  o.oconst = blk.size();
  o.ocode = o.oconst + kExprConstPad;
  blk.resize(o.ocode + PBH_EXPR_MAX_CODE / 2, 0.0);
  for (int i = 0; i < p.n_consts; ++i) blk[o.oconst + i] = p.consts[i];
  std::memcpy(&blk[o.ocode], p.code, (size_t)p.n_code * sizeof(int32_t));
  if (!p.data) return o;
  o.n_obs = p.n_obs;
  blk.resize((blk.size() + 7) / 8 * 8, 0.0);
  o.odata = blk.size();
  o.npad = (p.n_obs + 7) / 8 * 8;
  blk.resize(o.odata + (size_t)p.n_cols * o.npad, 0.0);
  for (int c = 0; c < p.n_cols; ++c)
    std::memcpy(&blk[o.odata + (size_t)c * o.npad], p.data + (size_t)c * p.n_obs,
                (size_t)p.n_obs * sizeof(double));
  std::vector<uint32_t> leaves;
  [[maybe_unused]] const int deepest = expr_leaves(leaves, p.n_obs);
  assert(deepest <= kExprLeafStack);   // 8 at PBH_EXPR_MAX_OBS terms
  o.nleaf = (int32_t)leaves.size();
  o.oleaf = blk.size();
  blk.resize(o.oleaf + (leaves.size() + 1) / 2, 0.0);
  std::memcpy(&blk[o.oleaf], leaves.data(), leaves.size() * sizeof(uint32_t));
  return o;
}

}  // namespace pbh
