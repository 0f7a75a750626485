// pbh_expr_words.h -- the words of a PBH_TARGET_EXPR program (pbhip.h) and of
// its pairwise-sum leaves: the interpreter (pbh_expr_impl.h) and the host's checker
// (pbh_expr_host.cpp) read every field through these helpers.  No HIP header needed.
#pragma once
#include <stdint.h>
#include "../../include/pbhip.h"

#if defined(__HIPCC__)
#define PBH_HD __host__ __device__
#else
#define PBH_HD
#endif

namespace pbh {

// code word = op | dst << 6 | store << 10 | akind << 11 | aidx << 13 | bkind << 21
//             | bidx << 23; a LOOP word holds its body's length in aidx
PBH_HD inline uint32_t expr_op(uint32_t w) { return w & 63u; }
PBH_HD inline uint32_t expr_dst(uint32_t w) { return (w >> 6) & 15u; }
PBH_HD inline bool expr_store(uint32_t w) { return (w >> 10) & 1u; }
PBH_HD inline uint32_t expr_a_kind(uint32_t w) { return (w >> 11) & 3u; }
PBH_HD inline uint32_t expr_a_idx(uint32_t w) { return (w >> 13) & 255u; }
PBH_HD inline uint32_t expr_b_kind(uint32_t w) { return (w >> 21) & 3u; }
PBH_HD inline uint32_t expr_b_idx(uint32_t w) { return (w >> 23) & 255u; }
PBH_HD inline int expr_loop_len(uint32_t w) { return (int)expr_a_idx(w); }
// an elementwise opcode (< PBH_EXPR_N_OPS) that reads operand B
PBH_HD inline bool expr_binary(uint32_t op) {
  return (op >= PBH_EXPR_ADD && op <= PBH_EXPR_DIV) || op >= PBH_EXPR_MAX;
}
// doubles the uploaded block keeps for the constants; the code words follow
constexpr int kExprConstPad = 256;

// One leaf of the pairwise sum (NumPy's pairwise_sum: a block of at most 128
// terms that starts at a multiple of 8): start / 8 | terms << 13 | pops << 21,
// pops = the pending left sums this leaf's result is then added to.
constexpr int kExprLeafStack = 12;   // pending sums: 8 at 65 536 terms
PBH_HD inline uint32_t expr_leaf_word(int start, int terms, int pops) {
  return (uint32_t)(start / 8) | ((uint32_t)terms << 13) | ((uint32_t)pops << 21);
}
PBH_HD inline int expr_leaf_start(uint32_t lw) { return (int)(lw & 8191u) * 8; }
PBH_HD inline int expr_leaf_terms(uint32_t lw) { return (int)((lw >> 13) & 255u); }
PBH_HD inline int expr_leaf_pops(uint32_t lw) { return (int)(lw >> 21); }

}  // namespace pbh
