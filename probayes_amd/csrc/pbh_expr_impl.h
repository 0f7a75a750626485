// pbh_expr_impl.h -- PBH_TARGET_EXPR: the interpreter of a density given as a
// program (pbhip.h pbh_expr_op; probayes_amd/expr.py evaluate() is the NumPy
// definition; DESIGN.md section 4 has the design), its eval kernel and its
// launchers.  Only the two expression units include it: pbh_expr.hip makes the
// form without loop regions (DATA = false), pbh_expr_data.hip the one with.
//
// Every lane runs the same program on its own chain, so the program counter,
// every decoded field and the observation index are wave-uniform: words,
// constants and data columns are scalar loads through the constant address
// space, the opcode dispatch is a scalar branch.  The previous result stays in
// a register (acc); slots live in LDS as [slot][thread], body temporaries as
// [temp][8][thread]; a variable or a pending sum is an unrolled select on a
// uniform index: nothing is a runtime-indexed private array.  The host checked
// the program (expr_check); the index masks only keep a wrong word inside its
// block.  -ffp-contract=off: + - * / are NumPy's IEEE operations; exp / log /
// log1p / expm1 / pow are OCML's in every RNG mode.
// A region LOOP, body, SUM sums the body's last value over the observations in
// np.sum's order: the engine lists the leaves (KArgs.eleaf, expr_leaf_word),
// each at most 128 consecutive terms from a multiple of 8, and how many pending
// left sums its result is added to.  A leaf below 8 terms adds them one by one
// from 0.; else eight accumulators r[k] run over the blocks of 8, ((r0 + r1) +
// (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the last terms one by one.  ewide:
// a body word is decoded once per block of 8 observations (one 64-byte load per
// column: zero-padded to 8, 64-byte aligned) and applied to all 8, the leaf's 8
// accumulators; ewide = 0: one observation at a time into the same 8 results.
#pragma once
#include "pbh_kernels_impl.h"

namespace pbh {
namespace {

constexpr int kExprSlots = PBH_EXPR_MAX_SLOTS, kExprTemps = PBH_EXPR_MAX_TEMPS;
constexpr int kExprCols = PBH_EXPR_MAX_COLS, kW = 8;   // kW: observations per body block

__device__ __forceinline__ uint32_t cldw(const int32_t *p, int i) {
  return (uint32_t)((const __attribute__((address_space(4))) int32_t *)p)[i];
}

// The arithmetic of each elementwise opcode but MOV, stated once: X(opcode,
// its value for the operands va, vb).  log1p and expm1 of -0. are -0. (C99, and
// NumPy's) where OCML's are +0.: both functions have the sign of their operand
// wherever they are a number, so the result takes it (one bit-field insert; a
// compare and select on the operand cost the d = 10 kernels 6 % of their rate).
#define PBH_EXPR_OPS(X)                                                                \
  X(ADD, va + vb) X(SUB, va - vb) X(MUL, va * vb) X(DIV, va / vb) X(NEG, -va)          \
  X(ABS, __builtin_fabs(va)) X(SQRT, sqrt(va)) X(EXP, exp(va)) X(LOG, log(va))         \
  X(LOG1P, __builtin_copysign(log1p(va), va)) X(EXPM1, __builtin_copysign(expm1(va), va)) \
  X(MAX, np_maximum(va, vb))                                                           \
  X(MIN, np_minimum(va, vb)) X(POW, pow(va, vb))

__device__ __forceinline__ double expr_apply(uint32_t op, double va, double vb) {
  switch (op) {
#define PBH_ONE(OP, VALUE) case PBH_EXPR_##OP: return VALUE;
    PBH_EXPR_OPS(PBH_ONE)
#undef PBH_ONE
    default: return va;   // PBH_EXPR_MOV, PBH_EXPR_SUM
  }
}

template <int D>
__device__ __forceinline__ double expr_operand(const KArgs &a, const double (&x)[D],
                                               const double *sl, double acc,
                                               uint32_t kind, uint32_t idx) {
  if (kind == PBH_EXPR_SLOT) return sl[(idx & (kExprSlots - 1)) * kBlock];
  if (kind == PBH_EXPR_CONST) return cld(a.econst, idx & (kExprConstPad - 1));
  if (kind == PBH_EXPR_ACC) return acc;
  double v = 0.;
#pragma unroll
  for (int k = 0; k < D; ++k)
    if (k == (int)idx) v = x[k];
  return v;
}

// One body operand for the W observations j0 .. j0 + W - 1.  sl: the outer
// slots [slot][thread], tl: the body temporaries [temp][8][thread], at this thread.
template <int D, int W>
__device__ __forceinline__ void body_operand(const KArgs &a, const double (&x)[D],
                                             const double *sl, const double *tl,
                                             const double (&acc)[W], uint32_t kind,
                                             uint32_t idx, int j0, double (&v)[W]) {
  if (kind == PBH_EXPR_ACC) {
#pragma unroll
    for (int i = 0; i < W; ++i) v[i] = acc[i];
    return;
  }
  if (kind == PBH_EXPR_SLOT && idx >= PBH_EXPR_BODY_BASE) {
    const double *t = tl + ((idx - PBH_EXPR_BODY_BASE) & (kExprTemps - 1)) * (kW * kBlock);
#pragma unroll
    for (int i = 0; i < W; ++i) v[i] = t[i * kBlock];
    return;
  }
  if (kind == PBH_EXPR_VAR && idx >= PBH_EXPR_BODY_BASE) {
    const double *col = a.edata +
        (int64_t)((idx - PBH_EXPR_BODY_BASE) & (kExprCols - 1)) * a.enpad + j0;
#pragma unroll
    for (int i = 0; i < W; ++i) v[i] = cld(col, i);
    return;
  }
  double s;   // the same for every observation
  if (kind == PBH_EXPR_SLOT) {
    s = sl[(idx & (kExprSlots - 1)) * kBlock];
  } else if (kind == PBH_EXPR_CONST) {
    s = cld(a.econst, idx & (kExprConstPad - 1));
  } else {
    s = 0.;
#pragma unroll
    for (int k = 0; k < D; ++k)
      if (k == (int)idx) s = x[k];
  }
#pragma unroll
  for (int i = 0; i < W; ++i) v[i] = s;
}

// The body words pc0 .. pc0 + len - 1 for the observations j0 .. j0 + W - 1; acc: the
// body's last value for each.  The opcode dispatch outside, the W observations inside.
template <int D, int W>
__device__ __forceinline__ void expr_body(const KArgs &a, const double (&x)[D],
                                          const double *sl, double *tl, int pc0, int len,
                                          int j0, double (&acc)[W]) {
#pragma unroll
  for (int i = 0; i < W; ++i) acc[i] = 0.;
  for (int pc = pc0; pc < pc0 + len; ++pc) {
    const uint32_t w = __builtin_amdgcn_readfirstlane(cldw(a.ecode, pc));
    const uint32_t op = expr_op(w);
    double va[W], vb[W], r[W];
    body_operand<D, W>(a, x, sl, tl, acc, expr_a_kind(w), expr_a_idx(w), j0, va);
    if (expr_binary(op)) {
      body_operand<D, W>(a, x, sl, tl, acc, expr_b_kind(w), expr_b_idx(w), j0, vb);
    } else {
#pragma unroll
      for (int i = 0; i < W; ++i) vb[i] = 0.;
    }
#define PBH_EACH(OP, VALUE)                                                     \
  case PBH_EXPR_##OP:                                                           \
    _Pragma("unroll")                                                           \
    for (int i = 0; i < W; ++i) r[i] = expr_apply(PBH_EXPR_##OP, va[i], vb[i]); \
    break;
    switch (op) {
      PBH_EXPR_OPS(PBH_EACH)
      default:
#pragma unroll
        for (int i = 0; i < W; ++i) r[i] = va[i];   // PBH_EXPR_MOV
    }
#undef PBH_EACH
#pragma unroll
    for (int i = 0; i < W; ++i) acc[i] = r[i];
    if (expr_store(w)) {
      double *t = tl + (expr_dst(w) & (kExprTemps - 1)) * (kW * kBlock);
#pragma unroll
      for (int i = 0; i < W; ++i) t[i * kBlock] = r[i];
    }
  }
}

// One region: the pairwise sum over the observations of the body's last value.
template <int D>
__device__ __forceinline__ double expr_region(const KArgs &a, const double (&x)[D],
                                              const double *sl, double *tl, int pc0,
                                              int len) {
  double st[kExprLeafStack];   // pending left sums; sp is wave-uniform
#pragma unroll
  for (int k = 0; k < kExprLeafStack; ++k) st[k] = 0.;
  int sp = 0;
  double v = 0.;
  const bool wide = a.ewide != 0;
  for (int q = 0; q < a.enleaf; ++q) {
    const uint32_t lw = __builtin_amdgcn_readfirstlane(cldw(a.eleaf, q));
    const int s = expr_leaf_start(lw), m = expr_leaf_terms(lw);
    const int pops = expr_leaf_pops(lw);
    const int nfull = m >> 3, rem = m & 7, nblk = (m + 7) >> 3;
    double r[kW], res = 0.;
#pragma unroll
    for (int k = 0; k < kW; ++k) r[k] = 0.;
    for (int b = 0; b < nblk; ++b) {
      const int j0 = s + b * kW;
      double t[kW];
      if (wide) {
        expr_body<D, kW>(a, x, sl, tl, pc0, len, j0, t);
      } else {
        const int cnt = m - b * kW < kW ? m - b * kW : kW;
#pragma unroll
        for (int k = 0; k < kW; ++k) t[k] = 0.;
        for (int i = 0; i < cnt; ++i) {
          double one[1];
          expr_body<D, 1>(a, x, sl, tl, pc0, len, j0 + i, one);
#pragma unroll
          for (int k = 0; k < kW; ++k)
            if (k == i) t[k] = one[0];
        }
      }
      if (b < nfull) {   // a whole block: the eight accumulators
#pragma unroll
        for (int k = 0; k < kW; ++k) r[k] = b == 0 ? t[k] : r[k] + t[k];
        if (b == nfull - 1)
          res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
      } else {           // the last terms (all of them below 8), one by one
#pragma unroll
        for (int k = 0; k < kW; ++k)
          if (k < rem) res += t[k];
      }
    }
    v = res;
    for (int p = 0; p < pops; ++p) {   // left + right, innermost first
      --sp;
      double left = 0.;
#pragma unroll
      for (int k = 0; k < kExprLeafStack; ++k)
        if (k == sp) left = st[k];
      v = left + v;
    }
#pragma unroll
    for (int k = 0; k < kExprLeafStack; ++k)
      if (k == sp) st[k] = v;
    ++sp;
  }
  return v;
}

// The program at x.  DATA: LOOP runs the region and leaves its sum in the accumulator;
// the SUM word after the body is a MOV of the accumulator, which may store the sum.
template <int D, bool DATA>
__device__ __forceinline__ double expr_density(const KArgs &a, const double (&x)[D]) {
  __shared__ double s_slot[kExprSlots * kBlock];
  double *const sl = s_slot + threadIdx.x;
  double *tl = nullptr;
  if constexpr (DATA) {
    __shared__ double s_temp[kExprTemps * kW * kBlock];
    tl = s_temp + threadIdx.x;
  }
  double acc = 0.;
  const int n = a.en;
  for (int pc = 0; pc < n; ++pc) {
    const uint32_t w = __builtin_amdgcn_readfirstlane(cldw(a.ecode, pc));
    const uint32_t op = expr_op(w);
    bool binary = expr_binary(op);
    if constexpr (DATA) {
      if (op == PBH_EXPR_LOOP) {
        const int len = expr_loop_len(w);
        acc = expr_region<D>(a, x, sl, tl, pc + 1, len);
        pc += len;   // the next word is the region's SUM
        continue;
      }
      binary = binary && op < PBH_EXPR_N_OPS;   // not the SUM word
    }
    const double va = expr_operand<D>(a, x, sl, acc, expr_a_kind(w), expr_a_idx(w));
    double vb = 0.;
    if (binary) vb = expr_operand<D>(a, x, sl, acc, expr_b_kind(w), expr_b_idx(w));
    const double r = expr_apply(op, va, vb);
    acc = r;
    if (expr_store(w)) sl[(expr_dst(w) & (kExprSlots - 1)) * kBlock] = r;
  }
  return acc;
}

// pbh_eval_expr / pbh_eval_expr_data: the program at n points x [d][n] (a.d variables)
template <bool DATA>
__global__ __launch_bounds__(kBlock) void expr_eval_kernel(KArgs a, int64_t n, const double *xs,
                                                           double *out) {
  const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t cc = c < n ? c : 0;
  double x[PBH_EXPR_MAX_DIM];
#pragma unroll
  for (int k = 0; k < PBH_EXPR_MAX_DIM; ++k) x[k] = k < a.d ? xs[k * n + cc] : 0.;
  const double v = expr_density<PBH_EXPR_MAX_DIM, DATA>(a, x);
  if (c < n) out[c] = v;
}

// The launchers of one form: mh_kernel<D, RNG, TGT, 0> for d = 1..16 and the
// four RNG modes, and the eval kernel.  Each expression unit instantiates one.
template <bool DATA>
hipError_t launch_mh_expr_form(const KArgs &a, hipStream_t s) {
  constexpr int TGT = DATA ? kTargetExprData : (int)PBH_TARGET_EXPR;
  switch (a.d) {
#define PBH_CASE(D) case D: launch_mh_spec<D, TGT, 0>(a, s, 0); return hipGetLastError();
    PBH_CASE(1) PBH_CASE(2) PBH_CASE(3) PBH_CASE(4) PBH_CASE(5) PBH_CASE(6)
    PBH_CASE(7) PBH_CASE(8) PBH_CASE(9) PBH_CASE(10) PBH_CASE(11) PBH_CASE(12)
    PBH_CASE(13) PBH_CASE(14) PBH_CASE(15) PBH_CASE(16)
#undef PBH_CASE
    default:
      return hipErrorInvalidValue;
  }
}

template <bool DATA>
hipError_t launch_eval_expr_form(const KArgs &a, int64_t n, const double *x, double *out) {
  const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
  hipLaunchKernelGGL(expr_eval_kernel<DATA>, grid, block, 0, 0, a, n, x, out);
  hipError_t err = hipGetLastError();
  if (err == hipSuccess) err = hipDeviceSynchronize();
  return err;
}

}  // namespace

// the DATA = true forms (pbh_expr_data.hip), for pbh_expr.hip's launchers
hipError_t launch_mh_expr_data(const KArgs &a, hipStream_t s);
hipError_t launch_eval_expr_data(const KArgs &a, int64_t n, const double *x, double *out);

}  // namespace pbh
