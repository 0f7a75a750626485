// pbh_expr_data.hip -- the kernels of a PBH_TARGET_EXPR program with loop
// regions (pbhip.h: a likelihood summed over observed data columns):
// mh_kernel<D, RNG, kTargetExprData, 0> for d = 1..16 and the four RNG modes,
// and pbh_eval_expr_data's kernel.  The programs without regions keep the
// kernels of pbh_expr.hip.
//
// The outer program is interpreted as in expr_density.  A region LOOP, body,
// SUM is the sum over the observations j of the body's last value, in the
// order of NumPy's 1-D pairwise sum: the engine lists the leaves of that
// recursion for the model's n (KArgs.eleaf, expr_leaf_word), every leaf a block
// of at most 128 consecutive terms that starts at a multiple of 8, and how
// many pending left sums its result is added to.  A leaf is np_leaf's order:
// below 8 terms one after another from 0., else eight accumulators r[k] over
// the blocks of 8, ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the
// remaining terms one after another.
//
// The body (ewide): every body word is decoded once per block of 8 consecutive
// observations and applied to all 8 -- the leaf's eight accumulators take the
// 8 results, so the order is np_leaf's, and the 8 chains of operations are
// independent.  j is wave-uniform: the 8 values of a data column are one
// 64-byte scalar load (columns are padded to a multiple of 8 doubles and
// 64-byte aligned; a block past n reads the zero padding, whose results are
// not used).  Body temporaries live in LDS as [temp][8][thread]; the pending
// sums of the walk are registers selected by the uniform stack index.  Nothing
// is a runtime-indexed private array.  ewide = 0 evaluates the same body one
// observation at a time into the same 8 results (the comparison form).
#include "pbh_kernels_impl.h"

namespace pbh {

namespace {

constexpr int kW = 8;                          // observations per body block
constexpr int kExprTemps = PBH_EXPR_MAX_TEMPS;
constexpr int kExprCols = PBH_EXPR_MAX_COLS;

// One body operand for the W observations j0 .. j0 + W - 1.  sl: the outer
// slots [slot][thread], tl: the body temporaries [temp][8][thread], both at
// this thread.  The masks only keep a wrong word inside the blocks.
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

// The body words pc0 .. pc0 + len - 1 for the observations j0 .. j0 + W - 1;
// acc: the body's last value for each of them.
template <int D, int W>
__device__ __forceinline__ void expr_body(const KArgs &a, const double (&x)[D],
                                          const double *sl, double *tl, int pc0, int len,
                                          int j0, double (&acc)[W]) {
#pragma unroll
  for (int i = 0; i < W; ++i) acc[i] = 0.;
  for (int pc = pc0; pc < pc0 + len; ++pc) {
    const uint32_t w = __builtin_amdgcn_readfirstlane(cldw(a.ecode, pc));
    const uint32_t op = w & 63u;
    double va[W], vb[W], r[W];
    body_operand<D, W>(a, x, sl, tl, acc, (w >> 11) & 3u, (w >> 13) & 255u, j0, va);
    if ((op >= PBH_EXPR_ADD && op <= PBH_EXPR_DIV) || op >= PBH_EXPR_MAX) {
      body_operand<D, W>(a, x, sl, tl, acc, (w >> 21) & 3u, (w >> 23) & 255u, j0, vb);
    } else {
#pragma unroll
      for (int i = 0; i < W; ++i) vb[i] = 0.;
    }
#define PBH_EACH(EXPR)              \
  _Pragma("unroll")                 \
  for (int i = 0; i < W; ++i) r[i] = (EXPR); \
  break;
    switch (op) {
      case PBH_EXPR_ADD: PBH_EACH(va[i] + vb[i])
      case PBH_EXPR_SUB: PBH_EACH(va[i] - vb[i])
      case PBH_EXPR_MUL: PBH_EACH(va[i] * vb[i])
      case PBH_EXPR_DIV: PBH_EACH(va[i] / vb[i])
      case PBH_EXPR_NEG: PBH_EACH(-va[i])
      case PBH_EXPR_ABS: PBH_EACH(__builtin_fabs(va[i]))
      case PBH_EXPR_SQRT: PBH_EACH(sqrt(va[i]))
      case PBH_EXPR_EXP: PBH_EACH(exp(va[i]))
      case PBH_EXPR_LOG: PBH_EACH(log(va[i]))
      case PBH_EXPR_LOG1P: PBH_EACH(log1p(va[i]))
      case PBH_EXPR_EXPM1: PBH_EACH(expm1(va[i]))
      case PBH_EXPR_MAX: PBH_EACH(np_maximum(va[i], vb[i]))
      case PBH_EXPR_MIN: PBH_EACH(np_minimum(va[i], vb[i]))
      case PBH_EXPR_POW: PBH_EACH(pow(va[i], vb[i]))
      default: PBH_EACH(va[i])   // PBH_EXPR_MOV
    }
#undef PBH_EACH
#pragma unroll
    for (int i = 0; i < W; ++i) acc[i] = r[i];
    if ((w >> 10) & 1u) {
      double *t = tl + ((w >> 6) & (kExprTemps - 1)) * (kW * kBlock);
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
    const int s = (int)(lw & 8191u) * kW, m = (int)((lw >> 13) & 255u);
    const int pops = (int)(lw >> 21);
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

// expr_density with regions: LOOP runs the region and leaves its sum in the
// accumulator; the SUM word that follows the body is a MOV of the accumulator
// (its operand kind), which stores the sum where the program keeps it.
template <int D>
__device__ __forceinline__ double expr_data_density(const KArgs &a, const double (&x)[D]) {
  __shared__ double s_slot[kExprSlots * kBlock];
  __shared__ double s_temp[kExprTemps * kW * kBlock];
  double *const sl = s_slot + threadIdx.x;
  double *const tl = s_temp + threadIdx.x;
  double acc = 0.;
  const int n = a.en;
  for (int pc = 0; pc < n; ++pc) {
    const uint32_t w = __builtin_amdgcn_readfirstlane(cldw(a.ecode, pc));
    const uint32_t op = w & 63u;
    if (op == PBH_EXPR_LOOP) {
      const int len = (int)((w >> 13) & 255u);
      acc = expr_region<D>(a, x, sl, tl, pc + 1, len);
      pc += len;   // the next word is the region's SUM
      continue;
    }
    const double va = expr_operand<D>(a, x, sl, acc, (w >> 11) & 3u, (w >> 13) & 255u);
    double vb = 0.;
    if (((op >= PBH_EXPR_ADD && op <= PBH_EXPR_DIV) || op >= PBH_EXPR_MAX) &&
        op < PBH_EXPR_N_OPS)
      vb = expr_operand<D>(a, x, sl, acc, (w >> 21) & 3u, (w >> 23) & 255u);
    double r;
    switch (op) {
      case PBH_EXPR_ADD: r = va + vb; break;
      case PBH_EXPR_SUB: r = va - vb; break;
      case PBH_EXPR_MUL: r = va * vb; break;
      case PBH_EXPR_DIV: r = va / vb; break;
      case PBH_EXPR_NEG: r = -va; break;
      case PBH_EXPR_ABS: r = __builtin_fabs(va); break;
      case PBH_EXPR_SQRT: r = sqrt(va); break;
      case PBH_EXPR_EXP: r = exp(va); break;
      case PBH_EXPR_LOG: r = log(va); break;
      case PBH_EXPR_LOG1P: r = log1p(va); break;
      case PBH_EXPR_EXPM1: r = expm1(va); break;
      case PBH_EXPR_MAX: r = np_maximum(va, vb); break;
      case PBH_EXPR_MIN: r = np_minimum(va, vb); break;
      case PBH_EXPR_POW: r = pow(va, vb); break;
      default: r = va; break;   // PBH_EXPR_MOV, PBH_EXPR_SUM
    }
    acc = r;
    if ((w >> 10) & 1u) sl[((w >> 6) & (kExprSlots - 1)) * kBlock] = r;
  }
  return acc;
}

// pbh_eval_expr_data: the program at n points x [d][n] (a.d variables)
__global__ __launch_bounds__(kBlock) void expr_data_eval_kernel(KArgs a, int64_t n,
                                                                const double *xs,
                                                                double *out) {
  const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t cc = c < n ? c : 0;
  double x[PBH_EXPR_MAX_DIM];
#pragma unroll
  for (int k = 0; k < PBH_EXPR_MAX_DIM; ++k) x[k] = k < a.d ? xs[k * n + cc] : 0.;
  const double v = expr_data_density<PBH_EXPR_MAX_DIM>(a, x);
  if (c < n) out[c] = v;
}

}  // namespace

hipError_t launch_mh_expr_data(const KArgs &a, hipStream_t s) {
  switch (a.d) {
#define PBH_CASE(D)                                  \
  case D:                                            \
    launch_mh_spec<D, kTargetExprData, 0>(a, s, 0);  \
    return hipGetLastError();
    PBH_CASE(1) PBH_CASE(2) PBH_CASE(3) PBH_CASE(4) PBH_CASE(5) PBH_CASE(6)
    PBH_CASE(7) PBH_CASE(8) PBH_CASE(9) PBH_CASE(10) PBH_CASE(11) PBH_CASE(12)
    PBH_CASE(13) PBH_CASE(14) PBH_CASE(15) PBH_CASE(16)
#undef PBH_CASE
    default:
      return hipErrorInvalidValue;
  }
}

hipError_t launch_eval_expr_data(const KArgs &a, int64_t n, const double *x, double *out) {
  const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
  hipLaunchKernelGGL(expr_data_eval_kernel, grid, block, 0, 0, a, n, x, out);
  hipError_t err = hipGetLastError();
  if (err == hipSuccess) err = hipDeviceSynchronize();
  return err;
}

}  // namespace pbh
