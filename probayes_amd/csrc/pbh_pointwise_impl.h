// pbh_pointwise_impl.h -- what the kernels that walk the terms of a pointwise
// program share (pbh_pointwise.hip: the statistics; pbh_pointwise_tail.hip: the
// smallest terms and the log-sum-exp of the rest): the workgroup's place in the
// grid (observation tile of 8, block of 256 chains, record slice), the walk
// over its records -- the draw loads issued a record ahead, the scalar prefix
// with its slots in LDS, the body once for the tile through expr_body<D, 8> --
// and the merge of the lanes' partials in the fixed order of
// pointwise_combine.  What a kernel does with the 8 terms of a record is its
// own: the walk hands them to a functor.
#pragma once
#include "pbh_expr_host.h"
#include "pbh_expr_impl.h"
#include "pbh_trace_host.h"

namespace pbh {
namespace {

static_assert(kPointwiseLanes == kBlock && kPointwiseTile == kW, "one lane layout");
static_assert(kExprTemps * kW >= 4 * kPointwiseTile, "the partials fit the temporaries");

struct PointwiseArgs {
  const double *tx;          // the trace [record][d][n]
  int64_t n, first, count;   // chains, the window
  int64_t slice_len, slices, rows, npad;
  int32_t d, loop_pc, body_len;
  double *part;              // [6][rows][npad]
};

constexpr int D = PBH_EXPR_MAX_DIM;

__device__ __forceinline__ void load_draw(const PointwiseArgs &p, int64_t r, int64_t c,
                                          double (&x)[D]) {
  const double *at = p.tx + (p.first + r) * p.d * p.n + c;
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = k < p.d ? at[k * p.n] : 0.;
}

// The workgroup (tile, blockIdx.y, blockIdx.z) of the grid: its first
// observation, its lane's chain (cc: the chain a lane past N reads in its
// place) and its records [r0, r1).
struct PointwiseGroup {
  int j0;
  int64_t block, slice, c, cc, r0, r1;
  bool live;
};

__device__ __forceinline__ PointwiseGroup pointwise_group(const PointwiseArgs &p, int tile) {
  PointwiseGroup g;
  g.block = blockIdx.y;
  g.slice = blockIdx.z;
  g.c = g.block * kBlock + threadIdx.x;
  g.live = g.c < p.n;
  g.cc = g.live ? g.c : p.n - 1;
  g.r0 = g.slice * p.slice_len;
  g.r1 = g.r0 + p.slice_len < p.count ? g.r0 + p.slice_len : p.count;
  g.j0 = tile * kW;
  return g;
}

// The records of the group in order: fold(i, t) with i the record's index in
// the slice and t [kW] the terms of the lane's draw at observations j0 .. j0 +
// kW - 1.  sl, tl: the lane's slots and body temporaries in LDS.
template <class Fold>
__device__ __forceinline__ void pointwise_walk(const KArgs &a, const PointwiseArgs &p,
                                               const PointwiseGroup &g, double *sl, double *tl,
                                               Fold &&fold) {
  double x[D], xn[D];
  load_draw(p, g.r0, g.cc, x);
  for (int64_t r = g.r0; r < g.r1; ++r) {
    load_draw(p, r + 1 < g.r1 ? r + 1 : r, g.cc, xn);
    // the scalar prefix: the words before LOOP
    double acc = 0.;
    for (int pc = 0; pc < p.loop_pc; ++pc) {
      const uint32_t w = __builtin_amdgcn_readfirstlane(cldw(a.ecode, pc));
      const uint32_t op = expr_op(w);
      const double va = expr_operand<D>(a, x, sl, acc, expr_a_kind(w), expr_a_idx(w));
      double vb = 0.;
      if (expr_binary(op)) vb = expr_operand<D>(a, x, sl, acc, expr_b_kind(w), expr_b_idx(w));
      acc = expr_apply(op, va, vb);
      if (expr_store(w)) sl[(expr_dst(w) & (kExprSlots - 1)) * kBlock] = acc;
    }
    double t[kW];
    expr_body<D, kW>(a, x, sl, tl, p.loop_pc + 1, p.body_len, g.j0, t);
    fold(r - g.r0, t);
#pragma unroll
    for (int k = 0; k < D; ++k) x[k] = xn[k];
  }
}

// The lanes' partials of the tile's observations merged in the fixed order of
// pointwise_combine, after the walk (the slots and the temporaries are free by
// then).  The partials go over the temporaries, [observation][m, s, mean, M2]
// [lane], and over the slots: the counts [lane], the 32 folded counts of each
// observation, then the shifts [observation][lane]; 32 threads per observation
// merge them, thread t the lanes t, t + 32, .., then the 32 results fold by
// halves.  A lane that is not live holds the merges' identity.  Returns to the
// thread with *t_out == 0 the result of observation *o_out.
__device__ __forceinline__ void pointwise_merge_lanes(const LsePair (&lse)[kW],
                                                      const Moments (&mom)[kW], bool live,
                                                      double *s_slot, double *s_temp,
                                                      LsePair *fl_out, Moments *fm_out,
                                                      int *o_out, int *t_out) {
  __syncthreads();
  double *const s_n = s_slot, *const s_fn = s_slot + kBlock, *const s_k = s_slot + 2 * kBlock;
  s_n[threadIdx.x] = live ? mom[0].n : 0.;
#pragma unroll
  for (int i = 0; i < kW; ++i) {
    double *q = s_temp + (i * 4) * kBlock + threadIdx.x;
    q[0 * kBlock] = live ? lse[i].m : -INFINITY;
    q[1 * kBlock] = live ? lse[i].s : 0.;
    q[2 * kBlock] = live ? mom[i].mean : 0.;
    q[3 * kBlock] = live ? mom[i].m2 : 0.;
    s_k[i * kBlock + threadIdx.x] = live ? mom[i].k : 0.;
  }
  __syncthreads();
  const int o = threadIdx.x / kPointwiseFold, t = threadIdx.x % kPointwiseFold;
  double *const q = s_temp + (o * 4) * kBlock, *const qk = s_k + o * kBlock;
  double *const qn = s_fn + o * kPointwiseFold;
  const auto lse_at = [&](int lane) { return LsePair{q[lane], q[kBlock + lane]}; };
  const auto mom_at = [&](const double *n, int lane) {
    return Moments{n[lane], qk[lane], q[2 * kBlock + lane], q[3 * kBlock + lane]};
  };
  LsePair fl = lse_at(t);
  Moments fm = mom_at(s_n, t);
  for (int lane = t + kPointwiseFold; lane < kBlock; lane += kPointwiseFold) {
    fl = lse_merge(fl, lse_at(lane));
    fm = moments_merge(fm, mom_at(s_n, lane));
  }
  // the 32 results of each observation go where its lanes 0..31 stood, then
  // fold by halves
  __syncthreads();
  for (int w = kPointwiseFold; w > 0; w >>= 1) {
    if (t < w) {
      if (w < kPointwiseFold) {
        fl = lse_merge(fl, lse_at(t + w));
        fm = moments_merge(fm, mom_at(qn, t + w));
      }
      q[t] = fl.m;
      q[kBlock + t] = fl.s;
      q[2 * kBlock + t] = fm.mean;
      q[3 * kBlock + t] = fm.m2;
      qk[t] = fm.k;
      qn[t] = fm.n;
    }
    __syncthreads();
  }
  *fl_out = fl;
  *fm_out = fm;
  *o_out = o;
  *t_out = t;
}

}  // namespace
}  // namespace pbh
