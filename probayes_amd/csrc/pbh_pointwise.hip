// pbh_pointwise.hip -- pbh_trace_pointwise on gfx950: per observation j, the
// log-sum-exp, the mean and the variance over the draws of a trace window of
// the term T[s, j] a pointwise program gives (scalar prefix words, LOOP, body,
// SUM as the last word: probayes_amd/expr.py trace_pointwise; evaluate_pointwise
// and diag.pointwise_stats are the host definition).  T [draws][observations]
// is never formed: a draw's terms live in registers for as long as it takes to
// fold them.
//
//   pointwise_kernel   lane = chain.  Workgroup (tile, chain block, slice) owns
//       kPointwiseLanes chains, kPointwiseTile = 8 observations and slice_len
//       records of the window (pbh_trace_host.h pointwise_layout).  Per record
//       every lane loads its draw x[k] = trace[first + r][k][c] (512 contiguous
//       bytes per wave and dim; the next record's loads are issued before this
//       record's arithmetic), runs the scalar prefix with its slots in LDS,
//       then the body once for the tile through the interpreter's expr_body<D,
//       8> (one decode per word, one 64-byte load per column), and folds the 8
//       terms into 40 doubles of running state per lane: the online log-sum-exp
//       pair (m, s) and Welford's (shift, mean, M2) of each observation
//       (pbh_pointwise_merge.h).  The observation index of every accumulator is
//       a compile-time constant: nothing is a runtime-indexed private array.
//       At the end of the slice the lanes' partials go to LDS (the body
//       temporaries' 64 KB, free by then) and 32 threads per observation merge
//       them in the fixed order of pointwise_combine; a lane past N holds the
//       merges' identity.  One partial row per workgroup; no atomics.
//   pointwise_finish_kernel   a thread per observation merges the partial rows
//       in index order and writes lse, mean, var.  Observations of the last
//       tile at or past n_obs (computed on the columns' zero padding) have
//       partials and no result.
//
// The workgroup's place in the grid, the walk over its records and the lanes'
// merge are pbh_pointwise_impl.h's, shared with the tail select
// (pbh_pointwise_tail.hip).
//
// Every order is fixed, so two calls give the same bits.  -ffp-contract=off,
// and the unit goes through the E64 pass, as the expression units do.
#include "pbh_pointwise_impl.h"   // the group, the walk and the lanes' merge

namespace pbh {
namespace {

__global__ __launch_bounds__(kBlock) void pointwise_kernel(KArgs a, PointwiseArgs p) {
  __shared__ double s_slot[kExprSlots * kBlock];
  __shared__ double s_temp[kExprTemps * kW * kBlock];
  const PointwiseGroup g = pointwise_group(p, blockIdx.x);

  LsePair lse[kW];
  Moments mom[kW];
#pragma unroll
  for (int i = 0; i < kW; ++i) {
    lse[i] = lse_identity();
    mom[i] = moments_identity();
  }
  pointwise_walk(a, p, g, s_slot + threadIdx.x, s_temp + threadIdx.x,
                 [&](int64_t at, const double (&t)[kW]) {
    const double inv_n = 1. / (double)(at + 1);
#pragma unroll
    for (int i = 0; i < kW; ++i) {
      lse[i] = lse_push(lse[i], t[i]);
      mom[i] = moments_push(mom[i], t[i], inv_n);
    }
  });

  LsePair fl;
  Moments fm;
  int o, t;
  pointwise_merge_lanes(lse, mom, g.live, s_slot, s_temp, &fl, &fm, &o, &t);
  if (t == 0) {
    const int64_t row = g.block * p.slices + g.slice, plane = p.rows * p.npad;
    double *out = p.part + row * p.npad + g.j0 + o;
    out[0 * plane] = fl.m;
    out[1 * plane] = fl.s;
    out[2 * plane] = fm.n;
    out[3 * plane] = fm.k;
    out[4 * plane] = fm.mean;
    out[5 * plane] = fm.m2;
  }
}

__global__ __launch_bounds__(64) void pointwise_finish_kernel(const double *__restrict__ part,
                                                              int64_t rows, int64_t npad,
                                                              int32_t n_obs,
                                                              double *__restrict__ res) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_obs) return;
  const int64_t plane = rows * npad;
  LsePair l = lse_identity();
  Moments m = moments_identity();
  for (int64_t r = 0; r < rows; ++r) {
    const double *at = part + r * npad + j;
    l = lse_merge(l, LsePair{at[0], at[plane]});
    m = moments_merge(m, Moments{at[2 * plane], at[3 * plane], at[4 * plane], at[5 * plane]});
  }
  res[j] = lse_value(l);
  res[npad + j] = moments_mean(m);
  res[2 * npad + j] = m.m2 / (m.n - 1.);
}

}  // namespace

hipError_t launch_pointwise(const double *tx, int64_t n, int32_t d, int64_t first, int64_t count,
                            const double *prog, const ExprLayout &el, int32_t loop_pc,
                            int32_t n_obs, unsigned char *scratch, const PointwiseLayout &l,
                            hipStream_t s) {
  KArgs a{};
  a.d = d;
  expr_bind(a, prog, el);
  PointwiseArgs p{};
  p.tx = tx;
  p.n = n;
  p.first = first;
  p.count = count;
  p.slice_len = l.slice_len;
  p.slices = l.slices;
  p.rows = l.rows;
  p.npad = l.npad;
  p.d = d;
  p.loop_pc = loop_pc;
  p.body_len = el.n_code - loop_pc - 2;
  p.part = reinterpret_cast<double *>(scratch + l.part);
  hipLaunchKernelGGL(pointwise_kernel,
                     dim3((unsigned)l.tiles, (unsigned)l.chain_blocks, (unsigned)l.slices),
                     dim3(kBlock), 0, s, a, p);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(pointwise_finish_kernel, dim3((unsigned)((n_obs + 63) / 64)), dim3(64), 0, s,
                     p.part, l.rows, l.npad, n_obs, reinterpret_cast<double *>(scratch + l.res));
  return hipGetLastError();
}

}  // namespace pbh
