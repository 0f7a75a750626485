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
// Every order is fixed, so two calls give the same bits.  -ffp-contract=off,
// and the unit goes through the E64 pass, as the expression units do.
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

__global__ __launch_bounds__(kBlock) void pointwise_kernel(KArgs a, PointwiseArgs p) {
  __shared__ double s_slot[kExprSlots * kBlock];
  __shared__ double s_temp[kExprTemps * kW * kBlock];
  double *const sl = s_slot + threadIdx.x;
  double *const tl = s_temp + threadIdx.x;
  const int tile = blockIdx.x;
  const int64_t block = blockIdx.y, slice = blockIdx.z;
  const int64_t c = block * kBlock + threadIdx.x;
  const bool live = c < p.n;
  const int64_t cc = live ? c : p.n - 1;
  const int64_t r0 = slice * p.slice_len;
  const int64_t r1 = r0 + p.slice_len < p.count ? r0 + p.slice_len : p.count;
  const int j0 = tile * kW;

  LsePair lse[kW];
  Moments mom[kW];
#pragma unroll
  for (int i = 0; i < kW; ++i) {
    lse[i] = lse_identity();
    mom[i] = moments_identity();
  }
  double x[D], xn[D];
  load_draw(p, r0, cc, x);
  for (int64_t r = r0; r < r1; ++r) {
    load_draw(p, r + 1 < r1 ? r + 1 : r, cc, xn);
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
    expr_body<D, kW>(a, x, sl, tl, p.loop_pc + 1, p.body_len, j0, t);
    const double inv_n = 1. / (double)(r - r0 + 1);
#pragma unroll
    for (int i = 0; i < kW; ++i) {
      lse[i] = lse_push(lse[i], t[i]);
      mom[i] = moments_push(mom[i], t[i], inv_n);
    }
#pragma unroll
    for (int k = 0; k < D; ++k) x[k] = xn[k];
  }

  // the lanes' partials over the temporaries, [observation][m, s, mean, M2]
  // [lane], and over the slots: the counts [lane], the 32 folded counts of each
  // observation, then the shifts [observation][lane]
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
  if (t == 0) {
    const int64_t row = block * p.slices + slice, plane = p.rows * p.npad;
    double *out = p.part + row * p.npad + j0 + o;
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
