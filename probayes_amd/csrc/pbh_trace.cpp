// pbh_trace.cpp -- the trace entry points of include/pbhip.h: the recorded
// trace copied out, and the reductions over it that run on the device.  No
// kernel lives here: the launches are pbh_kernels.h's, the host arithmetic
// pbh_trace_host.h's.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <initializer_list>

#include "pbh_engine_state.h"
#include "pbh_expr_host.h"
#include "pbh_trace_host.h"

using pbh::check_ptr;
using pbh::fail;

namespace {

struct NamedPtr {
  const void *p;
  const char *name;
};

// what a refused window says, of (first, end, rec)
constexpr char kRange[] = "trace range [%lld, %lld) outside [0, %lld)";
constexpr char kRangeEss[] = "ESS needs >= 2 records inside [0, %3$lld), got [%1$lld, %2$lld)";

// The preamble of a trace entry point, in the order the ABI reports things:
// the engine and the caller's pointers `ptrs` are not null, the resident server
// is stopped, with need_trace a trace is allocated, `own` (the entry point's
// argument checks that come before the window's; a status) passes, and records
// [first, first + count) with count >= min_count lie inside the recorded ones.
template <class Own = int (*)()>
int trace_enter(pbh_engine *e, std::initializer_list<NamedPtr> ptrs, bool need_trace,
                int64_t first, int64_t count, int64_t min_count,
                Own own = [] { return PBH_OK; }, const char *range = kRange) {
  if (check_ptr(e, "engine")) return PBH_ERR_ARG;
  for (const NamedPtr &np : ptrs)
    if (check_ptr(np.p, np.name)) return PBH_ERR_ARG;
  SRV_STOP(e);
  if (need_trace && (e->cap <= 0 || !e->tx || !e->tlp))
    return fail(PBH_ERR_ARG, "no trace allocated (pbh_alloc_trace first)");
  if (const int rc = own()) return rc;
  int64_t rec = 0;
  pbh_trace_len(e, &rec);
  if (!pbh::trace_window_ok(rec, first, count, min_count))
    return fail(PBH_ERR_ARG, range, (long long)first,
                (long long)pbh::trace_window_end(first, count), (long long)rec);
  return PBH_OK;
}

// the checks of a quantile list and of its window's least count
int quantile_args(int32_t nq, const double *q, int64_t count) {
  const std::string bad = pbh::quantile_list_error(nq, q);
  if (!bad.empty()) return fail(PBH_ERR_ARG, "%s", bad.c_str());
  if (count < 1) return fail(PBH_ERR_ARG, "count = %lld: at least 1 record", (long long)count);
  return PBH_OK;
}

// the reduction scratch at `bytes` or more
int scratch(pbh_engine *e, size_t bytes) {
  return pbh::dgrow(e->scratch, e->scratch_bytes, bytes);
}

// the pinned staging buffer at n doubles or more
int stage(pbh_engine *e, size_t n) {
  if (e->stage_len >= n) return PBH_OK;
  if (e->stage) (void)hipHostFree(e->stage);
  e->stage = nullptr;
  e->stage_len = 0;
  HIP_TRY(hipHostMalloc(&e->stage, n * sizeof(double), hipHostMallocDefault));
  e->stage_len = n;
  return PBH_OK;
}

// the typed region of the reduction scratch that starts `byte_offset` in
template <class T>
T *at(unsigned char *scratch, int64_t byte_offset) {
  return reinterpret_cast<T *>(scratch + byte_offset);
}

// what an entry point says of a HIP call that failed
int hip_fail(const char *entry, hipError_t err) {
  return fail(PBH_ERR_HIP, "%s: %s", entry, hipGetErrorString(err));
}

// A pooled radix select as far as it is decided before the scratch is sized:
// where the quantiles lie among M values, the nt ranks the device selects, and
// the select's scratch words for d dims (default: no select, no words).
struct PooledSelect {
  pbh::PooledPlan plan;
  int32_t nt = 0;
  int64_t words = 0;
  PooledSelect() = default;
  PooledSelect(int64_t M, int32_t d, int32_t nq, const double *q)
      : plan(pbh::pooled_plan(M, nq, q)), nt((int32_t)plan.ranks.size()),
        words(pbh::select_scratch_words(d, nt)) {}
};

// Runs the select over records [first, first + count) on the engine's stream in
// the scratch words at `sel` and leaves the interpolated quantiles [nq][d] in
// the host memory `out` (and, not null, order_stats [nq][2][d]).  The lifetime
// rule of launch_select_init is kept here and nowhere else: `init` is the
// source of a queued copy, so the stream is synchronised on every path, a
// failed launch included, before it goes out of scope.
hipError_t run_select(pbh_engine *e, const PooledSelect &ps, int64_t first, int64_t count,
                      uint64_t *sel, double *out, double *order_stats) {
  const int32_t d = e->d;
  std::vector<uint64_t> init((size_t)(4 * d * pbh::kSelectMaxTargets + d));
  hipError_t err = pbh::launch_select_init(sel, d, ps.nt, ps.plan.ranks.data(), init.data(),
                                           e->stream);
  for (int32_t pass = 0; err == hipSuccess && pass < pbh::select_passes(); ++pass)
    err = pbh::launch_select_pass(e->tx, e->n, d, first, count, sel, ps.nt, pass, e->stream);
  const hipError_t drained = hipStreamSynchronize(e->stream);
  if (err == hipSuccess) err = drained;
  std::vector<double> order((size_t)d * ps.nt);   // [d][nt]
  if (err == hipSuccess)
    err = hipMemcpy(order.data(), sel + pbh::select_stats_offset(d, ps.nt),
                    order.size() * sizeof(double), hipMemcpyDeviceToHost);
  if (err == hipSuccess) pbh::pooled_interpolate(ps.plan, d, order.data(), out, order_stats);
  return err;
}

// The scores of dim k on the stream: its pooled ranks over the window turned to
// normal scores z [count][n] in the layout's z (folded about med[k] where med
// is not null; the rank rows in the layout's r with want_ranks), then, with
// `rows`, launch_rhat_chain on z as a one-dim trace into the layout's stats.
hipError_t launch_scores(pbh_engine *e, const pbh::RankLayout &l, int64_t k, int64_t first,
                         int64_t count, const double *med, bool want_ranks, bool rows) {
  hipError_t err = pbh::launch_rank_dim(e->tx, e->n, (int32_t)e->d, (int32_t)k, first, count, med,
                                        e->scratch, l, want_ranks, e->stream);
  if (err == hipSuccess && rows)
    err = pbh::launch_rhat_chain(at<const double>(e->scratch, l.z), e->n, 1, 0, count,
                                 at<double>(e->scratch, l.stats), e->stream);
  return err;
}

// The checks of a pointwise program that come before the window's, for `entry`:
// a trace, the engine's dims, expr_check and the pointwise shape.  Fills prog
// and loop_pc.
int pointwise_program(pbh_engine *e, const char *entry, const int32_t *code, int32_t n_code,
                      const double *consts, int32_t n_consts, int32_t depth, const double *data,
                      int32_t n_cols, int32_t n_obs, pbh::ExprProgram *out, int *loop_pc) {
  pbh::ExprProgram &prog = *out;
  if (e->cap <= 0 || !e->tx)
    return fail(PBH_ERR_STATE, "no trace allocated (pbh_alloc_trace first)");
  if (e->d > PBH_EXPR_MAX_DIM)
    return fail(PBH_ERR_ARG, "%s: the engine has %d dims, a program reads "
                "at most %d variables", entry, (int)e->d, PBH_EXPR_MAX_DIM);
  prog.d = (int32_t)e->d;
  prog.code = code;
  prog.n_code = n_code;
  prog.consts = consts;
  prog.n_consts = n_consts;
  prog.depth = depth;
  prog.data = data;
  prog.n_cols = n_cols;
  prog.n_obs = n_obs;
  int pc = -1;
  if (const char *bad = pbh::expr_check(prog, &pc))
    return fail(PBH_ERR_ARG, "%s: bad program at word %d: %s", entry, pc, bad);
  if (const char *bad = pbh::expr_pointwise_error(prog, loop_pc))
    return fail(PBH_ERR_ARG, "%s: %s", entry, bad);
  return PBH_OK;
}

}  // namespace

extern "C" {

int pbh_trace_len(pbh_engine *e, int64_t *n_recorded) {
  if (check_ptr(e, "engine") || check_ptr(n_recorded, "n_recorded")) return PBH_ERR_ARG;
  const int64_t r = e->cap > 0 ? e->g / e->thin - e->rec_base : 0;
  *n_recorded = std::max<int64_t>(0, std::min(r, e->cap));
  return PBH_OK;
}

int pbh_get_trace(pbh_engine *e, int64_t first, int64_t cnt, double *x,
                  double *logp, uint64_t *acc, double *p_x, double *p_p,
                  double *s) {
  if (const int rc = trace_enter(e, {}, false, first, cnt, 0)) return rc;
  if ((p_x || p_p || s) && !e->debug)
    return fail(PBH_ERR_STATE, "debug trace not allocated");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const size_t n = e->n, d = e->d, W = (e->n + 63) / 64;
  if (cnt == 0) return PBH_OK;
  if (x) HIP_TRY(hipMemcpy(x, e->tx + first * d * n, cnt * d * n * sizeof(double), hipMemcpyDeviceToHost));
  if (logp) HIP_TRY(hipMemcpy(logp, e->tlp + first * n, cnt * n * sizeof(double), hipMemcpyDeviceToHost));
  if (acc) HIP_TRY(hipMemcpy(acc, e->tacc + first * W, cnt * W * sizeof(uint64_t), hipMemcpyDeviceToHost));
  if (p_x) HIP_TRY(hipMemcpy(p_x, e->tpx + first * d * n, cnt * d * n * sizeof(double), hipMemcpyDeviceToHost));
  if (p_p) HIP_TRY(hipMemcpy(p_p, e->tpp + first * n, cnt * n * sizeof(double), hipMemcpyDeviceToHost));
  if (s) HIP_TRY(hipMemcpy(s, e->ts + first * n, cnt * n * sizeof(double), hipMemcpyDeviceToHost));
  return PBH_OK;
}

int pbh_trace_stats(pbh_engine *e, int64_t first, int64_t count, double *sum,
                    double *sumsq, int64_t *n_acc) {
  if (const int rc = trace_enter(e, {}, false, first, count, 0)) return rc;
  HIP_TRY(hipSetDevice(e->device));
  const int64_t n = e->n, W = (n + 63) / 64;
  HIP_TRY(pbh::launch_trace_stats(e->tx, e->tacc, n, e->d, W, first, count,
                                  e->msum, e->msq, e->nacc, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->mom_steps = count;
  const size_t dn = (size_t)e->d * n;
  if (sum) HIP_TRY(hipMemcpy(sum, e->msum, dn * sizeof(double), hipMemcpyDeviceToHost));
  if (sumsq) HIP_TRY(hipMemcpy(sumsq, e->msq, dn * sizeof(double), hipMemcpyDeviceToHost));
  if (n_acc) HIP_TRY(hipMemcpy(n_acc, e->nacc, n * sizeof(int64_t), hipMemcpyDeviceToHost));
  return PBH_OK;
}

int pbh_trace_expectation(pbh_engine *e, int64_t first, int64_t count,
                          double exponent, double *out) {
  if (const int rc = trace_enter(e, {{out, "out"}}, false, first, count, 1)) return rc;
  if (!std::isfinite(exponent)) return fail(PBH_ERR_ARG, "exponent must be finite");
  HIP_TRY(hipSetDevice(e->device));
  const size_t dn = (size_t)e->d * e->n;
  if (const int rc = scratch(e, dn * sizeof(double))) return rc;
  double *dout = at<double>(e->scratch, 0);
  hipError_t err = pbh::launch_trace_expectation(
      e->tx, e->tlp, e->n, e->d, first, count, exponent,
      e->k.pscale == PBH_PSCALE_LIN ? 1 : 0, e->k.log_npi, dout, e->stream);
  if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
  if (err == hipSuccess)
    err = hipMemcpy(out, dout, dn * sizeof(double), hipMemcpyDeviceToHost);
  if (err != hipSuccess) return hip_fail("pbh_trace_expectation", err);
  return PBH_OK;
}

int pbh_trace_quantile(pbh_engine *e, int64_t first, int64_t count, int32_t nq,
                       const double *q, int32_t weighted, double *out) {
  const auto own = [&] {
    if (const int rc = quantile_args(nq, q, count)) return rc;
    if (count > PBH_QUANTILE_MAX_RECORDS)
      return fail(PBH_ERR_ARG, "count = %lld above the %d records a series is sorted at",
                  (long long)count, PBH_QUANTILE_MAX_RECORDS);
    return PBH_OK;
  };
  if (const int rc = trace_enter(e, {{q, "q"}, {out, "out"}}, true, first, count, 1, own))
    return rc;
  HIP_TRY(hipSetDevice(e->device));
  const size_t res = (size_t)nq * e->d * e->n;
  if (const int rc = scratch(e, (PBH_QUANTILE_MAX_Q + res) * sizeof(double))) return rc;
  double *dbuf = at<double>(e->scratch, 0);   // q [nq], then the result [nq][d][n]
  hipError_t err = hipMemcpyAsync(dbuf, q, nq * sizeof(double), hipMemcpyHostToDevice,
                                  e->stream);
  if (err == hipSuccess)
    err = pbh::launch_trace_quantile(e->tx, e->tlp, e->n, e->d, first, (int32_t)count, nq,
                                     dbuf, weighted ? 1 : 0,
                                     e->k.pscale == PBH_PSCALE_LIN ? 1 : 0, e->k.log_npi,
                                     dbuf + PBH_QUANTILE_MAX_Q, e->stream);
  if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
  if (err == hipSuccess)
    err = hipMemcpy(out, dbuf + PBH_QUANTILE_MAX_Q, res * sizeof(double),
                    hipMemcpyDeviceToHost);
  if (err != hipSuccess) return hip_fail("pbh_trace_quantile", err);
  return PBH_OK;
}

int pbh_trace_rhat(pbh_engine *e, int64_t first, int64_t count, int32_t group,
                   double *split_rhat, double *nested_rhat, double *chain_stats) {
  if (const int rc = trace_enter(e, {}, true, first, count, 0)) return rc;
  if (count < 2)
    return fail(PBH_ERR_ARG, "count = %lld: a variance needs at least 2 records",
                (long long)count);
  if (split_rhat && count < 4)
    return fail(PBH_ERR_ARG, "count = %lld: split R-hat needs at least 4 records "
                "(two in each half)", (long long)count);
  const int64_t n = e->n, d = e->d;
  int64_t K = 0;
  if (nested_rhat) {
    if (group < 1) return fail(PBH_ERR_ARG, "group = %d: at least 1 chain per superchain",
                               (int)group);
    if (n % group != 0)
      return fail(PBH_ERR_ARG, "group = %d does not divide the %lld chains", (int)group,
                  (long long)n);
    K = n / group;
    if (K < 2)
      return fail(PBH_ERR_ARG, "group = %d leaves %lld superchain of %lld chains: nested "
                  "R-hat needs at least 2", (int)group, (long long)K, (long long)n);
  }
  HIP_TRY(hipSetDevice(e->device));
  // stats [6][d][n], the superchains' (mu, B + W) [2][d][K], the results [2][d]
  const int64_t n_stats = 6 * d * n, n_sc = 2 * d * K, need = n_stats + n_sc + 2 * d;
  if (const int rc = scratch(e, (size_t)need * sizeof(double))) return rc;
  double *stats = at<double>(e->scratch, 0), *sc = stats + n_stats, *res = sc + n_sc;
  hipError_t err = pbh::launch_rhat_chain(e->tx, n, (int32_t)d, first, count, stats, e->stream);
  if (err == hipSuccess && (split_rhat || nested_rhat))
    err = pbh::launch_rhat_cross(stats, n, (int32_t)d, count, group, sc,
                                 split_rhat ? res : nullptr, nested_rhat ? res + d : nullptr,
                                 e->stream);
  if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
  double host[2 * PBH_MAX_DIM];
  if (err == hipSuccess && (split_rhat || nested_rhat))
    err = hipMemcpy(host, res, 2 * d * sizeof(double), hipMemcpyDeviceToHost);
  if (err == hipSuccess && chain_stats)
    err = hipMemcpy(chain_stats, stats, n_stats * sizeof(double), hipMemcpyDeviceToHost);
  if (err != hipSuccess) return hip_fail("pbh_trace_rhat", err);
  if (split_rhat) std::memcpy(split_rhat, host, d * sizeof(double));
  if (nested_rhat) std::memcpy(nested_rhat, host + d, d * sizeof(double));
  return PBH_OK;
}

int pbh_trace_cov(pbh_engine *e, int64_t first, int64_t count, double *mean, double *cov,
                  double *corr) {
  if (!mean && !cov && !corr)
    return fail(PBH_ERR_ARG, "pbh_trace_cov: no output asked for (mean, cov and corr are all "
                "NULL)");
  if (const int rc = trace_enter(e, {}, true, first, count, 1)) return rc;
  const int64_t n = e->n, d = e->d;
  if (n < 2 && count < 2)
    return fail(PBH_ERR_ARG, "pbh_trace_cov: %lld chain of %lld record: a covariance needs at "
                "least 2 draws", (long long)n, (long long)count);
  pbh::CovLayout l;
  if (!pbh::cov_layout(n, count, (int32_t)d, &l))
    return fail(PBH_ERR_ARG, "pbh_trace_cov: no scratch layout for %lld chains of %lld records "
                "of %lld dims", (long long)n, (long long)count, (long long)d);
  HIP_TRY(hipSetDevice(e->device));
  if (const int rc = scratch(e, (size_t)l.bytes)) return rc;
  hipError_t err = pbh::launch_cov(e->tx, n, (int32_t)d, first, count, e->scratch, l, e->stream);
  if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
  // the shift and the merged sums (S, then P's packed triangle), then the last
  // step on the host
  double K[PBH_MAX_DIM], sums[PBH_MAX_DIM + PBH_MAX_DIM * (PBH_MAX_DIM + 1) / 2];
  if (err == hipSuccess)
    err = hipMemcpy(K, at<const double>(e->scratch, l.K), (size_t)d * sizeof(double),
                    hipMemcpyDeviceToHost);
  if (err == hipSuccess)
    err = hipMemcpy(sums, at<const double>(e->scratch, l.res), (size_t)l.cols * sizeof(double),
                    hipMemcpyDeviceToHost);
  if (err != hipSuccess) return hip_fail("pbh_trace_cov", err);
  pbh::cov_finish(K, sums, sums + d, n * count, (int32_t)d, mean, cov, corr);
  return PBH_OK;
}

int pbh_trace_hist(pbh_engine *e, int64_t first, int64_t count, const int32_t *n_bins,
                   const double *edges, int64_t *counts, int64_t *outside) {
  if (!counts)
    return fail(PBH_ERR_ARG, "pbh_trace_hist: no output asked for (counts is NULL)");
  const auto own = [&] {
    const std::string bad = pbh::hist_check_edges((int32_t)e->d, n_bins, edges);
    return bad.empty() ? PBH_OK : fail(PBH_ERR_ARG, "pbh_trace_hist: %s", bad.c_str());
  };
  if (const int rc = trace_enter(e, {{n_bins, "n_bins"}, {edges, "edges"}}, true, first, count, 1,
                                 own))
    return rc;
  const int64_t n = e->n;
  const int32_t d = (int32_t)e->d;
  pbh::HistLayout l;
  if (!pbh::hist_layout(n, count, d, n_bins, &l))
    return fail(PBH_ERR_ARG, "pbh_trace_hist: no scratch layout for %lld chains of %lld records",
                (long long)n, (long long)count);
  HIP_TRY(hipSetDevice(e->device));
  if (const int rc = scratch(e, (size_t)l.bytes)) return rc;
  // the tables go up and the counts come back through the pinned stage (the
  // tables, then the counts): queued copies, one wait
  if (const int rc = stage(e, (size_t)(l.n_tab + l.n_ctr))) return rc;
  double *tables = e->stage;
  const uint64_t *host = reinterpret_cast<const uint64_t *>(e->stage + l.n_tab);
  // every dim's lookup, and the listed dims' tables in the layout's order
  pbh::HistDimPlan plan[PBH_MAX_DIM];
  {
    const double *ed = edges;
    double *t = tables;
    for (int32_t k = 0; k < d; ++k) {
      plan[k] = pbh::hist_dim_plan(ed, n_bins[k]);
      if (n_bins[k] == 0) continue;
      pbh::hist_fill_table(ed, plan[k], t);
      t += pbh::hist_table_len(n_bins[k]);
      ed += n_bins[k] + 1;
    }
  }
  hipError_t err = hipMemcpyAsync(at<double>(e->scratch, l.tables), tables,
                                  (size_t)l.n_tab * sizeof(double), hipMemcpyHostToDevice,
                                  e->stream);
  if (err == hipSuccess)
    err = pbh::launch_hist(e->tx, n, d, first, count, e->scratch, l, plan, e->stream);
  if (err == hipSuccess)
    err = hipMemcpyAsync(e->stage + l.n_tab, at<const uint64_t>(e->scratch, l.counts),
                         (size_t)l.n_ctr * 8, hipMemcpyDeviceToHost, e->stream);
  // (the stage is the source and the target of queued copies: waited for on
  // every path)
  const hipError_t drained = pbh::stream_wait(e);
  if (err == hipSuccess) err = drained;
  if (err != hipSuccess) return hip_fail("pbh_trace_hist", err);
  // per listed dim: the bins, then below, above, NaN
  if (outside) std::fill(outside, outside + 3 * (size_t)d, (int64_t)0);
  const uint64_t *h = host;
  for (int32_t k = 0; k < d; ++k) {
    const int32_t B = n_bins[k];
    if (B == 0) continue;
    for (int32_t i = 0; i < B; ++i) *counts++ = (int64_t)h[i];
    if (outside)
      for (int i = 0; i < 3; ++i) outside[3 * k + i] = (int64_t)h[B + i];
    h += B + 3;
  }
  return PBH_OK;
}

int pbh_trace_hist2d(pbh_engine *e, int64_t first, int64_t count, const int32_t *n_bins,
                     const double *edges, int32_t n_pairs, const int32_t *pairs,
                     int64_t *counts) {
  if (!counts)
    return fail(PBH_ERR_ARG, "pbh_trace_hist2d: no output asked for (counts is NULL)");
  const auto own = [&] {
    std::string bad = pbh::hist_check_edges((int32_t)e->d, n_bins, edges);
    if (bad.empty()) bad = pbh::hist2d_check_pairs((int32_t)e->d, n_bins, n_pairs, pairs);
    return bad.empty() ? PBH_OK : fail(PBH_ERR_ARG, "pbh_trace_hist2d: %s", bad.c_str());
  };
  if (const int rc = trace_enter(e, {{n_bins, "n_bins"}, {edges, "edges"}, {pairs, "pairs"}}, true,
                                 first, count, 1, own))
    return rc;
  const int64_t n = e->n;
  const int32_t d = (int32_t)e->d;
  pbh::Hist2dLayout l;
  if (!pbh::hist2d_layout(n, count, d, n_bins, n_pairs, pairs, &l))
    return fail(PBH_ERR_ARG, "pbh_trace_hist2d: no scratch layout for %lld chains of %lld "
                "records", (long long)n, (long long)count);
  HIP_TRY(hipSetDevice(e->device));
  if (const int rc = scratch(e, (size_t)l.bytes)) return rc;
  // the tables and the pairs' records go up through the pinned stage, and the
  // counts come back through it while they are few (kStagedCounts: 16 MB): queued
  // copies, one wait.  More counts are copied to the caller after the wait.
  constexpr int64_t kStagedCounts = (int64_t)1 << 21;
  const bool staged = l.n_ctr <= kStagedCounts;
  const int64_t up = l.n_tab + 4 * (int64_t)n_pairs;
  if (const int rc = stage(e, (size_t)(up + (staged ? l.n_ctr : 0)))) return rc;
  double *tables = e->stage;
  int64_t *recs = reinterpret_cast<int64_t *>(e->stage + l.n_tab);
  pbh::HistDimPlan plan[PBH_MAX_DIM];
  {
    const double *ed = edges;
    for (int32_t k = 0; k < d; ++k) {
      plan[k] = pbh::hist_dim_plan(ed, n_bins[k]);
      if (n_bins[k] == 0) continue;
      pbh::hist_fill_table(ed, plan[k], tables + l.tab_off[k]);
      ed += n_bins[k] + 1;
    }
  }
  for (int32_t p = 0; p < n_pairs; ++p) {
    recs[(size_t)p * 4] = pairs[2 * p];
    recs[(size_t)p * 4 + 1] = pairs[2 * p + 1];
    recs[(size_t)p * 4 + 2] = l.out[(size_t)p];
    recs[(size_t)p * 4 + 3] = 0;
  }
  hipError_t err = hipMemcpyAsync(at<double>(e->scratch, l.tables), tables,
                                  (size_t)l.n_tab * sizeof(double), hipMemcpyHostToDevice,
                                  e->stream);
  if (err == hipSuccess)
    err = hipMemcpyAsync(at<int64_t>(e->scratch, l.pairs), recs, (size_t)n_pairs * 4 * 8,
                         hipMemcpyHostToDevice, e->stream);
  if (err == hipSuccess)
    err = pbh::launch_hist2d(e->tx, n, d, first, count, e->scratch, l, plan, e->stream);
  if (err == hipSuccess && staged)
    err = hipMemcpyAsync(e->stage + up, at<const uint64_t>(e->scratch, l.counts),
                         (size_t)l.n_ctr * 8, hipMemcpyDeviceToHost, e->stream);
  // (the stage is the source and the target of queued copies: waited for on
  // every path)
  const hipError_t drained = pbh::stream_wait(e);
  if (err == hipSuccess) err = drained;
  // the pairs' cells lie one after the other, as the caller's do; a count is
  // below 2^63, so its uint64 is the caller's int64
  if (err == hipSuccess && staged)
    std::memcpy(counts, e->stage + up, (size_t)l.n_ctr * 8);
  else if (err == hipSuccess)
    err = hipMemcpy(counts, at<const uint64_t>(e->scratch, l.counts), (size_t)l.n_ctr * 8,
                    hipMemcpyDeviceToHost);
  if (err != hipSuccess) return hip_fail("pbh_trace_hist2d", err);
  return PBH_OK;
}

int pbh_trace_quantile_pooled(pbh_engine *e, int64_t first, int64_t count, int32_t nq,
                              const double *q, double *out, double *order_stats) {
  if (const int rc = trace_enter(e, {{q, "q"}, {out, "out"}}, true, first, count, 1,
                                 [&] { return quantile_args(nq, q, count); }))
    return rc;
  const PooledSelect ps(e->n * count, (int32_t)e->d, nq, q);
  HIP_TRY(hipSetDevice(e->device));
  if (const int rc = scratch(e, (size_t)ps.words * sizeof(uint64_t))) return rc;
  const hipError_t err = run_select(e, ps, first, count, at<uint64_t>(e->scratch, 0), out,
                                    order_stats);
  if (err != hipSuccess) return hip_fail("pbh_trace_quantile_pooled", err);
  return PBH_OK;
}

int pbh_trace_rhat_rank(pbh_engine *e, int64_t first, int64_t count, double *bulk,
                        double *folded, double *ranks, double *folded_ranks) {
  if (!bulk && !folded && !ranks && !folded_ranks)
    return fail(PBH_ERR_ARG, "pbh_trace_rhat_rank: no output asked for (bulk, folded, ranks "
                "and folded_ranks are all NULL)");
  if (const int rc = trace_enter(e, {}, true, first, count, 0)) return rc;
  if (count < 4)
    return fail(PBH_ERR_ARG, "count = %lld: split R-hat needs at least 4 records "
                "(two in each half)", (long long)count);
  const int64_t n = e->n, d = e->d;
  const bool want[2] = {bulk || ranks, folded || folded_ranks};
  const bool want_ranks = ranks || folded_ranks;
  // the folded variant's fold point: the pooled median, selected for all dims
  const double half = 0.5;
  const PooledSelect ps = want[1] ? PooledSelect(n * count, (int32_t)d, 1, &half) : PooledSelect();
  pbh::RankLayout l;
  if (!pbh::rank_layout(n, count, (int32_t)d, ps.words, want_ranks, &l))
    return fail(PBH_ERR_UNSUPPORTED, "%lld chains of %lld records: the pooled sort indexes "
                "fewer than 2^32 elements per dim", (long long)n, (long long)count);
  HIP_TRY(hipSetDevice(e->device));
  if (const int rc = scratch(e, (size_t)l.bytes)) return rc;
  if (const int rc = want[1] ? stage(e, (size_t)d) : PBH_OK) return rc;
  unsigned char *sc = e->scratch;
  double *med = at<double>(sc, l.med), *res = at<double>(sc, l.res);
  hipError_t err = hipSuccess;
  if (want[1]) {
    // the median [d] through the pinned stage, which outlives the queued copy
    err = run_select(e, ps, first, count, at<uint64_t>(sc, l.select), e->stage, nullptr);
    if (err == hipSuccess)
      err = hipMemcpyAsync(med, e->stage, d * sizeof(double), hipMemcpyHostToDevice, e->stream);
  }
  for (int v = 0; v < 2; ++v) {
    if (!want[v]) continue;
    double *out_ranks = v ? folded_ranks : ranks;
    const bool reduce = v ? folded != nullptr : bulk != nullptr;
    for (int64_t k = 0; err == hipSuccess && k < d; ++k) {
      err = launch_scores(e, l, k, first, count, v ? med : nullptr, out_ranks != nullptr, reduce);
      if (err == hipSuccess && reduce)
        err = pbh::launch_rhat_cross(at<double>(sc, l.stats), n, 1, count, 0, nullptr,
                                     res + v * d + k, nullptr, e->stream);
      if (err == hipSuccess && out_ranks) {
        // the dim's [count][n] into the host's [count][d][n]
        err = hipStreamSynchronize(e->stream);
        if (err == hipSuccess)
          err = hipMemcpy2D(out_ranks + k * n, (size_t)(d * n) * sizeof(double),
                            at<const double>(sc, l.r), (size_t)n * sizeof(double),
                            (size_t)n * sizeof(double), (size_t)count, hipMemcpyDeviceToHost);
      }
    }
  }
  if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
  double host[2 * PBH_MAX_DIM];
  if (err == hipSuccess && (bulk || folded))
    err = hipMemcpy(host, res, 2 * d * sizeof(double), hipMemcpyDeviceToHost);
  if (err != hipSuccess) return hip_fail("pbh_trace_rhat_rank", err);
  if (bulk) std::memcpy(bulk, host, d * sizeof(double));
  if (folded) std::memcpy(folded, host + d, d * sizeof(double));
  return PBH_OK;
}

int pbh_trace_ess_rank(pbh_engine *e, int64_t first, int64_t count, double *bulk, double *tail,
                       double *tail_parts, double *basic, double *mean_acov) {
  if (!bulk && !tail && !tail_parts && !basic && !mean_acov)
    return fail(PBH_ERR_ARG, "pbh_trace_ess_rank: no output asked for (bulk, tail, tail_parts, "
                "basic and mean_acov are all NULL)");
  if (const int rc = trace_enter(e, {}, true, first, count, 0)) return rc;
  if (count < 4)
    return fail(PBH_ERR_ARG, "count = %lld: the split chains need at least 4 records "
                "(two in each half)", (long long)count);
  if (count / 2 > PBH_ESS_RANK_MAX_HALF)
    return fail(PBH_ERR_UNSUPPORTED, "count = %lld: at most %d records in each half of the "
                "window (a 4 096-point transform)", (long long)count, PBH_ESS_RANK_MAX_HALF);
  const int64_t n = e->n, d = e->d, h = count / 2, C = 2 * n;
  // the variants: bulk, tail_lower, tail_upper, basic
  const bool all = !bulk && !tail && !tail_parts && !basic;
  const bool want_tail = all || tail || tail_parts;
  const bool want[4] = {all || bulk, want_tail, want_tail, all || basic};
  pbh::RankLayout rl{};
  if (want[0] && !pbh::rank_layout(n, count, (int32_t)d, 0, false, &rl))
    return fail(PBH_ERR_UNSUPPORTED, "%lld chains of %lld records: the pooled sort indexes "
                "fewer than 2^32 elements per dim", (long long)n, (long long)count);
  // the tail's thresholds: the pooled 5 % and 95 % quantiles, selected for all dims
  const double q_tail[2] = {0.05, 0.95};
  const PooledSelect ps = want_tail ? PooledSelect(n * count, (int32_t)d, 2, q_tail) : PooledSelect();
  pbh::EssLayout l;
  if (!pbh::ess_layout(n, count, (int32_t)d, want[0] ? rl.bytes : 0, ps.words, &l))
    return fail(PBH_ERR_ARG, "pbh_trace_ess_rank: no scratch layout for %lld chains of %lld "
                "records", (long long)n, (long long)count);
  HIP_TRY(hipSetDevice(e->device));
  if (const int rc = scratch(e, (size_t)l.bytes)) return rc;
  if (const int rc = want_tail ? stage(e, (size_t)(2 * d)) : PBH_OK) return rc;
  unsigned char *sc = e->scratch;
  double *thr = at<double>(sc, l.thr), *part = at<double>(sc, l.part);
  double *acov = at<double>(sc, l.acov);     // [4][d][h]
  double *means = at<double>(sc, l.means);   // [4][2][d][n]
  double *stats = at<double>(sc, l.stats);   // [6][d][n]
  const size_t row = (size_t)n * sizeof(double);
  const auto mean_at = [&](int v, int half, int64_t k) { return means + ((v * 2 + half) * d + k) * n; };
  hipError_t err = hipSuccess;
  if (want_tail) {
    // the thresholds [2][d] through the pinned stage, which outlives the queued copy
    err = run_select(e, ps, first, count, at<uint64_t>(sc, l.select), e->stage, nullptr);
    if (err == hipSuccess)
      err = hipMemcpyAsync(thr, e->stage, 2 * d * sizeof(double), hipMemcpyHostToDevice,
                           e->stream);
  }
  if (want[0]) {
    // per dim: the scores z [count][n] as a one-dim trace, their half means
    // from rhat_chain's rows
    const double *z = at<const double>(sc, rl.z);
    const double *zstats = at<const double>(sc, rl.stats);   // [6][n]
    for (int64_t k = 0; err == hipSuccess && k < d; ++k) {
      err = launch_scores(e, rl, k, first, count, nullptr, false, true);
      if (err == hipSuccess)
        err = pbh::launch_ess_spectrum(z, n, n, count, nullptr, l, part, nullptr, nullptr,
                                       e->stream);
      if (err == hipSuccess) err = pbh::launch_ess_finish(part, n, l, acov + k * h, e->stream);
      for (int half = 0; err == hipSuccess && half < 2; ++half)
        err = hipMemcpyAsync(mean_at(0, half, k), zstats + 2 * half * n, row,
                             hipMemcpyDeviceToDevice, e->stream);
    }
  }
  if (err == hipSuccess && want[3]) {
    err = pbh::launch_rhat_chain(e->tx, n, (int32_t)d, first, count, stats, e->stream);
    for (int half = 0; err == hipSuccess && half < 2; ++half)
      err = hipMemcpyAsync(mean_at(3, half, 0), stats + 2 * half * d * n, (size_t)d * row,
                           hipMemcpyDeviceToDevice, e->stream);
  }
  for (int v = 1; v < 4; ++v) {
    if (!want[v]) continue;
    const bool ind = v < 3;
    for (int64_t k = 0; err == hipSuccess && k < d; ++k) {
      err = pbh::launch_ess_spectrum(e->tx + (first * d + k) * n, n, d * n, count,
                                     ind ? thr + (v - 1) * d + k : nullptr, l, part,
                                     ind ? mean_at(v, 0, k) : nullptr,
                                     ind ? mean_at(v, 1, k) : nullptr, e->stream);
      if (err == hipSuccess)
        err = pbh::launch_ess_finish(part, n, l, acov + (v * d + k) * h, e->stream);
    }
  }
  if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
  // the host stage: A and the means of the variants computed, then the estimator
  std::vector<double> hA((size_t)(d * h)), hm((size_t)(2 * d * n)), m((size_t)C);
  double ess[4][PBH_MAX_DIM];
  for (int v = 0; err == hipSuccess && v < 4; ++v) {
    if (!want[v]) continue;
    err = hipMemcpy(hA.data(), acov + v * d * h, hA.size() * sizeof(double),
                    hipMemcpyDeviceToHost);
    if (err == hipSuccess)
      err = hipMemcpy(hm.data(), mean_at(v, 0, 0), hm.size() * sizeof(double),
                      hipMemcpyDeviceToHost);
    if (err != hipSuccess) break;
    for (int64_t k = 0; k < d; ++k) {
      std::memcpy(m.data(), hm.data() + k * n, row);
      std::memcpy(m.data() + n, hm.data() + (d + k) * n, row);
      ess[v][k] = pbh::multi_chain_ess(m.data(), hA.data() + k * h, C, h);
    }
    if (mean_acov) std::memcpy(mean_acov + v * d * h, hA.data(), hA.size() * sizeof(double));
  }
  if (err != hipSuccess) return hip_fail("pbh_trace_ess_rank", err);
  if (bulk) std::memcpy(bulk, ess[0], d * sizeof(double));
  if (basic) std::memcpy(basic, ess[3], d * sizeof(double));
  if (tail_parts) {
    std::memcpy(tail_parts, ess[1], d * sizeof(double));
    std::memcpy(tail_parts + d, ess[2], d * sizeof(double));
  }
  if (tail)
    for (int64_t k = 0; k < d; ++k) {
      // np.minimum: a NaN propagates
      const double a = ess[1][k], b = ess[2][k];
      tail[k] = a != a ? a : b != b ? b : b < a ? b : a;
    }
  return PBH_OK;
}

int pbh_trace_pointwise(pbh_engine *e, int64_t first, int64_t count, const int32_t *code,
                        int32_t n_code, const double *consts, int32_t n_consts, int32_t depth,
                        const double *data, int32_t n_cols, int32_t n_obs, double *lse,
                        double *mean, double *var) {
  pbh::ExprProgram prog;
  int loop_pc = -1;
  const auto own = [&] {
    return pointwise_program(e, "pbh_trace_pointwise", code, n_code, consts, n_consts, depth, data,
                             n_cols, n_obs, &prog, &loop_pc);
  };
  if (const int rc = trace_enter(e, {{code, "code"}}, false, first, count, 1, own)) return rc;
  const int64_t n = e->n;
  if (n < 2 && count < 2)
    return fail(PBH_ERR_ARG, "pbh_trace_pointwise: %lld chain of %lld record: a variance needs "
                "at least 2 draws", (long long)n, (long long)count);
  std::vector<double> blk;
  const pbh::ExprLayout el = pbh::expr_pack(blk, prog);
  pbh::PointwiseLayout l;
  if (!pbh::pointwise_layout(n, count, n_obs, 0, (int64_t)blk.size(), &l))
    return fail(PBH_ERR_ARG, "pbh_trace_pointwise: no scratch layout for %lld chains of %lld "
                "records", (long long)n, (long long)count);
  HIP_TRY(hipSetDevice(e->device));
  if (const int rc = scratch(e, (size_t)l.bytes)) return rc;
  // the program in a block of its own in the reduction scratch: the model's
  // ecode / econst / edata are not touched
  double *dprog = at<double>(e->scratch, l.prog);
  hipError_t err = hipMemcpyAsync(dprog, blk.data(), blk.size() * sizeof(double),
                                  hipMemcpyHostToDevice, e->stream);
  if (err == hipSuccess)
    err = pbh::launch_pointwise(e->tx, n, (int32_t)e->d, first, count, dprog, el, loop_pc, n_obs,
                                e->scratch, l, e->stream);
  // (blk is the source of a queued copy: synchronised on every path)
  const hipError_t drained = hipStreamSynchronize(e->stream);
  if (err == hipSuccess) err = drained;
  const double *res = at<const double>(e->scratch, l.res);
  double *const outs[3] = {lse, mean, var};
  for (int v = 0; err == hipSuccess && v < 3; ++v)
    if (outs[v])
      err = hipMemcpy(outs[v], res + v * l.npad, (size_t)n_obs * sizeof(double),
                      hipMemcpyDeviceToHost);
  if (err != hipSuccess) return hip_fail("pbh_trace_pointwise", err);
  return PBH_OK;
}

// The scratch is pointwise_layout's with tail_layout's words as the select
// region.  The observations are taken in batches of tail_batch_tiles(capacity)
// tiles, so that the candidate lists hold at most kTailListBytes (256 MiB)
// whatever n_obs is, and the histograms at most 8 KB per observation of a
// batch; a capacity above kTailMaxCapacity, whose one tile would not fit, is
// refused.
int pbh_trace_pointwise_tail(pbh_engine *e, int64_t first, int64_t count, const int32_t *code,
                             int32_t n_code, const double *consts, int32_t n_consts,
                             int32_t depth, const double *data, int32_t n_cols, int32_t n_obs,
                             int64_t k, int64_t capacity, double *tail, double *rest_lse,
                             int32_t *passes) {
  constexpr char kEntry[] = "pbh_trace_pointwise_tail";
  pbh::ExprProgram prog;
  int loop_pc = -1;
  const auto own = [&] {
    if (!tail && !rest_lse)
      return fail(PBH_ERR_ARG, "%s: tail and rest_lse are both NULL", kEntry);
    return pointwise_program(e, kEntry, code, n_code, consts, n_consts, depth, data, n_cols, n_obs,
                             &prog, &loop_pc);
  };
  if (const int rc = trace_enter(e, {{code, "code"}}, false, first, count, 1, own)) return rc;
  const int64_t n = e->n, S = n * count;   // (the window lies in the trace: no overflow)
  if (k < 1 || k >= S)
    return fail(PBH_ERR_ARG, "%s: k = %lld outside 1 .. %lld, the draws less one", kEntry,
                (long long)k, (long long)(S - 1));
  if (capacity != 0 && capacity < k)
    return fail(PBH_ERR_ARG, "%s: capacity = %lld below k = %lld", kEntry, (long long)capacity,
                (long long)k);
  if (capacity == 0) capacity = pbh::tail_default_capacity(k);
  capacity = std::min(capacity, S);   // (no list holds more than every draw)
  if (capacity > pbh::kTailMaxCapacity)
    return fail(PBH_ERR_ARG, "%s: capacity = %lld above %lld, what one tile's lists may hold",
                kEntry, (long long)capacity, (long long)pbh::kTailMaxCapacity);
  std::vector<double> blk;
  const pbh::ExprLayout el = pbh::expr_pack(blk, prog);
  const int64_t tiles = ((int64_t)n_obs + pbh::kPointwiseTile - 1) / pbh::kPointwiseTile;
  const int64_t batch = std::min(pbh::tail_batch_tiles(capacity), tiles);
  const pbh::TailLayout tl = pbh::tail_layout(batch, capacity);
  std::vector<pbh::PointwiseLayout> layouts;
  size_t bytes = 0;
  for (int64_t tile0 = 0; tile0 < tiles; tile0 += batch) {
    const int64_t nb = std::min((int64_t)n_obs - tile0 * pbh::kPointwiseTile,
                                batch * pbh::kPointwiseTile);
    pbh::PointwiseLayout l;
    if (!pbh::pointwise_layout(n, count, (int32_t)nb, tl.words, (int64_t)blk.size(), &l))
      return fail(PBH_ERR_ARG, "%s: no scratch layout for %lld chains of %lld records", kEntry,
                  (long long)n, (long long)count);
    layouts.push_back(l);
    bytes = std::max(bytes, (size_t)l.bytes);
  }
  HIP_TRY(hipSetDevice(e->device));
  if (const int rc = scratch(e, bytes)) return rc;
  // (every batch has the same select and program regions)
  double *dprog = at<double>(e->scratch, layouts[0].prog);
  uint64_t *sel = at<uint64_t>(e->scratch, layouts[0].select);
  // (blk and pfx are the sources of queued copies: the stream is synchronised
  // after every launch and on the way out)
  hipError_t err = hipMemcpyAsync(dprog, blk.data(), blk.size() * sizeof(double),
                                  hipMemcpyHostToDevice, e->stream);
  int32_t most = 0;
  std::vector<uint64_t> pfx((size_t)tl.npad), hist, cursor, keys;
  std::vector<double> part;
  std::vector<pbh::LsePair> rows;
  const char *broken = nullptr;
  for (size_t b = 0; err == hipSuccess && !broken && b < layouts.size(); ++b) {
    const pbh::PointwiseLayout &l = layouts[b];
    const int64_t tile0 = (int64_t)b * batch, j0 = tile0 * pbh::kPointwiseTile;
    const int64_t nb = std::min((int64_t)n_obs - j0, l.npad);
    pbh::TailLaunch t{e->tx, n, first, count, (int32_t)e->d, loop_pc, n_obs, (int32_t)tile0,
                      dprog, &el, e->scratch, &l, &tl, capacity};
    std::vector<pbh::TailState> st((size_t)nb, pbh::TailState{0, (uint64_t)(k - 1), 0,
                                                              (uint64_t)S});
    std::fill(pfx.begin(), pfx.end(), 0);
    const auto settled = [&] {
      for (const pbh::TailState &s : st)
        if (!pbh::tail_settled(s, capacity)) return false;
      return true;
    };
    const auto put_prefixes = [&] {
      for (int64_t j = 0; j < nb; ++j) pfx[(size_t)j] = st[(size_t)j].prefix;
      return hipMemcpyAsync(sel + tl.prefix, pfx.data(), pfx.size() * 8, hipMemcpyHostToDevice,
                            e->stream);
    };
    int32_t done = 0, ran = 0;
    hist.resize((size_t)(nb * pbh::kTailBins));
    while (err == hipSuccess && done < 64 && !settled()) {
      err = put_prefixes();
      if (err == hipSuccess) err = pbh::launch_tail_count(t, done, e->stream);
      const hipError_t drained = hipStreamSynchronize(e->stream);
      if (err == hipSuccess) err = drained;
      if (err == hipSuccess)
        err = hipMemcpy(hist.data(), sel + tl.hist, hist.size() * 8, hipMemcpyDeviceToHost);
      if (err != hipSuccess) break;
      const int bits = pbh::tail_digit_bits(done);
      for (int64_t j = 0; j < nb; ++j)
        pbh::tail_pick(hist.data() + j * pbh::kTailBins, bits, &st[(size_t)j]);
      done += bits;
      ++ran;
    }
    most = std::max(most, ran);
    if (err == hipSuccess) err = put_prefixes();
    if (err == hipSuccess) err = pbh::launch_tail_gather(t, done, e->stream);
    const hipError_t drained = hipStreamSynchronize(e->stream);
    if (err == hipSuccess) err = drained;
    cursor.resize((size_t)nb);
    part.resize((size_t)(2 * l.rows * l.npad));
    rows.resize((size_t)l.rows);
    if (err == hipSuccess)
      err = hipMemcpy(cursor.data(), sel + tl.cursor, cursor.size() * 8, hipMemcpyDeviceToHost);
    if (err == hipSuccess)
      err = hipMemcpy(part.data(), at<const double>(e->scratch, l.part), part.size() * 8,
                      hipMemcpyDeviceToHost);
    for (int64_t j = 0; err == hipSuccess && j < nb; ++j) {
      const pbh::TailState &s = st[(size_t)j];
      if (cursor[(size_t)j] != pbh::tail_candidates(s, done) ||
          cursor[(size_t)j] > (uint64_t)capacity) {
        broken = "the candidates gathered are not those counted";
        break;
      }
      keys.resize((size_t)cursor[(size_t)j]);
      if (!keys.empty())
        err = hipMemcpy(keys.data(), sel + tl.list + j * capacity, keys.size() * 8,
                        hipMemcpyDeviceToHost);
      if (err != hipSuccess) break;
      for (int64_t r = 0; r < l.rows; ++r)
        rows[(size_t)r] = pbh::LsePair{part[(size_t)(r * l.npad + j)],
                                       part[(size_t)((l.rows + r) * l.npad + j)]};
      pbh::tail_finish(keys.data(), (int64_t)keys.size(), k, done, s, rows.data(), l.rows,
                       tail ? tail + (j0 + j) * k : nullptr,
                       rest_lse ? rest_lse + j0 + j : nullptr);
    }
  }
  (void)hipStreamSynchronize(e->stream);
  if (err != hipSuccess) return hip_fail(kEntry, err);
  if (broken) return fail(PBH_ERR_HIP, "%s: %s", kEntry, broken);
  if (passes) *passes = most;
  return PBH_OK;
}

int pbh_trace_ess(pbh_engine *e, int64_t first, int64_t count, double *ess) {
  if (const int rc = trace_enter(e, {}, false, first, count, 2, [] { return PBH_OK; }, kRangeEss))
    return rc;
  HIP_TRY(hipSetDevice(e->device));
  const size_t dn = (size_t)e->d * e->n;
  if (e->ess_fft >= 2)
    if (const int rc = pbh::dgrow(e->ess_list, e->ess_list_len, (dn + 1) / 2 + 1)) return rc;
  HIP_TRY(pbh::launch_trace_ess(e->tx, e->n, e->d, first, count, e->ess, e->stream,
                                e->ess_fft, e->ess_list));
  if (ess) {
    // through a pinned staging buffer: a pageable copy of the 512 KB cfg5
    // result was ~0.1 ms of the call
    if (const int rc = stage(e, dn)) return rc;
    HIP_TRY(hipMemcpyAsync(e->stage, e->ess, dn * sizeof(double), hipMemcpyDeviceToHost,
                           e->stream));
    HIP_TRY(pbh::stream_wait(e));
    std::memcpy(ess, e->stage, dn * sizeof(double));
  }
  return PBH_OK;
}

int pbh_trace_ess_total(pbh_engine *e, int64_t first, int64_t count, double *total) {
  if (check_ptr(e, "engine") || check_ptr(total, "total")) return PBH_ERR_ARG;
  // the per-chain ESS on the device (no copy), then the per-dim sums
  if (const int rc = pbh_trace_ess(e, first, count, nullptr)) return rc;
  const int d = e->d;
  if (const int rc = stage(e, d)) return rc;
  // the totals land in the scalar scratch (d doubles, allocated lazily)
  if (!e->ess_tot) {
    if (const int rc = pbh::dalloc(e->ess_tot, PBH_MAX_DIM)) return rc;
  }
  HIP_TRY(pbh::launch_ess_total(e->ess, e->n, d, e->ess_tot, e->stream));
  HIP_TRY(hipMemcpyAsync(e->stage, e->ess_tot, d * sizeof(double), hipMemcpyDeviceToHost,
                         e->stream));
  HIP_TRY(pbh::stream_wait(e));
  std::memcpy(total, e->stage, d * sizeof(double));
  return PBH_OK;
}

}  // extern "C"
