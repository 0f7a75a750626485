// pbh_pointwise_merge.h -- the two merges of the pointwise reduction
// (pbh_trace_pointwise): the log-sum-exp pair and Chan's moments, stated once
// for the kernels (pbh_pointwise.hip) and for the host (pbh_trace_host.h), so
// that both run the same operations in the same order.  No HIP header needed;
// built with -ffp-contract=off on both sides.
#pragma once
#include <math.h>
#include <stdint.h>

#include "pbh_expr_words.h"   // PBH_HD

namespace pbh {

// exp(m) s: the sum of exp over a set of terms, m their maximum.  The empty
// set is (-inf, 0).  A NaN term makes both fields NaN for good.
struct LsePair {
  double m, s;
};
// (count, shift, mean - shift, M2 = the sum of squared deviations from the
// mean) of a set of terms.  The shift k is the first term the set saw (0 if
// that term was not finite): Welford's update loses eps |mean| / sd
// of the variance to the rounding of its running mean, and a mean kept relative
// to a term of the set is of the size of the spread whatever the terms'
// offset (as pbh_rhat.hip shifts by the window's first record).  The empty set
// is (0, 0, 0, 0).
struct Moments {
  double n, k, mean, m2;
};

PBH_HD inline LsePair lse_identity() { return LsePair{-INFINITY, 0.}; }
PBH_HD inline Moments moments_identity() { return Moments{0., 0., 0., 0.}; }

// The merge of two pairs under the larger maximum M.  The side whose maximum
// is M keeps its sum as it is -- stated, not computed: exp(M - M) is inf - inf
// = NaN at M = +-inf -- and the other is scaled by exp(-|ma - mb|), which is 0
// for a side at -inf.  Two sides at -inf give (-inf, sa + sb); lse_value reads
// -inf from any pair whose maximum is -inf, whatever its sum.
PBH_HD inline LsePair lse_merge(LsePair a, LsePair b) {
  const bool nan = a.m != a.m || b.m != b.m;
  const double M = nan ? NAN : (b.m > a.m ? b.m : a.m);
  const double e = exp(-fabs(a.m - b.m));
  const double fa = a.m == M ? 1. : e, fb = b.m == M ? 1. : e;
  return LsePair{M, a.s * fa + b.s * fb};
}
// lse_merge(a, (v, 1))
PBH_HD inline LsePair lse_push(LsePair a, double v) { return lse_merge(a, LsePair{v, 1.}); }
// log of the sum: -inf for the empty set and for terms all -inf, +inf with a
// +inf term, NaN with a NaN term
PBH_HD inline double lse_value(LsePair a) { return a.m == -INFINITY ? a.m : a.m + log(a.s); }

PBH_HD inline double moments_mean(Moments a) { return a.k + a.mean; }

// Chan, Golub & LeVeque's merge; the result keeps a's shift.  An empty side
// leaves the other as it is (stated: 0 * inf is NaN).  A difference of the
// means that is not finite -- a side holds an infinite term, or a NaN -- gives
// the sum of the two means for the mean, which is what the sum of the terms
// gives: -inf beside finite terms, NaN for both infinities; M2 is NaN from the
// moment an infinite term enters (moments_push).
PBH_HD inline Moments moments_merge(Moments a, Moments b) {
  if (a.n == 0.) return b;
  if (b.n == 0.) return a;
  const double n = a.n + b.n, dk = b.k - a.k, delta = dk + (b.mean - a.mean);
  const bool finite = fabs(delta) < INFINITY;
  const double mean = finite ? a.mean + delta * (b.n / n) : a.mean + (dk + b.mean);
  return Moments{n, a.k, mean, a.m2 + b.m2 + delta * delta * (a.n * b.n / n)};
}
// Welford's step, the merge with one term v: inv_n = 1 / (a.n + 1), which the
// kernel forms once per record for all its terms.  The first term of a set
// becomes its shift.
PBH_HD inline Moments moments_push(Moments a, double v, double inv_n) {
  const double k = a.n == 0. ? (fabs(v) < INFINITY ? v : 0.) : a.k;
  const double x = v - k, delta = x - a.mean;
  const bool finite = fabs(delta) < INFINITY;
  const double mean = finite ? a.mean + delta * inv_n : a.mean + x;
  return Moments{a.n + 1., k, mean, a.m2 + delta * (x - mean)};
}

// How a workgroup of kPointwiseLanes lanes combines its lanes' partials of one
// observation (pointwise_kernel; pointwise_combine on the host): the thread t <
// kPointwiseFold takes the lanes t, t + kPointwiseFold, ... in order, then the
// kPointwiseFold results fold by halves, [t] with [t + w] for w =
// kPointwiseFold / 2 .. 1.
constexpr int kPointwiseLanes = 256, kPointwiseFold = 32, kPointwiseTile = 8;

}  // namespace pbh
