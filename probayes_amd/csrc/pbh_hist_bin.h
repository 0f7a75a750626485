// pbh_hist_bin.h -- the bin of a value among strictly increasing finite edges
// e[0 .. B], as probayes_amd/diag.py hist_bin defines it (and np.histogram
// counts): bin i holds e[i] <= x < e[i + 1], the last bin also x == e[B];
// kHistBelow for x < e[0], kHistAbove for x > e[B], kHistNan for a NaN.  Plain
// comparisons: -0.0 and +0.0 are one value, -inf is below and +inf above.
//
// The kernels of pbh_hist.hip and a host program (tests/hist_host_main.cpp)
// both include this file: the function the device runs is the one the CPU
// tests hold against diag.hist_bin.  Built without FMA contraction
// (-ffp-contract=off) on either side: the guess must round alike.
//
// A dim's lookup table has hist_table_len(B) = 2^depth + 1 doubles, depth the
// least with 2^depth >= B.  Two lookups:
//   search  t[0 .. B - 1] = e[0 .. B - 1], t[B .. 2^depth - 1] = +inf.  With x
//           inside [e[0], e[B]] the bin is the number of inner edges e[1 .. B -
//           1] that are <= x: a branch-free binary search of `depth` steps over
//           t[1 .. 2^depth - 1].  No step needs a bound check: the padding is
//           above every x that gets there.  The depth is a template parameter,
//           so the search is straight-line code.
//   guess   t[0 .. B] = e[0 .. B].  i = the integer part of (x - e[0]) s held to
//           [0, B - 1], s = B / (e[B] - e[0]); one step down if x < e[i], else
//           one step up if i < B - 1 and x >= e[i + 1]: two table reads, not
//           `depth` dependent ones.  Right for every x when hist_guess_ok
//           (pbh_trace_host.h) holds for the edges: the guess is monotone in x,
//           so if it is within one of i at e[i] and at the double just below e[i
//           + 1], it is within one of i for every x of bin i.
#pragma once
#include <stdint.h>

#if defined(__HIP__)   // (the compiler in HIP mode, not hipcc building plain C++)
#define PBH_HIST_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define PBH_HIST_HD inline
#endif
#if defined(__clang__)
#define PBH_HIST_UNROLL _Pragma("unroll")
#else
#define PBH_HIST_UNROLL
#endif

namespace pbh {

constexpr int kHistBelow = -1, kHistAbove = -2, kHistNan = -3;
constexpr int kHistMaxDepth = 12;   // 2^12 = PBH_HIST_MAX_BINS
constexpr int kHistGuess = -1;      // a dim's mode: the guess, else the search's depth

PBH_HIST_HD int hist_depth(int32_t bins) {
  int s = 0;
  while (((int32_t)1 << s) < bins) ++s;
  return s;
}

PBH_HIST_HD int64_t hist_table_len(int32_t bins) { return ((int64_t)1 << hist_depth(bins)) + 1; }

// The integer part of (x - e0) s held to [0, bins - 1], for e0 <= x (the
// product is >= +0; a product that is not finite never gets here, hist_guess_ok
// refuses such an s).  Monotone in x.
PBH_HIST_HD int32_t hist_guess(int32_t bins, double e0, double s, double x) {
  const double g = (x - e0) * s, top = (double)(bins - 1);
  return (int32_t)(g < top ? g : top);
}

template <int DEPTH>
PBH_HIST_HD int32_t hist_bin_search(const double *t, double e0, double eB, double x) {
  if (x != x) return kHistNan;
  if (x < e0) return kHistBelow;
  if (x > eB) return kHistAbove;
  int32_t pos = 0;
  PBH_HIST_UNROLL
  for (int s = DEPTH - 1; s >= 0; --s) {
    const int32_t j = pos + ((int32_t)1 << s);
    if (t[j] <= x) pos = j;
  }
  return pos;
}

PBH_HIST_HD int32_t hist_bin_guess(const double *t, int32_t bins, double e0, double eB, double s,
                                   double x) {
  if (x != x) return kHistNan;
  if (x < e0) return kHistBelow;
  if (x > eB) return kHistAbove;
  int32_t i = hist_guess(bins, e0, s, x);
  if (x < t[i])
    --i;   // (x >= e0 = t[0]: never from 0)
  else if (i < bins - 1 && x >= t[i + 1])
    ++i;
  return i;
}

// Either lookup by a dim's mode (kHistGuess, or the search's depth 0 ..
// kHistMaxDepth): what a caller without a compile-time mode runs.
PBH_HIST_HD int32_t hist_bin_any(int mode, const double *t, int32_t bins, double e0, double eB,
                                 double s, double x) {
  switch (mode) {
    case 0: return hist_bin_search<0>(t, e0, eB, x);
    case 1: return hist_bin_search<1>(t, e0, eB, x);
    case 2: return hist_bin_search<2>(t, e0, eB, x);
    case 3: return hist_bin_search<3>(t, e0, eB, x);
    case 4: return hist_bin_search<4>(t, e0, eB, x);
    case 5: return hist_bin_search<5>(t, e0, eB, x);
    case 6: return hist_bin_search<6>(t, e0, eB, x);
    case 7: return hist_bin_search<7>(t, e0, eB, x);
    case 8: return hist_bin_search<8>(t, e0, eB, x);
    case 9: return hist_bin_search<9>(t, e0, eB, x);
    case 10: return hist_bin_search<10>(t, e0, eB, x);
    case 11: return hist_bin_search<11>(t, e0, eB, x);
    case 12: return hist_bin_search<12>(t, e0, eB, x);
    default: return hist_bin_guess(t, bins, e0, eB, s, x);
  }
}

}  // namespace pbh
