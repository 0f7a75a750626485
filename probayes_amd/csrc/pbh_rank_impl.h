// pbh_rank_impl.h -- the two pieces of the rank-normalised R-hat that are the
// same arithmetic on the device and on the host: the normal score of a rank
// (Wichura's AS241, PPND16) and the search for the run of equal keys around a
// sorted position.  Compiles as device code (pbh_rank.hip) and with a host
// compiler alone (tests/rank_host_main.cpp): no HIP header is included, only
// the function qualifier below.  Build with -ffp-contract=off: on the host the
// scores must round as CPython's statistics.NormalDist.inv_cdf does.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PBH_RANK_HD __host__ __device__ inline
#else
#define PBH_RANK_HD inline
#endif

namespace pbh {

// The standard normal quantile of p in (0, 1): AS241 PPND16 in the operation
// order of CPython's _normal_dist_inv_cdf (mu = 0, sigma = 1).  Three branches:
// |p - 1/2| <= 0.425 (no libm call), r = sqrt(-log(min(p, 1 - p))) <= 5, r > 5.
// A NaN p gives NaN.
PBH_RANK_HD double normal_quantile(double p) {
  const double q = p - 0.5;
  if (fabs(q) <= 0.425) {
    const double r = 0.180625 - q * q;
    const double num = (((((((2.5090809287301226727e+3 * r +
                              3.3430575583588128105e+4) * r +
                             6.7265770927008700853e+4) * r +
                            4.5921953931549871457e+4) * r +
                           1.3731693765509461125e+4) * r +
                          1.9715909503065514427e+3) * r +
                         1.3314166789178437745e+2) * r +
                        3.3871328727963666080e+0) * q;
    const double den = (((((((5.2264952788528545610e+3 * r +
                              2.8729085735721942674e+4) * r +
                             3.9307895800092710610e+4) * r +
                            2.1213794301586595867e+4) * r +
                           5.3941960214247511077e+3) * r +
                          6.8718700749205790830e+2) * r +
                         4.2313330701600911252e+1) * r +
                        1.0);
    return num / den;
  }
  double r = q <= 0.0 ? p : 1.0 - p;
  r = sqrt(-log(r));
  double num, den;
  if (r <= 5.0) {
    r = r - 1.6;
    num = (((((((7.74545014278341407640e-4 * r +
                 2.27238449892691845833e-2) * r +
                2.41780725177450611770e-1) * r +
               1.27045825245236838258e+0) * r +
              3.64784832476320460504e+0) * r +
             5.76949722146069140550e+0) * r +
            4.63033784615654529590e+0) * r +
           1.42343711074968357734e+0);
    den = (((((((1.05075007164441684324e-9 * r +
                 5.47593808499534494600e-4) * r +
                1.51986665636164571966e-2) * r +
               1.48103976427480074590e-1) * r +
              6.89767334985100004550e-1) * r +
             1.67638483018380384940e+0) * r +
            2.05319162663775882187e+0) * r +
           1.0);
  } else if (r > 5.0) {
    r = r - 5.0;
    num = (((((((2.01033439929228813265e-7 * r +
                 2.71155556874348757815e-5) * r +
                1.24266094738807843860e-3) * r +
               2.65321895265761230930e-2) * r +
              2.96560571828504891230e-1) * r +
             1.78482653991729133580e+0) * r +
            5.46378491116411436990e+0) * r +
           6.65790464350110377720e+0);
    den = (((((((2.04426310338993978564e-15 * r +
                 1.42151175831644588870e-7) * r +
                1.84631831751005468180e-5) * r +
               7.86869131145613259100e-4) * r +
              1.48753612908506148525e-2) * r +
             1.36929880922735805310e-1) * r +
            5.99832206555887937690e-1) * r +
           1.0);
  } else {
    return r;   // (a NaN p)
  }
  const double x = num / den;
  return q < 0.0 ? -x : x;
}

// The normal score of the 1-based average rank r among M values:
// normal_quantile((r - 3/8) / (M + 1/4)).
PBH_RANK_HD double normal_score(double r, double M) {
  return normal_quantile((r - 0.375) / (M + 0.25));
}

// The run [lo, hi) of keys equal to keys[p] in the ascending array keys[0..M),
// 0 <= p < M: gallops outwards from p in doubling steps to the first key that
// differs (or the array's end), then bisects between the last equal and the
// first different one.  O(log run) reads on either side.
PBH_RANK_HD void equal_run(const uint64_t *keys, int64_t M, int64_t p, int64_t *lo,
                           int64_t *hi) {
  const uint64_t key = keys[p];
  int64_t good = p, bad = -1;
  for (int64_t step = 1;; step <<= 1) {
    const int64_t t = good - step;
    if (t < 0) break;   // (bad = -1: before the array)
    if (keys[t] != key) {
      bad = t;
      break;
    }
    good = t;
  }
  while (good - bad > 1) {
    const int64_t mid = bad + (good - bad) / 2;
    if (keys[mid] == key) good = mid; else bad = mid;
  }
  *lo = good;
  good = p;
  bad = M;
  for (int64_t step = 1;; step <<= 1) {
    if (step >= M - good) break;   // (good + step >= M: bad = M, past the array)
    const int64_t t = good + step;
    if (keys[t] != key) {
      bad = t;
      break;
    }
    good = t;
  }
  while (bad - good > 1) {
    const int64_t mid = good + (bad - good) / 2;
    if (keys[mid] == key) good = mid; else bad = mid;
  }
  *hi = bad;
}

// The 1-based average rank of the run [lo, hi): the mean of lo + 1 .. hi, a
// multiple of 1/2 and exact in fp64 below 2^52 elements.
PBH_RANK_HD double average_rank(int64_t lo, int64_t hi) {
  return (double)(lo + hi + 1) * 0.5;
}

}  // namespace pbh
