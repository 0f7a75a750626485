// pbh_trace_host.cpp -- see pbh_trace_host.h.
#include "pbh_trace_host.h"

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <limits>

#include "../../include/pbhip.h"

namespace pbh {

bool trace_window_ok(int64_t rec, int64_t first, int64_t count, int64_t min_count) {
  return first >= 0 && first <= rec && count >= min_count && count <= rec - first;
}

int64_t trace_window_end(int64_t first, int64_t count) {
  int64_t end;
  if (__builtin_add_overflow(first, count, &end))   // (the two have one sign)
    end = count > 0 ? std::numeric_limits<int64_t>::max() : std::numeric_limits<int64_t>::min();
  return end;
}

std::string quantile_list_error(int32_t nq, const double *q) {
  char buf[96];
  buf[0] = 0;
  if (nq < 1 || nq > PBH_QUANTILE_MAX_Q) {
    snprintf(buf, sizeof buf, "nq = %d outside 1..%d", (int)nq, PBH_QUANTILE_MAX_Q);
    return buf;
  }
  for (int32_t j = 0; j < nq; ++j)
    if (!(q[j] >= 0. && q[j] <= 1.)) {
      snprintf(buf, sizeof buf, "q[%d] = %g is not a quantile in [0, 1]", (int)j, q[j]);
      break;
    }
  return buf;
}

PooledPlan pooled_plan(int64_t M, int32_t nq, const double *q) {
  PooledPlan p;
  p.lo.resize(nq);
  p.hi.resize(nq);
  p.frac.resize(nq);
  for (int32_t j = 0; j < nq; ++j) {
    const double vi = (double)(M - 1) * q[j], fl = std::floor(vi);
    p.lo[j] = std::min((int64_t)fl, M - 1);
    p.hi[j] = std::min(p.lo[j] + 1, M - 1);
    p.frac[j] = vi - fl;
    p.ranks.push_back((uint64_t)p.lo[j]);
    p.ranks.push_back((uint64_t)p.hi[j]);
  }
  p.ranks.push_back((uint64_t)(M - 1));
  std::sort(p.ranks.begin(), p.ranks.end());
  p.ranks.erase(std::unique(p.ranks.begin(), p.ranks.end()), p.ranks.end());
  return p;
}

void pooled_interpolate(const PooledPlan &p, int64_t d, const double *stats, double *out,
                        double *order_stats) {
  const int64_t nq = (int64_t)p.lo.size(), nt = (int64_t)p.ranks.size();
  const auto at = [&](int64_t r) {
    return (int64_t)(std::lower_bound(p.ranks.begin(), p.ranks.end(), (uint64_t)r) -
                     p.ranks.begin());
  };
  for (int64_t k = 0; k < d; ++k) {
    const double *s = stats + k * nt;
    const bool has_nan = s[nt - 1] != s[nt - 1];
    for (int64_t j = 0; j < nq; ++j) {
      const double a = s[at(p.lo[j])], b = s[at(p.hi[j])], diff = b - a, g = p.frac[j];
      const double v = g >= 0.5 ? b - diff * (1. - g) : a + diff * g;
      out[j * d + k] = has_nan ? std::numeric_limits<double>::quiet_NaN() : v;
      if (order_stats) {
        order_stats[(2 * j) * d + k] = a;
        order_stats[(2 * j + 1) * d + k] = b;
      }
    }
  }
}

bool rank_layout(int64_t n, int64_t count, int32_t d, int64_t select_words, bool want_ranks,
                 RankLayout *out) {
  int64_t M;
  if (n < 1 || count < 1 || d < 1 || select_words < 0) return false;
  if (__builtin_mul_overflow(n, count, &M) || M >= ((int64_t)1 << 32)) return false;
  RankLayout l;
  l.M = M;
  l.tiles = (M + kRankTile - 1) / kRankTile;
  l.chunk_tiles = (l.tiles + kRankMaxChunks - 1) / kRankMaxChunks;
  l.chunks = (l.tiles + l.chunk_tiles - 1) / l.chunk_tiles;
  int64_t at = 0;
  const auto take = [&at](int64_t bytes) {
    const int64_t here = at;
    at += (bytes + 255) / 256 * 256;
    return here;
  };
  l.select = take(select_words * 8);
  l.med = take((int64_t)d * 8);
  l.res = take(2 * (int64_t)d * 8);
  l.state = take(8 * 4);
  l.chunk = take(l.chunks * kRankBins * 4);
  l.hist = take(l.tiles * kRankBins * 4);
  l.stats = take(6 * n * 8);
  l.key[0] = take(M * 8);
  l.key[1] = take(M * 8);
  l.idx[0] = take(M * 4);
  l.idx[1] = take(M * 4);
  l.z = take(M * 8);
  l.r = want_ranks ? take(M * 8) : at;
  l.bytes = at;
  *out = l;
  return true;
}

bool ess_layout(int64_t n, int64_t count, int32_t d, int64_t base, int64_t select_words,
                EssLayout *out) {
  if (n < 1 || count < 4 || count / 2 > PBH_ESS_RANK_MAX_HALF || d < 1 || base < 0 ||
      base % 256 != 0 || select_words < 0)
    return false;
  EssLayout l;
  l.h = count / 2;
  l.pairs = n / 2 + n % 2;
  l.run = (l.pairs + kEssMaxGroups - 1) / kEssMaxGroups;
  l.groups = (l.pairs + l.run - 1) / l.run;
  int64_t at = base;
  const auto take = [&at](int64_t bytes) {
    const int64_t here = at;
    at += (bytes + 255) / 256 * 256;
    return here;
  };
  l.select = take(select_words * 8);
  l.thr = take(2 * (int64_t)d * 8);
  l.part = take(l.groups * kEssPoints * 8);
  l.acov = take(4 * (int64_t)d * l.h * 8);
  l.means = take(4 * 2 * (int64_t)d * n * 8);
  l.stats = take(6 * (int64_t)d * n * 8);
  l.bytes = at;
  *out = l;
  return true;
}

double multi_chain_ess(const double *m, const double *A, int64_t C, int64_t h,
                       int64_t *k_star) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const double mean_var = A[0] * (double)h / ((double)h - 1.);
  // (of m - m[0]: equal means have variance 0 exactly)
  double sm = 0.;
  for (int64_t j = 0; j < C; ++j) sm += m[j] - m[0];
  const double mbar = sm / (double)C;
  double sd = 0.;
  for (int64_t j = 0; j < C; ++j) {
    const double dev = (m[j] - m[0]) - mbar;
    sd += dev * dev;
  }
  const double var_plus = A[0] + sd / ((double)C - 1.);
  const auto rho = [&](int64_t t) { return t == 0 ? 1. : 1. - (mean_var - A[t]) / var_plus; };
  const auto pair = [&](int64_t k) { return rho(2 * k) + rho(2 * k + 1); };
  const int64_t K = h / 2;
  int64_t ks = K;
  for (int64_t k = 1; k < K; ++k)
    if (!(pair(k) > 0.)) {
      ks = k;
      break;
    }
  // the running minimum as np.minimum forms it: a NaN stays
  double run = pair(0), sum = run;
  for (int64_t k = 1; k < ks; ++k) {
    const double p = pair(k);
    run = run != run ? run : p != p ? p : p < run ? p : run;
    sum += run;
  }
  double tau = -1. + 2. * sum;
  if (ks < K && rho(2 * ks) > 0.) tau = tau + rho(2 * ks);
  const double floor_tau = 1. / std::log10((double)C * (double)h);
  tau = tau != tau ? nan : floor_tau > tau ? floor_tau : tau;
  if (k_star) *k_star = ks;
  return (double)C * (double)h / tau;
}

bool pointwise_layout(int64_t n, int64_t count, int32_t n_obs, int64_t select_words,
                      int64_t prog_doubles, PointwiseLayout *out) {
  int64_t draws;
  if (n < 1 || count < 1 || n_obs < 1 || n_obs > PBH_EXPR_MAX_OBS || select_words < 0 ||
      prog_doubles < 1 || prog_doubles > ((int64_t)1 << 40))
    return false;
  if (__builtin_mul_overflow(n, count, &draws)) return false;
  PointwiseLayout l;
  l.chain_blocks = n / kPointwiseLanes + (n % kPointwiseLanes != 0);
  if (l.chain_blocks > 65535) return false;
  l.tiles = ((int64_t)n_obs + kPointwiseTile - 1) / kPointwiseTile;
  l.npad = l.tiles * kPointwiseTile;
  const int64_t groups = l.chain_blocks * l.tiles;
  const int64_t want = std::min(count, (kPointwiseGroups + groups - 1) / groups);
  l.slice_len = (count + want - 1) / want;
  l.slices = (count + l.slice_len - 1) / l.slice_len;
  l.rows = l.chain_blocks * l.slices;
  int64_t at = 0;
  const auto take = [&at](int64_t bytes) {
    const int64_t here = at;
    at += (bytes + 255) / 256 * 256;
    return here;
  };
  l.select = take(select_words * 8);
  l.prog = take(prog_doubles * 8);
  l.part = take(6 * l.rows * l.npad * 8);
  l.res = take(3 * l.npad * 8);
  l.bytes = at;
  *out = l;
  return true;
}

void pointwise_combine(const LsePair *lse, const Moments *mom, LsePair *lse_out,
                       Moments *mom_out) {
  LsePair fl[kPointwiseFold];
  Moments fm[kPointwiseFold];
  for (int t = 0; t < kPointwiseFold; ++t) {
    fl[t] = lse[t];
    fm[t] = mom[t];
    for (int c = t + kPointwiseFold; c < kPointwiseLanes; c += kPointwiseFold) {
      fl[t] = lse_merge(fl[t], lse[c]);
      fm[t] = moments_merge(fm[t], mom[c]);
    }
  }
  for (int w = kPointwiseFold / 2; w > 0; w >>= 1)
    for (int t = 0; t < w; ++t) {
      fl[t] = lse_merge(fl[t], fl[t + w]);
      fm[t] = moments_merge(fm[t], fm[t + w]);
    }
  *lse_out = fl[0];
  *mom_out = fm[0];
}

void pointwise_finish(const LsePair *lse, const Moments *mom, int64_t rows, double *lse_out,
                      double *mean_out, double *var_out) {
  LsePair l = lse_identity();
  Moments m = moments_identity();
  for (int64_t r = 0; r < rows; ++r) {
    l = lse_merge(l, lse[r]);
    m = moments_merge(m, mom[r]);
  }
  if (lse_out) *lse_out = lse_value(l);
  if (mean_out) *mean_out = moments_mean(m);
  if (var_out) *var_out = m.m2 / (m.n - 1.);
}

uint64_t tail_key(double v) {
  if (v != v) return ~0ull;
  if (v == 0.) v = 0.;
  uint64_t u;
  memcpy(&u, &v, 8);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

double tail_key_value(uint64_t key) {
  if (key == ~0ull) return std::numeric_limits<double>::quiet_NaN();
  const uint64_t u = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
  double v;
  memcpy(&v, &u, 8);
  return v;
}

void tail_pick(const uint64_t *hist, int bits, TailState *s) {
  const uint64_t bins = (uint64_t)1 << bits;
  uint64_t before = 0, digit = 0;
  for (; digit + 1 < bins && before + hist[digit] <= s->rank; ++digit) before += hist[digit];
  s->prefix = (s->prefix << bits) | digit;
  s->rank -= before;
  s->below += before;
  s->under = hist[digit];
}

void tail_finish(uint64_t *keys, int64_t n_keys, int64_t k, int done, const TailState &s,
                 const LsePair *rows, int64_t n_rows, double *tail, double *rest_lse) {
  std::sort(keys, keys + n_keys);
  const double cut = tail_key_value(s.prefix);   // (read with all 64 bits fixed only)
  if (tail)
    for (int64_t i = 0; i < k; ++i) tail[i] = i < n_keys ? tail_key_value(keys[i]) : cut;
  if (!rest_lse) return;
  LsePair rest = lse_identity();
  for (int64_t i = k; i < n_keys; ++i) rest = lse_push(rest, -tail_key_value(keys[i]));
  if (done == 64) {
    // of the `under` keys at the cut, rank + 1 went into the tail
    const uint64_t ties = s.under - (s.rank + 1);
    if (ties) rest = lse_merge(rest, LsePair{-cut, (double)ties});
  }
  LsePair dev = lse_identity();
  for (int64_t r = 0; r < n_rows; ++r) dev = lse_merge(dev, rows[r]);
  *rest_lse = lse_value(lse_merge(rest, dev));
}

int64_t tail_default_capacity(int64_t k) {
  return k > 32768 ? 2 * k : 65536;
}

int64_t tail_batch_tiles(int64_t capacity) {
  const int64_t tiles = kTailListBytes / (capacity * 8 * kPointwiseTile);
  return tiles < 1 ? 1 : tiles;
}

TailLayout tail_layout(int64_t tiles, int64_t capacity) {
  TailLayout l;
  l.npad = tiles * kPointwiseTile;
  l.prefix = 0;
  l.cursor = l.npad;
  l.hist = 2 * l.npad;
  l.list = l.hist + l.npad * kTailBins;
  l.words = l.list + l.npad * capacity;
  return l;
}

bool cov_layout(int64_t n, int64_t count, int32_t d, CovLayout *out) {
  int64_t draws;
  if (n < 1 || count < 1 || d < 1 || d > PBH_MAX_DIM) return false;
  if (__builtin_mul_overflow(n, count, &draws)) return false;
  CovLayout l;
  l.chain_blocks = n / kCovLanes + (n % kCovLanes != 0);
  if (l.chain_blocks > 0x7fffffff) return false;
  // above one tile: the two diagonal tiles, and per kCovHalf dims of the second
  // a rectangle for either half of the first
  l.pairs = d <= kCovTile
                ? 1
                : 2 + kCovTile / kCovHalf * ((d - kCovTile + kCovHalf - 1) / kCovHalf);
  const int64_t groups = l.chain_blocks * l.pairs;
  const int64_t want = std::min(count, (kPointwiseGroups + groups - 1) / groups);
  l.slice_len = (count + want - 1) / want;
  l.slices = (count + l.slice_len - 1) / l.slice_len;
  l.rows = l.chain_blocks * l.slices;
  l.cols = (int64_t)d + (int64_t)d * (d + 1) / 2;
  int64_t at = 0;
  const auto take = [&at](int64_t bytes) {
    const int64_t here = at;
    at += (bytes + 255) / 256 * 256;
    return here;
  };
  l.K = take((int64_t)d * 8);
  l.part = take(l.rows * l.cols * 8);
  l.res = take(l.cols * 8);
  l.bytes = at;
  *out = l;
  return true;
}

void cov_finish(const double *K, const double *S, const double *P, int64_t M, int32_t d,
                double *mean, double *cov, double *corr) {
  const double m = (double)M;
  double c[PBH_MAX_DIM * PBH_MAX_DIM];
  if (mean)
    for (int32_t a = 0; a < d; ++a) mean[a] = K[a] + S[a] / m;
  for (int32_t a = 0; a < d; ++a)
    for (int32_t b = a; b < d; ++b)
      c[a * d + b] = c[b * d + a] = (P[cov_tri(a, b, d)] - S[a] * S[b] / m) / (m - 1.);
  if (cov) memcpy(cov, c, (size_t)d * d * sizeof(double));
  if (corr)
    for (int32_t a = 0; a < d; ++a)
      for (int32_t b = a; b < d; ++b)
        corr[a * d + b] = corr[b * d + a] = c[a * d + b] / std::sqrt(c[a * d + a] * c[b * d + b]);
}

}  // namespace pbh
