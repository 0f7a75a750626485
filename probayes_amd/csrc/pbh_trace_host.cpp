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

static_assert(kHistMaxDims == PBH_MAX_DIM, "a dim group list per engine dim");
static_assert(((int64_t)1 << kHistMaxDepth) == PBH_HIST_MAX_BINS, "the deepest search");
static_assert(kHistLanes * kHistMaxSlice < ((int64_t)1 << 32), "a workgroup's uint32 counter");

std::string hist_check_edges(int32_t d, const int32_t *n_bins, const double *edges) {
  char buf[160];
  buf[0] = 0;
  bool any = false;
  const double *e = edges;
  for (int32_t k = 0; k < d; ++k) {
    const int32_t B = n_bins[k];
    if (B < 0 || B > PBH_HIST_MAX_BINS) {
      snprintf(buf, sizeof buf, "dim %d: n_bins = %d outside 0..%d", (int)k, (int)B,
               PBH_HIST_MAX_BINS);
      return buf;
    }
    if (B == 0) continue;
    any = true;
    for (int32_t i = 0; i <= B; ++i) {
      if (!std::isfinite(e[i])) {
        snprintf(buf, sizeof buf, "dim %d: edge %d = %g is not finite", (int)k, (int)i, e[i]);
        return buf;
      }
      if (i > 0 && !(e[i - 1] < e[i])) {
        snprintf(buf, sizeof buf, "dim %d: edge %d = %.17g does not lie above edge %d = %.17g "
                 "(the edges strictly increase)", (int)k, (int)i, e[i], (int)i - 1, e[i - 1]);
        return buf;
      }
    }
    e += B + 1;
  }
  if (!any) snprintf(buf, sizeof buf, "every n_bins[k] of the %d dims is 0: no dim to count", (int)d);
  return buf;
}

bool hist_guess_ok(const double *e, int32_t bins) {
  if (bins < 1) return false;
  const double e0 = e[0], s = (double)bins / (e[bins] - e0);
  if (!std::isfinite(s) || !(s > 0.)) return false;
  for (int32_t i = 0; i < bins; ++i) {
    const double last = std::nextafter(e[i + 1], -std::numeric_limits<double>::infinity());
    const int32_t lo = hist_guess(bins, e0, s, e[i]), hi = hist_guess(bins, e0, s, last);
    if (lo < i - 1 || lo > i + 1 || hi < i - 1 || hi > i + 1) return false;
  }
  return true;
}

HistDimPlan hist_dim_plan(const double *e, int32_t bins) {
  HistDimPlan p{bins, 0, 0., 0., 0.};
  if (bins < 1) return p;
  p.e0 = e[0];
  p.eB = e[bins];
  if (hist_guess_ok(e, bins)) {
    p.mode = kHistGuess;
    p.s = (double)bins / (p.eB - p.e0);
  } else {
    p.mode = hist_depth(bins);
  }
  return p;
}

void hist_fill_table(const double *e, const HistDimPlan &p, double *t) {
  const int64_t len = hist_table_len(p.bins);
  const double inf = std::numeric_limits<double>::infinity();
  // the guess reads e[0 .. bins]; the search e[0 .. bins - 1] and the padding
  const int64_t held = p.mode == kHistGuess ? (int64_t)p.bins + 1 : (int64_t)p.bins;
  for (int64_t i = 0; i < len; ++i) t[i] = i < held ? e[i] : inf;
}

namespace {

// the chain blocks and the record slices of a histogram's grid of `groups`
// jobs per (chain block, slice)
bool hist_slices(int64_t n, int64_t count, int64_t groups, int64_t *chain_blocks, int64_t *slices,
                 int64_t *slice_len) {
  int64_t draws;
  if (n < 1 || count < 1 || groups < 1) return false;
  if (__builtin_mul_overflow(n, count, &draws)) return false;
  const int64_t blocks = n / kHistLanes + (n % kHistLanes != 0);
  if (blocks > 0x7fffffff) return false;
  int64_t jobs;
  if (__builtin_mul_overflow(blocks, groups, &jobs)) return false;
  const int64_t want = std::min(count, (kPointwiseGroups + jobs - 1) / jobs);
  const int64_t len = std::min((count + want - 1) / want, kHistMaxSlice);
  const int64_t s = (count + len - 1) / len;
  if (s > 65535) return false;
  *chain_blocks = blocks;
  *slices = s;
  *slice_len = len;
  return true;
}

int64_t hist_dim_lds(int32_t bins) {
  return (8 * hist_table_len(bins) + 4 * ((int64_t)bins + 3) + 7) / 8 * 8;
}

}  // namespace

bool hist_layout(int64_t n, int64_t count, int32_t d, const int32_t *n_bins, HistLayout *out) {
  if (d < 1 || d > kHistMaxDims) return false;
  HistLayout l;
  memset(&l, 0, sizeof l);
  int64_t room = 0;   // what the open group may still take; 0: none is open
  for (int32_t k = 0; k < d; ++k) {
    const int32_t B = n_bins[k];
    if (B < 0 || B > PBH_HIST_MAX_BINS) return false;
    if (B == 0) continue;
    const int64_t need = hist_dim_lds(B);
    const bool alone = need > kHistLdsBudget / 2;
    if (alone || need > room) {
      // a new group
      l.group_first[l.groups] = l.dims;
      l.tab_off[l.groups] = (int32_t)l.n_tab;
      l.ctr_off[l.groups] = (int32_t)l.n_ctr;
      ++l.groups;
      room = alone ? need : kHistLdsBudget;
    }
    const int32_t g = l.groups - 1, j = l.dims++;
    l.dim[j] = k;
    l.tab[j] = l.tab_len[g];
    l.ctr[j] = l.ctr_len[g];
    l.tab_len[g] += (int32_t)hist_table_len(B);
    l.ctr_len[g] += B + 3;
    l.n_tab += hist_table_len(B);
    l.n_ctr += B + 3;
    room -= need;
  }
  if (l.dims == 0) return false;
  l.group_first[l.groups] = l.dims;
  for (int32_t g = 0; g < l.groups; ++g)
    l.lds_bytes = std::max(l.lds_bytes, ((int64_t)8 * l.tab_len[g] + 4 * l.ctr_len[g] + 7) / 8 * 8);
  if (!hist_slices(n, count, l.groups, &l.chain_blocks, &l.slices, &l.slice_len)) return false;
  int64_t at = 0;
  const auto take = [&at](int64_t bytes) {
    const int64_t here = at;
    at += (bytes + 255) / 256 * 256;
    return here;
  };
  l.tables = take(l.n_tab * 8);
  l.counts = take(l.n_ctr * 8);
  l.bytes = at;
  *out = l;
  return true;
}

std::string hist2d_check_pairs(int32_t d, const int32_t *n_bins, int32_t n_pairs,
                               const int32_t *pairs) {
  char buf[160];
  buf[0] = 0;
  if (n_pairs < 1 || n_pairs > 65535) {
    snprintf(buf, sizeof buf, "n_pairs = %d outside 1..65535", (int)n_pairs);
    return buf;
  }
  for (int32_t p = 0; p < n_pairs; ++p) {
    for (int side = 0; side < 2; ++side) {
      const int32_t k = pairs[2 * p + side];
      if (k < 0 || k >= d) {
        snprintf(buf, sizeof buf, "pair %d: dim %d outside [0, %d)", (int)p, (int)k, (int)d);
        return buf;
      }
      if (n_bins[k] < 1) {
        snprintf(buf, sizeof buf, "pair %d: dim %d has no edges (n_bins = %d)", (int)p, (int)k,
                 (int)n_bins[k]);
        return buf;
      }
    }
    const int64_t cells = (int64_t)n_bins[pairs[2 * p]] * n_bins[pairs[2 * p + 1]];
    if (cells > PBH_HIST2D_MAX_CELLS) {
      snprintf(buf, sizeof buf, "pair %d: dims %d and %d make %d x %d = %lld cells, above %d",
               (int)p, (int)pairs[2 * p], (int)pairs[2 * p + 1], (int)n_bins[pairs[2 * p]],
               (int)n_bins[pairs[2 * p + 1]], (long long)cells, PBH_HIST2D_MAX_CELLS);
      return buf;
    }
  }
  return buf;
}

bool hist2d_layout(int64_t n, int64_t count, int32_t d, const int32_t *n_bins, int32_t n_pairs,
                   const int32_t *pairs, Hist2dLayout *out) {
  if (d < 1 || d > kHistMaxDims) return false;
  for (int32_t k = 0; k < d; ++k)
    if (n_bins[k] < 0 || n_bins[k] > PBH_HIST_MAX_BINS) return false;
  if (!hist2d_check_pairs(d, n_bins, n_pairs, pairs).empty()) return false;
  Hist2dLayout l;
  l.n_pairs = n_pairs;
  l.n_tab = l.n_ctr = l.lds_bytes = 0;
  for (int32_t k = 0; k < kHistMaxDims; ++k) {
    l.tab_off[k] = -1;
    if (k < d && n_bins[k] > 0) {
      l.tab_off[k] = (int32_t)l.n_tab;
      l.n_tab += hist_table_len(n_bins[k]);
    }
  }
  l.out.resize((size_t)n_pairs);
  for (int32_t p = 0; p < n_pairs; ++p) {
    const int32_t Ba = n_bins[pairs[2 * p]], Bb = n_bins[pairs[2 * p + 1]];
    l.out[(size_t)p] = l.n_ctr;
    l.n_ctr += (int64_t)Ba * Bb;
    l.lds_bytes = std::max(l.lds_bytes,
                           8 * (hist_table_len(Ba) + hist_table_len(Bb)) + ((int64_t)4 * Ba * Bb + 7) / 8 * 8);
  }
  if (!hist_slices(n, count, n_pairs, &l.chain_blocks, &l.slices, &l.slice_len)) return false;
  int64_t at = 0;
  const auto take = [&at](int64_t bytes) {
    const int64_t here = at;
    at += (bytes + 255) / 256 * 256;
    return here;
  };
  l.tables = take(l.n_tab * 8);
  l.pairs = take((int64_t)n_pairs * 4 * 8);
  l.counts = take(l.n_ctr * 8);
  l.bytes = at;
  *out = std::move(l);
  return true;
}

}  // namespace pbh
