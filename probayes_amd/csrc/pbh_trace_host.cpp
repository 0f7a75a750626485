// pbh_trace_host.cpp -- see pbh_trace_host.h.
#include "pbh_trace_host.h"

#include <stdio.h>

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

}  // namespace pbh
