"""The bulk- and tail-ESS across chains (Vehtari et al. 2021) restated from
the definition in np.longdouble by direct sums, for the tests of
probayes_amd/diag.py and of pbh_trace_ess_rank: no FFT, and no code shared
with diag.py (the ranks and scores come from rank_reference.py, the quantiles
from np.sort).  Besides the ESS it returns every Geyer pair P_k and where the
scan stopped, so that a test can assert that no decision of the scan was
within rounding of zero."""
import numpy as np

from rank_reference import ndtri, ref_ranks
from rhat_reference import LD, _quiet

VARIANTS = ('bulk', 'tail_lower', 'tail_upper', 'basic')


@_quiet
def ref_acov(y, first, count):
  """(m [C], A [h]) longdouble of a series y [N, T]: the means of the C = 2 N
  split chains (first halves, then second halves) and their biased
  autocovariance averaged over the split chains, by direct sums."""
  w = np.asarray(y, LD)[:, first:first + count]
  h = count // 2
  halves = np.concatenate([w[:, :h], w[:, count - h:]], axis=0)   # [C, h]
  m = halves.mean(axis=1)
  c = halves - m[:, None]
  a = np.empty(h, LD)
  for t in range(h):
    a[t] = (c[:, :h - t] * c[:, t:]).sum(axis=1).mean() / LD(h)
  return m, a


@_quiet
def ref_ess(m, a):
  """{'ess', 'pairs' [K], 'k_star', 'K', 'rho', 'min_changed', 'added'} in
  longdouble from the split chains' means and averaged autocovariance."""
  m, a = np.asarray(m, LD), np.asarray(a, LD)
  c_all, h = m.size, a.size
  mean_var = a[0] * LD(h) / LD(h - 1)
  var_plus = a[0] + m.var(ddof=1)
  rho = LD(1) - (mean_var - a) / var_plus
  rho[0] = LD(1)
  K = h // 2
  pairs = np.array([rho[2 * k] + rho[2 * k + 1] for k in range(K)], LD)
  k_star = K
  for k in range(1, K):
    if not pairs[k] > 0:
      k_star = k
      break
  total, run, changed = LD(0), None, False
  for k in range(k_star):
    p = pairs[k]
    if run is not None and (np.isnan(run) or np.isnan(p)):
      run = LD(np.nan)
    elif run is not None and run < p:
      changed = True   # the running minimum replaces a larger pair
    else:
      run = p
    total += run
  tau = LD(-1) + LD(2) * total
  added = bool(k_star < K and rho[2 * k_star] > 0)
  if added:
    tau += rho[2 * k_star]
  floor = LD(1) / np.log10(LD(c_all) * LD(h))
  tau = LD(np.nan) if np.isnan(tau) else max(tau, floor)
  return {'ess': LD(c_all) * LD(h) / tau, 'pairs': pairs, 'k_star': k_star, 'K': K,
          'rho': rho, 'min_changed': changed, 'added': added}


def clear(ref, margin=1e-9):
  """Whether every decision of the scan is clear of rounding: |P_k| > margin
  for every k <= k* with k < K."""
  k_hi = min(ref['k_star'], ref['K'] - 1)
  return bool(np.all(np.abs(ref['pairs'][:k_hi + 1]) > margin))


@_quiet
def ref_series(x, first, count):
  """{variant: [N, count, d]}: the series each variant's estimator reads, from
  a host trace x [N, T, d] (fp64 values: scores by rank_reference, indicators
  0. / 1. against the pooled quantiles of the sorted values, as np.quantile
  places them)."""
  x = np.asarray(x, float)
  n, _, d = x.shape
  w = x[:, first:first + count, :]
  ranks = ref_ranks(x, first, count, None)
  z = ndtri((ranks - 0.375) / (n * count + 0.25))
  lower, upper = np.empty(w.shape), np.empty(w.shape)
  for k in range(d):
    v = w[:, :, k]
    if np.isnan(v).any():
      lower[:, :, k] = upper[:, :, k] = np.nan
      continue
    q05, q95 = np.quantile(v.ravel(), [.05, .95])
    lower[:, :, k] = v <= q05
    upper[:, :, k] = v <= q95
  return {'bulk': z, 'tail_lower': lower, 'tail_upper': upper, 'basic': w}


def ref_rank_ess(x, first, count, variants=VARIANTS):
  """{variant: [per dim: ref_ess's dict with 'm' and 'acov' added]}."""
  series = ref_series(x, first, count)
  out = {}
  for key in variants:
    s = series[key]
    per_dim = []
    for k in range(s.shape[2]):
      m, a = ref_acov(s[:, :, k], 0, count)
      r = ref_ess(m, a)
      r['m'], r['acov'] = m, a
      per_dim.append(r)
    out[key] = per_dim
  return out
