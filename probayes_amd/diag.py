"""Cross-chain convergence diagnostics, the host definition (NumPy only, no
GPU): split-R-hat (Gelman et al., BDA3; Vehtari et al. 2021, without rank
normalisation) and nested R-hat (Margossian et al. 2024).

Both need nothing of a chain but means and variances, so the work has two
parts.  chain_moments reduces a host trace [N, T, d] to six rows per chain and
dim; split_rhat and nested_rhat work from those rows only.  The engine does
the same on the device (pbh_trace_rhat, Engine.trace_rhat(stats=True) returns
the rows), and a multi-rank caller concatenates the rows of every rank in
global chain order (axis 1) and calls the same two functions.

The values are the IEEE results of the formulas with no special cases: all
chains constant and equal give NaN (0/0), constant but different +inf, and a
NaN record propagates.

pooled_quantile is the definition of the posterior quantiles pooled over every
chain and record (pbh_trace_quantile_pooled, Engine.trace_quantile_pooled).

average_ranks, normal_scores and rank_rhat are the definition of the
rank-normalised and the folded split-R-hat (Vehtari et al. 2021;
pbh_trace_rhat_rank, Engine.trace_rhat_rank): the ranks of every draw of a dim
pooled over chains and records, their normal scores, and split_rhat of those.

split_chain_acov, multi_chain_ess and rank_ess are the definition of the bulk-
and tail-ESS of the same paper (pbh_trace_ess_rank, Engine.trace_ess_rank):
the autocovariance averaged over the split chains, and Stan's estimator of the
effective sample size from it.

pointwise_stats and waic are the definition of the pointwise log-likelihood
reduction (pbh_trace_pointwise, Engine.trace_pointwise): per observation the
log-sum-exp, the mean and the variance over the draws of its term, and lppd,
p_waic and WAIC from those (Watanabe 2010; Vehtari, Gelman & Gabry 2017).

pointwise_tail, gpd_fit, psis_loo_from_tail and psis_loo are the definition of
PSIS-LOO, leave-one-out by Pareto-smoothed importance sampling (Vehtari,
Gelman & Gabry 2017; Vehtari et al. 2024; the generalised-Pareto fit is Zhang &
Stephens 2009): per observation the smallest terms and the log-sum-exp of the
rest (pbh_trace_pointwise_tail, Engine.trace_pointwise_tail), and elpd_loo and
the Pareto shape from those.  compare_elpd is the difference of two models'
pointwise rows, WAIC's or LOO's, with its standard error.

pooled_cov and pooled_cov_finish are the definition of the posterior covariance
and correlation pooled over chains and records (pbh_trace_cov, Engine.
trace_cov), and proposal_cov turns such a matrix into the covariance of a
random-walk proposal (Sampler.trace_tran, for RF.set_tran).

hist_bin, pooled_hist and pooled_hist2d are the definition of the posterior
histograms pooled over chains and records (pbh_trace_hist, pbh_trace_hist2d,
Engine.trace_hist, Engine.trace_hist2d): np.histogram's and np.histogram2d's
counts.  hist_edges forms the edges from (bins, range) as np.histogram does,
hist_density and hist2d_density divide the counts as density=True does
(Sampler.trace_hist, trace_hist2d, trace_corner).
"""
import math

import numpy as np

ROWS = ('mean_first', 'var_first', 'mean_second', 'var_second', 'mean', 'var')


def _mean_var(v, shift, n):
  """Mean and variance (ddof 1) along axis 1 of shift + v from the sums of v
  and of v * v: (S S / n cancels against Q only as far as the mean of v is
  large against its spread, and v is the record minus the window's first)."""
  s = v.sum(axis=1)
  q = (v * v).sum(axis=1)
  n = float(n)
  return shift + s / n, (q - s * s / n) / (n - 1.)


def chain_moments(x, first=0, count=None):
  """[6, N, d] from a host trace x [N, T, d] over records [first, first +
  count): per chain and dim the mean and the variance (ddof 1) of the first
  half [first, first + h), of the second half [first + count - h, first +
  count), h = count // 2, and of the whole window (rows: ROWS).  An odd count
  leaves the middle record out of both halves.  count >= 2; with count < 4 the
  half variances are 0/0."""
  x = np.asarray(x, float)
  if x.ndim != 3:
    raise ValueError('chain_moments: a trace [N, T, d], got shape {}'.format(x.shape))
  first = int(first)
  count = x.shape[1] - first if count is None else int(count)
  if first < 0 or count < 0 or first + count > x.shape[1]:
    raise ValueError('chain_moments: records [{}, {}) outside [0, {})'.format(
        first, first + count, x.shape[1]))
  if count < 2:
    raise ValueError('chain_moments: count = {}: a variance needs at least 2 '
                     'records'.format(count))
  h = count // 2
  w = x[:, first:first + count, :]
  shift = w[:, 0, :]
  v = w - shift[:, None, :]
  out = np.empty((6,) + shift.shape)
  with np.errstate(divide='ignore', invalid='ignore'):
    out[0], out[1] = _mean_var(v[:, :h], shift, h)
    out[2], out[3] = _mean_var(v[:, count - h:], shift, h)
    out[4], out[5] = _mean_var(v, shift, count)
  return out


def _var_of_means(m):
  """Variance (ddof 1) along axis 0: the mean first, then the squared
  deviations from it."""
  dev = m - m.mean(axis=0)
  return (dev * dev).sum(axis=0) / (m.shape[0] - 1.)


def split_rhat(moments, h):
  """[d]: split-R-hat from chain_moments' rows [6, N, d] with halves of h
  records.  Over the 2 N half chains with mean m_j and variance s2_j: W =
  mean_j s2_j, B/h = var_j m_j (ddof 1), sqrt(((h - 1) / h W + B/h) / W)."""
  moments = np.asarray(moments, float)
  h = int(h)
  if h < 2:
    raise ValueError('split_rhat: h = {}: at least 2 records in each half '
                     '(count >= 4)'.format(h))
  m = np.concatenate([moments[0], moments[2]], axis=0)
  s2 = np.concatenate([moments[1], moments[3]], axis=0)
  with np.errstate(divide='ignore', invalid='ignore'):
    w = s2.mean(axis=0)
    return np.sqrt(((h - 1.) / h * w + _var_of_means(m)) / w)


def nested_rhat(moments, count, group):
  """[d]: nested R-hat from chain_moments' rows [6, N, d] of a window of
  count records, with superchains of `group` consecutive chains (chain c
  belongs to superchain c // group).  Per superchain mu_k = mean_c m_c, B_k =
  var_c m_c (ddof 1; 0 at group = 1), W_k = mean_c s2_c; the result is sqrt(1 +
  var_k mu_k / mean_k (B_k + W_k)), var_k at ddof 1."""
  moments = np.asarray(moments, float)
  count, group = int(count), int(group)
  n, d = moments.shape[1:]
  if count < 2:
    raise ValueError('nested_rhat: count = {}: a variance needs at least 2 '
                     'records'.format(count))
  if group < 1:
    raise ValueError('nested_rhat: group = {}: at least 1 chain per '
                     'superchain'.format(group))
  if n % group:
    raise ValueError('nested_rhat: group = {} does not divide the {} '
                     'chains'.format(group, n))
  if n // group < 2:
    raise ValueError('nested_rhat: group = {} leaves {} superchain of {} chains: '
                     'at least 2'.format(group, n // group, n))
  m = moments[4].reshape(n // group, group, d)
  s2 = moments[5].reshape(n // group, group, d)
  with np.errstate(divide='ignore', invalid='ignore'):
    mu = m.mean(axis=1)
    if group > 1:
      dev = m - mu[:, None, :]
      b = (dev * dev).sum(axis=1) / (group - 1.)
    else:
      b = np.zeros_like(mu)
    bw = b + s2.mean(axis=1)
    return np.sqrt(1. + _var_of_means(mu) / bw.mean(axis=0))


def pooled_quantile(x, q, first=0, count=None):
  """[nq, d]: the quantiles q of a host trace x [N, T, d] over records [first,
  first + count), pooled over every chain and record, per dim.  With s the M =
  N count values of a dim sorted ascending: vi = (M - 1) q, lo = floor(vi), hi
  = min(lo + 1, M - 1), g = vi - lo, a = s[lo], b = s[hi]; the result is b - (b
  - a) (1 - g) if g >= 0.5, else a + (b - a) g -- np.quantile's default method,
  written out.  A dim that holds a NaN gives NaN for every q; there are no
  other special cases (a = b = inf gives inf - inf = NaN), and -0.0 and +0.0
  are one value."""
  x = np.asarray(x, float)
  if x.ndim != 3:
    raise ValueError('pooled_quantile: a trace [N, T, d], got shape {}'.format(x.shape))
  first = int(first)
  count = x.shape[1] - first if count is None else int(count)
  if count < 1:
    raise ValueError('pooled_quantile: count = {}: at least 1 record'.format(count))
  if first < 0 or first + count > x.shape[1]:
    raise ValueError('pooled_quantile: records [{}, {}) outside [0, {})'.format(
        first, first + count, x.shape[1]))
  q = np.atleast_1d(np.asarray(q, float)).ravel()
  if q.size == 0:
    raise ValueError('pooled_quantile: no quantile given')
  if not np.all((q >= 0.) & (q <= 1.)):   # (a NaN fails both comparisons)
    raise ValueError('pooled_quantile: every q in [0, 1], got {}'.format(q))
  m = x.shape[0] * count
  if m < 1:
    raise ValueError('pooled_quantile: a trace without chains')
  vi = (m - 1.) * q
  fl = np.floor(vi)
  lo = np.minimum(fl.astype(np.int64), m - 1)
  hi = np.minimum(lo + 1, m - 1)
  g = vi - fl
  out = np.empty((q.size, x.shape[2]))
  for k in range(x.shape[2]):   # a dim at a time: one contiguous copy to sort
    s = np.sort(x[:, first:first + count, k], axis=None)   # NaN last
    with np.errstate(invalid='ignore', over='ignore'):
      a, b = s[lo], s[hi]
      diff = b - a
      out[:, k] = np.where(g >= 0.5, b - diff * (1. - g), a + diff * g)
    if np.isnan(s[-1]):
      out[:, k] = np.nan
  return out


def _window(what, x, first, count):
  x = np.asarray(x, float)
  if x.ndim != 3:
    raise ValueError('{}: a trace [N, T, d], got shape {}'.format(what, x.shape))
  first = int(first)
  count = x.shape[1] - first if count is None else int(count)
  if first < 0 or count < 0 or first + count > x.shape[1]:
    raise ValueError('{}: records [{}, {}) outside [0, {})'.format(
        what, first, first + count, x.shape[1]))
  return x, first, count


def average_ranks(x, first=0, count=None, fold=False):
  """[N, count, d]: per dim, the 1-based rank of every value of a host trace x
  [N, T, d] over records [first, first + count) among the M = N count values of
  the dim pooled over chains and records.  Ties take the mean of their ranks
  (a multiple of 1/2, exact in fp64); -0.0 and +0.0 are one value.  fold=True
  ranks abs(x - med_k) instead, med_k = pooled_quantile(x, [.5], first, count)
  [0, k].  A dim that holds a NaN -- after folding also a NaN median or an inf
  - inf -- gives NaN for every rank of the dim."""
  x, first, count = _window('average_ranks', x, first, count)
  if count < 1 or x.shape[0] < 1:
    raise ValueError('average_ranks: count = {}: at least 1 record of at least 1 '
                     'chain'.format(count))
  w = x[:, first:first + count, :]
  if fold:
    med = pooled_quantile(x, [.5], first, count)[0]
    with np.errstate(invalid='ignore'):
      w = np.abs(w - med)
  n, _, d = w.shape
  m = n * count
  out = np.empty((n, count, d))
  for k in range(d):   # a dim at a time: one contiguous copy to sort
    v = w[:, :, k].ravel()
    if np.isnan(v).any():
      out[:, :, k] = np.nan
      continue
    order = np.argsort(v, kind='stable')
    s = v[order]
    head = np.ones(m, bool)
    head[1:] = s[1:] != s[:-1]   # (-0.0 == +0.0)
    starts = np.flatnonzero(head)
    ends = np.append(starts[1:], m)
    run = np.cumsum(head) - 1
    r = np.empty(m)
    r[order] = ((starts + ends + 1) * 0.5)[run]
    out[:, :, k] = r.reshape(n, count)
  return out


# Wichura's AS241, PPND16: the coefficients of the three rational
# approximations, highest power first, as CPython's statistics module lists
# them.
_A = (2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4,
      4.5921953931549871457e+4, 1.3731693765509461125e+4, 1.9715909503065514427e+3,
      1.3314166789178437745e+2, 3.3871328727963666080e+0)
_B = (5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4,
      2.1213794301586595867e+4, 5.3941960214247511077e+3, 6.8718700749205790830e+2,
      4.2313330701600911252e+1, 1.0)
_C = (7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1,
      1.27045825245236838258e+0, 3.64784832476320460504e+0, 5.76949722146069140550e+0,
      4.63033784615654529590e+0, 1.42343711074968357734e+0)
_D = (1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2,
      1.48103976427480074590e-1, 6.89767334985100004550e-1, 1.67638483018380384940e+0,
      2.05319162663775882187e+0, 1.0)
_E = (2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3,
      2.65321895265761230930e-2, 2.96560571828504891230e-1, 1.78482653991729133580e+0,
      5.46378491116411436990e+0, 6.65790464350110377720e+0)
_F = (2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5,
      7.86869131145613259100e-4, 1.48753612908506148525e-2, 1.36929880922735805310e-1,
      5.99832206555887937690e-1, 1.0)


def _horner(c, r):
  acc = c[0] * r + c[1]
  for ci in c[2:]:
    acc = acc * r + ci
  return acc


def _ndtri(p):
  """The standard normal quantile of p in (0, 1), elementwise: AS241 PPND16 in
  fp64 in exactly the operation order of CPython's statistics.NormalDist.inv_cdf
  (mu 0, sigma 1).  Three branches: |p - 1/2| <= 0.425 (no libm call), r =
  sqrt(-log(min(p, 1 - p))) <= 5, and r > 5.  A NaN gives NaN."""
  p = np.asarray(p, float)
  q = p - 0.5
  out = np.full(p.shape, np.nan)
  with np.errstate(all='ignore'):
    mid = np.abs(q) <= 0.425
    r = 0.180625 - q[mid] * q[mid]
    out[mid] = _horner(_A, r) * q[mid] / _horner(_B, r)
    tail = ~mid & ~np.isnan(q)
    qt = q[tail]
    r = np.sqrt(-np.log(np.where(qt <= 0., p[tail], 1. - p[tail])))
    near = r <= 5.
    x = np.empty(r.shape)
    rn = r[near] - 1.6
    x[near] = _horner(_C, rn) / _horner(_D, rn)
    rf = r[~near] - 5.
    x[~near] = _horner(_E, rf) / _horner(_F, rf)
    out[tail] = np.where(qt < 0., -x, x)
  return out


def normal_scores(r, M):
  """ndtri((r - 0.375) / (M + 0.25)) of the 1-based average ranks r among M
  values, elementwise (Blom's offsets, as Vehtari et al. 2021 take them);
  ndtri is AS241 as _ndtri writes it out.  A NaN rank gives a NaN score."""
  r = np.asarray(r, float)
  return _ndtri((r - 0.375) / (float(M) + 0.25))


def rank_rhat(x, first=0, count=None):
  """{'bulk': [d], 'folded': [d], 'rhat': [d]}: the rank-normalised split-R-hat
  of a host trace x [N, T, d] over records [first, first + count).  bulk is
  split_rhat(chain_moments(z), count // 2) of the scores z = normal_scores(
  average_ranks(x, first, count), N count); folded the same of the folded
  ranks; rhat = np.maximum of the two, so a NaN propagates.  count >= 4.  No
  other special cases: constant chains give W = 0 and so inf or NaN, as
  split_rhat does."""
  x, first, count = _window('rank_rhat', x, first, count)
  if count < 4:
    raise ValueError('rank_rhat: count = {}: split R-hat needs at least 4 records '
                     '(two in each half)'.format(count))
  m = x.shape[0] * count
  res = {}
  for key, fold in (('bulk', False), ('folded', True)):
    z = normal_scores(average_ranks(x, first, count, fold), m)
    res[key] = split_rhat(chain_moments(z), count // 2)
  res['rhat'] = np.maximum(res['bulk'], res['folded'])
  return res


def _seq_sum(v):
  """The sum of a 1-D array added in index order (np.sum adds pairwise): the
  order pbh_trace_host.cpp's multi_chain_ess adds in."""
  return np.cumsum(v)[-1] if v.size else 0.


def split_chain_acov(y, first=0, count=None):
  """(m [C], A [h]) of a series y [N, T] of one dim over records [first, first +
  count), h = count // 2: the C = 2 N split chains are the first halves [first,
  first + h) of chains 0 .. N - 1, then the second halves [first + count - h,
  first + count) -- the order split_rhat concatenates in; an odd count leaves
  the middle record out.  Per split chain j the mean m_j and the biased
  autocovariance a_j[t] = (1 / h) sum_{i = 0}^{h - 1 - t} (y_i - m_j) (y_{i + t} -
  m_j), t = 0 .. h - 1; A[t] = mean_j a_j[t].
  In fp64: m is chain_moments' mean_first and mean_second.  The sums of
  products are linear in the power spectrum, so the split chains, each centred
  by its first record plus the mean of its differences from it (a constant
  chain is centred to exact zeros), are zero-padded to a power of two >= 2 h
  and transformed, the power spectra summed over j, and one inverse transform
  gives h C A[t].  count >= 2.  A NaN record gives NaN for every A[t]."""
  y = np.asarray(y, float)
  if y.ndim != 2:
    raise ValueError('split_chain_acov: a series [N, T], got shape {}'.format(y.shape))
  x, first, count = _window('split_chain_acov', y[:, :, None], first, count)
  if count < 2 or x.shape[0] < 1:
    raise ValueError('split_chain_acov: count = {}: at least 2 records of at least 1 '
                     'chain'.format(count))
  h = count // 2
  mom = chain_moments(x, first, count)
  m = np.concatenate([mom[0, :, 0], mom[2, :, 0]])
  w = y[:, first:first + count]
  halves = np.concatenate([w[:, :h], w[:, count - h:]], axis=0)   # [C, h]
  c_all = halves.shape[0]
  size = 1
  while size < 2 * h:
    size *= 2
  power = np.zeros(size // 2 + 1)
  with np.errstate(all='ignore'):
    for j0 in range(0, c_all, 4096):   # (a block of split chains at a time)
      blk = halves[j0:j0 + 4096]
      v = blk - blk[:, :1]
      v = v - (v.sum(axis=1) / float(h))[:, None]
      f = np.fft.rfft(v, size, axis=1)
      power += (f.real * f.real + f.imag * f.imag).sum(axis=0)
    acov = np.fft.irfft(power, size)[:h] / (float(h) * float(c_all))
  return m, acov


def multi_chain_ess(m, A, C, h):
  """The effective sample size of C split chains of h records each from their
  means m [C] and their mean autocovariance A [h] (split_chain_acov): Stan's
  estimator (Vehtari et al. 2021 section 3.2; Geyer's initial positive and
  monotone sequences), every sum added in index order:
    mean_var = A[0] h / (h - 1);  var_plus = A[0] + var_j m_j (ddof 1: the mean
    of m - m[0] first, then the squared deviations of m - m[0] from it, so
    that equal means have variance 0 exactly);
    rho[t] = 1 - (mean_var - A[t]) / var_plus, rho[0] = 1;
    P_k = rho[2 k] + rho[2 k + 1], k = 0 .. K - 1, K = h // 2;
    k* = the first k in 1 .. K - 1 for which P_k > 0 is false (a NaN stops the
    scan), K if there is none;
    P'_0 = P_0, P'_k = np.minimum(P'_{k - 1}, P_k) for k < k* (a NaN propagates);
    tau = -1 + 2 sum_{k < k*} P'_k, plus rho[2 k*] if k* < K and rho[2 k*] > 0;
    tau = np.maximum(tau, 1 / log10(C h));  ESS = C h / tau.
  There are no other special cases: all chains constant and equal give NaN
  (0 / 0), a NaN record gives NaN, constant chains that differ a finite value
  (rho = 1 throughout).  C >= 2, h >= 2."""
  m = np.asarray(m, float).ravel()
  A = np.asarray(A, float).ravel()
  C, h = int(C), int(h)
  if C < 2 or h < 2 or m.size != C or A.size != h:
    raise ValueError('multi_chain_ess: C = {} (>= 2) means and h = {} (>= 2) lags, got {} '
                     'and {}'.format(C, h, m.size, A.size))
  with np.errstate(all='ignore'):
    mean_var = A[0] * float(h) / (h - 1.)
    dev = m - m[0]
    dev = dev - _seq_sum(dev) / float(C)
    var_plus = A[0] + _seq_sum(dev * dev) / (C - 1.)
    rho = 1. - (mean_var - A) / var_plus
    rho[0] = 1.
    K = h // 2
    P = rho[0:2 * K:2] + rho[1:2 * K:2]
    bad = np.flatnonzero(~(P[1:] > 0.))
    ks = int(bad[0]) + 1 if bad.size else K
    mono = np.minimum.accumulate(P[:ks])
    tau = -1. + 2. * _seq_sum(mono)
    if ks < K and rho[2 * ks] > 0.:
      tau = tau + rho[2 * ks]
    tau = np.maximum(tau, 1. / math.log10(float(C) * float(h)))
    return float(C) * float(h) / tau


def rank_ess(x, first=0, count=None):
  """{'bulk': [d], 'tail': [d], 'tail_lower': [d], 'tail_upper': [d], 'basic':
  [d]}: the effective sample sizes of a host trace x [N, T, d] over records
  [first, first + count), across the 2 N split chains (Vehtari et al. 2021).
  Each is multi_chain_ess(*split_chain_acov(s), 2 N, count // 2) of a series s
  per dim: bulk of the scores normal_scores(average_ranks(x, first, count), N
  count); tail_lower and tail_upper of the indicators x <= q05 and x <= q95 as
  0. / 1. (not rank-normalised), q = pooled_quantile(x, [.05, .95], first,
  count); tail = np.minimum of the two; basic of the values themselves.  count
  >= 4.  A dim that holds a NaN gives NaN everywhere (its indicators are NaN)."""
  x, first, count = _window('rank_ess', x, first, count)
  if count < 4:
    raise ValueError('rank_ess: count = {}: the split chains need at least 4 records '
                     '(two in each half)'.format(count))
  n, _, d = x.shape
  if n < 1:
    raise ValueError('rank_ess: a trace without chains')
  h, c_all = count // 2, 2 * n
  w = x[:, first:first + count, :]
  z = normal_scores(average_ranks(x, first, count), n * count)
  q = pooled_quantile(x, [.05, .95], first, count)
  res = {key: np.empty(d) for key in ('bulk', 'tail_lower', 'tail_upper', 'basic')}
  for k in range(d):
    series = {'bulk': z[:, :, k], 'basic': w[:, :, k]}
    for key, thr in (('tail_lower', q[0, k]), ('tail_upper', q[1, k])):
      with np.errstate(invalid='ignore'):
        series[key] = np.where(np.isnan(thr), np.nan, (w[:, :, k] <= thr).astype(float))
    for key, s in series.items():
      m, acov = split_chain_acov(s)
      res[key][k] = multi_chain_ess(m, acov, c_all, h)
  res['tail'] = np.minimum(res['tail_lower'], res['tail_upper'])
  return res


def pointwise_stats(T):
  """(lse [n], mean [n], var [n]) of the terms T [S, n] over the S >= 2 draws,
  per observation j.  lse_j = log sum_s exp T[s, j] with scipy.special.
  logsumexp's treatment of infinities: shifted by the column's maximum, taken
  as 0 when that is not finite, so a column that is all -inf gives -inf, one
  with a +inf gives +inf, and any NaN gives NaN.  mean_j is the mean and var_j
  the sample variance (ddof 1) by two passes: the deviations from the mean,
  then the mean of their squares over S - 1."""
  T = np.asarray(T, float)
  if T.ndim != 2 or T.shape[0] < 2:
    raise ValueError('pointwise_stats: terms [S >= 2, n], got shape {}'.format(T.shape))
  S = T.shape[0]
  with np.errstate(all='ignore'):
    top = T.max(axis=0)
    top = np.where(np.isfinite(top), top, 0.)
    lse = np.log(np.exp(T - top).sum(axis=0)) + top
    mean = T.sum(axis=0) / S
    dev = T - mean
    var = (dev * dev).sum(axis=0) / (S - 1.)
  return lse, mean, var


def waic(lse, mean, var, S):
  """WAIC from pointwise_stats' rows over S draws (Vehtari, Gelman & Gabry
  2017): lppd_i = lse - log S, p_waic_i = var, elpd_i = lppd_i - p_waic_i per
  observation; lppd, p_waic and elpd_waic their sums; se = sqrt(n var(elpd_i))
  (np.var, ddof 0); waic = -2 elpd_waic.  mean is not read: it is there for the
  call waic(*pointwise_stats(T), S)."""
  lse, var = np.asarray(lse, float), np.asarray(var, float)
  with np.errstate(all='ignore'):
    lppd_i = lse - math.log(S)
    p_waic_i = var
    elpd_i = lppd_i - p_waic_i
    elpd = float(elpd_i.sum())
    return {'lppd_i': lppd_i, 'p_waic_i': p_waic_i, 'elpd_i': elpd_i,
            'lppd': float(lppd_i.sum()), 'p_waic': float(p_waic_i.sum()),
            'elpd_waic': elpd, 'se': float(np.sqrt(lse.size * np.var(elpd_i))),
            'waic': -2. * elpd}


def pointwise_tail(T, k):
  """(tail [n, k], rest_lse [n]) of the terms T [S, n], 1 <= k < S: per
  observation j the k smallest terms, ascending, and log sum exp(-T[s, j]) over
  the other S - k draws.  The order is that of the terms' 64-bit images: either
  zero is +0.0, and NaN, one quiet NaN for every payload, comes last, so a tail
  holds a NaN only when fewer than k terms are not NaN.  rest_lse has
  pointwise_stats' conventions: shifted by the maximum, taken as 0 when that is
  not finite, so -inf when every other term is +inf, +inf with a -inf among
  them, NaN with a NaN."""
  T = np.asarray(T, float)
  k = int(k)
  if T.ndim != 2 or not 1 <= k < T.shape[0]:
    raise ValueError('pointwise_tail: terms [S, n] and 1 <= k < S, got shape {} and k = {}'
                     .format(T.shape, k))
  with np.errstate(all='ignore'):
    t = np.sort(np.where(np.isnan(T), np.nan, T + 0.), axis=0)
    rest = -t[k:]
    top = rest.max(axis=0)
    top = np.where(np.isfinite(top), top, 0.)
    rest_lse = np.log(np.exp(rest - top).sum(axis=0)) + top
  return np.ascontiguousarray(t[:k].T), rest_lse


def gpd_fit(x):
  """(k, sigma) of the generalised Pareto distribution fitted to the ascending
  sample x >= 0, x[-1] > 0, of m exceedances: Zhang & Stephens' (2009)
  estimator, the posterior mean of theta = -k / sigma under their data-
  dependent prior on a grid of 30 + floor(sqrt(m)) points theta_j = 1 / x_m + (1
  - sqrt(M / (j - 1/2))) / (3 x*), x* the first-quartile element x[floor(m / 4
  + 1/2) - 1], weighted by the profile likelihood L(theta) = m (log(-theta /
  k(theta)) - k(theta) - 1), k(theta) = mean log1p(-theta x); then k at the
  mean theta, sigma = -k / theta, and k drawn towards 1/2 by the weakly
  informative prior of Vehtari et al. (2024), k <- (m k + 5) / (m + 10).
  x -> c x leaves k and sigma / c unchanged."""
  x = np.asarray(x, float)
  m = x.size
  M = 30 + int(math.floor(math.sqrt(m)))
  xstar = x[int(math.floor(m / 4. + 0.5)) - 1]
  j = np.arange(1, M + 1, dtype=float)
  theta = 1. / x[-1] + (1. - np.sqrt(M / (j - 0.5))) / (3. * xstar)
  kj = np.log1p(-theta[:, None] * x[None, :]).mean(axis=1)
  L = m * (np.log(-theta / kj) - kj - 1.)
  with np.errstate(over='ignore'):    # (a point far below the best weighs 1 / inf = 0)
    w = 1. / np.exp(L[None, :] - L[:, None]).sum(axis=1)
  th = float((theta * w).sum())
  k = float(np.log1p(-th * x).mean())
  sigma = -k / th
  return (m * k + 5.) / (m + 10.), sigma


def psis_tail_length(S):
  """m = min(floor(S / 5), ceil(3 sqrt(S))), the draws PSIS smooths; m >= 5, so
  S >= 25, or ValueError."""
  S = int(S)
  m = min(S // 5, int(math.ceil(3. * math.sqrt(S)))) if S > 0 else 0
  if m < 5:
    raise ValueError('psis: S = {} draws leave a tail of {}: at least 5, S >= 25'.format(S, m))
  return m


def _lse(v):
  """log sum exp of a vector, pointwise_stats' conventions"""
  top = v.max()
  top = top if np.isfinite(top) else 0.
  return float(np.log(np.exp(v - top).sum()) + top)


def psis_loo_from_tail(tail, rest_lse, S, lse=None):
  """PSIS-LOO per observation from pointwise_tail(T, m + 1) of its S draws, m =
  psis_tail_length(S): {'elpd_loo_i': [n], 'pareto_k': [n]}.  Write a sorted
  tail t_0 <= .. <= t_m.  The importance log-ratios are -T: the cutoff is -t_m,
  the m tail ratios lw_i = -t_i, i < m, all shifted by -t_0 so that the largest
  is 0.  gpd_fit on exp(lw) - exp(cutoff), ascending, gives (k, sigma); the r-th
  smallest tail ratio is replaced by log(sigma expm1(-k log1p(-p_r)) / k +
  exp(cutoff)), p_r = (r - 1/2) / m, truncated at the raw maximum.  log sum w
  is the log-sum-exp of rest_lse, the cutoff and the smoothed ratios; sum w p =
  (S - m) + sum_r exp(smoothed_r + t_(r)), a draw outside the tail giving
  exactly 1; elpd_loo_i = log sum w p - log sum w, pareto_k = k.
  One rule for the degenerate rows.  A NaN in the tail or in rest_lse makes the
  row NaN, both values.  Otherwise an infinite term in the tail, an infinite
  rest_lse, or a zero at the fit's first-quartile element (the tail is tied
  with the cutoff that far) gives pareto_k = +inf and no smoothing: elpd_loo_i
  = log S - log sum w over the raw ratios.
  With lse [n], pointwise_stats' log-sum-exp of the same terms, the summary is
  added: 'p_loo_i' = lppd_i - elpd_loo_i with lppd_i = lse - log S; 'elpd_loo'
  and 'p_loo', the sums; 'se' = sqrt(n var(elpd_loo_i)) (np.var, ddof 0);
  'looic' = -2 elpd_loo; 'n_bad_k', the observations whose pareto_k is not <=
  min(1 - 1 / log10(S), 0.7), where neither estimate can be trusted."""
  tail, rest_lse = np.asarray(tail, float), np.asarray(rest_lse, float)
  S = int(S)
  m = psis_tail_length(S)
  if tail.ndim != 2 or tail.shape[1] != m + 1 or rest_lse.shape != tail.shape[:1]:
    raise ValueError('psis_loo_from_tail: tail [n, {}] and rest_lse [n] for S = {}, got {} and {}'
                     .format(m + 1, S, tail.shape, rest_lse.shape))
  n = tail.shape[0]
  elpd, khat = np.empty(n), np.empty(n)
  p = (np.arange(1, m + 1) - 0.5) / m
  quartile = int(math.floor(m / 4. + 0.5)) - 1
  with np.errstate(all='ignore'):
    for j in range(n):
      t, rest = tail[j], float(rest_lse[j])
      if np.isnan(t).any() or np.isnan(rest):
        elpd[j] = khat[j] = np.nan
        continue
      shift = t[0]
      lw = (shift - t[:m])[::-1]          # ascending, the largest 0
      cut = shift - t[m]
      x = np.exp(lw) - np.exp(cut)
      if not (np.isfinite(t).all() and np.isfinite(rest)) or not x[quartile] > 0.:
        khat[j] = np.inf
        elpd[j] = math.log(S) - _lse(np.concatenate(([rest], -t)))
        continue
      k, sigma = gpd_fit(x)
      q = -np.log1p(-p) * sigma if k == 0. else sigma * np.expm1(-k * np.log1p(-p)) / k
      smooth = np.minimum(np.log(q + np.exp(cut)), 0.)
      log_sum_w = _lse(np.concatenate(([rest, -t[m]], smooth - shift)))
      sum_wp = (S - m) + float(np.exp((smooth - shift) + t[:m][::-1]).sum())
      khat[j] = k
      elpd[j] = math.log(sum_wp) - log_sum_w
    res = {'elpd_loo_i': elpd, 'pareto_k': khat}
    if lse is not None:
      lppd_i = np.asarray(lse, float) - math.log(S)
      total = float(elpd.sum())
      bad = min(1. - 1. / math.log10(S), 0.7)
      res.update({'p_loo_i': lppd_i - elpd, 'elpd_loo': total,
                  'p_loo': float((lppd_i - elpd).sum()),
                  'se': float(np.sqrt(n * np.var(elpd))), 'looic': -2. * total,
                  'n_bad_k': int(np.count_nonzero(~(khat <= bad)))})
  return res


def psis_loo(T):
  """PSIS-LOO of the terms T [S, n], the pointwise log-likelihood of S draws:
  pointwise_tail(T, m + 1), then psis_loo_from_tail with pointwise_stats' lse --
  the rows 'elpd_loo_i', 'pareto_k', 'p_loo_i' and 'elpd_loo', 'p_loo', 'se',
  'looic', 'n_bad_k'."""
  T = np.asarray(T, float)
  if T.ndim != 2:
    raise ValueError('psis_loo: terms [S, n], got shape {}'.format(T.shape))
  S = T.shape[0]
  tail, rest_lse = pointwise_tail(T, psis_tail_length(S) + 1)
  with np.errstate(all='ignore'):
    lse = pointwise_stats(T)[0]
  return psis_loo_from_tail(tail, rest_lse, S, lse)


def compare_elpd(a_i, b_i):
  """(elpd_diff, se) of two models on the same n observations from their
  pointwise elpd rows, waic's 'elpd_i' or psis_loo's 'elpd_loo_i': the sum of
  a_i - b_i -- positive where a predicts better -- and sqrt(n var(a_i - b_i))
  (np.var, ddof 0), the standard error of that sum."""
  a_i, b_i = np.asarray(a_i, float), np.asarray(b_i, float)
  if a_i.ndim != 1 or a_i.shape != b_i.shape:
    raise ValueError('compare_elpd: two rows [n], got {} and {}'.format(a_i.shape, b_i.shape))
  diff = a_i - b_i
  return float(diff.sum()), float(np.sqrt(diff.size * np.var(diff)))


def pooled_cov_finish(K, S, P, M):
  """{'mean': [d], 'cov': [d, d], 'corr': [d, d]} from the sums over M draws of
  v = x - K: S [d] = sum v_a and P, the upper triangle of sum v_a v_b packed row
  by row (np.triu_indices order; a full [d, d] is read above its diagonal).
  mean = K + S / M; cov_ab = (P_ab - S_a S_b / M) / (M - 1) for a <= b and
  mirrored; corr_ab = cov_ab / sqrt(cov_aa cov_bb), the diagonal included (1,
  or NaN for a dim that never moves).  Sums of several ranks taken about one K
  add before this step."""
  K, S = np.asarray(K, float).ravel(), np.asarray(S, float).ravel()
  d = K.size
  P = np.asarray(P, float)
  ia, ib = np.triu_indices(d)
  if P.shape == (d, d) and d > 1:
    P = P[ia, ib]
  P = P.ravel()
  if S.size != d or P.size != d * (d + 1) // 2 or d < 1:
    raise ValueError('pooled_cov_finish: K [d], S [d] and P [d (d + 1) / 2], got {}, {} and '
                     '{}'.format(K.shape, S.shape, P.shape))
  if int(M) < 2:
    raise ValueError('pooled_cov_finish: M = {}: a covariance needs at least 2 '
                     'draws'.format(M))
  m = float(int(M))
  cov, corr = np.empty((d, d)), np.empty((d, d))
  with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
    mean = K + S / m
    tri = (P - S[ia] * S[ib] / m) / (m - 1.)
    cov[ia, ib] = tri
    cov[ib, ia] = tri
    var = np.diagonal(cov)
    r = tri / np.sqrt(var[ia] * var[ib])
    corr[ia, ib] = r
    corr[ib, ia] = r
  return {'mean': mean, 'cov': cov, 'corr': corr}


def pooled_cov(x, first=0, count=None):
  """{'mean': [d], 'cov': [d, d], 'corr': [d, d]}: the mean, the covariance
  (ddof 1) and the correlation of a host trace x [N, T, d] over records [first,
  first + count), pooled over every chain and record, M = N count draws.  The
  sums are taken of v = x - K, K the mean over chains of the window's first
  record: it lies within the cloud of draws, so S S / M cancels against P only
  mildly wherever the posterior lies (sums of raw products lose everything once
  the mean is large against the spread), and it costs no pass.  The values are
  the IEEE results of pooled_cov_finish's formulas with no special cases:
  constant and equal chains give cov exactly 0 and corr NaN, and a NaN record
  propagates.  count >= 1, M >= 2."""
  x, first, count = _window('pooled_cov', x, first, count)
  if count < 1:
    raise ValueError('pooled_cov: count = {}: at least 1 record'.format(count))
  m = x.shape[0] * count
  if m < 2:
    raise ValueError('pooled_cov: {} chain of {} record: a covariance needs at least 2 '
                     'draws'.format(x.shape[0], count))
  d = x.shape[2]
  w = x[:, first:first + count, :]
  with np.errstate(invalid='ignore', over='ignore'):
    K = w[:, 0, :].mean(axis=0)
    # [d, M], the draws contiguous: NumPy's pairwise sum runs along them
    v = np.ascontiguousarray((w - K).reshape(m, d).T)
    S = v.sum(axis=1)
    P = np.concatenate([(v[a:] * v[a]).sum(axis=1) for a in range(d)])
  return pooled_cov_finish(K, S, P, m)


def proposal_cov(cov, scale=None, eps=0.):
  """[d, d]: the covariance of a random-walk proposal from a posterior
  covariance: s (cov + eps mean(diag cov) I), s = 2.38^2 / d when scale is
  None (Haario et al. 2001; Roberts & Rosenthal 2001: the optimal scale of a
  Gaussian random walk on a Gaussian target) -- what RF.set_tran takes.  eps
  lifts a covariance estimated from few draws off singularity.  ValueError
  when the result is not a finite symmetric positive definite matrix (np.
  linalg.cholesky fails on it)."""
  cov = np.asarray(cov, float)
  if cov.ndim != 2 or cov.shape[0] != cov.shape[1] or cov.shape[0] < 1:
    raise ValueError('proposal_cov: a square matrix [d, d], got shape {}'.format(cov.shape))
  d = cov.shape[0]
  s = 2.38 ** 2 / d if scale is None else float(scale)
  with np.errstate(invalid='ignore', over='ignore'):
    out = s * (cov + float(eps) * np.mean(np.diagonal(cov)) * np.eye(d))
  if not np.all(np.isfinite(out)):
    raise ValueError('proposal_cov: the matrix has an entry that is not finite (a NaN or '
                     'infinite draw, or a scale that is not finite)')
  if not np.array_equal(out, out.T):
    raise ValueError('proposal_cov: the matrix is not symmetric')
  try:
    np.linalg.cholesky(out)
  except np.linalg.LinAlgError:
    raise ValueError('proposal_cov: the matrix is not positive definite (a variable that '
                     'never moved, variables that move as one, or fewer draws than '
                     'variables; eps > 0 lifts it)')
  return out


def _edges(what, edges):
  e = np.asarray(edges, float)
  if e.ndim != 1 or e.size < 2:
    raise ValueError('{}: edges [B + 1] with B >= 1, got shape {}'.format(what, e.shape))
  if not np.all(np.isfinite(e)):
    raise ValueError('{}: an edge is not finite'.format(what))
  if not np.all(e[:-1] < e[1:]):
    raise ValueError('{}: the edges do not strictly increase'.format(what))
  return e


def hist_bin(x, edges):
  """The bin of every value of x among strictly increasing finite edges [B +
  1], an int64 array of x's shape: bin i holds edges[i] <= x < edges[i + 1], the
  last bin also x == edges[B]; -1 is below edges[0], -2 above edges[B], -3 a
  NaN.  Plain comparisons: -0.0 and +0.0 are one value, -inf is below and +inf
  above.  This is where np.histogram(x, edges), np.histogram(x, B, range=(lo,
  hi)) with edges = np.linspace(lo, hi, B + 1), and np.histogram2d with
  explicit edges count a value."""
  e = _edges('hist_bin', edges)
  x = np.asarray(x, float)
  nb = e.size - 1
  # the edges that are <= x, less one (a NaN sorts behind every edge)
  out = np.searchsorted(e, x, side='right').astype(np.int64) - 1
  out = np.where(x == e[nb], nb - 1, out)
  out = np.where(x < e[0], -1, out)
  out = np.where(x > e[nb], -2, out)
  return np.where(np.isnan(x), -3, out).astype(np.int64)


def _edge_list(what, edges, d):
  if len(edges) != d:
    raise ValueError('{}: {} edge arrays for {} dims (None skips a dim)'.format(
        what, len(edges), d))
  return [None if e is None else _edges(what, e) for e in edges]


def pooled_hist(x, edges, first=0, count=None):
  """{'counts': [int64 [B_k] or None per dim], 'outside': int64 [d, 3]}: the
  histograms of a host trace x [N, T, d] over records [first, first + count)
  pooled over every chain and record (pbh_trace_hist, Engine.trace_hist).
  edges: a list of d arrays, None for a dim to skip.  counts[k][i] is the number
  of draws with hist_bin(x_k, edges[k]) == i; outside[k] the numbers below,
  above and NaN (0 for a skipped dim), so that counts[k].sum() + outside[k].sum()
  == N count."""
  x, first, count = _window('pooled_hist', x, first, count)
  if count < 1:
    raise ValueError('pooled_hist: count = {}: at least 1 record'.format(count))
  d = x.shape[2]
  edges = _edge_list('pooled_hist', edges, d)
  if all(e is None for e in edges):
    raise ValueError('pooled_hist: every dim is skipped')
  w = x[:, first:first + count, :]
  counts, outside = [], np.zeros((d, 3), np.int64)
  for k, e in enumerate(edges):
    if e is None:
      counts.append(None)
      continue
    b = hist_bin(w[:, :, k].ravel(), e)
    counts.append(np.bincount(b[b >= 0], minlength=e.size - 1).astype(np.int64))
    outside[k] = [(b == -1).sum(), (b == -2).sum(), (b == -3).sum()]
  return {'counts': counts, 'outside': outside}


def pooled_hist2d(x, edges, pairs, first=0, count=None):
  """A list of int64 [B_a, B_b], one per (a, b) in pairs: H[i, j] counts the
  draws of a host trace x [N, T, d] over records [first, first + count), pooled
  over every chain and record, with hist_bin(x_a, edges[a]) == i and
  hist_bin(x_b, edges[b]) == j; a draw with either bin negative is dropped --
  np.histogram2d(x_a, x_b, bins=[edges[a], edges[b]]) (pbh_trace_hist2d, Engine.
  trace_hist2d).  a == b is allowed."""
  x, first, count = _window('pooled_hist2d', x, first, count)
  if count < 1:
    raise ValueError('pooled_hist2d: count = {}: at least 1 record'.format(count))
  d = x.shape[2]
  edges = _edge_list('pooled_hist2d', edges, d)
  if len(pairs) < 1:
    raise ValueError('pooled_hist2d: no pair')
  w = x[:, first:first + count, :]
  out = []
  for a, b in pairs:
    a, b = int(a), int(b)
    if not (0 <= a < d and 0 <= b < d) or edges[a] is None or edges[b] is None:
      raise ValueError('pooled_hist2d: pair ({}, {}) names a dim outside [0, {}) or one '
                       'without edges'.format(a, b, d))
    na, nb = edges[a].size - 1, edges[b].size - 1
    ia = hist_bin(w[:, :, a].ravel(), edges[a])
    ib = hist_bin(w[:, :, b].ravel(), edges[b])
    keep = (ia >= 0) & (ib >= 0)
    cells = np.bincount(ia[keep] * nb + ib[keep], minlength=na * nb)
    out.append(cells.astype(np.int64).reshape(na, nb))
  return out


def _hist_edges_one(what, bins, rng, minmax):
  """np.histogram's bin edges of one variable: bins an int (then rng (lo, hi),
  or minmax() -> (lo, hi) of the data) or an edge array (rng is not read)."""
  if np.ndim(bins) == 0:
    try:
      nb = int(bins)
      whole = nb == bins
    except (TypeError, ValueError):
      whole = False
    if not whole:
      raise TypeError('{}: bins = {!r} is neither a whole number nor an edge array'.format(
          what, bins))
    if nb < 1:
      raise ValueError('{}: bins = {}: at least 1'.format(what, nb))
    if rng is not None:
      lo, hi = (float(v) for v in rng)
      if lo > hi:
        raise ValueError('{}: range ({}, {}): max must be larger than min'.format(what, lo, hi))
      if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError('{}: range ({}, {}) is not finite'.format(what, lo, hi))
    else:
      lo, hi = (float(v) for v in minmax())
      if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError('{}: the values\' range [{}, {}] is not finite: give range=(lo, '
                         'hi)'.format(what, lo, hi))
    if lo == hi:
      lo, hi = lo - 0.5, hi + 0.5
    e = np.linspace(lo, hi, nb + 1)
    if not (np.all(np.isfinite(e)) and np.all(e[:-1] < e[1:])):
      raise ValueError('{}: {} bins over ({}, {}) do not give strictly increasing finite '
                       'edges'.format(what, nb, lo, hi))
    return e
  return _edges(what, bins)


def hist_edges(bins=10, range=None, names=None, minmax=None):
  """The bin edges np.histogram forms from (bins, range), without the data.
  One variable (names=None): bins is an int or an edge array, range (lo, hi) or
  None, and the result one float64 array.  With an int: the edges are
  np.linspace(lo, hi, bins + 1); lo == hi becomes lo - 0.5, hi + 0.5; with
  range=None, (lo, hi) = minmax(), the smallest and the largest value of the
  data, asked for only then.  An edge array is returned as float64; range is
  not read.  names=[...]: bins may also be {name: int or array} -- a name left
  out is skipped -- and range {name: (lo, hi)}; minmax() then returns {name:
  (lo, hi)} and is called at most once; the result is a list in the order of
  names, None for a skipped name.  ValueError as np.histogram: bins < 1, lo >
  hi, a range or a data range that is not finite; and for edges that are not
  finite or do not strictly increase (np.histogram takes equal edges; the
  device does not)."""
  what = 'hist_edges'
  if names is None:
    if isinstance(bins, dict) or isinstance(range, dict):
      raise ValueError('hist_edges: a dict of bins or ranges needs names')
    return _hist_edges_one(what, bins, range, minmax)
  names = list(names)
  for given in (bins, range):
    if isinstance(given, dict):
      unknown = [k for k in given if k not in names]
      if unknown:
        raise ValueError('hist_edges: {!r} is not one of the names {}'.format(unknown[0], names))
  found = {}

  def data_range(name):
    if not found:
      found.update(minmax())
    return found[name]

  out = []
  for name in names:
    if isinstance(bins, dict) and name not in bins:
      out.append(None)
      continue
    b = bins[name] if isinstance(bins, dict) else bins
    r = range.get(name) if isinstance(range, dict) else range
    out.append(_hist_edges_one('hist_edges ({})'.format(name), b, r,
                               lambda name=name: data_range(name)))
  return out


def hist_density(h, edges):
  """np.histogram's density=True from the counts: h / np.diff(edges) / h.sum(),
  in NumPy's operation order."""
  h = np.asarray(h)
  return h / np.diff(np.asarray(edges, float)) / h.sum()


def hist2d_density(h, xedges, yedges):
  """np.histogram2d's H from the counts [B_x, B_y]: float64, and with density
  divided by the bins' widths along x, then along y, then by the sum, in
  NumPy's operation order."""
  out = np.asarray(h).astype(float)
  s = out.sum()
  out = out / np.diff(np.asarray(xedges, float)).reshape(-1, 1)
  out = out / np.diff(np.asarray(yedges, float)).reshape(1, -1)
  out /= s
  return out
