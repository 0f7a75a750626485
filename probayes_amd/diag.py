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
"""
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
