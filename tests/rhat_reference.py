"""split-R-hat and nested R-hat restated from their definitions in
np.longdouble, for the tests of probayes_amd/diag.py and of pbh_trace_rhat:
np.mean / np.var(ddof=1) on explicitly sliced halves and reshaped superchains
of a host trace x [N, T, d].  Shares no code with diag.py.  Also the measure
of agreement the tests use, and synthetic traces."""
import warnings

import numpy as np

LD = np.longdouble
EPS = float(np.finfo(float).eps)


def _quiet(fn):
  def run(*a, **k):
    with warnings.catch_warnings(), np.errstate(all='ignore'):
      warnings.simplefilter('ignore')
      return fn(*a, **k)
  return run


@_quiet
def ref_moments(x, first, count):
  """[6, N, d] longdouble: mean, variance (ddof 1) of the first half, of the
  second half, of the window."""
  w = np.asarray(x, LD)[:, first:first + count, :]
  h = count // 2
  a, b = w[:, :h, :], w[:, count - h:, :]
  return np.stack([a.mean(axis=1), a.var(axis=1, ddof=1),
                   b.mean(axis=1), b.var(axis=1, ddof=1),
                   w.mean(axis=1), w.var(axis=1, ddof=1)])


@_quiet
def ref_split(x, first, count):
  """[d] longdouble."""
  w = np.asarray(x, LD)[:, first:first + count, :]
  h = count // 2
  halves = np.concatenate([w[:, :h, :], w[:, count - h:, :]], axis=0)   # [2N, h, d]
  m = halves.mean(axis=1)
  s2 = halves.var(axis=1, ddof=1)
  W = s2.mean(axis=0)
  B_over_h = m.var(axis=0, ddof=1)
  return np.sqrt((LD(h - 1) / LD(h) * W + B_over_h) / W)


@_quiet
def ref_nested(x, first, count, group):
  """[d] longdouble."""
  w = np.asarray(x, LD)[:, first:first + count, :]
  n, _, d = w.shape
  m = w.mean(axis=1).reshape(n // group, group, d)
  s2 = w.var(axis=1, ddof=1).reshape(n // group, group, d)
  mu = m.mean(axis=1)
  B = m.var(axis=1, ddof=1) if group > 1 else np.zeros_like(mu)
  W = s2.mean(axis=1)
  return np.sqrt(LD(1) + mu.var(axis=0, ddof=1) / (B + W).mean(axis=0))


def rel_dist(got, ref):
  """The largest relative distance |got - ref| / |ref| over the arrays.  Equal
  values are at distance 0: the same number (0 and 0 too), the same infinity,
  NaN and NaN.  Anything else that has no finite quotient is at distance inf
  (a number against NaN, a nonzero against 0)."""
  got, ref = np.asarray(got, LD), np.asarray(ref, LD)
  assert got.shape == ref.shape, (got.shape, ref.shape)
  same = (got == ref) | (np.isnan(got) & np.isnan(ref))
  with np.errstate(all='ignore'):
    r = np.abs(got - ref) / np.abs(ref)
  r = np.where(same, LD(0), np.where(np.isnan(r), LD(np.inf), r))
  return float(r.max()) if r.size else 0.


def device_bound(host, ref):
  """What the device may differ from the longdouble reference by, relatively:
  64 eps, or 32 times the distance of diag.py's own fp64 result from it -- the
  margin for the device's sequential record-order sums against NumPy's."""
  return max(64 * EPS, 32 * rel_dist(host, ref))


def ar1_with_repeats(n, t, d, seed, rho=0.6, hold=0.3, loc=0., sd=1.):
  """[n, t, d]: stationary AR(1) chains (marginal loc, sd) in which a record
  repeats its predecessor with probability `hold`, as a Metropolis chain does
  after a rejection."""
  rng = np.random.RandomState(seed)
  z = rng.normal(size=(n, t, d))
  keep = rng.uniform(size=(n, t, d)) < hold
  x = np.empty((n, t, d))
  x[:, 0] = z[:, 0]
  for i in range(1, t):
    step = rho * x[:, i - 1] + np.sqrt(1. - rho * rho) * z[:, i]
    x[:, i] = np.where(keep[:, i], x[:, i - 1], step)
  return loc + sd * x
