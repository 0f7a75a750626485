"""The pooled posterior covariance restated from its definition in
np.longdouble, for the tests of probayes_amd/diag.py pooled_cov and of
pbh_trace_cov: two passes, the mean first and then the products of the
deviations from it, over every chain and record of a window of a host trace x
[N, T, d].  Shares no code with diag.py.  Also the measure of agreement the
tests use."""
import numpy as np

from rhat_reference import EPS, LD, _quiet


@_quiet
def ref_cov(x, first, count):
  """{'mean': [d], 'cov': [d, d], 'corr': [d, d]} in longdouble."""
  w = np.asarray(x, LD)[:, first:first + count, :]
  d = w.shape[2]
  w = w.reshape(-1, d)
  m = w.shape[0]
  mean = w.sum(axis=0) / LD(m)
  dev = w - mean
  cov = np.empty((d, d), LD)
  dev = np.ascontiguousarray(dev.T)
  for a in range(d):
    for b in range(a, d):
      cov[a, b] = cov[b, a] = (dev[a] * dev[b]).sum() / LD(m - 1)
  sd = np.sqrt(np.diagonal(cov))
  return {'mean': mean, 'cov': cov, 'corr': cov / (sd[:, None] * sd[None, :])}


def _dist(got, ref, unit):
  got, ref = np.asarray(got, LD), np.asarray(ref, LD)
  assert got.shape == ref.shape, (got.shape, ref.shape)
  same = (got == ref) | (np.isnan(got) & np.isnan(ref))
  r = np.abs(got - ref) / unit
  r = np.where(same, LD(0), np.where(np.isnan(r), LD(np.inf), r))
  return float(r.max()) if r.size else 0.


@_quiet
def scaled_dist(got, ref):
  """max over a, b of |got_ab - ref_ab| / sqrt(ref_aa ref_bb) of two covariance
  matrices.  The plain relative distance is wrong for this statistic: an
  off-diagonal entry of independent dims is near 0, and its error is that of
  the two variances' product.  Equal values are at distance 0: the same
  number, the same infinity, NaN and NaN.  Anything else that has no finite
  quotient is at distance inf."""
  var = np.diagonal(np.asarray(ref, LD))
  return _dist(got, ref, np.sqrt(var[:, None] * var[None, :]))


@_quiet
def mean_dist(got, ref, cov):
  """max over a of |got_a - ref_a| / (|ref_a| + sqrt(cov_aa)) of two mean
  vectors: a mean K + S / M carries the rounding of K, relative to the mean
  itself, and that of S / M, relative to the spread -- whichever is larger is
  its unit.  Equal values at distance 0 as in scaled_dist."""
  ref = np.asarray(ref, LD)
  return _dist(got, ref, np.abs(ref) + np.sqrt(np.diagonal(np.asarray(cov, LD))))


@_quiet
def corr_dist(got, ref):
  """max |got_ab - ref_ab| of two correlation matrices, whose unit is 1; equal
  values at distance 0 as in scaled_dist."""
  return _dist(got, ref, LD(1))


def dists(got, ref):
  """{'mean', 'cov', 'corr'}: the three distances of a result from a
  reference, each in its own unit."""
  return {'mean': mean_dist(got['mean'], ref['mean'], ref['cov']),
          'cov': scaled_dist(got['cov'], ref['cov']),
          'corr': corr_dist(got['corr'], ref['corr'])}


def device_bounds(host, ref):
  """What the device may differ from the longdouble reference by, per result
  and in its distance: 64 eps, or 32 times the distance of diag.py's own fp64
  result from it -- the project's bound for a device reduction (rhat_reference.
  device_bound), restated for this statistic's distances."""
  return {k: max(64 * EPS, 32 * v) for k, v in dists(host, ref).items()}
