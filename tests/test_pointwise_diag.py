"""diag.pointwise_stats and diag.waic, the host definition of the pointwise
reduction: against scipy.special.logsumexp, np.mean and np.var on random terms,
on the columns where a naive form goes wrong, and WAIC on a case worked by
hand."""
import math

import numpy as np
import pytest
import scipy.special

from probayes_amd import diag


def _same(a, b, rtol=0.):
  """equal, infinities and NaNs in the same places (finite values within rtol)"""
  a, b = np.asarray(a, float), np.asarray(b, float)
  with np.errstate(all='ignore'):
    near = np.isfinite(a) & np.isfinite(b) & (np.abs(a - b) <= rtol * np.abs(b))
  return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b)) | near))


@pytest.mark.parametrize('shape', [(2, 1), (3, 5), (257, 9), (3120, 137)])
def test_pointwise_stats_on_random_terms(shape):
  T = np.random.default_rng(shape[0]).normal(-3., 2.5, size=shape)
  lse, mean, var = diag.pointwise_stats(T)
  assert lse.shape == mean.shape == var.shape == (shape[1],)
  assert np.allclose(lse, scipy.special.logsumexp(T, axis=0), rtol=1e-14, atol=0.)
  assert np.allclose(mean, np.mean(T, axis=0), rtol=1e-13, atol=1e-15)
  assert np.allclose(var, np.var(T, axis=0, ddof=1), rtol=1e-13, atol=0.)


def test_pointwise_stats_edge_columns():
  rng = np.random.default_rng(5)
  T = rng.normal(-2., 1., size=(50, 6))
  T[3, 0] = -np.inf            # one -inf
  T[:, 1] = -np.inf            # all -inf
  T[7, 2] = np.nan             # a NaN
  T[9, 3] = np.inf             # a +inf
  T[:, 4] = np.linspace(-745., 709., 50)   # exp overflows without the shift
  lse, mean, var = diag.pointwise_stats(T)
  with np.errstate(all='ignore'):
    assert _same(lse, scipy.special.logsumexp(T, axis=0), 1e-14)
    assert _same(mean, np.mean(T, axis=0), 1e-14)
    want_var = np.var(T, axis=0, ddof=1)
  assert np.isfinite(lse[0]) and mean[0] == -np.inf and np.isnan(var[0])
  assert lse[1] == -np.inf and mean[1] == -np.inf and np.isnan(var[1])
  assert np.isnan(lse[2]) and np.isnan(mean[2]) and np.isnan(var[2])
  assert lse[3] == np.inf and mean[3] == np.inf and np.isnan(var[3])
  assert np.isfinite(lse[4]) and 709. <= lse[4] < 710.
  assert abs(lse[4] - scipy.special.logsumexp(T[:, 4])) <= 1e-13 * lse[4]
  assert np.allclose(var[4:], want_var[4:], rtol=1e-13, atol=0.)
  assert np.all(np.isnan(want_var[:4]))


def test_pointwise_stats_of_two_draws():
  T = np.array([[0., -1., 2.], [0., -3., 2.5]])
  lse, mean, var = diag.pointwise_stats(T)
  assert _same(lse, scipy.special.logsumexp(T, axis=0), 1e-14)
  assert np.array_equal(mean, [0., -2., 2.25])
  assert np.array_equal(var, [0., 2., 0.125])
  with pytest.raises(ValueError):
    diag.pointwise_stats(T[:1])


def test_waic_by_hand():
  # S = 2 draws, n = 3 observations
  T = np.log(np.array([[0.5, 0.25, 0.125], [0.5, 0.75, 0.5]]))
  lse, mean, var = diag.pointwise_stats(T)
  res = diag.waic(lse, mean, var, 2)
  lppd_i = np.log(np.array([0.5, 0.5, 0.3125]))       # log of the mean density
  p_i = np.array([0., math.log(3.) ** 2 / 2., math.log(4.) ** 2 / 2.])
  elpd_i = lppd_i - p_i
  assert np.allclose(res['lppd_i'], lppd_i, rtol=1e-15, atol=1e-16)
  assert np.allclose(res['p_waic_i'], p_i, rtol=1e-15, atol=0.)
  assert np.allclose(res['elpd_i'], elpd_i, rtol=1e-15, atol=0.)
  assert math.isclose(res['lppd'], lppd_i.sum(), rel_tol=1e-15)
  assert math.isclose(res['p_waic'], p_i.sum(), rel_tol=1e-15)
  assert math.isclose(res['elpd_waic'], elpd_i.sum(), rel_tol=1e-15)
  m = elpd_i.sum() / 3.
  se = math.sqrt(3. * ((elpd_i - m) ** 2).sum() / 3.)
  assert math.isclose(res['se'], se, rel_tol=1e-14)
  assert res['waic'] == -2. * res['elpd_waic']
