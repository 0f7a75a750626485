"""The host definition of PSIS-LOO (no GPU): diag.pointwise_tail, gpd_fit,
psis_loo_from_tail, psis_loo and compare_elpd.

gpd_fit is held to scale equivariance at 1e-12 and to the recovery of the
shape of scipy.stats.genpareto samples within 5 (1 + k) / sqrt(m) + 10 |0.5 -
k| / (m + 10): five asymptotic standard errors of the maximum-likelihood
estimate plus the shrinkage of the weakly informative prior.  psis_loo is held
to a second route written here from the full sorted column -- all S weights,
the tail's replaced, then logsumexp(lw + T) - logsumexp(lw) -- at 1e-12 with
floor 1."""
import math

import numpy as np
import pytest
import scipy.special
import scipy.stats

from probayes_amd import diag

RTOL = 1e-12


# ---------------------------------------------------------------------------
# the generalised-Pareto fit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('m', [100, 538, 2000])
@pytest.mark.parametrize('k', [-0.3, 0.2, 0.7])
def test_gpd_fit_recovers_the_shape(k, m):
  bound = 5. * (1. + k) / math.sqrt(m) + 10. * abs(0.5 - k) / (m + 10.)
  worst = 0.
  for seed in range(20):
    x = np.sort(scipy.stats.genpareto.rvs(k, size=m, random_state=seed))
    khat, sigma = diag.gpd_fit(x)
    worst = max(worst, abs(khat - k))
    assert sigma > 0.
  print('k = {}, m = {}: worst error {:.4f}, bound {:.4f}'.format(k, m, worst, bound))
  assert worst <= bound


@pytest.mark.parametrize('m', [100, 538, 2000])
def test_gpd_fit_is_scale_equivariant(m):
  for seed, k in enumerate((-0.3, 0.2, 0.7)):
    x = np.sort(scipy.stats.genpareto.rvs(k, size=m, random_state=seed))
    k1, s1 = diag.gpd_fit(x)
    k8, s8 = diag.gpd_fit(8. * x)
    assert abs(k8 - k1) <= RTOL and abs(s8 / 8. - s1) <= RTOL * max(s1, 1.)


# ---------------------------------------------------------------------------
# the tail
# ---------------------------------------------------------------------------
def test_pointwise_tail_is_sorting():
  rng = np.random.default_rng(2)
  T = rng.normal(-3., 2., (780, 6))
  T[5, 1], T[6, 1] = -0., 0.
  T[:, 2] = -1.5
  T[::3, 3] = np.nan
  T[:4, 4] = -np.inf
  T[4:500, 5] = np.inf
  k = 157
  tail, rest = diag.pointwise_tail(T, k)
  assert tail.shape == (6, k) and rest.shape == (6,)
  for j in range(6):
    s = np.sort(T[:, j])
    assert np.array_equal(tail[j], s[:k], equal_nan=True)
    assert not np.signbit(tail[j][tail[j] == 0]).any()
    want = scipy.special.logsumexp(-s[k:]) if not np.isnan(s[k:]).any() else np.nan
    if np.isfinite(want):
      assert abs(rest[j] - want) <= RTOL * max(abs(want), 1.)
    else:
      assert np.array_equal([rest[j]], [want], equal_nan=True)
  assert np.isnan(rest[3]) and np.isnan(tail[3]).sum() == 0    # 520 terms are not NaN
  assert rest[4] < np.inf and np.all(tail[4][:4] == -np.inf)
  assert np.all(np.isfinite(tail[5])) and np.isfinite(rest[5])  # (+inf terms weigh nothing)
  both = T[:, :1].copy()
  both[:200, 0] = -np.inf
  assert diag.pointwise_tail(both, k)[1][0] == np.inf
  for bad in (0, 780, 781):
    with pytest.raises(ValueError):
      diag.pointwise_tail(T, bad)


# ---------------------------------------------------------------------------
# PSIS-LOO against a second route
# ---------------------------------------------------------------------------
def _second_route(col):
  """(elpd_loo, pareto_k) of one finite column from all its S weights"""
  S = col.size
  m = min(S // 5, int(math.ceil(3. * math.sqrt(S))))
  order = np.argsort(-col, kind='stable')          # the log-ratios -T ascending
  lw = -col[order]
  lw = lw - lw[-1]
  cut = lw[S - m - 1]
  x = np.exp(lw[S - m:]) - np.exp(cut)
  k, sigma = diag.gpd_fit(x)
  p = (np.arange(1, m + 1) - 0.5) / m
  smooth = np.log(sigma * np.expm1(-k * np.log1p(-p)) / k + np.exp(cut))
  lw = lw.copy()
  lw[S - m:] = np.minimum(smooth, 0.)
  elpd = scipy.special.logsumexp(lw + col[order]) - scipy.special.logsumexp(lw)
  return elpd, k


def _columns(S):
  rng = np.random.default_rng(S)
  mu = rng.normal(0., 1., S)
  sd = np.exp(rng.normal(0., 0.3, S))
  ys = np.array([-2.5, -0.4, 0.1, 1.3, 4.])
  return scipy.stats.norm.logpdf(ys[None, :], mu[:, None], sd[:, None])


@pytest.mark.parametrize('S', [780, 910, 3120, 32064])
def test_psis_loo_against_a_second_route(S):
  T = _columns(S)
  got = diag.psis_loo(T)
  assert sorted(got) == ['elpd_loo', 'elpd_loo_i', 'looic', 'n_bad_k', 'p_loo', 'p_loo_i',
                         'pareto_k', 'se']
  want = [_second_route(T[:, j]) for j in range(T.shape[1])]
  for j, (elpd, k) in enumerate(want):
    e_elpd = abs(got['elpd_loo_i'][j] - elpd) / max(abs(elpd), 1.)
    e_k = abs(got['pareto_k'][j] - k) / max(abs(k), 1.)
    print('S = {} observation {}: elpd {:.6f} (err {:.3g}), k {:.4f} (err {:.3g})'.format(
        S, j, elpd, e_elpd, k, e_k))
    assert e_elpd <= RTOL and e_k <= RTOL
  lppd_i = scipy.special.logsumexp(T, axis=0) - math.log(S)
  assert np.allclose(got['p_loo_i'], lppd_i - got['elpd_loo_i'], rtol=0, atol=1e-12)
  assert np.all(got['p_loo_i'] > 0.)               # leaving a point out predicts it worse
  assert got['elpd_loo'] == float(got['elpd_loo_i'].sum())
  assert got['looic'] == -2. * got['elpd_loo']
  assert abs(got['p_loo'] - float(got['p_loo_i'].sum())) <= 1e-12
  assert abs(got['se'] - math.sqrt(5 * np.var(got['elpd_loo_i']))) <= 1e-12
  thr = min(1. - 1. / math.log10(S), 0.7)
  assert got['n_bad_k'] == int((got['pareto_k'] > thr).sum())


def test_the_device_route_is_the_same_function():
  T = _columns(3120)
  S = T.shape[0]
  m = diag.psis_tail_length(S)
  assert m == 168
  tail, rest = diag.pointwise_tail(T, m + 1)
  a = diag.psis_loo_from_tail(tail, rest, S, diag.pointwise_stats(T)[0])
  b = diag.psis_loo(T)
  for key in a:
    assert np.array_equal(a[key], b[key]), key
  rows = diag.psis_loo_from_tail(tail, rest, S)
  assert sorted(rows) == ['elpd_loo_i', 'pareto_k']


def test_degenerate_rows():
  T = _columns(780)
  S = T.shape[0]
  base = diag.psis_loo(T)
  nan, minus, plus, tied, const = (T.copy() for _ in range(5))
  nan[3, 0] = np.nan
  minus[3, 0] = -np.inf
  plus[:300, 0] = np.inf
  tied[:, 0] = np.where(np.arange(S) % 2, -1., -2.)
  const[:, 0] = -1.25
  with np.errstate(all='ignore'):
    for T2, k, elpd in ((nan, np.nan, np.nan), (minus, np.inf, -np.inf), (tied, np.inf, None),
                        (const, np.inf, None)):
      got = diag.psis_loo(T2)
      assert np.array_equal([got['pareto_k'][0]], [k], equal_nan=True)
      if elpd is not None:
        assert np.array_equal([got['elpd_loo_i'][0]], [elpd], equal_nan=True)
      else:
        raw = math.log(S) - scipy.special.logsumexp(-T2[:, 0])
        assert abs(got['elpd_loo_i'][0] - raw) <= RTOL * max(abs(raw), 1.)
      assert got['n_bad_k'] >= 1
      for key in ('pareto_k', 'elpd_loo_i'):
        assert np.array_equal(got[key][1:], base[key][1:]), key   # the other rows as they were
    # +inf terms weigh nothing: a finite tail, a finite fit
    got = diag.psis_loo(plus)
    assert np.isfinite(got['pareto_k'][0])


def test_too_few_draws():
  with pytest.raises(ValueError, match='S >= 25'):
    diag.psis_loo(np.zeros((24, 3)))
  with pytest.raises(ValueError):
    diag.psis_tail_length(0)
  assert diag.psis_tail_length(25) == 5 and diag.psis_tail_length(82 * 10 ** 6) == 27167
  diag.psis_loo(_columns(25))
  with pytest.raises(ValueError):
    diag.psis_loo_from_tail(np.zeros((3, 5)), np.zeros(3), 25)   # 6 columns are wanted


# ---------------------------------------------------------------------------
# the comparison of two models
# ---------------------------------------------------------------------------
def test_compare_elpd_on_two_rows():
  a = np.array([-1., -2., -3., -4.])
  b = np.array([-1.5, -1.5, -3.5, -5.])
  diff, se = diag.compare_elpd(a, b)
  # a - b = (0.5, -0.5, 0.5, 1): sum 1.5, mean 0.375, squares about it 1.1875
  assert diff == 1.5
  assert abs(se - math.sqrt(1.1875)) <= 1e-15
  assert diag.compare_elpd(b, a) == (-diff, se)
  assert diag.compare_elpd(a, a) == (0., 0.)
  with pytest.raises(ValueError):
    diag.compare_elpd(a, b[:3])
