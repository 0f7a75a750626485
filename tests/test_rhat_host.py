"""probayes_amd/diag.py (CPU): the host definition of split-R-hat and nested
R-hat against the longdouble restatement of rhat_reference.py on synthetic
AR(1)-with-repeats traces, and values pinned by construction.

The bounds diag.py's fp64 results are held to come from the arithmetic, not
from its output (u = eps / 2, n the records summed, all conditioning figures
taken from the longdouble reference):
  mean   K + S / n with S a sequential sum of v = x - K: |error| <= eps (|mean|
         + n max|v|).
  var    (Q - S S / n) / (n - 1), the one-pass form on the shifted v, whose
         relative error is n u kappa^2 to first order (Chan, Golub, LeVeque
         1983), kappa^2 = Q / (Q - S S / n): 2 (n + 3) eps kappa^2 here.
  R-hat  sqrt of a ratio of a variance of means V and a mean of variances W:
         64 eps for the sums, the variances' own bound, and the means' error
         eps |m| against the spread they are compared at, sqrt(V) (and, for
         nested R-hat with group > 1, sqrt of the smallest B_k).
"""
import numpy as np
import pytest

from probayes_amd import diag
from rhat_reference import (EPS, LD, ar1_with_repeats, ref_moments, ref_nested,
                            ref_split, rel_dist)


def _var_bounds(x, first, count):
  """[3, N, d]: the relative bound of the three variance rows."""
  w = np.asarray(x, LD)[:, first:first + count, :]
  v = w - w[:, :1, :]
  h = count // 2
  out = []
  for seg in (v[:, :h], v[:, count - h:], v):
    n = seg.shape[1]
    q, s = (seg * seg).sum(axis=1), seg.sum(axis=1)
    with np.errstate(all='ignore'):   # (a constant segment: 0/0, checked for equality)
      out.append(2 * (n + 3) * EPS * q / (q - s * s / n))
  return np.array(out, float)


def _check_moments(x, first, count):
  got = diag.chain_moments(x, first, count)
  ref = ref_moments(x, first, count)
  assert got.shape == ref.shape == (6,) + (x.shape[0], x.shape[2])
  w = np.asarray(x, LD)[:, first:first + count, :]
  vmax = np.abs(w - w[:, :1, :]).max(axis=1)
  vb = _var_bounds(x, first, count)
  h = count // 2
  for i, n in ((0, h), (2, h), (4, count)):
    err = np.abs(got[i] - ref[i])
    assert (err <= EPS * (np.abs(ref[i]) + n * vmax)).all(), (i, float(err.max()))
    if n < 2:
      assert np.isnan(got[i + 1]).all()   # 0/0, as stated
      continue
    flat = ref[i + 1] == 0   # a segment of repeats: variance 0, and exactly so
    assert np.array_equal(got[i + 1][flat], np.zeros(flat.sum()))
    rel = np.abs(got[i + 1] - ref[i + 1])[~flat] / ref[i + 1][~flat]
    assert (rel <= vb[i // 2][~flat]).all(), (i + 1, float(rel.max()))
  return got, ref, float(vb[np.isfinite(vb)].max())


def _rhat_bound(means, V, var_bound, B=None):
  tol = 64 * EPS + var_bound + 2 * EPS * float(np.abs(means).max() / np.sqrt(V.min()))
  if B is not None:
    tol += 2 * EPS * float(np.abs(means).max() / np.sqrt(B.min()))
  return tol


def _check_all(x, first, count, groups):
  got, ref, vb = _check_moments(x, first, count)
  h, (n, _, d) = count // 2, x.shape
  dist = {}
  if h >= 2:
    m = np.concatenate([ref[0], ref[2]])
    want = ref_split(x, first, count)
    dist['split'] = rel_dist(diag.split_rhat(got, h), want)
    assert dist['split'] <= _rhat_bound(m, m.var(axis=0, ddof=1), vb), dist
  for g in groups:
    mk = ref[4].reshape(n // g, g, d)
    mu = mk.mean(axis=1)
    B = mk.var(axis=1, ddof=1) if g > 1 else None
    want = ref_nested(x, first, count, g)
    dist[g] = rel_dist(diag.nested_rhat(got, count, g), want)
    assert dist[g] <= _rhat_bound(ref[4], mu.var(axis=0, ddof=1), vb, B), (g, dist)
  return dist


@pytest.mark.parametrize('first,count', [(0, 41), (0, 40), (5, 36), (7, 33), (0, 4),
                                         (3, 5), (2, 2), (1, 3)])
def test_against_the_definition(first, count):
  n = 12
  x = ar1_with_repeats(n, 41, 3, seed=11)
  rep = x[:, 1:] == x[:, :-1]
  assert rep.any() and not rep.all()
  dist = _check_all(x, first, count, [1, 3, n // 2])
  print('fp64 - longdouble distances', (first, count), dist)


def test_odd_count_drops_the_middle_record():
  x = ar1_with_repeats(6, 9, 2, seed=5)
  y = x.copy()
  y[:, 4] += 100.    # the middle of [0, 9): in neither half
  a, b = diag.chain_moments(x, 0, 9), diag.chain_moments(y, 0, 9)
  assert np.array_equal(a[:4], b[:4]) and not np.array_equal(a[4:], b[4:])
  assert np.array_equal(diag.split_rhat(a, 4), diag.split_rhat(b, 4))


def test_large_offset():
  n, t = 64, 200
  x = ar1_with_repeats(n, t, 2, seed=3, loc=1e6, sd=1e-3)
  dist = _check_all(x, 0, t, [1, 4, n // 2])
  print('mean 1e6, sd 1e-3: fp64 - longdouble distances', dist)
  # the shift is what keeps the variances: sums of raw squares lose them
  w = x[:, :, 0]
  raw = ((w * w).sum(axis=1) - w.sum(axis=1) ** 2 / t) / (t - 1.)
  ref = ref_moments(x, 0, t)[5][:, 0]
  assert rel_dist(raw, ref) > 1e-3
  assert rel_dist(diag.chain_moments(x, 0, t)[5][:, 0], ref) < 1e-12


def _both(x, group, first=0, count=None):
  count = x.shape[1] - first if count is None else count
  mom = diag.chain_moments(x, first, count)
  return diag.split_rhat(mom, count // 2), diag.nested_rhat(mom, count, group)


def test_values_pinned_by_construction():
  n, t, d = 512, 200, 2
  x = np.random.RandomState(1).normal(size=(n, t, d))
  for g in (1, 4, n // 2):
    split, nested = _both(x, g)
    assert (np.abs(split - 1.) < 0.02).all() and (np.abs(nested - 1.) < 0.02).all(), g
  # every chain drifts by one standard deviation between its halves
  y = x.copy()
  y[:, t // 2:] += 1.
  split, nested = _both(y, 4)
  assert (split > 1.1).all() and (nested < 1.05).all(), (split, nested)
  # half the superchains sit one standard deviation away: the halves of a
  # chain agree (the between-chain term is all split-R-hat sees of it)
  z = x.copy()
  z[:n // 2] += 1.
  split, nested = _both(z, 4)
  assert (nested > 1.1).all(), nested
  # one superchain per mode and group = N / 2
  assert (_both(z, n // 2)[1] > 1.1).all()


def test_constant_chains_and_nan():
  n, t, d = 8, 10, 2
  same = np.full((n, t, d), 1.5)
  split, nested = _both(same, 2)
  assert np.isnan(split).all() and np.isnan(nested).all()
  diff = same + np.arange(n)[:, None, None]
  split, nested = _both(diff, 1)
  assert (split == np.inf).all() and (nested == np.inf).all()
  # (within a superchain the chains start at one point: B_k + W_k = 0 as well)
  pairs = same + (np.arange(n) // 2)[:, None, None]
  split, nested = _both(pairs, 2)
  assert (split == np.inf).all() and (nested == np.inf).all()
  x = ar1_with_repeats(n, t, d, seed=2)
  x[3, 7, 1] = np.nan
  split, nested = _both(x, 2)
  assert np.isnan(split[1]) and np.isnan(nested[1])
  assert np.isfinite(split[0]) and np.isfinite(nested[0])


def test_rows_of_several_ranks_concatenate():
  x = ar1_with_repeats(12, 30, 3, seed=8)
  whole = diag.chain_moments(x, 2, 27)
  parts = np.concatenate([diag.chain_moments(x[:5], 2, 27),
                          diag.chain_moments(x[5:], 2, 27)], axis=1)
  assert np.array_equal(whole, parts)
  assert np.array_equal(diag.split_rhat(whole, 13), diag.split_rhat(parts, 13))
  assert np.array_equal(diag.nested_rhat(whole, 27, 3), diag.nested_rhat(parts, 27, 3))


def test_refusals():
  x = ar1_with_repeats(6, 12, 2, seed=4)
  mom = diag.chain_moments(x)
  for bad in (dict(first=0, count=1), dict(first=-1, count=4), dict(first=10, count=3)):
    with pytest.raises(ValueError):
      diag.chain_moments(x, **bad)
  with pytest.raises(ValueError, match='h = 1'):
    diag.split_rhat(mom, 1)
  with pytest.raises(ValueError, match='count = 1'):
    diag.nested_rhat(mom, 1, 2)
  with pytest.raises(ValueError, match='group = 0'):
    diag.nested_rhat(mom, 12, 0)
  with pytest.raises(ValueError, match='group = 4'):
    diag.nested_rhat(mom, 12, 4)
  with pytest.raises(ValueError, match='group = 6'):
    diag.nested_rhat(mom, 12, 6)
