"""diag.pooled_cov, pooled_cov_finish and proposal_cov (no GPU): the host
definition of the pooled posterior covariance against the longdouble two-pass
restatement of cov_reference.py, on AR(1) chains with repeats mixed by a fixed
matrix so that the dims are correlated.

The bound is 64 eps in units of sqrt(cov_aa cov_bb) (cov_reference.
scaled_dist), and the same in the mean's and the correlation's own units; the
same data through a copy of the formula without the shift
must miss it at loc = 1e6, which shows that the test sees the shift."""
import numpy as np
import pytest

from probayes_amd import diag
from cov_reference import dists, ref_cov, scaled_dist
from rhat_reference import EPS, ar1_with_repeats

N, T, D = 2004, 160, 10
WINDOWS = ((40, 120), (40, 119), (0, 1), (0, 4))
BOUND = 64 * EPS


def _mix():
  rng = np.random.RandomState(11)
  return np.eye(D) + 0.4 * rng.normal(size=(D, D))


_CACHE = {}


def trace(loc):
  if loc not in _CACHE:
    _CACHE[loc] = loc + ar1_with_repeats(N, T, D, seed=5).dot(_mix().T)
  return _CACHE[loc]


def unshifted_cov(x, first, count):
  """pooled_cov's formula with K = 0"""
  w = x[:, first:first + count, :].reshape(-1, x.shape[2])
  m = float(w.shape[0])
  s = w.sum(axis=0)
  p = w.T.dot(w)
  return (p - np.outer(s, s) / m) / (m - 1.)


@pytest.mark.parametrize('first,count', WINDOWS)
@pytest.mark.parametrize('loc', [0., 1e6])
def test_against_the_longdouble_reference(loc, first, count):
  x = trace(loc)
  got, ref = diag.pooled_cov(x, first, count), ref_cov(x, first, count)
  assert got['mean'].shape == (D,) and got['cov'].shape == got['corr'].shape == (D, D)
  assert np.abs(ref['corr'] - np.eye(D)).max() > 0.3   # the dims are correlated
  dist = dists(got, ref)
  print('loc {} window {}: {}'.format(loc, (first, count),
                                      {k: '{:.3g} eps'.format(v / EPS) for k, v in dist.items()}))
  for key, v in dist.items():
    assert v <= BOUND, (key, v / EPS)
  # symmetric in its bits, the diagonal of corr exactly 1
  assert got['cov'].tobytes() == got['cov'].T.copy().tobytes()
  assert got['corr'].tobytes() == got['corr'].T.copy().tobytes()
  assert np.array_equal(np.diagonal(got['corr']), np.ones(D))


def test_the_shift_is_what_keeps_the_digits():
  x = trace(1e6)
  ref = ref_cov(x, 40, 120)['cov']
  without = scaled_dist(unshifted_cov(x, 40, 120), ref)
  with_shift = scaled_dist(diag.pooled_cov(x, 40, 120)['cov'], ref)
  print('loc 1e6: no shift {:.3g} eps, shifted {:.3g} eps'.format(without / EPS,
                                                                  with_shift / EPS))
  assert without > BOUND >= with_shift
  # at loc 0 the same copy is fine: it is the formula, not the copy, that fails
  x = trace(0.)
  assert scaled_dist(unshifted_cov(x, 40, 120), ref_cov(x, 40, 120)['cov']) <= BOUND


def test_finish_alone_gives_the_same_bits():
  x = trace(0.)
  w = x[:, 40:160, :]
  K = w[:, 0, :].mean(axis=0)
  v = np.ascontiguousarray((w - K).reshape(-1, D).T)   # [D, M]
  M = v.shape[1]
  S = v.sum(axis=1)
  P = np.concatenate([(v[a:] * v[a]).sum(axis=1) for a in range(D)])
  a, b = diag.pooled_cov_finish(K, S, P, M), diag.pooled_cov(x, 40, 120)
  for key in ('mean', 'cov', 'corr'):
    assert a[key].tobytes() == b[key].tobytes(), key
  full = np.zeros((D, D))
  full[np.triu_indices(D)] = P
  c = diag.pooled_cov_finish(K, S, full, M)
  assert c['cov'].tobytes() == a['cov'].tobytes()
  # sums of two ranks about one K add
  parts = [(u.sum(axis=1), np.concatenate([(u[a:] * u[a]).sum(axis=1) for a in range(D)]))
           for u in (v[:, :M // 2], v[:, M // 2:])]
  both = diag.pooled_cov_finish(K, parts[0][0] + parts[1][0], parts[0][1] + parts[1][1], M)
  assert scaled_dist(both['cov'], ref_cov(x, 40, 120)['cov']) <= BOUND


def test_constant_and_equal_chains():
  x = np.broadcast_to(np.array([-1., 0.5, 1e6]), (7, 12, 3)).copy()
  got = diag.pooled_cov(x, 2, 9)
  assert np.array_equal(got['cov'], np.zeros((3, 3))) and not np.signbit(got['cov']).any()
  assert np.isnan(got['corr']).all()
  assert np.array_equal(got['mean'], x[0, 0])
  # one dim that never moves beside one that does
  x[:, :, 1] = np.random.RandomState(3).normal(size=(7, 12))
  got = diag.pooled_cov(x)
  nan = np.isnan(got['corr'])
  assert nan[0].all() and nan[:, 2].all() and got['corr'][1, 1] == 1. and nan.sum() == 8
  assert got['cov'][0, 0] == 0. and got['cov'][1, 1] > 0.


def test_a_nan_record_propagates():
  x = trace(0.)[:50, :8, :3].copy()
  x[7, 3, 1] = np.nan
  got = diag.pooled_cov(x)
  assert np.isnan(got['mean'][1]) and np.isnan(got['cov'][1]).all() and \
      np.isnan(got['cov'][:, 1]).all()
  assert np.isfinite(got['cov'][np.ix_([0, 2], [0, 2])]).all()
  assert np.isfinite(diag.pooled_cov(x, 4, 4)['cov']).all()   # the window leaves it out


def test_argument_errors():
  x = trace(0.)[:4, :8, :2]
  with pytest.raises(ValueError, match=r'a trace \[N, T, d\]'):
    diag.pooled_cov(x[0])
  with pytest.raises(ValueError, match=r'records \[5, 9\) outside \[0, 8\)'):
    diag.pooled_cov(x, 5, 4)
  with pytest.raises(ValueError, match=r'records \[-1, 3\)'):
    diag.pooled_cov(x, -1, 4)
  with pytest.raises(ValueError, match='count = 0'):
    diag.pooled_cov(x, 3, 0)
  with pytest.raises(ValueError, match='at least 2 draws'):
    diag.pooled_cov(x[:1], 3, 1)
  assert diag.pooled_cov(x[:2], 3, 1)['cov'].shape == (2, 2)   # M = 2 is enough
  with pytest.raises(ValueError, match='at least 2 draws'):
    diag.pooled_cov_finish(np.zeros(2), np.zeros(2), np.zeros(3), 1)
  with pytest.raises(ValueError, match=r'P \[d \(d \+ 1\) / 2\]'):
    diag.pooled_cov_finish(np.zeros(2), np.zeros(2), np.zeros(4), 9)


@pytest.mark.parametrize('d', [1, 2, 10])
def test_proposal_scale(d):
  rng = np.random.RandomState(d)
  a = rng.normal(size=(d, d))
  cov = a.dot(a.T) + 0.1 * np.eye(d)
  cov = (cov + cov.T) / 2.
  got = diag.proposal_cov(cov)
  assert got.tobytes() == (2.38 ** 2 / d * cov).tobytes()
  assert diag.proposal_cov(cov, scale=0.25).tobytes() == (0.25 * cov).tobytes()
  lifted = diag.proposal_cov(cov, eps=1e-3)
  want = 2.38 ** 2 / d * (cov + 1e-3 * np.mean(np.diagonal(cov)) * np.eye(d))
  assert lifted.tobytes() == want.tobytes()
  np.linalg.cholesky(got)


def test_proposal_refusals():
  with pytest.raises(ValueError, match='not positive definite'):
    diag.proposal_cov(np.array([[1., 1.], [1., 1.]]))      # two variables that move as one
  with pytest.raises(ValueError, match='not positive definite'):
    diag.proposal_cov(np.zeros((3, 3)))                    # chains that never moved
  # eps lifts a singular estimate
  np.linalg.cholesky(diag.proposal_cov(np.array([[1., 1.], [1., 1.]]), eps=1e-6))
  for bad in (np.nan, np.inf):
    with pytest.raises(ValueError, match='not finite'):
      diag.proposal_cov(np.array([[1., 0.], [0., bad]]))
  with pytest.raises(ValueError, match='not finite'):
    diag.proposal_cov(np.eye(2), scale=np.inf)
  with pytest.raises(ValueError, match='square'):
    diag.proposal_cov(np.ones((2, 3)))
  with pytest.raises(ValueError, match='square'):
    diag.proposal_cov(np.ones(4))
  with pytest.raises(ValueError, match='not symmetric'):
    diag.proposal_cov(np.array([[1., 0.1], [0.2, 1.]]))
  with pytest.raises(ValueError, match='not positive definite'):
    diag.proposal_cov(np.eye(2), scale=-1.)
