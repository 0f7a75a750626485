"""diag.pooled_quantile (CPU): the written-out definition of the quantiles
pooled over chains and records against np.quantile (default method) of the
same values, bit for bit; the NaN rule, the inf case and the refusals."""
import numpy as np
import pytest

from probayes_amd import diag

QS = [0, 1e-9, .025, .25, 1 / 3, .5, .75, .975, 1 - 1e-9, 1]
SHAPES = [(1, 1, 1), (3, 5, 2), (67, 37, 2), (130, 130, 3)]
KINDS = ['gauss', 'halves', 'constant', 'decades']


def _data(kind, shape, seed):
  rng = np.random.default_rng(seed)
  x = rng.standard_normal(shape)
  if kind == 'halves':
    return np.round(2. * x) / 2.
  if kind == 'constant':
    return np.full(shape, 1.25)
  if kind == 'decades':
    return x * 10. ** rng.uniform(-300., 300., shape)
  return x


def _numpy(x, q, first, count):
  return np.stack([np.quantile(x[:, first:first + count, k].ravel(), q)
                   for k in range(x.shape[2])], axis=1)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES)
def test_equals_numpy_quantile(shape, kind):
  x = _data(kind, shape, 11)
  t = shape[1]
  windows = {(0, t), (0, 1), (t // 3, t - t // 3), (t - 1, 1)}
  for first, count in sorted(windows):
    got = diag.pooled_quantile(x, QS, first, count)
    assert got.shape == (len(QS), shape[2])
    assert np.array_equal(got, _numpy(x, QS, first, count)), (first, count)
  assert np.array_equal(diag.pooled_quantile(x, QS), _numpy(x, QS, 0, t))
  assert np.array_equal(diag.pooled_quantile(x, .5), _numpy(x, [.5], 0, t))


def test_zeros_of_either_sign_are_one_value():
  x = np.array([0., -0., 0., -0., -1., 1.]).reshape(6, 1, 1)
  got = diag.pooled_quantile(x, QS)
  assert np.array_equal(got, _numpy(x, QS, 0, 1))
  assert got[5, 0] == 0.


def test_a_nan_makes_every_quantile_of_its_dim_nan():
  x = _data('gauss', (9, 7, 3), 5)
  x[4, 2, 1] = np.nan
  got = diag.pooled_quantile(x, QS)
  assert np.isnan(got[:, 1]).all()
  want = _numpy(x, QS, 0, 7)
  assert np.array_equal(got, want, equal_nan=True)
  assert np.isfinite(got[:, [0, 2]]).all()
  # the NaN outside the window does not count
  assert np.array_equal(diag.pooled_quantile(x, QS, 3, 4), _numpy(x, QS, 3, 4))


def test_infinities_follow_ieee():
  x = np.array([-np.inf, -1., 0., 2., np.inf, np.inf]).reshape(6, 1, 1)
  with np.errstate(invalid='ignore'):
    want = _numpy(x, QS, 0, 1)
  got = diag.pooled_quantile(x, QS)
  assert np.array_equal(got, want, equal_nan=True)
  assert np.isnan(got[-1, 0])          # a = b = inf: inf - inf
  assert np.isnan(got[-2, 0])          # between inf and inf likewise
  assert np.isnan(got[0, 0])           # -inf + inf * 0, as NumPy gives it
  assert got[5, 0] == 1.


def test_refusals():
  x = _data('gauss', (4, 6, 2), 1)
  for kw in (dict(count=0), dict(count=-1), dict(first=-1, count=2), dict(first=5, count=2),
             dict(first=7), dict(first=6)):
    with pytest.raises(ValueError):
      diag.pooled_quantile(x, [.5], **kw)
  for q in ([], [-0.1], [1.1], [.5, np.nan], np.nan):
    with pytest.raises(ValueError):
      diag.pooled_quantile(x, q)
  with pytest.raises(ValueError):
    diag.pooled_quantile(x[0], [.5])
