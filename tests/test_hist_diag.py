"""The host definition of the pooled histograms (no GPU): diag.hist_bin,
pooled_hist and pooled_hist2d against np.histogram and np.histogram2d, and
diag.hist_edges, hist_density and hist2d_density against the edges and the
densities NumPy forms.  Every comparison of counts is integer equality.

The data is a [6, 37, 3] trace that holds NaN, +-inf, +-0.0, values equal to the
first, an inner and the last edge and the doubles either side of each."""
import numpy as np
import pytest

from probayes_amd import diag

N, T, D = 6, 37, 3
WINDOWS = ((0, 37), (7, 3), (36, 1))
EDGES = {'uniform': np.linspace(-1., 7., 51), 'geometric': np.geomspace(1e-3, 6., 24),
         'one bin': np.array([-0.5, 2.5]), 'about zero': np.array([-2., -0., 1e-300, 3.])}


def _trace():
  rng = np.random.RandomState(12)
  x = rng.normal(size=(N, T, D)) * 2.5 + 2.
  special = [np.nan, np.inf, -np.inf, 0., -0., 5e-324, -5e-324]
  for e in EDGES.values():
    for v in (e[0], e[len(e) // 2], e[-1]):
      special += [v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf)]
  special = np.array(special)
  # every special value in every dim, and in every window's records
  for k in range(D):
    at = rng.permutation(N * (T - 4))[:special.size]
    x[at % N, at // N, k] = special[rng.permutation(special.size)]
    x[:, 7:10, k].flat[:16] = special[rng.permutation(special.size)[:16]]
    x[:, 36, k] = special[rng.permutation(special.size)[:N]]
  return x


X = _trace()


def _pooled(first, count, k):
  return X[:, first:first + count, k].ravel()


def _np_hist(a, e):
  return np.histogram(a, e)[0]


def test_the_trace_holds_the_special_values():
  assert np.isnan(X).any() and np.isposinf(X).any() and np.isneginf(X).any()
  assert ((X == 0.) & np.signbit(X)).any() and ((X == 0.) & ~np.signbit(X)).any()
  for e in EDGES.values():
    for v in (e[0], e[len(e) // 2], e[-1]):
      for w in (v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf)):
        assert (X == w).any()


@pytest.mark.parametrize('name', sorted(EDGES))
def test_hist_bin_is_where_numpy_counts(name):
  e = EDGES[name]
  a = X.ravel()
  b = diag.hist_bin(a, e)
  assert b.dtype == np.int64 and b.shape == a.shape
  assert np.array_equal(np.bincount(b[b >= 0], minlength=e.size - 1), _np_hist(a, e))
  assert np.array_equal(b == -3, np.isnan(a))
  assert np.array_equal(b == -1, a < e[0]) and np.array_equal(b == -2, a > e[-1])
  # the rule itself, value by value
  for i in range(e.size - 1):
    inside = (a >= e[i]) & ((a < e[i + 1]) | ((i == e.size - 2) & (a == e[-1])))
    assert np.array_equal(b == i, inside), i
  # a shape is kept; the zeros are one value
  assert diag.hist_bin(X, e).shape == X.shape
  assert diag.hist_bin(-0., [0., 1.]) == 0 and diag.hist_bin(0., [-1., -0.]) == 0


@pytest.mark.parametrize('first,count', WINDOWS)
def test_pooled_hist_equals_np_histogram(first, count):
  names = sorted(EDGES)
  for shift in range(len(names)):
    edges = [EDGES[names[(k + shift) % len(names)]] for k in range(D)]
    got = diag.pooled_hist(X, edges, first, count)
    assert got['outside'].dtype == np.int64 and got['outside'].shape == (D, 3)
    for k, e in enumerate(edges):
      a = _pooled(first, count, k)
      assert got['counts'][k].dtype == np.int64
      assert np.array_equal(got['counts'][k], _np_hist(a, e))
      assert list(got['outside'][k]) == [(a < e[0]).sum(), (a > e[-1]).sum(), np.isnan(a).sum()]
      assert got['counts'][k].sum() + got['outside'][k].sum() == N * count


@pytest.mark.parametrize('first,count', WINDOWS)
def test_pooled_hist_equals_np_histogram_with_bins_and_range(first, count):
  for nb, (lo, hi) in ((50, (-1., 7.)), (1, (0., 2.)), (7, (-3., 3.)), (33, (2.9, 3.1))):
    e = np.linspace(lo, hi, nb + 1)
    got = diag.pooled_hist(X, [e, None, e], first, count)
    assert got['counts'][1] is None and list(got['outside'][1]) == [0, 0, 0]
    for k in (0, 2):
      a = _pooled(first, count, k)
      h, edges = np.histogram(a, nb, range=(lo, hi))
      assert np.array_equal(edges, e) and np.array_equal(got['counts'][k], h)


@pytest.mark.parametrize('first,count', WINDOWS)
def test_pooled_hist2d_equals_np_histogram2d(first, count):
  edges = [EDGES['uniform'], EDGES['geometric'], EDGES['about zero']]
  pairs = [(0, 1), (1, 0), (0, 0), (2, 1), (1, 2), (2, 2)]
  got = diag.pooled_hist2d(X, edges, pairs, first, count)
  assert len(got) == len(pairs)
  for (a, b), h in zip(pairs, got):
    xa, xb = _pooled(first, count, a), _pooled(first, count, b)
    ref = np.histogram2d(xa, xb, bins=[edges[a], edges[b]])[0]
    assert h.dtype == np.int64 and h.shape == (edges[a].size - 1, edges[b].size - 1)
    assert np.array_equal(h, ref.astype(np.int64)) and ref.sum() == h.sum()
  # (a, b) is (b, a) transposed; (a, a) is the marginal on the diagonal
  assert np.array_equal(got[0], got[1].T)
  one = diag.pooled_hist(X, edges, first, count)['counts']
  assert np.array_equal(np.diagonal(got[2]), one[0]) and got[2].sum() == one[0].sum()


def test_refusals():
  e = EDGES['uniform']
  for bad in ([0., 1., 1.], [0., np.inf], [1., 0.], [np.nan, 1.], [1.], np.zeros((2, 2))):
    with pytest.raises(ValueError):
      diag.hist_bin(0., bad)
  for kw in (dict(edges=[e, e]), dict(edges=[None] * 3), dict(edges=[e] * 3, first=30, count=8),
             dict(edges=[e] * 3, count=0)):
    with pytest.raises(ValueError):
      diag.pooled_hist(X, **kw)
  for pairs in ([], [(0, 3)], [(0, 1)], [(-1, 0)]):
    with pytest.raises(ValueError):
      diag.pooled_hist2d(X, [e, None, e], pairs)
  with pytest.raises(ValueError):
    diag.pooled_hist(X[0], [e] * 3)


# ---- hist_edges ----------------------------------------------------------------
def test_hist_edges_of_one_variable():
  a = np.random.RandomState(2).normal(size=500) * 3. + 1.
  lohi = lambda: (a.min(), a.max())
  for nb in (1, 10, 40, 4096):
    for rng in (None, (-2., 5.), (0, 1), (3., 3.), (-1e300, 1e300)):
      got = diag.hist_edges(nb, rng, minmax=lohi)
      assert got.dtype == np.float64
      assert got.tobytes() == np.histogram_bin_edges(a, nb, rng).tobytes(), (nb, rng)
  # the data's range is asked for only when it is needed
  boom = lambda: 1 / 0
  assert diag.hist_edges(4, (0., 1.), minmax=boom).tobytes() == np.linspace(0., 1., 5).tobytes()
  e = [0, 1, 4, 9.5]
  got = diag.hist_edges(e, (100., 200.), minmax=boom)
  assert got.dtype == np.float64 and got.tobytes() == np.histogram_bin_edges(a, e).tobytes()
  assert diag.hist_edges(np.int64(3), (0., 3.)).tolist() == [0., 1., 2., 3.]
  # lo == hi, from the range and from the data
  assert diag.hist_edges(2, (3., 3.)).tolist() == [2.5, 3., 3.5]
  one = np.full(9, -7.25)
  assert diag.hist_edges(5, None, minmax=lambda: (-7.25, -7.25)).tobytes() == \
      np.histogram_bin_edges(one, 5).tobytes()


def test_hist_edges_refusals_are_numpys():
  a = np.arange(5.)
  lohi = lambda: (0., 4.)
  for nb, rng in ((0, None), (-3, (0., 1.)), (4, (2., 1.)), (4, (0., np.inf)), (4, (np.nan, 1.))):
    with pytest.raises(ValueError):
      np.histogram_bin_edges(a, nb, rng)
    with pytest.raises(ValueError):
      diag.hist_edges(nb, rng, minmax=lohi)
  # a data range that is not finite: np.histogram refuses such data too
  for lo, hi in ((np.nan, np.nan), (0., np.inf), (-np.inf, 0.)):
    with pytest.raises(ValueError):
      np.histogram_bin_edges(np.array([lo, hi]), 4)
    with pytest.raises(ValueError, match='not finite'):
      diag.hist_edges(4, None, minmax=lambda lo=lo, hi=hi: (lo, hi))
  with pytest.raises(TypeError):
    diag.hist_edges(2.5, (0., 1.))
  # edges: NumPy refuses what decreases; equal and infinite edges are refused here as well
  with pytest.raises(ValueError):
    np.histogram_bin_edges(a, [0., 2., 1.])
  for e in ([0., 2., 1.], [0., 1., 1.], [0., np.inf], [1.], [[0., 1.]]):
    with pytest.raises(ValueError):
      diag.hist_edges(e)
  # bins so many over a range so small that the edges repeat
  with pytest.raises(ValueError, match='strictly increasing'):
    diag.hist_edges(4, (1., np.nextafter(1., 2.)))
  with pytest.raises(ValueError, match='needs names'):
    diag.hist_edges({'x': 3}, (0., 1.))


def test_hist_edges_by_name():
  names = ['a', 'b', 'c']
  data = {'a': (-1., 2.), 'b': (5., 5.), 'c': (0., 1e-3)}
  calls = []

  def minmax():
    calls.append(1)
    return data

  got = diag.hist_edges(7, None, names, minmax)
  assert len(calls) == 1
  for k, e in zip(names, got):
    assert e.tobytes() == np.histogram_bin_edges(np.array(data[k]), 7).tobytes()
  got = diag.hist_edges({'a': 3, 'c': [0., 1., 10.]}, {'a': (0., 3.)}, names, minmax)
  assert got[1] is None and len(calls) == 1   # a has a range, c its edges: the data is not asked
  assert got[0].tolist() == [0., 1., 2., 3.] and got[2].tolist() == [0., 1., 10.]
  got = diag.hist_edges({'b': 2}, {'a': (0., 3.)}, names, minmax)
  assert got[0] is None and got[2] is None and got[1].tolist() == [4.5, 5., 5.5]
  got = diag.hist_edges(4, (0., 2.), names, minmax)
  assert all(e.tolist() == [0., .5, 1., 1.5, 2.] for e in got)
  got = diag.hist_edges(np.array([0., 1., 3.]), None, names, minmax)
  assert all(e.tolist() == [0., 1., 3.] for e in got) and len(calls) == 2
  for bins, rng in (({'z': 3}, None), (3, {'z': (0., 1.)}), ({'a': 0}, None), ({'a': 3}, {'a': (1., 0.)})):
    with pytest.raises(ValueError):
      diag.hist_edges(bins, rng, names, minmax)


def test_densities_are_numpys():
  rng = np.random.RandomState(4)
  a, b = rng.normal(size=4000), rng.normal(size=4000) * 2.
  for e in (np.linspace(-3., 3., 41), np.array([-4., -1., -0.5, 0., 2.5, 4.])):
    h, _ = np.histogram(a, e)
    ref, _ = np.histogram(a, e, density=True)
    assert diag.hist_density(h, e).tobytes() == ref.tobytes()
  ex, ey = np.linspace(-3., 3., 31), np.array([-5., -1., 0., 0.5, 6.])
  h = np.histogram2d(a, b, bins=[ex, ey])[0]
  ref = np.histogram2d(a, b, bins=[ex, ey], density=True)[0]
  assert diag.hist2d_density(h.astype(np.int64), ex, ey).tobytes() == ref.tobytes()
