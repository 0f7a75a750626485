"""pbh_trace_hist and pbh_trace_hist2d (Engine.trace_hist / trace_hist2d, Sampler.
trace_hist / trace_hist2d / trace_corner): the posterior histograms of a recorded
trace pooled over chains and records, computed on the device, against
np.histogram and np.histogram2d applied to the same trace copied to the host.

The reference is NumPy, never the code under test nor diag.py.  Every comparison
is integer equality: no tolerance, and nothing is left out of a comparison.

Shapes, the smallest at which each part can go wrong: N = 2 004 chains (no
multiple of 64 or 256: the last chain block is ragged), T = 160, windows (40,
120), (40, 119), (0, 4), (0, 1) and (7, 3), each asked twice (the counters are
cleared before every call); d = 10 and d = 2; d = 32 at 130 chains x 40 records
and 300 bins a dim, where the dims go in three groups; 33 000 chains of 8
records for more workgroups than counters; chains that never move, with every
value on an edge; a NaN and an infinite start; 129 grids of 128 x 128, more
counts than come back through the pinned stage."""
import numpy as np
import pytest
import scipy.stats

import oracle
import probayes_amd as pb
from oracle.workloads import golden_init
from probayes_amd import _lib
from probayes_amd._lib import PbhError
from mcmc_examples import WORKLOADS
from trace_helpers import (N_BIG, T_BIG, WINDOWS, big_run, check_no_side_effects, run,
                           sampler_block, tied_starts)

pytestmark = pytest.mark.gpu

HIST_WINDOWS = WINDOWS + ((0, 1), (7, 3))
MAX_BINS = 4096


def _pooled(x, k, first, count):
  return x[:, first:first + count, k].ravel()


def _check_hist(what, got, x, edges, first, count):
  """got against np.histogram of x's window, dim by dim"""
  n, d = x.shape[0], x.shape[2]
  assert len(got['counts']) == d and got['outside'].shape == (d, 3), what
  assert got['outside'].dtype == np.int64
  for k, e in enumerate(edges):
    if e is None:
      assert got['counts'][k] is None and list(got['outside'][k]) == [0, 0, 0], (what, k)
      continue
    a = _pooled(x, k, first, count)
    h = got['counts'][k]
    assert h.dtype == np.int64 and h.shape == (e.size - 1,), (what, k)
    assert np.array_equal(h, np.histogram(a, e)[0]), (what, k)
    assert list(got['outside'][k]) == [(a < e[0]).sum(), (a > e[-1]).sum(),
                                       np.isnan(a).sum()], (what, k)
    assert h.sum() + got['outside'][k].sum() == n * count, (what, k)


def _check_hist2d(what, got, x, edges, pairs, first, count):
  assert len(got) == len(pairs), what
  for (a, b), h in zip(pairs, got):
    ref = np.histogram2d(_pooled(x, a, first, count), _pooled(x, b, first, count),
                         bins=[edges[a], edges[b]])[0]
    assert h.dtype == np.int64 and h.shape == ref.shape, (what, a, b)
    assert np.array_equal(h, ref.astype(np.int64)), (what, a, b)


def _same(res, again):
  for h, g in zip(res['counts'], again['counts']):
    assert (h is None and g is None) or np.array_equal(h, g)
  assert np.array_equal(res['outside'], again['outside'])


def _quantile_edges(a, nb):
  """nb or fewer bins between quantiles of a: unevenly placed, strictly increasing"""
  e = np.unique(np.quantile(a[np.isfinite(a)], np.linspace(0.02, 0.98, nb + 1)))
  return e if e.size >= 2 else np.array([e[0] - 1., e[0] + 1.])


def _edge_sets(x):
  """the edge sets of a run from the host copy of its trace"""
  d = x.shape[2]
  flat = [x[:, :, k].ravel() for k in range(d)]
  lo, hi = [np.quantile(a, .1) for a in flat], [np.quantile(a, .9) for a in flat]
  uniform = [np.linspace(lo[k], hi[k], 51) for k in range(d)]
  placed = [_quantile_edges(flat[k], 40) for k in range(d)]
  geometric = [np.geomspace(1e-3, 1., 25) * (hi[k] - lo[k]) + lo[k] for k in range(d)]
  # some dims skipped, one dim at 1 bin, one at 4 096
  mixed = [None] * d
  mixed[0] = np.array([np.quantile(flat[0], .3), np.quantile(flat[0], .7)])
  mixed[d - 1] = np.linspace(flat[d - 1].min(), flat[d - 1].max(), MAX_BINS + 1)
  for k in range(2, d - 1, 2):
    mixed[k] = uniform[k] if k % 4 else geometric[k]
  # the pairs' edges: dim 0 evenly placed, the others by quantiles -- two lookups
  two = [np.linspace(lo[0], hi[0], 65)] + [_quantile_edges(flat[k], 64) for k in range(1, d)]
  return {'uniform': uniform, 'placed': placed, 'mixed': mixed, 'two': two}


PAIRS3 = [(0, 1), (1, 0), (0, 0)]


def _reduce(eng, first, count):
  """every edge set's histograms of a window, each asked twice, and the three
  pairs'; the edge sets are formed once per engine"""
  if not hasattr(eng, 'hist_test_sets'):
    eng.hist_test_sets = _edge_sets(eng.trace()['v_x'])
  sets = eng.hist_test_sets
  res = {'sets': sets}
  for key in ('uniform', 'placed', 'mixed'):
    res[key] = [eng.trace_hist(sets[key], first, count) for _ in range(2)]
  res['pairs'] = [eng.trace_hist2d(sets['two'], PAIRS3, first, count) for _ in range(2)]
  if (first, count) == HIST_WINDOWS[0]:
    d = eng.dim
    sq = [np.linspace(e[0], e[-1], 65) for e in sets['uniform']]
    every = [(a, b) for a in range(d) for b in range(a + 1, d)]
    res['every'] = (sq, every, eng.trace_hist2d(sq, every, first, count))
    limit = [np.linspace(e[0], e[-1], 129) for e in sets['uniform']]
    res['limit'] = (limit, eng.trace_hist2d(limit, [(d - 1, 0)], first, count))
  return res


def _big(name):
  return big_run(name, _reduce, HIST_WINDOWS)


@pytest.mark.parametrize('first,count', HIST_WINDOWS)
@pytest.mark.parametrize('name', ['diag10', 'gmm2'])
def test_against_np_histogram(name, first, count):
  spec, x, res = _big(name)
  assert x.shape == (N_BIG, T_BIG, spec['dim'])
  r = res[first, count]
  for key in ('uniform', 'placed', 'mixed'):
    got, again = r[key]
    _check_hist('{} {} {}'.format(name, key, (first, count)), got, x, r['sets'][key], first, count)
    _same(got, again)
  # draws lie below and above the evenly placed edges
  out = r['uniform'][0]['outside']
  if count >= 100:
    assert (out[:, 0] > 0).all() and (out[:, 1] > 0).all()
  assert (out[:, 2] == 0).all()


@pytest.mark.parametrize('first,count', HIST_WINDOWS)
@pytest.mark.parametrize('name', ['diag10', 'gmm2'])
def test_pairs_against_np_histogram2d(name, first, count):
  spec, x, res = _big(name)
  r = res[first, count]
  got, again = r['pairs']
  _check_hist2d('{} {}'.format(name, (first, count)), got, x, r['sets']['two'], PAIRS3, first,
                count)
  for h, g in zip(got, again):
    assert np.array_equal(h, g)
  assert np.array_equal(got[0], got[1].T)


@pytest.mark.parametrize('name', ['diag10', 'gmm2'])
def test_every_pair_and_the_cell_limit(name):
  spec, x, res = _big(name)
  first, count = HIST_WINDOWS[0]
  r = res[first, count]
  d = spec['dim']
  sq, every, got = r['every']
  assert len(every) == d * (d - 1) // 2 and all(h.shape == (64, 64) for h in got)
  _check_hist2d(name + ' every pair', got, x, sq, every, first, count)
  limit, got = r['limit']
  assert got[0].shape == (128, 128)
  _check_hist2d(name + ' 128 x 128', got, x, limit, [(d - 1, 0)], first, count)


def _diag_gauss(d, mu, sigma, scale):
  return pb.make_spec(d, {'kind': 'diag_gauss', 'mu': mu, 'sigma': sigma},
                      {'kind': 'gauss', 'scale': scale}, pscale='log')


def test_dim_groups():
  """d = 32 at 130 chains x 40 records and 300 bins a dim: three dim groups, one
  ragged chain block, a slice per record."""
  d = 32
  sigma, mu = np.linspace(0.5, 2.5, d), np.linspace(-2., 2., d)
  spec = _diag_gauss(d, mu, sigma, 0.4 * sigma)
  init = np.random.RandomState(d).normal(size=(130, d)) * sigma + mu
  even = [np.linspace(mu[k] - 2. * sigma[k], mu[k] + 2. * sigma[k], 301) for k in range(d)]
  eng = run(spec, init, 40)
  try:
    x = eng.trace()['v_x']
    placed = [_quantile_edges(x[:, :, k].ravel(), 300) if k % 3 else even[k] for k in range(d)]
    res = {(key, w): [eng.trace_hist(e, *w) for _ in range(2)]
           for key, e in (('even', even), ('placed', placed))
           for w in ((0, 40), (3, 37), (39, 1))}
    pairs = [(0, 31), (31, 5), (17, 17)]
    sq = [e[::6] for e in even]    # 50 bins
    grids = eng.trace_hist2d(sq, pairs, 3, 37)
  finally:
    eng.close()
  assert x.shape == (130, 40, d)
  for (key, (first, count)), (got, again) in res.items():
    _check_hist('d = 32 {} {}'.format(key, (first, count)), got, x,
                even if key == 'even' else placed, first, count)
    _same(got, again)
  _check_hist2d('d = 32', grids, x, sq, pairs, 3, 37)


def test_many_chains():
  """33 000 chains of 8 records at d = 10: 129 chain blocks of 8 slices, 1 032
  workgroups flushing into 1 030 counters: the 64-bit adds must meet the totals."""
  n, t = 33000, 8
  eng = run(oracle.golden_spec('diag10'), golden_init('diag10', n), t)
  try:
    x = eng.trace()['v_x']
    edges = [np.linspace(np.quantile(x[:, :, k], .05), np.quantile(x[:, :, k], .95), 101)
             for k in range(10)]
    got, part = eng.trace_hist(edges, 0, t), eng.trace_hist(edges, 2, 5)
    pairs = [(0, 9), (4, 3)]
    sq = [e[::2] for e in edges]
    grids = eng.trace_hist2d(sq, pairs, 1, 7)
  finally:
    eng.close()
  _check_hist('N = 33 000', got, x, edges, 0, t)
  _check_hist('N = 33 000 (2, 5)', part, x, edges, 2, 5)
  _check_hist2d('N = 33 000', grids, x, sq, pairs, 1, 7)


def _ladder(n):
  v = np.empty(n)
  v[0] = 1.
  for i in range(1, n):
    v[i] = np.nextafter(v[i - 1], 2.)
  return v


LAD = _ladder(130)
TIED_EDGES = {
    # the value on the first edge, on the last edge, on an inner one
    'one_value': [([-1., 0.], [0., 0.5]), ([-2., -1.], [0.5, 1.]), ([-2., -1., 3.], [0., 0.5, 1.]),
                  (np.linspace(-1., 1., 5), np.linspace(-0.5, 0.5, 65))],
    # every value on an edge: each double of the ladder, every third, the ends alone
    'last_ulps': [(LAD, -LAD[:5][::-1]), (LAD[::3], -LAD[:5][::-2]), (LAD[[0, 129]], -LAD[[4, 0]]),
                  (LAD[64:], -LAD[:3][::-1])],
    # edges that include 0.: -0.0, the denormals and +-1e300
    'top_bits': [([-1e300, -1., 0., 1., 1e300], [-1e-300, 0., 1e-300]),
                 ([-3., 0., 3.], [-5e-324, 0., 5e-324]), ([0., 1e300], [-1e300, -0.]),
                 (np.linspace(-1e300, 1e300, 9), np.linspace(-3., 3., 7))]}


@pytest.mark.parametrize('kind', sorted(TIED_EDGES))
def test_chains_that_never_move(kind):
  base = oracle.golden_spec('gmm2')
  spec = dict(base, proposal=dict(base['proposal'], scale=np.zeros(2)))
  x0 = tied_starts(kind)
  sets = [[np.asarray(e, float) for e in pair] for pair in TIED_EDGES[kind]]
  eng = run(spec, x0, 12)
  try:
    x = eng.trace()['v_x']
    assert x.shape == (130, 12, 2) and (x == x0[:, None, :]).all()   # the chains did not move
    # (the ladder's 129 bins against themselves are above the cell limit)
    pairs = [[(a, b) for a, b in PAIRS3 + [(1, 1)] if (e[a].size - 1) * (e[b].size - 1) <= 16384]
             for e in sets]
    res = [(eng.trace_hist(e, 0, 12), eng.trace_hist(e, 5, 1), eng.trace_hist2d(e, p, 0, 12))
           for e, p in zip(sets, pairs)]
  finally:
    eng.close()
  for e, p, (got, part, grids) in zip(sets, pairs, res):
    _check_hist(kind, got, x, e, 0, 12)
    _check_hist(kind + ' one record', part, x, e, 5, 1)
    assert len(p) >= 3
    _check_hist2d(kind, grids, x, e, p, 0, 12)
  if kind == 'last_ulps':
    # a bin per double, the last bin holding the two last doubles
    h = res[0][0]['counts'][0]
    assert list(h[:-1]) == [12] * 128 and h[-1] == 24 and res[0][0]['outside'].sum() == 0


def test_nan_and_infinite_starts():
  """The engine accepts a NaN and an infinite start, and with a proposal of scale
  0 the chains stay there: they are counted in `outside`, dropped from both
  dims' pairs, and the other dim is exact."""
  base = oracle.golden_spec('gmm2')
  spec = dict(base, proposal=dict(base['proposal'], scale=np.zeros(2)))
  x0 = np.repeat(np.array([[-1., 0.5], [0.25, 2.], [3., -1.]]), 2, axis=0)
  x0[4, 1] = np.nan
  x0[1, 0] = np.inf
  x0[3, 0] = -np.inf
  edges = [np.array([-1., 0., 0.25, 3.]), np.linspace(-1., 2., 7)]
  eng = run(spec, x0, 12)
  try:
    x = eng.trace()['v_x']
    assert np.array_equal(x, np.broadcast_to(x0[:, None, :], x.shape), equal_nan=True)
    got = eng.trace_hist(edges, 0, 12)
    grids = eng.trace_hist2d(edges, PAIRS3 + [(1, 1)], 2, 9)
  finally:
    eng.close()
  _check_hist('NaN and inf', got, x, edges, 0, 12)
  assert got['outside'].tolist() == [[12, 12, 0], [0, 0, 12]]
  assert got['counts'][0].tolist() == [12, 0, 36] and got['counts'][1].sum() == 60
  _check_hist2d('NaN and inf', grids, x, edges, PAIRS3 + [(1, 1)], 2, 9)
  # three of the six chains have both values inside the edges
  assert grids[0].sum() == 3 * 9 and grids[2].sum() == 4 * 9 and grids[3].sum() == 5 * 9


def test_more_counts_than_the_stage_takes():
  """129 grids of 128 x 128 are more than the 2^21 counts a pair call brings back
  through the pinned stage: they are copied to the caller after the wait."""
  eng = run(oracle.golden_spec('gmm2'), golden_init('gmm2', 130), 40)
  try:
    x = eng.trace()['v_x']
    edges = [np.linspace(np.quantile(x[:, :, k], .05), np.quantile(x[:, :, k], .95), 129)
             for k in range(2)]
    pairs = [(0, 1)] * 128 + [(1, 0)]
    assert sum(128 * 128 for _ in pairs) > 2 ** 21
    got = eng.trace_hist2d(edges, pairs, 3, 37)
    few = eng.trace_hist2d(edges, [(0, 1), (1, 0)], 3, 37)   # through the stage again
  finally:
    eng.close()
  _check_hist2d('129 grids', [got[0], got[-1]], x, edges, [(0, 1), (1, 0)], 3, 37)
  assert all(np.array_equal(g, got[0]) for g in got[:128])
  assert np.array_equal(few[0], got[0]) and np.array_equal(few[1], got[-1])


def test_no_side_effects():
  e = [np.linspace(-4., 4., 101), np.geomspace(0.01, 5., 30)]
  check_no_side_effects(lambda eng: (eng.trace_hist(e, 0, 64),
                                     eng.trace_hist2d(e, [(0, 1), (1, 1)], 0, 64)), 516)


def test_refusals_leave_the_engine_working():
  from probayes_amd import Engine
  import ctypes as c
  spec = oracle.golden_spec('gmm2')
  ok = np.linspace(-4., 4., 9)
  eng = Engine(spec)
  try:
    eng.init_chains(golden_init('gmm2', 6))
    eng.set_rng('philox', seed=3)
    with pytest.raises(PbhError, match='no trace'):
      eng.trace_hist([ok, ok], 0, 4)
    with pytest.raises(PbhError, match='no trace'):
      eng.trace_hist2d([ok, ok], [(0, 1)], 0, 4)
    eng.alloc_trace(40, 1)
    eng.run(40, steps_per_launch=64)
    big = np.arange(MAX_BINS + 2.)
    for edges, msg in (([None, None], 'every n_bins'),
                       ([ok, big], r'dim 1: n_bins = 4097'),
                       ([ok, [0., np.inf, 2.]], r'dim 1: edge 1 .*not finite'),
                       ([[np.nan, 1.], ok], r'dim 0: edge 0 .*not finite'),
                       ([ok, [0., 1., 1., 2.]], r'dim 1: edge 2 .*strictly increase'),
                       ([[0., -0., 1.], None], r'dim 0: edge 1 .*strictly increase')):
      with pytest.raises(PbhError, match=msg) as err:
        eng.trace_hist(edges, 0, 40)
      assert err.value.code == -1   # PBH_ERR_ARG
      with pytest.raises(PbhError, match=msg) as err:
        eng.trace_hist2d(edges, [(0, 0)], 0, 40)
      assert err.value.code == -1
    # a negative n_bins, which no list of arrays makes
    n_bins = np.array([8, -1], np.int32)
    out = np.zeros(64, np.int64)
    i64p = c.POINTER(c.c_int64)
    args = (eng._h, c.c_int64(0), c.c_int64(40), n_bins.ctypes.data_as(c.POINTER(c.c_int32)),
            ok.ctypes.data_as(c.POINTER(c.c_double)))
    with pytest.raises(PbhError, match=r'dim 1: n_bins = -1'):
      _lib.call('pbh_trace_hist', *args, out.ctypes.data_as(i64p), None)
    pair = np.zeros(2, np.int32)
    with pytest.raises(PbhError, match=r'dim 1: n_bins = -1'):
      _lib.call('pbh_trace_hist2d', *args, c.c_int32(1), pair.ctypes.data_as(c.POINTER(c.c_int32)),
                out.ctypes.data_as(i64p))
    wide = np.linspace(-4., 4., 130)
    for edges, pairs, msg in (([ok, ok], [], 'n_pairs = 0'),
                              ([ok, ok], [(0, 1), (2, 0)], r'pair 1: dim 2 outside'),
                              ([ok, ok], [(-1, 0)], r'pair 0: dim -1 outside'),
                              ([ok, None], [(0, 0), (0, 1)], r'pair 1: dim 1 has no edges'),
                              ([wide, wide[:-1]], [(1, 1), (0, 1)], r'pair 1: .*129 x 128')):
      with pytest.raises(PbhError, match=msg) as err:
        eng.trace_hist2d(edges, pairs, 0, 40)
      assert err.value.code == -1
    for kw, msg in ((dict(first=30, count=11), r'range \[30, 41\)'),
                    (dict(first=-1, count=8), r'range \[-1, 7\)'),
                    (dict(first=0, count=0), r'range \[0, 0\)')):
      with pytest.raises(PbhError, match=msg):
        eng.trace_hist([ok, ok], **kw)
      with pytest.raises(PbhError, match=msg):
        eng.trace_hist2d([ok, ok], [(0, 1)], **kw)
    for bad in ([ok], [ok, ok, ok], [ok, [1.]]):
      with pytest.raises(ValueError):
        eng.trace_hist(bad, 0, 40)
    x = eng.trace()['v_x']
    _check_hist('after refusals', eng.trace_hist([ok, None], 0, 40), x, [ok, None], 0, 40)
    _check_hist2d('after refusals', eng.trace_hist2d([wide[:-1], wide[:-1]], [(0, 1)], 0, 40), x,
                  [wide[:-1], wide[:-1]], [(0, 1)], 0, 40)
  finally:
    eng.close()


def test_the_sampler():
  n, t = 2004, 96
  with sampler_block(n, t) as (sampler, process, x, keys, v):
    pooled = {k: np.asarray(v[k]).ravel() for k in keys}
    assert list(keys) == list(sampler.names) and len(keys) >= 2
    # bins alone: the range is the pooled minimum and maximum, found on the device
    got = sampler.trace_hist(bins=40)
    dens = sampler.trace_hist(bins=40, density=True)
    assert set(got) == set(keys)
    for k in keys:
      h, e = np.histogram(pooled[k], 40)
      assert got[k][0].dtype == np.int64 and np.array_equal(got[k][0], h)
      assert got[k][1].tobytes() == e.tobytes()
      hd, ed = np.histogram(pooled[k], 40, density=True)
      assert dens[k][0].tobytes() == hd.tobytes() and dens[k][1].tobytes() == ed.tobytes()
    # a window, a range, dicts: a name left out is skipped
    a, b = keys[0], keys[1]
    win = {k: np.asarray(v[k])[8:95].ravel() for k in keys}
    lo, hi = np.quantile(win[a], [.2, .8])
    got = sampler.trace_hist(bins=25, range=(lo, hi), first=8, count=87)
    for k in keys:
      h, e = np.histogram(win[k], 25, range=(lo, hi))
      assert np.array_equal(got[k][0], h) and got[k][1].tobytes() == e.tobytes()
    mine = np.quantile(win[b], np.linspace(0., 1., 12))
    got = sampler.trace_hist(bins={b: mine}, first=8, count=87, density=True)
    assert set(got) == {b}
    hd, ed = np.histogram(win[b], mine, density=True)
    assert got[b][0].tobytes() == hd.tobytes() and got[b][1].tobytes() == ed.tobytes()
    got = sampler.trace_hist(bins={a: 7, b: 3}, range={a: (lo, hi)})
    assert np.array_equal(got[a][0], np.histogram(pooled[a], 7, range=(lo, hi))[0])
    assert np.array_equal(got[b][0], np.histogram(pooled[b], 3)[0])
    assert got[b][1].tobytes() == np.histogram(pooled[b], 3)[1].tobytes()
    # the joint histogram, every form of bins np.histogram2d takes
    ea, eb = np.linspace(lo, hi, 9), np.quantile(pooled[b], np.linspace(0.05, 0.9, 14))
    for bins, rng in ((12, None), ([6, 20], None), (ea, None), ([ea, eb], None),
                      (16, [[lo, hi], [eb[0], eb[-1]]]), ([5, eb], None)):
      for density in (False, True):
        H, xe, ye = sampler.trace_hist2d(a, b, bins=bins, range=rng, density=density)
        R, rx, ry = np.histogram2d(pooled[a], pooled[b], bins=bins, range=rng, density=density)
        assert H.dtype == R.dtype and H.tobytes() == R.tobytes(), (bins, rng, density)
        assert xe.tobytes() == rx.tobytes() and ye.tobytes() == ry.tobytes()
    H, xe, ye = sampler.trace_hist2d(b, a, bins=[eb, ea], first=8, count=87)
    assert H.tobytes() == np.histogram2d(win[b], win[a], bins=[eb, ea])[0].tobytes()
    # the corner: one call for the marginals, one for every pair
    corner = sampler.trace_corner(bins=30, first=8, count=87)
    alone = sampler.trace_hist(bins=30, first=8, count=87)
    assert corner['names'] == list(keys) and set(corner['hist']) == set(keys)
    for k in keys:
      assert np.array_equal(corner['hist'][k][0], alone[k][0])
      assert corner['hist'][k][1].tobytes() == alone[k][1].tobytes()
    want = [(p, q) for i, p in enumerate(keys) for q in keys[i + 1:]]
    assert list(corner['hist2d']) == want
    for p, q in want:
      H = sampler.trace_hist2d(p, q, bins=[alone[p][1], alone[q][1]], first=8, count=87)[0]
      assert corner['hist2d'][p, q].dtype == np.int64
      assert np.array_equal(corner['hist2d'][p, q], H)
    for call in (lambda: sampler.trace_hist(count=0), lambda: sampler.trace_hist(first=90, count=7),
                 lambda: sampler.trace_hist(bins=0), lambda: sampler.trace_hist(range=(2., 1.)),
                 lambda: sampler.trace_hist(bins={'nobody': 3}),
                 lambda: sampler.trace_hist2d(a, 'nobody'), lambda: sampler.trace_corner(bins={})):
      with pytest.raises(ValueError):
        call()
    # a second block: the engine's trace is no longer the first block's
    process.next(sampler)
    for call in (sampler.trace_hist, sampler.trace_corner, lambda: sampler.trace_hist2d(a, b)):
      with pytest.raises(ValueError, match='another block'):
        call()


def test_the_examples_last_lines_on_the_device():
  """mcmc_prob3's model at 2 004 chains: the example's histogram of the samples
  over its own xbins, divided as the example divides, from the device."""
  n, t = 2004, 96
  builder, params = WORKLOADS['mcmc_prob3'][:2]
  process, init, extra, kwds, keys = builder(pb, params)
  sampler = process.sampler(init, extra, stop=t, chains=n, rng='philox', seed=5, **kwds)
  try:
    samples = process.walk(sampler)
    xvals = np.asarray(process(samples).v['x'])
    assert xvals.size == n * t
    # the example's lines, on the copied values
    xbins = np.linspace(np.min(xvals), np.max(xvals), 128)
    xhist, _ = np.histogram(xvals, xbins)
    xprop = xhist / (xvals.size * (xbins[1] - xbins[0]))
    # the same from the device: the bins from the pooled range, no copy of the values
    got, edges = sampler.trace_hist(bins=127)['x']
    assert edges.tobytes() == xbins.tobytes() and np.array_equal(got, xhist)
    dev = got / (n * t * (edges[1] - edges[0]))
    assert dev.tobytes() == xprop.tobytes()
    again, _ = sampler.trace_hist(bins=xbins)['x']
    assert np.array_equal(again, xhist)
  finally:
    sampler.close()
  true = scipy.stats.uniform.pdf(xbins[:-1], loc=3., scale=4.)
  print('mcmc_prob3 at {} chains x {} steps: the largest distance of the histogram from the '
        'true density {:.4f} (density {:.2f})'.format(n, t, np.abs(dev - true).max(), 0.25))
