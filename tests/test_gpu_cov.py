"""pbh_trace_cov (Engine.trace_cov, Sampler.trace_cov, Sampler.trace_tran): the
posterior mean, covariance and correlation of a recorded trace pooled over
chains and records, computed on the device, against the longdouble two-pass
restatement of cov_reference.py applied to the same trace copied to the host.

The reference is never the code under test.  The device's three results must
agree with it, each in its own unit (cov_reference: sqrt(cov_aa cov_bb) for the
covariance, |mean_a| + sqrt(cov_aa) for the mean, 1 for the correlation),
within max(64 eps, 32 x the distance of diag.pooled_cov's own fp64 result on
that copy from it) (cov_reference.device_bounds); nothing is left out of a
comparison, and equal zeros, infinities and NaNs are at distance 0.  Each test
prints the distances it measured before it asserts.

Shapes, the smallest at which each part can go wrong: N = 2 004 chains (no
multiple of 64 or 256: the last chain block is ragged), T = 160; windows (40,
120), (40, 119), (0, 4), (0, 1) and (7, 3); d = 10 and d = 2; d = 16, 20, 24 and
32 at 130 chains x 40 records, where one tile is full, the second tile and the
two rectangles hold 4 dims of their 16 and 8 columns, the second tile is half
full beside full rectangles, and both tiles and all four rectangles are full (the
engine runs no dims between 16 and 20: the tiling at d = 17 is tested on the
host, test_cov_host.py), and where few chains put the record slices and a
partial block to work; the same dims at enough chains that a
slice is longer than the records a lane keeps in flight (test_long_slices: up
to there every slice is shorter); 33 000 chains of 8 records for more partial
rows than the finish has threads; N = 1 with 2 records and N = 6.

The tuned run at the end is the use the matrix is for: a first block under an
isotropic proposal, Sampler.trace_tran of its second half into RF.set_tran, and
a second sampler from the first one's last states."""
import functools

import numpy as np
import pytest
import scipy.stats

import oracle
import probayes_amd as pb
from oracle.workloads import golden_init
from probayes_amd import diag
from probayes_amd._lib import PbhError
from cov_reference import device_bounds, dists, ref_cov
from rhat_reference import EPS
from trace_helpers import (N_BIG, T_BIG, WINDOWS, big_run, check_no_side_effects, run,
                           sampler_block, tied_starts)

pytestmark = pytest.mark.gpu

COV_WINDOWS = WINDOWS + ((0, 1), (7, 3))
KEYS = ('mean', 'cov', 'corr')


def _twice(eng, first, count):
  return [eng.trace_cov(first, count) for _ in range(2)]


def _big(name):
  """One run per model: the spec, the host copy of the trace and every window's
  device result, each asked for twice."""
  return big_run(name, _twice, COV_WINDOWS)


@functools.lru_cache(maxsize=None)
def _refs(name, first, count):
  x = _big(name)[1]
  return ref_cov(x, first, count), diag.pooled_cov(x, first, count)


def _close(what, got, x, first, count, refs=None):
  """got against the longdouble covariance of x's window, within the bound"""
  ref, host = refs or (ref_cov(x, first, count), diag.pooled_cov(x, first, count))
  d = x.shape[2]
  assert got['mean'].shape == (d,) and got['cov'].shape == got['corr'].shape == (d, d)
  bound, dist, own = device_bounds(host, ref), dists(got, ref), dists(host, ref)
  for k in KEYS:
    print('{} {}: device - longdouble {:.3g} eps, diag.py - longdouble {:.3g} eps, bound '
          '{:.3g} eps'.format(what, k, dist[k] / EPS, own[k] / EPS, bound[k] / EPS))
  for k in KEYS:
    assert np.isfinite(bound[k]), (what, k)
    assert dist[k] <= bound[k], (what, k, dist[k] / EPS, bound[k] / EPS)
  assert got['cov'].tobytes() == got['cov'].T.copy().tobytes(), what
  assert got['corr'].tobytes() == got['corr'].T.copy().tobytes(), what


@pytest.mark.parametrize('first,count', COV_WINDOWS)
@pytest.mark.parametrize('name', ['diag10', 'gmm2'])
def test_against_the_reference(name, first, count):
  spec, x, res = _big(name)
  assert x.shape == (N_BIG, T_BIG, spec['dim'])
  got, again = res[first, count]
  _close('{} {}'.format(name, (first, count)), got, x, first, count, _refs(name, first, count))
  assert np.array_equal(np.diagonal(got['corr']), np.ones(spec['dim']))
  # two calls give the same bits
  for k in KEYS:
    assert got[k].tobytes() == again[k].tobytes(), k


def _diag_gauss(d, mu, sigma, scale):
  return pb.make_spec(d, {'kind': 'diag_gauss', 'mu': mu, 'sigma': sigma},
                      {'kind': 'gauss', 'scale': scale}, pscale='log')


@pytest.mark.parametrize('d', [16, 20, 24, 32])
def test_tile_edges(d):
  """130 chains x 40 records: one ragged chain block, a slice per record, and
  the dims at which the tiling changes."""
  sigma = np.linspace(0.5, 2.5, d)
  spec = _diag_gauss(d, np.linspace(-2., 2., d), sigma, 0.4 * sigma)
  init = np.random.RandomState(d).normal(size=(130, d)) * sigma + np.linspace(-2., 2., d)
  eng = run(spec, init, 40)
  try:
    x = eng.trace()['v_x']
    res = {w: _twice(eng, *w) for w in ((0, 40), (3, 37), (39, 1))}
  finally:
    eng.close()
  assert x.shape == (130, 40, d)
  for (first, count), (got, again) in res.items():
    _close('d = {} {}'.format(d, (first, count)), got, x, first, count)
    for k in KEYS:
      assert got[k].tobytes() == again[k].tobytes(), k


@pytest.mark.parametrize('d,n,count', [(2, 262044, 19), (10, 262044, 6), (16, 262044, 4),
                                       (20, 65436, 7), (32, 43676, 4)])
def test_long_slices(d, n, count):
  """Enough chain blocks that a slice is the whole window, and a window longer
  than the records a lane loads ahead (8, 4 and 3 at d = 2, 10 and 16; 3 in the
  diagonal tiles and in the rectangles above): the loop that keeps several
  records in flight runs, twice at d = 2 and d = 20, and the one-record loop
  behind it takes what is left.  The last chain block is
  ragged."""
  sigma = np.linspace(0.5, 2.5, d)
  mu = np.linspace(-2., 2., d)
  spec = _diag_gauss(d, mu, sigma, 0.4 * sigma)
  init = np.random.RandomState(d).normal(size=(n, d)) * sigma + mu
  eng = run(spec, init, count)
  try:
    x = eng.trace()['v_x']
    got, again = _twice(eng, 0, count)
  finally:
    eng.close()
  _close('d = {} N = {}'.format(d, n), got, x, 0, count)
  for k in KEYS:
    assert got[k].tobytes() == again[k].tobytes(), k


def test_many_chains():
  """33 000 chains of 8 records at d = 10: 129 chain blocks of 8 slices, 1 032
  partial rows against the finish's 256 threads; the shift's 1 024 threads take
  a third sweep of the chains."""
  n, t = 33000, 8
  spec = oracle.golden_spec('diag10')
  eng = run(spec, golden_init('diag10', n), t)
  try:
    x = eng.trace()['v_x']
    got = eng.trace_cov(0, t)
    part = eng.trace_cov(2, 5)
  finally:
    eng.close()
  _close('N = 33 000', got, x, 0, t)
  _close('N = 33 000 (2, 5)', part, x, 2, 5)


def test_smallest_shapes():
  spec = oracle.golden_spec('gmm2')
  eng = run(spec, golden_init('gmm2', 1), 40)
  try:
    x = eng.trace()['v_x']
    r = int(np.flatnonzero((x[0, 1:] != x[0, :-1]).any(axis=1))[0])   # two draws that differ
    _close('N = 1, count = 2', eng.trace_cov(r, 2), x, r, 2)
    _close('N = 1', eng.trace_cov(), x, 0, 40)
  finally:
    eng.close()
  eng = run(spec, golden_init('gmm2', 6), 40)
  try:
    x = eng.trace()['v_x']
    _close('N = 6', eng.trace_cov(3, 37), x, 3, 37)
  finally:
    eng.close()


def test_large_mean():
  """A posterior at 1e6 (1 .. d) with unit spread: sums of raw products would
  keep no digit of the covariance (test_cov_diag.py shows it on the host)."""
  d = 4
  mu = 1e6 * np.arange(1., d + 1.)
  spec = _diag_gauss(d, mu, np.ones(d), 0.7 * np.ones(d))
  eng = run(spec, np.repeat(mu[None, :], 516, axis=0), 96)
  try:
    x = eng.trace()['v_x']
    got = eng.trace_cov(32, 64)
  finally:
    eng.close()
  assert np.abs(x[:, 32:] - mu).max() < 20. and x[:, 32:, 0].std() > 0.3
  _close('mean 1e6', got, x, 32, 64)


@pytest.mark.parametrize('kind', ['one_value', 'last_ulps'])
def test_chains_that_never_move(kind):
  base = oracle.golden_spec('gmm2')
  spec = dict(base, proposal=dict(base['proposal'], scale=np.zeros(2)))
  x0 = tied_starts(kind)
  eng = run(spec, x0, 12)
  try:
    x = eng.trace()['v_x']
    assert x.shape == (130, 12, 2) and (x == x0[:, None, :]).all()   # the chains did not move
    got, part = eng.trace_cov(0, 12), eng.trace_cov(5, 1)
  finally:
    eng.close()
  for what, res, first, count in (('all', got, 0, 12), ('one record', part, 5, 1)):
    if kind == 'one_value':
      assert np.array_equal(res['cov'], np.zeros((2, 2))), res['cov']
      assert not np.signbit(res['cov']).any()
      assert np.isnan(res['corr']).all(), res['corr']
      assert np.array_equal(res['mean'], x0[0]), res['mean']
    _close('{} {}'.format(kind, what), res, x, first, count)


def test_no_side_effects():
  check_no_side_effects(lambda eng: eng.trace_cov(0, 64), 516)


def test_refusals_leave_the_engine_working():
  from probayes_amd import Engine
  spec = oracle.golden_spec('gmm2')
  eng = Engine(spec)
  try:
    eng.init_chains(golden_init('gmm2', 1))
    eng.set_rng('philox', seed=3)
    with pytest.raises(PbhError, match='no trace'):
      eng.trace_cov(0, 4)
    eng.alloc_trace(40, 1)
    eng.run(40, steps_per_launch=64)
    for kw, msg in ((dict(first=30, count=11), r'range \[30, 41\)'),
                    (dict(first=-1, count=8), r'range \[-1, 7\)'),
                    (dict(first=0, count=0), r'range \[0, 0\)'),
                    (dict(first=4, count=1), 'at least 2 draws')):   # N count = 1
      with pytest.raises(PbhError, match=msg) as err:
        eng.trace_cov(**kw)
      assert err.value.code == -1   # PBH_ERR_ARG
    x = eng.trace()['v_x']
    _close('after refusals', eng.trace_cov(0, 40), x, 0, 40)
  finally:
    eng.close()


def test_sampler_trace_cov():
  n, t = 130, 96
  with sampler_block(n, t) as (sampler, process, x, keys, _):
    got = sampler.trace_cov(8, 87)
    assert set(got) == {'names', 'mean', 'cov', 'corr'}
    assert got['names'] == list(keys) == list(sampler.names)
    eng = sampler._eng.trace_cov(8, 87)
    assert [got['mean'][k] for k in keys] == list(eng['mean'])
    assert got['cov'].tobytes() == eng['cov'].tobytes()
    assert got['corr'].tobytes() == eng['corr'].tobytes()
    _close('sampler', dict(eng, mean=np.array([got['mean'][k] for k in keys])), x, 8, 87)
    _close('sampler, the block', sampler._eng.trace_cov(), x, 0, t)
    assert sampler.trace_cov()['cov'].tobytes() == sampler._eng.trace_cov()['cov'].tobytes()
    for kw in (dict(count=0), dict(first=90, count=7), dict(first=-1)):
      with pytest.raises(ValueError):
        sampler.trace_cov(**kw)
    # this sampler's sigma steps through a ufun: its trace has a covariance,
    # its proposal takes none
    with pytest.raises(ValueError, match='ufun'):
      sampler.trace_tran()
    # a second block: the engine's trace is no longer the first block's
    process.next(sampler)
    with pytest.raises(ValueError, match='another block'):
      sampler.trace_cov()


# ---- the tuned run ------------------------------------------------------------
R = 0.95
N_TUNE, T_TUNE = 2004, 400


def correlated2(tran):
  """A user-written density of two variables with correlation R, through the
  expression target, under a covariance random walk: N(0, 1) deltas per
  variable times the Cholesky factor of `tran` (RF.set_tran)."""
  x = pb.RV('x', vtype=float, vset=(-10., 10.))
  y = pb.RV('y', vtype=float, vset=(-10., 10.))
  rf = pb.RF(x, y)
  rf.set_tran(tran)
  rf.set_delta(lambda: rf.Delta(x=scipy.stats.norm.rvs(), y=scipy.stats.norm.rvs()))
  process = pb.SP(rf)
  process.set_prob(lambda x, y: -0.5 * (x * x - 2 * R * x * y + y * y) / (1 - R * R),
                   pscale='log')
  process.set_tran('leafs')
  process.set_delta('leafs')
  process.set_scores('hastings')
  process.set_update('metropolis')
  return process


def _stage(tran, init, seed):
  """One sampler of T_TUNE steps: (sampler, process, last values per chain)."""
  process = correlated2(tran)
  sampler = process.sampler(init, stop=T_TUNE, chains=N_TUNE, rng='philox', seed=seed)
  samples = process.walk(sampler)
  assert len(samples) == T_TUNE
  v = process(samples).v
  return sampler, process, {k: np.array(np.asarray(v[k])[-1]) for k in ('x', 'y')}


def test_tuned_run_end_to_end():
  iso = 0.05 * np.eye(2)
  a, _, last = _stage(iso, {'x': 0., 'y': 0.}, seed=11)
  try:
    assert a.spec['target']['kind'] == 'expr'
    tran = a.trace_tran(first=T_TUNE // 2)
    cov = a.trace_cov(first=T_TUNE // 2)
    ess_a = a.trace_ess_rank()['bulk']
  finally:
    a.close()
  assert last['x'].shape == (N_TUNE,)
  print('Sigma-hat of stage A\'s second half: {}, corr {:.4f}'.format(
      cov['cov'].tolist(), cov['corr'][0, 1]))
  assert tran.tobytes() == (2.38 ** 2 / 2 * cov['cov']).tobytes()

  b, _, _ = _stage(tran, last, seed=12)
  try:
    # the matrix reached the kernels as its Cholesky factor
    assert b.spec['proposal']['tfun'].tobytes() == np.linalg.cholesky(tran).tobytes()
    # B starts where A stopped, chain by chain
    assert np.array_equal(b._init_array(), np.stack([last['x'], last['y']], axis=1))
    acc_b = b._eng.trace()['u'][:, 1:].mean()   # (the first step accepts by rule)
    ess_b = b.trace_ess_rank()['bulk']
  finally:
    b.close()

  a2, _, _ = _stage(iso, last, seed=12)   # A': A's proposal over the same steps
  try:
    acc_a2 = a2._eng.trace()['u'][:, 1:].mean()
    ess_a2 = a2.trace_ess_rank()['bulk']
  finally:
    a2.close()
  lo_b, lo_a2 = min(ess_b.values()), min(ess_a2.values())
  print('acceptance: tuned {:.4f}, isotropic {:.4f}'.format(acc_b, acc_a2))
  print('min bulk-ESS over names: stage A {:.0f}, tuned B {:.0f}, isotropic A\' {:.0f}, '
        'ratio B / A\' {:.2f}'.format(min(ess_a.values()), lo_b, lo_a2, lo_b / lo_a2))
  # 0.35 is the rate of an optimally scaled Gaussian random walk at d = 2
  # (Gelman, Roberts & Gilks 1996); the interval leaves room for Sigma-hat's error
  assert 0.2 <= acc_b <= 0.5, acc_b
  # the direction theory fixes (Roberts & Rosenthal 2001: the inhomogeneity
  # factor is >= 1); the size of the ratio is a measurement
  assert lo_b >= lo_a2, (lo_b, lo_a2)
