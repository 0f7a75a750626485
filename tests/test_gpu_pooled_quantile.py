"""pbh_trace_quantile_pooled (Engine.trace_quantile_pooled, Sampler.
trace_quantile_pooled): the quantiles of a recorded trace pooled over every
chain and record, found on the device by a radix select, against
diag.pooled_quantile (np.quantile's default method, written out) applied to
the same trace copied to the host.

Every comparison is np.array_equal: the device's state is integer counts, so
there is nothing to tolerate.  Nothing is left out of a comparison.

Shapes, the smallest at which each part can go wrong: N = 67 (no multiple of
64) with window (3, 37); N = 2 004, T = 160 with windows (40, 120), (40, 119)
and (0, 1); N = 1 with one record (M = 1); 1, 10 and 64 quantiles (64 make
more targets than the 16 groups counted in LDS, so the global counters and the
wave's single add run too); d = 2 and d = 10; 33 000 chains of 8 records for
several workgroups per dim and more than one unrolled round per thread.

Ties and every digit position run on the device with a Gaussian proposal of
scale 0, which leaves every chain at its start (as test_gpu_rhat.py's constant
chains): one value everywhere; a np.nextafter ladder from 1.0 (only the last
digit decides); starts that differ in the top bits only.  The engine accepts
a NaN start and the chain stays there, so the NaN rule runs on the device too.
"""
import numpy as np
import pytest

import oracle
from oracle.workloads import golden_init
from probayes_amd import diag
from probayes_amd._lib import PbhError
from trace_helpers import (N_BIG, Q64, QS, T_BIG, big_run, check_no_side_effects, run,
                           sampler_block, tied_starts)

pytestmark = pytest.mark.gpu

QSETS = {'qs': QS, 'one': [.5], 'q64': Q64}
WINDOWS = ((40, 120), (40, 119), (0, 1))


def _order_stats(x, q, first, count):
  """[nq, 2, d]: the sorted pooled values at lo and hi."""
  d = x.shape[2]
  s = np.sort(x[:, first:first + count, :].reshape(-1, d), axis=0)
  m = s.shape[0]
  lo = np.floor((m - 1.) * np.asarray(q, float)).astype(np.int64)
  hi = np.minimum(lo + 1, m - 1)
  return np.stack([s[lo], s[hi]], axis=1)


def _exact(what, got, x, q, first, count, equal_nan=False):
  quant, stats = got
  want = diag.pooled_quantile(x, q, first, count)
  assert quant.shape == want.shape == (len(q), x.shape[2]), what
  assert np.array_equal(quant, want, equal_nan=equal_nan), (what, quant, want)
  assert np.array_equal(stats, _order_stats(x, q, first, count), equal_nan=equal_nan), what


def _every_list_twice(eng, first, count):
  return {key: [eng.trace_quantile_pooled(q, first, count, order_stats=True) for _ in range(2)]
          for key, q in QSETS.items()}


def _big(name):
  """One run per model: the host copy of the trace and every device result,
  each asked for twice."""
  spec, x, res = big_run(name, _every_list_twice, WINDOWS)
  dev, again = ({(first, count, key): r[key][i] for (first, count), r in res.items()
                 for key in QSETS} for i in range(2))
  return spec, x, dev, again


@pytest.mark.parametrize('first,count', WINDOWS)
@pytest.mark.parametrize('name', ['diag10', 'gmm2'])
def test_continuous_data(name, first, count):
  spec, x, dev, _ = _big(name)
  assert x.shape == (N_BIG, T_BIG, spec['dim'])
  for key, q in QSETS.items():
    _exact('{} {} {}'.format(name, (first, count), key), dev[first, count, key], x, q, first,
           count)
  # the definition is NumPy's
  want = np.stack([np.quantile(x[:, first:first + count, k].ravel(), QS)
                   for k in range(spec['dim'])], axis=1)
  assert np.array_equal(dev[first, count, 'qs'][0], want)


@pytest.mark.parametrize('name', ['diag10', 'gmm2'])
def test_two_calls_give_the_same_bits(name):
  _, _, dev, again = _big(name)
  for key, a in dev.items():
    b = again[key]
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), key


@pytest.mark.parametrize('name', ['diag10', 'gmm2'])
def test_few_chains(name):
  spec = oracle.golden_spec(name)
  eng = run(spec, golden_init(name, 67), 40)
  try:
    x = eng.trace()['v_x']
    for key, q in QSETS.items():
      _exact('N = 67 ' + key, eng.trace_quantile_pooled(q, 3, 37, order_stats=True), x, q, 3, 37)
    only = eng.trace_quantile_pooled(QS, 3, 37)
    assert np.array_equal(only, diag.pooled_quantile(x, QS, 3, 37))
    whole = eng.trace_quantile_pooled(.5)   # a scalar q, the whole trace
    assert np.array_equal(whole, diag.pooled_quantile(x, [.5]))
  finally:
    eng.close()
  eng = run(spec, golden_init(name, 1), 1)
  try:
    x = eng.trace()['v_x']
    assert x.shape == (1, 1, spec['dim'])
    for key, q in QSETS.items():
      _exact('M = 1 ' + key, eng.trace_quantile_pooled(q, 0, 1, order_stats=True), x, q, 0, 1)
  finally:
    eng.close()


@pytest.mark.parametrize('kind', ['one_value', 'last_ulps', 'top_bits'])
def test_ties_and_every_digit(kind):
  base = oracle.golden_spec('gmm2')
  spec = dict(base, proposal=dict(base['proposal'], scale=np.zeros(2)))
  x0 = tied_starts(kind)
  eng = run(spec, x0, 12)
  try:
    x = eng.trace()['v_x']
    assert x.shape == (130, 12, 2) and (x == x0[:, None, :]).all()   # the chains did not move
    for key, q in QSETS.items():
      for first, count in ((0, 12), (5, 1)):
        _exact('{} {} {}'.format(kind, key, (first, count)),
               eng.trace_quantile_pooled(q, first, count, order_stats=True), x, q, first, count)
    quant, stats = eng.trace_quantile_pooled(QS, 0, 12, order_stats=True)
  finally:
    eng.close()
  assert not np.signbit(stats[stats == 0.]).any()   # zeros come back as +0.0
  if kind == 'one_value':
    assert np.array_equal(quant, np.broadcast_to(x0[0], (len(QS), 2)))


def test_a_nan_chain_makes_its_dim_nan():
  """The engine accepts a NaN start, and with a proposal of scale 0 the chain
  stays there: every quantile of that dim is NaN, the other dim's are exact,
  and the order statistics are the sorted values with the NaNs last."""
  base = oracle.golden_spec('gmm2')
  spec = dict(base, proposal=dict(base['proposal'], scale=np.zeros(2)))
  x0 = np.repeat(np.array([[-1., 0.5], [0.25, 2.], [3., -1.]]), 2, axis=0)
  x0[4, 1] = np.nan
  eng = run(spec, x0, 12)
  try:
    x = eng.trace()['v_x']
    assert np.array_equal(x, np.broadcast_to(x0[:, None, :], x.shape), equal_nan=True)
    for key, q in QSETS.items():
      got = eng.trace_quantile_pooled(q, 0, 12, order_stats=True)
      _exact('NaN chain ' + key, got, x, q, 0, 12, equal_nan=True)
      assert np.isnan(got[0][:, 1]).all() and np.isfinite(got[0][:, 0]).all()
      assert np.array_equal(got[0][:, 0], diag.pooled_quantile(x, q)[:, 0])
  finally:
    eng.close()


def test_many_chains():
  """33 000 chains of 8 records: 264 000 elements per dim, 33 workgroups per
  dim in the count kernel, each flushing its LDS histogram, and a tail after
  the unrolled rounds."""
  n, t = 33000, 8
  eng = run(oracle.golden_spec('gmm2'), golden_init('gmm2', n), t)
  try:
    x = eng.trace()['v_x']
    dev = {key: eng.trace_quantile_pooled(q, 0, t, order_stats=True) for key, q in QSETS.items()}
    odd = eng.trace_quantile_pooled(QS, 1, 7, order_stats=True)
  finally:
    eng.close()
  for key, q in QSETS.items():
    _exact('N = 33 000 ' + key, dev[key], x, q, 0, t)
  _exact('N = 33 000 (1, 7)', odd, x, QS, 1, 7)


def test_no_side_effects():
  def reduce(eng):
    eng.trace_quantile_pooled(QS, 3, 61)
    eng.trace_quantile_pooled(Q64, 0, 64, order_stats=True)

  check_no_side_effects(reduce, 516)


def test_refusals_leave_the_engine_working():
  from probayes_amd import Engine
  spec = oracle.golden_spec('gmm2')
  eng = Engine(spec)
  try:
    eng.init_chains(golden_init('gmm2', 12))
    eng.set_rng('philox', seed=3)
    with pytest.raises(PbhError, match='no trace'):
      eng.trace_quantile_pooled(QS, 0, 4)
    eng.alloc_trace(40, 1)
    eng.run(40, steps_per_launch=64)
    x = eng.trace()['v_x']
    bad = [(dict(q=QS, first=0, count=0), 'count = 0'),
           (dict(q=QS, first=30, count=11), r'range \[30, 41\)'),
           (dict(q=QS, first=-1, count=8), r'range \[-1, 7\)'),
           (dict(q=[], first=0, count=40), 'nq = 0'),
           (dict(q=list(np.linspace(0., 1., 65)), first=0, count=40), 'nq = 65'),
           (dict(q=[.5, -0.1], first=0, count=40), r'q\[1\]'),
           (dict(q=[1.1], first=0, count=40), r'q\[0\]'),
           (dict(q=[.25, .5, np.nan], first=0, count=40), r'q\[2\]')]
    for kw, msg in bad:
      with pytest.raises(PbhError, match=msg):
        eng.trace_quantile_pooled(**kw)
      # the next valid call on the same engine is still exact
      _exact('after ' + msg, eng.trace_quantile_pooled(QS, 2, 38, order_stats=True), x, QS, 2,
             38)
  finally:
    eng.close()


def test_sampler_trace_quantile_pooled():
  n, t = 67, 96
  with sampler_block(n, t) as (sampler, process, _, keys, v):
    got = sampler.trace_quantile_pooled(QS)
    assert set(got) == set(keys)
    for k in keys:
      vals = np.asarray(v[k])
      assert vals.size == n * t
      assert got[k].shape == (len(QS),)
      assert np.array_equal(got[k], np.quantile(vals.ravel(), QS)), k
    part = sampler.trace_quantile_pooled([.5], first=8, count=80)
    for k in keys:
      assert np.array_equal(part[k], np.quantile(np.asarray(v[k])[8:88].ravel(), [.5])), k
    for kw in (dict(count=0), dict(first=90, count=7), dict(first=-1)):
      with pytest.raises(ValueError):
        sampler.trace_quantile_pooled(QS, **kw)
    # a second block: the engine's trace is no longer the first block's
    process.next(sampler)
    with pytest.raises(ValueError, match='another block'):
      sampler.trace_quantile_pooled(QS)
