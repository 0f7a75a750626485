"""pbh_trace_rhat_rank (Engine.trace_rhat_rank, Sampler.trace_rhat_rank): the
rank-normalised and the folded split-R-hat of a recorded trace computed on the
device by a pooled radix sort, against rank_reference.py (scipy's rankdata and
ndtri, split-R-hat in longdouble) applied to the same trace copied to the host.

The ranks are compared with np.array_equal: the sort's state is integers, so
there is nothing to tolerate.  The two R-hat vectors must agree with the
longdouble reference relatively within max(64 eps, 32 x the distance of
diag.rank_rhat's own fp64 result on that copy from it) (rhat_reference.
device_bound); that bound covers the device's scores too (its log is not the
host's), which are not compared separately.  Nothing is left out of a
comparison, and each test prints what it measured before it asserts.

Shapes, the smallest at which each part can go wrong: N = 2 004 chains, T = 160
with windows (40, 120), (40, 119) and (0, 4) (M is no multiple of the 2 048-
element tile, tens of tiles, the rejected steps as ties); d = 10 and d = 2; N =
6 with window (3, 37) (less than one tile); N = 1; 130 chains of 12 records
that never move for ties and every digit; and test_many_elements for more
tiles than one chunk of the scan holds.
"""
import numpy as np
import pytest

import oracle
from oracle.workloads import golden_init
from probayes_amd import diag
from probayes_amd._lib import PbhError
from rank_reference import ref_rank_rhat, ref_ranks
from rhat_reference import device_bound, rel_dist
from trace_helpers import (N_BIG, Q64, T_BIG, WINDOWS, big_run, check_no_side_effects, flat,
                           run, sampler_block, tied_starts)

pytestmark = pytest.mark.gpu


def _median(x, first, count):
  return diag.pooled_quantile(x, [.5], first, count)[0]


def _exact_ranks(what, got, x, first, count, equal_nan=False):
  """both rank arrays of a device result against scipy's on the host copy"""
  shape = (x.shape[0], count, x.shape[2])
  for key, med in (('ranks', None), ('folded_ranks', _median(x, first, count))):
    want = ref_ranks(x, first, count, med)
    differ = int((got[key] != want).sum()) - int((np.isnan(got[key]) & np.isnan(want)).sum())
    print('{} {}: {} of {} ranks differ from scipy'.format(what, key, differ, want.size))
    assert got[key].shape == want.shape == shape, (what, key)
    assert np.array_equal(got[key], want, equal_nan=equal_nan), (what, key)


def _close_rhat(what, got, x, first, count):
  """bulk, folded and their maximum against the longdouble reference"""
  host = diag.rank_rhat(x, first, count)
  ref = ref_rank_rhat(x, first, count, _median(x, first, count))
  for key in ('bulk', 'folded'):
    bound, dist = device_bound(host[key], ref[key]), rel_dist(got[key], ref[key])
    print('{} {}: device - longdouble {:.3g}, diag.py - longdouble {:.3g}, bound {:.3g}'.format(
        what, key, dist, rel_dist(host[key], ref[key]), bound))
    assert got[key].shape == (x.shape[2],), (what, key)
    assert np.isfinite(bound), what
    assert dist <= bound, (what, key, dist, bound)
  assert got['rhat'].tobytes() == np.maximum(got['bulk'], got['folded']).tobytes(), what
  return host


def _with_ranks_twice_then_without(eng, first, count):
  return (eng.trace_rhat_rank(first, count, ranks=True),
          eng.trace_rhat_rank(first, count, ranks=True), eng.trace_rhat_rank(first, count))


def _big(name):
  """One run per model: the host copy of the trace and every device result,
  each asked for twice, and once without the ranks."""
  spec, x, res = big_run(name, _with_ranks_twice_then_without)
  dev, again, plain = ({w: r[i] for w, r in res.items()} for i in range(3))
  return spec, x, dev, again, plain


@pytest.mark.parametrize('first,count', WINDOWS)
@pytest.mark.parametrize('name', ['diag10', 'gmm2'])
def test_ranks_are_exact(name, first, count):
  spec, x, dev, _, _ = _big(name)
  assert x.shape == (N_BIG, T_BIG, spec['dim'])
  # MH traces hold runs of equal values (the rejected steps): both wanted
  rep = x[:, first + 1:first + count, 0] == x[:, first:first + count - 1, 0]
  assert rep.any() and not rep.all()
  _exact_ranks('{} {}'.format(name, (first, count)), dev[first, count], x, first, count)
  # the definition's ranks are the same
  assert np.array_equal(dev[first, count]['ranks'], diag.average_ranks(x, first, count))
  assert np.array_equal(dev[first, count]['folded_ranks'],
                        diag.average_ranks(x, first, count, fold=True))


@pytest.mark.parametrize('first,count', WINDOWS)
@pytest.mark.parametrize('name', ['diag10', 'gmm2'])
def test_rhat_per_dim(name, first, count):
  _, x, dev, _, plain = _big(name)
  got = dev[first, count]
  host = _close_rhat('{} {}'.format(name, (first, count)), got, x, first, count)
  assert np.isfinite(host['rhat']).all()
  # the device's scores are its ranks' scores: what the host makes of them
  # lies within the same bound of the reference (no tolerance of its own)
  m = N_BIG * count
  scored = {k: diag.split_rhat(diag.chain_moments(diag.normal_scores(got[r], m)), count // 2)
            for k, r in (('bulk', 'ranks'), ('folded', 'folded_ranks'))}
  assert scored['bulk'].tobytes() == host['bulk'].tobytes()
  assert scored['folded'].tobytes() == host['folded'].tobytes()
  # the result does not depend on whether the ranks were asked for
  for key in ('bulk', 'folded', 'rhat'):
    assert plain[first, count][key].tobytes() == got[key].tobytes(), key
  assert set(plain[first, count]) == {'bulk', 'folded', 'rhat'}


@pytest.mark.parametrize('name', ['diag10', 'gmm2'])
def test_two_calls_give_the_same_bits(name):
  _, _, dev, again, _ = _big(name)
  for key, a in dev.items():
    b = again[key]
    assert set(a) == set(b) == {'bulk', 'folded', 'rhat', 'ranks', 'folded_ranks'}
    for k in a:
      assert a[k].tobytes() == b[k].tobytes(), (key, k)


def test_few_chains():
  spec = oracle.golden_spec('gmm2')
  eng = run(spec, golden_init('gmm2', 6), 40)
  try:
    x = eng.trace()['v_x']
    got = eng.trace_rhat_rank(3, 37, ranks=True)
    whole = eng.trace_rhat_rank()
  finally:
    eng.close()
  _exact_ranks('N = 6', got, x, 3, 37)
  _close_rhat('N = 6', got, x, 3, 37)
  _close_rhat('N = 6, the whole trace', whole, x, 0, 40)
  eng = run(spec, golden_init('gmm2', 1), 40)
  try:
    x = eng.trace()['v_x']
    got = eng.trace_rhat_rank(0, 40, ranks=True)
  finally:
    eng.close()
  _exact_ranks('N = 1', got, x, 0, 40)
  _close_rhat('N = 1', got, x, 0, 40)


@pytest.mark.parametrize('kind', ['one_value', 'last_ulps', 'top_bits'])
def test_ties_and_every_digit(kind):
  """Chains that never move (a Gaussian proposal of scale 0): one value
  everywhere is one run of M and every pass skipped; a np.nextafter ladder
  lets only the lowest digit decide; starts that differ in sign, exponent,
  denormals and both zeros let the top digits decide."""
  base = oracle.golden_spec('gmm2')
  spec = dict(base, proposal=dict(base['proposal'], scale=np.zeros(2)))
  x0 = tied_starts(kind)
  eng = run(spec, x0, 12)
  try:
    x = eng.trace()['v_x']
    assert x.shape == (130, 12, 2) and (x == x0[:, None, :]).all()   # the chains did not move
    got = eng.trace_rhat_rank(0, 12, ranks=True)
    part = eng.trace_rhat_rank(5, 4, ranks=True)
  finally:
    eng.close()
  _exact_ranks(kind, got, x, 0, 12)
  _exact_ranks(kind + ' (5, 4)', part, x, 5, 4)
  if kind == 'one_value':
    assert (got['ranks'] == (130 * 12 + 1) / 2.).all()
  # constant chains: W = 0, so inf or NaN exactly as the definition gives
  host = diag.rank_rhat(x, 0, 12)
  for key in ('bulk', 'folded', 'rhat'):
    print(kind, key, got[key], host[key])
    assert not np.isfinite(host[key]).any()
    assert np.array_equal(got[key], host[key], equal_nan=True), (kind, key)


def test_a_nan_chain_makes_its_dim_nan():
  """The engine accepts a NaN start, and with a proposal of scale 0 the chain
  stays there: every rank and both statistics of that dim are NaN, the other
  dim's ranks are exact."""
  base = oracle.golden_spec('gmm2')
  spec = dict(base, proposal=dict(base['proposal'], scale=np.zeros(2)))
  x0 = np.repeat(np.array([[-1., 0.5], [0.25, 2.], [3., -1.]]), 2, axis=0)
  x0[4, 1] = np.nan
  eng = run(spec, x0, 12)
  try:
    x = eng.trace()['v_x']
    assert np.array_equal(x, np.broadcast_to(x0[:, None, :], x.shape), equal_nan=True)
    got = eng.trace_rhat_rank(0, 12, ranks=True)
  finally:
    eng.close()
  for key in ('ranks', 'folded_ranks'):
    assert np.isnan(got[key][:, :, 1]).all() and np.isfinite(got[key][:, :, 0]).all(), key
  _exact_ranks('NaN chain', got, x, 0, 12, equal_nan=True)
  host = diag.rank_rhat(x, 0, 12)
  for key in ('bulk', 'folded', 'rhat'):
    print('NaN chain', key, got[key], host[key])
    assert np.isnan(got[key][1]), key
    assert np.array_equal(got[key], host[key], equal_nan=True), key


def test_many_elements():
  """33 000 chains: 8 records are M = 264 000 elements in 129 tiles, one tile
  per chunk of the scan (at most 256 chunks); 16 records are M = 528 000
  elements in 258 tiles, just above 256, so a chunk holds two tiles and the
  chunk and tile kernels loop.  (15 records: 242 tiles and an odd count.)"""
  n, t = 33000, 16
  eng = run(oracle.golden_spec('gmm2'), golden_init('gmm2', n), t)
  try:
    x = eng.trace()['v_x']
    dev = {w: eng.trace_rhat_rank(w[0], w[1], ranks=True) for w in ((0, 8), (0, 16), (1, 15))}
  finally:
    eng.close()
  for (first, count), got in dev.items():
    _exact_ranks('N = 33 000 {}'.format((first, count)), got, x, first, count)
  _close_rhat('N = 33 000 (0, 16)', dev[0, 16], x, 0, 16)


def test_no_side_effects():
  def reduce(eng):
    eng.trace_rhat_rank(3, 61, ranks=True)
    eng.trace_rhat_rank(3, 60)

  check_no_side_effects(reduce, 516)


def test_results_do_not_depend_on_what_the_scratch_held():
  """Two engines with one seed make the same four calls on the shared
  reduction scratch, one in this order and one in reverse: the same bits."""
  calls = [
      ('rank', lambda e: e.trace_rhat_rank()),
      ('pooled_64', lambda e: e.trace_quantile_pooled(Q64, order_stats=True)),
      ('rhat_2', lambda e: e.trace_rhat(group=2, stats=True)),
      ('rank_ranks', lambda e: e.trace_rhat_rank(ranks=True)),
  ]
  n, t = 130, 70
  spec = oracle.golden_spec('gmm2')
  got, traces = [], []
  for order in (calls, calls[::-1]):
    eng = run(spec, golden_init('gmm2', n), t)
    try:
      got.append({name: call(eng) for name, call in order})
      traces.append(eng.trace()['v_x'])
    finally:
      eng.close()
  a, b = got
  assert np.array_equal(traces[0], traces[1])
  for name, _ in calls:
    fa, fb = flat(a[name]), flat(b[name])
    assert len(fa) == len(fb) > 0, name
    for u, v in zip(fa, fb):
      assert u.shape == v.shape and u.tobytes() == v.tobytes(), name
  # and they are the host's definitions on the trace copied out
  x = traces[0]
  for res in got:
    _exact_ranks('after other reductions', res['rank_ranks'], x, 0, t)
    _close_rhat('after other reductions', res['rank'], x, 0, t)
    for key in ('bulk', 'folded', 'rhat'):
      assert res['rank'][key].tobytes() == res['rank_ranks'][key].tobytes(), key
    assert np.array_equal(res['pooled_64'][0], diag.pooled_quantile(x, Q64))


def test_refusals_leave_the_engine_working():
  from probayes_amd import Engine
  spec = oracle.golden_spec('gmm2')
  eng = Engine(spec)
  try:
    eng.init_chains(golden_init('gmm2', 12))
    eng.set_rng('philox', seed=3)
    with pytest.raises(PbhError, match='no trace'):
      eng.trace_rhat_rank(0, 4)
    eng.alloc_trace(40, 1)
    eng.run(40, steps_per_launch=64)
    x = eng.trace()['v_x']
    bad = [(dict(first=30, count=11), r'range \[30, 41\)'),
           (dict(first=-1, count=8), r'range \[-1, 7\)'),
           (dict(first=0, count=3), 'count = 3'),
           (dict(first=0, count=0), 'count = 0')]
    for kw, msg in bad:
      with pytest.raises(PbhError, match=msg):
        eng.trace_rhat_rank(**kw)
      # the next valid call on the same engine is still right
      got = eng.trace_rhat_rank(2, 38, ranks=True)
      _exact_ranks('after ' + msg, got, x, 2, 38)
      _close_rhat('after ' + msg, got, x, 2, 38)
  finally:
    eng.close()


def test_sampler_trace_rhat_rank():
  n, t = 68, 96
  with sampler_block(n, t) as (sampler, process, x, keys, _):
    got = sampler.trace_rhat_rank(8, 87)
    assert set(got) == {'bulk', 'folded', 'rhat'} and set(got['rhat']) == set(keys)
    _close_rhat('sampler', {k: np.array([got[k][name] for name in keys]) for k in got}, x, 8, 87)
    whole = sampler.trace_rhat_rank()
    _close_rhat('sampler, the whole block',
                {k: np.array([whole[k][name] for name in keys]) for k in whole}, x, 0, t)
    for kw in (dict(count=3), dict(first=90, count=7), dict(first=-1)):
      with pytest.raises(ValueError):
        sampler.trace_rhat_rank(**kw)
    # a second block: the engine's trace is no longer the first block's
    process.next(sampler)
    with pytest.raises(ValueError, match='another block'):
      sampler.trace_rhat_rank()
