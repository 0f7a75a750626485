"""pbh_trace_rhat (Engine.trace_rhat, Sampler.trace_rhat): split-R-hat and
nested R-hat of a recorded trace computed on the device, against the
longdouble restatement of rhat_reference.py applied to the same trace copied
to the host.

The reference is never the code under test.  The device's per-chain rows and
its two R-hat vectors must agree with it relatively within max(64 eps, 32 x
the distance of diag.py's own fp64 result on that copy from it)
(rhat_reference.device_bound); nothing is left out of a comparison, and equal
zeros, infinities and NaNs are at distance 0.  Each test prints the distances
it measured before it asserts.

Shapes, the smallest at which each part can go wrong: N = 2 004 chains (no
multiple of 64 or 256, divisible by 4 and 12), T = 160; windows (40, 120),
(40, 119) (odd: the middle record dropped) and (0, 4) (h = 2, where halves of
two equal records have variance exactly 0); group 1, 4, 12 (a thread per
superchain), 167 and N / 2 = 1 002 (a workgroup per superchain, below and above
its width); d = 10 and d = 2; N = 6 with group 3; N = 1 (split only); and
33 000 chains of 8 records for the paths only many chains reach
(test_many_chains).

The constant-chain case runs on the device: a Gaussian proposal of scale 0
leaves every chain at its start (the golden specs have no uniform delta; this
is their equivalent).
"""
import functools

import numpy as np
import pytest

import oracle
from oracle.workloads import golden_init
from probayes_amd import diag
from probayes_amd._lib import PbhError
from rhat_reference import device_bound, ref_moments, ref_nested, ref_split, rel_dist
from trace_helpers import N_BIG, WINDOWS, big_run, check_no_side_effects, run, sampler_block

pytestmark = pytest.mark.gpu

GROUPS = [1, 4, 12, 167, N_BIG // 2]


def _every_group_twice(eng, first, count):
  return {g: [eng.trace_rhat(first, count, g, stats=True) for _ in range(2)] for g in GROUPS}


def _big(name):
  """One run per model: the host copy of the trace and every device result,
  each asked for twice."""
  spec, x, res = big_run(name, _every_group_twice)
  dev, again = ({(first, count, g): r[g][i] for (first, count), r in res.items() for g in GROUPS}
                for i in range(2))
  return spec, x, dev, again


@functools.lru_cache(maxsize=None)
def _refs(name, first, count):
  """The longdouble rows and diag.py's fp64 rows of one window, computed once."""
  x = _big(name)[1]
  return ref_moments(x, first, count), diag.chain_moments(x, first, count)


def _close(what, got, host, ref):
  bound, dist = device_bound(host, ref), rel_dist(got, ref)
  print('{}: device - longdouble {:.3g}, diag.py - longdouble {:.3g}, bound {:.3g}'.format(
      what, dist, rel_dist(host, ref), bound))
  assert np.isfinite(bound), what
  assert dist <= bound, (what, dist, bound)


@pytest.mark.parametrize('first,count', WINDOWS)
@pytest.mark.parametrize('name', ['diag10', 'gmm2'])
def test_chain_stats_per_chain(name, first, count):
  spec, x, dev, _ = _big(name)
  ref, host = _refs(name, first, count)
  got = dev[first, count, 1]['stats']
  assert got.shape == (6, N_BIG, spec['dim'])
  # MH traces hold runs of equal values (the rejected steps): both wanted
  rep = x[:, first + 1:first + count, 0] == x[:, first:first + count - 1, 0]
  assert rep.any() and not rep.all()
  for i, row in enumerate(diag.ROWS):
    _close('{} {} {}'.format(name, (first, count), row), got[i], host[i], ref[i])
  for g in GROUPS:   # the rows do not depend on what else was asked for
    assert dev[first, count, g]['stats'].tobytes() == got.tobytes(), g


@pytest.mark.parametrize('first,count', WINDOWS)
@pytest.mark.parametrize('name', ['diag10', 'gmm2'])
def test_rhat_per_dim(name, first, count):
  spec, x, dev, _ = _big(name)
  host = _refs(name, first, count)[1]
  want = ref_split(x, first, count)
  assert np.isfinite(np.asarray(want, float)).all()
  for g in GROUPS:
    got = dev[first, count, g]
    assert got['split'].shape == got['nested'].shape == (spec['dim'],)
    _close('{} {} split'.format(name, (first, count)), got['split'],
           diag.split_rhat(host, count // 2), want)
    _close('{} {} nested, group {}'.format(name, (first, count), g), got['nested'],
           diag.nested_rhat(host, count, g), ref_nested(x, first, count, g))


@pytest.mark.parametrize('name', ['diag10', 'gmm2'])
def test_two_calls_give_the_same_bits(name):
  _, _, dev, again = _big(name)
  for key, a in dev.items():
    b = again[key]
    for k in ('split', 'nested', 'stats'):
      assert a[k].tobytes() == b[k].tobytes(), (key, k)


def test_few_chains_and_optional_outputs():
  spec = oracle.golden_spec('gmm2')
  eng = run(spec, golden_init('gmm2', 6), 40)
  try:
    x = eng.trace()['v_x']
    got = eng.trace_rhat(3, 37, 3, stats=True)
    host = diag.chain_moments(x, 3, 37)
    _close('N = 6 split', got['split'], diag.split_rhat(host, 18), ref_split(x, 3, 37))
    _close('N = 6 nested', got['nested'], diag.nested_rhat(host, 37, 3),
           ref_nested(x, 3, 37, 3))
    for i, row in enumerate(diag.ROWS):
      _close('N = 6 ' + row, got['stats'][i], host[i], ref_moments(x, 3, 37)[i])
    only = eng.trace_rhat(3, 37)
    assert only['nested'] is None and 'stats' not in only
    assert only['split'].tobytes() == got['split'].tobytes()
  finally:
    eng.close()
  eng = run(spec, golden_init('gmm2', 1), 40)
  try:
    x = eng.trace()['v_x']
    got = eng.trace_rhat(0, 40)
    _close('N = 1 split', got['split'], diag.split_rhat(diag.chain_moments(x, 0, 40), 20),
           ref_split(x, 0, 40))
    with pytest.raises(PbhError, match='group = 1'):
      eng.trace_rhat(0, 40, 1)
  finally:
    eng.close()


def test_many_chains():
  """33 000 chains of 8 records: the final reduction's threads take more than
  one batch of elements (2 N = 66 000 and N = 33 000 against 16 384 per sweep
  of the workgroup), and superchains of 16 500 chains take the 1 024-thread
  workgroup, also with a second batch; 2 200 chains stays within its first."""
  n, t = 33000, 8
  spec = oracle.golden_spec('gmm2')
  eng = run(spec, golden_init('gmm2', n), t)
  try:
    x = eng.trace()['v_x']
    dev = {g: eng.trace_rhat(0, t, g) for g in (1, 2200, n // 2)}
  finally:
    eng.close()
  host = diag.chain_moments(x, 0, t)
  want = ref_split(x, 0, t)
  for g, got in dev.items():
    _close('N = 33 000 split', got['split'], diag.split_rhat(host, t // 2), want)
    _close('N = 33 000 nested, group {}'.format(g), got['nested'],
           diag.nested_rhat(host, t, g), ref_nested(x, 0, t, g))


def test_constant_chains():
  base = oracle.golden_spec('gmm2')
  spec = dict(base, proposal=dict(base['proposal'], scale=np.zeros(2)))
  starts = np.array([[-1., 0.5], [0.25, 2.], [3., -1.]])
  for same in (True, False):
    x0 = np.repeat(starts[:1], 6, axis=0) if same else np.repeat(starts, 2, axis=0)
    eng = run(spec, x0, 12)
    try:
      x = eng.trace()['v_x']
      assert (x == x0[:, None, :]).all()   # the chains did not move
      got = eng.trace_rhat(0, 12, 2, stats=True)
    finally:
      eng.close()
    assert np.array_equal(got['stats'][[1, 3, 5]], np.zeros((3, 6, 2)))
    assert np.array_equal(got['stats'][[0, 2, 4]], np.broadcast_to(x0, (3, 6, 2)))
    for k in ('split', 'nested'):
      if same:
        assert np.isnan(got[k]).all(), (k, got[k])      # 0 / 0
      else:
        assert (got[k] == np.inf).all(), (k, got[k])    # B / 0


def test_no_side_effects():
  def reduce(eng):
    eng.trace_rhat(3, 61, 4, stats=True)
    eng.trace_rhat(3, 60, 258)

  check_no_side_effects(reduce, 516)


def test_refusals_leave_the_engine_working():
  from probayes_amd import Engine
  spec = oracle.golden_spec('gmm2')
  eng = Engine(spec)
  try:
    eng.init_chains(golden_init('gmm2', 12))
    eng.set_rng('philox', seed=3)
    with pytest.raises(PbhError, match='no trace'):
      eng.trace_rhat(0, 4)
    eng.alloc_trace(40, 1)
    eng.run(40, steps_per_launch=64)
    bad = [(dict(first=30, count=11), r'range \[30, 41\)'),
           (dict(first=-1, count=8), r'range \[-1, 7\)'),
           (dict(first=0, count=3), 'count = 3'),
           (dict(first=0, count=1, group=2), 'count = 1'),
           (dict(first=0, count=40, group=0), 'group = 0'),
           (dict(first=0, count=40, group=-3), 'group = -3'),
           (dict(first=0, count=40, group=5), 'group = 5'),
           (dict(first=0, count=40, group=12), 'group = 12')]
    for kw, msg in bad:
      with pytest.raises(PbhError, match=msg):
        eng.trace_rhat(**kw)
    x = eng.trace()['v_x']
    got = eng.trace_rhat(0, 40, 6)
    host = diag.chain_moments(x, 0, 40)
    _close('after refusals, split', got['split'], diag.split_rhat(host, 20),
           ref_split(x, 0, 40))
    _close('after refusals, nested', got['nested'], diag.nested_rhat(host, 40, 6),
           ref_nested(x, 0, 40, 6))
  finally:
    eng.close()


def test_sampler_trace_rhat():
  n, t = 68, 96
  with sampler_block(n, t) as (sampler, process, x, keys, _):
    got = sampler.trace_rhat(8, 87, group=4)
    assert set(got) == {'split', 'nested'} and set(got['split']) == set(keys)
    host = diag.chain_moments(x, 8, 87)
    _close('sampler split', [got['split'][k] for k in keys], diag.split_rhat(host, 43),
           ref_split(x, 8, 87))
    _close('sampler nested', [got['nested'][k] for k in keys],
           diag.nested_rhat(host, 87, 4), ref_nested(x, 8, 87, 4))
    assert sampler.trace_rhat()['nested'] is None
    for kw in (dict(count=3), dict(first=90, count=7), dict(group=0), dict(group=5),
               dict(group=n)):
      with pytest.raises(ValueError):
        sampler.trace_rhat(**kw)
    # a second block: the engine's trace is no longer the first block's
    process.next(sampler)
    with pytest.raises(ValueError, match='another block'):
      sampler.trace_rhat()
