"""Chain state in and out of an engine: pbh_get_state / pbh_set_chains,
pbh_get_checkpoint / pbh_restore and the carried ufun logs.  pbh_set_chains
and pbh_restore share one body (the copy in, the detached trace and replay
rows); pbh_restore alone takes the xoshiro state and marks seeded legacy
streams stale.  Small shapes on purpose: 130 chains are two full wavefronts
and a partial one with an odd lane-pair tail, 33 a single partial one."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import oracle
from oracle.workloads import golden_init

pytestmark = pytest.mark.gpu

CASES = [('diag10', 130), ('gmm2', 33)]
T, T1, SPL = 48, 17, 16   # an odd cut inside the second launch
KEYS = ('v_x', 'v_p', 'u')


def _engine(name, n, rng):
  from probayes_amd import Engine
  e = Engine(oracle.golden_spec(name))
  e.init_chains(golden_init(name, n))
  e.set_rng(rng, seed=21)
  return e


@functools.lru_cache(maxsize=None)
def _uninterrupted(name, n, rng):
  """The trace of T steps in one engine: computed once, read only."""
  e = _engine(name, n, rng)
  e.alloc_trace(T, 1)
  e.run(T, steps_per_launch=SPL)
  tr = e.trace()
  e.close()
  for k in KEYS:
    tr[k].setflags(write=False)
  return tr


def _continue(b, name, n, rng):
  """Runs the engine from step T1 to T and compares with the uninterrupted run."""
  b.alloc_trace(T - T1, 1)
  b.run(T - T1, steps_per_launch=SPL)
  got = b.trace()
  ref = _uninterrupted(name, n, rng)
  for k in KEYS:
    assert np.array_equal(got[k], ref[k][:, T1:]), k
  assert 0 < got['u'].mean() < 1


def _trace_outcome(e):
  """What trace() does, comparable between engines: the error text, or the
  arrays' shapes."""
  from probayes_amd._lib import PbhError
  try:
    tr = e.trace()
  except PbhError as err:
    return ('error', str(err))
  return ('ok', tuple(tr[k].shape for k in KEYS))


@pytest.mark.parametrize('name,n', CASES)
def test_state_then_set_chains_continues_the_run(name, n):
  """Philox is keyed by (seed, chain, absolute step): x, lp, the step and the
  step-1 flag are the whole state."""
  a = _engine(name, n, 'philox')
  a.run(T1, steps_per_launch=SPL)
  x, lp = a.state()
  a.close()
  b = _engine(name, n, 'philox')
  b.set_chains(x, lp, T1, True)
  _continue(b, name, n, 'philox')
  b.close()


@pytest.mark.parametrize('name,n', CASES)
def test_checkpoint_then_restore_continues_the_run_xoshiro(name, n):
  a = _engine(name, n, 'xoshiro')
  a.run(T1, steps_per_launch=SPL)
  ck = a.checkpoint()
  a.close()
  assert ck['step'] == T1 and ck['has_pred'] and ck['xo'].shape == (8, n)
  b = _engine(name, n, 'xoshiro')
  b.restore(ck)
  _continue(b, name, n, 'xoshiro')
  b.close()


def test_chain_logs_round_trip_through_a_checkpoint():
  """The production ufun logs ([d][n] on the device, [n][d] in a checkpoint):
  none before the first production run, the same words after set + get, and
  the restored engine continues the run."""
  name, n = 'metrohast_norm1d', 33
  a = _engine(name, n, 'philox')
  assert a.checkpoint()['lx'] is None       # valid == 0
  a.run(T1, steps_per_launch=SPL)
  ck = a.checkpoint()
  a.close()
  assert ck['lx'] is not None and ck['lx'].shape == (n, a.dim)
  b = _engine(name, n, 'philox')
  b.restore(ck)
  back = b.checkpoint()
  # (bit for bit: the dims without a ufun hold whatever the kernel left there)
  assert np.array_equal(back['lx'].view(np.uint64), ck['lx'].view(np.uint64))
  assert np.array_equal(back['x'], ck['x']) and np.array_equal(back['lp'], ck['lp'])
  assert back['step'] == T1 and back['has_pred']
  _continue(b, name, n, 'philox')
  b.close()


@pytest.mark.parametrize('how', ['set_chains', 'restore'])
@pytest.mark.parametrize('name,n', CASES)
def test_trace_and_replay_rows_are_detached(name, n, how):
  """After either call a run records nothing, trace() behaves as in an engine
  without one, and pbh_get_replay holds no rows."""
  from probayes_amd._lib import PbhError
  bare = _engine(name, n, 'replay')
  bare.alloc_trace(0, 1)                   # capacity 0: no trace
  want = _trace_outcome(bare)
  bare.close()
  e = _engine(name, n, 'replay')
  e.seed_legacy(np.arange(n) + 7)
  e.legacy_replay(6)
  e.alloc_trace(6, 1)
  e.run(4)
  assert e.trace_len() == 4
  assert e.get_replay(0, 6).shape == (6, e.stream_width(), n)
  ck = e.checkpoint()
  if how == 'set_chains':
    e.set_chains(ck['x'], ck['lp'], ck['step'], ck['has_pred'])
  else:
    e.restore(ck)
  assert e.trace_len() == 0
  assert _trace_outcome(e) == want
  with pytest.raises(PbhError, match='outside the 0-row stream'):
    e.get_replay(0, 1)
  e.legacy_replay(3)
  e.run(3)
  assert e.trace_len() == 0
  assert _trace_outcome(e) == want
  x, _ = e.state()
  assert not np.array_equal(x, ck['x'])    # the run itself ran
  e.close()


def test_restore_marks_seeded_legacy_streams_stale_set_chains_does_not():
  from probayes_amd._lib import PbhError
  name, n = 'diag10', 130
  e = _engine(name, n, 'replay')
  e.seed_legacy(np.arange(n) + 7)
  e.legacy_replay(2)
  e.run(2)
  ck = e.checkpoint()
  assert ck['mt'] is not None
  calls = (lambda: e.legacy_replay(2), lambda: e.legacy_run(2),
           lambda: e.legacy_draws(2, kind='gauss'))
  e.set_chains(ck['x'], ck['lp'], ck['step'], ck['has_pred'])
  for call in calls:
    call()                                   # the streams go on
  e.restore(dict(ck, mt=None))               # ... the legacy state not set
  for call in calls:
    with pytest.raises(PbhError, match='pbh_set_legacy_state'):
      call()
  e.restore(ck)
  for call in calls:
    call()
  e.close()


def test_restore_argument_checks():
  from probayes_amd._lib import PbhError
  name, n = 'gmm2', 33
  a = _engine(name, n, 'xoshiro')
  a.run(T1, steps_per_launch=SPL)
  ck = a.checkpoint()
  a.close()
  b = _engine(name, n, 'xoshiro')
  with pytest.raises(PbhError, match='XOSHIRO needs the generator state xo'):
    b.restore(dict(ck, xo=None))
  x, lp = b.state()
  assert not np.array_equal(x, ck['x'])      # refused before any copy
  b.close()
  c = _engine(name, n, 'philox')
  with pytest.raises(PbhError, match='xo given but the rng is not XOSHIRO'):
    c.restore(ck)
  x, lp = c.state()                          # x and lp were copied by then
  assert np.array_equal(x, ck['x']) and np.array_equal(lp, ck['lp'])
  c.close()
