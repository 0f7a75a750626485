"""pbh_trace_ess_rank (Engine.trace_ess_rank, Sampler.trace_ess_rank): the
bulk- and tail-ESS across chains of a recorded trace computed on the device
(power spectra summed over the split chains, one inverse transform per dim and
variant, Stan's estimator on the host), against ess_reference.py (direct sums
in longdouble) applied to the same trace copied to the host.

Every variant's averaged autocovariance must agree with the reference within
max_t |A_dev[t] - A_ref[t]| / A_ref[0] <= max(1e-12, 32 x diag.py's own
distance), 1e-12 being the project's tolerance for sums over a trace; every ESS
relatively within max(1e-9, 32 x diag.py's own distance), 1e-9 being the
project's tolerance for the device ESS.  Every decision of Geyer's scan must be
clear of rounding in the reference (ess_reference.clear, margin 1e-9), which is
asserted for every dim compared.  Nothing is left out of a comparison, and each
test prints what it measured before it asserts.

Shapes, the smallest at which each part can go wrong: N = 2 004 chains, T = 160
with windows (40, 120), (40, 119) and (0, 4) (more chain pairs than workgroups
of a launch can hold one each is test_many_chains'; here 1 002 pairs in 501
workgroups of two, an odd count, h = 2, the rejected steps as ties), d = 10 and
d = 2; N = 33 with an odd count (a last chain without a partner, dims that do
not start on a 16-byte boundary); N = 6 and N = 1; T = 4 098 of slow chains for
h = 2 048, the whole transform; chains that never move; a NaN."""
import functools

import numpy as np
import pytest

import oracle
from oracle.workloads import golden_init
from probayes_amd import diag
from probayes_amd._lib import PbhError
from ess_reference import VARIANTS, clear, ref_rank_ess
from rhat_reference import rel_dist
from trace_helpers import (N_BIG, Q64, T_BIG, WINDOWS, big_run, check_no_side_effects, flat,
                           run, sampler_block, tied_starts)

pytestmark = pytest.mark.gpu

KEYS = VARIANTS + ('tail',)
LD = np.longdouble


def _diag_acov(x, first, count):
  """{variant: [d, h]}: diag.py's own averaged autocovariances of a host trace"""
  n, _, d = x.shape
  w = x[:, first:first + count, :]
  z = diag.normal_scores(diag.average_ranks(x, first, count), n * count)
  q = diag.pooled_quantile(x, [.05, .95], first, count)
  out = {key: np.empty((d, count // 2)) for key in VARIANTS}
  for k in range(d):
    series = {'bulk': z[:, :, k], 'basic': w[:, :, k],
              'tail_lower': (w[:, :, k] <= q[0, k]).astype(float),
              'tail_upper': (w[:, :, k] <= q[1, k]).astype(float)}
    for key in VARIANTS:
      out[key][k] = diag.split_chain_acov(series[key])[1]
  return out


def _acov_dist(a, ref_dims):
  """max over dims and lags of |A[t] - A_ref[t]| / A_ref[0]"""
  worst = 0.
  for k, r in enumerate(ref_dims):
    with np.errstate(all='ignore'):
      dist = np.max(np.abs(np.asarray(a[k], LD) - r['acov'])) / r['acov'][0]
    worst = max(worst, float(dist) if np.isfinite(dist) else np.inf)
  return worst


def _close(what, got, x, first, count, variants=VARIANTS):
  """every ESS and every averaged autocovariance of a device result (basic=True,
  acov=True) against the longdouble reference on the host copy"""
  host = diag.rank_ess(x, first, count)
  host_acov = _diag_acov(x, first, count)
  ref = ref_rank_ess(x, first, count, variants)
  d, h = x.shape[2], count // 2
  for key in variants:
    dims = ref[key]
    assert all(clear(r) for r in dims), (what, key, [r['k_star'] for r in dims])
    want = np.array([r['ess'] for r in dims])
    own = rel_dist(host[key], want)
    bound, dist = max(1e-9, 32 * own), rel_dist(got[key], want)
    own_a = _acov_dist(host_acov[key], dims)
    bound_a, dist_a = max(1e-12, 32 * own_a), _acov_dist(got['acov'][key], dims)
    print('{} {}: ESS device - longdouble {:.3g} (diag.py {:.3g}, bound {:.3g}); acov {:.3g} '
          '(diag.py {:.3g}, bound {:.3g}); k* {} of K {}'.format(
              what, key, dist, own, bound, dist_a, own_a, bound_a,
              [r['k_star'] for r in dims], dims[0]['K']))
    assert got[key].shape == (d,) and got['acov'][key].shape == (d, h), (what, key)
    assert np.isfinite(bound) and np.isfinite(bound_a), what
    assert dist_a <= bound_a, (what, key, dist_a, bound_a)
    assert dist <= bound, (what, key, dist, bound)
  if 'tail_lower' in variants:
    assert got['tail'].tobytes() == np.minimum(got['tail_lower'], got['tail_upper']).tobytes()
  return ref


def _same(a, b):
  """two results of trace_ess_rank: the same keys and bits"""
  assert set(a) == set(b)
  for k in a:
    if k == 'acov':
      assert set(a[k]) == set(b[k])
      for v in a[k]:
        assert a[k][v].tobytes() == b[k][v].tobytes(), (k, v)
    else:
      assert a[k].tobytes() == b[k].tobytes(), k


def _everything_twice_then_the_defaults(eng, first, count):
  return (eng.trace_ess_rank(first, count, basic=True, acov=True),
          eng.trace_ess_rank(first, count, basic=True, acov=True),
          eng.trace_ess_rank(first, count))


def _big(name):
  """One run per model: the host copy of the trace and every device result,
  each asked for twice, and once with the default outputs only."""
  spec, x, res = big_run(name, _everything_twice_then_the_defaults)
  dev, again, plain = ({w: r[i] for w, r in res.items()} for i in range(3))
  return spec, x, dev, again, plain


@pytest.mark.parametrize('first,count', WINDOWS)
@pytest.mark.parametrize('name', ['diag10', 'gmm2'])
def test_ess_per_dim(name, first, count):
  spec, x, dev, _, plain = _big(name)
  assert x.shape == (N_BIG, T_BIG, spec['dim'])
  rep = x[:, first + 1:first + count, 0] == x[:, first:first + count - 1, 0]
  assert rep.any() and not rep.all()   # the rejected steps: runs of equal values
  got = dev[first, count]
  _close('{} {}'.format(name, (first, count)), got, x, first, count)
  # the result does not depend on which optional outputs were asked for
  assert set(plain[first, count]) == {'bulk', 'tail', 'tail_lower', 'tail_upper'}
  for key in plain[first, count]:
    assert plain[first, count][key].tobytes() == got[key].tobytes(), key


@pytest.mark.parametrize('name', ['diag10', 'gmm2'])
def test_two_calls_give_the_same_bits(name):
  _, _, dev, again, _ = _big(name)
  for key, a in dev.items():
    assert set(a) == set(KEYS) | {'acov'} and set(a['acov']) == set(VARIANTS)
    _same(a, again[key])


def test_outputs_asked_for_one_at_a_time():
  """every combination of the C entry point's outputs that selects other
  variants: the same bits as when all are asked for, and rows of mean_acov
  that were not computed are left untouched"""
  import ctypes as c
  from probayes_amd import _lib
  spec = oracle.golden_spec('gmm2')
  n, t, first, count = 33, 40, 2, 37
  eng = run(spec, golden_init('gmm2', n), t)
  try:
    full = eng.trace_ess_rank(first, count, basic=True, acov=True)
    d, h = 2, count // 2
    dp = lambda a: a.ctypes.data_as(c.POINTER(c.c_double))

    def call(bulk=False, tail=False, parts=False, basic=False, acov=False):
      out = {k: np.full(s, -7.) for k, s in (('bulk', d), ('tail', d), ('parts', (2, d)),
                                             ('basic', d), ('acov', (4, d, h)))}
      want = dict(bulk=bulk, tail=tail, parts=parts, basic=basic, acov=acov)
      _lib.call('pbh_trace_ess_rank', eng._h, c.c_int64(first), c.c_int64(count),
                *[dp(out[k]) if want[k] else None for k in ('bulk', 'tail', 'parts', 'basic',
                                                            'acov')])
      return out

    rows = {0: 'bulk', 1: 'tail_lower', 2: 'tail_upper', 3: 'basic'}
    for kw, computed in ((dict(bulk=True, acov=True), {0}), (dict(tail=True, acov=True), {1, 2}),
                         (dict(parts=True, acov=True), {1, 2}), (dict(basic=True, acov=True), {3}),
                         (dict(acov=True), {0, 1, 2, 3}),
                         (dict(bulk=True, basic=True, acov=True), {0, 3})):
      out = call(**kw)
      for v, key in rows.items():
        if v in computed:
          assert out['acov'][v].tobytes() == full['acov'][key].tobytes(), (kw, key)
        else:
          assert (out['acov'][v] == -7.).all(), (kw, key)
      if kw.get('bulk'):
        assert out['bulk'].tobytes() == full['bulk'].tobytes()
      if kw.get('tail'):
        assert out['tail'].tobytes() == full['tail'].tobytes()
      if kw.get('parts'):
        assert out['parts'][0].tobytes() == full['tail_lower'].tobytes()
        assert out['parts'][1].tobytes() == full['tail_upper'].tobytes()
      if kw.get('basic'):
        assert out['basic'].tobytes() == full['basic'].tobytes()
  finally:
    eng.close()


def test_odd_chains_and_few_chains():
  spec = oracle.golden_spec('gmm2')
  # (N = 1: seed 3 puts a pair of dim 0's upper-tail scan within 1e-9 of zero)
  for n, t, first, count, seed in ((33, 40, 2, 37, 3), (6, 40, 3, 37, 3), (1, 40, 0, 40, 1)):
    eng = run(spec, golden_init('gmm2', n), t, seed=seed)
    try:
      x = eng.trace()['v_x']
      got = eng.trace_ess_rank(first, count, basic=True, acov=True)
      whole = eng.trace_ess_rank(basic=True, acov=True)
    finally:
      eng.close()
    _close('N = {} {}'.format(n, (first, count)), got, x, first, count)
    _close('N = {}, the whole trace'.format(n), whole, x, 0, t)


@functools.lru_cache(maxsize=None)
def _slow():
  """8 chains of 4 098 records with a narrow proposal: slow mixing, a late stop
  of the scan, the running minimum at work; h = 2 048 fills the transform"""
  base = oracle.golden_spec('gmm2')
  spec = dict(base, proposal=dict(base['proposal'], scale=np.full(2, 0.05)))
  eng = run(spec, golden_init('gmm2', 8), 4098)
  try:
    x = eng.trace()['v_x']
    dev = {w: eng.trace_ess_rank(w[0], w[1], basic=True, acov=True)
           for w in ((0, 4096), (1, 4097))}
    with pytest.raises(PbhError, match='at most 2048') as refused:
      eng.trace_ess_rank(0, 4098)
    after = eng.trace_ess_rank(0, 4096, basic=True, acov=True)
  finally:
    eng.close()
  return x, dev, refused.value, after


@pytest.mark.parametrize('first,count', [(0, 4096), (1, 4097)])
def test_longest_halves(first, count):
  x, dev, _, _ = _slow()
  ref = _close('h = 2 048 {}'.format((first, count)), dev[first, count], x, first, count)
  stops = [r['k_star'] for key in VARIANTS for r in ref[key]]
  print('k* of', stops)
  assert max(stops) > 16   # slow mixing: the scan runs long
  assert any(r['min_changed'] for key in VARIANTS for r in ref[key])


def test_a_longer_half_is_unsupported_and_the_engine_works_afterwards():
  _, dev, refused, after = _slow()
  assert refused.code == -4   # PBH_ERR_UNSUPPORTED
  assert 'count = 4098' in str(refused)
  _same(after, dev[0, 4096])


def test_many_chains():
  """33 000 chains: 16 500 chain pairs in 500 workgroups of 33 each, so the
  per-workgroup loop runs and 500 partial rows are added."""
  n, t = 33000, 16
  eng = run(oracle.golden_spec('gmm2'), golden_init('gmm2', n), t)
  try:
    x = eng.trace()['v_x']
    dev = {w: eng.trace_ess_rank(w[0], w[1], basic=True, acov=True) for w in ((0, 16), (1, 15))}
  finally:
    eng.close()
  for (first, count), got in dev.items():
    _close('N = 33 000 {}'.format((first, count)), got, x, first, count)


def _against_diag(what, got, x, first, count):
  """where the definition gives a non-finite value the device gives the same;
  elsewhere it is within the ESS bound of the definition itself"""
  host = diag.rank_ess(x, first, count)
  for key in KEYS:
    print(what, key, got[key], host[key])
    fin = np.isfinite(host[key])
    assert np.array_equal(got[key][~fin], host[key][~fin], equal_nan=True), (what, key)
    assert rel_dist(got[key][fin], host[key][fin]) <= 1e-9, (what, key)
  return host


@pytest.mark.parametrize('kind', ['one_value', 'top_bits'])
def test_constant_chains(kind):
  """Chains that never move (a Gaussian proposal of scale 0): all equal gives
  0 / 0 = NaN everywhere; constant but different gives rho = 1 at every lag and
  a finite value."""
  base = oracle.golden_spec('gmm2')
  spec = dict(base, proposal=dict(base['proposal'], scale=np.zeros(2)))
  x0 = tied_starts(kind)
  eng = run(spec, x0, 12)
  try:
    x = eng.trace()['v_x']
    assert x.shape == (130, 12, 2) and (x == x0[:, None, :]).all()   # the chains did not move
    got = eng.trace_ess_rank(0, 12, basic=True, acov=True)
    part = eng.trace_ess_rank(5, 5, basic=True, acov=True)
  finally:
    eng.close()
  host = _against_diag(kind, got, x, 0, 12)
  _against_diag(kind + ' (5, 5)', part, x, 5, 5)
  if kind == 'one_value':
    for key in KEYS:
      assert np.isnan(got[key]).all() and np.isnan(host[key]).all(), key
  else:
    assert np.isfinite(got['bulk']).all() and np.isfinite(host['bulk']).all()
  for key in VARIANTS:   # a constant chain is centred to exact zeros
    a = got['acov'][key]
    assert ((a == 0.) | np.isnan(a)).all(), key


def test_a_nan_chain_makes_its_dim_nan():
  """The engine accepts a NaN start, and with a proposal of scale 0 the chain
  stays there: every output of that dim is NaN, the other dim is within bound
  (24 chains at 24 values: fewer than 5 % of its elements are at its largest)."""
  base = oracle.golden_spec('gmm2')
  spec = dict(base, proposal=dict(base['proposal'], scale=np.zeros(2)))
  x0 = np.stack([np.linspace(-2., 3., 24), np.resize([0.5, 2., -1.], 24)], axis=1)
  x0[4, 1] = np.nan
  eng = run(spec, x0, 12)
  try:
    x = eng.trace()['v_x']
    assert np.array_equal(x, np.broadcast_to(x0[:, None, :], x.shape), equal_nan=True)
    got = eng.trace_ess_rank(0, 12, basic=True, acov=True)
  finally:
    eng.close()
  for key in KEYS:
    assert np.isnan(got[key][1]) and np.isfinite(got[key][0]), (key, got[key])
  for key in VARIANTS:
    assert np.isnan(got['acov'][key][1]).all() and np.isfinite(got['acov'][key][0]).all(), key
  # the other dim: constant chains, so A = 0 exactly (no quotient by A[0] to
  # take) and the ESS within bound of the longdouble reference
  ref = ref_rank_ess(x[:, :, :1], 0, 12)
  for key in VARIANTS:
    assert clear(ref[key][0]), key
    assert (got['acov'][key][0] == 0.).all() and (ref[key][0]['acov'] == 0).all(), key
    dist = rel_dist(got[key][:1], np.array([ref[key][0]['ess']]))
    print('NaN chain, the other dim', key, got[key][0], 'device - longdouble', dist)
    assert dist <= 1e-9, (key, dist)
  _against_diag('NaN chain', got, x, 0, 12)


def test_no_side_effects():
  def reduce(eng):
    eng.trace_ess_rank(3, 61, basic=True, acov=True)
    eng.trace_ess_rank(3, 60)

  check_no_side_effects(reduce, 516)


def test_results_do_not_depend_on_what_the_scratch_held():
  """Two engines with one seed make the same calls on the shared reduction
  scratch, one in this order and one in reverse: the same bits."""
  calls = [
      ('ess', lambda e: e.trace_ess_rank(basic=True, acov=True)),
      ('rank_ranks', lambda e: e.trace_rhat_rank(ranks=True)),
      ('pooled_64', lambda e: e.trace_quantile_pooled(Q64, order_stats=True)),
      ('rhat_2', lambda e: e.trace_rhat(group=2, stats=True)),
      ('ess_tail', lambda e: e.trace_ess_rank(3, 61)),
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
  # and they are the host's definition on the trace copied out
  _close('after other reductions', a['ess'], traces[0], 0, t)


def test_refusals_leave_the_engine_working():
  from probayes_amd import Engine
  spec = oracle.golden_spec('gmm2')
  eng = Engine(spec)
  try:
    eng.init_chains(golden_init('gmm2', 12))
    eng.set_rng('philox', seed=3)
    with pytest.raises(PbhError, match='no trace'):
      eng.trace_ess_rank(0, 4)
    eng.alloc_trace(40, 1)
    eng.run(40, steps_per_launch=64)
    x = eng.trace()['v_x']
    bad = [(dict(first=30, count=11), r'range \[30, 41\)'),
           (dict(first=-1, count=8), r'range \[-1, 7\)'),
           (dict(first=0, count=3), 'count = 3'),
           (dict(first=0, count=0), 'count = 0')]
    for kw, msg in bad:
      with pytest.raises(PbhError, match=msg):
        eng.trace_ess_rank(**kw)
      # the next valid call on the same engine is still right
      _close('after ' + msg, eng.trace_ess_rank(2, 38, basic=True, acov=True), x, 2, 38)
    import ctypes as c
    lib = __import__('probayes_amd')._lib.load()
    rc = lib.pbh_trace_ess_rank(eng._h, c.c_int64(2), c.c_int64(38), None, None, None, None, None)
    assert rc == -1 and b'no output' in lib.pbh_last_error()
    _close('after no output', eng.trace_ess_rank(2, 38, basic=True, acov=True), x, 2, 38)
  finally:
    eng.close()


def test_sampler_trace_ess_rank():
  n, t = 68, 96
  with sampler_block(n, t) as (sampler, process, x, keys, _):
    names = ('bulk', 'tail', 'tail_lower', 'tail_upper')
    for kw, (first, count) in ((dict(first=8, count=87), (8, 87)), (dict(), (0, t))):
      got = sampler.trace_ess_rank(**kw)
      assert set(got) == set(names) and all(set(got[k]) == set(keys) for k in names)
      host = diag.rank_ess(x, first, count)
      ref = ref_rank_ess(x, first, count, ('bulk', 'tail_lower', 'tail_upper'))
      for key in ('bulk', 'tail_lower', 'tail_upper'):
        assert all(clear(r) for r in ref[key]), key
        want = np.array([r['ess'] for r in ref[key]])
        bound = max(1e-9, 32 * rel_dist(host[key], want))
        dist = rel_dist(np.array([got[key][name] for name in keys]), want)
        print('sampler {} {}: {:.3g} (bound {:.3g})'.format((first, count), key, dist, bound))
        assert dist <= bound, (key, dist, bound)
      for name in keys:
        assert got['tail'][name] == min(got['tail_lower'][name], got['tail_upper'][name])
    for kw in (dict(count=3), dict(first=90, count=7), dict(first=-1)):
      with pytest.raises(ValueError):
        sampler.trace_ess_rank(**kw)
    # a second block: the engine's trace is no longer the first block's
    process.next(sampler)
    with pytest.raises(ValueError, match='another block'):
      sampler.trace_ess_rank()
