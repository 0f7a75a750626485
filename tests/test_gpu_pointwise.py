"""The pointwise reduction on the GPU (pbh_trace_pointwise, Engine.
trace_pointwise, Sampler.trace_pointwise / trace_waic): per observation the
log-sum-exp, the mean and the variance over the draws of a trace window of the
term a pointwise program gives, against the host definition -- the trace
downloaded, the terms T [draws, n] formed by expr.evaluate_pointwise and reduced
by diag.pointwise_stats.

lse and mean are held to the project's RTOL of 1e-12 with floor 1.  The
variance is held as the host merges are (test_pointwise_host.py): its error
against a two-pass np.longdouble value lies within 8x that of NumPy's own fp64
against the same value, or within 1e-12 relative where NumPy's is smaller."""
import ctypes

import numpy as np
import pytest
import scipy.stats

import oracle
import probayes_amd as pb
from oracle.workloads import golden_init
from probayes_amd import _lib, diag, expr
from probayes_amd._lib import PbhError
from probayes_amd.engine import Engine
from expr_data_examples import DATA_WORKLOADS
from trace_helpers import check_no_side_effects, run, sampler_block
import test_pointwise_lower as lower

pytestmark = pytest.mark.gpu

RTOL = 1e-12


def _program(name, keys):
  fn, own = lower.TERMS[name][:2]
  return expr.trace_pointwise(lambda **kw: fn(*[kw[k] for k in own]), keys)


# the three term vectors over the dims of data_linreg3 (b0, b1, s): the logistic
# terms read (b0, b1), the robust ones (b0, s)
PROGRAMS = {
  137: lambda: _program('linreg', ['b0', 'b1', 's']),
  40: lambda: _program('logistic', ['a', 'b', 'unused']),
  7: lambda: _program('robust_cauchy', ['m', 'unused', 's']),
}


def _linreg_spec():
  builder, params = DATA_WORKLOADS['data_linreg3'][:2]
  return builder(pb, params)[0].lower()


def _linreg_starts(n):
  rs = np.random.RandomState(6)
  return np.stack([rs.normal(0.7, 0.1, n), rs.normal(-1.2, 0.1, n), rs.uniform(0.6, 1.1, n)], -1)


def _terms(prog, x):
  """T [draws, n] of the host trace window x [N, count, d]"""
  return expr.evaluate_pointwise(prog['code'], prog['consts'], x.reshape(-1, x.shape[2]),
                                 prog['data'])


def _var_bounds(T):
  """per observation: the two-pass longdouble variance, and how far from it
  (relative) the device may lie"""
  with np.errstate(all='ignore'):
    own = diag.pointwise_stats(T)[2]
    t = T.astype(np.longdouble)
    mean = t.sum(axis=0) / t.shape[0]
    truth = ((t - mean) ** 2).sum(axis=0) / (t.shape[0] - 1)
    e_np = np.abs(own - truth) / np.abs(truth)
  return truth, np.maximum(8. * np.where(np.isfinite(e_np), e_np, 0.).astype(float), 1e-12)


def _check(what, got, T):
  """got against diag.pointwise_stats(T); the places of infinities and NaNs
  must agree exactly"""
  with np.errstate(all='ignore'):
    lse, mean, var = diag.pointwise_stats(T)
  assert got['lse'].shape == got['mean'].shape == got['var'].shape == (T.shape[1],)
  for key, want in (('lse', lse), ('mean', mean)):
    fin = np.isfinite(want)
    assert np.array_equal(got[key][~fin], want[~fin], equal_nan=True), (what, key)
    err = np.abs(got[key][fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1.)
    print(what, key, 'max err', float(err.max()) if err.size else 0.)
    assert np.all(err <= RTOL), (what, key, float(err.max()))
  fin = np.isfinite(var)
  assert np.array_equal(got['var'][~fin], var[~fin], equal_nan=True), (what, 'var')
  truth, bound = _var_bounds(T[:, fin])
  zero = truth == 0
  assert np.all(got['var'][fin][zero] == 0.)
  err = (np.abs(got['var'][fin] - truth) / np.abs(np.where(zero, 1., truth))).astype(float)
  err = np.where(zero, 0., err)
  print(what, 'var max err', float(err.max()) if err.size else 0., 'bound at it',
        float(bound[np.argmax(err)]) if err.size else 0.)
  assert np.all(err <= bound), (what, 'var', float(err.max()))


# ---------------------------------------------------------------------------
# 1. against the host definition
# ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def linreg_runs():
  """data_linreg3 engines with their host traces: 130 chains x 24 records, 1 x
  24 and 2 004 x 16; the device results of every program and window"""
  spec = _linreg_spec()
  shapes = {(130, 24): ((0, 24), (5, 7), (3, 1)), (1, 24): ((0, 24),), (2004, 16): ((0, 16),)}
  progs = {n: make() for n, make in PROGRAMS.items()}
  out = {}
  for (n, t), windows in shapes.items():
    eng = run(spec, _linreg_starts(n), t)
    try:
      x = eng.trace()['v_x']
      res = {(n_obs, w): eng.trace_pointwise(progs[n_obs], *w) for n_obs in progs for w in windows}
    finally:
      eng.close()
    out[(n, t)] = (x, res)
  return progs, out


@pytest.mark.parametrize('n_obs', [137, 40, 7])
@pytest.mark.parametrize('shape', [(130, 24), (1, 24), (2004, 16)])
def test_against_the_host_definition(linreg_runs, shape, n_obs):
  progs, runs = linreg_runs
  x, res = runs[shape]
  assert x.shape == shape + (3,)
  for (m, (first, count)), got in res.items():
    if m == n_obs:
      _check('{} n={} [{}, {})'.format(shape, n_obs, first, first + count), got,
             _terms(progs[n_obs], x[:, first:first + count]))


# ---------------------------------------------------------------------------
# 2. any model
# ---------------------------------------------------------------------------
def _diag10_case():
  spec = oracle.golden_spec('diag10')
  rs = np.random.RandomState(1910)
  X = rs.normal(0., 1., 19)
  Y = 0.3 + 0.5 * X + 1.3 * rs.standard_normal(19)
  keys = ['k{}'.format(i) for i in range(10)]
  prog = expr.trace_pointwise(
      lambda **kw: scipy.stats.norm.logpdf(Y, kw['k0'] + kw['k9'] * X, 1.3), keys)
  return spec, prog


def test_a_closed_form_model():
  spec, prog = _diag10_case()
  eng = run(spec, golden_init('diag10', 130), 24)
  try:
    x = eng.trace()['v_x']
    got = eng.trace_pointwise(prog, 2, 20)
    # a program that reads variable d = 10
    keys = ['k{}'.format(i) for i in range(11)]
    beyond = expr.trace_pointwise(lambda **kw: kw['k10'] * np.arange(19.), keys)
    with pytest.raises(PbhError, match='variable index'):
      eng.trace_pointwise(beyond)
  finally:
    eng.close()
  _check('diag10', got, _terms(prog, x[:, 2:22]))


def test_an_engine_of_more_dims_than_a_program_reads_is_refused():
  d = 20   # (the engine has no kernel of 17 dims; 20 is its next)
  spec = pb.make_spec(d, {'kind': 'diag_gauss', 'mu': np.zeros(d), 'sigma': np.ones(d)},
                      {'kind': 'gauss', 'scale': 0.3}, pscale='log')
  eng = run(spec, np.zeros((8, d)), 4)
  try:
    with pytest.raises(PbhError, match='20 dims'):
      eng.trace_pointwise(PROGRAMS[40]())
  finally:
    eng.close()


# ---------------------------------------------------------------------------
# 3. edges, on chains that never move
# ---------------------------------------------------------------------------
EDGE_Y = np.array([2., 0.5, -1., 0.25, 1., 3., 0.75, 0., 1.5, 0.125, 5.])   # n = 11


def _edge_programs():
  keys = ['x', 'w']
  return {
    '-inf': expr.trace_pointwise(lambda **kw: np.log(np.maximum(EDGE_Y - kw['x'], 0.)), keys),
    'NaN': expr.trace_pointwise(lambda **kw: np.log(EDGE_Y - kw['x']), keys),
    'spread': expr.trace_pointwise(lambda **kw: kw['w'] + 0.001 * EDGE_Y, keys),
  }


def test_edges_on_chains_that_never_move():
  base = oracle.golden_spec('gmm2')
  spec = dict(base, proposal=dict(base['proposal'], scale=np.zeros(2)))
  # dim 0 from 0 to 1: Y - x is positive for all chains, for some, and for none;
  # dim 1 from -745 to +709
  x0 = np.stack([np.linspace(0., 1., 130), np.linspace(-745., 709., 130)], axis=1)
  progs = _edge_programs()
  eng = run(spec, x0, 6)
  try:
    x = eng.trace()['v_x']
    assert (x == x0[:, None, :]).all()   # the chains did not move
    got = {k: (eng.trace_pointwise(p, 0, 6), eng.trace_pointwise(p, 2, 1)) for k, p in progs.items()}
  finally:
    eng.close()
  for key, prog in progs.items():
    for (first, count), res in zip(((0, 6), (2, 1)), got[key]):
      T = _terms(prog, x[:, first:first + count])
      _check('{} [{}, {})'.format(key, first, first + count), res, T)
  T = _terms(progs['-inf'], x)
  some = np.isinf(T).any(axis=0) & ~np.isinf(T).all(axis=0)
  assert some.any() and np.isinf(T).all(axis=0).any() and np.isfinite(T).all(axis=0).any()
  lse = got['-inf'][0]['lse']
  assert np.all(np.isfinite(lse[some])) and np.all(lse[np.isinf(T).all(axis=0)] == -np.inf)
  assert np.all(got['-inf'][0]['mean'][some] == -np.inf) and np.all(np.isnan(got['-inf'][0]['var'][some]))
  nan = np.isnan(_terms(progs['NaN'], x)).any(axis=0)
  assert nan.any() and not nan.all()
  for k in ('lse', 'mean', 'var'):
    assert np.all(np.isnan(got['NaN'][0][k][nan]))
  assert np.all(np.isfinite(got['spread'][0]['lse'])) and np.all(got['spread'][0]['lse'] > 709.)


# ---------------------------------------------------------------------------
# 4. every body opcode
# ---------------------------------------------------------------------------
def _every_opcode_program(n):
  """The body of test_gpu_expr_data.py's program of the same name -- every
  elementwise opcode, an outer slot, the four temporaries, three columns -- in
  the pointwise shape: the outer words before the region, SUM last."""
  E, V, C, A, S, B = expr.encode, expr.VAR, expr.CONST, expr.ACC, expr.SLOT, expr.BODY_BASE
  rs = np.random.RandomState(70 + n)
  X, Y, W = rs.normal(0., 1.5, n), rs.normal(1., 2., n), rs.uniform(0.5, 2., n)
  code = [E(expr.ABS, (V, 1)),
          E(expr.ADD, (A, 0), (C, 0), dst=0, store=True),       # slot 0 = |b| + 0.5
          E(expr.LOOP, (S, 20)),
          E(expr.MOV, (V, B + 0), dst=0, store=True),           # t0 = X
          E(expr.MUL, (A, 0), (V, 1)),
          E(expr.ADD, (A, 0), (V, 0), dst=1, store=True),       # t1 = a + b X
          E(expr.SUB, (V, B + 1), (A, 0)),
          E(expr.DIV, (A, 0), (V, B + 2), dst=2, store=True),   # t2 = (Y - t1) / W
          E(expr.ABS, (A, 0)),
          E(expr.SQRT, (A, 0)),
          E(expr.NEG, (A, 0)),
          E(expr.EXP, (A, 0), dst=3, store=True),               # t3 = exp(-sqrt|t2|)
          E(expr.LOG1P, (A, 0)),
          E(expr.EXPM1, (A, 0)),
          E(expr.ADD, (A, 0), (S, 0)),                          # + the outer slot
          E(expr.LOG, (A, 0)),
          E(expr.POW, (A, 0), (C, 1)),
          E(expr.MAX, (A, 0), (S, B + 2)),
          E(expr.MIN, (A, 0), (S, B + 3)),
          E(expr.MUL, (A, 0), (S, B + 1)),
          E(expr.SUB, (A, 0), (S, B + 0)),
          E(expr.ADD, (A, 0), (S, B + 3)),
          E(expr.MUL, (A, 0), (C, 2)),
          E(expr.SUM, (A, 0))]
  return {'code': np.array(code, np.int32), 'consts': np.array([0.5, 3.0, 0.125]),
          'depth': 1, 'data': np.stack([X, Y, W])}


def test_every_body_opcode():
  prog = _every_opcode_program(9)
  assert {expr.decode(w)[0] for w in prog['code'][3:23]} == set(range(expr.N_OPS))
  expr.check_program(prog['code'], prog['consts'], prog['depth'], 2, prog['data'])
  x0 = np.random.RandomState(12).normal(0., 1., size=(130, 2))
  eng = run(oracle.golden_spec('gmm2'), x0, 12)
  try:
    x = eng.trace()['v_x']
    got = eng.trace_pointwise(prog)
  finally:
    eng.close()
  T = _terms(prog, x)
  assert np.all(np.isfinite(T))
  _check('every opcode', got, T)


# ---------------------------------------------------------------------------
# 5. the tail tile
# ---------------------------------------------------------------------------
def test_nothing_is_written_past_n_obs():
  prog = _every_opcode_program(9)   # two tiles, the second with one observation
  eng = run(oracle.golden_spec('gmm2'), golden_init('gmm2', 130), 12)
  try:
    want = eng.trace_pointwise(prog)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    code = np.ascontiguousarray(prog['code'], np.int32)
    consts, data = np.ascontiguousarray(prog['consts']), np.ascontiguousarray(prog['data'])
    bufs = [np.full(64, -777.25) for _ in range(3)]
    _lib.call('pbh_trace_pointwise', eng._h, ctypes.c_int64(0), ctypes.c_int64(12),
              code.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.c_int32(code.size),
              dp(consts), ctypes.c_int32(consts.size), ctypes.c_int32(prog['depth']), dp(data),
              ctypes.c_int32(3), ctypes.c_int32(9), dp(bufs[0]), dp(bufs[1]), dp(bufs[2]))
    # and with outputs left out
    only = np.full(64, -777.25)
    _lib.call('pbh_trace_pointwise', eng._h, ctypes.c_int64(0), ctypes.c_int64(12),
              code.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.c_int32(code.size),
              dp(consts), ctypes.c_int32(consts.size), ctypes.c_int32(prog['depth']), dp(data),
              ctypes.c_int32(3), ctypes.c_int32(9), None, dp(only), None)
  finally:
    eng.close()
  for key, buf in zip(('lse', 'mean', 'var'), bufs):
    assert np.array_equal(buf[:9], want[key]) and np.all(buf[9:] == -777.25), key
  assert np.array_equal(only[:9], want['mean']) and np.all(only[9:] == -777.25)


# ---------------------------------------------------------------------------
# 6. leaves everything else alone
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('n', [130, 257])
def test_no_side_effects(n):
  prog = _program('logistic', ['a', 'b'])
  check_no_side_effects(lambda eng: eng.trace_pointwise(prog, 0, 64), n)


def test_an_expression_engine_keeps_its_own_program():
  """An engine whose own target is the data_linreg3 program makes the call with
  the logistic program over other data, and runs on bit-equal to a twin that
  never made it."""
  spec = _linreg_spec()
  prog = PROGRAMS[40]()
  engs = []
  try:
    for _ in range(2):
      eng = Engine(spec)
      engs.append(eng)
      eng.init_chains(_linreg_starts(257))
      eng.set_rng('philox', seed=3)
      eng.alloc_trace(32, 1)
      eng.run(16, steps_per_launch=64)
    before = engs[0].trace()['v_x']
    assert before.shape == (257, 16, 3)
    _check('own program', engs[0].trace_pointwise(prog), _terms(prog, before))
    for eng in engs:
      eng.run(16, steps_per_launch=64)
    a, b = engs[0].trace(), engs[1].trace()
    assert a['v_x'].shape == (257, 32, 3) and not np.array_equal(a['v_x'][:, 16:], before)
    for k in ('v_x', 'v_p', 'u'):
      assert np.array_equal(a[k], b[k]), k
  finally:
    for eng in engs:
      eng.close()


# ---------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------
def test_refusals():
  E, col, var, acc = expr.encode, (expr.VAR, expr.BODY_BASE), (expr.VAR, 0), (expr.ACC, 0)
  region = [E(expr.LOOP, (expr.SLOT, 1)), E(expr.MUL, col, var), E(expr.SUM, acc)]
  def prog(code, depth=1):
    return {'code': np.array(code, np.int32), 'consts': np.zeros(0), 'depth': depth,
            'data': np.arange(9.)[None, :]}
  good = prog(region)
  eng = Engine(oracle.golden_spec('gmm2'))
  try:
    eng.init_chains(golden_init('gmm2', 12))
    eng.set_rng('philox', seed=3)
    with pytest.raises(PbhError, match='no trace') as e:
      eng.trace_pointwise(good, 0, 4)
    assert e.value.code != 0
    eng.alloc_trace(40, 1)
    eng.run(40, steps_per_launch=64)
    for first, count in ((0, 41), (-1, 4), (38, 3), (40, 1), (0, 0)):
      with pytest.raises(PbhError, match='outside'):
        eng.trace_pointwise(good, first, count)
    two = region[:2] + [E(expr.SUM, acc, dst=0, store=True)] + region
    with pytest.raises(PbhError, match='several'):
      eng.trace_pointwise(prog(two))
    with pytest.raises(PbhError, match='SUM'):
      eng.trace_pointwise(prog(region + [E(expr.NEG, acc)]))
    with pytest.raises(PbhError, match='none'):
      eng.trace_pointwise(prog([E(expr.MUL, var, var)]))
    with pytest.raises(PbhError, match='bad program at word 1'):
      eng.trace_pointwise(prog(region[:1] + [E(63, col)] + region[2:]))
    with pytest.raises(PbhError, match='bad program'):
      eng.trace_pointwise(prog([-5] + region))
    # the engine works on
    x = eng.trace()['v_x']
    _check('after refusals', eng.trace_pointwise(good), _terms(good, x))
  finally:
    eng.close()
  one = run(oracle.golden_spec('gmm2'), golden_init('gmm2', 1), 4)
  try:
    with pytest.raises(PbhError, match='2 draws'):
      one.trace_pointwise(good, 1, 1)
    assert np.all(np.isfinite(one.trace_pointwise(good, 1, 2)['var']))
  finally:
    one.close()


# ---------------------------------------------------------------------------
# 8. determinism
# ---------------------------------------------------------------------------
def test_two_calls_give_the_same_bits(linreg_runs):
  progs, _ = linreg_runs
  eng = run(_linreg_spec(), _linreg_starts(515), 10)
  try:
    a = [eng.trace_pointwise(progs[137], 1, 9) for _ in range(3)]
  finally:
    eng.close()
  for other in a[1:]:
    for k in ('lse', 'mean', 'var'):
      assert a[0][k].tobytes() == other[k].tobytes(), k


# ---------------------------------------------------------------------------
# 9. the facade
# ---------------------------------------------------------------------------
def test_facade_waic_and_fitted_values():
  rs = np.random.RandomState(11)
  Y, X = rs.normal(0.2, 1.1, 11), rs.normal(0., 1., 11)
  with sampler_block(130) as (sampler, process, x, keys, v):
    key = keys[0]
    got = sampler.trace_waic(lambda **kw: scipy.stats.norm.logpdf(Y, kw[key], 1.))
    part = sampler.trace_waic(lambda **kw: scipy.stats.norm.logpdf(Y, kw[key], 1.), 7, 50)
    fit = sampler.trace_pointwise(lambda **kw: kw[key] * X)
    with pytest.raises(ValueError):
      sampler.trace_pointwise(lambda **kw: kw[key] * X, 90, 10)
  for what, res, xs in (('all', got, x), ('[7, 57)', part, x[:, 7:57])):
    draws = xs[:, :, 0].reshape(-1, 1)   # the first name's values
    T = scipy.stats.norm.logpdf(Y[None, :], draws, 1.)
    S = T.shape[0]
    lse, mean, var = diag.pointwise_stats(T)
    want = diag.waic(lse, mean, var, S)
    truth, rel = _var_bounds(T)
    b_lppd = RTOL * np.maximum(np.abs(lse), 1.)
    b_p = (rel * np.abs(truth)).astype(float) + np.abs(var - truth).astype(float)
    bounds = {'lppd_i': b_lppd, 'p_waic_i': b_p, 'elpd_i': b_lppd + b_p, 'lppd': b_lppd.sum(),
              'p_waic': b_p.sum(), 'elpd_waic': (b_lppd + b_p).sum(), 'se': (b_lppd + b_p).sum(),
              'waic': 2. * (b_lppd + b_p).sum()}
    assert sorted(res) == sorted(want) == sorted(bounds)
    for k, bound in bounds.items():
      err = np.abs(np.asarray(res[k]) - np.asarray(want[k]))
      print('waic', what, k, 'max err', float(np.max(err)), 'bound', float(np.max(bound)))
      assert np.all(err <= bound), (what, k)
  draws = x[:, :, 0].reshape(-1, 1)
  _check('fitted values', fit, draws * X[None, :])
