"""Pointwise functions on the CPU: a callable that returns the unreduced vector
of per-observation terms lowers to the program of its sum (expr.trace_pointwise:
scalar words, LOOP, the body, SUM last), the NumPy interpreter's terms
(expr.evaluate_pointwise) equal the callable called point by point (bit for bit
where the body is IEEE arithmetic alone), their sum is evaluate()'s, what
stays outside is refused with its cause, and evaluate() itself gives what it
gave."""
import numpy as np
import pytest
import scipy.stats

import probayes_amd as pb
from probayes_amd import expr
from probayes_amd.lower import NotLowerable
from expr_data_examples import (DATA_WORKLOADS, DATA_DENSITIES, LIN_X, LIN_Y, LOG_X, LOG_Y,
                                ROB_Y, ROB_Z)

RTOL = 1e-12          # the project's parity bar (tests/test_gpu_parity.py)


def linreg_terms(b0, b1, s):
  return scipy.stats.norm.logpdf(LIN_Y, b0 + b1 * LIN_X, s)


def logistic_terms(a, b):
  eta = a + b * LOG_X
  return LOG_Y * eta - np.log1p(np.exp(eta))


def robust_cauchy_terms(m, s):
  return -np.log1p(((ROB_Y - m) / s) ** 2) - np.log(s)


def robust_pull_terms(m, s):
  return -abs(ROB_Z - m)


# name: (the terms, the keys, n, whether the body is IEEE arithmetic alone)
TERMS = {
  'linreg': (linreg_terms, ['b0', 'b1', 's'], 137, False),
  'logistic': (logistic_terms, ['a', 'b'], 40, False),
  'robust_cauchy': (robust_cauchy_terms, ['m', 's'], 7, False),
  'robust_pull': (robust_pull_terms, ['m', 's'], 7, True),
}


def program(name):
  fn, keys = TERMS[name][:2]
  return expr.trace_pointwise(lambda **kw: fn(*[kw[k] for k in keys]), keys)


def points(name, n=60):
  """Random points inside each model's support, [n, d]."""
  rs = np.random.RandomState(322)
  if name == 'linreg':
    return np.stack([rs.uniform(-5., 5., n), rs.uniform(-5., 5., n),
                     rs.uniform(0.05, 10., n)], -1)
  if name == 'logistic':
    return rs.normal(0., 2., size=(n, 2))
  return np.stack([rs.uniform(-10., 10., n), rs.uniform(0.05, 10., n)], -1)


def rel_err(a, b, floor=1.):
  a, b = np.asarray(a, float), np.asarray(b, float)
  same = (a == b) | (np.isnan(a) & np.isnan(b))
  err = np.where(same, 0., np.abs(a - b) / np.maximum(np.abs(b), floor))
  return float(err.max()) if err.size else 0.


def pointwise_shape(code):
  """(where the LOOP stands, how many there are, whether SUM is the last word)"""
  ops = [expr.decode(w)[0] for w in code]
  return ops.index(expr.LOOP), ops.count(expr.LOOP), ops[-1] == expr.SUM


@pytest.mark.parametrize('name', sorted(TERMS))
def test_term_functions_lower_to_the_pointwise_shape(name):
  fn, keys, n, ieee = TERMS[name]
  tg = program(name)
  assert sorted(tg) == ['code', 'consts', 'data', 'depth', 'kind'] and tg['kind'] == 'expr'
  assert tg['code'].dtype == np.int32 and tg['consts'].dtype == np.float64
  assert tg['data'].dtype == np.float64 and tg['data'].shape[1] == n
  expr.check_program(tg['code'], tg['consts'], tg['depth'], len(keys), tg['data'])
  at, loops, last = pointwise_shape(tg['code'])
  assert loops == 1 and last
  assert at + expr.decode(tg['code'][at])[3][1] + 1 == len(tg['code']) - 1
  x = points(name)
  want = np.array([fn(*[np.float64(v) for v in p]) for p in x])
  got = expr.evaluate_pointwise(tg['code'], tg['consts'], x, tg['data'])
  assert got.shape == want.shape == (len(x), n) and np.all(np.isfinite(want))
  print(name, 'max rel err', rel_err(got, want))
  if ieee:
    assert np.array_equal(got, want)
  else:
    assert rel_err(got, want) <= RTOL
  one = expr.evaluate_pointwise(tg['code'], tg['consts'], x[5], tg['data'])
  assert one.shape == (n,) and np.array_equal(one, got[5])
  # the program is that of the sum: evaluate() reduces the same terms
  total = expr.evaluate(tg['code'], tg['consts'], x, tg['data'])
  assert np.array_equal(np.add.reduce(got, axis=1), total)


def test_ieee_bodies_are_bit_equal():
  rs = np.random.RandomState(77)
  X, Y, W = rs.normal(0., 1.5, 29), rs.normal(1., 2., 29), rs.uniform(0.5, 2., 29)

  def fn(a, b):
    r = (Y - (a + b * X)) / W
    return np.sqrt(abs(r) + 0.25) * r - r * r / (abs(b) + 1.5)
  tg = expr.trace_pointwise(lambda **kw: fn(kw['a'], kw['b']), ['a', 'b'])
  pts = rs.normal(0., 1., size=(23, 2))
  want = np.array([fn(np.float64(p[0]), np.float64(p[1])) for p in pts])
  got = expr.evaluate_pointwise(tg['code'], tg['consts'], pts, tg['data'])
  assert np.array_equal(got, want)
  assert np.array_equal(np.add.reduce(got, axis=1),
                        expr.evaluate(tg['code'], tg['consts'], pts, tg['data']))


def test_a_column_or_a_constant_vector_is_a_mov():
  for fn, want in ((lambda **kw: LOG_X, LOG_X), (lambda **kw: 2. * LOG_X + 1., 2. * LOG_X + 1.)):
    tg = expr.trace_pointwise(fn, ['a', 'b'])
    expr.check_program(tg['code'], tg['consts'], tg['depth'], 2, tg['data'])
    ops = [expr.decode(w)[0] for w in tg['code']]
    assert ops == [expr.LOOP, expr.MOV, expr.SUM]
    got = expr.evaluate_pointwise(tg['code'], tg['consts'], np.zeros((3, 2)), tg['data'])
    assert np.array_equal(got, np.broadcast_to(want, (3, 40)))


REFUSED = [
  (lambda **kw: np.sum(linreg_terms(kw['a'], kw['b'], 1.)), 'already reduced'),
  (lambda **kw: np.mean(kw['a'] * LOG_X) + kw['b'], 'already reduced'),
  (lambda **kw: 3., 'already reduced'),
  (lambda **kw: kw['a'] * kw['b'], 'depends on no data array'),
  (lambda **kw: kw['a'], 'depends on no data array'),
  (lambda **kw: kw['a'] * LOG_X + kw['b'] * LIN_X, 'two lengths'),
  (lambda **kw: kw['a'] * np.zeros(expr.MAX_OBS + 1), 'observations'),
  (lambda **kw: sum(kw['a'] ** (k + 2) * (LOG_X + k) for k in range(9)), 'data columns'),
  (lambda **kw: np.where(kw['a'] * LOG_X > 0., 1., 0.), 'comparison'),
]


@pytest.mark.parametrize('case', range(len(REFUSED)))
def test_refusals_name_their_cause(case):
  fn, cause = REFUSED[case]
  with pytest.raises(NotLowerable) as e:
    expr.trace_pointwise(fn, ['a', 'b'])
  assert cause in str(e.value), str(e.value)


def test_too_many_temporaries_are_refused():
  def fn(**kw):
    v = [np.exp(kw['a'] * LOG_X + k) for k in range(6)]
    return ((v[0] * v[1]) * (v[2] * v[3])) * (v[4] * v[5]) + v[0] + v[1] + v[2] + v[3] + v[4]
  with pytest.raises(NotLowerable) as e:
    expr.trace_pointwise(fn, ['a', 'b'])
  assert 'intermediate vectors' in str(e.value)


def test_a_density_that_returns_a_vector_still_raises():
  with pytest.raises(NotLowerable) as e:
    expr.trace_expr(lambda **kw: linreg_terms(kw['a'], kw['b'], 1.), ['a', 'b'])
  assert 'unreduced' in str(e.value)


@pytest.mark.parametrize('name', sorted(DATA_WORKLOADS))
def test_evaluate_is_unchanged_on_the_data_goldens(name):
  builder, params = DATA_WORKLOADS[name][:2]
  process, init, extra, kwds, keys = builder(pb, params)
  tg = process.lower()['target']
  rs = np.random.RandomState(321)
  if name == 'data_linreg3':
    x = np.stack([rs.uniform(-5., 5., 200), rs.uniform(-5., 5., 200),
                  rs.uniform(0.05, 10., 200)], -1)
  elif name == 'data_logistic2':
    x = rs.normal(0., 2., size=(200, 2))
  else:
    x = np.stack([rs.uniform(-10., 10., 200), rs.uniform(0.05, 10., 200)], -1)
  fn = DATA_DENSITIES[name]
  want = np.array([fn(*[np.float64(v) for v in p]) for p in x])
  got = expr.evaluate(tg['code'], tg['consts'], x, tg['data'])
  assert got.shape == want.shape and np.all(np.isfinite(want))
  assert rel_err(got, want) <= RTOL
  assert abs(expr.evaluate(tg['code'], tg['consts'], x[7], tg['data']) - want[7]) \
      <= RTOL * max(1., abs(want[7]))
