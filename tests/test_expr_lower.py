"""The expression target on the CPU: user-written scalar densities lower to a
program (probayes_amd/expr.py), the NumPy interpreter of that program equals
the callable bit for bit, the closed forms still lower to themselves, and
everything outside the listed operations raises NotLowerable."""
import numpy as np
import pytest
import scipy.special
import scipy.stats

import probayes_amd as pb
from probayes_amd import _lib, expr
from probayes_amd.lower import NotLowerable
from expr_examples import EXPR_WORKLOADS, DENSITIES
from mcmc_examples import WORKLOADS


def _points(name, n=1000):
  """Random points inside each model's support, [n, d]."""
  rs = np.random.RandomState(123)
  if name == 'expr_banana2':
    return rs.normal(0., 2., size=(n, 2))
  if name == 'expr_well1':
    return rs.normal(0., 1.5, size=(n, 1))
  return np.stack([rs.uniform(0.05, 12., n), rs.uniform(-3., 3., n)], -1)


@pytest.mark.parametrize('name', sorted(EXPR_WORKLOADS))
def test_user_densities_lower_to_expr(name):
  builder, params = EXPR_WORKLOADS[name][:2]
  process, init, extra, kwds, keys = builder(pb, params)
  spec = process.lower()
  tg = spec['target']
  assert tg['kind'] == 'expr'
  assert spec['pscale'] == ('lin' if name == 'expr_well1' else 'log')
  assert tg['code'].dtype == np.int32 and tg['consts'].dtype == np.float64
  assert 1 <= len(tg['code']) <= expr.MAX_CODE and tg['depth'] <= expr.MAX_SLOTS
  expr.check_program(tg['code'], tg['consts'], tg['depth'], len(keys))
  # bit for bit the callable itself on arrays: both run the same NumPy loops
  x = _points(name)
  with np.errstate(all='ignore'):
    want = DENSITIES[name](*[np.ascontiguousarray(x[:, i]) for i in range(len(keys))])
  got = expr.evaluate(tg['code'], tg['consts'], x)
  assert got.shape == want.shape and np.all(np.isfinite(want))
  assert np.array_equal(got, want)
  # and one point at a time
  assert expr.evaluate(tg['code'], tg['consts'], x[7]) == want[7]


@pytest.mark.parametrize('name,kind', [('diag10', 'diag_gauss'), ('gmm2', 'gmm')])
def test_closed_forms_still_lower_to_themselves(name, kind):
  builder, params = WORKLOADS[name][:2]
  process = builder(pb, params)[0]
  assert process.lower()['target']['kind'] == kind


def _lower1(fn, **kw):
  x = pb.RV('x', vtype=float, vset=(-np.inf, np.inf))
  y = pb.RV('y', vtype=float, vset=(-np.inf, np.inf))
  process = pb.SP(x & y)
  process.set_prob(fn, pscale='log')
  process.set_tran(lambda **kw: 1.)
  process.set_delta(lambda: process.Delta(x=scipy.stats.norm.rvs(),
                                          y=scipy.stats.norm.rvs()))
  process.set_scores('hastings')
  return process.lower()


_MU = np.array([[0., 1.], [1., 0.], [2., 2.]])


def _branch(**kw):
  if kw['x'] > 0:
    return -kw['x']
  return kw['x']


def _many_consts(**kw):
  out = kw['x']
  for i in range(expr.MAX_CONSTS + 1):
    out = out * (1. + i / 1000.)
  return out


def _too_long(**kw):
  out = kw['x']
  for i in range(expr.MAX_CODE + 1):
    out = out + kw['y']
  return out


def _too_deep(**kw):
  # every value is read twice, far apart: all of them are alive at once
  vals = [np.exp(kw['x'] * float(i + 1)) for i in range(expr.MAX_SLOTS + 1)]
  out = sum(vals)
  for v in vals:
    out = out * v
  return out


REFUSED = {
    'cos': lambda **kw: np.cos(kw['x']) + kw['y'],
    'tanh': lambda **kw: np.tanh(kw['x']) * kw['y'],
    'np.sum': lambda **kw: np.sum(kw['x']) + kw['y'],
    'add.reduce': lambda **kw: np.add.reduce(kw['x']) + kw['y'],
    'array constant': lambda **kw: kw['x'] * np.array([1., 2.]) + kw['y'],
    'mixture over arrays': lambda **kw: np.max(
        scipy.stats.norm.logpdf(kw['x'], _MU[:, 0], 1.) + kw['y']),
    'np.where': lambda **kw: np.where(kw['x'] > 0, kw['x'], kw['y']),
    'where without a comparison': lambda **kw: np.where(kw['x'], kw['x'], kw['y']),
    'truth test': _branch,
    'uniform.pdf': lambda **kw: scipy.stats.uniform.pdf(kw['x'], 0., 2.) * kw['y'],
    'symbolic exponent': lambda **kw: kw['x'] ** kw['y'],
    'constant base': lambda **kw: 2. ** kw['x'] + kw['y'],
    'floor division': lambda **kw: kw['x'] // 2. + kw['y'],
    'constants over the limit': _many_consts,
    'code over the limit': _too_long,
    'slots over the limit': _too_deep,
    'not a scalar': lambda **kw: [kw['x'], kw['y']],
}


@pytest.mark.parametrize('what', sorted(REFUSED))
def test_refusals_name_the_cause(what):
  with pytest.raises(NotLowerable) as e:
    _lower1(REFUSED[what])
  assert str(e.value)


def test_seventeen_variables_are_refused():
  keys = ['v{}'.format(i) for i in range(expr.MAX_DIM + 1)]
  with pytest.raises(NotLowerable):
    expr.trace_expr(lambda **kw: sum(kw[k] * kw[k] for k in keys), keys)
  tg = expr.trace_expr(lambda **kw: -sum(kw[k] * kw[k] for k in keys[:-1]), keys[:-1])
  assert tg['kind'] == 'expr'


def test_shared_values_are_evaluated_once():
  """y = y * y + x twenty times: a tree would hold 2^20 copies of x; the
  program is linear in the source operations (40 of them)."""
  def fn(**kw):
    x = kw['x']
    y = x
    for _ in range(20):
      y = y * y + x
    return y
  tg = expr.trace_expr(fn, ['x'])
  assert len(tg['code']) <= 4 * 40
  pts = np.random.RandomState(5).uniform(-0.7, 0.25, size=(500, 1))
  want = fn(x=pts[:, 0])
  assert np.array_equal(expr.evaluate(tg['code'], tg['consts'], pts), want)
  # a value read long after it was computed lives in a slot
  def far(**kw):
    e = np.exp(kw['x'])
    z = (kw['x'] * 3. + 1.) / 7.
    return z * z - e + e * z
  tg = expr.trace_expr(far, ['x'])
  assert tg['depth'] >= 1
  assert np.array_equal(expr.evaluate(tg['code'], tg['consts'], pts), far(x=pts[:, 0]))


def test_host_constants_and_scipy_order():
  """A subexpression without a variable is NumPy's value on the host; the
  norm densities expand in scipy's operation order (bit-equal to scipy)."""
  c = np.log(3.) * np.sqrt(2.)
  tg = expr.trace_expr(lambda **kw: kw['x'] * (np.log(3.) * np.sqrt(2.)), ['x'])
  assert len(tg['code']) == 1 and list(tg['consts']) == [c]
  pts = np.random.RandomState(6).normal(size=(300, 2))
  pts[:, 1] = np.abs(pts[:, 1]) + 0.1
  for name in ('logpdf', 'pdf'):
    def f(*args, **kwds):   # looked up at the call, as user code does
      return getattr(scipy.stats.norm, name)(*args, **kwds)
    tg = expr.trace_expr(lambda **kw: f(kw['x'], 0.25, kw['s']), ['x', 's'])
    assert np.array_equal(expr.evaluate(tg['code'], tg['consts'], pts),
                          f(pts[:, 0], 0.25, pts[:, 1]))
    tg = expr.trace_expr(lambda **kw: f(1.5, loc=kw['x'], scale=2.) + kw['s'], ['x', 's'])
    assert np.array_equal(expr.evaluate(tg['code'], tg['consts'], pts),
                          f(1.5, loc=pts[:, 0], scale=2.) + pts[:, 1])
  # Python sum starts from 0; max / min / abs / neg / expm1 / square
  def fn(**kw):
    x, s = kw['x'], kw['s']
    return sum([np.maximum(x, 0.5) * 2., np.minimum(s, x), abs(-x),
                np.expm1(np.square(x) / 10.), x ** 1.5 if False else s ** 1.5])
  tg = expr.trace_expr(fn, ['x', 's'])
  assert np.array_equal(expr.evaluate(tg['code'], tg['consts'], pts),
                        fn(x=pts[:, 0], s=pts[:, 1]))


def test_program_checks():
  good = expr.trace_expr(lambda **kw: np.exp(kw['x']) * kw['y'], ['x', 'y'])
  expr.check_program(good['code'], good['consts'], good['depth'], 2)
  bad_var = [expr.encode(expr.ADD, (expr.VAR, 2), (expr.VAR, 0))]
  bad_slot = [expr.encode(expr.NEG, (expr.SLOT, 0))]
  bad_acc = [expr.encode(expr.NEG, (expr.ACC, 0))]
  bad_op = [expr.encode(expr.N_OPS, (expr.VAR, 0))]
  bad_const = [expr.encode(expr.MUL, (expr.VAR, 0), (expr.CONST, 0))]
  for code in (bad_var, bad_slot, bad_acc, bad_op, bad_const, []):
    with pytest.raises(ValueError):
      expr.check_program(code, [], 1, 2)
    with pytest.raises(ValueError):
      pb.make_spec(2, {'kind': 'expr', 'code': code, 'consts': [], 'depth': 1},
                   {'kind': 'gauss', 'scale': 1.}, pscale='log')


def test_abi_version():
  assert _lib.ABI_VERSION == 7
  assert _lib.TARGET['expr'] == 7
