"""Likelihoods summed over observed data arrays on the CPU: the densities of
expr_data_examples.py lower to an expression program with loop regions
(probayes_amd/expr.py), the NumPy interpreter of that program equals the
callable called point by point (bit for bit where the body is IEEE arithmetic
alone, which pins the pairwise order of the sum), what stays outside is
refused with its cause, the program checks reject malformed regions, and the
CPU oracle with the interpreter as its density reproduces the reference's
recorded chains."""
import numpy as np
import pytest
import scipy.stats

import oracle
import oracle.mh
import probayes_amd as pb
from probayes_amd import expr
from probayes_amd.lower import NotLowerable
from expr_data_examples import DATA_WORKLOADS, DATA_DENSITIES, LIN_X, LIN_Y

RTOL = 1e-12          # the project's parity bar (tests/test_gpu_parity.py)
SIZES = [1, 7, 8, 9, 127, 128, 129, 137, 300, 1000]


def _rel_err(a, b, floor=np.finfo(float).tiny):
  a, b = np.asarray(a, float), np.asarray(b, float)
  same = (a == b) | (np.isnan(a) & np.isnan(b))
  err = np.where(same, 0., np.abs(a - b) / np.maximum(np.abs(b), floor))
  return float(err.max()) if err.size else 0.


def _points(name, n=200):
  """Random points inside each model's support, [n, d]."""
  rs = np.random.RandomState(321)
  if name == 'data_linreg3':
    return np.stack([rs.uniform(-5., 5., n), rs.uniform(-5., 5., n),
                     rs.uniform(0.05, 10., n)], -1)
  if name == 'data_logistic2':
    return rs.normal(0., 2., size=(n, 2))
  return np.stack([rs.uniform(-10., 10., n), rs.uniform(0.05, 10., n)], -1)


# ---------------------------------------------------------------------------
# lowering
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(DATA_WORKLOADS))
def test_data_densities_lower_to_expr_with_data(name):
  builder, params = DATA_WORKLOADS[name][:2]
  process, init, extra, kwds, keys = builder(pb, params)
  spec = process.lower()
  tg = spec['target']
  assert tg['kind'] == 'expr' and spec['pscale'] == 'log'
  n_obs = {'data_linreg3': 137, 'data_logistic2': 40, 'data_robust2': 7}[name]
  assert tg['data'].dtype == np.float64 and tg['data'].shape == (2, n_obs)
  ops = [expr.decode(w)[0] for w in tg['code']]
  assert ops.count(expr.LOOP) == ops.count(expr.SUM) == (2 if name == 'data_robust2' else 1)
  assert len(tg['code']) <= expr.MAX_CODE and tg['depth'] <= expr.MAX_SLOTS
  expr.check_program(tg['code'], tg['consts'], tg['depth'], len(keys), tg['data'])
  x = _points(name)
  fn = DATA_DENSITIES[name]
  want = np.array([fn(*[np.float64(v) for v in p]) for p in x])
  got = expr.evaluate(tg['code'], tg['consts'], x, tg['data'])
  assert got.shape == want.shape and np.all(np.isfinite(want))
  print(name, 'max rel err', _rel_err(got, want, 1.))
  assert _rel_err(got, want, 1.) <= RTOL
  assert abs(expr.evaluate(tg['code'], tg['consts'], x[7], tg['data']) - want[7]) \
      <= RTOL * max(1., abs(want[7]))


def _data(n, seed=50):
  rs = np.random.RandomState(seed + n)
  return rs.normal(0., 1.5, n), rs.normal(1., 2., n), rs.uniform(0.5, 2., n)


def _arith_fn(X, Y, W):
  """+ - * / sqrt abs alone: every operation is IEEE in NumPy and in the
  interpreter, so only the order of the sum can differ."""
  def fn(a, b):
    r = (Y - (a + b * X)) / W
    return np.sum(np.sqrt(abs(r) + 0.25) * r - r * r / (abs(b) + 1.5)) - a * a / 7.
  return fn


def _mixed_fn(X, Y, W):
  def fn(a, b):
    eta = a + b * X
    return np.mean(Y * eta - np.log1p(np.exp(eta))) + \
        np.sum(scipy.stats.norm.logpdf(Y, eta, W)) / len(X) - np.log(abs(b) + 1.)
  return fn


@pytest.mark.parametrize('n', SIZES)
def test_evaluate_equals_the_callable_point_by_point(n):
  X, Y, W = _data(n)
  pts = np.random.RandomState(9).normal(0., 1., size=(23, 2))
  fn = _arith_fn(X, Y, W)
  tg = expr.trace_expr(lambda **kw: fn(kw['a'], kw['b']), ['a', 'b'])
  assert tg['data'].shape == (3, n)
  used = {expr.decode(w)[0] for w in tg['code']}
  assert used <= {expr.ADD, expr.SUB, expr.MUL, expr.DIV, expr.SQRT, expr.ABS,
                  expr.NEG, expr.MOV, expr.LOOP, expr.SUM}
  expr.check_program(tg['code'], tg['consts'], tg['depth'], 2, tg['data'])
  want = np.array([fn(np.float64(p[0]), np.float64(p[1])) for p in pts])
  got = expr.evaluate(tg['code'], tg['consts'], pts, tg['data'])
  assert np.all(np.isfinite(want))
  assert np.array_equal(got, want)          # bit for bit: NumPy's pairwise order
  assert expr.evaluate(tg['code'], tg['consts'], pts[3], tg['data']) == want[3]
  fn = _mixed_fn(X, Y, W)
  tg = expr.trace_expr(lambda **kw: fn(kw['a'], kw['b']), ['a', 'b'])
  expr.check_program(tg['code'], tg['consts'], tg['depth'], 2, tg['data'])
  want = np.array([fn(np.float64(p[0]), np.float64(p[1])) for p in pts])
  got = expr.evaluate(tg['code'], tg['consts'], pts, tg['data'])
  assert _rel_err(got, want, 1.) <= RTOL


def test_a_sequential_sum_is_told_apart():
  """The check above has teeth: at n > 8 a left-to-right sum of the same
  terms differs from NumPy's pairwise sum at some point."""
  X, Y, W = _data(137)
  pts = np.random.RandomState(9).normal(0., 1., size=(23, 2))
  def terms(a, b):
    r = (Y - (a + b * X)) / W
    return np.sqrt(abs(r) + 0.25) * r - r * r / (abs(b) + 1.5)
  seq = np.array([np.cumsum(terms(*p))[-1] for p in pts])
  pair = np.array([np.sum(terms(*p)) for p in pts])
  assert not np.array_equal(seq, pair)


def test_columns_are_deduplicated_and_host_subexpressions_are_numpys():
  X, Y, W = _data(40)
  Xc = X - X.mean()
  def fn(**kw):
    # X - X.mean() twice (two arrays, the same bytes), Y as int and as float
    return np.sum((Y - kw['a'] * (X - X.mean())) ** 2) + \
        np.sum(abs(Y - kw['b'] * (X - np.mean(X))))
  tg = expr.trace_expr(fn, ['a', 'b'])
  assert tg['data'].shape == (2, 40)
  assert any(np.array_equal(c, Xc) for c in tg['data'])     # NumPy's own values
  assert any(np.array_equal(c, Y) for c in tg['data'])
  # an integer / bool array becomes a float64 column
  K = (Y > 1.).astype(np.int64)
  tg = expr.trace_expr(lambda **kw: np.sum(K * kw['a'] - (K > 0) * kw['b']), ['a', 'b'])
  assert tg['data'].dtype == np.float64 and tg['data'].shape == (1, 40)
  # a sum feeds a later region's body; .sum() / .mean() methods
  def two(**kw):
    m = (kw['a'] * X).mean()
    return -((Y - m - kw['b']) ** 2).sum()
  tg = expr.trace_expr(two, ['a', 'b'])
  pts = np.random.RandomState(2).normal(size=(17, 2))
  want = np.array([two(a=np.float64(p[0]), b=np.float64(p[1])) for p in pts])
  assert np.array_equal(expr.evaluate(tg['code'], tg['consts'], pts, tg['data']), want)
  # traced norm.logpdf on arrays is scipy's array result, bit for bit
  def lp(**kw):
    return np.sum(scipy.stats.norm.logpdf(LIN_Y, kw['b0'] + kw['b1'] * LIN_X, kw['s']))
  tg = expr.trace_expr(lp, ['b0', 'b1', 's'])
  pts = _points('data_linreg3', 50)
  want = np.array([lp(b0=p[0], b1=p[1], s=p[2]) for p in pts])
  assert np.array_equal(expr.evaluate(tg['code'], tg['consts'], pts, tg['data']), want)


def test_scalar_programs_keep_their_words():
  """A density without arrays holds no region and no data block."""
  tg = expr.trace_expr(lambda **kw: np.exp(kw['x']) * kw['y'] - np.log1p(kw['x'] ** 2),
                       ['x', 'y'])
  assert 'data' not in tg
  assert all(expr.decode(w)[0] < expr.N_OPS for w in tg['code'])
  assert expr.N_OPS == 15 and expr.LOOP == 32 and expr.SUM == 33


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
_X40, _Y40, _W40 = _data(40)
_X9 = _data(9)[0]


def _nine_columns(**kw):
  return np.sum(sum(kw['x'] * (_X40 + float(i)) for i in range(9)))


def _five_temps(**kw):
  v = [np.exp(kw['x'] * (_X40 + float(i))) for i in range(5)]
  out = v[0] + v[1] + v[2] + v[3] + v[4]
  for t in v:
    out = out * t
  return np.sum(out) + kw['y']


REFUSED_DATA = {
    'sum of a scalar': (lambda **kw: np.sum(kw['x'] * kw['y']), 'scalar'),
    'mean of a scalar': (lambda **kw: (kw['x'] * kw['y']).mean(), 'scalar'),
    'add.reduce': (lambda **kw: np.add.reduce(kw['x'] * _X40) + kw['y'], 'reduc'),
    'np.max': (lambda **kw: np.max(kw['x'] * _X40) + kw['y'], 'max'),
    'np.prod': (lambda **kw: np.prod(kw['x'] * _X40) + kw['y'], 'prod'),
    'np.cumsum': (lambda **kw: np.cumsum(kw['x'] * _X40)[-1] + kw['y'], 'cumsum'),
    'unreduced': (lambda **kw: kw['x'] * _X40 + kw['y'], 'unreduced'),
    'iterating': (lambda **kw: sum(kw['x'] * _X40) + kw['y'], 'iterating'),
    'indexing': (lambda **kw: (kw['x'] * _X40)[0] + kw['y'], 'indexing'),
    'len': (lambda **kw: np.sum(kw['x'] * _X40) / len(kw['y'] * _X40), 'len'),
    'two lengths': (lambda **kw: np.sum(kw['x'] * _X40) + np.sum(kw['y'] * _X9),
                    'lengths'),
    'two lengths in one term': (lambda **kw: np.sum(kw['x'] * _X40[:9] + kw['y'] * _X9[:8]),
                                'lengths'),
    '2-D': (lambda **kw: np.sum(kw['x'] * np.ones((4, 10))) + kw['y'], '2-D'),
    'nine columns': (_nine_columns, 'columns'),
    'five temporaries': (_five_temps, 'intermediate'),
    'too many observations': (lambda **kw: np.sum(kw['x'] * np.ones(expr.MAX_OBS + 1)),
                              'observations'),
    'axis=': (lambda **kw: np.sum(kw['x'] * _X40, axis=0) + kw['y'], 'options'),
    'dtype=': (lambda **kw: np.sum(kw['x'] * _X40, dtype=np.float32), 'options'),
    'keepdims=': (lambda **kw: np.mean(kw['x'] * _X40, keepdims=True), 'options'),
    'where=': (lambda **kw: np.sum(kw['x'] * _X40, where=_X40 > 0), 'options'),
    'method axis': (lambda **kw: (kw['x'] * _X40).sum(0) + kw['y'], 'options'),
    'unshifted log-sum-exp': (lambda **kw: np.log(np.sum(np.exp(kw['x'] * _X40))) + kw['y'],
                              'shift'),
    'array exponent': (lambda **kw: np.sum(abs(kw['x']) ** _X40) + kw['y'], 'exponent'),
}


@pytest.mark.parametrize('what', sorted(REFUSED_DATA))
def test_data_refusals_name_the_cause(what):
  fn, word = REFUSED_DATA[what]
  with pytest.raises(NotLowerable) as e:
    expr.trace_expr(fn, ['x', 'y'])
  assert word in str(e.value), str(e.value)


def test_the_limits_themselves_lower():
  """8 columns, 4 temporaries and 65 536 observations are inside."""
  def eight(**kw):
    return np.sum(sum(kw['x'] * (_X40 + float(i)) for i in range(8)))
  assert expr.trace_expr(eight, ['x'])['data'].shape == (8, 40)
  tg = expr.trace_expr(lambda **kw: np.sum(kw['x'] * np.ones(expr.MAX_OBS)), ['x'])
  assert tg['data'].shape == (1, expr.MAX_OBS)
  assert expr.evaluate(tg['code'], tg['consts'], [0.5], tg['data']) == 0.5 * expr.MAX_OBS


# ---------------------------------------------------------------------------
# program checks
# ---------------------------------------------------------------------------
def test_region_checks():
  E, V, C, A, S, B = expr.encode, expr.VAR, expr.CONST, expr.ACC, expr.SLOT, expr.BODY_BASE
  data = np.ones((2, 9))
  loop = lambda n: E(expr.LOOP, (S, n))
  total = lambda **kw: E(expr.SUM, (A, 0), **kw)
  good = [E(expr.EXP, (V, 0), dst=0, store=True),
          loop(3),
          E(expr.MUL, (V, B + 0), (S, 0), dst=1, store=True),     # temporary 1
          E(expr.ADD, (A, 0), (V, B + 1)),
          E(expr.SUB, (A, 0), (S, B + 1)),
          total(dst=0, store=True),
          E(expr.ADD, (A, 0), (S, 0))]
  expr.check_program(good, [], 1, 1, data)
  x = np.array([[0.3], [-1.2]])
  want = 2. * (9 * (np.exp(x[:, 0]) + 1. - np.exp(x[:, 0])))
  assert np.allclose(expr.evaluate(good, [], x, data), want, rtol=1e-15, atol=0)
  spec = pb.make_spec(1, {'kind': 'expr', 'code': good, 'consts': [], 'depth': 1,
                          'data': data}, {'kind': 'gauss', 'scale': 1.}, pscale='log')
  assert spec['target']['data'].shape == (2, 9)

  def bad(code, depth=1, dat=data):
    with pytest.raises(ValueError):
      expr.check_program(code, [], depth, 1, dat)
    with pytest.raises(ValueError):
      pb.make_spec(1, {'kind': 'expr', 'code': code, 'consts': [], 'depth': depth,
                       'data': dat}, {'kind': 'gauss', 'scale': 1.}, pscale='log')

  body = [E(expr.MUL, (V, B + 0), (V, 0))]
  bad([loop(3), loop(1)] + body + [total(), total()])                  # nested
  bad([loop(1), E(expr.MUL, (V, B + 2), (V, 0)), total()])             # column 2 of 2
  bad([loop(1), E(expr.MUL, (V, B + 0), (S, B + 0)), total()])         # unwritten temporary
  bad([loop(1), E(expr.MUL, (V, B + 0), (S, B + 4)), total()])         # temporary 4 of 4
  bad([loop(1), E(expr.MUL, (V, B + 0), (V, 0), dst=4, store=True), total()])  # writes past
                                                                       # the temporaries
  bad([loop(1), E(expr.NEG, (A, 0)), total()])                         # acc in a first word
  bad([E(expr.NEG, (V, 0)), loop(1), E(expr.NEG, (A, 0)), total()])    # ... the outer acc
  bad([loop(2)] + body + [total()])                                    # no SUM at the end
  bad([loop(1)] + body)                                                # region past the end
  bad([loop(0), total()])                                              # empty body
  bad(body + [total()])                                                # SUM without LOOP
  bad([E(expr.MUL, (V, B + 0), (V, 0))])                               # a column outside
  bad([loop(1), E(expr.MUL, (V, B + 0), (S, 0)), total()])             # unwritten outer slot
  bad([loop(1)] + body + [total()], dat=np.ones((9, 4)))               # nine columns
  bad([loop(1)] + body + [total()], dat=np.ones((1, expr.MAX_OBS + 1)))
  with pytest.raises(ValueError):                                      # a region, no data
    expr.check_program([loop(1)] + body + [total()], [], 0, 1)
  # a body's store names a temporary: the outer slot 0 stays unwritten
  with pytest.raises(ValueError):
    expr.check_program([loop(1), E(expr.MUL, (V, B + 0), (V, 0), dst=0, store=True),
                        total(), E(expr.ADD, (A, 0), (S, 0))], [], 1, 1, data)


# ---------------------------------------------------------------------------
# the CPU oracle with the interpreter as its density, against the reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(DATA_WORKLOADS))
def test_oracle_with_the_interpreter_reproduces_the_golden(name, monkeypatch):
  builder, params, n, t, seed0 = DATA_WORKLOADS[name]
  process, init, extra, kwds, keys = builder(pb, params)
  g = oracle.load_golden(name)
  assert g['v_x'].shape[:2] == (n, t) and 0.1 < g['u'].mean() < 0.9
  spec = process.lower()
  tg = spec['target']
  monkeypatch.setattr(
      oracle.mh, 'target_prob',
      lambda spec, x: expr.evaluate(tg['code'], tg['consts'], np.asarray(x).T, tg['data']))
  streams = oracle.legacy_streams(spec, g['seeds'], t)
  x0 = np.tile(np.array([init[k] for k in keys], np.float64), (n, 1))
  out = oracle.run_mh(spec, x0, streams)
  flips = int(np.sum(out['u'] != g['u']))
  print(name, 'flips', flips, 'v_x', _rel_err(out['v_x'], g['v_x'], 1.),
        'v_p', _rel_err(out['v_p'], g['v_p']), 'p_p', _rel_err(out['p_p'], g['p_p']))
  assert flips == 0
  assert _rel_err(out['v_x'], g['v_x'], 1.) <= RTOL
  assert _rel_err(out['v_p'], g['v_p']) <= RTOL
  assert _rel_err(out['p_x'], g['p_x'], 1.) <= RTOL
  assert _rel_err(out['p_p'], g['p_p']) <= RTOL
