"""The opcode harness on the CPU: the reference table reproduces from its
generator, the NumPy definition expr.evaluate passes the harness that the device
is held to (tests/test_gpu_expr_ops.py) with its own measured error printed,
and its array form agrees with NumPy's scalar form at every special value."""
import importlib.util
import os

import numpy as np
import pytest

from probayes_amd import expr
import expr_ops_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUMPY_BAR = 1.0       # ulp: the reference measured against the exact table


def _generator():
  spec = importlib.util.spec_from_file_location(
      'gen_expr_ops_golden', os.path.join(ROOT, 'tools', 'gen_expr_ops_golden.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def _evaluate(code, consts, depth, pts, data):
  return expr.evaluate(code, consts, pts, data)


def test_table_reproduces_from_its_generator():
  pytest.importorskip('mpmath')
  fresh, held = _generator().generate(), cases.table()
  assert list(fresh) == list(held)
  for k in held:
    assert fresh[k].dtype == held[k].dtype == np.float64 and fresh[k].shape == held[k].shape, k
    assert fresh[k].tobytes() == held[k].tobytes(), k


def test_table_is_what_the_cases_expect():
  gen, t = _generator(), cases.table()
  assert np.array(gen.SPECIAL).tobytes() == cases.S.tobytes()
  assert np.array(gen.SPECIAL_EXPONENTS).tobytes() == cases.POW_EXPONENTS.tobytes()
  assert os.path.getsize(cases.GOLDEN) <= 400000
  for op in cases.INEXACT:
    for c in cases.classes(op):
      key = '{}.{}.'.format(op, c)
      assert np.all(np.abs(t[key + 'resid']) <= 0.5), key
      assert t[key + 'want'].shape == t[key + 'a'].shape == t[key + 'resid'].shape
  # results beyond both ends of the range, and subnormal ones, are in the table
  pw = np.concatenate([t[k] for k in t if k.startswith('pow.') and k.endswith('.want')])
  assert np.isinf(pw).sum() > 50 and (pw == 0.).sum() > 20
  assert ((np.abs(pw) < cases.TINY) & (pw != 0.)).sum() > 20
  # the special values that have a finite real value are all there
  for op, n in (('exp', 19), ('expm1', 19), ('log', 10), ('log1p', 13)):
    assert t['{}.special.a'.format(op)].size == n, op
  a, b, want, resid = cases.special_cases('pow')
  assert a.size == cases.S.size * cases.POW_EXPONENTS.size
  assert np.isfinite(resid).sum() == t['pow.special.a'].size > 200


@pytest.mark.parametrize('routing', cases.ROUTINGS)
@pytest.mark.parametrize('op', cases.EXACT)
def test_numpy_definition_is_exact_on_the_table(op, routing):
  n = 0
  for c, a, b, want, _ in cases.table_cases(op, routing):
    got = cases.run(_evaluate, op, routing, a, b)
    ok = cases.passes(op, got, cases.through(routing, want))
    assert ok.all(), (op, routing, c, a[~ok][:4], None if b is None else b[~ok][:4],
                      got[~ok][:4], want[~ok][:4])
    n += a.size
  assert n >= 20


@pytest.mark.parametrize('routing', cases.ROUTINGS)
@pytest.mark.parametrize('op', cases.INEXACT)
def test_numpy_definition_is_within_one_ulp_of_the_table(op, routing):
  """expr.evaluate measured by the harness the device is held to: NumPy's own
  libm against the exact values.  Measured: at most 0.66 ulp (pow, exponent
  0.1), 0.62 ulp for exp."""
  worst = 0.
  for c, a, b, want, resid in cases.table_cases(op, routing):
    got = cases.run(_evaluate, op, routing, a, b)
    want = cases.through(routing, want)
    fin = np.isfinite(want) & (want != 0.)
    err = cases.ulp_error(got[fin], want[fin], resid[fin])
    top = float(err.max()) if err.size else 0.
    worst = max(worst, top)
    print('numpy {:6s} {:10s} {:24s} n {:4d} max ulp err {:.3f}'.format(
        op, routing, c, a.size, top))
    ok = cases.passes(op, got, want, resid, NUMPY_BAR)
    assert ok.all(), (op, routing, c, a[~ok][:4], got[~ok][:4], want[~ok][:4])
  assert worst <= NUMPY_BAR


@pytest.mark.parametrize('routing', cases.ROUTINGS)
@pytest.mark.parametrize('op', cases.OPS)
def test_array_and_scalar_forms_agree_at_the_special_values(op, routing):
  """expr.evaluate (arrays) against NumPy on scalars, point by point: NaN with
  NaN, zeros and infinities with their signs, the exact opcodes bit for bit,
  the inexact ones within the bar of the exact value where there is one."""
  a, b, want, resid = cases.special_cases(op)
  scalar = cases.numpy_scalar(op, a, b)
  # NumPy's scalar form passes against the exact values: the two expectations
  # (NumPy's scalar result, the table) are one
  ok = cases.passes(op, scalar, want, resid, NUMPY_BAR)
  assert ok.all(), (op, a[~ok], None if b is None else b[~ok], scalar[~ok], want[~ok])
  got = cases.run(_evaluate, op, routing, a, b)
  ok = cases.passes(op, got, cases.through(routing, want), resid, NUMPY_BAR)
  assert ok.all(), (op, routing, a[~ok], None if b is None else b[~ok], got[~ok], want[~ok])
  # and where the value is not measured, array and scalar results are the same
  free = ~np.isfinite(resid) if resid is not None else np.ones(a.size, bool)
  ok = cases.same(got, cases.through(routing, scalar)) | ~free
  assert ok.all(), (op, routing, a[~ok], None if b is None else b[~ok], got[~ok], scalar[~ok])


def test_pow_is_c99_pow_at_the_points_array_power_rewrites():
  """`array ** 0.5` is sqrt in NumPy: -0. and nan.  pow gives +0. and +inf."""
  code = [expr.encode(expr.POW, (expr.VAR, 0), (expr.CONST, 0))]
  got = expr.evaluate(code, [0.5], np.array([[-0.], [-cases.INF], [4.]]))
  assert cases.same(got, np.array([0., cases.INF, 2.])).all(), got
