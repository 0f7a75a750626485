"""Writes tests/golden/expr_ops.npz: the reference table of the expression
interpreter's opcodes (tests/expr_ops_cases.py reads it).

For each inexact opcode (exp log log1p expm1 pow) and each class of points:
  <op>.<class>.a       the operand (for pow the base)
  <op>.<class>.b       pow only: the exponent
  <op>.<class>.want    the exact value (mpmath, 200 bits) rounded to nearest fp64
  <op>.<class>.resid   (exact - want) / spacing(|want|), |resid| <= 0.5
so that a candidate g is measured without mpmath:
  ulp_err = |(g - want) / spacing(|want|) - resid|.
For the exact opcodes (add sub mul div neg abs sqrt max min mov) only points:
  exact.<class>.a, exact.<class>.b (operand pairs), sqrt.<class>.a;
their expectation is NumPy's correctly rounded IEEE result.

  python tools/gen_expr_ops_golden.py        # needs mpmath

The points are seeded (RandomState); generate() is deterministic, and
tests/test_expr_ops_host.py checks that it reproduces the committed file.
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, 'tests', 'golden', 'expr_ops.npz')

PREC = 200
N_CLASS = 512          # points per class of a unary inexact opcode
N_POW = 128            # points per (exponent, base range) class of pow
N_PAIR = 300           # pairs per class of the exact opcodes
TINY, MAX = 2.2250738585072014e-308, 1.7976931348623157e308
POW_EXPONENTS = (3., -1., 0.5, 1.5, -2.5, 7., -3., 1. / 3., 10., 0.1, 2.5, 33.)
EXP_THRESHOLDS = (709.782712893384, -745.1332191019411, -708.3964185322641)
# the special-value set of tests/expr_ops_cases.py and the exponents it is
# crossed with for pow: where the value is a real number, the table holds it
INF, NAN = float('inf'), float('nan')
SPECIAL = (0., -0., 1., -1., 0.5, -0.5, 2., -2., 3., -3., INF, -INF, NAN, 5e-324, -5e-324,
           1e-320, TINY, MAX, -MAX, 709.782712893384, 709.782712893385,
           -745.13321910194111, -745.2, -1. + 2. ** -53)
SPECIAL_EXPONENTS = (0., -0., 0.5, -0.5, 1., -1., 2., 3., -3., 1.5, -2., 4., 1. / 3., INF,
                     -INF, NAN, 1e300, 2. ** 53, 2. ** 53 + 2., -(2. ** 52 + 1.))


def _logu(rs, lo, hi, n):
  """n values spread evenly over the binades of [lo, hi]: a uniform exponent,
  a uniform significand, values outside the range drawn again.  Exact
  operations only, so that every machine's libm makes the same points."""
  elo, ehi = math.frexp(lo)[1] - 1, math.frexp(hi)[1] - 1
  out, have = [], 0
  while have < n:
    x = np.ldexp(rs.uniform(1., 2., n), rs.randint(elo, ehi + 1, n))
    x = x[(x >= lo) & (x <= hi)]
    out.append(x)
    have += x.size
  return np.concatenate(out)[:n]


def _signed(rs, v):
  return v * np.where(rs.randint(0, 2, v.size) == 1, 1., -1.)


def _around(v, k):
  """v and its k neighbours on either side"""
  out = [np.float64(v)]
  lo = hi = np.float64(v)
  for _ in range(k):
    lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
    out += [lo, hi]
  return out


def points():
  """{(op, class): (a, b or None)}, in a fixed order"""
  rs = np.random.RandomState(20240917)
  n = N_CLASS
  out = {}
  out['exp', 'wide'] = rs.uniform(-745.2, 709.78, n), None
  out['exp', 'unit'] = rs.uniform(-2., 2., n), None
  out['exp', 'tiny'] = _signed(rs, _logu(rs, 1e-300, 1e-3, n)), None
  out['exp', 'thresholds'] = np.array(sum((_around(t, 8) for t in EXP_THRESHOLDS), [])), None
  out['log', 'subnormal'] = np.minimum(
      np.maximum(np.round(_logu(rs, 1., 2. ** 52, n)), 1.) * 5e-324,
      np.nextafter(TINY, 0.)), None
  out['log', 'normal'] = _logu(rs, TINY, MAX, n), None
  out['log', 'near_one'] = 1. + _signed(rs, _logu(rs, 1e-16, 0.5, n)), None
  out['log1p', 'tiny'] = _signed(rs, _logu(rs, 1e-300, 1e-3, n)), None
  out['log1p', 'unit'] = 2. - rs.uniform(0., 3., n), None            # (-1, 2]
  out['log1p', 'near_minus_one'] = -1. + _logu(rs, 1e-16, 1e-3, n), None
  out['log1p', 'large'] = _logu(rs, 2., MAX, n), None
  out['expm1', 'tiny'] = _signed(rs, _logu(rs, 1e-300, 1e-3, n)), None
  out['expm1', 'wide'] = rs.uniform(-40., 709.78, n), None
  out['expm1', 'unit'] = rs.uniform(-2., 2., n), None
  for e in POW_EXPONENTS:
    name = '{:.4g}'.format(e)
    for cls, lo, hi in (('wide', 1e-30, 1e30), ('near_one', 0.5, 2.)):
      a = _logu(rs, lo, hi, N_POW)
      out['pow', '{}.{}'.format(name, cls)] = a, np.full(N_POW, e)
      if e == np.floor(e):
        out['pow', '{}.{}.neg'.format(name, cls)] = -a, np.full(N_POW, e)
  # results beyond both ends of the range: 1e30 ** 33 overflows above, so the
  # classes above hold some already; these straddle the two limits
  a = _logu(rs, 1e9, 1e10, N_POW)
  out['pow', '33.overflow'] = a, np.full(N_POW, 33.)                 # 1e297 .. 1e330
  out['pow', '33.underflow'] = 1. / a, np.full(N_POW, 33.)           # 1e-330 .. 1e-297
  out['pow', '-2.5.underflow'] = _logu(rs, 1e120, 1e131, N_POW), np.full(N_POW, -2.5)
  out['pow', '1.5.overflow'] = _logu(rs, 1e200, 1e207, N_POW), np.full(N_POW, 1.5)
  sp = np.array(SPECIAL)
  real = np.isfinite(sp) & (sp != 0.)
  out['exp', 'special'] = sp[real], None
  out['expm1', 'special'] = sp[real], None
  out['log', 'special'] = sp[real & (sp > 0.)], None
  out['log1p', 'special'] = sp[real & (sp > -1.)], None
  a, b = (v.reshape(-1) for v in np.meshgrid(sp, np.array(SPECIAL_EXPONENTS), indexing='ij'))
  with np.errstate(invalid='ignore'):
    real = np.isfinite(a) & (a != 0.) & np.isfinite(b) & (b != 0.) & \
        ((a > 0.) | (b == np.floor(b)))
  out['pow', 'special'] = a[real], b[real]
  return out


def exact_points():
  """{(kind, class): (a, b or None)}: operand pairs of the exact binary opcodes
  (their first operand also goes to neg, abs and mov) and operands of sqrt"""
  rs = np.random.RandomState(20240918)
  n = N_PAIR
  out = {}
  for cls, lo, hi in (('tiny', 1e-300, 1e-3), ('wide', 1e-30, 1e30), ('near_one', 0.5, 2.),
                      ('normal', TINY, MAX)):
    out['exact', cls] = (_signed(rs, _logu(rs, lo, hi, n)), _signed(rs, _logu(rs, lo, hi, n)))
  sub = lambda: np.maximum(np.round(_logu(rs, 1., 2. ** 52, n)), 1.) * 5e-324
  out['exact', 'subnormal'] = _signed(rs, sub()), _signed(rs, sub())
  # a - b (or a + b) is a subnormal or 0
  a = _signed(rs, _logu(rs, TINY, 2. ** 52 * TINY, n))
  k = np.round(_logu(rs, 1., 2. ** 40, n)) * np.where(rs.randint(0, 4, n) == 0, 0., 1.)
  s = _signed(rs, np.ones(n))
  out['exact', 'cancel'] = a, s * (a + _signed(rs, k) * 5e-324)
  # a * b and a / b in the subnormal range, or beyond the largest finite value
  a, b = _logu(rs, 1e-162, 1e-147, n), _logu(rs, 1e-162, 1e-147, n)
  out['exact', 'product_small'] = _signed(rs, a), _signed(rs, b)
  out['exact', 'quotient_small'] = _signed(rs, a), _signed(rs, 1. / b)
  a, b = _logu(rs, 1e147, 1e162, n), _logu(rs, 1e147, 1e162, n)
  out['exact', 'product_large'] = _signed(rs, a), _signed(rs, b)
  out['exact', 'quotient_large'] = _signed(rs, a), _signed(rs, 1. / b)
  out['sqrt', 'subnormal'] = sub(), None
  out['sqrt', 'normal'] = _logu(rs, TINY, MAX, n), None
  return out


def ulp(w):
  """spacing(|w|), the last place of w; at the largest finite value, where
  NumPy's spacing overflows, the spacing below it."""
  w = np.abs(np.asarray(w, np.float64))
  with np.errstate(all='ignore'):
    return np.where(w == MAX, 2. ** 971, np.spacing(w))


def _round(y):
  """An mpf -> (the nearest fp64, ties to even; the residual in units of
  spacing(|want|)).  In integers: no second rounding in the subnormal range."""
  import mpmath
  sign, man, ex, bc = y._mpf_
  if man == 0:
    if not mpmath.isfinite(y):
      return float(y), 0.
    return (-0. if sign else 0.), 0.
  e = bc + ex - 1                      # 2**e <= |y| < 2**(e + 1)
  if e > 1024:
    return (-np.inf if sign else np.inf), 0.
  if e < -1080:
    return (-0. if sign else 0.), 0.
  q = max(e - 52, -1074)               # the last place
  if ex >= q:
    k = man << (ex - q)
  else:
    sh = q - ex
    k, rem, half = man >> sh, man & ((1 << sh) - 1), 1 << (sh - 1)
    if rem > half or (rem == half and k & 1):
      k += 1
  if q > 971 or (q == 971 and k == 1 << 53):     # past the largest finite value
    return (-np.inf if sign else np.inf), 0.
  if k == 1 << 53:
    k, q = 1 << 52, q + 1
  want = np.float64(np.ldexp(np.float64(k), q))     # k < 2**53: exact
  mag = mpmath.mpf(float(want))
  resid = float((abs(y) - mag) / mpmath.mpf(float(ulp(want))))
  if sign:
    want, resid = -want, -resid
  return want, resid


def exact_value(op, a, b=None):
  """The opcode at fp64 operands as an mpf of PREC bits."""
  import mpmath
  x = mpmath.mpf(float(a))
  if op == 'exp':
    return mpmath.exp(x)
  if op == 'log':
    return mpmath.log(x)
  if op == 'log1p':
    # log(1 + x) with 1 + x formed exactly (x has 53 bits, above 2**-1074)
    if mpmath.mag(x) < -2 * PREC:
      return x - x * x / 2
    with mpmath.workprec(1200):
      return +mpmath.log(1 + x)
  if op == 'expm1':
    if mpmath.mag(x) < -2 * PREC:
      return x + x * x / 2
    with mpmath.workprec(1200):
      return +(mpmath.exp(x) - 1)
  if op == 'pow':
    return mpmath.power(x, mpmath.mpf(float(b)))
  raise ValueError(op)


def generate():
  """{key: array} of the whole fixture."""
  import mpmath
  out = {}
  with mpmath.workprec(PREC):
    for (op, cls), (a, b) in points().items():
      a = np.asarray(a, np.float64)
      want, resid = np.empty(a.size), np.empty(a.size)
      for i in range(a.size):
        y = exact_value(op, a[i], None if b is None else b[i])
        want[i], resid[i] = _round(+y)
      assert np.all(np.abs(resid) <= 0.5), (op, cls)
      key = '{}.{}.'.format(op, cls)
      out[key + 'a'] = a
      if b is not None:
        out[key + 'b'] = np.asarray(b, np.float64)
      out[key + 'want'], out[key + 'resid'] = want, resid
  for (kind, cls), (a, b) in exact_points().items():
    key = '{}.{}.'.format(kind, cls)
    out[key + 'a'] = np.asarray(a, np.float64)
    if b is not None:
      out[key + 'b'] = np.asarray(b, np.float64)
  return out


def main():
  arrays = generate()
  np.savez_compressed(PATH, **arrays)
  print('{}: {} arrays, {} values, {} bytes'.format(
      os.path.relpath(PATH, ROOT), len(arrays), sum(v.size for v in arrays.values()),
      os.path.getsize(PATH)))
  return 0


if __name__ == '__main__':
  sys.exit(main())
