"""One opcode of the expression interpreter at a time: the one-opcode programs
in every routing the interpreter has, the special-value set, the reference
table tests/golden/expr_ops.npz (tools/gen_expr_ops_golden.py) and the
comparison by class.  Shared by tests/test_expr_ops_host.py (expr.evaluate, the
NumPy definition, measured by the same harness) and tests/test_gpu_expr_ops.py
(the device).

An `evaluate` below is any function (code, consts, depth, points [n, 2], data
or None) -> values [n]: expr.evaluate or engine.eval_expr.
"""
import os

import numpy as np

from probayes_amd import expr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'expr_ops.npz')
INF, NAN = float('inf'), float('nan')
TINY, MAX = 2.2250738585072014e-308, 1.7976931348623157e308

# the special-value set: every unary opcode sees S, every binary one S x S
S = np.array([0., -0., 1., -1., 0.5, -0.5, 2., -2., 3., -3., INF, -INF, NAN, 5e-324, -5e-324,
              1e-320, TINY, MAX, -MAX, 709.782712893384, 709.782712893385,
              -745.13321910194111, -745.2, -1. + 2. ** -53])
# pow: S x these exponents
POW_EXPONENTS = np.array([0., -0., 0.5, -0.5, 1., -1., 2., 3., -3., 1.5, -2., 4., 1. / 3., INF,
                          -INF, NAN, 1e300, 2. ** 53, 2. ** 53 + 2., -(2. ** 52 + 1.)])

EXACT = ('mov', 'add', 'sub', 'mul', 'div', 'neg', 'abs', 'sqrt', 'max', 'min')
INEXACT = ('exp', 'log', 'log1p', 'expm1', 'pow')
OPS = EXACT + INEXACT
OPCODE = {name: i for i, name in enumerate(expr.OP_NAMES)}
assert sorted(OPCODE[op] for op in OPS) == list(range(expr.N_OPS))

# the routings of one word `op a, b` (a unary word reads a alone):
#   var_var    outer word, a = variable 0, b = variable 1
#   var_const  outer word, a = variable 0, b = a constant (unary: a = the constant)
#   acc_slot   outer word after two MOVs, a = the accumulator, b = a slot
#              (unary: a = the slot)
#   loop_outer the single body word of a region over one observation, operands
#              the outer variables
#   loop_col   body word, a = data column 1, b = body temporary 1 (unary: the column)
#   loop_temp  body word, a = body temporary 1, b = data column 1 (unary: the
#              temporary, after a word that replaces the body's accumulator)
SCALAR_ROUTINGS = ('var_var', 'var_const', 'acc_slot')
DATA_ROUTINGS = ('loop_outer', 'loop_col', 'loop_temp')
ROUTINGS = SCALAR_ROUTINGS + DATA_ROUTINGS


def is_binary(op):
  return expr.ARITY[OPCODE[op]] == 2


def fixed_side(op, routing):
  """'a' / 'b': the operand that is one value per program (a constant or a
  column of one observation), or None: both operands vary with the point."""
  if routing == 'var_const':
    return 'b' if is_binary(op) else 'a'
  if routing == 'loop_col':
    return 'a'
  if routing == 'loop_temp':
    return 'b' if is_binary(op) else None
  return None


def program(op, routing, fixed=0.):
  """(code, consts, depth, data or None) of the one-opcode program over d = 2
  variables; the operand that varies with the point is variable 0 (with
  var_var, acc_slot and loop_outer a = variable 0 and b = variable 1)."""
  E, V, C, A, SL, B = expr.encode, expr.VAR, expr.CONST, expr.ACC, expr.SLOT, expr.BODY_BASE
  o, two = OPCODE[op], is_binary(op)
  consts, depth, data = [], 0, None
  if routing == 'var_var':
    code = [E(o, (V, 0), (V, 1))]
  elif routing == 'var_const':
    consts = [fixed]
    code = [E(o, (V, 0), (C, 0))] if two else [E(o, (C, 0))]
  elif routing == 'acc_slot':
    depth = 1
    if two:
      code = [E(expr.MOV, (V, 1), dst=0, store=True), E(expr.MOV, (V, 0)),
              E(o, (A, 0), (SL, 0))]
    else:
      code = [E(expr.MOV, (V, 0), dst=0, store=True), E(expr.MOV, (V, 1)), E(o, (SL, 0))]
  elif routing == 'loop_outer':
    data = np.array([[1.25]])
    code = [E(expr.LOOP, (SL, 1)), E(o, (V, 0), (V, 1)), E(expr.SUM, (A, 0))]
  elif routing == 'loop_col':
    data = np.array([[1.25], [fixed]])
    code = [E(expr.LOOP, (SL, 2)), E(expr.MOV, (V, 0), dst=1, store=True),
            E(o, (V, B + 1), (SL, B + 1)), E(expr.SUM, (A, 0))]
  elif routing == 'loop_temp':
    data = np.array([[1.25], [fixed]])
    if two:
      code = [E(expr.LOOP, (SL, 2)), E(expr.MOV, (V, 0), dst=1, store=True),
              E(o, (SL, B + 1), (V, B + 1)), E(expr.SUM, (A, 0))]
    else:
      code = [E(expr.LOOP, (SL, 3)), E(expr.MOV, (V, 0), dst=1, store=True),
              E(expr.MOV, (V, B + 1)), E(o, (SL, B + 1)), E(expr.SUM, (A, 0))]
  else:
    raise ValueError(routing)
  code, consts = np.array(code, np.int32), np.array(consts, np.float64)
  expr.check_program(code, consts, depth, 2, data)
  return code, consts, depth, data


def _bits(v):
  return np.ascontiguousarray(v, np.float64).view(np.int64)


def run(evaluate, op, routing, a, b=None):
  """The opcode at the operands a [n] (and b [n]) through `routing`: one call
  of `evaluate` per value of the routing's fixed operand."""
  a = np.ascontiguousarray(a, np.float64)
  b = np.full(a.size, 0.25) if b is None else np.ascontiguousarray(b, np.float64)
  side = fixed_side(op, routing)
  if side is None:
    code, consts, depth, data = program(op, routing)
    return np.asarray(evaluate(code, consts, depth, np.stack([a, b], -1), data))
  fixed, free = (a, b) if side == 'a' else (b, a)
  out = np.empty(a.size)
  keys = _bits(fixed)
  for k in np.unique(keys):
    idx = np.flatnonzero(keys == k)
    code, consts, depth, data = program(op, routing, fixed[idx[0]])
    pts = np.stack([free[idx], np.full(idx.size, 0.25)], -1)
    out[idx] = evaluate(code, consts, depth, pts, data)
  return out


# ---------------------------------------------------------------------------
# expectations
# ---------------------------------------------------------------------------
_NUMPY = {'mov': lambda a, b: a, 'add': np.add, 'sub': np.subtract, 'mul': np.multiply,
          'div': np.true_divide, 'neg': lambda a, b: np.negative(a),
          'abs': lambda a, b: np.absolute(a), 'sqrt': lambda a, b: np.sqrt(a),
          'exp': lambda a, b: np.exp(a), 'log': lambda a, b: np.log(a),
          'log1p': lambda a, b: np.log1p(a), 'expm1': lambda a, b: np.expm1(a),
          'max': np.maximum, 'min': np.minimum, 'pow': np.power}


def numpy_array(op, a, b=None):
  """NumPy's array result: for the exact opcodes the correctly rounded one."""
  with np.errstate(all='ignore'):
    return np.asarray(_NUMPY[op](np.asarray(a, np.float64),
                                 None if b is None else np.asarray(b, np.float64)), np.float64)


def numpy_scalar(op, a, b=None):
  """NumPy's result on float64 scalars, point by point: what the reference
  computes when it calls a density with scalars (`x ** c` is C's pow)."""
  a = np.asarray(a, np.float64)
  b = np.zeros(a.size) if b is None else np.asarray(b, np.float64)
  out = np.empty(a.size)
  with np.errstate(all='ignore'):
    for i in range(a.size):
      if op == 'pow':
        out[i] = np.float64(a[i]) ** float(b[i])
      else:
        out[i] = _NUMPY[op](np.float64(a[i]), np.float64(b[i]))
  return out


def through(routing, want):
  """The expectation as the routing delivers it: a region of one observation
  returns 0. + t, which turns -0. into +0."""
  return 0. + np.asarray(want, np.float64) if routing in DATA_ROUTINGS else want


def ulp(w):
  """spacing(|w|); at the largest finite value, where it overflows, the
  spacing below it (as the table's generator)."""
  w = np.abs(np.asarray(w, np.float64))
  with np.errstate(all='ignore'):
    return np.where(w == MAX, 2. ** 971, np.spacing(w))


def ulp_error(got, want, resid):
  """|got - exact| in units of the last place of want, exact = want + resid *
  ulp(want).  inf / nan where got is not finite."""
  with np.errstate(all='ignore'):
    return np.abs((np.asarray(got, np.float64) - want) / ulp(want) - resid)


def same(got, want):
  """Both NaN (sign and payload not compared), or the same bits (so zeros and
  infinities with the same sign)."""
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  return (np.isnan(got) & np.isnan(want)) | (_bits(got) == _bits(want))


def passes(op, got, want, resid=None, bar=None):
  """Per point: an exact opcode is `same`; an inexact one is within `bar` ulp
  of the exact value where the table has its residual (resid finite, want
  finite and not 0), `same` everywhere else."""
  ok = same(got, want)
  if op in EXACT or resid is None:
    return ok
  measured = np.isfinite(resid) & np.isfinite(want) & (want != 0.)
  return np.where(measured, ulp_error(got, want, np.where(measured, resid, 0.)) <= bar, ok)


# ---------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------
_TABLE = {}


def table():
  if not _TABLE:
    with np.load(GOLDEN) as z:
      _TABLE.update({k: z[k] for k in z.files})
  return _TABLE


def classes(kind):
  """The class names under `kind` (an inexact opcode, 'exact' or 'sqrt')."""
  pre = kind + '.'
  return [k[len(pre):-2] for k in table() if k.startswith(pre) and k.endswith('.a')]


def table_cases(op, routing=None):
  """[(class, a, b or None, want, resid or None)] of the table for `op`.  An
  exact opcode's want is NumPy's array result.  With a routing whose fixed
  operand is one value per program, the classes are cut down to few programs:
  an exact opcode takes the class's first value of that operand at every point,
  an inexact one (whose wants belong to the table's own operands) keeps the
  class's first two points unless the operand is one value already."""
  t = table()
  side = fixed_side(op, routing) if routing else None
  out = []
  if op in INEXACT:
    for c in classes(op):
      if c == 'special':
        continue
      key = '{}.{}.'.format(op, c)
      a, b = t[key + 'a'], t.get(key + 'b')
      want, resid = t[key + 'want'], t[key + 'resid']
      fixed = {'a': a, 'b': b, None: None}[side]
      if fixed is not None and np.unique(_bits(fixed)).size > 1:
        a, want, resid = a[:2], want[:2], resid[:2]
        b = None if b is None else b[:2]
      out.append((c, a, b, want, resid))
    return out
  kinds = ['exact'] + (['sqrt'] if op == 'sqrt' else [])
  for kind in kinds:
    for c in classes(kind):
      key = '{}.{}.'.format(kind, c)
      a = t[key + 'a']
      b = t[key + 'b'] if is_binary(op) else None
      if side == 'a':
        a = np.full(a.size, a[0]) if is_binary(op) else a[:2]
      elif side == 'b':
        b = np.full(b.size, b[0])
      out.append((kind + '.' + c, a, b, numpy_array(op, a, b), None))
  return out


def special_cases(op):
  """(a, b or None, want, resid): S (S x S, S x POW_EXPONENTS for pow) with
  NumPy's scalar result, or for an inexact opcode where the value is a finite
  real number the table's exact one and its residual (resid NaN elsewhere)."""
  if is_binary(op):
    a, b = (v.reshape(-1) for v in np.meshgrid(S, POW_EXPONENTS if op == 'pow' else S,
                                               indexing='ij'))
  else:
    a, b = S.copy(), None
  want = numpy_scalar(op, a, b)
  if op in EXACT:
    return a, b, want, None
  t = table()
  key = '{}.special.'.format(op)
  zeros = np.zeros(t[key + 'a'].size)
  known = {k: i for i, k in enumerate(zip(_bits(t[key + 'a']),
                                          _bits(t.get(key + 'b', zeros))))}
  resid = np.full(a.size, NAN)
  for i, k in enumerate(zip(_bits(a), _bits(np.zeros(a.size) if b is None else b))):
    if k in known:
      want[i], resid[i] = t[key + 'want'][known[k]], t[key + 'resid'][known[k]]
  return a, b, want, resid
