"""Expression target: a scalar density as a small program (data, not code).

A density callable that matches none of the closed forms is traced once with
symbolic scalars (trace_expr) and compiled to a straight-line program that the
HIP kernels interpret (pbh_kernels_impl.h expr_density): the same program for
every chain, so its control flow is wave-uniform.

The machine
  One instruction per code word, one result per instruction.  The result of
  the previous instruction is the accumulator; an instruction whose result is
  needed later than by its successor also stores it to one of `depth` slots.
  An operand is a slot, a variable, a constant or the accumulator.

  word = op | dst << 6 | store << 10 | akind << 11 | aidx << 13
            | bkind << 21 | bidx << 23
  kinds: 0 slot, 1 variable, 2 constant, 3 accumulator.

  The value of the program is the accumulator after the last instruction.
  Limits: MAX_CODE words, MAX_CONSTS constants, MAX_SLOTS slots, MAX_DIM
  variables.  A slot is read only after it was written, the accumulator only
  after the first instruction (pbh_set_model checks every program).

evaluate() below is the written definition of each opcode: a plain NumPy
interpreter, vectorised over chains, whose loops are the ones the callable
itself runs when it is called on arrays.
"""
import numbers

import numpy as np
import scipy.stats

MAX_CODE, MAX_CONSTS, MAX_SLOTS, MAX_DIM = 256, 128, 16, 16

(MOV, ADD, SUB, MUL, DIV, NEG, ABS, SQRT, EXP, LOG, LOG1P, EXPM1, MAX, MIN,
 POW) = range(15)
N_OPS = 15
OP_NAMES = ('mov', 'add', 'sub', 'mul', 'div', 'neg', 'abs', 'sqrt', 'exp',
            'log', 'log1p', 'expm1', 'max', 'min', 'pow')
ARITY = (1, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2)
SLOT, VAR, CONST, ACC = range(4)


def _not_lowerable(msg):
  from probayes_amd.lower import NotLowerable
  return NotLowerable(msg)


def encode(op, a, b=(SLOT, 0), dst=0, store=False):
  """One code word; a, b = (kind, index)."""
  return (op | dst << 6 | int(bool(store)) << 10 | a[0] << 11 | a[1] << 13 |
          b[0] << 21 | b[1] << 23)


def decode(w):
  """(op, dst, store, (akind, aidx), (bkind, bidx)) of one code word."""
  w = int(w)
  return (w & 63, (w >> 6) & 15, (w >> 10) & 1,
          ((w >> 11) & 3, (w >> 13) & 255), ((w >> 21) & 3, (w >> 23) & 255))


# ---------------------------------------------------------------------------
# the NumPy interpreter
# ---------------------------------------------------------------------------
_UNARY = {NEG: np.negative, ABS: np.absolute, SQRT: np.sqrt, EXP: np.exp,
          LOG: np.log, LOG1P: np.log1p, EXPM1: np.expm1}
_BINARY = {ADD: np.add, SUB: np.subtract, MUL: np.multiply,
           DIV: np.true_divide, MAX: np.maximum, MIN: np.minimum}


def evaluate(code, consts, x):
  """The program at the points x [n, d] (or [d]) -> values [n] (or a scalar).
  IEEE float64 throughout; POW is NumPy's `a ** c`."""
  x = np.asarray(x, np.float64)
  single = x.ndim == 1
  x = np.ascontiguousarray(np.atleast_2d(x).T)   # [d, n]: contiguous columns
  n = x.shape[1]
  consts = np.asarray(consts, np.float64)
  slots = {}
  acc = None

  def fetch(o):
    kind, i = o
    if kind == SLOT:
      return slots[i]
    if kind == VAR:
      return x[i]
    if kind == CONST:
      return consts[i]          # a float64 scalar, as in the callable
    return acc

  with np.errstate(all='ignore'):
    for w in np.asarray(code).reshape(-1):
      op, dst, store, a, b = decode(w)
      va = fetch(a)
      if op == MOV:
        r = va
      elif op in _UNARY:
        r = _UNARY[op](va)
      elif op == POW:
        vb = fetch(b)
        r = va ** (float(vb) if np.ndim(vb) == 0 else vb)
      else:
        r = _BINARY[op](va, fetch(b))
      acc = np.broadcast_to(np.asarray(r, np.float64), (n,))
      if store:
        slots[dst] = acc
  out = np.array(acc)
  return out[0] if single else out


# ---------------------------------------------------------------------------
# tracing
# ---------------------------------------------------------------------------
def _const(v):
  """A Python / NumPy real scalar as float64, else None."""
  if isinstance(v, (bool, np.bool_)):
    return None
  if isinstance(v, numbers.Real):
    return np.float64(v)
  if isinstance(v, np.ndarray) and v.ndim == 0 and v.dtype.kind in 'fiu':
    return np.float64(v)
  return None


def _operand(v, what):
  if isinstance(v, Val):
    return v
  c = _const(v)
  if c is None:
    if isinstance(v, (np.ndarray, list, tuple)):
      raise _not_lowerable('array-valued constant in a scalar density ({})'
                           .format(what))
    raise _not_lowerable('{} operand of type {} in a density'
                         .format(what, type(v).__name__))
  return c


def _mk(op, a, b=None):
  return Val(op, _operand(a, OP_NAMES[op]),
             None if b is None else _operand(b, OP_NAMES[op]))


def _power(base, ex):
  if isinstance(ex, Val):
    raise _not_lowerable('** with a symbolic exponent in a density')
  if not isinstance(base, Val):
    raise _not_lowerable('** with a constant base in a density')
  c = _operand(ex, 'pow')
  if c == 2.0:
    return _mk(MUL, base, base)
  return _mk(POW, base, c)


class Val:
  """A symbolic float64 scalar: arithmetic and the listed NumPy ufuncs on it
  record nodes of a DAG (each Python object is evaluated once)."""
  __array_priority__ = 1000
  __slots__ = ('op', 'a', 'b', 'var')

  def __init__(self, op, a=None, b=None, var=None):
    self.op, self.a, self.b, self.var = op, a, b, var

  _UFUNCS = {np.add: ADD, np.subtract: SUB, np.multiply: MUL,
             np.true_divide: DIV, np.negative: NEG, np.absolute: ABS,
             np.sqrt: SQRT, np.exp: EXP, np.log: LOG, np.log1p: LOG1P,
             np.expm1: EXPM1, np.maximum: MAX, np.minimum: MIN}

  def __array_ufunc__(self, ufunc, method, *inputs, **kw):
    if method != '__call__':
      raise _not_lowerable('{}.{} (a reduction) in a scalar density'
                           .format(ufunc.__name__, method))
    if kw:
      raise _not_lowerable('{} with options in a density'.format(ufunc.__name__))
    if ufunc is np.square:
      return _mk(MUL, inputs[0], inputs[0])
    if ufunc is np.power:
      return _power(*inputs)
    if ufunc not in self._UFUNCS:
      raise _not_lowerable('{} in a density (supported: + - * / ** abs exp log '
                           'sqrt log1p expm1 square maximum minimum)'
                           .format(ufunc.__name__))
    return _mk(self._UFUNCS[ufunc], *inputs)

  def __array_function__(self, func, types, args, kwargs):
    raise _not_lowerable('np.{} in a scalar density'.format(func.__name__))

  def __bool__(self):
    raise _not_lowerable('truth value of a symbolic variable (a data-dependent '
                         'branch) in a density')

  def _compare(self, o):
    raise _not_lowerable('comparison of a symbolic variable in a density')

  __lt__ = __le__ = __gt__ = __ge__ = _compare
  __hash__ = object.__hash__

  def __eq__(self, o):
    return self._compare(o)

  def __ne__(self, o):
    return self._compare(o)

  def __add__(self, o): return _mk(ADD, self, o)
  def __radd__(self, o): return _mk(ADD, o, self)
  def __sub__(self, o): return _mk(SUB, self, o)
  def __rsub__(self, o): return _mk(SUB, o, self)
  def __mul__(self, o): return _mk(MUL, self, o)
  def __rmul__(self, o): return _mk(MUL, o, self)
  def __truediv__(self, o): return _mk(DIV, self, o)
  def __rtruediv__(self, o): return _mk(DIV, o, self)
  def __neg__(self): return _mk(NEG, self)
  def __pos__(self): return self
  def __abs__(self): return _mk(ABS, self)
  def __pow__(self, o): return _power(self, o)
  def __rpow__(self, o): return _power(o, self)

  def _unsupported(self, *a):
    raise _not_lowerable('operator without a kernel form in a density')

  __floordiv__ = __rfloordiv__ = __mod__ = __rmod__ = __matmul__ = _unsupported
  __float__ = __int__ = __index__ = __iter__ = __len__ = _unsupported
  __getitem__ = _unsupported


# scipy's own constants and operation order (_continuous_distns.py):
#   _norm_logpdf(y) = -y**2 / 2.0 - _norm_pdf_logC,  logpdf = that - log(scale)
#   _norm_pdf(y) = exp(-y**2 / 2.0) / _norm_pdf_C,   pdf = that / scale
# with y = (x - loc) / scale; pbh_kernels_impl.h norm_logpdf / norm_pdf restate
# the same order.
_NORM_PDF_C = np.sqrt(2 * np.pi)
_NORM_PDF_LOGC = np.log(_NORM_PDF_C)


def _loc_scale(args, kwds):
  loc = kwds.get('loc', args[0] if len(args) > 0 else 0.)
  scale = kwds.get('scale', args[1] if len(args) > 1 else 1.)
  return loc, scale


def _split(args, kwds, name):
  kwds = dict(kwds)
  x = args[0] if args else kwds.pop('x')
  loc, scale = _loc_scale(args[1:], kwds)
  if set(kwds) - {'loc', 'scale'}:
    raise _not_lowerable('norm.{} with options in a density'.format(name))
  vals = [_operand(v, 'norm.' + name) for v in (x, loc, scale)]
  return vals, any(isinstance(v, Val) for v in vals)


def _traced_logpdf(real):
  def logpdf(*args, **kwds):
    (x, loc, scale), sym = _split(args, kwds, 'logpdf')
    if not sym:
      return real(*args, **kwds)
    y = (x - loc) / scale
    return -y ** 2 / 2.0 - _NORM_PDF_LOGC - np.log(scale)
  return logpdf


def _traced_pdf(real):
  def pdf(*args, **kwds):
    (x, loc, scale), sym = _split(args, kwds, 'pdf')
    if not sym:
      return real(*args, **kwds)
    y = (x - loc) / scale
    return np.exp(-y ** 2 / 2.0) / _NORM_PDF_C / scale
  return pdf


def _traced_updf(real):
  def updf(*args, **kwds):
    if any(isinstance(v, Val) for v in list(args) + list(kwds.values())):
      raise _not_lowerable('uniform.pdf inside an expression (a support test '
                           'is a data-dependent branch)')
    return real(*args, **kwds)
  return updf


def trace_expr(fn, keys):
  """A scalar density callable over the variables `keys` -> {'kind': 'expr',
  'code': int32[], 'consts': float64[], 'depth': int}, or NotLowerable."""
  from probayes_amd.lower import NotLowerable, _patched
  d = len(keys)
  if d > MAX_DIM:
    raise NotLowerable('an expression density takes at most {} variables, '
                       'got {}'.format(MAX_DIM, d))
  kw = {k: Val(None, var=i) for i, k in enumerate(keys)}
  norm, unif = scipy.stats.norm, scipy.stats.uniform
  with _patched(norm, logpdf=_traced_logpdf(norm.logpdf),
                pdf=_traced_pdf(norm.pdf)), \
       _patched(unif, pdf=_traced_updf(unif.pdf)):
    try:
      out = fn(**kw)
    except NotLowerable:
      raise
    except Exception as e:
      raise NotLowerable('density callable not traceable: {}: {}'
                         .format(type(e).__name__, e))
  if not isinstance(out, Val):
    c = _const(out)
    if c is None:
      raise NotLowerable('density returned {}, not a scalar'
                         .format(type(out).__name__))
    out = c
  return compile_dag(out, d)


# ---------------------------------------------------------------------------
# DAG -> program
# ---------------------------------------------------------------------------
def compile_dag(root, d):
  """Linearises the DAG under `root` in dependency order (each node once),
  keeps a result in the accumulator when only the next instruction reads it,
  and allocates slots by last use."""
  from probayes_amd.lower import NotLowerable
  consts, cindex = [], {}

  def const(c):
    key = np.float64(c).tobytes()
    if key not in cindex:
      cindex[key] = len(consts)
      consts.append(np.float64(c))
    return (CONST, cindex[key])

  # post-order without recursion: operands before users, first use first
  order, index = [], {}
  if isinstance(root, Val) and root.var is None:
    stack = [(root, False)]
    while stack:
      node, done = stack.pop()
      if id(node) in index:
        continue
      if done:
        index[id(node)] = len(order)
        order.append(node)
        continue
      stack.append((node, True))
      for o in (node.b, node.a):
        if isinstance(o, Val) and o.var is None and id(o) not in index:
          stack.append((o, False))
  if len(order) > MAX_CODE:
    raise NotLowerable('expression of {} operations exceeds {} code words'
                       .format(len(order), MAX_CODE))
  users = [[] for _ in order]
  for i, node in enumerate(order):
    for o in (node.a, node.b):
      if isinstance(o, Val) and o.var is None:
        users[index[id(o)]].append(i)
  code, slot_of, free, depth = [], {}, [], 0
  if not order:   # a bare variable or a constant
    src = (VAR, root.var) if isinstance(root, Val) else const(root)
    code.append(encode(MOV, src))
  for i, node in enumerate(order):
    ops = []
    for o in (node.a, node.b):
      if o is None:
        ops.append((SLOT, 0))
      elif not isinstance(o, Val):
        ops.append(const(o))
      elif o.var is not None:
        ops.append((VAR, o.var))
      elif index[id(o)] == i - 1:
        ops.append((ACC, 0))
      else:
        ops.append((SLOT, slot_of[index[id(o)]]))
    # slots whose last reader is this instruction are free for its result
    for o in {index[id(o)] for o in (node.a, node.b)
              if isinstance(o, Val) and o.var is None}:
      if o in slot_of and max(users[o]) == i:
        free.append(slot_of.pop(o))
    store = any(u != i + 1 for u in users[i])
    dst = 0
    if store:
      if free:
        dst = min(free)
        free.remove(dst)
      else:
        dst = depth
        depth += 1
        if depth > MAX_SLOTS:
          raise NotLowerable('expression keeps more than {} intermediate '
                             'values alive'.format(MAX_SLOTS))
      slot_of[i] = dst
    code.append(encode(node.op, ops[0], ops[1], dst, store))
  if len(consts) > MAX_CONSTS:
    raise NotLowerable('expression with {} constants exceeds {}'
                       .format(len(consts), MAX_CONSTS))
  return {'kind': 'expr', 'code': np.asarray(code, np.int32),
          'consts': np.asarray(consts, np.float64), 'depth': int(depth)}


def check_program(code, consts, depth, d):
  """The checks pbh_set_model makes (ValueError with the cause)."""
  code = np.asarray(code).reshape(-1)
  n_consts = np.asarray(consts).size
  if not 1 <= code.size <= MAX_CODE:
    raise ValueError('expr: {} code words outside 1..{}'.format(code.size, MAX_CODE))
  if n_consts > MAX_CONSTS or not 0 <= depth <= MAX_SLOTS or not 1 <= d <= MAX_DIM:
    raise ValueError('expr: constants / depth / dim over the limits')
  written = set()
  for pc, w in enumerate(code):
    if w < 0:
      raise ValueError('expr: bad code word at {}'.format(pc))
    op, dst, store, a, b = decode(w)
    if op >= N_OPS:
      raise ValueError('expr: bad opcode {} at {}'.format(op, pc))
    for kind, i in (a, b)[:ARITY[op]]:
      ok = (kind == SLOT and i in written) or (kind == VAR and i < d) or \
           (kind == CONST and i < n_consts) or (kind == ACC and pc > 0)
      if not ok:
        raise ValueError('expr: bad operand ({}, {}) at {}'.format(kind, i, pc))
    if store:
      if dst >= depth:
        raise ValueError('expr: slot {} >= depth {} at {}'.format(dst, depth, pc))
      written.add(dst)
