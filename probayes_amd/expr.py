"""Expression target: a scalar density as a small program (data, not code).

A density callable that matches none of the closed forms is traced once with
symbolic scalars (trace_expr; the 1-D arrays it holds become data columns) and
compiled to a straight-line program that the HIP kernels interpret
(pbh_kernels_impl.h expr_density, pbh_expr_data.hip expr_data_density): the
same program for every chain, so its control flow is wave-uniform.

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

Loop regions (likelihoods summed over observed data)
  A density may hold 1-D data arrays, all of one length n.  A value that
  depends on one is a vector; a program reduces it to a scalar in a non-nested
  loop region:

    LOOP | body_len << 13      opens the region
    body_len body words        a straight-line program run once per observation
                               j = 0..n-1, with an accumulator of its own
    SUM  | dst << 6 | store << 10 | ACC << 11
                               closes it: the accumulator becomes the sum over
                               j of the body's last value (and goes to slot dst)

  Inside a body a VAR index >= 16 is data column idx - 16 at observation j, a
  SLOT index >= 16 is body temporary idx - 16 (MAX_TEMPS of them), a SLOT
  index < 16 reads an outer slot, and the store field names a body temporary.
  The sum is NumPy's 1-D pairwise sum (sequential below 8 terms, eight
  accumulators per block up to 128, halving above that).  Limits: MAX_COLS
  columns, 1 <= n <= MAX_OBS.  LOOP and SUM lie outside range(N_OPS): a
  program without data holds neither.

Pointwise programs (statistics per observation over the trace)
  trace_pointwise compiles a callable that returns the unreduced vector of
  per-observation terms as the program of its sum: scalar words, one LOOP, the
  body, and SUM as the last word.  The body's last value is the term;
  evaluate_pointwise returns the terms [points, n], and the engine reduces
  them over the draws of its trace (Engine.trace_pointwise) without forming
  the sum.

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
# loop regions: outside range(N_OPS), so that a program without data arrays
# keeps its words
LOOP, SUM = 32, 33
MAX_COLS, MAX_TEMPS, MAX_OBS = 8, 4, 65536
BODY_BASE = 16   # a body's VAR / SLOT index from here on: data column / temporary


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


def _apply(op, va, fetch_b):
  if op == MOV:
    return va
  if op in _UNARY:
    return _UNARY[op](va)
  if op == POW:
    vb = fetch_b()
    if np.ndim(va) == 0 and np.ndim(vb) == 0:
      return va ** float(vb)     # scalars: C's pow, as the callable's own `**`
    # arrays: the pow ufunc, not `array ** scalar`, whose fast paths for the
    # exponents 0.5, -1, 1 and 2 (sqrt, reciprocal, copy, square) are not pow
    return np.power(va, vb)
  return _BINARY[op](va, fetch_b())


def _run(code, consts, x, data, pointwise):
  """evaluate / evaluate_pointwise at x [d, n] (contiguous columns): the
  accumulator [n] after the last word, or with `pointwise` the terms [n, n_obs]
  of the first region met."""
  n = x.shape[1]
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

  def terms(body):
    """the body's last value at every point and observation -> [n, n_obs],
    C-contiguous"""
    n_obs = data.shape[1]
    temps = {}
    bacc = None

    def bfetch(o):
      kind, i = o
      if kind == SLOT:
        return temps[i - BODY_BASE] if i >= BODY_BASE else slots[i][:, None]
      if kind == VAR:
        return data[i - BODY_BASE][None, :] if i >= BODY_BASE else x[i][:, None]
      if kind == CONST:
        return consts[i]
      return bacc

    for w in body:
      op, dst, store, a, b = decode(w)
      r = _apply(op, bfetch(a), lambda: bfetch(b))
      bacc = np.asarray(r, np.float64)
      if store:
        temps[dst] = bacc
    return np.ascontiguousarray(np.broadcast_to(bacc, (n, n_obs)))

  with np.errstate(all='ignore'):
    pc = 0
    while pc < len(code):
      op, dst, store, a, b = decode(code[pc])
      if op == LOOP:
        length = a[1]
        t = terms(code[pc + 1:pc + 1 + length])
        if pointwise:
          return t
        # the sum over the observations of the body's last value -> [n]
        r = np.add.reduce(t, axis=1)
        pc += length + 1          # at the SUM word, which may store the sum
        op, dst, store, a, b = decode(code[pc])
      else:
        r = _apply(op, fetch(a), lambda: fetch(b))
      acc = np.broadcast_to(np.asarray(r, np.float64), (n,))
      if store:
        slots[dst] = acc
      pc += 1
  if pointwise:
    raise ValueError('expr: a pointwise program needs a loop region')
  return np.array(acc)


def _points(code, consts, x, data):
  x = np.asarray(x, np.float64)
  single = x.ndim == 1
  x = np.ascontiguousarray(np.atleast_2d(x).T)   # [d, n]: contiguous columns
  consts = np.asarray(consts, np.float64)
  if data is not None:
    data = np.ascontiguousarray(np.atleast_2d(np.asarray(data, np.float64)))
  code = [int(w) for w in np.asarray(code).reshape(-1)]
  return code, consts, x, data, single


def evaluate(code, consts, x, data=None):
  """The program at the points x [n, d] (or [d]) -> values [n] (or a scalar).
  IEEE float64 throughout; POW is pow(a, c) (np.power: C99's special values,
  pow(-0., 0.5) = +0. and pow(-inf, 0.5) = +inf, as the device's pow and as
  `a ** c` on scalars; not `array ** c`, which NumPy rewrites to sqrt,
  reciprocal or square for c = 0.5, -1, 2).  data [C, n_obs]: the
  columns the loop regions read.  A region's terms are laid out [points,
  n_obs], C-contiguous, and reduced along the last axis: NumPy's pairwise sum
  of each point's terms (a reduction along axis 0 would add rows in
  sequence)."""
  code, consts, x, data, single = _points(code, consts, x, data)
  out = _run(code, consts, x, data, False)
  return out[0] if single else out


def evaluate_pointwise(code, consts, x, data):
  """The terms of a pointwise program (trace_pointwise) at the points x [n, d]
  (or [d]) -> [n, n_obs] (or [n_obs]): what evaluate() sums in the program's
  region, unreduced -- the same body loop, without the np.add.reduce."""
  code, consts, x, data, single = _points(code, consts, x, data)
  out = _run(code, consts, x, data, True)
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
    if isinstance(v, np.ndarray) and v.dtype.kind in 'fiub':
      if v.ndim != 1:
        raise _not_lowerable('{}-D array in a density ({}): data arrays are 1-D'
                             .format(v.ndim, what))
      if not 1 <= v.size <= MAX_OBS:
        raise _not_lowerable('data array of {} observations outside 1..{} ({})'
                             .format(v.size, MAX_OBS, what))
      return Val(None, col=np.ascontiguousarray(v, np.float64), n=v.size)
    if isinstance(v, (np.ndarray, list, tuple)):
      raise _not_lowerable('array-valued constant in a scalar density ({})'
                           .format(what))
    raise _not_lowerable('{} operand of type {} in a density'
                         .format(what, type(v).__name__))
  return c


def _symbolic(v):
  """Depends on a variable (a data column alone does not)."""
  return isinstance(v, Val) and v.col is None


def _mk(op, a, b=None):
  ops = [_operand(v, OP_NAMES[op]) for v in ((a,) if b is None else (a, b))]
  lens = {v.n for v in ops if isinstance(v, Val) and v.n}
  if len(lens) > 1:
    raise _not_lowerable('data arrays of two lengths ({}) in one density'
                         .format(' and '.join(str(n) for n in sorted(lens))))
  if op == LOG and isinstance(ops[0], Val) and ops[0].op == SUM and ops[0].a.op == EXP:
    # as before this target had sums: a mixture is the gmm form or nothing
    raise _not_lowerable('np.log(np.sum(np.exp(v))): a log-sum-exp without the max '
                         'shift in a density (the shifted form m + log(sum(exp(a - m))) '
                         'of a Gaussian mixture lowers to the gmm target)')
  if not any(_symbolic(v) for v in ops):
    # no variable below: NumPy's own value on the host, a column again
    raw = [v.col if isinstance(v, Val) else v for v in ops]
    with np.errstate(all='ignore'):
      return _operand(_apply(op, raw[0], lambda: raw[1]), OP_NAMES[op])
  return Val(op, ops[0], None if b is None else ops[1], n=lens.pop() if lens else 0)


def _reduce(v, name, args, kwargs):
  """np.sum / np.mean (or the methods) of a vector, without options."""
  if args or kwargs:
    raise _not_lowerable('{} with options (axis=, dtype=, keepdims=, where=, '
                         'out=) in a density'.format(name))
  if not v.n:
    raise _not_lowerable('{} of a scalar symbolic value (a reduction needs a '
                         'data array) in a density'.format(name))
  total = Val(SUM, v)
  # np.mean: the pairwise sum, then a true divide by the count
  return total if name.endswith('sum') else _mk(DIV, total, float(v.n))


def _power(base, ex):
  if isinstance(ex, Val):
    raise _not_lowerable('** with a symbolic exponent in a density')
  if not isinstance(base, Val):
    raise _not_lowerable('** with a constant base in a density')
  c = _operand(ex, 'pow')
  if isinstance(c, Val):
    raise _not_lowerable('** with an array exponent in a density')
  if c == 2.0:
    return _mk(MUL, base, base)
  return _mk(POW, base, c)


class Val:
  """A symbolic float64 scalar: arithmetic and the listed NumPy ufuncs on it
  record nodes of a DAG (each Python object is evaluated once).  n > 0: a
  vector of n observations, either a data column (col) or a value computed
  from one; np.sum / np.mean of a vector is a scalar again (op SUM)."""
  __array_priority__ = 1000
  __slots__ = ('op', 'a', 'b', 'var', 'col', 'n')

  def __init__(self, op, a=None, b=None, var=None, col=None, n=0):
    self.op, self.a, self.b, self.var, self.col, self.n = op, a, b, var, col, n

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
    if func in (np.sum, np.mean) and args and args[0] is self:
      return _reduce(self, 'np.' + func.__name__, args[1:], kwargs)
    raise _not_lowerable('np.{} of a {} in a density (reductions: np.sum, np.mean '
                         'of a data vector)'.format(
                             func.__name__, 'data vector' if self.n else 'scalar'))

  def sum(self, *args, **kwargs):
    return _reduce(self, '.sum', args, kwargs)

  def mean(self, *args, **kwargs):
    return _reduce(self, '.mean', args, kwargs)

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

  def _elements(self, *a):
    raise _not_lowerable('iterating, indexing or len() of a {} in a density '
                         '(the builtin sum iterates: use np.sum)'
                         .format('data vector' if self.n else 'symbolic scalar'))

  __floordiv__ = __rfloordiv__ = __mod__ = __rmod__ = __matmul__ = _unsupported
  __float__ = __int__ = __index__ = _unsupported
  __iter__ = __len__ = __getitem__ = _elements


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
  return vals, any(_symbolic(v) for v in vals)


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


def _trace(fn, keys):
  """fn called on symbolic variables under the patches: what it returned."""
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
      return fn(**kw)
    except NotLowerable:
      raise
    except Exception as e:
      raise NotLowerable('density callable not traceable: {}: {}'
                         .format(type(e).__name__, e))


def trace_expr(fn, keys):
  """A scalar density callable over the variables `keys` -> {'kind': 'expr',
  'code': int32[], 'consts': float64[], 'depth': int}, or NotLowerable.  A
  density that sums over 1-D data arrays also carries 'data' [C, n]."""
  from probayes_amd.lower import NotLowerable
  out = _trace(fn, keys)
  if not isinstance(out, Val):
    c = _const(out)
    if c is None:
      raise NotLowerable('density returned {}, not a scalar'
                         .format(type(out).__name__))
    out = c
  elif out.n:
    raise NotLowerable('density returned a vector of {} values unreduced (np.sum '
                       'or np.mean makes it a scalar)'.format(out.n))
  return compile_dag(out, len(keys))


def trace_pointwise(fn, keys):
  """A callable of the variables `keys` that returns the unreduced vector of n
  per-observation terms (a pointwise log-likelihood, a fitted value) -> the
  program of its sum, {'kind': 'expr', 'code', 'consts', 'depth', 'data'} as
  trace_expr gives it, of the pointwise shape: scalar words, LOOP, the body,
  and SUM as the last word.  The body's last value is the term
  (evaluate_pointwise; Engine.trace_pointwise reduces it over the trace)."""
  from probayes_amd.lower import NotLowerable
  out = _trace(fn, keys)
  if isinstance(out, np.ndarray) and out.ndim:
    out = _operand(out, 'the pointwise result')   # a data column as it is: a MOV
  if not isinstance(out, Val):
    if _const(out) is not None:
      raise NotLowerable('pointwise function returned a scalar, already reduced: '
                         'return the terms, not their sum')
    raise NotLowerable('pointwise function returned {}, not a vector of terms'
                       .format(type(out).__name__))
  if not out.n:
    if out.op == SUM or _under_sum(out):
      raise NotLowerable('pointwise function returned a scalar, already reduced: '
                         'return the terms, not their sum')
    raise NotLowerable('pointwise function returned a scalar that depends on no '
                       'data array: return one term per observation')
  return compile_dag(Val(SUM, out), len(keys))


def _under_sum(root):
  """Whether a SUM node lies under the scalar node root."""
  stack, seen = [root], set()
  while stack:
    v = stack.pop()
    if not isinstance(v, Val) or id(v) in seen:
      continue
    seen.add(id(v))
    if v.op == SUM:
      return True
    if not v.n:
      stack += [v.a, v.b]
  return False


# ---------------------------------------------------------------------------
# DAG -> program
# ---------------------------------------------------------------------------
def _computed(o):
  """A node with an instruction of its own (not a variable, a data column or
  a constant)."""
  return isinstance(o, Val) and o.var is None and o.col is None


def _region(total):
  """The vector nodes under a SUM node in dependency order, and the scalar
  nodes they read (which the outer program computes before the region)."""
  body, outer, seen = [], [], set()
  stack = [(total.a, False)]
  while stack:
    node, done = stack.pop()
    if not _computed(node) or id(node) in seen:
      continue
    if not node.n:        # a scalar: the outer program's
      seen.add(id(node))
      outer.append(node)
      continue
    if done:
      seen.add(id(node))
      body.append(node)
      continue
    stack.append((node, True))
    for o in (node.b, node.a):
      stack.append((o, False))
  return body, outer


def compile_dag(root, d):
  """Linearises the DAG under `root` in dependency order (each node once),
  keeps a result in the accumulator when only the next instruction reads it,
  and allocates slots by last use.  A SUM node becomes a loop region whose
  body is linearised the same way over body temporaries."""
  from probayes_amd.lower import NotLowerable
  consts, cindex = [], {}
  cols, colindex = [], {}

  def const(c):
    key = np.float64(c).tobytes()
    if key not in cindex:
      cindex[key] = len(consts)
      consts.append(np.float64(c))
    return (CONST, cindex[key])

  def column(v):
    key = v.col.tobytes()
    if key not in colindex:
      if cols and v.col.size != cols[0].size:   # two sums over different data
        raise NotLowerable('data arrays of two lengths ({} and {}) in one density'
                           .format(cols[0].size, v.col.size))
      if len(cols) == MAX_COLS:
        raise NotLowerable('density with more than {} data columns'.format(MAX_COLS))
      colindex[key] = len(cols)
      cols.append(v.col)
    return (VAR, BODY_BASE + colindex[key])

  regions = {}

  def children(node):
    if node.op == SUM:
      if id(node) not in regions:
        regions[id(node)] = _region(node)
      return regions[id(node)][1]
    return [o for o in (node.a, node.b) if _computed(o)]

  # post-order without recursion: operands before users, first use first
  order, index = [], {}
  if _computed(root):
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
      for o in reversed(children(node)):
        if id(o) not in index:
          stack.append((o, False))
  n_words = sum(len(regions[id(v)][0]) + 2 if v.op == SUM else 1 for v in order)
  if n_words > MAX_CODE:
    raise NotLowerable('expression of {} operations exceeds {} code words'
                       .format(n_words, MAX_CODE))
  users = [[] for _ in order]
  for i, node in enumerate(order):
    for o in children(node):
      users[index[id(o)]].append(i)
  code, slot_of, free, depth = [], {}, [], 0

  def body_words(total):
    """The region of one SUM node: LOOP, the body, without the SUM word."""
    body = regions[id(total)][0]
    bindex = {id(v): j for j, v in enumerate(body)}
    busers = [[] for _ in body]
    for j, node in enumerate(body):
      for o in (node.a, node.b):
        if id(o) in bindex:
          busers[bindex[id(o)]].append(j)
    words, temp_of, tfree, n_temps = [], {}, [], 0
    if not body:          # the sum of a column as it is
      words.append(encode(MOV, column(total.a)))
    for j, node in enumerate(body):
      ops = []
      for o in (node.a, node.b):
        if o is None:
          ops.append((SLOT, 0))
        elif not isinstance(o, Val):
          ops.append(const(o))
        elif o.var is not None:
          ops.append((VAR, o.var))
        elif o.col is not None:
          ops.append(column(o))
        elif not o.n:     # computed by the outer program, kept in a slot
          ops.append((SLOT, slot_of[index[id(o)]]))
        elif bindex[id(o)] == j - 1:
          ops.append((ACC, 0))
        else:
          ops.append((SLOT, BODY_BASE + temp_of[bindex[id(o)]]))
      for o in {bindex[id(o)] for o in (node.a, node.b) if id(o) in bindex}:
        if o in temp_of and max(busers[o]) == j:
          tfree.append(temp_of.pop(o))
      store = any(u != j + 1 for u in busers[j])
      dst = 0
      if store:
        if tfree:
          dst = min(tfree)
          tfree.remove(dst)
        else:
          dst = n_temps
          n_temps += 1
          if n_temps > MAX_TEMPS:
            raise NotLowerable('a sum whose terms keep more than {} intermediate '
                               'vectors alive'.format(MAX_TEMPS))
        temp_of[j] = dst
      words.append(encode(node.op, ops[0], ops[1], dst, store))
    return [encode(LOOP, (SLOT, len(words)))] + words

  if not order:   # a bare variable or a constant
    src = (VAR, root.var) if isinstance(root, Val) else const(root)
    code.append(encode(MOV, src))
  for i, node in enumerate(order):
    ops = []
    if node.op == SUM:
      code += body_words(node)
      ops = [(ACC, 0), (SLOT, 0)]
    else:
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
    for o in {index[id(o)] for o in children(node)}:
      if o in slot_of and max(users[o]) == i:
        free.append(slot_of.pop(o))
    # a region's body has an accumulator of its own: what it reads is in a slot
    store = any(u != i + 1 or order[u].op == SUM for u in users[i])
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
  out = {'kind': 'expr', 'code': np.asarray(code, np.int32),
         'consts': np.asarray(consts, np.float64), 'depth': int(depth)}
  if cols:
    out['data'] = np.stack(cols)
  return out


def check_program(code, consts, depth, d, data=None):
  """The checks pbh_set_model makes (ValueError with the cause).  data: the
  [C, n] block of a program with loop regions."""
  code = np.asarray(code).reshape(-1)
  n_consts = np.asarray(consts).size
  if not 1 <= code.size <= MAX_CODE:
    raise ValueError('expr: {} code words outside 1..{}'.format(code.size, MAX_CODE))
  if n_consts > MAX_CONSTS or not 0 <= depth <= MAX_SLOTS or not 1 <= d <= MAX_DIM:
    raise ValueError('expr: constants / depth / dim over the limits')
  n_cols = 0
  if data is not None:
    data = np.asarray(data)
    if data.ndim != 2 or not 1 <= data.shape[0] <= MAX_COLS or \
       not 1 <= data.shape[1] <= MAX_OBS:
      raise ValueError('expr: data of shape {} outside [1..{}, 1..{}]'
                       .format(data.shape, MAX_COLS, MAX_OBS))
    n_cols = data.shape[0]
  written = set()
  end = -1          # the SUM word of the open region, -1 outside one
  for pc, w in enumerate(code):
    if w < 0:
      raise ValueError('expr: bad code word at {}'.format(pc))
    op, dst, store, a, b = decode(w)
    if op == LOOP:
      if end >= 0:
        raise ValueError('expr: nested loop region at {}'.format(pc))
      if n_cols == 0:
        raise ValueError('expr: loop region without data at {}'.format(pc))
      end = pc + a[1] + 1
      if a[1] < 1 or end >= code.size or decode(code[end])[0] != SUM:
        raise ValueError('expr: loop region at {} does not end in SUM'.format(pc))
      first, temps = pc + 1, set()
      continue
    if op == SUM:
      if pc != end or a != (ACC, 0):
        raise ValueError('expr: SUM outside a loop region at {}'.format(pc))
      end = -1
    elif op >= N_OPS:
      raise ValueError('expr: bad opcode {} at {}'.format(op, pc))
    body = end >= 0
    for kind, i in (a, b)[:1 if op == SUM else ARITY[op]]:
      if body:
        ok = (kind == SLOT and (i - BODY_BASE in temps if i >= BODY_BASE
                                else i in written)) or \
             (kind == VAR and (i - BODY_BASE < n_cols if i >= BODY_BASE else i < d)) or \
             (kind == CONST and i < n_consts) or (kind == ACC and pc > first)
      else:
        ok = (kind == SLOT and i in written) or (kind == VAR and i < d) or \
             (kind == CONST and i < n_consts) or (kind == ACC and pc > 0)
      if not ok:
        raise ValueError('expr: bad operand ({}, {}) at {}'.format(kind, i, pc))
    if store and body:
      if dst >= MAX_TEMPS:
        raise ValueError('expr: body temporary {} >= {} at {} (a body writes no '
                         'outer slot)'.format(dst, MAX_TEMPS, pc))
      temps.add(dst)
    elif store:
      if dst >= depth:
        raise ValueError('expr: slot {} >= depth {} at {}'.format(dst, depth, pc))
      written.add(dst)
