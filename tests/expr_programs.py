"""Programs the engine's checker must accept or refuse, shared by the GPU
tests (through pbh_eval_expr* / pbh_set_model) and the CPU test of the host
unit (tests/test_expr_host.py, through the stand-alone program).

A case is a Program: code, consts, depth, the number of variables d and the
data block [C, n] (None: a program without regions)."""
import collections

import numpy as np

from probayes_amd import expr

Program = collections.namedtuple('Program', 'code consts depth d data')


def arith(**kw):
  """+ - * /, square, sqrt, neg, abs, max, min: IEEE operations only."""
  x, y, z = kw['x'], kw['y'], kw['z']
  r = np.sqrt(abs(x) + y * y + 1.5) / (np.square(z) + 0.25)
  m = np.maximum(x - y, z * 0.5) + np.minimum(-x, y / 3.)
  return -(r * m - x / (abs(z) + 2.)) + r


def scalar_cases():
  """(good, bad): a traced program of three variables and the ways to spoil it."""
  tg = expr.trace_expr(arith, ['x', 'y', 'z'])
  good = Program(tg['code'], tg['consts'], tg['depth'], 3, None)
  bad = []
  for word in (expr.encode(expr.ADD, (expr.VAR, 3), (expr.VAR, 0)),   # variable 3 of 3
               expr.encode(expr.NEG, (expr.SLOT, 5)),                 # unwritten slot
               expr.N_OPS):                                           # unknown opcode
    code = good.code.copy()
    code[0] = word
    bad.append(good._replace(code=code))
  bad.append(good._replace(consts=good.consts[:1]))                   # constants missing
  return good, bad


def data_cases():
  """(good, bad): a one-word body over two columns of nine observations."""
  E, V, A, S, B = expr.encode, expr.VAR, expr.ACC, expr.SLOT, expr.BODY_BASE
  data = np.ones((2, 9))
  loop = lambda n: E(expr.LOOP, (S, n))
  total = E(expr.SUM, (A, 0))
  body = [E(expr.MUL, (V, B + 0), (V, 0))]
  good = Program([loop(1)] + body + [total], [], 0, 1, data)
  codes = [
      [loop(3), loop(1)] + body + [total, total],                        # nested
      [loop(1), E(expr.MUL, (V, B + 2), (V, 0)), total],                 # column 2 of 2
      [loop(1), E(expr.MUL, (V, B + 0), (S, B + 0)), total],             # unwritten temporary
      [loop(1), E(expr.MUL, (V, B + 0), (V, 0), dst=4, store=True), total],
      [loop(1), E(expr.NEG, (A, 0)), total],                             # acc, first word
      [loop(2)] + body + [total],                                        # no SUM at the end
      [loop(1)] + body,                                                  # past the end
      body + [total],                                                    # SUM alone
      [loop(1), E(expr.MUL, (V, B + 0), (S, 0)), total],                 # unwritten slot
  ]
  bad = [Program(code, [], 1, 1, data) for code in codes]
  bad.append(good._replace(data=np.ones((9, 4))))                        # nine columns
  bad.append(good._replace(data=np.ones((1, expr.MAX_OBS + 1))))
  return good, bad
