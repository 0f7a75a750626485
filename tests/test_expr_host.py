"""The host side of the expression target on the CPU: pbh_expr_host.cpp's
checker and pairwise-sum leaves, driven by the stand-alone program
tests/expr_host_main.cpp built with the address and undefined-behaviour
sanitizers and run as a child process.

The checker is the trust boundary of the interpreter: its verdict must agree
with expr.check_program on every program the GPU tests use as good or bad, and
it must accept every example density.  The leaves fix the order of NumPy's
pairwise sum: summing in their order must give np.sum's bits."""
import os
import re
import subprocess

import numpy as np
import pytest

import probayes_amd as pb
from probayes_amd import expr
import expr_programs
from expr_examples import EXPR_WORKLOADS
from expr_data_examples import DATA_WORKLOADS
from host_program import compiler as _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'probayes_amd', 'csrc')
LEAF_STACK = 12        # kExprLeafStack (pbh_expr_words.h)
N_OBS = [1, 7, 8, 9, 127, 128, 129, 136, 137, 255, 256, 257, 300, 1000, 4097, 65536]
# np.sum adds the pairwise sums of buffers of 8192 elements one after another
N_OBS += [8192, 8193, 50000]


@pytest.fixture(scope='module')
def host(tmp_path_factory):
  """run(lines) -> the program's answers, one per request line"""
  cxx = _compiler()
  if cxx is None:
    pytest.skip('no host C++ compiler')
  tmp = tmp_path_factory.mktemp('expr_host')
  exe = str(tmp / 'expr_host_main')
  # the sanitizer runtimes linked into the program (clang's default), so that
  # it runs whatever else the loader brings in first
  version = subprocess.run([cxx, '--version'], capture_output=True, text=True).stdout
  static = [] if 'clang' in version else ['-static-libasan', '-static-libubsan']
  subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-Wall',
                         '-fsanitize=address,undefined', '-fno-sanitize-recover=all'] + static +
                        [os.path.join(ROOT, 'tests', 'expr_host_main.cpp'),
                         os.path.join(CSRC, 'pbh_expr_host.cpp'), '-o', exe])

  def run(lines):
    req = tmp / 'requests.txt'
    req.write_text(''.join(l + '\n' for l in lines))
    r = subprocess.run([exe, str(req)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out
  return run


def _request(p):
  code = [int(w) for w in np.asarray(p.code).reshape(-1)]
  n_cols, n_obs = (0, 0) if p.data is None else np.shape(p.data)
  return 'check {} {} {} {} {} {} {}'.format(
      p.d, p.depth, np.asarray(p.consts).size, n_cols, n_obs, len(code),
      ' '.join(str(w) for w in code))


def _python_verdict(p):
  """(accepted, failing pc or None) of expr.check_program"""
  try:
    expr.check_program(p.code, p.consts, p.depth, p.d, p.data)
  except ValueError as e:
    m = re.search(r'\bat (\d+)', str(e))
    return False, int(m.group(1)) if m else None
  return True, None


def _example_programs():
  out = []
  for workloads in (EXPR_WORKLOADS, DATA_WORKLOADS):
    for name in sorted(workloads):
      builder, params = workloads[name][:2]
      process, init, extra, kwds, keys = builder(pb, params)
      tg = process.lower()['target']
      assert tg['kind'] == 'expr'
      out.append(expr_programs.Program(tg['code'], tg['consts'], tg['depth'], len(keys),
                                       tg.get('data')))
  return out


def test_checker_agrees_with_check_program(host):
  sgood, sbad = expr_programs.scalar_cases()
  dgood, dbad = expr_programs.data_cases()
  cases = [sgood, dgood] + sbad + dbad
  assert len(sbad) == 4 and len(dbad) == 11
  answers = host([_request(p) for p in cases])
  for i, (p, ans) in enumerate(zip(cases, answers)):
    ok, pc = _python_verdict(p)
    assert ok == (i < 2), i           # the lists are what they say
    word = ans.split()
    assert (word[0] == 'ok') == ok, (i, ans)
    if pc is not None:
      assert word[0] == 'bad' and int(word[1]) == pc, (i, ans, pc)


def test_checker_accepts_every_example(host):
  progs = _example_programs()
  assert len(progs) == len(EXPR_WORKLOADS) + len(DATA_WORKLOADS)
  for p, ans in zip(progs, host([_request(p) for p in progs])):
    assert _python_verdict(p) == (True, None)
    assert ans.split()[0] == 'ok', ans


@pytest.fixture(scope='module')
def leaves(host):
  """n_obs -> (deepest stack, [(start, terms, pops)])"""
  out = {}
  for n, ans in zip(N_OBS, host(['leaves {}'.format(n) for n in N_OBS])):
    word = ans.split()
    assert word[0] == 'leaves'
    ws = [int(w) for w in word[2:]]
    out[n] = (int(word[1]), [((w & 8191) * 8, (w >> 13) & 255, w >> 21) for w in ws])
  return out


@pytest.mark.parametrize('n', N_OBS)
def test_leaves_tile_the_observations(leaves, n):
  deepest, ls = leaves[n]
  at, depth, most = 0, 0, 0       # depth: the pending sums on the stack
  for start, terms, pops in ls:
    assert start == at and start % 8 == 0 and 1 <= terms <= 128
    assert pops <= depth
    most = max(most, depth + 1)   # the pending sums and this leaf's result
    depth += 1 - pops
    at += terms
  assert at == n and depth == 1
  assert most == deepest <= LEAF_STACK


@pytest.mark.parametrize('n', N_OBS)
def test_sum_in_leaf_order_is_numpy_sum(leaves, n):
  """8 accumulators over whole blocks, the fixed tree, the tail one by one,
  then the pops (left + right, innermost first): np.sum's bits."""
  a = np.random.RandomState(500 + n % 1000).normal(0., 1e3, n)
  stack = []
  for start, terms, pops in leaves[n][1]:
    t = a[start:start + terms]
    if terms < 8:
      res, tail = np.float64(0.), t
    else:
      whole = terms - terms % 8
      r = t[:8].copy()
      for b in range(8, whole, 8):
        r += t[b:b + 8]
      res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
      tail = t[whole:]
    for v in tail:
      res = res + v
    for _ in range(pops):
      res = stack.pop() + res
    stack.append(res)
  assert len(stack) == 1
  want = np.sum(a)
  assert stack[0].tobytes() == np.float64(want).tobytes(), (stack[0], want)
