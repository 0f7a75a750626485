"""The expression target on the GPU: the interpreter against its NumPy
definition, bit-equality with the hand-written kernels on densities both can
run, the reference's recorded chains, the CPU oracle, and the production RNG
modes."""
import numpy as np
import pytest
import scipy.stats

import oracle
import oracle.mh
import probayes_amd as pb
from probayes_amd import expr
from probayes_amd.engine import Engine, eval_expr
import expr_programs
from expr_examples import EXPR_WORKLOADS, banana_lp

pytestmark = pytest.mark.gpu

RTOL = 1e-12          # the project's parity bar (tests/test_gpu_parity.py)


def _rel_err(a, b, floor=np.finfo(float).tiny):
  """max |a - b| / max(|b|, floor), as tests/test_gpu_parity.py."""
  a, b = np.asarray(a, float), np.asarray(b, float)
  both_nan = np.isnan(a) & np.isnan(b)
  same = (a == b) | both_nan
  den = np.maximum(np.abs(b), floor)
  err = np.where(same, 0., np.abs(a - b) / den)
  return float(err.max()) if err.size else 0.


# ---------------------------------------------------------------------------
# 1. pbh_eval_expr against expr.evaluate
# ---------------------------------------------------------------------------
_arith = expr_programs.arith


def _every_opcode():
  """All fifteen opcodes, hand-assembled (MOV comes from no traced density
  but a bare variable); the same thing as a Python function of scalars."""
  E, V, C, A, S = expr.encode, expr.VAR, expr.CONST, expr.ACC, expr.SLOT
  code = [E(expr.MOV, (V, 0), dst=0, store=True),
          E(expr.ABS, (A, 0)),
          E(expr.ADD, (A, 0), (C, 0), dst=1, store=True),
          E(expr.SQRT, (A, 0)),
          E(expr.LOG, (A, 0)),
          E(expr.EXP, (A, 0)),
          E(expr.LOG1P, (A, 0)),
          E(expr.EXPM1, (A, 0)),
          E(expr.POW, (A, 0), (C, 1)),
          E(expr.MUL, (A, 0), (V, 1)),
          E(expr.SUB, (A, 0), (S, 0)),
          E(expr.DIV, (A, 0), (S, 1)),
          E(expr.NEG, (A, 0)),
          E(expr.MAX, (A, 0), (V, 2)),
          E(expr.MIN, (A, 0), (C, 2))]
  consts = [0.5, 1.5, 3.0]

  def fn(x, y, z):
    a = abs(x) + 0.5
    v = np.expm1(np.log1p(np.exp(np.log(np.sqrt(a))))) ** 1.5
    return np.minimum(np.maximum(-((v * y - x) / a), z), 3.0)
  return {'code': np.array(code, np.int32), 'consts': np.array(consts), 'depth': 2}, fn


def _deep(**kw):
  """Fifteen values each read twice, far apart, and the running sum: 16
  slots alive at once."""
  vals = [np.exp(kw['x'] * ((i + 1) / 16.)) for i in range(15)]
  out = sum(vals)
  for v in vals:
    out = out * v
  return out + kw['y'] + kw['z']


def _long(**kw):
  """256 code words: 128 times (multiply, add)."""
  out = abs(kw['x']) + kw['z'] * kw['z']
  for _ in range(126):
    out = out * 0.75 + kw['y']
  return np.log1p(out)


def _eval_points(n):
  rs = np.random.RandomState(11)
  pts = np.empty((257, 3))
  pts[:, 0] = -rs.uniform(0.1, 2., 257)      # x < 0: nothing cancels below
  pts[:, 1] = rs.uniform(1., 2., 257)
  pts[:, 2] = rs.uniform(-1., 1., 257)
  return np.ascontiguousarray(pts[:n])


def _program(which):
  keys = ['x', 'y', 'z']
  if which == 'every_opcode':
    tg, fn = _every_opcode()
    return tg, (lambda **kw: fn(kw['x'], kw['y'], kw['z']))
  fn = {'arith': _arith, 'deep': _deep, 'long': _long}[which]
  return expr.trace_expr(fn, keys), fn


@pytest.mark.parametrize('n', [1, 64, 65, 257])
@pytest.mark.parametrize('which', ['arith', 'every_opcode', 'deep', 'long'])
def test_eval_expr_matches_numpy_interpreter(which, n):
  tg, fn = _program(which)
  if which == 'every_opcode':
    assert sorted({expr.decode(w)[0] for w in tg['code']}) == list(range(expr.N_OPS))
  if which == 'deep':
    assert tg['depth'] == expr.MAX_SLOTS
  if which == 'long':
    assert len(tg['code']) == expr.MAX_CODE
  expr.check_program(tg['code'], tg['consts'], tg['depth'], 3)
  pts = _eval_points(n)
  want = expr.evaluate(tg['code'], tg['consts'], pts)
  assert np.all(np.isfinite(want))
  # NumPy's scalar results agree with its array results at these points
  scalar = np.array([fn(x=np.float64(p[0]), y=np.float64(p[1]), z=np.float64(p[2]))
                     for p in pts])
  assert _rel_err(scalar, want, 1.) <= RTOL
  got = eval_expr(tg['code'], tg['consts'], tg['depth'], pts)
  print(which, n, 'max rel err', _rel_err(got, want, 1.),
        'bit-equal', bool(np.array_equal(got, want)))
  if which == 'arith':
    assert np.array_equal(got, want)
  else:
    assert _rel_err(got, want, 1.) <= RTOL


def test_set_model_refuses_bad_programs():
  from probayes_amd._lib import PbhError
  good, bad = expr_programs.scalar_cases()
  pts = _eval_points(4)
  assert len(bad) == 4
  for p in bad:
    with pytest.raises(PbhError):
      eval_expr(p.code, p.consts, p.depth, pts)


# ---------------------------------------------------------------------------
# 2. bit-equality with the hand-written kernels
# ---------------------------------------------------------------------------
_MU3 = np.array([-0.5, 0.25, 1.0])
_SG3 = np.array([0.7, 1.3, 2.1])
_LOGC = np.log(np.sqrt(2 * np.pi))
_C = np.sqrt(2 * np.pi)


def _gauss3(**kw):
  """The 3-d diagonal Gaussian in scipy's operation order; log(sigma) is the
  array value the engine uploads for diag_gauss."""
  lsg = np.log(_SG3)
  return sum(-((kw[k] - _MU3[i]) / _SG3[i]) ** 2 / 2. - _LOGC - lsg[i]
             for i, k in enumerate(('x', 'y', 'z')))


def _normpdf1(**kw):
  y = (kw['x'] - 0.4) / 1.7
  return np.exp(-y ** 2 / 2.) / _C / 1.7


def _pair(model):
  if model == 'gauss3':
    d, keys, fn, ps = 3, ['x', 'y', 'z'], _gauss3, 'log'
    hand = {'kind': 'diag_gauss', 'mu': _MU3, 'sigma': _SG3}
  else:
    d, keys, fn, ps = 1, ['x'], _normpdf1, 'lin'
    hand = {'kind': 'norm_pdf', 'loc': [0.4], 'scale': [1.7]}
  prop = {'kind': 'gauss', 'scale': 0.8}
  tg = expr.trace_expr(fn, keys)
  assert tg['kind'] == 'expr'
  return (pb.make_spec(d, tg, prop, pscale=ps), pb.make_spec(d, hand, prop, pscale=ps))


def _run_trace(spec, init, t, thin, rng, streams=None, seed=4321):
  eng = Engine(spec)
  eng.init_chains(init)
  eng.set_rng(rng, seed=seed)
  if streams is not None:
    eng.upload_replay(streams)
  eng.alloc_trace(t // thin, thin, debug=True)
  eng.run(t, steps_per_launch=25)
  out, mom = eng.trace(), eng.moments()
  eng.close()
  return out, mom


@pytest.mark.parametrize('thin', [1, 3])
@pytest.mark.parametrize('rng', ['replay', 'philox_f64'])
@pytest.mark.parametrize('model', ['gauss3', 'normpdf1'])
def test_expr_is_bit_equal_to_the_handwritten_kernels(model, rng, thin):
  """The same operations in the same order with the same OCML calls."""
  e_spec, h_spec = _pair(model)
  n, t = 257, 64 - 64 % thin
  d = e_spec['dim']
  init = np.random.RandomState(3).normal(size=(n, d))
  streams = oracle.legacy_streams(e_spec, np.arange(900, 900 + n), t) \
      if rng == 'replay' else None
  got, gmom = _run_trace(e_spec, init, t, thin, rng, streams)
  ref, rmom = _run_trace(h_spec, init, t, thin, rng, streams)
  assert 0.05 < ref['u'].mean() < 0.95
  for k in ('v_x', 'v_p', 'p_x', 'p_p', 's', 'u'):
    np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
  for k in ('sum', 'sumsq', 'n_acc', 'n_steps'):
    np.testing.assert_array_equal(gmom[k], rmom[k], err_msg=k)


# ---------------------------------------------------------------------------
# 3. the reference's recorded chains
# ---------------------------------------------------------------------------
def _build(name):
  builder, params, n, t, seed0 = EXPR_WORKLOADS[name]
  process, init, extra, kwds, keys = builder(pb, params)
  return process, init, keys, oracle.load_golden(name)


@pytest.mark.parametrize('name', sorted(EXPR_WORKLOADS))
def test_replay_matches_reference_golden(name):
  process, init, keys, g = _build(name)
  spec = process.lower()
  assert spec['target']['kind'] == 'expr'
  n, t = g['v_x'].shape[:2]
  streams = oracle.legacy_streams(spec, g['seeds'], t)
  x0 = np.tile(np.array([init[k] for k in keys], np.float64), (n, 1))
  out, mom = _run_trace(spec, x0, t, 1, 'replay', streams)
  flips = int(np.sum(out['u'] != g['u']))
  print(name, 'flips', flips, 'v_x', _rel_err(out['v_x'], g['v_x'], 1.),
        'v_p', _rel_err(out['v_p'], g['v_p']), 'p_x', _rel_err(out['p_x'], g['p_x'], 1.),
        'p_p', _rel_err(out['p_p'], g['p_p']))
  assert flips == 0, '{}: {} accept flips'.format(name, flips)
  assert _rel_err(out['v_x'], g['v_x'], 1.) <= RTOL
  assert _rel_err(out['v_p'], g['v_p']) <= RTOL
  assert _rel_err(out['p_x'], g['p_x'], 1.) <= RTOL
  assert _rel_err(out['p_p'], g['p_p']) <= RTOL
  assert _rel_err(out['s'], g['s']) <= 1e-10
  assert np.array_equal(mom['n_acc'], g['u'].sum(axis=1))


@pytest.mark.parametrize('name', sorted(EXPR_WORKLOADS))
def test_batched_sampler_reproduces_reference_chains(name):
  """The facade's seeded sampler: the device's own legacy streams, then the
  run (pbh_legacy_run's generation-then-run path)."""
  process, init, keys, g = _build(name)
  n, t = g['v_x'].shape[:2]
  sampler = process.sampler(init, stop=t, chains=n, seeds=g['seeds'])
  summary = process(process.walk(sampler))
  assert sampler.spec['target']['kind'] == 'expr'
  for i, k in enumerate(keys):
    got = np.asarray(summary.v[k]).T            # [N, T]
    assert _rel_err(got, g['v_x'][:, :, i], 1.) <= RTOL
  assert _rel_err(np.asarray(summary.v.prob).T, g['v_p']) <= RTOL
  assert summary.u.count(True) == int(g['u'].sum())


# ---------------------------------------------------------------------------
# 4. the CPU oracle with the Python callable as its density
# ---------------------------------------------------------------------------
def test_banana_matches_the_oracle(monkeypatch):
  process, init, keys, g = _build('expr_banana2')
  spec = process.lower()
  n, t = 257, 40
  monkeypatch.setattr(oracle.mh, 'target_prob',
                      lambda spec, x: np.asarray(banana_lp(x[0], x[1]), np.float64))
  streams = oracle.legacy_streams(spec, np.arange(31000, 31000 + n), t)
  x0 = np.random.RandomState(8).normal(0., 1., size=(n, 2))
  ref = oracle.run_mh(spec, x0, streams)
  out, _ = _run_trace(spec, x0, t, 1, 'replay', streams)
  assert int(np.sum(out['u'] != ref['u'])) == 0
  assert 0.1 < ref['u'].mean() < 0.9
  for k, floor in (('v_x', 1.), ('p_x', 1.)):
    assert _rel_err(out[k], ref[k], floor) <= RTOL
  for k in ('v_p', 'p_p'):
    assert _rel_err(out[k], ref[k]) <= RTOL


# ---------------------------------------------------------------------------
# 5. production modes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['philox', 'xoshiro'])
def test_production_modes_statistics_and_invariants(mode):
  """The hand-written Gaussian through the interpreter in the production RNG
  modes: the posterior within 5 MCSE (the criterion of
  test_philox_diag10_statistics_and_invariants), determinism, sharding."""
  spec, _ = _pair('gauss3')
  n, t = 4096, 600
  init = _MU3 + _SG3 * np.random.RandomState(77).standard_normal((n, 3))
  eng = Engine(spec)
  eng.init_chains(init)
  eng.set_rng(mode, seed=1234)
  eng.run(t)
  mom = eng.moments()
  eng.close()
  steps = mom['n_steps']
  m_c, q_c = mom['sum'] / steps, mom['sumsq'] / steps
  mean, mcse_m = m_c.mean(0), m_c.std(0) / np.sqrt(n)
  assert np.all(np.abs(mean - _MU3) <= 5 * mcse_m), ((mean - _MU3) / mcse_m)
  q, mcse_q = q_c.mean(0), q_c.std(0) / np.sqrt(n)
  assert np.all(np.abs(q - (_MU3 ** 2 + _SG3 ** 2)) <= 5 * mcse_q), \
      ((q - _MU3 ** 2 - _SG3 ** 2) / mcse_q)
  acc = mom['n_acc'].sum() / (n * steps)
  assert 0.05 < acc < 0.9

  def run(n0, n1, spl=17):
    e = Engine(spec)
    e.init_chains(np.zeros((n1 - n0, 3)), chain_offset=n0)
    e.set_rng(mode, seed=99)
    e.alloc_trace(50, 1)
    e.run(50, steps_per_launch=spl)
    tr = e.trace()
    e.close()
    return tr
  full, again = run(0, 4096), run(0, 4096)
  lo, hi = run(0, 2048), run(2048, 4096)
  for k in ('v_x', 'v_p', 'u'):
    np.testing.assert_array_equal(full[k], again[k])
    np.testing.assert_array_equal(full[k][:2048], lo[k])
    np.testing.assert_array_equal(full[k][2048:], hi[k])
