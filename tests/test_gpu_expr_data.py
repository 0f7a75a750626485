"""Likelihoods summed over observed data arrays on the GPU: the interpreter
with loop regions against its NumPy definition, bit-equality with the
hand-written iid-Normal kernel, the reference's recorded chains, the production
RNG modes, and the two body forms (8 observations wide, one at a time)."""
import numpy as np
import pytest
import scipy.stats

import oracle
import probayes_amd as pb
from probayes_amd import expr
from probayes_amd._lib import PbhError
from probayes_amd.engine import Engine, eval_expr
import expr_programs
from expr_data_examples import DATA_WORKLOADS

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
# 1. pbh_eval_expr_data against expr.evaluate
# ---------------------------------------------------------------------------
def _data(n):
  rs = np.random.RandomState(70 + n)
  return rs.normal(0., 1.5, n), rs.normal(1., 2., n), rs.uniform(0.5, 2., n)


def _arith_program(n):
  """+ - * / sqrt abs neg alone, two columns re-read through temporaries."""
  X, Y, W = _data(n)
  def fn(**kw):
    r = (Y - (kw['a'] + kw['b'] * X)) / W
    return np.sum(np.sqrt(abs(r) + 0.25) * r - r * r / (abs(kw['b']) + 1.5)) \
        - kw['a'] * kw['a'] / 7.
  return expr.trace_expr(fn, ['a', 'b'])


def _every_opcode_program(n):
  """A hand-assembled body with every elementwise opcode, an outer slot, the
  four temporaries and three columns; outer code before and after."""
  E, V, C, A, S, B = expr.encode, expr.VAR, expr.CONST, expr.ACC, expr.SLOT, expr.BODY_BASE
  X, Y, W = _data(n)
  code = [E(expr.ABS, (V, 1)),
          E(expr.ADD, (A, 0), (C, 0), dst=0, store=True),       # slot 0 = |b| + 0.5
          E(expr.LOOP, (S, 20)),
          E(expr.MOV, (V, B + 0), dst=0, store=True),           # t0 = X
          E(expr.MUL, (A, 0), (V, 1)),
          E(expr.ADD, (A, 0), (V, 0), dst=1, store=True),       # t1 = a + b X
          E(expr.SUB, (V, B + 1), (A, 0)),
          E(expr.DIV, (A, 0), (V, B + 2), dst=2, store=True),   # t2 = (Y - t1) / W
          E(expr.ABS, (A, 0)),
          E(expr.SQRT, (A, 0)),
          E(expr.NEG, (A, 0)),
          E(expr.EXP, (A, 0), dst=3, store=True),               # t3 = exp(-sqrt|t2|)
          E(expr.LOG1P, (A, 0)),
          E(expr.EXPM1, (A, 0)),
          E(expr.ADD, (A, 0), (S, 0)),                          # + the outer slot
          E(expr.LOG, (A, 0)),
          E(expr.POW, (A, 0), (C, 1)),
          E(expr.MAX, (A, 0), (S, B + 2)),
          E(expr.MIN, (A, 0), (S, B + 3)),
          E(expr.MUL, (A, 0), (S, B + 1)),
          E(expr.SUB, (A, 0), (S, B + 0)),
          E(expr.ADD, (A, 0), (S, B + 3)),
          E(expr.MUL, (A, 0), (C, 2)),
          E(expr.SUM, (A, 0), dst=1, store=True),
          E(expr.MUL, (A, 0), (S, 0)),
          E(expr.SUB, (A, 0), (S, 1))]
  return {'code': np.array(code, np.int32), 'consts': np.array([0.5, 3.0, 0.125]),
          'depth': 2, 'data': np.stack([X, Y, W])}


@pytest.mark.parametrize('points', [1, 65, 257])
@pytest.mark.parametrize('n', [1, 7, 8, 9, 128, 129, 137, 300])
@pytest.mark.parametrize('which', ['arith', 'every_opcode'])
def test_eval_expr_data_matches_numpy_interpreter(which, n, points):
  tg = _arith_program(n) if which == 'arith' else _every_opcode_program(n)
  if which == 'every_opcode':
    ops = {expr.decode(w)[0] for w in tg['code'][3:23]}
    assert ops == set(range(expr.N_OPS))
    stores = {expr.decode(w)[1] for w in tg['code'][3:23] if expr.decode(w)[2]}
    assert stores == set(range(expr.MAX_TEMPS))
  expr.check_program(tg['code'], tg['consts'], tg['depth'], 2, tg['data'])
  pts = np.random.RandomState(12).normal(0., 1., size=(257, 2))[:points]
  want = expr.evaluate(tg['code'], tg['consts'], pts, tg['data'])
  assert np.all(np.isfinite(want))
  got = eval_expr(tg['code'], tg['consts'], tg['depth'], pts, data=tg['data'])
  print(which, n, points, 'max rel err', _rel_err(got, want, 1.),
        'bit-equal', bool(np.array_equal(got, want)))
  if which == 'arith':
    assert np.array_equal(got, want)
  else:
    assert _rel_err(got, want, 1.) <= RTOL


# ---------------------------------------------------------------------------
# 2. bad programs are refused before any launch
# ---------------------------------------------------------------------------
def test_set_model_refuses_bad_data_programs(monkeypatch):
  good, bad = expr_programs.data_cases()
  pts = np.zeros((4, 1))
  assert np.array_equal(eval_expr(good.code, good.consts, good.depth, pts + 2., data=good.data),
                        np.full(4, 18.))
  assert len(bad) == 11
  for p in bad:
    with pytest.raises(PbhError):
      eval_expr(p.code, p.consts, p.depth, pts, data=p.data)
  # through pbh_set_model: the engine's own check (make_spec's is bypassed)
  spec = pb.make_spec(1, {'kind': 'expr', 'code': good.code, 'consts': [], 'depth': 0,
                          'data': good.data}, {'kind': 'gauss', 'scale': 1.}, pscale='log')
  spec['target']['code'] = np.array(bad[1].code, np.int32)
  import probayes_amd.engine as engine_mod
  monkeypatch.setattr(engine_mod, 'normalize_spec', lambda s: s)
  with pytest.raises(PbhError):
    Engine(spec)


# ---------------------------------------------------------------------------
# 3. bit-equality with the hand-written iid-Normal kernel
# ---------------------------------------------------------------------------
def _run_trace(spec, init, t, thin, rng, streams=None, seed=4321, spl=25):
  eng = Engine(spec)
  eng.init_chains(init)
  eng.set_rng(rng, seed=seed)
  if streams is not None:
    eng.upload_replay(streams)
  eng.alloc_trace(t // thin, thin, debug=True)
  eng.run(t, steps_per_launch=spl)
  out, mom = eng.trace(), eng.moments()
  eng.close()
  return out, mom


@pytest.mark.parametrize('thin', [1, 3])
@pytest.mark.parametrize('rng', ['replay', 'philox_f64'])
@pytest.mark.parametrize('n_obs', [7, 137])
def test_expr_sum_is_bit_equal_to_norm_iid(n_obs, rng, thin):
  """np.sum(norm.logpdf(OBS, mu, sg)) as an expression and as the norm_iid
  target: both run np_pairwise over norm_logpdf in scipy's operation order."""
  obs = np.random.RandomState(40 + n_obs).normal(0.8, 1.7, n_obs)
  tg = expr.trace_expr(
      lambda **kw: np.sum(scipy.stats.norm.logpdf(obs, kw['mu'], kw['sg'])), ['mu', 'sg'])
  assert tg['kind'] == 'expr' and tg['data'].shape == (1, n_obs)
  # sg starts at 2.5 .. 3.5 and moves by less than 0.02 a step: positive; mu
  # moves on the scale of its posterior, sg / sqrt(n_obs)
  prop = {'kind': 'uniform', 'delta': [4.0 if n_obs == 7 else 0.6, 0.02]}
  e_spec = pb.make_spec(2, tg, prop, pscale='log')
  h_spec = pb.make_spec(2, {'kind': 'norm_iid', 'obs': obs, 'loc': 0, 'scale': 1}, prop,
                        pscale='log')
  n, t = 257, 64 - 64 % thin
  rs = np.random.RandomState(3)
  init = np.stack([rs.normal(0.8, 0.5, n), rs.uniform(2.5, 3.5, n)], -1)
  streams = oracle.legacy_streams(e_spec, np.arange(900, 900 + n), t) \
      if rng == 'replay' else None
  got, gmom = _run_trace(e_spec, init, t, thin, rng, streams)
  ref, rmom = _run_trace(h_spec, init, t, thin, rng, streams)
  assert ref['p_x'][..., 1].min() > 0. and ref['v_x'][..., 1].min() > 0.
  assert 0.05 < ref['u'].mean() < 0.95
  for k in ('v_x', 'v_p', 'p_x', 'p_p', 's', 'u'):
    np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
  for k in ('sum', 'sumsq', 'n_acc', 'n_steps'):
    np.testing.assert_array_equal(gmom[k], rmom[k], err_msg=k)


# ---------------------------------------------------------------------------
# 4, 5. the reference's recorded chains
# ---------------------------------------------------------------------------
def _build(name):
  builder, params, n, t, seed0 = DATA_WORKLOADS[name]
  process, init, extra, kwds, keys = builder(pb, params)
  return process, init, keys, oracle.load_golden(name)


@pytest.mark.parametrize('name', sorted(DATA_WORKLOADS))
def test_replay_matches_reference_golden(name):
  process, init, keys, g = _build(name)
  spec = process.lower()
  assert spec['target']['kind'] == 'expr' and spec['target']['data'].ndim == 2
  n, t = g['v_x'].shape[:2]
  streams = oracle.legacy_streams(spec, g['seeds'], t)
  x0 = np.tile(np.array([init[k] for k in keys], np.float64), (n, 1))
  out, mom = _run_trace(spec, x0, t, 1, 'replay', streams)
  flips = int(np.sum(out['u'] != g['u']))
  print(name, 'flips', flips, 'v_x', _rel_err(out['v_x'], g['v_x'], 1.),
        'v_p', _rel_err(out['v_p'], g['v_p']), 'p_x', _rel_err(out['p_x'], g['p_x'], 1.),
        'p_p', _rel_err(out['p_p'], g['p_p']), 's', _rel_err(out['s'], g['s']))
  assert flips == 0, '{}: {} accept flips'.format(name, flips)
  assert _rel_err(out['v_x'], g['v_x'], 1.) <= RTOL
  assert _rel_err(out['v_p'], g['v_p']) <= RTOL
  assert _rel_err(out['p_x'], g['p_x'], 1.) <= RTOL
  assert _rel_err(out['p_p'], g['p_p']) <= RTOL
  assert _rel_err(out['s'], g['s']) <= 1e-10
  assert np.array_equal(mom['n_acc'], g['u'].sum(axis=1))


@pytest.mark.parametrize('name', sorted(DATA_WORKLOADS))
def test_batched_sampler_reproduces_reference_chains(name):
  """The facade's seeded sampler: the device's own legacy streams, then the
  run (pbh_legacy_run's generation-then-run path)."""
  process, init, keys, g = _build(name)
  n, t = g['v_x'].shape[:2]
  sampler = process.sampler(init, stop=t, chains=n, seeds=g['seeds'])
  summary = process(process.walk(sampler))
  assert sampler.spec['target']['kind'] == 'expr'
  assert sampler.spec['target']['data'].ndim == 2
  for i, k in enumerate(keys):
    got = np.asarray(summary.v[k]).T            # [N, T]
    assert _rel_err(got, g['v_x'][:, :, i], 1.) <= RTOL
  assert _rel_err(np.asarray(summary.v.prob).T, g['v_p']) <= RTOL
  assert summary.u.count(True) == int(g['u'].sum())


# ---------------------------------------------------------------------------
# 6. production modes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['philox', 'xoshiro'])
def test_production_modes_statistics_and_invariants(mode):
  """np.sum(norm.logpdf(OBS, mu, 1.3)) with n = 40: the posterior of mu under
  the flat prior is N(mean(OBS), 1.3^2 / 40); mean and second moment within 5
  MCSE (the criterion of test_philox_diag10_statistics_and_invariants),
  determinism, sharding, launch splits."""
  obs = np.random.RandomState(91).normal(0.4, 1.3, 40)
  tg = expr.trace_expr(
      lambda **kw: np.sum(scipy.stats.norm.logpdf(obs, kw['mu'], 1.3)), ['mu'])
  spec = pb.make_spec(1, tg, {'kind': 'gauss', 'scale': 0.4}, pscale='log')
  m0, v0 = obs.mean(), 1.3 ** 2 / 40
  n, t = 4096, 600
  init = m0 + np.sqrt(v0) * np.random.RandomState(77).standard_normal((n, 1))
  eng = Engine(spec)
  eng.init_chains(init)
  eng.set_rng(mode, seed=1234)
  eng.run(t)
  mom = eng.moments()
  eng.close()
  steps = mom['n_steps']
  m_c, q_c = mom['sum'] / steps, mom['sumsq'] / steps
  mean, mcse_m = m_c.mean(0), m_c.std(0) / np.sqrt(n)
  assert np.all(np.abs(mean - m0) <= 5 * mcse_m), ((mean - m0) / mcse_m)
  q, mcse_q = q_c.mean(0), q_c.std(0) / np.sqrt(n)
  assert np.all(np.abs(q - (m0 ** 2 + v0)) <= 5 * mcse_q), ((q - m0 ** 2 - v0) / mcse_q)
  acc = mom['n_acc'].sum() / (n * steps)
  assert 0.05 < acc < 0.9

  def run(n0, n1, spl):
    e = Engine(spec)
    e.init_chains(np.zeros((n1 - n0, 1)), chain_offset=n0)
    e.set_rng(mode, seed=99)
    e.alloc_trace(50, 1)
    e.run(50, steps_per_launch=spl)
    tr = e.trace()
    e.close()
    return tr
  full, again, split = run(0, 4096, 50), run(0, 4096, 50), run(0, 4096, 17)
  lo, hi = run(0, 2048, 50), run(2048, 4096, 50)
  for k in ('v_x', 'v_p', 'u'):
    np.testing.assert_array_equal(full[k], again[k])
    np.testing.assert_array_equal(full[k], split[k])
    np.testing.assert_array_equal(full[k][:2048], lo[k])
    np.testing.assert_array_equal(full[k][2048:], hi[k])


# ---------------------------------------------------------------------------
# 7. the two body forms
# ---------------------------------------------------------------------------
def test_wide_and_one_at_a_time_bodies_give_identical_traces(monkeypatch):
  process, init, keys, g = _build('data_linreg3')
  spec = process.lower()
  n, t = 257, 48
  streams = oracle.legacy_streams(spec, np.arange(5000, 5000 + n), t)
  rs = np.random.RandomState(6)
  x0 = np.stack([rs.normal(0.7, 0.1, n), rs.normal(-1.2, 0.1, n),
                 rs.uniform(0.6, 1.2, n)], -1)
  tg = spec['target']
  pts = np.stack([rs.normal(0., 2., n), rs.normal(0., 2., n), rs.uniform(0.1, 5., n)], -1)
  monkeypatch.setenv('PBH_EXPR_DATA_WIDE', '1')
  wide, wmom = _run_trace(spec, x0, t, 1, 'replay', streams)
  wide_f64, _ = _run_trace(spec, x0, t, 1, 'philox_f64')
  wide_eval = eval_expr(tg['code'], tg['consts'], tg['depth'], pts, data=tg['data'])
  monkeypatch.setenv('PBH_EXPR_DATA_WIDE', '0')
  one, omom = _run_trace(spec, x0, t, 1, 'replay', streams)
  one_f64, _ = _run_trace(spec, x0, t, 1, 'philox_f64')
  one_eval = eval_expr(tg['code'], tg['consts'], tg['depth'], pts, data=tg['data'])
  assert 0.05 < wide['u'].mean() < 0.95
  for k in ('v_x', 'v_p', 'p_x', 'p_p', 's', 'u'):
    np.testing.assert_array_equal(wide[k], one[k], err_msg=k)
    np.testing.assert_array_equal(wide_f64[k], one_f64[k], err_msg=k)
  for k in ('sum', 'sumsq', 'n_acc', 'n_steps'):
    np.testing.assert_array_equal(wmom[k], omom[k], err_msg=k)
  np.testing.assert_array_equal(wide_eval, one_eval)
