"""The production Philox kernels pinned to the oracle on fixed seeds.

Each kernel's draws are a pure function of (seed, chain id, absolute step);
tests/philox_host.py rebuilds them in NumPy.  check_steps then replays EVERY
recorded step of EVERY chain through oracle.mh from the GPU's own previous
record (so nothing accumulates and a chain is checked past its first
disagreement): the proposal, the density, the score and the decision are the
oracle's, the randoms are the host-rebuilt ones.

Forms covered (thin 1, trace allocated): the lane-pair kernel in its
steady-state and general forms and at the ends of its d range, cfg1's
one-lane steady-state kernel, the GMM quad kernel (8- and 4-step groups, and
its general form), the GMM lane-pair kernel, the general mh_kernel with
Gaussian and with uniform draws (d = 1 takes the lead from another word), a
covariance-matrix random walk on either stream (golden covrw5: a spherical
delta, uniform draws, odd d; test_gpu_covrw's d = 10 Gaussian one: measured
v_x 5.0e-16, v_p 4.2e-16, score 1.5e-14, no tie, accept rates 0.55 / 0.66), the
expression kernels (d = 3, a scratch-free d = 12, a d = 9 data program), the
same models in PBH_RNG_PHILOX_F64 (there also whole chains against
oracle.run_mh), chain ids straddling 2^32 and a step origin straddling 2^32.

The lane-pair and iid steady-state forms are launched only without running
moments (launch_mh_pair, iid_full_form), so those cases switch them off; the
cases that keep them also check n_acc against the trace bits.

Engine.set_step's contract is clear from pbh_engine.hip (pbh_set_step sets
e->g and leaves has_pred false; pbh_alloc_trace bases the records at that
step), so the host mirrors it: the first run step is absolute step g, it has
no predecessor, and record 0 holds it.

RTOL = 1e-12 is the project's bar.  The device normals are within 1e-14
max(1, r) of the host construction (tests/test_gpu_normals.py), r <= 8.6, and
every proposal scale here is <= 2: the proposals differ by under 2e-13.
"""
import numpy as np
import pytest

import oracle
import oracle.mh
from oracle.workloads import golden_init, _spec, _diag, _gauss, _bound

import philox_host as ph

pytestmark = pytest.mark.gpu

RTOL = 1e-12
SEED = (0x5EED1234 << 32) | 0x9ABCDEF1      # both key words in use
STD = ((1, 0), (4, 1), (56, 13))            # launches start on either step of a pair


def _rel_err(a, b, floor=np.finfo(float).tiny):
  """max |a - b| / max(|b|, floor), as tests/test_gpu_parity.py."""
  a, b = np.asarray(a, float), np.asarray(b, float)
  both_nan = np.isnan(a) & np.isnan(b)
  same = (a == b) | both_nan
  den = np.maximum(np.abs(b), floor)
  err = np.where(same, 0., np.abs(a - b) / den)
  return float(err.max()) if err.size else 0.


def _bits(a):
  return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_steps(spec, trace, r, thr, init, density=None):
  """Every recorded step of every chain against oracle.mh on the host draws
  r [T, d, N], thr [T, N].  Step t starts from the GPU's record t - 1 (init
  and "no predecessor" at t = 0).  Returns the measured figures."""
  d = int(spec['dim'])
  vx, vp = np.asarray(trace['v_x']), np.asarray(trace['v_p'])
  u = np.asarray(trace['u']).astype(bool)
  N, T = vp.shape
  assert r.shape == (T, d, N) and thr.shape == (T, N) and vx.shape == (N, T, d)
  init = np.asarray(init, np.float64).reshape(N, d)
  prev_x = np.concatenate([init[:, None, :], vx[:, :-1]], axis=1)     # [N, T, d]
  prev_p = np.concatenate([np.zeros((N, 1)), vp[:, :-1]], axis=1)     # [N, T]
  # one lane per (step, chain)
  X = np.ascontiguousarray(prev_x.transpose(2, 1, 0).reshape(d, T * N))
  LP = np.ascontiguousarray(prev_p.T.reshape(T * N))
  draws = np.ascontiguousarray(r.transpose(1, 0, 2).reshape(d, T * N))
  if spec['proposal']['kind'] == 'gauss':
    # the kernels give dim k the k-th normal; eval_delta gives draw j to dim order[j]
    draws = draws[np.asarray(spec['proposal']['order'])]
  dens = density if density is not None else (lambda x: oracle.mh.joint_prob(spec, x))
  with np.errstate(all='ignore'):
    XP = oracle.mh.apply_delta(spec, X, oracle.mh.eval_delta(spec, draws))
    LPP = np.asarray(dens(XP), np.float64)
    S, none = oracle.mh.scores(spec, LP, LPP, X, XP)
    VX = np.ascontiguousarray(vx.transpose(2, 1, 0).reshape(d, T * N))
    LPV = np.asarray(dens(VX), np.float64)        # the density at the GPU's own state
  first = np.zeros(T * N, bool)
  first[:N] = True
  none = none | first
  TH = thr.reshape(T * N)
  host = none | (S >= TH)
  gpu = u.T.reshape(T * N)
  # ---- decisions ----
  with np.errstate(all='ignore'):
    near = ~none & (np.abs(S - TH) <= RTOL * np.maximum(S, TH))
  differ = host != gpu
  wrong = differ & ~near
  ties = int(near.sum())
  print('near-ties {} (of them decided differently {}), decisions differing '
        'elsewhere {}'.format(ties, int((differ & near).sum()), int(wrong.sum())))
  assert not wrong.any(), 'decisions differ at (step, chain) {}'.format(
      [(int(i // N), int(i % N)) for i in np.flatnonzero(wrong)[:8]])
  assert ties <= 1, ties
  # ---- accepted steps ----
  acc = gpu
  e_x = _rel_err(VX[:, acc], XP[:, acc], 1.)
  e_p = _rel_err(vp.T.reshape(T * N)[acc], LPV[acc])
  print('accepted: v_x rel err {:.3g}, v_p rel err {:.3g}'.format(e_x, e_p))
  assert e_x <= RTOL, e_x
  assert e_p <= RTOL, e_p
  # ---- rejected steps: the previous record, bit for bit ----
  rej = ~gpu
  assert np.array_equal(_bits(VX[:, rej]), _bits(X[:, rej]))
  assert np.array_equal(_bits(vp.T.reshape(T * N)[rej]), _bits(LP[rej]))
  out = {'ties': ties, 'v_x': e_x, 'v_p': e_p}
  # ---- debug records (general mh_kernel only) ----
  if 'p_x' in trace:
    px = np.asarray(trace['p_x']).transpose(2, 1, 0).reshape(d, T * N)
    pp = np.asarray(trace['p_p']).T.reshape(T * N)
    e_px, e_pp = _rel_err(px, XP, 1.), _rel_err(pp, LPP)
    sc = np.asarray(trace['s']).T.reshape(T * N)
    e_s = _rel_err(sc[~none], S[~none])
    print('debug: p_x rel err {:.3g}, p_p rel err {:.3g}, s rel err {:.3g}'.format(
        e_px, e_pp, e_s))
    assert e_px <= RTOL and e_pp <= RTOL
    assert e_s <= 1e-10          # tests/test_gpu_parity.py's bar for the score
    out.update(p_x=e_px, p_p=e_pp)
  # ---- both outcomes, and the filter's interesting region ----
  rate = float(u[:, 1:].mean())
  with np.errstate(all='ignore'):
    close = float(np.mean(np.abs(LPP - LP)[N:] < 1.))
  print('accept rate {:.3f}, |lp\' - lp| < 1 at {:.3f} of the steps'.format(rate, close))
  assert 0.05 < rate < 0.95, rate
  assert close >= 0.01, close
  # ---- moments ----
  if trace.get('n_acc') is not None:
    assert np.array_equal(trace['n_acc'], u.sum(axis=1))
  return out


def _run(spec, init, mode, launches, debug=False, moments=True, chain_offset=0,
         step0=None):
  from probayes_amd import Engine
  T = sum(n for n, _ in launches)
  eng = Engine(spec)
  eng.init_chains(init, chain_offset=chain_offset)
  if step0 is not None:
    eng.set_step(step0)
  eng.set_rng(mode, seed=SEED)
  eng.set_collect(moments=moments)
  eng.alloc_trace(T, 1, debug=debug)
  for n, spl in launches:
    eng.run(n, steps_per_launch=spl)
  tr = eng.trace()
  tr['n_acc'] = eng.moments()['n_acc'] if moments else None
  eng.close()
  return tr


def _host(contract, spec, T, n, chain_offset=0, g0=0):
  d = int(spec['dim'])
  a = (SEED, d, g0, T, chain_offset, n)
  kind = spec['proposal']['kind']
  if contract == 'step':
    return ph.step_draws(*a)[:2]
  if contract == 'uniform':
    return ph.uniform_draws(*a)[:2]
  if contract == 'pair':
    return ph.pair_draws(*a)[:2]
  if contract == 'f64':
    return ph.f64_draws(*a, kind='gauss' if kind == 'gauss' else 'uniform')[:2]
  assert contract == 'f64pair'
  return ph.f64_draws(*a, pair=True)[:2]


def _norm(spec):
  from probayes_amd.spec import normalize_spec
  return normalize_spec(spec)


def _pin(spec, init, contract, launches=STD, mode='philox', density=None, **kw):
  spec = _norm(spec)
  init = np.asarray(init, np.float64)
  tr = _run(spec, init, mode, launches, **kw)
  T = sum(n for n, _ in launches)
  r, thr = _host(contract, spec, T, init.shape[0], kw.get('chain_offset', 0),
                 kw.get('step0') or 0)
  return spec, tr, r, thr, check_steps(spec, tr, r, thr, init, density)


def _spread(spec, n, seed):
  """Initial states drawn near the target (both outcomes from the start)."""
  tg = spec['target']
  rs = np.random.RandomState(seed)
  return tg['mu'] + tg['sigma'] * rs.standard_normal((n, len(tg['mu'])))


def _diag_spec(d, step=0.6):
  mu = np.linspace(-1., 1., d) if d > 1 else np.array([0.3])
  sg = np.linspace(0.5, 2., d) if d > 1 else np.array([0.8])
  return _spec(d, ['x{}'.format(i) for i in range(d)], _diag(mu, sg),
               _gauss(d, step, loc=np.linspace(-0.1, 0.1, d) if d > 1 else 0.05))


def _cfg2():
  import bench
  return bench.cfg2_spec()


# ---------------------------------------------------------------------------
# 1-3: the lane-pair kernel
# ---------------------------------------------------------------------------
def test_pair_kernel_steady_state_form():
  """bench cfg2 (zero proposal loc), 544 chains: a multiple of 32 whose last
  workgroup is partial; moments off, so every launch past step 1 is FULL."""
  spec = _norm(_cfg2())
  _pin(spec, _spread(spec, 544, 1), 'pair', moments=False)


def test_pair_kernel_general_form():
  """golden diag10 (non-zero loc), 257 chains (ragged: the general form),
  running moments on."""
  spec = oracle.golden_spec('diag10')
  _pin(spec, _spread(spec, 257, 2), 'pair')


@pytest.mark.parametrize('moments', [False, True])
@pytest.mark.parametrize('d', [4, 16])
def test_pair_kernel_ends_of_the_d_range(d, moments):
  spec = _diag_spec(d, 0.5 if d == 4 else 0.25)
  _pin(spec, _spread(spec, 96, d), 'pair', moments=moments)


# ---------------------------------------------------------------------------
# 4: cfg1's one-lane steady-state kernel
# ---------------------------------------------------------------------------
def _iid_init(n):
  init = golden_init('metrohast_norm1d', n)
  rs = np.random.RandomState(4)
  init[:, 0] += rs.uniform(-3., 3., n)
  init[:, 1] += rs.uniform(-4., 4., n)
  init[::17, 1] = 30.          # sigma outside (5, 20): density -inf until inside
  return init


def test_iid_full_kernel():
  spec = oracle.golden_spec('metrohast_norm1d')
  _pin(spec, _iid_init(101), 'uniform', moments=False)


# ---------------------------------------------------------------------------
# 5-6: the GMM kernels
# ---------------------------------------------------------------------------
def _gmm_init(n):
  return np.random.RandomState(5).normal(0., 2., size=(n, 2))


@pytest.mark.parametrize('launches', [((8, 0), (56, 0)), ((4, 0), (20, 4))])
def test_gmm_quad_steady_state_form(launches):
  """8-step groups (launches of 8 and 56 from step 8) and 4-step groups."""
  _pin(oracle.golden_spec('gmm2'), _gmm_init(72), 'step', launches=launches)


def test_gmm_quad_general_form():
  """Launches that are no whole groups: the general quad form, ragged."""
  _pin(oracle.golden_spec('gmm2'), _gmm_init(37), 'step')


def test_gmm_lane_pair_kernel(monkeypatch):
  monkeypatch.setenv('PBH_GMM_LANES', '2')
  _pin(oracle.golden_spec('gmm2'), _gmm_init(37), 'step')


# ---------------------------------------------------------------------------
# 7-8: the general mh_kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('debug', [True, False])
@pytest.mark.parametrize('d', [3, 9])
def test_mh_kernel_gaussian_proposal(d, debug):
  """Odd d: the last pair gives one normal.  debug=True records the proposal
  and takes the unfiltered score; debug=False takes the acceptance filter."""
  spec = _diag_spec(d, 0.8 if d == 3 else 0.4)
  _pin(spec, _spread(spec, 65, d), 'step', debug=debug)


def _uniform_spec(kind, d):
  """One uniform (list delta), one sphere and one bounded vardelta proposal
  (oracle.workloads' delta forms) on a diagonal Gaussian, at d = 1 and 3."""
  mu, sg = [-0.8, 0.8, 1.9][:d], [0.5, 0.5, 0.6][:d]
  bnd = _bound([-1., -1., 0.][:d], [1., 1., 2.][:d], [1, 0, 0][:d], [0, 1, 0][:d])
  if kind == 'uniform':
    prop = {'kind': 'uniform', 'delta': np.array([0.4, 0.4, 0.15][:d]), 'bound': bnd}
  elif kind == 'sphere':
    prop = {'kind': 'sphere', 'delta': 0.5, 'lengths': np.array([1., 0.8, 1.5][:d])}
  else:   # polarity, uniform, fixed (d = 1: the uniform mode alone)
    mode = [2] if d == 1 else [1, 2, 0]
    prop = {'kind': 'vardelta', 'mode': np.array(mode, np.int32),
            'delta': np.array([0.3] if d == 1 else [0.25, 0.3, 0.1]), 'bound': bnd}
  return _spec(d, ['x', 'y', 'z'][:d], _diag(mu, sg), prop)


@pytest.mark.parametrize('d', [1, 3])
@pytest.mark.parametrize('kind', ['uniform', 'sphere', 'vardelta'])
def test_mh_kernel_uniform_draws(kind, d):
  spec = _uniform_spec(kind, d)
  rs = np.random.RandomState(8 + d)
  init = np.stack([rs.uniform(-0.9, 0.9, 65), rs.uniform(-0.9, 0.9, 65),
                   rs.uniform(0.1, 1.9, 65)], 1)[:, :d]
  _pin(spec, init, 'uniform')


# ---------------------------------------------------------------------------
# 8b: a covariance-matrix random walk (proposal['tfun']) on the general mh_kernel
# ---------------------------------------------------------------------------
def _covrw_case(which):
  """covrw5: odd d, a spherical delta (uniform draws) times chol(cov).
  spec10: test_gpu_covrw's d = 10 Gaussian delta times chol(cov10); with a
  tfun it is no lane-pair form, so mh_kernel's step_draws stream feeds it."""
  if which == 'covrw5':
    return oracle.golden_spec('covrw5'), 'uniform'
  from test_gpu_covrw import _spec10
  return _spec10(), 'step'


@pytest.mark.parametrize('debug', [True, False])
@pytest.mark.parametrize('which', ['covrw5', 'spec10'])
def test_mh_kernel_covariance_random_walk(which, debug):
  """eval_delta multiplies the base delta by the tfun after check_steps'
  order line has given dim k the k-th draw, which is the kernel's order
  (apply_tfun on dl[0 .. d-1]): no further permutation is needed."""
  spec, contract = _covrw_case(which)
  spec = _norm(spec)
  _pin(spec, _spread(spec, 65, 14), contract, debug=debug)


# ---------------------------------------------------------------------------
# 9: the expression kernels
# ---------------------------------------------------------------------------
_MU12 = np.linspace(-1.5, 1.5, 12)
_SG12 = np.linspace(0.6, 1.8, 12)
_KEYS12 = ['v{}'.format(i) for i in range(12)]
_LOGC = np.log(np.sqrt(2 * np.pi))


def _gauss12(**kw):
  lsg = np.log(_SG12)
  return sum(-((kw[k] - _MU12[i]) / _SG12[i]) ** 2 / 2. - _LOGC - lsg[i]
             for i, k in enumerate(_KEYS12))


_RS9 = np.random.RandomState(90)
_X9 = _RS9.normal(0., 1.5, 9)
_OBS9 = 0.5 + 1.2 * _X9 + _RS9.normal(0., 1.5, 9)
_KEYS9 = ['a0', 'a1'] + ['w{}'.format(i) for i in range(7)]
_C9 = np.linspace(-0.5, 0.5, 7)


def _data9(**kw):
  """9 observations regressed on a0 + a1 X, and 7 further variables in a
  quadratic prior: a d = 9 program with a loop region (an instance with
  scratch)."""
  import scipy.stats
  lik = np.sum(scipy.stats.norm.logpdf(_OBS9, kw['a0'] + kw['a1'] * _X9, 1.5))
  prior = sum(-(kw['w{}'.format(i)] - _C9[i]) ** 2 / (2. * (0.5 + 0.1 * i) ** 2)
              for i in range(7))
  return lik + prior - (kw['a0'] ** 2 + kw['a1'] ** 2) / 50.


def _expr_case(which):
  import probayes_amd as pb
  from probayes_amd import expr
  if which == 'gauss3':
    from test_gpu_expr import _gauss3, _MU3, _SG3
    fn, keys, scale = _gauss3, ['x', 'y', 'z'], 0.8
    init = _MU3 + _SG3 * np.random.RandomState(9).standard_normal((65, 3))
  elif which == 'gauss12':
    fn, keys, scale = _gauss12, _KEYS12, 0.35
    init = _MU12 + _SG12 * np.random.RandomState(9).standard_normal((65, 12))
  else:
    fn, keys, scale = _data9, _KEYS9, 0.3
    init = np.random.RandomState(9).normal(0., 0.7, size=(65, 9)) + \
        np.concatenate([[0.5, 1.2], _C9])
  tg = expr.trace_expr(fn, keys)
  assert tg['kind'] == 'expr' and (tg.get('data') is not None) == (which == 'data9')
  spec = pb.make_spec(len(keys), tg, {'kind': 'gauss', 'scale': scale}, pscale='log')
  dens = lambda x: expr.evaluate(tg['code'], tg['consts'], np.ascontiguousarray(x.T),
                                 tg.get('data'))
  return spec, init, dens


@pytest.mark.parametrize('which', ['gauss3', 'gauss12', 'data9'])
def test_expression_kernels(which):
  spec, init, dens = _expr_case(which)
  _pin(spec, init, 'step', density=dens)


# ---------------------------------------------------------------------------
# 10: PBH_RNG_PHILOX_F64 -- the reference's arithmetic on libm draws
# ---------------------------------------------------------------------------
def _f64_case(which):
  if which == 'pair':
    spec = _norm(_cfg2())
    return spec, _spread(spec, 544, 1), 'f64pair', {}
  if which == 'iid':
    return oracle.golden_spec('metrohast_norm1d'), _iid_init(101), 'f64', {}
  if which == 'gmm':
    return oracle.golden_spec('gmm2'), _gmm_init(72), 'f64', {}
  spec = _diag_spec(3, 0.8)
  return spec, _spread(spec, 65, 3), 'f64', {'debug': True}


@pytest.mark.parametrize('which', ['pair', 'iid', 'gmm', 'mh3'])
def test_philox_f64_steps_and_whole_chains(which):
  spec, init, contract, kw = _f64_case(which)
  spec, tr, r, thr, _ = _pin(spec, init, contract, mode='philox_f64', **kw)
  # whole chains: the arithmetic is the reference's and the draws differ from
  # the host's by libm rounding only, so the oracle's own chain on the host
  # streams stays within RTOL over the 61 steps, with no flip
  ref = oracle.run_mh(spec, init, ph.streams(r, thr))
  flips = int(np.sum(tr['u'] != ref['u']))
  e_x, e_p = _rel_err(tr['v_x'], ref['v_x'], 1.), _rel_err(tr['v_p'], ref['v_p'])
  print('whole chains: flips {}, v_x rel err {:.3g}, v_p rel err {:.3g}'.format(
      flips, e_x, e_p))
  assert flips == 0
  assert e_x <= RTOL and e_p <= RTOL


# ---------------------------------------------------------------------------
# 11-12: chain ids and steps straddling 2^32
# ---------------------------------------------------------------------------
def _wide_case(which):
  if which == 'pair':
    spec = _norm(_cfg2())
    return spec, _spread(spec, 96, 11), 'pair', {'moments': False}
  spec = _diag_spec(3, 0.8)
  return spec, _spread(spec, 96, 12), 'step', {'debug': True}


@pytest.mark.parametrize('which', ['pair', 'mh3'])
def test_chain_ids_straddling_2_32(which):
  spec, init, contract, kw = _wide_case(which)
  _pin(spec, init, contract, chain_offset=2 ** 32 - 40, **kw)


@pytest.mark.parametrize('which', ['pair', 'mh3'])
def test_step_origin_straddling_2_32(which):
  """Engine.set_step(2^32 - 30): steps 2^32 - 30 .. 2^32 + 30 (an odd origin
  would start on a pair's second step; this one starts on its first, the
  4 one-step launches then alternate)."""
  spec, init, contract, kw = _wide_case(which)
  _pin(spec, init, contract, step0=2 ** 32 - 30, **kw)
  _pin(spec, init, contract, step0=2 ** 32 - 29, **kw)
