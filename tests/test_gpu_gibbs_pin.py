"""The production CondCov Gibbs kernel pinned step for step to a host model.

gibbs_fast_kernel's draws are a pure function of (seed, chain id, cycle-start
step, lanes per chain); tests/philox_host.py rebuilds them (gibbs_fast_draws).
check_gibbs_steps replays EVERY record of EVERY chain from the GPU's own
previous record (record 0 from the initial state), applying the thin steps in
between with the host model, so nothing accumulates.  The host model is the
reference's law as oracle/gibbs.py restates it -- the conditional mean in the
form mean_k + coef_k . (x_-k - mean_-k), accumulated in np.longdouble, the
standard normal truncated to [ndtri(cdf_lo), ndtri(cdf_hi)] -- and not the
kernel's algebra (a_k + coef_k . x, the cf table, the lane split); the CPU
tests anchor it to oracle.gibbs.run_gibbs (tests/test_philox_host.py).

Asserted per case: the truncation choice of every draw (a host normal within
1e-13 of a limit is a tie: either candidate passes; at most one tie), v_x of
Box-Muller and of inversion draws within 1e-12 max(1, |host|), untouched
coordinates bit for bit, v_p against scipy's multivariate_normal at the
permuted GPU state within 1e-9 relative (1e-9 max(1, |ref|) in log form), the
accept words all ones for exactly the N chains, n_acc == n_steps, the running
moments equal to the trace sums (thin 1), and that between 2 % and 98 % of
the draws of EVERY coordinate take the inversion.

The inversion draws' host value is ndtri by mpmath at 50 digits for the first
8 chains and scipy.special.ndtri for the others (the two agree to 1e-15 here),
at the fp64 argument lo + (hi - lo) u rounded separately or fused: a record
passes when it matches under one of the two.

The ndtri kernel gibbs_kernel (d > 16, PBH_GIBBS_FAST=0) in Philox mode is
compared as whole chains with oracle.gibbs.run_gibbs on
philox_host.gibbs_uniform_streams: its arithmetic is the reference's.  The
build instantiates d = 1..12, 16, 20, 24, 32: d = 20 is the smallest above 16
(d = 17 is not built).

Measured on the MI355X (max error of v_x at Box-Muller draws / at inversion
draws / of v_p; ties; inversion share per coordinate, least .. greatest):

  a  d 8, L 2, 37 chains, 330 steps     8.1e-16 / 5.7e-16 / 2.3e-14; 0; 8.0 .. 24.9 %
  b  L 1                                8.3e-16 / 4.4e-16 / 1.8e-14; 0; 7.9 .. 27.0 %
  b  L 4                                7.8e-16 / 5.6e-16 / 2.0e-14; 0; 8.0 .. 24.1 %
  c  d 16, L 4, 21 chains, 40 steps     6.5e-16 / 3.8e-16 / 1.4e-14; 0; 4.8 .. 34.9 %
  d  d 3, L 1, 65 chains, 40 steps      6.0e-16 / 2.4e-16 / 3.6e-15; 0; 19.2 .. 32.8 %
  e  d 1                                9.7e-16 / 2.2e-16 / 4.7e-16; 0; 62.8 %
  f  d 2, L 2, tsteps 1, 80 steps       6.1e-16 / 5.6e-16 / 1.1e-15; 0; 45.8 .. 59.6 %
  f  tsteps 2                           6.1e-16 / 5.6e-16 / 1.1e-15; 0; 46.0 .. 58.9 %
  g  d 4, L 4, tsteps 3                 6.7e-16 / 6.7e-16 / 4.4e-15; 0; 6.2 .. 19.9 %
  h  thin 3, 66 records (both forms)    7.8e-16 / 5.6e-16 / 1.4e-14; 0; 7.0 .. 24.6 %
  i  case a, log v.prob                 8.1e-16 / 5.7e-16 / 1.8e-15; 0; 8.0 .. 24.9 %
  j  chain ids across 2^32              6.7e-16 / 2.2e-16 / 1.1e-14; 0; 3.8 .. 21.1 %
  j  steps across 2^32                  6.7e-16 / 4.4e-16 / 7.2e-15; 0; 6.5 .. 24.9 %

mpmath's and scipy's ndtri differed by at most 6.2e-16 max(1, |z|) at the
inversion draws of the first 8 chains.  The separately rounded and the fused
argument differ at 3 to 8 % of the inversion draws; both fit (the library is
built with -ffp-contract=off, and an ulp of the argument moves z by under
3e-14).  gibbs_kernel's whole chains, v_x / v_p relative error over 40 steps:
d 20: 6.7e-16 / 1.4e-14; d 8 VALU form: 6.7e-16 / 1.4e-14; d 8 MFMA form:
6.7e-16 / 2.1e-14; d 2, tsteps 2: 4.4e-16 / 5.4e-15.
"""
import ctypes
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.special
import scipy.stats

import oracle
import oracle.gibbs
from oracle.mh import mvn_perm
from oracle.workloads import _gibbs, spec_gibbs_norm2d

import philox_host as ph
from test_gpu_gibbs_fast import _spec_d
from test_gpu_philox_pin import SEED, RTOL, _rel_err, _bits

pytestmark = pytest.mark.gpu

LD = np.longdouble
TIE = 1e-13          # ten times test_gpu_normals' 1e-14 max(1, r), r = O(1) at a limit
X_BAR = 1e-12        # v_x: |gpu - host| <= X_BAR max(1, |host|)
P_BAR = 1e-9         # v_p: test_vprob_is_the_permuted_mvn_pdf's bar
MP_CHAINS = 8        # chains whose inversion draws take mpmath's ndtri
A_LAUNCHES = (13, 1, 8, 3, 300, 5)


# ---------------------------------------------------------------------------
# the host model
# ---------------------------------------------------------------------------
def tables(spec):
  """cond_cov.py's tables (oracle.gibbs.condcov_tables) and the z limits."""
  p = spec['proposal']
  d = int(spec['dim'])
  coef, stdv, cdfs = oracle.gibbs.condcov_tables(p['mean'], p['cov'], p['lo'], p['hi'])
  coef = np.array([np.asarray(c, np.float64).reshape(-1) for c in coef]).reshape(d, d - 1)
  zl = scipy.special.ndtri(cdfs)
  ts = int(p.get('tsteps', 1))
  return SimpleNamespace(d=d, mean=np.asarray(p['mean'], np.float64), coef=coef,
                         stdv=stdv, cdfs=cdfs, zlo=zl[:, 0], zhi=zl[:, 1], ts=ts,
                         nblk=-(-d // ts))


def step_coords(tb, g):
  cm = (int(g) % tb.nblk) * tb.ts
  return range(cm, min(tb.d, cm + tb.ts))


def _fma(a, b, c):
  """a b + c with one rounding."""
  return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def ndtri_mp(p):
  import mpmath
  with mpmath.workdps(50):
    return float(mpmath.sqrt(2) * mpmath.erfinv(2 * mpmath.mpf(float(p)) - 1))


def host_draws(tb, L, g0, T, chain_offset, N, seed=SEED, mp_chains=MP_CHAINS):
  """The draws of steps g0 .. g0 + T - 1 ([T, d, N] arrays): the normals z,
  whether each lies inside its limits, whether it ties with one, and the
  inversion normals zi (separately rounded argument) and zi_f (fused).  The
  inversion normals are exact only where a step uses them."""
  d = tb.d
  z, u = ph.gibbs_fast_draws(seed, d, L, tb.ts, g0, T, chain_offset, N)
  zlo, zhi = tb.zlo[None, :, None], tb.zhi[None, :, None]
  lo, hi = tb.cdfs[None, :, 0, None], tb.cdfs[None, :, 1, None]
  inside = (z >= zlo) & (z <= zhi)
  tie = (np.abs(z - zlo) <= TIE) | (np.abs(z - zhi) <= TIE)
  used = np.zeros((T, d, 1), bool)
  for t in range(T):
    used[t, list(step_coords(tb, int(g0) + t))] = True
  wid = np.broadcast_to(hi - lo, u.shape)
  arg = lo + wid * u
  arg_f = arg.copy()
  need = (~inside | tie) & used
  los = np.broadcast_to(lo, u.shape)
  for i in zip(*np.nonzero(need)):
    arg_f[i] = _fma(wid[i], u[i], los[i])
  zi, zi_f = scipy.special.ndtri(arg), scipy.special.ndtri(arg_f)
  mp_err = 0.
  for i in zip(*np.nonzero(need[:, :, :mp_chains])):
    for a, out in ((arg, zi), (arg_f, zi_f)):
      v = ndtri_mp(a[i])
      mp_err = max(mp_err, abs(v - out[i]) / max(1., abs(v)))
      out[i] = v
  return SimpleNamespace(z=z, u=u, inside=inside, tie=tie & used, used=used, zi=zi,
                         zi_f=zi_f, n_fused=int((arg != arg_f).sum()), mp_err=mp_err)


def cond_mean(tb, x, k):
  """mean_k + coef_k . (x_-k - mean_-k) of the rows of x [N, d] (longdouble)."""
  acc = np.zeros(x.shape[0], LD)
  for i in range(tb.d):
    if i != k:
      acc = acc + LD(tb.coef[k, i if i < k else i - 1]) * (x[:, i] - LD(tb.mean[i]))
  return LD(tb.mean[k]) + acc


def advance(tb, dr, x, t, g, flip=False, fused=False):
  """Step g (row t of the draws) on the states x [N, d] (longdouble, changed
  in place).  Returns [(k, took the inversion [N], the other candidate [N])]."""
  out = []
  zi = dr.zi_f if fused else dr.zi
  for k in step_coords(tb, g):
    inv = ~dr.inside[t, k]
    if flip:
      inv = inv ^ dr.tie[t, k]
    m = cond_mean(tb, x, k)
    x_bm = (m + LD(tb.stdv[k]) * dr.z[t, k]).astype(np.float64)
    x_inv = (m + LD(tb.stdv[k]) * zi[t, k]).astype(np.float64)
    x[:, k] = np.where(inv, x_inv, x_bm)
    out.append((k, inv, np.where(inv, x_bm, x_inv)))
  return out


def host_chain(spec, L, init, T, g0=0, chain_offset=0, seed=SEED):
  """Whole chains by the host model: (v_x [N, T, d], the uniforms [T, tsteps,
  N] on which oracle.gibbs.run_gibbs makes the same chains, inversion draws)."""
  tb = tables(spec)
  init = np.asarray(init, np.float64).reshape(-1, tb.d)
  N = init.shape[0]
  dr = host_draws(tb, L, g0, T, chain_offset, N, seed)
  x = init.astype(LD)
  vx = np.empty((N, T, tb.d))
  streams = np.zeros((T, tb.ts, N))
  n_inv = 0
  for t in range(T):
    for j, (k, inv, _) in enumerate(advance(tb, dr, x, t, int(g0) + t)):
      lo, hi = tb.cdfs[k]
      streams[t, j] = np.where(inv, dr.u[t, k],
                               (scipy.special.ndtr(dr.z[t, k]) - lo) / (hi - lo))
      n_inv += int(inv.sum())
    vx[:, t] = x.astype(np.float64)
  return vx, streams, n_inv


def _mvn_ref(spec, vx):
  d = int(spec['dim'])
  mvn = scipy.stats.multivariate_normal(np.asarray(spec['target']['mean']),
                                        np.asarray(spec['target']['cov']))
  x = np.asarray(vx).reshape(-1, d)[:, mvn_perm(d)]
  f = mvn.logpdf if spec['pscale'] == 'log' else mvn.pdf
  return np.asarray(f(x), np.float64).reshape(np.asarray(vx).shape[:-1])


def host_trace(spec, L, init, T, **kw):
  """The host chain as a trace check_gibbs_steps takes (the checker's own test)."""
  vx, _, _ = host_chain(spec, L, init, T, **kw)
  N = vx.shape[0]
  full = (1 << 64) - 1
  words = [full] * (N // 64) + ([(1 << (N % 64)) - 1] if N % 64 else [])
  return {'v_x': vx, 'v_p': _mvn_ref(spec, vx), 'u': np.ones((N, T), np.uint8),
          'acc_words': np.tile(np.array(words, np.uint64), (T, 1)),
          'moments': {'sum': vx.sum(axis=1), 'n_acc': np.full(N, T), 'n_steps': T}}


# ---------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------
def check_gibbs_steps(spec, trace, L, init, thin=1, g0=0, chain_offset=0):
  """Every record of every chain against the host model from the GPU's own
  previous record.  Returns the measured figures."""
  tb = tables(spec)
  d = tb.d
  vx, vp = np.asarray(trace['v_x']), np.asarray(trace['v_p'])
  N, R = vp.shape
  assert vx.shape == (N, R, d) and int(g0) % thin == 0
  init = np.asarray(init, np.float64).reshape(N, d)
  prev = np.concatenate([init[:, None, :], vx[:, :-1]], axis=1)
  T = R * thin
  dr = host_draws(tb, L, g0, T, chain_offset, N)
  ties = int(dr.tie.sum())
  print('ties {} of {} draws; fused argument differs at {} inversion draws; '
        'mpmath vs scipy ndtri {:.3g}'.format(ties, int(dr.used.sum()) * N, dr.n_fused,
                                             dr.mp_err))
  assert ties <= 1, ties

  variants = [(f, fu) for f in ((False, True) if ties else (False,)) for fu in (False, True)]
  hosts, alts = [], []
  cls = np.zeros((N, R, d), np.int8)       # 0 untouched, 1 Box-Muller, 2 inversion
  tied = np.zeros((N, R, d), bool)
  for vi, (flip, fused) in enumerate(variants):
    host, alt = np.empty((N, R, d)), np.full((N, R, d), np.nan)
    for r in range(R):
      x = prev[:, r].astype(LD)
      for s in range(thin):
        t = r * thin + s
        for k, inv, other in advance(tb, dr, x, t, int(g0) + t, flip, fused):
          alt[:, r, k] = other
          if vi == 0:
            cls[:, r, k] = np.where(inv, 2, 1)
            tied[:, r, k] |= dr.tie[t, k]
      host[:, r] = x.astype(np.float64)
    hosts.append(host)
    alts.append(alt)
  hosts, alts = np.array(hosts), np.array(alts)
  err_v = np.abs(vx[None] - hosts) / np.maximum(1., np.abs(hosts))      # [V, N, R, d]
  best = np.argmin(err_v.max(axis=3), axis=0)                            # [N, R]
  pick = lambda a: np.take_along_axis(a, best[None, :, :, None], axis=0)[0]
  err, host, alt = pick(err_v), pick(hosts), pick(alts)
  upd = cls > 0

  # ---- the truncation choice ----
  with np.errstate(invalid='ignore'):
    other = upd & (np.abs(vx - alt) < np.abs(vx - host)) & ~tied
  assert not other.any(), 'the other candidate was taken at (chain, record, k) {}'.format(
      [tuple(int(v) for v in i) for i in np.argwhere(other)[:8]])
  # ---- v_x ----
  e_bm = float(err[cls == 1].max()) if (cls == 1).any() else 0.
  e_inv = float(err[cls == 2].max()) if (cls == 2).any() else 0.
  share = np.array([(cls[:, :, k] == 2).sum() / max(1, upd[:, :, k].sum()) for k in range(d)])
  print('v_x err: Box-Muller draws {:.3g}, inversion draws {:.3g} (fused argument fits '
        'best at {} records); inversion share per coordinate {:.3f} .. {:.3f}'.format(
            e_bm, e_inv, int((best % 2 == 1).sum()), share.min(), share.max()))
  assert e_bm <= X_BAR, e_bm
  assert e_inv <= X_BAR, e_inv
  # ---- untouched coordinates: the previous record, bit for bit ----
  assert np.array_equal(_bits(vx[~upd]), _bits(prev[~upd]))
  # ---- v_p at the GPU's own state ----
  ref = _mvn_ref(spec, vx)
  den = np.maximum(1., np.abs(ref)) if spec['pscale'] == 'log' else np.abs(ref)
  e_p = float(np.max(np.abs(vp - ref) / den))
  print('v_p err {:.3g}'.format(e_p))
  assert e_p <= P_BAR, e_p
  # ---- u: all ones for exactly the N chains ----
  assert np.asarray(trace['u']).shape == (N, R) and np.asarray(trace['u']).all()
  if trace.get('acc_words') is not None:
    full = (1 << 64) - 1
    want = [full] * (N // 64) + ([(1 << (N % 64)) - 1] if N % 64 else [])
    assert np.array_equal(np.asarray(trace['acc_words'], np.uint64),
                          np.tile(np.array(want, np.uint64), (R, 1)))
  # ---- running moments ----
  mom = trace.get('moments')
  if mom is not None:
    assert mom['n_steps'] == T and np.array_equal(mom['n_acc'], np.full(N, T))
    if thin == 1:
      np.testing.assert_allclose(mom['sum'], vx.sum(axis=1), rtol=1e-12, atol=1e-9)
  # ---- coverage: both branches in every coordinate ----
  assert upd.any(axis=(0, 1)).all()
  assert share.min() >= 0.02 and share.max() <= 0.98, share
  return {'ties': ties, 'v_x_bm': e_bm, 'v_x_inv': e_inv, 'v_p': e_p,
          'share': (float(share.min()), float(share.max()))}


# ---------------------------------------------------------------------------
# running the engine
# ---------------------------------------------------------------------------
def _acc_words(eng, count):
  """The records' raw accept words [count, W] (Engine.trace unpacks only the
  first n bits)."""
  from probayes_amd import _lib
  from probayes_amd.engine import _dp
  n, d = eng.n, eng.dim
  x, lp = np.empty((count, d, n)), np.empty((count, n))
  acc = np.empty((count, (n + 63) // 64), np.uint64)
  nul = ctypes.POINTER(ctypes.c_double)()
  _lib.call('pbh_get_trace', eng._h, ctypes.c_int64(0), ctypes.c_int64(count), _dp(x),
            _dp(lp), acc.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), nul, nul, nul)
  return acc


def _run(spec, init, launches, thin=1, moments=True, chain_offset=0, step0=None):
  from probayes_amd import Engine
  T = sum(launches)
  assert T % thin == 0
  eng = Engine(spec)
  eng.init_chains(init, chain_offset=chain_offset)
  if step0 is not None:
    eng.set_step(step0)
  eng.set_rng('philox', seed=SEED)
  eng.set_collect(moments=moments)
  eng.alloc_trace(T // thin, thin)
  for n in launches:
    eng.run(n)
  tr = eng.trace()
  tr['acc_words'] = _acc_words(eng, T // thin)
  tr['moments'] = eng.moments() if moments else None
  eng.close()
  return tr


def _init(spec, n, seed):
  """Initial states spread about the mean, inside the limits."""
  p = spec['proposal']
  rs = np.random.RandomState(seed)
  x = p['mean'] + 0.4 * rs.standard_normal((n, int(spec['dim'])))
  return np.clip(x, p['lo'] + 0.05, p['hi'] - 0.05)


def _pin(spec, n, launches, monkeypatch, lanes=None, **kw):
  from probayes_amd.spec import normalize_spec
  spec = normalize_spec(spec)
  d = int(spec['dim'])
  monkeypatch.setenv('PBH_GIBBS_FAST', '1')
  if lanes is None:
    monkeypatch.delenv('PBH_GIBBS_LANES', raising=False)
    L = ph.gibbs_lanes(d, {})
  else:
    monkeypatch.setenv('PBH_GIBBS_LANES', str(lanes))
    L = ph.gibbs_lanes(d, {'PBH_GIBBS_LANES': str(lanes)})
    assert L == lanes
  init = _init(spec, n, d)
  tr = _run(spec, init, launches, **kw)
  return check_gibbs_steps(spec, tr, L, init, thin=kw.get('thin', 1),
                           g0=kw.get('step0') or 0,
                           chain_offset=kw.get('chain_offset', 0))


def _norm2d(lo, hi, tsteps):
  g = spec_gibbs_norm2d({})['proposal']      # examples/mcmc/gibbs_norm2d.py's model
  spec = _gibbs(g['mean'], g['cov'], lo, hi, ['x', 'y'])
  spec['proposal']['tsteps'] = tsteps
  return spec


# ---------------------------------------------------------------------------
# gibbs_fast_kernel
# ---------------------------------------------------------------------------
def test_a_d8_two_lanes_every_launch_form(monkeypatch):
  """37 chains (the second 32-chain wavefront is ragged); launches that leave
  and enter mid-cycle, whole pipelined cycles, a launch shorter than a cycle,
  and cycle 32 (step 256, the exact refresh of g and Q) inside a launch."""
  assert ph.gibbs_lanes(8, {}) == 2
  _pin(_spec_d(8, 7, -1.5, 2.), 37, A_LAUNCHES, monkeypatch)


@pytest.mark.parametrize('lanes', [1, 4])
def test_b_d8_other_lane_layouts(lanes, monkeypatch):
  _pin(_spec_d(8, 7, -1.5, 2.), 37, A_LAUNCHES, monkeypatch, lanes=lanes)


def test_c_d16_four_lanes_16_bit_accept_words(monkeypatch):
  """21 chains: the second 16-chain wavefront is ragged.  The first launch
  ends mid-cycle, the second continues.  Limits -1.5, 1.5: at -2, 2 one
  coordinate's inversion probability is 1.96 %, and of the 42 to 63 draws a
  coordinate gets here three coordinates have none outside their limits, so
  the coverage bar could not hold; here the probabilities are 8 % to 30 %."""
  assert ph.gibbs_lanes(16, {}) == 4
  _pin(_spec_d(16, 7, -1.5, 1.5), 21, (21, 19), monkeypatch)


def test_d_d3_one_lane(monkeypatch):
  """Odd d: one lane per chain, post() without pairing, odd M."""
  _pin(_spec_d(3, 7, -1., 1.5), 65, (40,), monkeypatch)


def test_e_d1_no_coef(monkeypatch):
  _pin(_spec_d(1, 7, -0.6, 1.2), 65, (40,), monkeypatch)


@pytest.mark.parametrize('tsteps', [1, 2])
def test_f_d2_two_lanes(tsteps, monkeypatch):
  """tsteps = 2: a cycle is one step, cycle 32 is step 32."""
  _pin(_norm2d(-0.5, 1., tsteps), 65, (80,), monkeypatch)


def test_g_d4_four_lanes_short_last_block(monkeypatch):
  spec = _spec_d(4, 7, -1.5, 2.)
  spec['proposal']['tsteps'] = 3
  _pin(spec, 65, (5, 35), monkeypatch, lanes=4)


@pytest.mark.parametrize('moments', [True, False])
def test_h_thinning(moments, monkeypatch):
  """66 records of every third step."""
  _pin(_spec_d(8, 7, -1.5, 2.), 37, (13, 1, 8, 3, 173), monkeypatch, thin=3,
       moments=moments)


def test_i_log_pscale(monkeypatch):
  spec = _spec_d(8, 7, -1.5, 2.)
  spec['pscale'] = 'log'
  _pin(spec, 37, A_LAUNCHES, monkeypatch)


@pytest.mark.parametrize('which', ['chains', 'steps'])
def test_j_chain_ids_and_steps_across_2_32(which, monkeypatch):
  """Chain ids 2^32 - 20 .. 2^32 + 16; steps from 2^32 - 13, a mid-cycle
  origin (coordinate 3) whose cycle starts below 2^32, with rec_base."""
  kw = {'chain_offset': 2 ** 32 - 20} if which == 'chains' else {'step0': 2 ** 32 - 13}
  _pin(_spec_d(8, 7, -1.5, 2.), 37, (13, 1, 8, 3, 15), monkeypatch, lanes=2, **kw)


# ---------------------------------------------------------------------------
# gibbs_kernel under Philox: whole chains against the oracle
# ---------------------------------------------------------------------------
def _whole(spec, monkeypatch, fast, mfma):
  from probayes_amd import Engine
  from probayes_amd.spec import normalize_spec
  spec = normalize_spec(spec)
  d, ts = int(spec['dim']), int(spec['proposal']['tsteps'])
  n, t = 65, 40
  monkeypatch.setenv('PBH_GIBBS_FAST', '1' if fast else '0')
  monkeypatch.setenv('PBH_GIBBS_MFMA', '1' if mfma else '0')
  init = _init(spec, n, 30 + d)
  eng = Engine(spec)
  eng.init_chains(init)
  eng.set_rng('philox', seed=SEED)
  eng.alloc_trace(t, 1)
  eng.run(t)
  tr = eng.trace()
  eng.close()
  ref = oracle.gibbs.run_gibbs(spec, init, ph.gibbs_uniform_streams(SEED, d, ts, 0, t, 0, n))
  e_x, e_p = _rel_err(tr['v_x'], ref['v_x'], 1.), _rel_err(tr['v_p'], ref['v_p'])
  print('whole chains: v_x rel err {:.3g}, v_p rel err {:.3g}'.format(e_x, e_p))
  assert e_x <= RTOL, e_x
  assert e_p <= RTOL, e_p
  assert tr['u'].all()


def test_ndtri_kernel_d20(monkeypatch):
  """d = 20, the smallest d above 16 the build instantiates: the production
  kernel does not take it whatever PBH_GIBBS_FAST says."""
  _whole(_spec_d(20, 7), monkeypatch, True, True)


@pytest.mark.parametrize('mfma', [0, 1])
def test_ndtri_kernel_d8(mfma, monkeypatch):
  _whole(_spec_d(8, 7), monkeypatch, False, bool(mfma))


def test_ndtri_kernel_d2_sweep(monkeypatch):
  _whole(_norm2d(-20., 20., 2), monkeypatch, False, True)
