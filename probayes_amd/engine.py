"""Engine: a spec (probayes_amd/spec.py) bound to one libpbhip engine/device.

Host-side precompute mirrors what the reference evaluates with NumPy/SciPy
once per model, so the device sees bit-identical constants:
  * log(scale) of every Normal (scipy norm.logpdf, _distn_infrastructure.py);
  * the mvn whitening matrix, log_pdet and rank of scipy's CovViaPSD
    (prob.py:349-358 -> multivariate_normal.pdf);
  * the CondCov tables coef / stdv / cdf limits (cond_cov.py:22-39).
Everything per chain-step runs in the HIP kernels; nothing here loops over
chains or steps.
"""
import atexit
import ctypes
import weakref

import numpy as np
import scipy.stats

from probayes_amd import _lib
from probayes_amd.spec import normalize_spec

_c = ctypes


def _dp(a):
  return a.ctypes.data_as(_c.POINTER(_c.c_double))


def _ip(a):
  return a.ctypes.data_as(_c.POINTER(_c.c_int32))


def _f64(a):
  return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
  return np.ascontiguousarray(a, dtype=np.int32)


def _quantiles(q):
  """q as the C-ABI takes it: (a contiguous float64 array, nq).  An empty q
  is (one zero nobody reads, 0): the library refuses nq = 0 itself."""
  qs = np.ascontiguousarray(np.atleast_1d(np.asarray(q, float)).ravel())
  return (qs, qs.size) if qs.size else (np.zeros(1), 0)


def condcov_tables(mean, cov, lo, hi):
  """CondCov.__init__ (cond_cov.py:22-39): per coordinate i the regression
  row Sigma_{i,-i} Sigma_{-i,-i}^{-1}, the Schur sd and the cdf limits of the
  bounds recentred on the unconditional mean (App. A-5)."""
  mean = np.atleast_1d(_f64(mean))
  cov = np.atleast_2d(_f64(cov))
  n = len(mean)
  lims = np.stack([_f64(lo), _f64(hi)], -1) - np.expand_dims(mean, -1)
  stdv = np.empty(n)
  coef = np.zeros((n, max(n - 1, 0)))
  for i in range(n):
    ll = np.delete(cov[:, i].reshape([n, 1]), i, axis=0)
    ru = np.delete(cov[i, :].reshape([1, n]), i, axis=1)
    sub = np.delete(np.delete(cov, i, axis=1), i, axis=0)
    row = ru.dot(np.linalg.inv(sub))
    coef[i] = row.reshape(-1)
    stdv[i] = np.sqrt(cov[i, i] - row.dot(ll).item())
  cdfs = np.array([scipy.stats.norm.cdf(lim, loc=0., scale=stdv[i])
                   for i, lim in enumerate(lims)])
  return coef, stdv, cdfs


def mvn_psd(mean, cov):
  """scipy multivariate_normal's CovViaPSD: (whitening U, rank*log(2pi) +
  log_pdet) exactly as scipy forms them (_multivariate.py _logpdf)."""
  mvn = scipy.stats.multivariate_normal(_f64(mean), _f64(cov))
  co = mvn.cov_object
  const = co.rank * np.log(2 * np.pi) + co.log_pdet
  return _f64(co._LP), float(const)


def eval_expr(code, consts, depth, x, device=0, data=None):
  """pbh_eval_expr: the expr program at the points x [n, d] with the
  kernels' own device function (diagnostic; probayes_amd.expr.evaluate is
  the NumPy definition).  data [C, n_obs]: a program with loop regions, through
  pbh_eval_expr_data (the interpreter of the data kernels)."""
  x = np.ascontiguousarray(np.atleast_2d(x), np.float64)
  n, d = x.shape
  code, consts = _i32(code).reshape(-1), _f64(consts).reshape(-1)
  out = np.empty(n)
  if data is not None:
    data = np.ascontiguousarray(np.atleast_2d(_f64(data)))
    _lib.call('pbh_eval_expr_data', int(device), d, _ip(code), len(code),
              _dp(consts), len(consts), int(depth), _dp(data), data.shape[0],
              data.shape[1], n, _dp(x), _dp(out))
    return out
  _lib.call('pbh_eval_expr', int(device), d, _ip(code), len(code), _dp(consts),
            len(consts), int(depth), n, _dp(x), _dp(out))
  return out


def unpack_stats(out, counts, d):
  """[world][3d+1][n_max] gather block (pbh_rccl_allgather_stats) -> the
  per-chain statistics of all ranks concatenated in rank (= global chain)
  order, padding columns dropped."""
  cols = [out[r, :, :counts[r]] for r in range(len(counts))]
  a = np.concatenate(cols, axis=1) if cols else np.empty((3 * d + 1, 0))
  return {'sum': a[:d].T.copy(), 'sumsq': a[d:2 * d].T.copy(),
          'n_acc': a[2 * d].astype(np.int64), 'ess': a[2 * d + 1:].T.copy(),
          'counts': np.asarray(counts, np.int64)}


# engines still open at interpreter exit are destroyed then (a resident
# sampling server is stopped and its chain state stored: no kernel outlives
# the process's last Python code)
_LIVE = weakref.WeakSet()


@atexit.register
def _close_live_engines():
  for eng in list(_LIVE):
    try:
      eng.close()
    except Exception:
      pass


def unpack_accept(acc, n):
  """Accept words [T, W] (uint64, bit c % 64 of word c // 64 = chain c) as
  u [N, T] uint8, C-contiguous.  The words are transposed first ([W, T]: 8
  bytes per 64 chains and record) and then unpacked along the chain axis --
  transposing the unpacked [T, N] bytes instead took ~2.8 s at 65 536 chains
  x 1 000 records (a strided read per byte)."""
  acc = np.ascontiguousarray(acc, np.uint64)
  count, W = acc.shape
  by = np.ascontiguousarray(
      np.ascontiguousarray(acc.T).view(np.uint8).reshape(W, count, 8).transpose(0, 2, 1))
  return np.unpackbits(by, axis=1, bitorder='little').reshape(W * 64, count)[:n]


class Engine:
  """One libpbhip engine on one device, running one lowered model."""

  def __init__(self, spec, device=0):
    self.spec = normalize_spec(spec)
    self.dim = self.spec['dim']
    self._h = _c.c_void_p()
    _lib.call('pbh_create', int(device), _c.byref(self._h))
    # the hot entry points, bound once (the timed run is two calls: a
    # getattr and c_int64 boxing per call were ~1 us of a 20-step run's ~35)
    lib = _lib.load()
    self._fn_run, self._fn_sync = lib.pbh_run, lib.pbh_sync
    self._fn_run_wait = lib.pbh_run_wait
    _LIVE.add(self)
    self.device = device
    self.n = 0
    self.chain_offset = 0
    self._rng = 'philox'
    self._set_model()
    if self.spec['proposal']['kind'] == 'gibbs':
      self._set_gibbs()
    else:
      self._set_proposal()

  # ---- model -------------------------------------------------------------
  def _set_model(self):
    s, d = self.spec, self.dim
    tg = s['target']
    m = _lib.PbhModel()
    m.dim = d
    m.target_kind = _lib.TARGET[tg['kind']]
    m.pscale = _lib.PSCALE[s['pscale']]
    m.scores = _lib.SCORES[s['scores']]
    keep = []

    def arr(a, conv=_f64):
      a = conv(a)
      keep.append(a)
      return a

    kind = tg['kind']
    if kind == 'diag_gauss':
      m.a, m.b = _dp(arr(tg['mu'])), _dp(arr(tg['sigma']))
      m.c = _dp(arr(np.log(_f64(tg['sigma']))))
      m.e = _dp(arr(1.0 / _f64(tg['sigma'])))
    elif kind == 'norm_iid':
      m.a = _dp(arr(tg['obs']))
      m.n = len(tg['obs'])
      m.i0, m.i1 = tg['loc'], tg['scale']
    elif kind == 'gmm':
      m.a, m.b = _dp(arr(tg['logw'])), _dp(arr(tg['mu']))
      m.c, m.e = _dp(arr(tg['sd'])), _dp(arr(np.log(_f64(tg['sd']))))
      m.n = len(tg['logw'])
    elif kind in ('norm_pdf',):
      m.a, m.b = _dp(arr(tg['loc'])), _dp(arr(tg['scale']))
    elif kind == 'uniform_pdf':
      m.a, m.b = _dp(arr(tg['lo'])), _dp(arr(tg['scale']))
    elif kind == 'mvn':
      U, const = mvn_psd(tg['mean'], tg['cov'])
      m.a, m.b = _dp(arr(tg['mean'])), _dp(arr(U))
      m.c = _dp(arr(np.array([const])))
    elif kind == 'expr':
      m.expr_code = _ip(arr(tg['code'], _i32))
      m.expr_n_code = len(tg['code'])
      m.expr_consts = _dp(arr(tg['consts']))
      m.expr_n_consts = len(tg['consts'])
      m.expr_depth = tg['depth']
      if tg.get('data') is not None:     # [C, n]: the loop regions' columns
        m.expr_data = _dp(arr(tg['data']))
        m.expr_n_cols, m.expr_n_obs = tg['data'].shape
    pr = s['prior']
    if pr is not None:
      m.has_prior = 1
      m.prior_lo, m.prior_hi = _dp(arr(pr['lo'])), _dp(arr(pr['hi']))
      m.prior_lo_incl = _ip(arr(pr['lo_incl'], _i32))
      m.prior_hi_incl = _ip(arr(pr['hi_incl'], _i32))
      m.prior_logp = pr['logp']
    m.ufun = _ip(arr(s['ufun'], _i32))
    tr = s['tran']
    m.tran_kind = _lib.TRAN[tr['kind']]
    m.tran_sym = 1 if tr['sym'] else 0
    if tr['kind'] == 'const':
      m.tran_value = tr['value']
    else:
      m.tran_scale = tr['scale']
      m.tran_offset = _dp(arr(tr['offset']))
      m.tran_order = _ip(arr(tr['order'], _i32))
    _lib.call('pbh_set_model', self._h, _c.byref(m))

  def _set_proposal(self):
    p, d = self.spec['proposal'], self.dim
    q = _lib.PbhProposal()
    q.kind = _lib.PROPOSAL[p['kind']]
    keep = []

    def arr(a, conv=_f64):
      a = conv(a)
      keep.append(a)
      return a

    if p['kind'] == 'gauss':
      q.loc, q.scale = _dp(arr(p['loc'])), _dp(arr(p['scale']))
      q.order = _ip(arr(p['order'], _i32))
    elif p['kind'] == 'sphere':
      q.delta = p['delta']
      q.lengths = _dp(arr(p['lengths']))
    elif p['kind'] == 'uniform':
      q.delta_vec = _dp(arr(p['delta']))
    elif p['kind'] == 'vardelta':
      q.delta_vec = _dp(arr(p['delta']))
      q.var_mode = _ip(arr(p['mode'], _i32))
    if p.get('vint') is not None:
      q.var_int = _ip(arr(p['vint'], _i32))
    b = p.get('bound')
    if b is not None:
      q.bound_on = _ip(arr(b['on'], _i32))
      q.bound_lo, q.bound_hi = _dp(arr(b['lo'])), _dp(arr(b['hi']))
      q.bound_xlo = _ip(arr(b['xlo'], _i32))
      q.bound_xhi = _ip(arr(b['xhi'], _i32))
    if p.get('tfun') is not None:
      q.tfun = _dp(arr(np.ascontiguousarray(p['tfun'], np.float64)))
    _lib.call('pbh_set_proposal', self._h, _c.byref(q))

  def _set_gibbs(self):
    p = self.spec['proposal']
    coef, stdv, cdfs = condcov_tables(p['mean'], p['cov'], p['lo'], p['hi'])
    keep = [_f64(p['mean']), _f64(coef), _f64(stdv), _f64(cdfs)]
    g = _lib.PbhGibbs()
    g.mean, g.coef, g.stdv, g.cdf = [_dp(a) for a in keep]
    g.tsteps = p['tsteps']
    _lib.call('pbh_set_gibbs', self._h, _c.byref(g))

  # ---- chains / randomness -------------------------------------------------
  def init_chains(self, init, chain_offset=0):
    """init [N, d] (or [d] broadcast to n chains via init_like)."""
    init = _f64(init).reshape(-1, self.dim)
    self.n = init.shape[0]
    _lib.call('pbh_init_chains', self._h, _c.c_int64(self.n),
              _c.c_int64(int(chain_offset)), _dp(init))
    self.chain_offset = int(chain_offset)

  def set_step(self, step):
    """Global step index of the first run step (the CondCov cycle phase,
    rf.py:446-452); right after init_chains."""
    _lib.call('pbh_set_step', self._h, _c.c_int64(int(step)))

  def set_rng(self, mode='philox', seed=0):
    _lib.call('pbh_set_rng', self._h, _lib.RNG[mode],
              _c.c_uint64(int(seed) & (2 ** 64 - 1)))
    self._rng = mode

  def stream_width(self):
    r = _c.c_int32()
    _lib.call('pbh_stream_width', self._h, _c.byref(r))
    return r.value

  def upload_replay(self, streams):
    """streams [T, R, N] in the reference's per-step consumption order."""
    streams = _f64(streams)
    T, R, N = streams.shape
    if N != self.n or R != self.stream_width():
      raise ValueError('replay stream shape {} does not match R={}, N={}'
                       .format(streams.shape, self.stream_width(), self.n))
    _lib.call('pbh_upload_replay', self._h, _c.c_int64(T), _dp(streams))

  def seed_legacy(self, seeds):
    """One NumPy legacy RandomState(seeds[c]) per chain, on the device."""
    seeds = np.ascontiguousarray(np.asarray(seeds).reshape(-1), dtype=np.int64)
    if seeds.size != self.n:
      raise ValueError('need {} seeds, got {}'.format(self.n, seeds.size))
    if np.any(seeds < 0) or np.any(seeds > 0xFFFFFFFF):
      raise ValueError('Seed must be between 0 and 2**32 - 1')
    s32 = np.ascontiguousarray(seeds.astype(np.uint32))
    _lib.call('pbh_legacy_seed', self._h,
              s32.ctypes.data_as(_c.POINTER(_c.c_uint32)))

  def legacy_replay(self, n_steps):
    """Fills the replay stream with the next n_steps rows of every chain's
    device RandomState (the reference's per-step draw order)."""
    _lib.call('pbh_legacy_replay', self._h, _c.c_int64(int(n_steps)))

  def reserve_replay(self, n_steps):
    """Sizes the replay stream buffer for n_steps rows (draws nothing): a
    later legacy_replay / upload_replay of at most that many rows allocates
    nothing.  Call it before filling the buffer."""
    _lib.call('pbh_reserve_replay', self._h, _c.c_int64(int(n_steps)))

  def get_replay(self, first, n_steps, draw=-1):
    """Rows of the current replay stream: [n, R, N], or [n, N] of one draw."""
    r = self.stream_width()
    shape = (n_steps, r, self.n) if draw < 0 else (n_steps, self.n)
    out = np.empty(shape, np.float64)
    _lib.call('pbh_get_replay', self._h, _c.c_int64(int(first)),
              _c.c_int64(int(n_steps)), int(draw), _dp(out))
    return out

  # ---- running -----------------------------------------------------------
  def alloc_trace(self, capacity, thin=1, debug=False, fill=True):
    """fill=False: no zero fill of the records (the next run writes every
    one of them: PBH_TRACE_NOFILL)."""
    flags = (1 if debug else 0) | (0 if fill else 0x100)
    _lib.call('pbh_alloc_trace', self._h, _c.c_int64(int(capacity)),
              int(thin), flags)
    self.debug = bool(debug)

  def run(self, n_steps, steps_per_launch=0, sync=True):
    # sync: one library call (pbh_run_wait) instead of pbh_run + pbh_sync
    fn = self._fn_run_wait if sync else self._fn_run
    rc = fn(self._h, int(n_steps), int(steps_per_launch))
    if rc:
      _lib.raise_status('pbh_run_wait' if sync else 'pbh_run', rc)

  def legacy_run(self, n_steps, steps_per_launch=0, sync=True):
    """legacy_replay(n) + run(n) in one kernel per launch (the draws go
    from each chain's device RandomState straight into the step): the same
    chains, trace and generator state; no replay rows are held afterwards."""
    _lib.call('pbh_legacy_run', self._h, _c.c_int64(int(n_steps)),
              int(steps_per_launch))
    if sync:
      self.sync()

  def set_record_threshold(self, on=True):
    """Keep each step's MH threshold t of the next legacy_run calls on the
    device (get_thresholds)."""
    _lib.call('pbh_set_record_threshold', self._h, 1 if on else 0)

  def get_thresholds(self, first, n_steps):
    """Thresholds of steps [first, first + n_steps) of the last legacy_run
    (set_record_threshold first): [n_steps, N]."""
    out = np.empty((int(n_steps), self.n), np.float64)
    _lib.call('pbh_get_thresholds', self._h, _c.c_int64(int(first)),
              _c.c_int64(int(n_steps)), _dp(out))
    return out

  def legacy_draws(self, n_steps, step0=0, kind='linreg', param=1.0):
    """The next n_steps draws of every chain's device RandomState, [n_steps,
    N]: kind 'linreg' -- standard_gamma(param) on steps (step0 + t) % 3 == 2,
    the legacy gauss otherwise (gibbs_linreg's cond_reg order); 'gauss' --
    the legacy gauss every step."""
    k = {'gauss': _lib.DRAWS_GAUSS, 'linreg': _lib.DRAWS_LINREG}[kind]
    out = np.empty((int(n_steps), self.n), np.float64)
    _lib.call('pbh_legacy_draws', self._h, _c.c_int64(int(n_steps)),
              _c.c_int64(int(step0)), k, _c.c_double(float(param)), _dp(out))
    return out

  def sync(self):
    rc = self._fn_sync(self._h)
    if rc:
      _lib.raise_status('pbh_sync', rc)

  def set_collect(self, moments=True):
    """moments=False: the kernels keep no running moments (no per-launch
    read-modify-write); trace_stats() reduces the recorded trace instead."""
    _lib.call('pbh_set_collect', self._h,
              _lib.COLLECT_MOMENTS if moments else 0)

  def last_run_ms(self):
    ms, nl = _c.c_double(), _c.c_int64()
    _lib.call('pbh_last_run_ms', self._h, _c.byref(ms), _c.byref(nl))
    return ms.value, nl.value

  def stop_server(self):
    """Stops the resident sampling server (PBH_SERVER=1) if it runs: the
    chain state is stored and the stream is idle afterwards."""
    _lib.call('pbh_server_stop', self._h)

  def server_stamps(self):
    """Per-workgroup (seq, t0, t1) of the server's last command (10 ns)."""
    cap = 4096
    q = np.zeros(cap, np.uint32)
    t0 = np.zeros(cap, np.uint64)
    t1 = np.zeros(cap, np.uint64)
    n = _c.c_int32()
    _lib.call('pbh_server_stamps', self._h, cap, q.ctypes.data_as(_lib._u32p),
              t0.ctypes.data_as(_lib._u64p), t1.ctypes.data_as(_lib._u64p),
              _c.byref(n))
    k = min(n.value, cap)
    return q[:k], t0[:k], t1[:k]

  def server_info(self):
    """{'active', 'commands', 'launches'} of the resident sampling server."""
    a, c, n = _c.c_int32(), _c.c_int64(), _c.c_int64()
    _lib.call('pbh_server_info', self._h, _c.byref(a), _c.byref(c), _c.byref(n))
    return {'active': bool(a.value), 'commands': c.value, 'launches': n.value}

  # ---- results -----------------------------------------------------------
  def state(self):
    x = np.empty((self.n, self.dim))
    lp = np.empty(self.n)
    _lib.call('pbh_get_state', self._h, _dp(x), _dp(lp))
    return x, lp

  def checkpoint(self):
    """Everything the chains need to continue exactly (pbh_get_checkpoint):
    x [N, d], lp [N], the global step, the step-1 flag, and the xoshiro
    generator state when that is the RNG."""
    x = np.empty((self.n, self.dim))
    lp = np.empty(self.n)
    step, hp = _c.c_int64(), _c.c_int32()
    xo = np.empty((8, self.n), np.uint32) if self._rng == 'xoshiro' else None
    _lib.call('pbh_get_checkpoint', self._h, _dp(x), _dp(lp), _c.byref(step),
              _c.byref(hp),
              None if xo is None else xo.ctypes.data_as(_lib._u32p))
    lx = np.empty((self.n, self.dim))
    valid = _c.c_int32()
    _lib.call('pbh_get_chain_logs', self._h, _dp(lx), _c.byref(valid))
    return {'x': x, 'lp': lp, 'step': step.value, 'has_pred': bool(hp.value),
            'xo': xo, 'mt': self._legacy_state(), 'chain_offset': self.chain_offset,
            'lx': lx if valid.value else None}

  def _legacy_state(self):
    """The device legacy streams' state (key, pos, has, gauss) or None."""
    words = _c.c_int64()
    _lib.call('pbh_legacy_state_words', self._h, _c.byref(words))
    if not words.value:
      return None
    key = np.empty((words.value, self.n), np.uint32)
    pos = np.empty(self.n, np.int32)
    has = np.empty(self.n, np.int32)
    gauss = np.empty(self.n)
    _lib.call('pbh_get_legacy_state', self._h, key.ctypes.data_as(_lib._u32p),
              pos.ctypes.data_as(_lib._i32p), has.ctypes.data_as(_lib._i32p),
              _dp(gauss))
    return {'key': key, 'pos': pos, 'has': has, 'gauss': gauss}

  def set_chains(self, x, lp, step, has_pred):
    """Replaces the chain state and step anywhere in a run; generator
    states continue (pbh_set_chains).  The trace and the replay rows are
    detached: alloc_trace (and upload_replay / legacy_replay) again."""
    x = np.ascontiguousarray(x, np.float64).reshape(self.n, self.dim)
    lp = np.ascontiguousarray(lp, np.float64).reshape(self.n)
    _lib.call('pbh_set_chains', self._h, _dp(x), _dp(lp), _c.c_int64(int(step)),
              1 if has_pred else 0)

  def restore(self, ck):
    """Resume from checkpoint() (after init_chains of the same N and set_rng
    with the same mode and seed, before alloc_trace)."""
    x = np.ascontiguousarray(ck['x'], np.float64)
    lp = np.ascontiguousarray(ck['lp'], np.float64)
    if x.shape != (self.n, self.dim) or lp.shape != (self.n,):
      raise ValueError('checkpoint shape does not match the engine')
    xo = ck.get('xo')
    xo = None if xo is None else np.ascontiguousarray(xo, np.uint32)
    if xo is not None and xo.size != 8 * self.n:   # [4 words][2 halves][N]
      raise ValueError('checkpoint xoshiro state has {} words, the engine needs '
                       '{}'.format(xo.size, 8 * self.n))
    mt = ck.get('mt')
    if mt is not None:
      # the C side copies words x N, N, N, N values from these arrays: a
      # checkpoint of the other legacy layout (PBH_LEGACY_K4) or of another
      # chain count would be read past its end
      words = _c.c_int64()
      _lib.call('pbh_legacy_state_words', self._h, _c.byref(words))
      want = {'key': (words.value, self.n), 'pos': (self.n,), 'has': (self.n,),
              'gauss': (self.n,)}
      layouts = {640: 'Mt4, its current chunked block (the default since round 6)',
                 2560: 'Mt4, four chunked blocks (rounds 4-5)',
                 1248: 'double-buffered window (PBH_LEGACY_K4=0, and the automatic '
                       'choice from 104 858 chains)'}
      for k, shape in want.items():
        got = np.shape(mt[k])
        if got != shape:
          hint = ''
          if k == 'key' and len(got) == 2 and got[1] == self.n:
            hint = ('; the checkpoint holds the {} layout, this engine the {}: '
                    'restore it in an engine created with that layout\'s '
                    'environment'.format(
                        layouts.get(got[0], '{}-word'.format(got[0])),
                        layouts.get(words.value, '{}-word'.format(words.value))))
            if got[0] == 624:
              hint = ('; the checkpoint holds the round-1 in-place layout, which '
                      'is gone: no engine restores it')
          raise ValueError('checkpoint legacy state {} has shape {}, this engine '
                           'needs {} (legacy layout words per chain: {}){}'.format(
                               k, got, shape, words.value, hint))
    _lib.call('pbh_restore', self._h, _dp(x), _dp(lp),
              _c.c_int64(int(ck['step'])), 1 if ck['has_pred'] else 0,
              None if xo is None else xo.ctypes.data_as(_lib._u32p))
    lx = ck.get('lx')
    if lx is not None:   # the production ufun logs (pbh_set_chain_logs)
      lx = np.ascontiguousarray(lx, np.float64)
      if lx.shape != (self.n, self.dim):
        raise ValueError('checkpoint ufun logs have shape {}, the engine needs {}'
                         .format(lx.shape, (self.n, self.dim)))
      _lib.call('pbh_set_chain_logs', self._h, _dp(lx))
    if mt is not None:   # device legacy streams continue where they were
      key = np.ascontiguousarray(mt['key'], np.uint32)
      pos = np.ascontiguousarray(mt['pos'], np.int32)
      has = np.ascontiguousarray(mt['has'], np.int32)
      gauss = np.ascontiguousarray(mt['gauss'], np.float64)
      _lib.call('pbh_set_legacy_state', self._h, key.ctypes.data_as(_lib._u32p),
                pos.ctypes.data_as(_lib._i32p), has.ctypes.data_as(_lib._i32p),
                _dp(gauss))

  def trace_len(self):
    r = _c.c_int64()
    _lib.call('pbh_trace_len', self._h, _c.byref(r))
    return r.value

  def _window(self, first, count):
    """(first, count), count defaulting to every record from first on."""
    return first, self.trace_len() - first if count is None else count

  def trace(self, first=0, count=None, debug=None):
    """Recorded steps as chain-major arrays shaped like the golden fixtures:
    v_x [N, T, d], v_p [N, T], u [N, T] (uint8); with debug also p_x, p_p, s."""
    first, count = self._window(first, count)
    n, d = self.n, self.dim
    W = (n + 63) // 64
    x = np.empty((count, d, n))
    lp = np.empty((count, n))
    acc = np.empty((count, W), np.uint64)
    debug = self.debug if debug is None else debug
    px = np.empty((count, d, n)) if debug else None
    pp = np.empty((count, n)) if debug else None
    sc = np.empty((count, n)) if debug else None
    nul = _c.POINTER(_c.c_double)()
    _lib.call('pbh_get_trace', self._h, _c.c_int64(first), _c.c_int64(count),
              _dp(x), _dp(lp), acc.ctypes.data_as(_c.POINTER(_c.c_uint64)),
              _dp(px) if debug else nul, _dp(pp) if debug else nul,
              _dp(sc) if debug else nul)
    out = {'v_x': x.transpose(2, 0, 1), 'v_p': lp.T, 'u': unpack_accept(acc, n)}
    if debug:
      out.update({'p_x': px.transpose(2, 0, 1), 'p_p': pp.T, 's': sc.T})
    return out

  def moments(self):
    n, d = self.n, self.dim
    s = np.empty((d, n))
    q = np.empty((d, n))
    na = np.empty(n, np.int64)
    steps = _c.c_int64()
    _lib.call('pbh_get_moments', self._h, _dp(s), _dp(q),
              na.ctypes.data_as(_c.POINTER(_c.c_int64)), _c.byref(steps))
    return {'sum': s.T.copy(), 'sumsq': q.T.copy(), 'n_acc': na,
            'n_steps': steps.value}

  def trace_stats(self, first=0, count=None):
    """Per-chain sum / sumsq / n_acc of trace records [first, first +
    count), reduced on the device (also replaces the engine's moments)."""
    first, count = self._window(first, count)
    n, d = self.n, self.dim
    s = np.empty((d, n))
    q = np.empty((d, n))
    na = np.empty(n, np.int64)
    _lib.call('pbh_trace_stats', self._h, _c.c_int64(int(first)),
              _c.c_int64(int(count)), _dp(s), _dp(q),
              na.ctypes.data_as(_c.POINTER(_c.c_int64)))
    return {'sum': s.T.copy(), 'sumsq': q.T.copy(), 'n_acc': na,
            'n_steps': int(count)}

  def reset_moments(self):
    _lib.call('pbh_reset_moments', self._h)

  # ---- RCCL ---------------------------------------------------------------
  @staticmethod
  def rccl_unique_id():
    buf = (_c.c_uint8 * 128)()
    _lib.call('pbh_rccl_unique_id', buf)
    return bytes(buf)

  def rccl_init(self, rank, world, uid):
    buf = (_c.c_uint8 * 128).from_buffer_copy(uid)
    _lib.call('pbh_rccl_init', self._h, int(rank), int(world), buf)
    self.world = int(world)

  def rccl_allgather_stats(self):
    """The one RCCL all-gather: every rank's per-chain statistics, in
    global chain order (ranks hold contiguous blocks, dist.shard).  Returns
    {'sum': [N, d], 'sumsq': [N, d], 'n_acc': [N], 'ess': [N, d],
    'counts': [world]}; ess is NaN for a rank that never ran trace_ess."""
    d = self.dim
    nm = _c.c_int64()
    _lib.call('pbh_rccl_max_chains', self._h, _c.byref(nm))
    out = np.empty((self.world, 3 * d + 1, nm.value))
    counts = np.empty(self.world, np.int64)
    _lib.call('pbh_rccl_allgather_stats', self._h, _dp(out),
              counts.ctypes.data_as(_c.POINTER(_c.c_int64)))
    return unpack_stats(out, counts, d)

  def trace_ess(self, first=0, count=None):
    """Per-chain, per-dim initial-positive-sequence ESS of trace records
    [first, first + count), computed on the device: [N, d]."""
    first, count = self._window(first, count)
    out = np.empty((self.dim, self.n))
    _lib.call('pbh_trace_ess', self._h, _c.c_int64(int(first)),
              _c.c_int64(int(count)), _dp(out))
    return out.T   # a [N, d] view of the [d][N] result (no 2-D transpose copy)

  def trace_ess_total(self, first=0, count=None):
    """Per dim, the sum over chains of trace_ess (reduced on the device):
    [d]."""
    first, count = self._window(first, count)
    out = np.empty(self.dim)
    _lib.call('pbh_trace_ess_total', self._h, _c.c_int64(int(first)),
              _c.c_int64(int(count)), _dp(out))
    return out

  def trace_expectation(self, first=0, count=None, exponent=None):
    """PD.expectation (pd.py:373-405) of the summary of trace records
    [first, first + count), computed on the device: [N, d] of
    sum p v^exponent / sum p with p the recorded prob rescaled to linear."""
    first, count = self._window(first, count)
    out = np.empty((self.dim, self.n))
    _lib.call('pbh_trace_expectation', self._h, _c.c_int64(int(first)),
              _c.c_int64(int(count)), _c.c_double(float(exponent or 0.)),
              _dp(out))
    return out.T.copy()

  def trace_quantile(self, q, first=0, count=None, weighted=True):
    """summary.sorted(key).quantile(q)[key] (pd.py:408-493) of trace records
    [first, first + count) for every chain and every key, computed on the
    device: [nq, N, d], or [N, d] for a scalar q.  Each dim is sorted by
    itself.  weighted: the recorded prob rescaled to linear as weights;
    otherwise unit weights (the empirical quantile).  count is at most 2 048
    records (PBH_QUANTILE_MAX_RECORDS), nq at most 64."""
    first, count = self._window(first, count)
    scalar = np.isscalar(q)
    qs, nq = _quantiles(q)
    out = np.empty((qs.size, self.dim, self.n))
    _lib.call('pbh_trace_quantile', self._h, _c.c_int64(int(first)),
              _c.c_int64(int(count)), _c.c_int32(nq), _dp(qs),
              _c.c_int32(1 if weighted else 0), _dp(out))
    res = out.transpose(0, 2, 1).copy()
    return res[0] if scalar else res

  def trace_rhat(self, first=0, count=None, group=None, stats=False):
    """Cross-chain convergence of trace records [first, first + count), per
    dim, computed on the device (probayes_amd/diag.py is the definition):
    {'split': [d], 'nested': [d] or None}.  split: split-R-hat over the 2 N
    half chains (count >= 4; an odd count drops the middle record).  nested,
    with group=M: nested R-hat over the N / M superchains of M consecutive
    chains, which the caller started at one point each (M >= 1 divides N, N /
    M >= 2).  stats=True adds 'stats': [6, N, d], the per-chain mean and
    variance (ddof 1) of the first half, the second half and the whole window
    -- the rows diag.split_rhat / diag.nested_rhat work from."""
    first, count = self._window(first, count)
    d, n = self.dim, self.n
    split = np.empty(d)
    nested = None if group is None else np.empty(d)
    rows = np.empty((6, d, n)) if stats else None
    _lib.call('pbh_trace_rhat', self._h, _c.c_int64(int(first)),
              _c.c_int64(int(count)), _c.c_int32(0 if group is None else int(group)),
              _dp(split), None if nested is None else _dp(nested),
              None if rows is None else _dp(rows))
    res = {'split': split, 'nested': nested}
    if stats:
      res['stats'] = rows.transpose(0, 2, 1).copy()
    return res

  def trace_quantile_pooled(self, q, first=0, count=None, order_stats=False):
    """The quantiles q of trace records [first, first + count) pooled over
    every chain and record, per dim, computed on the device: [nq, d]
    (diag.pooled_quantile is the definition; np.quantile's default method, bit
    for bit).  A radix select in six streaming passes over the window: no
    record limit.  A dim holding a NaN gives NaN.  nq is at most 64.
    order_stats=True returns (quantiles, [nq, 2, d]): the two sorted values
    each quantile is interpolated between."""
    first, count = self._window(first, count)
    qs, nq = _quantiles(q)
    out = np.empty((qs.size, self.dim))
    stats = np.empty((qs.size, 2, self.dim)) if order_stats else None
    _lib.call('pbh_trace_quantile_pooled', self._h, _c.c_int64(int(first)),
              _c.c_int64(int(count)), _c.c_int32(nq), _dp(qs), _dp(out),
              None if stats is None else _dp(stats))
    return (out, stats) if order_stats else out

  def trace_rhat_rank(self, first=0, count=None, ranks=False):
    """The rank-normalised split-R-hat (Vehtari et al. 2021) of trace records
    [first, first + count), per dim, computed on the device (diag.rank_rhat is
    the definition): {'bulk': [d], 'folded': [d], 'rhat': [d]}.  bulk is
    split-R-hat of the normal scores of the ranks of every draw pooled over
    chains and records; folded the same of the ranks of |x - pooled median|,
    which sees chains that agree in location but not in scale; rhat is the
    larger of the two, the number to read.  count >= 4; N count < 2^32.
    ranks=True adds 'ranks' and 'folded_ranks': [N, count, d], the 1-based
    average ranks themselves (diag.average_ranks, exactly)."""
    first, count = self._window(first, count)
    d, n = self.dim, self.n
    bulk, folded = np.empty(d), np.empty(d)
    rows = [np.empty((count, d, n)) for _ in range(2)] if ranks else [None, None]
    _lib.call('pbh_trace_rhat_rank', self._h, _c.c_int64(int(first)),
              _c.c_int64(int(count)), _dp(bulk), _dp(folded),
              None if rows[0] is None else _dp(rows[0]),
              None if rows[1] is None else _dp(rows[1]))
    res = {'bulk': bulk, 'folded': folded, 'rhat': np.maximum(bulk, folded)}
    if ranks:
      res['ranks'] = rows[0].transpose(2, 0, 1).copy()
      res['folded_ranks'] = rows[1].transpose(2, 0, 1).copy()
    return res

  def trace_ess_rank(self, first=0, count=None, basic=False, acov=False):
    """The bulk- and tail-ESS across chains (Vehtari et al. 2021) of trace
    records [first, first + count), per dim, computed on the device
    (diag.rank_ess is the definition): {'bulk': [d], 'tail': [d], 'tail_lower':
    [d], 'tail_upper': [d]}, the effective sample sizes to read beside the
    rank-normalised R-hat.  Each is Stan's estimator over the 2 N split chains
    from their means and their averaged autocovariance: bulk of the normal
    scores of the pooled ranks, tail_lower / tail_upper of the indicators x <=
    the pooled 5 % / 95 % quantile, tail the smaller of the two.  basic=True
    adds 'basic', the same of the values themselves.  acov=True adds 'acov':
    {variant: [d, h]}, the averaged autocovariances A[t], t < h = count // 2, of
    every variant computed.  count >= 4, count // 2 <= 2 048; N count < 2^32."""
    first, count = self._window(first, count)
    d, h = self.dim, max(int(count) // 2, 0)
    bulk, tail, parts = np.empty(d), np.empty(d), np.empty((2, d))
    vals = np.empty(d) if basic else None
    rows = np.empty((4, d, h)) if acov else None
    _lib.call('pbh_trace_ess_rank', self._h, _c.c_int64(int(first)),
              _c.c_int64(int(count)), _dp(bulk), _dp(tail), _dp(parts),
              None if vals is None else _dp(vals), None if rows is None else _dp(rows))
    res = {'bulk': bulk, 'tail': tail, 'tail_lower': parts[0].copy(),
           'tail_upper': parts[1].copy()}
    if basic:
      res['basic'] = vals
    if acov:
      res['acov'] = {key: rows[v].copy()
                     for v, key in enumerate(('bulk', 'tail_lower', 'tail_upper', 'basic'))
                     if basic or key != 'basic'}
    return res

  def trace_pointwise(self, program, first=0, count=None):
    """Per observation, the statistics over the N count draws of trace records
    [first, first + count) of the term a pointwise program gives, computed on
    the device without the terms [draws, n_obs] ever being stored
    (expr.evaluate_pointwise and diag.pointwise_stats are the definition):
    {'lse': [n_obs], 'mean': [n_obs], 'var': [n_obs]} -- the log-sum-exp (lppd_j
    = lse_j - log(N count)), the mean and the sample variance (ddof 1).
    program: what expr.trace_pointwise returns, over this engine's dims in
    order; it has nothing to do with the engine's own model, which may be of
    any kind.  N count >= 2."""
    first, count = self._window(first, count)
    args, n_obs = self._pointwise_args(program, first, count)
    out = np.empty((3, max(n_obs, 1)))
    _lib.call('pbh_trace_pointwise', *args, _dp(out[0]), _dp(out[1]), _dp(out[2]))
    return {'lse': out[0].copy(), 'mean': out[1].copy(), 'var': out[2].copy()}

  def _pointwise_args(self, program, first, count):
    """The engine, window and program arguments pbh_trace_pointwise and
    pbh_trace_pointwise_tail share (each pointer keeps its array alive), and
    n_obs."""
    code = np.ascontiguousarray(program['code'], dtype=np.int32)
    consts = _f64(program['consts']).ravel()
    if consts.size == 0:
      consts = np.zeros(1)
    data = program.get('data')
    data = None if data is None else np.atleast_2d(_f64(data))
    n_cols, n_obs = (0, 0) if data is None else data.shape
    args = (self._h, _c.c_int64(int(first)), _c.c_int64(int(count)), _ip(code),
            _c.c_int32(code.size), _dp(consts),
            _c.c_int32(np.asarray(program['consts']).size),
            _c.c_int32(int(program['depth'])), None if data is None else _dp(data),
            _c.c_int32(int(n_cols)), _c.c_int32(int(n_obs)))
    return args, int(n_obs)

  def trace_pointwise_tail(self, program, k, first=0, count=None, capacity=0):
    """Per observation, the k smallest of the terms a pointwise program gives
    over the S = N count draws of trace records [first, first + count) and the
    log-sum-exp of minus the other S - k, computed on the device without the
    terms ever being stored (expr.evaluate_pointwise and diag.pointwise_tail are
    the definition): {'tail': [n_obs, k] ascending (either zero as +0.0, NaN
    last), 'rest_lse': [n_obs], 'passes': the count passes of the radix select}
    -- what diag.psis_loo_from_tail needs with k = m + 1.  capacity: the
    candidates kept per observation for the host's sort (0: max(2 k, 65 536));
    the select passes until they fit.  1 <= k < S, capacity >= k."""
    first, count = self._window(first, count)
    args, n_obs = self._pointwise_args(program, first, count)
    k = int(k)
    tail, rest = np.empty((max(n_obs, 1), max(k, 1))), np.empty(max(n_obs, 1))
    passes = _c.c_int32(0)
    _lib.call('pbh_trace_pointwise_tail', *args, _c.c_int64(k), _c.c_int64(int(capacity)),
              _dp(tail), _dp(rest), _c.byref(passes))
    return {'tail': tail, 'rest_lse': rest, 'passes': int(passes.value)}

  def trace_cov(self, first=0, count=None):
    """The posterior covariance of trace records [first, first + count) pooled
    over every chain and record, computed on the device (diag.pooled_cov is the
    definition): {'mean': [d], 'cov': [d, d], 'corr': [d, d]}.  The sums are
    taken about the mean over chains of the window's first record, so a
    posterior far from 0 costs no digits.  cov is symmetric in its bits; corr
    has a diagonal of exactly 1, or NaN for a dim that never moves.  One pass
    over the window; count >= 1, N count >= 2."""
    first, count = self._window(first, count)
    d = self.dim
    mean, cov, corr = np.empty(d), np.empty((d, d)), np.empty((d, d))
    _lib.call('pbh_trace_cov', self._h, _c.c_int64(int(first)), _c.c_int64(int(count)),
              _dp(mean), _dp(cov), _dp(corr))
    return {'mean': mean, 'cov': cov, 'corr': corr}

  def _hist_args(self, what, edges):
    """edges, a list of d arrays or None, as the C-ABI takes them: (n_bins
    int32 [d], the dims' edges one after the other).  The library checks the
    edges themselves."""
    if len(edges) != self.dim:
      raise ValueError('{}: {} edge arrays for {} dims (None skips a dim)'.format(
          what, len(edges), self.dim))
    arrays = [None if e is None else _f64(e).ravel() for e in edges]
    for k, e in enumerate(arrays):
      if e is not None and e.size < 2:
        raise ValueError('{}: dim {} has {} edges, a bin needs 2'.format(what, k, e.size))
    n_bins = _i32([0 if e is None else e.size - 1 for e in arrays])
    flat = _f64(np.concatenate([e for e in arrays if e is not None] or [np.zeros(1)]))
    return arrays, n_bins, flat

  def trace_hist(self, edges, first=0, count=None):
    """The histograms of trace records [first, first + count) pooled over every
    chain and record, per dim, computed on the device (diag.pooled_hist is the
    definition; np.histogram(values, edges) bit for bit).  edges: a list of d
    arrays of strictly increasing finite edges, at most 4 096 bins each, None
    for a dim to skip.  {'counts': [int64 [B_k] or None per dim], 'outside':
    int64 [d, 3]}: outside holds the draws below the first edge, above the last
    one and NaN, so that a dim's counts and its row add up to N count.  One
    pass over the window for dims that fit a workgroup's LDS together."""
    first, count = self._window(first, count)
    arrays, n_bins, flat = self._hist_args('trace_hist', edges)
    counts = np.zeros(max(int(n_bins.sum()), 1), np.int64)
    outside = np.zeros((self.dim, 3), np.int64)
    i64p = _c.POINTER(_c.c_int64)
    _lib.call('pbh_trace_hist', self._h, _c.c_int64(int(first)), _c.c_int64(int(count)),
              _ip(n_bins), _dp(flat), counts.ctypes.data_as(i64p),
              outside.ctypes.data_as(i64p))
    ends = np.cumsum(n_bins)
    return {'counts': [None if e is None else counts[end - b:end].copy()
                       for e, b, end in zip(arrays, n_bins, ends)],
            'outside': outside}

  def trace_hist2d(self, edges, pairs, first=0, count=None):
    """The joint histograms of pairs of dims over trace records [first, first
    + count), pooled over every chain and record, computed on the device
    (diag.pooled_hist2d is the definition; np.histogram2d with explicit edges
    bit for bit): a list of int64 [B_a, B_b], one per (a, b) in pairs.  H[i, j]
    counts the draws with x_a in bin i of dim a and x_b in bin j of dim b; a
    draw with either value outside its edges, or NaN, is dropped.  edges as
    trace_hist takes them; a pair has at most 16 384 cells; a == b is
    allowed."""
    first, count = self._window(first, count)
    _, n_bins, flat = self._hist_args('trace_hist2d', edges)
    pr = _i32(np.asarray(pairs, np.int64).reshape(-1, 2) if len(pairs) else np.zeros((0, 2)))
    # The library refuses a pair it cannot count -- a dim outside [0, d) or
    # without edges, more than PBH_HIST2D_MAX_CELLS cells -- with the message
    # that names it, before it writes anything (hist2d_check_pairs runs ahead
    # of the window check), so such a pair is passed on, not refused here.  The
    # buffer does not lean on that order: a pair the library would refuse is
    # given the most cells any pair may have.
    max_cells = 16384   # PBH_HIST2D_MAX_CELLS
    d = self.dim
    shapes = [(int(n_bins[a]), int(n_bins[b])) if 0 <= a < d and 0 <= b < d else (0, 0)
              for a, b in pr]
    sizes = [ba * bb if 0 < ba * bb <= max_cells else max_cells for ba, bb in shapes]
    counts = np.zeros(max(sum(sizes), 1), np.int64)
    _lib.call('pbh_trace_hist2d', self._h, _c.c_int64(int(first)), _c.c_int64(int(count)),
              _ip(n_bins), _dp(flat), _c.c_int32(pr.shape[0]),
              _ip(pr if pr.size else np.zeros(2, np.int32)),
              counts.ctypes.data_as(_c.POINTER(_c.c_int64)))
    ends = np.cumsum(sizes)
    return [counts[end - size:end].reshape(shape).copy()
            for shape, size, end in zip(shapes, sizes, ends)]

  def rccl_allreduce_max(self, value):
    v = _c.c_double(float(value))
    _lib.call('pbh_rccl_allreduce_max', self._h, _c.byref(v))
    return v.value

  @staticmethod
  def cache_release():
    """Frees the device buffers and streams destroyed engines left in the
    library's resource cache (pbh_cache_release)."""
    _lib.call('pbh_cache_release')

  @staticmethod
  def cache_info():
    """(idle bytes, hits, misses) of the library's resource cache."""
    v = [_c.c_int64() for _ in range(3)]
    _lib.call('pbh_cache_info', *[_c.byref(x) for x in v])
    return tuple(x.value for x in v)

  def close(self):
    if getattr(self, '_h', None) is not None and self._h.value:
      _lib.load().pbh_destroy(self._h)
      self._h = _c.c_void_p()

  def __del__(self):
    try:
      self.close()
    except Exception:
      pass

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    self.close()
