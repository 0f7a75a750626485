"""pbh_trace_quantile (Engine.trace_quantile, Sampler.trace_quantile): the
sorted-summary quantiles of a recorded trace computed on the device, against
PD.sorted(key).quantile(q)[key] applied to the same trace copied to the host.

The host reference of key k is PD('v', {k: vals}, prob, pscale).sorted(k)
.quantile(q)[c][j][k]: the other keys of a summary do not enter the
arithmetic of key k (after sorted(k) they give {size}), so the single-key PD
is the same computation and the reference takes a fraction of the time.
"""
import functools
import os
import sys

import numpy as np
import pytest

import oracle
from oracle.workloads import golden_init
from probayes_amd._lib import PbhError
from probayes_amd.pd import PD
from probayes_amd.pscales import rescale
from trace_helpers import check_no_side_effects, run, sampler_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

QS = [0., 0.05, 0.5, 0.95, 1.]


def _host(vals, prob, pscale, qs):
  """[nq, N] of PD.sorted('k').quantile(qs) for one key's values [T, N]."""
  res = PD('v', {'k': vals}, prob=prob, pscale=pscale).sorted('k').quantile(list(qs))
  return np.array([[res[c][j]['k'] for c in range(vals.shape[1])]
                   for j in range(len(qs))], float)


def _host_all(tr, first, count, names, pscale, qs, weighted):
  """[nq, N, d] from a host trace (v_x [N, T, d], v_p [N, T])."""
  n = tr['v_x'].shape[0]
  out = np.empty((len(qs), n, len(names)))
  for i in range(len(names)):
    vals = tr['v_x'][:, first:first + count, i].T
    if weighted:
      prob, ps = tr['v_p'][:, first:first + count].T, pscale
    else:
      prob, ps = np.ones((count, n)), 'lin'
    out[:, :, i] = _host(vals, prob, ps, qs)
  return out


def _at_threshold(vals, prob, pscale, qs):
  """[nq, N] bool: the host's own numbers sit at a decision threshold of q
  (within 1e-9), for 0 < q < 1 -- the only cases a weighted comparison may
  leave out."""
  T, N = vals.shape
  order = np.argsort(vals, axis=0)
  p = np.take_along_axis(rescale(np.asarray(prob, float), pscale, 'lin'), order, axis=0)
  cum = np.cumsum(p, axis=0)
  cumprob = cum / np.maximum(2.2250738585072014e-308, cum[-1])
  cols = np.arange(N)
  out = np.zeros((len(qs), N), bool)
  for j, q in enumerate(qs):
    if not 0. < q < 1.:
      continue
    near_q = (np.abs(cumprob - q) <= 1e-9).any(axis=0)
    idx = np.minimum(np.maximum(0, np.sum(cumprob <= q, axis=0) - 1), T - 1)
    i1 = np.minimum(idx + 1, T - 1)
    gap = np.abs(np.abs(p[i1, cols] - p[idx, cols]) - min(q, 1. - q)) <= 1e-9
    out[j] = near_q | (gap & (idx != T - 1))
  return out


N_BIG, T_BIG, FIRST_BIG = 2003, 160, 40


@functools.lru_cache(maxsize=None)
def _big(name):
  """One run per model shared by the unweighted and the weighted test: the
  host trace and both device results."""
  spec = oracle.golden_spec(name)
  eng = run(spec, golden_init(name, N_BIG), T_BIG)
  try:
    tr = eng.trace()
    cnt = T_BIG - FIRST_BIG
    dev_u = eng.trace_quantile(QS, FIRST_BIG, cnt, weighted=False)
    dev_w = eng.trace_quantile(QS, FIRST_BIG, cnt, weighted=True)
  finally:
    eng.close()
  return spec, tr, dev_u, dev_w


@pytest.mark.parametrize('name', ['diag10', 'gmm2'])
def test_unweighted_equals_the_host_bit_for_bit(name):
  spec, tr, dev_u, _ = _big(name)
  cnt = T_BIG - FIRST_BIG
  assert dev_u.shape == (len(QS), N_BIG, spec['dim'])
  host = _host_all(tr, FIRST_BIG, cnt, spec['names'], spec['pscale'], QS, False)
  # MH traces hold runs of equal values (the rejected steps): both wanted
  x = tr['v_x'][:, FIRST_BIG:, 0]
  rep = x[:, 1:] == x[:, :-1]
  assert rep.any() and not rep.all()
  assert np.array_equal(dev_u, host)


@pytest.mark.parametrize('name', ['diag10', 'gmm2'])
def test_weighted_matches_the_host(name):
  spec, tr, _, dev_w = _big(name)
  cnt = T_BIG - FIRST_BIG
  names, ps = spec['names'], spec['pscale']
  host = _host_all(tr, FIRST_BIG, cnt, names, ps, QS, True)
  prob = tr['v_p'][:, FIRST_BIG:].T
  skip = np.zeros(host.shape, bool)
  scale = np.empty(host.shape)
  for i in range(len(names)):
    vals = tr['v_x'][:, FIRST_BIG:, i].T
    skip[:, :, i] = _at_threshold(vals, prob, ps, QS)
    scale[:, :, i] = np.abs(vals).max(axis=0)[None, :]
  assert not skip[0].any() and not skip[-1].any()     # q = 0, q = 1: never
  assert skip.sum() <= 1e-3 * skip.size, skip.sum()
  assert np.isfinite(host).all() and np.isfinite(dev_w).all()
  rel = np.abs(dev_w - host) / np.maximum(np.maximum(np.abs(host), scale), 1e-300)
  print('weighted {}: max rel {:.3g}, left out {}'.format(name, rel[~skip].max(),
                                                         int(skip.sum())))
  assert rel[~skip].max() <= 1e-12, rel[~skip].max()


EDGES = [(1, 0), (1, 2047), (2, 5), (3, 2045), (64, 0), (65, 1983), (1024, 1024),
         (2047, 1), (2048, 0)]   # (count, first)


def test_record_count_edges():
  spec = oracle.golden_spec('gmm2')
  eng = run(spec, golden_init('gmm2', 67), 2048)
  try:
    tr = eng.trace()
    for cnt, first in EDGES:
      dev = eng.trace_quantile(QS, first, cnt, weighted=False)
      host = _host_all(tr, first, cnt, spec['names'], spec['pscale'], QS, False)
      assert np.array_equal(dev, host), (cnt, first)
      if cnt == 1:
        for j in range(len(QS)):
          assert np.array_equal(dev[j], tr['v_x'][:, first, :]), (first, j)
    # a scalar q: [N, d], the row of the list form
    one = eng.trace_quantile(0.5, 0, 65, weighted=False)
    assert np.array_equal(one, eng.trace_quantile([0.5], 0, 65, weighted=False)[0])
  finally:
    eng.close()


def test_refusals_leave_the_engine_working():
  from probayes_amd import Engine
  spec = oracle.golden_spec('gmm2')
  eng = Engine(spec)
  try:
    eng.init_chains(golden_init('gmm2', 67))
    eng.set_rng('philox', seed=3)
    with pytest.raises(PbhError, match='no trace'):
      eng.trace_quantile(0.5, 0, 1)
    eng.alloc_trace(2100, 1)
    eng.run(2100, steps_per_launch=64)
    bad = [dict(q=0.5, first=0, count=2049),
           dict(q=0.5, first=2000, count=101),
           dict(q=0.5, first=0, count=0),
           dict(q=[], first=0, count=10),
           dict(q=np.linspace(0., 1., 65), first=0, count=10),
           dict(q=[0.5, -0.1], first=0, count=10),
           dict(q=1.5, first=0, count=10),
           dict(q=[float('nan')], first=0, count=10)]
    for kw in bad:
      with pytest.raises(PbhError):
        eng.trace_quantile(**kw)
    tr = eng.trace()
    dev = eng.trace_quantile(QS, 52, 2048, weighted=False)
    host = _host_all(tr, 52, 2048, spec['names'], spec['pscale'], QS, False)
    assert np.array_equal(dev, host)
  finally:
    eng.close()


def test_no_side_effects_and_determinism():
  def reduce(eng):
    a = eng.trace_quantile(QS, 3, 61, weighted=True)
    b = eng.trace_quantile(QS, 3, 61, weighted=True)
    assert a.tobytes() == b.tobytes()
    u = eng.trace_quantile(QS, 3, 61, weighted=False)
    assert u.tobytes() == eng.trace_quantile(QS, 3, 61, weighted=False).tobytes()

  check_no_side_effects(reduce, 515)


# ---- with the resident server (the pattern of test_gpu_server.py) ----------
N_SRV = 8192
PLAN = [1, 1, 1, 1, 20, 7, 1, 2, 3, 64, 65, 1, 100]


def _engine(monkeypatch, server):
  import bench
  from probayes_amd import Engine
  monkeypatch.setenv('PBH_SERVER', '1' if server else '0')
  eng = Engine(bench.cfg2_spec())
  x0 = np.random.RandomState(5).normal(size=(N_SRV, bench.D))
  eng.init_chains(x0)
  eng.set_rng('philox', seed=31)
  eng.set_collect(moments=False)
  eng.alloc_trace(400, 1)
  return eng


def _runs(eng, plan, between=None):
  for i, k in enumerate(plan):
    eng.run(k, steps_per_launch=k)
    if between:
      between(i, eng)


def test_trace_quantile_between_server_commands(monkeypatch):
  got = {}

  def between(i, eng):
    if i == 8:   # 37 records so far
      active = eng.server_info()['active']
      got[(active, 'q')] = eng.trace_quantile([0.25, 0.5], 2, 35, weighted=False)
      assert not eng.server_info()['active']   # the call stopped the server
      got[(active, 'active')] = active

  ref = _engine(monkeypatch, False)
  _runs(ref, PLAN, between)
  tr_ref = ref.trace()
  ref.close()
  eng = _engine(monkeypatch, True)
  _runs(eng, PLAN, between)
  info = eng.server_info()
  assert info['launches'] == 2, info   # relaunched after the call
  tr = eng.trace()
  eng.close()
  assert got[(True, 'active')] and not got[(False, 'active')]
  assert np.array_equal(got[(True, 'q')], got[(False, 'q')])
  for k in ('v_x', 'v_p', 'u'):
    assert np.array_equal(tr[k], tr_ref[k]), k


# ---- the facade --------------------------------------------------------------
def test_sampler_trace_quantile():
  n, t, qs = 67, 96, [0.05, 0.5, 0.95]
  with sampler_block(n, t) as (sampler, process, _, keys, v):
    dev_u = sampler.trace_quantile(qs, weighted=False)
    dev_w = sampler.trace_quantile(qs, weighted=True)
    one = sampler.trace_quantile(0.5, weighted=False)
    prob = np.asarray(v.prob)
    assert prob.shape == (t, n)
    for k in keys:
      vals = np.asarray(v[k])
      assert dev_u[k].shape == (len(qs), n) and one[k].shape == (n,)
      assert np.array_equal(dev_u[k], _host(vals, np.ones((t, n)), 'lin', qs))
      assert np.array_equal(one[k], dev_u[k][1])
      host = _host(vals, prob, v.pscale, qs)
      skip = _at_threshold(vals, prob, v.pscale, qs)
      assert skip.sum() <= 1e-3 * skip.size
      scale = np.abs(vals).max(axis=0)[None, :]
      rel = np.abs(dev_w[k] - host) / np.maximum(np.maximum(np.abs(host), scale), 1e-300)
      assert rel[~skip].max() <= 1e-12, (k, rel[~skip].max())
    # a second block: the engine's trace is no longer the first block's
    process.next(sampler)
    with pytest.raises(ValueError, match='another block'):
      sampler.trace_quantile(qs)
