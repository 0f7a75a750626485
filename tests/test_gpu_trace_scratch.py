"""The one scratch buffer the trace reductions share (pbh_trace_expectation,
pbh_trace_quantile, pbh_trace_rhat, pbh_trace_quantile_pooled): whatever a
call finds in it, left by another reduction or by a larger one, its result is
the same bits.

Two engines with one seed make the same six calls, one in an order in which
the scratch grows step by step, the other in reverse, so that it starts at
its largest and every later call finds it dirty.  gmm2 (d = 2) with N = 130
chains (no multiple of 64, three waves) and T = 70 records (the per-series
sort pads to 128): the smallest shapes at which a stale or undersized scratch
can show.  Nothing is left out of a comparison."""
import numpy as np
import pytest

import oracle
from oracle.workloads import golden_init
from probayes_amd import diag
from test_gpu_quantile import _host_all
from trace_helpers import Q64, run

pytestmark = pytest.mark.gpu

N, T = 130, 70
CALLS = [
    ('pooled_one', lambda e: e.trace_quantile_pooled([.5])),
    ('rhat_2', lambda e: e.trace_rhat(group=2, stats=True)),
    ('quantile_64', lambda e: e.trace_quantile(Q64, weighted=False)),
    ('expectation', lambda e: e.trace_expectation()),
    ('pooled_64', lambda e: e.trace_quantile_pooled(Q64, order_stats=True)),
    ('rhat_65', lambda e: e.trace_rhat(group=65)),
]


def _flat(res):
  """every array of a result, in a fixed order"""
  if isinstance(res, dict):
    return [res[k] for k in sorted(res) if res[k] is not None]
  return list(res) if isinstance(res, tuple) else [res]


def test_results_do_not_depend_on_what_the_scratch_held():
  spec = oracle.golden_spec('gmm2')
  got, traces = [], []
  for calls in (CALLS, CALLS[::-1]):
    eng = run(spec, golden_init('gmm2', N), T)
    try:
      got.append({name: call(eng) for name, call in calls})
      traces.append(eng.trace())
    finally:
      eng.close()
  a, b = got
  assert np.array_equal(traces[0]['v_x'], traces[1]['v_x'])
  assert a['rhat_2']['stats'].shape == (6, N, 2) and a['rhat_65']['nested'].shape == (2,)
  for name, _ in CALLS:
    fa, fb = _flat(a[name]), _flat(b[name])
    assert len(fa) == len(fb) > 0, name
    for u, v in zip(fa, fb):
      assert u.shape == v.shape and u.tobytes() == v.tobytes(), name
  # and they are the host's definitions on the trace copied out
  x = traces[0]['v_x']
  assert x.shape == (N, T, 2)
  host = _host_all(traces[0], 0, T, spec['names'], spec['pscale'], Q64, False)
  for res in got:
    assert np.array_equal(res['pooled_one'], diag.pooled_quantile(x, [.5]))
    quant, stats = res['pooled_64']
    assert np.array_equal(quant, diag.pooled_quantile(x, Q64))
    assert stats.shape == (64, 2, 2)
    assert np.array_equal(res['quantile_64'], host)
