"""What the device tests of the trace reductions share (test_gpu_quantile.py,
test_gpu_rhat.py, test_gpu_pooled_quantile.py, test_gpu_trace_scratch.py): an
engine with a recorded trace, and the check that a reduction changes nothing
but its own result."""
import numpy as np

import oracle
from oracle.workloads import golden_init


def run(spec, init, t, seed=3):
  """An engine of spec started at init with t steps run and recorded."""
  from probayes_amd import Engine
  eng = Engine(spec)
  eng.init_chains(init)
  eng.set_rng('philox', seed=seed)
  eng.alloc_trace(t, 1)
  eng.run(t, steps_per_launch=64)
  return eng


def check_no_side_effects(reduce, n):
  """reduce(eng) makes the reductions under test on a gmm2 engine of n chains
  with 64 of 96 records.  They must leave alone the trace, the moments, the
  chain state, what the RCCL all-gather sends (the moments and the per-chain
  ESS), and what trace_stats and trace_ess give next; and the run must go on
  as that of an engine that never made them."""
  from probayes_amd import Engine

  def start():
    eng = Engine(oracle.golden_spec('gmm2'))
    eng.init_chains(golden_init('gmm2', n))
    eng.set_rng('philox', seed=9)
    eng.alloc_trace(96, 1)
    eng.run(64, steps_per_launch=64)
    return eng

  eng, ref = start(), start()
  try:
    eng.rccl_init(0, 1, Engine.rccl_unique_id())
    st0 = eng.trace_stats(0, 64)
    ess0 = eng.trace_ess(0, 64).copy()
    tr0, mom0, x0 = eng.trace(0, 64), eng.moments(), eng.state()
    g0 = eng.rccl_allgather_stats()
    reduce(eng)
    tr1, mom1, x1 = eng.trace(0, 64), eng.moments(), eng.state()
    g1 = eng.rccl_allgather_stats()
    for k in ('v_x', 'v_p', 'u'):
      assert np.array_equal(tr0[k], tr1[k]), k
    for k in ('sum', 'sumsq', 'n_acc'):
      assert np.array_equal(mom0[k], mom1[k]), k
      assert np.array_equal(g0[k], g1[k]), k
    assert mom0['n_steps'] == mom1['n_steps']
    assert np.isfinite(g0['ess']).all() and np.array_equal(g0['ess'], g1['ess'])
    assert np.array_equal(x0[0], x1[0]) and np.array_equal(x0[1], x1[1])
    st1 = eng.trace_stats(0, 64)
    for k in ('sum', 'sumsq', 'n_acc'):
      assert np.array_equal(st0[k], st1[k]), k
    assert np.array_equal(ess0, eng.trace_ess(0, 64))
    # the run continues as it does without the calls
    eng.run(32, steps_per_launch=64)
    ref.run(32, steps_per_launch=64)
    ta, tb = eng.trace(), ref.trace()
    for k in ('v_x', 'v_p', 'u'):
      assert np.array_equal(ta[k], tb[k]), k
    sa, sb = eng.state(), ref.state()
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])
  finally:
    eng.close()
    ref.close()
