"""What the tests of the trace reductions share (test_gpu_quantile.py,
test_gpu_rhat.py, test_gpu_pooled_quantile.py, test_gpu_rank_rhat.py,
test_gpu_ess_rank.py, test_gpu_trace_scratch.py; test_trace_host.py for the
quantile lists): an engine with a recorded trace, the big shape with its
windows and one cached run of it per model and set of reductions, the
quantile lists and the starts of chains that never move, the facade's sampler
with its block copied out, and the check that a reduction changes nothing but
its own result."""
import contextlib
import functools

import numpy as np

import oracle
from oracle.workloads import golden_init

# N = 2 004 chains (no multiple of 64 or 256, divisible by 4 and 12), T = 160;
# an even window, an odd one (the middle record dropped) and h = 2
N_BIG, T_BIG = 2004, 160
WINDOWS = ((40, 120), (40, 119), (0, 4))

QS = [0, 1e-9, .025, .25, 1 / 3, .5, .75, .975, 1 - 1e-9, 1]
Q64 = list(np.linspace(0., 1., 64))


def run(spec, init, t, seed=3):
  """An engine of spec started at init with t steps run and recorded."""
  from probayes_amd import Engine
  eng = Engine(spec)
  eng.init_chains(init)
  eng.set_rng('philox', seed=seed)
  eng.alloc_trace(t, 1)
  eng.run(t, steps_per_launch=64)
  return eng


@functools.lru_cache(maxsize=None)
def big_run(name, reduce, windows=WINDOWS):
  """One run of N_BIG chains for T_BIG records per model and `reduce`: the spec,
  the host copy of the trace, and {(first, count): reduce(eng, first, count)} in
  the windows' order."""
  spec = oracle.golden_spec(name)
  eng = run(spec, golden_init(name, N_BIG), T_BIG)
  try:
    x = eng.trace()['v_x']
    res = {(first, count): reduce(eng, first, count) for first, count in windows}
  finally:
    eng.close()
  return spec, x, res


def flat(res):
  """every array of a result, in a fixed order"""
  if isinstance(res, dict):
    return [a for k in sorted(res) if res[k] is not None for a in flat(res[k])]
  return list(res) if isinstance(res, tuple) else [res]


def _ladder(n):
  v = np.empty(n)
  v[0] = 1.
  for i in range(1, n):
    v[i] = np.nextafter(v[i - 1], 2.)
  return v


TOP = np.array([1e300, -1e300, 1e-300, -1e-300, 5e-324, 0., -0., -5e-324, 3., -3., 1e300,
                -1e-300, 0.])


def tied_starts(kind):
  """[130, 2] starts for chains that never move (a proposal of scale 0)"""
  if kind == 'one_value':
    return np.repeat(np.array([[-1., 0.5]]), 130, axis=0)
  if kind == 'last_ulps':
    lad = _ladder(130)
    # dim 0 climbs through 130 neighbours of 1.0; dim 1 holds 5 of them, 26 times each
    return np.stack([lad[np.random.default_rng(1).permutation(130)], -lad[np.arange(130) % 5]],
                    axis=1)
  assert kind == 'top_bits'
  a = np.resize(TOP, 130)
  return np.stack([a, np.resize(TOP[::-1], 130)], axis=1)


@contextlib.contextmanager
def sampler_block(n, t=96):
  """The facade's batched sampler of metrohast_norm1d with n chains after one
  block of t steps: (sampler, process, x, keys, v) with v the block's values
  and x [n, t, d] the same values in the trace's layout.  Closed on exit."""
  import probayes_amd as pb
  from mcmc_examples import WORKLOADS
  builder, params, _, _, _ = WORKLOADS['metrohast_norm1d']
  g = oracle.load_golden('metrohast_norm1d')
  params = oracle.workloads.golden_params(g) if params else params
  process, init, extra, kwds, keys = builder(pb, params)
  sampler = process.sampler(init, extra, stop=t, chains=n, rng='philox', seed=7, **kwds)
  try:
    samples = process.walk(sampler)
    assert len(samples) == t
    v = process(samples).v
    x = np.stack([np.asarray(v[k]).T for k in keys], axis=2)   # [n, t, d]
    assert x.shape == (n, t, len(keys))
    yield sampler, process, x, keys, v
  finally:
    sampler.close()


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
