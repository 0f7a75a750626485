"""What the quantiles of a trace pooled over chains and records cost on the
device (pbh_trace_quantile_pooled, a radix select in six streaming passes)
against their yardsticks, at cfg2's shape (bench.cfg2_spec(), 65 536 chains, d
= 10, 1 250 records), at cfg5's (gmm2, 32 768 chains, d = 2, records [500,
2 000) of a 2 000-step trace), and on one fully tied trace (cfg2's shape, every
chain started at one point, proposal scale 0: every element falls under every
target's prefix in every pass, the worst case for the counters).

    python tools/measure_pooled_quantile.py [--shapes cfg2,cfg5,tied]
                                            [--reps 7] [--no-host]

Per shape, on the same records of the same engine, each call timed by the host
clock around the whole call (every one ends with a device synchronise):
  (a) Engine.trace_quantile_pooled for the three quantiles 0.025, 0.5, 0.975
      and for 10 and 64 quantiles; the time per pass is the call's over the
      number of passes (the pick kernels, the scratch set-up and the copy-out
      are in it);
  (b) pbh_trace_rhat with no output asked for: its per-chain stage, the one
      pass over the same window that is the yardstick of a pass;
  (c) the host path: Engine.trace() of the records, then
      diag.pooled_quantile -- once, not repeated.
One warm-up call each, then the median of `reps`, (a) and (b) alternating
within a repetition.  Bytes: the d N count doubles of the window, read once
per pass, over the time per pass, against the 8 TB/s HBM peak.  Also checks
that the device and the host path give the same bits.  Prints one JSON line
per shape.  Needs the GPU.
"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import bench  # noqa: E402
import oracle  # noqa: E402
from oracle.workloads import golden_init  # noqa: E402
import probayes_amd as pb  # noqa: E402
from probayes_amd import _lib, diag  # noqa: E402

HBM_PEAK_GBS = bench.HBM_PEAK_GBS
PASSES = 6
QSETS = {'q3': [.025, .5, .975],
         'q10': [0, 1e-9, .025, .25, 1 / 3, .5, .75, .975, 1 - 1e-9, 1],
         'q64': list(np.linspace(0., 1., 64))}


def make(shape):
  """(engine, first, count) with the trace recorded."""
  if shape in ('cfg2', 'tied'):
    n, steps, burn = 65536, 1250, 0
    spec = bench.cfg2_spec()
    init = np.random.RandomState(5).normal(size=(n, bench.D))
    if shape == 'tied':
      spec = dict(spec, proposal=dict(spec['proposal'], scale=np.zeros(bench.D)))
      init = np.repeat(init[:1], n, axis=0)
    eng = pb.Engine(spec)
    eng.init_chains(init)
  else:
    n, steps, burn = 32768, 2000, 500
    eng = pb.Engine(oracle.golden_spec('gmm2'))
    eng.init_chains(golden_init('gmm2', n))
  eng.set_rng('philox', seed=2024)
  eng.set_collect(moments=False)
  eng.alloc_trace(steps, 1, fill=False)
  eng.run(steps, steps_per_launch=250)
  return eng, burn, steps - burn


def measure(shape, reps, host):
  eng, first, count = make(shape)
  n, d = eng.n, eng.dim

  def chain_only():
    _lib.call('pbh_trace_rhat', eng._h, ctypes.c_int64(first), ctypes.c_int64(count),
              ctypes.c_int32(0), None, None, None)

  calls = {'rhat_chain_stage': chain_only}
  for key, q in QSETS.items():
    calls[key] = lambda q=q: eng.trace_quantile_pooled(q, first, count)
  ms = {k: [] for k in calls}
  for rep in range(reps + 1):   # (the first round warms up)
    for k, fn in calls.items():
      t0 = time.perf_counter()
      fn()
      if rep:
        ms[k].append((time.perf_counter() - t0) * 1e3)
  med = {k: float(np.median(v)) for k, v in ms.items()}
  gb = d * n * count * 8 / 1e9
  per_pass = {k: med[k] / PASSES for k in QSETS}
  out = {'shape': shape, 'chains': n, 'dim': d, 'records': [first, first + count],
         'window_gb': round(gb, 3), 'passes': PASSES,
         'ms': {k: round(v, 4) for k, v in med.items()},
         'ms_runs': {k: [round(x, 4) for x in v] for k, v in ms.items()},
         'ms_per_pass': {k: round(v, 4) for k, v in per_pass.items()},
         'pass_gbs': {k: round(gb / (v * 1e-3), 1) for k, v in per_pass.items()},
         'pass_of_hbm_peak': {k: round(gb / (v * 1e-3) / HBM_PEAK_GBS, 3)
                              for k, v in per_pass.items()},
         'rhat_chain_stage_gbs': round(gb / (med['rhat_chain_stage'] * 1e-3), 1),
         'pass_over_rhat_chain_stage': {k: round(v / med['rhat_chain_stage'], 3)
                                        for k, v in per_pass.items()}}
  if host:
    q = QSETS['q10']
    t0 = time.perf_counter()
    want = diag.pooled_quantile(eng.trace(first, count)['v_x'], q)
    out['host_trace_diag_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
    got = eng.trace_quantile_pooled(q, first, count)
    out['device_equals_host'] = bool(np.array_equal(got, want))
    out['q3_of_dim_0'] = [float(v) for v in eng.trace_quantile_pooled(QSETS['q3'], first,
                                                                     count)[:, 0]]
  eng.close()
  print(json.dumps(out), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--shapes', default='cfg2,cfg5,tied')
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--no-host', action='store_true')
  a = ap.parse_args()
  for shape in a.shapes.split(','):
    if shape not in ('cfg2', 'cfg5', 'tied'):
      sys.exit('unknown shape ' + shape)
    measure(shape, a.reps, not a.no_host)


if __name__ == '__main__':
  main()
