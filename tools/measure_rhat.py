"""What cross-chain convergence (split-R-hat, nested R-hat) of a trace costs on
the device against its yardsticks, at cfg2's shape (bench.cfg2_spec(), 65 536
chains, d = 10, 1 250 records) and cfg5's (gmm2, 32 768 chains, d = 2, records
[500, 2 000) of a 2 000-step trace).

    python tools/measure_rhat.py [--shapes cfg2,cfg5] [--reps 7] [--no-host]

Per shape, on the same records of the same engine, each call timed by the host
clock around the whole call (every one ends with a device synchronise):
  (a) pbh_trace_rhat with no output asked for: the per-chain stage alone (the
      one pass over the trace);
  (b) Engine.trace_rhat, split only, and with group = 1, 4, N / 2: (b) - (a) is
      the cross-chain stage and the [d] copy-out;
  (c) Engine.trace_stats, which reads the same bytes once;
  (d) the host path: Engine.trace() of the records, then diag.py (the chains
      in slices, their rows concatenated) -- once, not repeated.
One warm-up call each, then the median of `reps`, (a), (b) and (c) alternating
within a repetition.  Bytes: the d N count doubles of the window, read once,
over the time of (a), against the 8 TB/s HBM peak.  Also checks that the
device and diag.py on the host copy give the same numbers.  Prints one JSON
line per shape.  Needs the GPU.
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


def make(shape):
  """(engine, first, count) with the trace recorded."""
  if shape == 'cfg2':
    n, steps, burn = 65536, 1250, 0
    eng = pb.Engine(bench.cfg2_spec())
    eng.init_chains(np.random.RandomState(5).normal(size=(n, bench.D)))
  else:
    n, steps, burn = 32768, 2000, 500
    eng = pb.Engine(oracle.golden_spec('gmm2'))
    eng.init_chains(golden_init('gmm2', n))
  eng.set_rng('philox', seed=2024)
  eng.set_collect(moments=False)
  eng.alloc_trace(steps, 1, fill=False)
  eng.run(steps, steps_per_launch=250)
  return eng, burn, steps - burn


def host_path(eng, first, count, group, step=4096):
  x = eng.trace(first, count)['v_x']
  rows = np.concatenate([diag.chain_moments(x[c:c + step], 0, count)
                         for c in range(0, x.shape[0], step)], axis=1)
  return diag.split_rhat(rows, count // 2), diag.nested_rhat(rows, count, group)


def measure(shape, reps, host):
  eng, first, count = make(shape)
  n, d = eng.n, eng.dim
  groups = [1, 4, n // 2]

  def chain_only():
    _lib.call('pbh_trace_rhat', eng._h, ctypes.c_int64(first), ctypes.c_int64(count),
              ctypes.c_int32(0), None, None, None)

  calls = {'chain_stage': chain_only,
           'split': lambda: eng.trace_rhat(first, count),
           'trace_stats': lambda: eng.trace_stats(first, count)}
  for g in groups:
    calls['group_{}'.format(g)] = lambda g=g: eng.trace_rhat(first, count, g)
  ms = {k: [] for k in calls}
  for rep in range(reps + 1):   # (the first round warms up)
    for k, fn in calls.items():
      t0 = time.perf_counter()
      fn()
      if rep:
        ms[k].append((time.perf_counter() - t0) * 1e3)
  med = {k: float(np.median(v)) for k, v in ms.items()}
  gb = d * n * count * 8 / 1e9
  out = {'shape': shape, 'chains': n, 'dim': d, 'records': [first, first + count],
         'window_gb': round(gb, 3),
         'ms': {k: round(v, 4) for k, v in med.items()},
         'ms_runs': {k: [round(x, 4) for x in v] for k, v in ms.items()},
         'chain_stage_gbs': round(gb / (med['chain_stage'] * 1e-3), 1),
         'chain_stage_of_hbm_peak': round(gb / (med['chain_stage'] * 1e-3) / HBM_PEAK_GBS, 3),
         'trace_stats_gbs': round(gb / (med['trace_stats'] * 1e-3), 1),
         'chain_stage_over_trace_stats': round(med['chain_stage'] / med['trace_stats'], 3),
         'cross_stage_ms': {k: round(med[k] - med['chain_stage'], 4)
                            for k in med if k.startswith(('split', 'group_'))}}
  if host:
    g = 4
    t0 = time.perf_counter()
    split, nested = host_path(eng, first, count, g)
    out['host_trace_diag_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
    dev = eng.trace_rhat(first, count, g)
    out['max_rel_diff_device_host'] = float(max(
        np.max(np.abs(dev['split'] - split) / split),
        np.max(np.abs(dev['nested'] - nested) / nested)))
    out['split'] = [float(v) for v in dev['split']]
    out['nested_group_4'] = [float(v) for v in dev['nested']]
  eng.close()
  print(json.dumps(out), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--shapes', default='cfg2,cfg5')
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--no-host', action='store_true')
  a = ap.parse_args()
  for shape in a.shapes.split(','):
    if shape not in ('cfg2', 'cfg5'):
      sys.exit('unknown shape ' + shape)
    measure(shape, a.reps, not a.no_host)


if __name__ == '__main__':
  main()
