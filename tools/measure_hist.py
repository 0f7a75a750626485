"""What the pooled histograms cost on the device (pbh_trace_hist, pbh_trace_hist2d)
against the project's yardsticks, at cfg2's shape (65 536 chains, d = 10, 1 250
records), cfg5's (gmm2, 32 768 chains, d = 2, records [500, 2 000)) and on one
fully tied trace (cfg2's shape, every chain at one point, proposal scale 0: a
whole wave on one counter, every value of the window).

    python tools/measure_hist.py [--shapes cfg2,cfg5,tied] [--reps 7] [--no-host]

Per shape, on the same records of the same engine, each call timed by the host
clock around the whole call (every one ends with a device synchronise), one
warm-up each, then the median of `reps`, the calls alternating within a
repetition:
  (a) trace_hist of every dim at 100 evenly placed bins between the pooled 0.1 %
      and 99.9 % quantiles: the guess path, one read of the window;
  (b) the same at 100 geometrically placed bins over the same range: the search;
  (c) trace_corner's second call: every pair a < b at 64 x 64 evenly placed bins,
      2 pairs / d reads of the window;
  (d) pbh_trace_rhat with no output asked for: its per-chain stage, one streaming
      read of the same window -- the project's one-pass yardstick;
  (e) trace_quantile_pooled with ten quantiles, whose time over its six passes is
      what one pass of a deeper search with the same kind of counting costs;
  (f) once, where the window fits (cfg5; the others at --host-records records):
      the host route, Engine.trace() of the window and np.histogram per dim, whose
      counts the device's must equal.
`hist_over_pass` is (a) over (e) / 6 and `pairs_over_reads` is (c) over (a) times
the reads (c) makes: both should be at most 1.  Prints one JSON line per shape.
Needs the GPU."""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import probayes_amd as pb  # noqa: E402,F401
from probayes_amd import _lib  # noqa: E402
from measure_pooled_quantile import make  # noqa: E402

QS = list(np.linspace(0.05, 0.95, 10))


def measure(shape, reps, host, host_records):
  eng, first, count = make(shape)
  n, d = eng.n, eng.dim
  lo, hi = eng.trace_quantile_pooled([0.001, 0.999], first, count)
  hi = np.where(hi > lo, hi, lo + 1.)   # (the tied trace: one value a dim)
  even = [np.linspace(lo[k], hi[k], 101) for k in range(d)]
  geo = [lo[k] + (hi[k] - lo[k]) * np.geomspace(1e-3, 1., 101) for k in range(d)]
  geo = [np.concatenate([[lo[k]], g[1:]]) for k, g in enumerate(geo)]
  sq = [np.linspace(lo[k], hi[k], 65) for k in range(d)]
  pairs = [(a, b) for a in range(d) for b in range(a + 1, d)]

  def chain_only():
    _lib.call('pbh_trace_rhat', eng._h, ctypes.c_int64(first), ctypes.c_int64(count),
              ctypes.c_int32(0), None, None, None)

  calls = {'rhat_chain_stage': chain_only,
           'hist_even': lambda: eng.trace_hist(even, first, count),
           'hist_geometric': lambda: eng.trace_hist(geo, first, count),
           'hist2d_pairs': lambda: eng.trace_hist2d(sq, pairs, first, count),
           'pooled_quantile_10': lambda: eng.trace_quantile_pooled(QS, first, count)}
  ms = {k: [] for k in calls}
  for rep in range(reps + 1):   # (the first round warms up)
    for k, fn in calls.items():
      t0 = time.perf_counter()
      fn()
      if rep:
        ms[k].append((time.perf_counter() - t0) * 1e3)
  med = {k: float(np.median(v)) for k, v in ms.items()}
  gb = d * n * count * 8 / 1e9
  reads = 2. * len(pairs) / d
  got = eng.trace_hist(even, first, count)
  out = {'shape': shape, 'chains': n, 'dim': d, 'records': [first, first + count],
         'draws': n * count, 'window_gb': round(gb, 3), 'pairs': len(pairs),
         'ms': {k: round(v, 3) for k, v in med.items()},
         'ms_runs': {k: [round(x, 3) for x in v] for k, v in ms.items()},
         'rhat_chain_stage_gbs': round(gb / (med['rhat_chain_stage'] * 1e-3), 1),
         'hist_even_gbs': round(gb / (med['hist_even'] * 1e-3), 1),
         'hist_geometric_gbs': round(gb / (med['hist_geometric'] * 1e-3), 1),
         'hist2d_read_gbs': round(reads * gb / (med['hist2d_pairs'] * 1e-3), 1),
         'select_pass_ms': round(med['pooled_quantile_10'] / 6., 3),
         'hist_over_rhat': round(med['hist_even'] / med['rhat_chain_stage'], 3),
         'hist_over_pass': round(med['hist_even'] / (med['pooled_quantile_10'] / 6.), 3),
         'search_over_guess': round(med['hist_geometric'] / med['hist_even'], 3),
         'pairs_window_reads': round(reads, 3),
         'pairs_over_reads': round(med['hist2d_pairs'] / (reads * med['hist_even']), 3),
         'inside': [int(h.sum()) for h in got['counts']]}
  if host:
    hc = count if shape == 'cfg5' else min(count, host_records)
    dev = eng.trace_hist(even, first, hc)
    t0 = time.perf_counter()
    x = eng.trace(first, hc)['v_x']
    t1 = time.perf_counter()
    ref = [np.histogram(x[:, :, k].ravel(), even[k])[0] for k in range(d)]
    t2 = time.perf_counter()
    equal = all(np.array_equal(h, r) for h, r in zip(dev['counts'], ref))
    out['host'] = {'records': hc, 'copy_ms': round((t1 - t0) * 1e3, 1),
                   'np_histogram_ms': round((t2 - t1) * 1e3, 1), 'counts_equal': equal}
    assert equal
  eng.close()
  print(json.dumps(out), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--shapes', default='cfg2,cfg5,tied')
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--no-host', action='store_true')
  ap.add_argument('--host-records', type=int, default=50)
  a = ap.parse_args()
  for shape in a.shapes.split(','):
    if shape not in ('cfg2', 'cfg5', 'tied'):
      sys.exit('unknown shape ' + shape)
    measure(shape, a.reps, not a.no_host, a.host_records)


if __name__ == '__main__':
  main()
