"""What the rank-normalised split-R-hat costs on the device (pbh_trace_rhat_rank:
per dim a pooled radix sort of (key, index) pairs, the run search and the
normal scores, then pbh_trace_rhat's two stages on the scores) against its
yardsticks, at the three shapes of tools/measure_pooled_quantile.py: cfg2's
(65 536 chains, d = 10, 1 250 records), cfg5's (gmm2, 32 768 chains, d = 2,
records [500, 2 000)) and cfg2's shape fully tied (every pass of the sort
skipped, one run of M in the run search).

    python tools/measure_rank_rhat.py [--shapes cfg2,cfg5,tied] [--reps 7]
                                      [--no-host] [--host-dims K]

Per shape, on the same records of the same engine, each call timed by the host
clock around the whole call (every one ends with a device synchronise), one
warm-up each, then the median of `reps`, the calls alternating within a
repetition:
  (a) pbh_trace_rhat_rank for bulk only and for bulk and folded (the second
      adds the pooled median's select and the folded variant's sort);
  (b) pbh_trace_rhat with no output asked for: its per-chain stage, one
      streaming read of the same window -- the yardstick, and the achieved
      bandwidth the model is priced at.
The model: the bytes pbh_rank.hip's header comment says a dim moves per element
(keys 16; a pass that runs 32, the first 28, a skipped one 8; scores 20; the
reduction's read 8), times M d, over the yardstick's bandwidth.  It is a
model: which passes run depends on the data, the scatter and the score
kernels write partial lines, and the tables' traffic is left out; `passes_run`
is the assumption it was priced with (all eight, none when tied).  A split per
kernel comes from a kernel trace in a run of its own (--reps 1 --no-host).
  (c) the host route, once: Engine.trace() of the window, then diag.rank_rhat.
      With --host-dims K only the first K dims are ranked on the host and the
      time is scaled by d / K (cfg2's ten dims take minutes); the comparison
      is then over those dims.
Also checks the device against the host: the ranks bit for bit where they fit
the host's memory (cfg5, and any shape under 2^28 elements in all), else bulk
and folded of the compared dims within 64 eps.  Prints one JSON line per shape.
Needs the GPU.
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
import probayes_amd as pb  # noqa: E402,F401
from probayes_amd import _lib, diag  # noqa: E402
from measure_pooled_quantile import make  # noqa: E402

HBM_PEAK_GBS = bench.HBM_PEAK_GBS
KEYS_B, PASS_B, FIRST_PASS_B, SKIPPED_B, SCORE_B, REDUCE_B = 16, 32, 28, 8, 20, 8


def model_bytes(passes_run):
  """per element of a dim and variant"""
  run = FIRST_PASS_B + (passes_run - 1) * PASS_B if passes_run else 0
  return KEYS_B + run + (8 - passes_run) * SKIPPED_B + SCORE_B + REDUCE_B


def measure(shape, reps, host, host_dims):
  eng, first, count = make(shape)
  n, d = eng.n, eng.dim
  dp = ctypes.POINTER(ctypes.c_double)
  bulk, folded = np.empty(d), np.empty(d)

  def rank(with_folded):
    _lib.call('pbh_trace_rhat_rank', eng._h, ctypes.c_int64(first), ctypes.c_int64(count),
              bulk.ctypes.data_as(dp), folded.ctypes.data_as(dp) if with_folded else None,
              None, None)

  def chain_only():
    _lib.call('pbh_trace_rhat', eng._h, ctypes.c_int64(first), ctypes.c_int64(count),
              ctypes.c_int32(0), None, None, None)

  calls = {'rhat_chain_stage': chain_only, 'bulk': lambda: rank(False),
           'bulk_and_folded': lambda: rank(True)}
  ms = {k: [] for k in calls}
  for rep in range(reps + 1):   # (the first round warms up)
    for k, fn in calls.items():
      t0 = time.perf_counter()
      fn()
      if rep:
        ms[k].append((time.perf_counter() - t0) * 1e3)
  med = {k: float(np.median(v)) for k, v in ms.items()}
  m = n * count
  gb = d * m * 8 / 1e9
  yard_gbs = gb / (med['rhat_chain_stage'] * 1e-3)
  passes_run = 0 if shape == 'tied' else 8
  per_elem = model_bytes(passes_run)
  model_ms = per_elem * m * d / 1e9 / yard_gbs * 1e3
  out = {'shape': shape, 'chains': n, 'dim': d, 'records': [first, first + count],
         'elements_per_dim': m, 'window_gb': round(gb, 3),
         'ms': {k: round(v, 3) for k, v in med.items()},
         'ms_runs': {k: [round(x, 3) for x in v] for k, v in ms.items()},
         'rhat_chain_stage_gbs': round(yard_gbs, 1),
         'rhat_chain_stage_of_hbm_peak': round(yard_gbs / HBM_PEAK_GBS, 3),
         'model': {'passes_run': passes_run, 'bytes_per_element': per_elem,
                   'bulk_ms': round(model_ms, 3), 'bulk_and_folded_ms': round(2 * model_ms, 3)},
         'measured_over_model': {'bulk': round(med['bulk'] / model_ms, 2),
                                 'bulk_and_folded': round(med['bulk_and_folded'] /
                                                          (2 * model_ms), 2)},
         'ms_per_dim_and_variant': round(med['bulk'] / d, 3),
         'achieved_gbs_of_model_bytes': round(per_elem * m * d / 1e9 / (med['bulk'] * 1e-3), 1)}
  if host:
    kd = d if not host_dims else min(d, host_dims)
    t0 = time.perf_counter()
    x = eng.trace(first, count)['v_x']
    t_copy = time.perf_counter() - t0
    t0 = time.perf_counter()
    want = diag.rank_rhat(x[:, :, :kd])
    t_rank = time.perf_counter() - t0
    out['host'] = {'dims_ranked': kd, 'trace_copy_ms': round(t_copy * 1e3, 1),
                   'rank_rhat_ms': round(t_rank * 1e3, 1),
                   'route_ms_scaled_to_d': round((t_copy + t_rank * d / kd) * 1e3, 1)}
    out['call_over_host_route'] = round(med['bulk_and_folded'] /
                                        out['host']['route_ms_scaled_to_d'], 5)
    rank(True)
    eps = float(np.finfo(float).eps)
    with np.errstate(all='ignore'):
      dist = {k: np.abs(v[:kd] - want[k]) / np.abs(want[k])
              for k, v in (('bulk', bulk), ('folded', folded))}
    same = {k: bool(np.all((v[:kd] == want[k]) | (np.isnan(v[:kd]) & np.isnan(want[k])) |
                           (dist[k] <= 64 * eps)))
            for k, v in (('bulk', bulk), ('folded', folded))}
    out['device_rhat_within_64_eps_of_host'] = same
    out['rhat'] = {'bulk': [float(v) for v in bulk], 'folded': [float(v) for v in folded]}
    if d * m <= 2 ** 28:
      got = eng.trace_rhat_rank(first, count, ranks=True)
      out['device_ranks_equal_host'] = bool(
          np.array_equal(got['ranks'][:, :, :kd], diag.average_ranks(x[:, :, :kd]),
                         equal_nan=True) and
          np.array_equal(got['folded_ranks'][:, :, :kd],
                         diag.average_ranks(x[:, :, :kd], fold=True), equal_nan=True))
  eng.close()
  print(json.dumps(out), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--shapes', default='cfg2,cfg5,tied')
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--no-host', action='store_true')
  ap.add_argument('--host-dims', type=int, default=0)
  a = ap.parse_args()
  for shape in a.shapes.split(','):
    if shape not in ('cfg2', 'cfg5', 'tied'):
      sys.exit('unknown shape ' + shape)
    measure(shape, a.reps, not a.no_host, a.host_dims)


if __name__ == '__main__':
  main()
