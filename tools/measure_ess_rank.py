"""What the bulk- and tail-ESS across chains cost on the device
(pbh_trace_ess_rank: per dim and variant the power spectra of the split chains
summed by ess_spectrum_kernel, one inverse transform by ess_finish_kernel, the
estimator on the host; the bulk variant behind the pooled sort of
pbh_trace_rhat_rank, the tail variants behind one radix select) against its
yardsticks, at the three shapes of tools/measure_rank_rhat.py: cfg2's (65 536
chains, d = 10, 1 250 records), cfg5's (gmm2, 32 768 chains, d = 2, records
[500, 2 000)) and cfg2's shape fully tied.

    python tools/measure_ess_rank.py [--shapes cfg2,cfg5,tied] [--reps 7]
                                     [--no-host] [--host-dims K]

Per shape, on the same records of the same engine, each call timed by the host
clock around the whole call (every one ends with a device synchronise), one
warm-up each, then the median of `reps`, the calls alternating within a
repetition:
  (a) pbh_trace_ess_rank for bulk only, tail only, basic only and all four
      variants;
  (b) pbh_trace_rhat_rank for bulk only: the same sort and scores without the
      ESS stage -- (a)'s bulk only minus this is what the ESS stage adds;
  (c) pbh_trace_rhat with no output asked for: one streaming read of the same
      window, the yardstick for bandwidth.
The basic-only call is one rhat_chain pass, then per dim one spectrum and one
finish kernel and nothing else on the device: its time over d bounds the two
kernels' from above, and `spectrum_gbs_of_trace_read` prices the window's bytes
(each element is read once per variant) at it.  The kernels' device times on
their own come from a kernel trace in a run of its own (--reps 1 --no-host
under the profiler's kernel trace with statistics).
  (d) the host route, once: Engine.trace() of the window, then diag.rank_ess.
      With --host-dims K only the first K dims are reduced on the host and the
      time is scaled by d / K; the comparison is then over those dims.
Also checks the device against the host: every ESS of the compared dims
relatively within 1e-9.  Prints one JSON line per shape.  Needs the GPU.
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


def measure(shape, reps, host, host_dims):
  eng, first, count = make(shape)
  n, d = eng.n, eng.dim
  dp = ctypes.POINTER(ctypes.c_double)
  bulk, tail, basic = np.empty(d), np.empty(d), np.empty(d)
  parts, rhat = np.empty((2, d)), np.empty(d)
  ptr = lambda a: a.ctypes.data_as(dp)

  def ess(want_bulk, want_tail, want_basic):
    _lib.call('pbh_trace_ess_rank', eng._h, ctypes.c_int64(first), ctypes.c_int64(count),
              ptr(bulk) if want_bulk else None, ptr(tail) if want_tail else None,
              ptr(parts) if want_tail else None, ptr(basic) if want_basic else None, None)

  def rhat_rank_bulk():
    _lib.call('pbh_trace_rhat_rank', eng._h, ctypes.c_int64(first), ctypes.c_int64(count),
              ptr(rhat), None, None, None)

  def chain_only():
    _lib.call('pbh_trace_rhat', eng._h, ctypes.c_int64(first), ctypes.c_int64(count),
              ctypes.c_int32(0), None, None, None)

  calls = {'rhat_chain_stage': chain_only, 'rhat_rank_bulk': rhat_rank_bulk,
           'ess_bulk': lambda: ess(True, False, False),
           'ess_tail': lambda: ess(False, True, False),
           'ess_basic': lambda: ess(False, False, True),
           'ess_all': lambda: ess(True, True, True)}
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
  stage = med['ess_basic'] - med['rhat_chain_stage']
  out = {'shape': shape, 'chains': n, 'dim': d, 'records': [first, first + count],
         'half': count // 2, 'split_chains': 2 * n, 'window_gb': round(gb, 3),
         'ms': {k: round(v, 3) for k, v in med.items()},
         'ms_runs': {k: [round(x, 3) for x in v] for k, v in ms.items()},
         'rhat_chain_stage_gbs': round(gb / (med['rhat_chain_stage'] * 1e-3), 1),
         'ess_stage_added_to_bulk_ms': round(med['ess_bulk'] - med['rhat_rank_bulk'], 3),
         'spectrum_and_finish_ms_per_dim_at_most': round(stage / d, 3),
         'spectrum_gbs_of_trace_read': round(gb / (stage * 1e-3), 1),
         'spectrum_of_hbm_peak': round(gb / (stage * 1e-3) / HBM_PEAK_GBS, 4),
         'transforms_per_s': round(d * n / (stage * 1e-3), 0)}
  if host:
    kd = d if not host_dims else min(d, host_dims)
    t0 = time.perf_counter()
    x = eng.trace(first, count)['v_x']
    t_copy = time.perf_counter() - t0
    t0 = time.perf_counter()
    want = diag.rank_ess(x[:, :, :kd])
    t_ess = time.perf_counter() - t0
    out['host'] = {'dims_reduced': kd, 'trace_copy_ms': round(t_copy * 1e3, 1),
                   'rank_ess_ms': round(t_ess * 1e3, 1),
                   'route_ms_scaled_to_d': round((t_copy + t_ess * d / kd) * 1e3, 1)}
    out['call_over_host_route'] = round(med['ess_all'] / out['host']['route_ms_scaled_to_d'], 5)
    ess(True, True, True)
    got = {'bulk': bulk, 'tail': tail, 'tail_lower': parts[0], 'tail_upper': parts[1],
           'basic': basic}
    with np.errstate(all='ignore'):
      dist = {k: float(np.max(np.where(
          (v[:kd] == want[k]) | (np.isnan(v[:kd]) & np.isnan(want[k])), 0.,
          np.abs(v[:kd] - want[k]) / np.abs(want[k])))) for k, v in got.items()}
    out['device_minus_host_relative'] = dist
    out['device_within_1e-9_of_host'] = bool(all(v <= 1e-9 for v in dist.values()))
    out['ess'] = {k: [float(u) for u in v] for k, v in got.items()}
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
