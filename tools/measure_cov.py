"""What the pooled covariance costs on the device (pbh_trace_cov: the shift, one
pass over the window with the sums in registers, the finish) against its
yardstick, at cfg2's shape (65 536 chains, d = 10, 1 250 records), cfg5's (gmm2,
32 768 chains, d = 2, records [500, 2 000)) and cfg2's chains and records at d =
16 and d = 32 (a diagonal Gaussian), where the triangle fills a lane's registers
and where the dims go in tiles.

    python tools/measure_cov.py [--shapes cfg2,cfg5,d16,d32] [--reps 7] [--no-host]

Per shape, on the same records of the same engine, each call timed by the host
clock around the whole call (every one ends with a device synchronise), one
warm-up each, then the median of `reps`, the calls alternating within a
repetition:
  (a) pbh_trace_cov for mean, cov and corr;
  (b) pbh_trace_rhat with no output asked for: its per-chain stage, one
      streaming read of the same window -- the project's one-pass yardstick.
`over_rhat` is (a) / (b); `window_reads` is how often (a) reads the window (1 up
to 16 dims; above, every tile job reads its own dims: 96 / 32 at d = 32), and
`fma_per_draw` the fused multiply-adds and adds a lane issues per draw.
  (c) the host route, once, where the window fits (cfg5; the others at
      --host-records records): Engine.trace() of the window, then np.cov of the
      pooled draws; and diag.pooled_cov of the same copy, whose covariance the
      device must meet within 64 eps of sqrt(cov_aa cov_bb).
Prints one JSON line per shape.  Needs the GPU.
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
import probayes_amd as pb  # noqa: E402
from probayes_amd import _lib, diag  # noqa: E402
from measure_pooled_quantile import make  # noqa: E402

HBM_PEAK_GBS = bench.HBM_PEAK_GBS
EPS = float(np.finfo(float).eps)


def make_shape(shape):
  if shape in ('cfg2', 'cfg5'):
    return make(shape)
  d = int(shape[1:])
  n, steps = 65536, 1250
  sigma = np.linspace(0.5, 2.5, d)
  spec = pb.make_spec(d, {'kind': 'diag_gauss', 'mu': np.linspace(-2., 2., d), 'sigma': sigma},
                      {'kind': 'gauss', 'scale': 0.4 * sigma}, pscale='log')
  eng = pb.Engine(spec)
  eng.init_chains(np.random.RandomState(5).normal(size=(n, d)))
  eng.set_rng('philox', seed=2024)
  eng.set_collect(moments=False)
  eng.alloc_trace(steps, 1, fill=False)
  eng.run(steps, steps_per_launch=250)
  return eng, 0, steps


def work(d):
  """(window reads, multiply-adds and adds per draw) of the partial kernel"""
  if d <= 16:
    return 1., d + d * (d + 1) // 2
  rects = -(-(d - 16) // 8)
  return (2 * 16 + 2 * rects * 16) / d, 2 * 152 + 2 * rects * 64


def measure(shape, reps, host, host_records):
  eng, first, count = make_shape(shape)
  n, d = eng.n, eng.dim
  dp = ctypes.POINTER(ctypes.c_double)
  mean, cov, corr = np.empty(d), np.empty((d, d)), np.empty((d, d))

  def cov_call(c=count):
    _lib.call('pbh_trace_cov', eng._h, ctypes.c_int64(first), ctypes.c_int64(c),
              mean.ctypes.data_as(dp), cov.ctypes.data_as(dp), corr.ctypes.data_as(dp))

  def chain_only():
    _lib.call('pbh_trace_rhat', eng._h, ctypes.c_int64(first), ctypes.c_int64(count),
              ctypes.c_int32(0), None, None, None)

  calls = {'rhat_chain_stage': chain_only, 'cov': cov_call}
  ms = {k: [] for k in calls}
  for rep in range(reps + 1):   # (the first round warms up)
    for k, fn in calls.items():
      t0 = time.perf_counter()
      fn()
      if rep:
        ms[k].append((time.perf_counter() - t0) * 1e3)
  med = {k: float(np.median(v)) for k, v in ms.items()}
  gb = d * n * count * 8 / 1e9
  reads, fma = work(d)
  out = {'shape': shape, 'chains': n, 'dim': d, 'records': [first, first + count],
         'draws': n * count, 'window_gb': round(gb, 3),
         'ms': {k: round(v, 3) for k, v in med.items()},
         'ms_runs': {k: [round(x, 3) for x in v] for k, v in ms.items()},
         'rhat_chain_stage_gbs': round(gb / (med['rhat_chain_stage'] * 1e-3), 1),
         'cov_window_gbs': round(gb / (med['cov'] * 1e-3), 1),
         'cov_read_gbs': round(reads * gb / (med['cov'] * 1e-3), 1),
         'cov_read_of_hbm_peak': round(reads * gb / (med['cov'] * 1e-3) / HBM_PEAK_GBS, 3),
         'over_rhat': round(med['cov'] / med['rhat_chain_stage'], 3),
         'window_reads': round(reads, 3), 'fma_per_draw': fma,
         'corr_max_offdiag': float(np.abs(corr - np.diag(np.diagonal(corr))).max())}
  if host:
    hc = count if shape == 'cfg5' else min(count, host_records)
    cov_call(hc)
    dev = cov.copy()
    t0 = time.perf_counter()
    x = eng.trace(first, hc)['v_x']
    t1 = time.perf_counter()
    ref = np.cov(x.reshape(-1, d), rowvar=False).reshape(d, d)
    t2 = time.perf_counter()
    own = diag.pooled_cov(x)['cov']
    unit = np.sqrt(np.outer(np.diagonal(own), np.diagonal(own)))
    dist = float((np.abs(dev - own) / unit).max())
    out['host'] = {'records': hc, 'copy_ms': round((t1 - t0) * 1e3, 1),
                   'np_cov_ms': round((t2 - t1) * 1e3, 1),
                   'device_minus_diag_eps': round(dist / EPS, 2),
                   'np_cov_minus_diag_eps': round(float((np.abs(ref - own) / unit).max()) / EPS,
                                                  2)}
    assert dist <= 64 * EPS, dist / EPS
  eng.close()
  print(json.dumps(out), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--shapes', default='cfg2,cfg5,d16,d32')
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--no-host', action='store_true')
  ap.add_argument('--host-records', type=int, default=50)
  a = ap.parse_args()
  for shape in a.shapes.split(','):
    measure(shape, a.reps, not a.no_host, a.host_records)


if __name__ == '__main__':
  main()
