"""What sorted-summary quantiles of a trace cost on the device against the
host path they replace, at cfg5's shape: gmm2, 32 768 chains, d = 2, records
[500, 2 000) of a 2 000-step trace, q = 0.05 / 0.5 / 0.95.

    python tools/measure_quantile.py [--chains 32768] [--steps 2000] [--burn 500] [--reps 5]

Three calls on the same records of the same engine, each timed by the host
clock around the whole call (every one ends with its result on the host):
  (a) Engine.trace_quantile (weighted, the default; the unweighted call is
      reported beside it);
  (b) the host path: Engine.trace() of those records, then
      PD.sorted(k).quantile(q) for both keys;
  (c) Engine.trace_ess, for scale (it moves the same records through LDS once).
One warm-up call each, then the median of `reps`.  Prints one JSON line.
Needs the GPU.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import oracle  # noqa: E402
from oracle.workloads import golden_init  # noqa: E402
import probayes_amd as pb  # noqa: E402
from probayes_amd.pd import PD  # noqa: E402

QS = [0.05, 0.5, 0.95]


def median_ms(fn, reps):
  fn()   # warm-up
  ms = []
  for _ in range(reps):
    t0 = time.perf_counter()
    fn()
    ms.append((time.perf_counter() - t0) * 1e3)
  return float(np.median(ms)), ms


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--chains', type=int, default=32768)
  ap.add_argument('--steps', type=int, default=2000)
  ap.add_argument('--burn', type=int, default=500)
  ap.add_argument('--reps', type=int, default=5)
  a = ap.parse_args()
  spec = oracle.golden_spec('gmm2')
  names, first, count = spec['names'], a.burn, a.steps - a.burn
  eng = pb.Engine(spec)
  eng.init_chains(golden_init('gmm2', a.chains))
  eng.set_rng('philox', seed=2024)
  eng.alloc_trace(a.steps, 1, fill=False)
  eng.run(a.steps, steps_per_launch=250)

  def host():
    tr = eng.trace(first, count)
    prob = tr['v_p'].T
    vals = {k: tr['v_x'][:, :, i].T for i, k in enumerate(names)}
    pd_ = PD('v', vals, prob=prob, pscale=spec['pscale'])
    return [pd_.sorted(k).quantile(QS) for k in names]

  dev, dev_all = median_ms(lambda: eng.trace_quantile(QS, first, count), a.reps)
  dev_u, _ = median_ms(lambda: eng.trace_quantile(QS, first, count, weighted=False),
                       a.reps)
  ess, _ = median_ms(lambda: eng.trace_ess(first, count), a.reps)
  hst, hst_all = median_ms(host, a.reps)
  # the two paths answer the same question
  got = eng.trace_quantile(QS, first, count)
  ref = host()
  err = 0.
  for i, k in enumerate(names):
    h = np.array([[ref[i][c][j][k] for c in range(a.chains)] for j in range(len(QS))])
    err = max(err, float(np.max(np.abs(got[:, :, i] - h))))
  eng.close()
  print(json.dumps({
      'chains': a.chains, 'dim': spec['dim'], 'records': [first, first + count], 'q': QS,
      'device_quantile_ms': round(dev, 3), 'device_quantile_unweighted_ms': round(dev_u, 3),
      'host_trace_sorted_quantile_ms': round(hst, 1), 'device_ess_ms': round(ess, 3),
      'device_runs_ms': [round(x, 3) for x in dev_all],
      'host_runs_ms': [round(x, 1) for x in hst_all],
      'max_abs_diff_device_host': err,
      'device_faster_than_host': bool(dev < hst)}))
  if not dev < hst:
    sys.exit('the device quantile is not faster than the host path')


if __name__ == '__main__':
  main()
