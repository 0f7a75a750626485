"""What PSIS-LOO costs on the device against its yardstick, the pointwise
reduction of the same terms, on data_linreg3 (137 observations), 65 536 chains,
1 250 records: 82 million draws, a [draws, observations] matrix of 90 GB that is
never stored.

    python tools/measure_psis.py [--chains 65536] [--records 1250] [--runs 3]
                                 [--host-chains 2048] [--host-records 125]

What Sampler.trace_loo does, step by step on one engine, each step timed by the
host clock around the whole call (every device call ends synchronised), one
warm-up, then `runs` times, the median reported:
  tail       Engine.trace_pointwise_tail with k = m + 1: `passes` count passes,
             one gather pass, the copy-out and the host's sort of the lists;
  pointwise  Engine.trace_pointwise, for lse -- the yardstick: one pass of the
             same walk;
  finish     diag.psis_loo_from_tail on the host: per observation the
             generalised-Pareto fit over m values on 30 + sqrt(m) grid points.
trace_loo is the sum.  The expectation from the code is tail + pointwise ~
(passes + 2) pointwise passes; `device_over_expected` is the ratio, and
`tail_over_pointwise` less passes + 1 says how much the count and gather
kernels' integer atomics and the host's part of the select add.  A split per
kernel comes from a kernel trace in a run of its own.  Also the host's time for
the same numbers -- Engine.trace(), expr.evaluate_pointwise, diag.psis_loo -- at
a shape where the terms fit the host's memory, the largest differences between
the two there, and the sensitivity of the host definition (8 random-sign
relative perturbations of T by 1e-12).  Prints one JSON line.  Needs the GPU.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import numpy as np  # noqa: E402
import scipy.stats  # noqa: E402

from probayes_amd import diag, expr  # noqa: E402
from expr_data_examples import LIN_X, LIN_Y  # noqa: E402
from measure_pointwise import engine  # noqa: E402


def loo(eng, prog, t, times=None):
  S = eng.n * t
  k = diag.psis_tail_length(S) + 1
  t0 = time.perf_counter()
  tail = eng.trace_pointwise_tail(prog, k, 0, t)
  t1 = time.perf_counter()
  lse = eng.trace_pointwise(prog, 0, t)['lse']
  t2 = time.perf_counter()
  res = diag.psis_loo_from_tail(tail['tail'], tail['rest_lse'], S, lse)
  t3 = time.perf_counter()
  if times is not None:
    for key, v in (('tail', t1 - t0), ('pointwise', t2 - t1), ('finish', t3 - t2)):
      times[key].append(v * 1e3)
  return res, tail['passes'], k


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--chains', type=int, default=65536)
  ap.add_argument('--records', type=int, default=1250)
  ap.add_argument('--runs', type=int, default=3)
  ap.add_argument('--host-chains', type=int, default=2048)
  ap.add_argument('--host-records', type=int, default=125)
  a = ap.parse_args()
  prog = expr.trace_pointwise(
      lambda **kw: scipy.stats.norm.logpdf(LIN_Y, kw['b0'] + kw['b1'] * LIN_X, kw['s']),
      ['b0', 'b1', 's'])
  n, t = a.chains, a.records
  eng = engine(n, t)
  eng.run(t, steps_per_launch=250)
  loo(eng, prog, min(t, 8))                    # warm-up
  times = {'tail': [], 'pointwise': [], 'finish': []}
  for _ in range(a.runs):
    res, passes, k = loo(eng, prog, t, times)
  eng.close()
  med = {key: float(np.median(v)) for key, v in times.items()}
  device = med['tail'] + med['pointwise']
  out = {'chains': n, 'records': t, 'n_obs': 137, 'draws': n * t, 'k': k, 'passes': passes,
         'ms_runs': {key: [round(x, 3) for x in v] for key, v in times.items()},
         'ms': {key: round(v, 3) for key, v in med.items()},
         'trace_loo_ms': round(device + med['finish'], 3),
         'device_ms': round(device, 3),
         'tail_over_pointwise': round(med['tail'] / med['pointwise'], 3),
         'device_over_expected': round(device / ((passes + 2) * med['pointwise']), 3),
         'elpd_loo': res['elpd_loo'], 'p_loo': res['p_loo'], 'n_bad_k': res['n_bad_k'],
         'pareto_k_max': float(np.max(res['pareto_k']))}
  # the host, where it can hold the terms
  hn, ht = a.host_chains, a.host_records
  eng = engine(hn, ht)
  eng.run(ht, steps_per_launch=250)
  loo(eng, prog, ht)
  t0 = time.perf_counter()
  dev, hp, _ = loo(eng, prog, ht)
  dev_ms = (time.perf_counter() - t0) * 1e3
  t0 = time.perf_counter()
  x = eng.trace()['v_x']
  T = expr.evaluate_pointwise(prog['code'], prog['consts'], x.reshape(-1, 3), prog['data'])
  host = diag.psis_loo(T)
  host_ms = (time.perf_counter() - t0) * 1e3
  eng.close()
  rng = np.random.default_rng(2017)
  sens = {'pareto_k': 0., 'elpd_loo_i': 0.}
  for _ in range(8):
    other = diag.psis_loo(T * (1. + 1e-12 * rng.choice([-1., 1.], T.shape)))
    for key in sens:
      sens[key] = max(sens[key], float(np.max(np.abs(other[key] - host[key]))))
  out['host'] = {'chains': hn, 'records': ht, 'passes': hp, 'host_ms': round(host_ms, 1),
                 'device_route_ms': round(dev_ms, 3),
                 'max_abs_diff': {key: float(np.max(np.abs(dev[key] - host[key])))
                                  for key in ('pareto_k', 'elpd_loo_i')},
                 'host_sensitivity_1e-12': sens}
  print(json.dumps(out), flush=True)


if __name__ == '__main__':
  main()
