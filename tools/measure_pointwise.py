"""What the pointwise reduction (pbh_trace_pointwise: per observation the
log-sum-exp, mean and variance of its log-likelihood term over every draw of
the trace) costs on the device against its yardstick, the sampler's own step on
the same model: data_linreg3 (137 observations), 65 536 chains, 1 250 records.

    python tools/measure_pointwise.py [--chains 65536] [--records 1250]
                                      [--runs 3] [--host-chains 2048]
                                      [--host-records 125]

The yardstick evaluates the same 137-term body once per chain-step, so the
pointwise time per draw over the run time per chain-step says what the fold
(an online log-sum-exp and Welford's step per term) and the re-read of the
trace per observation tile add.  `runs` times, interleaved: eng.run of
`records` steps, timed by the device stamps on its first and last dispatch
(pbh_last_run_ms), then Engine.trace_pointwise over all the records, timed by
the host clock around the whole call (it ends with a device synchronise; the
upload of the program and the copy-out of 3 x 137 doubles are in it).  Also
the host's time for the same statistics -- Engine.trace(), expr.
evaluate_pointwise, diag.pointwise_stats -- at a shape where the terms [draws,
137] fit the host's memory, and the largest difference between the two there.
Prints one JSON line.  Needs the GPU.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import scipy.stats  # noqa: E402

import probayes_amd as pb  # noqa: E402
from probayes_amd import diag, expr  # noqa: E402
from expr_data_examples import DATA_WORKLOADS, LIN_X, LIN_Y  # noqa: E402


def engine(n, t):
  builder, params = DATA_WORKLOADS['data_linreg3'][:2]
  spec = builder(pb, params)[0].lower()
  rs = np.random.RandomState(6)
  eng = pb.Engine(spec)
  eng.init_chains(np.stack([rs.normal(0.7, 0.1, n), rs.normal(-1.2, 0.1, n),
                            rs.uniform(0.6, 1.1, n)], -1))
  eng.set_rng('philox', seed=2024)
  eng.set_collect(moments=False)
  eng.alloc_trace(t, 1, fill=False)
  return eng


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
  eng.run(t, steps_per_launch=250)           # warm-up: the trace is full
  eng.trace_pointwise(prog, 0, min(t, 8))
  run_ms, pw_ms = [], []
  for _ in range(a.runs):
    eng.alloc_trace(t, 1, fill=False)
    eng.run(t, steps_per_launch=250)
    run_ms.append(eng.last_run_ms()[0])
    t0 = time.perf_counter()
    res = eng.trace_pointwise(prog, 0, t)
    pw_ms.append((time.perf_counter() - t0) * 1e3)
  eng.close()
  draws = n * t
  out = {'chains': n, 'records': t, 'n_obs': 137,
         'run_ms': [round(v, 3) for v in run_ms], 'pointwise_ms': [round(v, 3) for v in pw_ms],
         'run_ns_per_chain_step': round(float(np.median(run_ms)) * 1e6 / draws, 4),
         'pointwise_ns_per_draw': round(float(np.median(pw_ms)) * 1e6 / draws, 4),
         'ratio': round(float(np.median(pw_ms) / np.median(run_ms)), 3),
         'waic': diag.waic(res['lse'], res['mean'], res['var'], draws)['waic']}
  # the host, where it can hold the terms
  hn, ht = a.host_chains, a.host_records
  eng = engine(hn, ht)
  eng.run(ht, steps_per_launch=250)
  eng.trace_pointwise(prog, 0, ht)
  t0 = time.perf_counter()
  dev = eng.trace_pointwise(prog, 0, ht)
  dev_ms = (time.perf_counter() - t0) * 1e3
  t0 = time.perf_counter()
  x = eng.trace()['v_x']
  T = expr.evaluate_pointwise(prog['code'], prog['consts'], x.reshape(-1, 3), prog['data'])
  host = diag.pointwise_stats(T)
  host_ms = (time.perf_counter() - t0) * 1e3
  eng.close()
  out['host'] = {'chains': hn, 'records': ht, 'host_ms': round(host_ms, 1),
                 'device_ms': round(dev_ms, 3),
                 'max_rel_diff': float(max(
                     np.max(np.abs(dev[k] - h) / np.maximum(np.abs(h), 1.))
                     for k, h in zip(('lse', 'mean', 'var'), host)))}
  print(json.dumps(out), flush=True)


if __name__ == '__main__':
  main()
