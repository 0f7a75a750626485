"""What interpreting a density costs: cfg2's diagonal Gaussian (d = 10)
written by hand as an expression (the expr target, mh_kernel<10, PHILOX, EXPR,
0>) against the built-in mh_kernel<10, PHILOX, DIAG_GAUSS, GAUSS> on the same
numbers, in the same process, alternating, with the lane-pair kernel off.

    python tools/measure_expr.py [--chains 65536] [--steps 1000] [--reps 3]

Each engine runs `steps` warm-up steps, then `reps` timed runs of `steps`
steps (250 per launch, full trace, production Philox); the time is the
kernel-only pbh_last_run_ms.  Prints one JSON line.  Needs the GPU.
"""
import argparse
import json
import os
import sys

os.environ['PBH_NO_PAIR'] = '1'   # read at pbh_create: the general kernel
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import probayes_amd as pb  # noqa: E402
from probayes_amd import expr  # noqa: E402

MU = np.linspace(-1., 1., 10)
SIGMA = np.linspace(0.5, 2., 10)
STEP = 0.5
KEYS = ['x{}'.format(i) for i in range(10)]
LOGC = np.log(np.sqrt(2 * np.pi))


def density(**kw):
  lsg = np.log(SIGMA)
  return sum(-((kw[k] - MU[i]) / SIGMA[i]) ** 2 / 2. - LOGC - lsg[i]
             for i, k in enumerate(KEYS))


def timed(spec, n, steps, reps, spl):
  eng = pb.Engine(spec)
  eng.init_chains(np.zeros((n, 10)))
  eng.set_rng('philox', seed=2024)
  eng.alloc_trace(steps * (reps + 1), 1, fill=False)
  eng.run(steps, steps_per_launch=spl)          # warm-up, step 1 included
  ms = []
  for _ in range(reps):
    eng.run(steps, steps_per_launch=spl)
    ms.append(eng.last_run_ms()[0])
  mom = eng.moments()
  eng.close()
  return ms, float(mom['n_acc'].sum()) / (n * mom['n_steps'])


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--chains', type=int, default=65536)
  ap.add_argument('--steps', type=int, default=1000)
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--rounds', type=int, default=2)
  a = ap.parse_args()
  prop = {'kind': 'gauss', 'scale': STEP}
  tg = expr.trace_expr(density, KEYS)
  specs = {'expr': pb.make_spec(10, tg, prop, pscale='log'),
           'builtin': pb.make_spec(10, {'kind': 'diag_gauss', 'mu': MU, 'sigma': SIGMA},
                                   prop, pscale='log')}
  ms = {'expr': [], 'builtin': []}
  acc = {}
  for _ in range(a.rounds):                      # alternate the two forms
    for name in ('expr', 'builtin'):
      m, acc[name] = timed(specs[name], a.chains, a.steps, a.reps, 250)
      ms[name] += m
  work = a.chains * a.steps
  out = {'chains': a.chains, 'steps': a.steps, 'steps_per_launch': 250,
         'code_words': int(len(tg['code'])), 'slots': tg['depth'],
         'accept': acc}
  for name in ms:
    out[name + '_ms'] = [round(v, 3) for v in ms[name]]
    out[name + '_chain_steps_per_s'] = work / (min(ms[name]) * 1e-3)
  out['ratio_min'] = min(ms['expr']) / min(ms['builtin'])
  print(json.dumps(out))


if __name__ == '__main__':
  main()
