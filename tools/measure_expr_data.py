"""What interpreting a likelihood over data costs: np.sum(norm.logpdf(OBS, mu,
sg)) over n observations written as an expression (the data kernels of the expr
target, mh_kernel<2, PHILOX_F64, kTargetExprData, 0>), its body evaluated 8
observations wide and one observation at a time (PBH_EXPR_DATA_WIDE=0), against
the built-in iid-Normal kernel mh_kernel<2, PHILOX_F64, NORM_IID, SPHERE> on
the same numbers, in the same process, alternating.  All three walk the same
pairwise sum over norm_logpdf and give the same chains.

    python tools/measure_expr_data.py [--chains 65536] [--obs 1024] [--steps 1000]

Each engine runs a warm-up, then `reps` timed runs of `steps` steps (250 per
launch, full trace, Philox with fp64 reference arithmetic); the time is the
kernel-only pbh_last_run_ms.  Prints one JSON line.  Needs the GPU.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import scipy.stats  # noqa: E402

import probayes_amd as pb  # noqa: E402
from probayes_amd import expr  # noqa: E402

CLOCK_GHZ = 2.4   # MI355X peak engine clock, for the cycles estimate


def timed(spec, wide, n, steps, warmup, reps, spl):
  os.environ['PBH_EXPR_DATA_WIDE'] = '1' if wide else '0'   # read at set_model
  eng = pb.Engine(spec)
  rs = np.random.RandomState(1)
  eng.init_chains(np.stack([rs.normal(0.5, 0.05, n), rs.uniform(1.4, 1.6, n)], -1))
  eng.set_rng('philox_f64', seed=2024)
  eng.alloc_trace(warmup + steps * reps, 1, fill=False)
  eng.run(warmup, steps_per_launch=spl)          # warm-up, step 1 included
  ms = []
  for _ in range(reps):
    eng.run(steps, steps_per_launch=spl)
    ms.append(eng.last_run_ms()[0])
  mom = eng.moments()
  eng.close()
  return ms, float(mom['n_acc'].sum()) / (n * mom['n_steps']), \
      float(mom['sum'].sum()), float(mom['sumsq'].sum())


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--chains', type=int, default=65536)
  ap.add_argument('--obs', type=int, default=1024)
  ap.add_argument('--steps', type=int, default=1000)
  ap.add_argument('--warmup', type=int, default=100)
  ap.add_argument('--reps', type=int, default=2)
  ap.add_argument('--rounds', type=int, default=2)
  a = ap.parse_args()
  obs = np.random.RandomState(7).normal(0.5, 1.5, a.obs)
  prop = {'kind': 'sphere', 'delta': 0.02}
  tg = expr.trace_expr(
      lambda **kw: np.sum(scipy.stats.norm.logpdf(obs, kw['mu'], kw['sg'])), ['mu', 'sg'])
  ops = [expr.decode(w)[0] for w in tg['code']]
  body_words = expr.decode(tg['code'][ops.index(expr.LOOP)])[3][1]
  e_spec = pb.make_spec(2, tg, prop, pscale='log')
  b_spec = pb.make_spec(2, {'kind': 'norm_iid', 'obs': obs, 'loc': 0, 'scale': 1}, prop,
                        pscale='log')
  forms = {'builtin': (b_spec, True), 'expr_wide': (e_spec, True),
           'expr_one': (e_spec, False)}
  ms = {k: [] for k in forms}
  acc, sums = {}, {}
  for _ in range(a.rounds):                      # alternate the three forms
    for name, (spec, wide) in forms.items():
      m, acc[name], s1, s2 = timed(spec, wide, a.chains, a.steps, a.warmup, a.reps, 250)
      ms[name] += m
      sums[name] = (s1, s2)
  work = a.chains * a.steps
  out = {'chains': a.chains, 'obs': a.obs, 'steps': a.steps, 'steps_per_launch': 250,
         'rng': 'philox_f64', 'code_words': int(len(tg['code'])),
         'body_words': int(body_words), 'accept': acc,
         'same_chains': len(set(sums.values())) == 1}
  for name in ms:
    out[name + '_ms'] = [round(v, 3) for v in ms[name]]
    out[name + '_chain_steps_per_s'] = work / (min(ms[name]) * 1e-3)
  best = {k: min(v) for k, v in ms.items()}
  out['wide_over_builtin'] = best['expr_wide'] / best['builtin']
  out['one_over_builtin'] = best['expr_one'] / best['builtin']
  out['one_over_wide'] = best['expr_one'] / best['expr_wide']
  # one wavefront's time per body word and observation (the waves of a grid
  # that fits the device at once run side by side), in cycles at CLOCK_GHZ
  for name in ('expr_wide', 'expr_one'):
    ns = best[name] * 1e6 / (a.steps * body_words * a.obs)
    out[name + '_cycles_per_body_word_obs'] = round(ns * CLOCK_GHZ, 2)
  print(json.dumps(out))


if __name__ == '__main__':
  main()
