"""Scalar densities that match none of the closed forms, as builder functions
of the API module `pb` (the style of mcmc_examples.py: `pb` is the reference
package when tools/gen_golden.py records tests/golden/, probayes_amd in the
tests).  probayes_amd lowers each to the expression target
(probayes_amd/expr.py); the reference calls the callable as it is
(rf.py:91, prob.py:331-380).

Each builder returns (process, init, extra, sampler_kwds, keys); the density
callables are module-level so that the tests can call them on arrays.
"""
import numpy as np
import scipy
import scipy.stats


def banana_lp(x, y):
  """Rosenbrock-type banana, log scale."""
  return -((1. - x) ** 2 + 5. * (y - x ** 2) ** 2) / 2.


def well_p(x):
  """Double well exp(x^2 / 2 - x^4 / 4), returned as a linear probability."""
  return np.exp(x ** 2 / 2. - x ** 4 / 4.)


def bound_lp(a, b):
  """A Gamma-like shape in a, a heavy-tailed factor in b whose weight grows
  with a, and a Normal in b whose scale is the variable a."""
  return 2.5 * np.log(a) - a / 1.5 - np.log1p(b ** 2) * np.sqrt(a) + \
      scipy.stats.norm.logpdf(b, 0.25, a)


def expr_banana2(pb, params):
  """2-d banana, log pscale, callable Gaussian delta, constant tran."""
  x = pb.RV('x', vtype=float, vset=(-np.inf, np.inf))
  y = pb.RV('y', vtype=float, vset=(-np.inf, np.inf))
  process = pb.SP(x & y)
  def lp(**kw):   # a def: the reference calls a **kw lambda without arguments
    return banana_lp(kw['x'], kw['y'])
  process.set_prob(lp, pscale='log')
  process.set_tran(lambda **kw: 1.)
  step = params['step']
  process.set_delta(lambda: process.Delta(
      x=scipy.stats.norm.rvs(scale=step), y=scipy.stats.norm.rvs(scale=step)))
  process.set_scores('hastings')
  process.set_update('metropolis')
  return process, {'x': 0., 'y': 0.}, None, {}, ['x', 'y']


def expr_well1(pb, params):
  """1-d double well as a linear probability."""
  x = pb.RV('x', vtype=float, vset=(-np.inf, np.inf))
  process = pb.SP(x)
  def p(**kw):
    return well_p(kw['x'])
  process.set_prob(p)
  process.set_tran(lambda **kw: 1.)
  step = params['step']
  process.set_delta(lambda: process.Delta(x=scipy.stats.norm.rvs(scale=step)))
  process.set_scores('hastings')
  process.set_update('metropolis')
  return process, {'x': 0.5}, None, {}, ['x']


def expr_bound2(pb, params):
  """Bounded 2-d density of log, log1p, sqrt and a norm.logpdf with a
  variable scale; list delta scaled by the lengths, bound=True (a clamps at
  its closed limits, b bounces off its exclusive lower one)."""
  a = pb.RV('a', vtype=float, vset=[0.05, 12.])
  b = pb.RV('b', vtype=float, vset=[(-3.,), 3.])
  process = pb.SP(pb.RF(a, b))
  def lp(**kw):
    return bound_lp(kw['a'], kw['b'])
  process.set_prob(lp, pscale='log')
  process.set_tran(lambda **kw: 1.)
  process.set_delta([params['step']], scale=True, bound=True)
  process.set_scores('hastings')
  process.set_update('metropolis')
  return process, {'a': 0.1, 'b': 0.25}, None, {}, ['a', 'b']


# the density of each workload on arrays, in the order of its keys
DENSITIES = {'expr_banana2': banana_lp, 'expr_well1': well_p,
             'expr_bound2': bound_lp}

EXPR_WORKLOADS = {
  # name: (builder, params, n_chains, n_steps, seed0)
  'expr_banana2': (expr_banana2, {'step': 0.5}, 8, 128, 21000),
  'expr_well1': (expr_well1, {'step': 0.7}, 8, 128, 22000),
  'expr_bound2': (expr_bound2, {'step': 0.08}, 8, 128, 23000),
}
