"""Densities over observed data arrays: likelihoods summed with np.sum /
np.mean, as builder functions of the API module `pb` (the style of
expr_examples.py: `pb` is the reference package when tools/gen_golden.py
records tests/golden/, probayes_amd in the tests).  probayes_amd lowers each to
the expression target with loop regions (probayes_amd/expr.py); the reference
calls the callable as it is, with float64 scalars.

The data live in the callables' closures and are generated here from fixed
RandomState seeds.  Each builder returns (process, init, extra, sampler_kwds,
keys); the density callables are module-level so that the tests can call them
point by point.
"""
import numpy as np
import scipy
import scipy.stats


def _linreg_data(n=137):
  rs = np.random.RandomState(4101)
  x = rs.normal(0., 1.5, n)
  return x, 0.7 - 1.2 * x + 0.8 * rs.standard_normal(n)


def _logistic_data(n=40):
  rs = np.random.RandomState(4102)
  x = rs.normal(0., 1.2, n)
  p = 1. / (1. + np.exp(-(0.4 + 1.1 * x)))
  return x, (rs.uniform(size=n) < p).astype(np.int64)   # an integer 0/1 array


def _robust_data(n=7):
  rs = np.random.RandomState(4103)
  return 1.5 + 0.6 * rs.standard_cauchy(n), 1.5 + rs.standard_normal(n)


LIN_X, LIN_Y = _linreg_data()      # n = 137: crosses the 128 split
LOG_X, LOG_Y = _logistic_data()    # n = 40: one 8-accumulator leaf
ROB_Y, ROB_Z = _robust_data()      # n = 7: the sequential leaf


def linreg_lp(b0, b1, s):
  """Linear regression with Normal priors on the coefficients and 1 / s on
  the noise scale."""
  return np.sum(scipy.stats.norm.logpdf(LIN_Y, b0 + b1 * LIN_X, s)) \
      + scipy.stats.norm.logpdf(b0, 0., 10.) \
      + scipy.stats.norm.logpdf(b1, 0., 10.) - np.log(s)


def logistic_lp(a, b):
  """Logistic regression on an integer 0/1 response, Normal(0, 5) priors."""
  eta = a + b * LOG_X
  return np.sum(LOG_Y * eta - np.log1p(np.exp(eta))) - (a * a + b * b) / 50.


def robust_lp(m, s):
  """Cauchy location-scale likelihood of Y and a Laplace-like pull of the
  location towards Z: two sums (one of them a mean)."""
  n = len(ROB_Y)
  return -np.sum(np.log1p(((ROB_Y - m) / s) ** 2)) - n * np.log(s) \
      - np.mean(abs(ROB_Z - m))


def data_linreg3(pb, params):
  """3-d regression posterior; list delta scaled by the lengths, bound=True
  (as expr_bound2)."""
  b0 = pb.RV('b0', vtype=float, vset=[-5., 5.])
  b1 = pb.RV('b1', vtype=float, vset=[-5., 5.])
  s = pb.RV('s', vtype=float, vset=[0.05, 10.])
  process = pb.SP(pb.RF(b0, b1, s))
  def lp(**kw):   # a def: the reference calls a **kw lambda without arguments
    return linreg_lp(kw['b0'], kw['b1'], kw['s'])
  process.set_prob(lp, pscale='log')
  process.set_tran(lambda **kw: 1.)
  process.set_delta([params['step']], scale=True, bound=True)
  process.set_scores('hastings')
  process.set_update('metropolis')
  return process, {'b0': 0.5, 'b1': -1., 's': 1.}, None, {}, ['b0', 'b1', 's']


def data_logistic2(pb, params):
  """2-d logistic regression, callable Gaussian delta, constant tran."""
  a = pb.RV('a', vtype=float, vset=(-np.inf, np.inf))
  b = pb.RV('b', vtype=float, vset=(-np.inf, np.inf))
  process = pb.SP(a & b)
  def lp(**kw):
    return logistic_lp(kw['a'], kw['b'])
  process.set_prob(lp, pscale='log')
  process.set_tran(lambda **kw: 1.)
  step = params['step']
  process.set_delta(lambda: process.Delta(
      a=scipy.stats.norm.rvs(scale=step), b=scipy.stats.norm.rvs(scale=step)))
  process.set_scores('hastings')
  process.set_update('metropolis')
  return process, {'a': 0., 'b': 0.}, None, {}, ['a', 'b']


def data_robust2(pb, params):
  """2-d robust location-scale posterior: two regions and a mean over n = 7
  observations; list delta scaled by the lengths, bound=True."""
  m = pb.RV('m', vtype=float, vset=[-10., 10.])
  s = pb.RV('s', vtype=float, vset=[0.05, 10.])
  process = pb.SP(pb.RF(m, s))
  def lp(**kw):
    return robust_lp(kw['m'], kw['s'])
  process.set_prob(lp, pscale='log')
  process.set_tran(lambda **kw: 1.)
  process.set_delta([params['step']], scale=True, bound=True)
  process.set_scores('hastings')
  process.set_update('metropolis')
  return process, {'m': 1., 's': 1.}, None, {}, ['m', 's']


# the density of each workload, in the order of its keys
DATA_DENSITIES = {'data_linreg3': linreg_lp, 'data_logistic2': logistic_lp,
                  'data_robust2': robust_lp}

DATA_WORKLOADS = {
  # name: (builder, params, n_chains, n_steps, seed0)
  'data_linreg3': (data_linreg3, {'step': 0.012}, 8, 128, 24000),
  'data_logistic2': (data_logistic2, {'step': 0.5}, 8, 128, 25000),
  'data_robust2': (data_robust2, {'step': 0.06}, 8, 128, 26000),
}
