"""The rank-normalised and the folded split-R-hat (Vehtari et al. 2021)
restated for the tests of probayes_amd/diag.py and of pbh_trace_rhat_rank:
the ranks by scipy.stats.rankdata(method='average') on the raveled dim, the
normal scores by scipy.special.ndtri, split-R-hat by rhat_reference.ref_split
in longdouble.  Shares no code with diag.py -- but for the fold point, which
the callers pass in (diag.pooled_quantile's median, exact by its own tests)."""
import numpy as np
from scipy.special import ndtri
from scipy.stats import rankdata

from rhat_reference import LD, ref_split


def ref_ranks(x, first, count, med=None):
  """[N, count, d]: the 1-based average ranks of every value among its dim's,
  pooled over chains and records; with med [d] those of abs(x - med).  A dim
  that holds a NaN is all NaN (rankdata's 'propagate')."""
  w = np.asarray(x, float)[:, first:first + count, :]
  if med is not None:
    with np.errstate(invalid='ignore'):
      w = np.abs(w - np.asarray(med, float))
  n, _, d = w.shape
  out = np.empty((n, count, d))
  for k in range(d):
    out[:, :, k] = rankdata(w[:, :, k].ravel(), method='average').reshape(n, count)
  return out


def ref_scores(ranks):
  """The normal scores of ranks [N, count, d] among M = N count values."""
  m = ranks.shape[0] * ranks.shape[1]
  return ndtri((np.asarray(ranks, float) - 0.375) / (m + 0.25))


def ref_rank_rhat(x, first, count, med):
  """{'bulk', 'folded'}: [d] longdouble each."""
  out = {}
  for key, fold in (('bulk', None), ('folded', med)):
    z = ref_scores(ref_ranks(x, first, count, fold))
    out[key] = ref_split(np.asarray(z, LD), 0, count)
  return out
