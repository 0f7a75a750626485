"""Host-side trace handling (no GPU).

The accept words' unpacking into the u [N, T] array the summaries read
(probayes_amd.engine.unpack_accept), against the per-record unpack it
replaced, at ragged chain counts.

The host arithmetic of the trace reductions: pbh_trace_host.cpp's window
check, quantile-list check and pooled-quantile steps, driven by the
stand-alone program tests/trace_host_main.cpp built with the address and
undefined-behaviour sanitizers (and -ffp-contract=off, as the library builds
the unit) and run as a child process (host_program.py).

The window check must give the verdict of first >= 0 and count >= min and
first + count <= rec in unbounded integers for every corner of int64, with no
overflow on the way (the sanitizer ends the program on one).  The pooled steps
must place ranks and interpolate as diag.pooled_quantile does, bit for bit."""
import numpy as np
import pytest

from probayes_amd import diag
from probayes_amd.engine import unpack_accept
from host_program import doubles, hex_words, host
from trace_helpers import Q64, QS

I64_MIN, I64_MAX = -2**63, 2**63 - 1


@pytest.mark.parametrize('n,count', [(1, 5), (63, 7), (64, 3), (65, 9), (1000, 13),
                                     (4097, 2), (65536, 20)])
def test_unpack_accept_equals_per_record_unpack(n, count):
  rng = np.random.default_rng(n * 31 + count)
  W = (n + 63) // 64
  acc = (rng.integers(0, 2 ** 63, size=(count, W), dtype=np.uint64) * np.uint64(2) +
         rng.integers(0, 2, size=(count, W), dtype=np.uint64))
  bits = np.unpackbits(acc.view(np.uint8).reshape(count, W * 8), axis=1,
                       bitorder='little')[:, :n]
  u = unpack_accept(acc, n)
  assert u.shape == (n, count) and u.dtype == np.uint8 and u.flags.c_contiguous
  np.testing.assert_array_equal(u, bits.T)
  # chain c, record t is bit c % 64 of word c // 64
  t, c = count - 1, n - 1
  assert u[c, t] == (int(acc[t, c // 64]) >> (c % 64)) & 1


def test_window_check_at_every_corner(host):
  cases = []
  for rec in (0, 1, 40, 2**40):
    edge = (I64_MIN, -1, 0, 1, rec - 1, rec, rec + 1, I64_MAX)
    cases += [(rec, first, count, least) for first in edge for count in edge
              for least in (0, 1, 2)]
  assert len(cases) == 4 * 8 * 8 * 3
  answers = host(['window {} {} {} {}'.format(*c) for c in cases])
  overflows = 0
  for (rec, first, count, least), ans in zip(cases, answers):
    verdict, end = ans.split()
    want = first >= 0 and count >= least and first + count <= rec
    assert (verdict == 'ok') == want, (rec, first, count, least, ans)
    # the end a refusal names: the sum, saturated where int64 cannot hold it
    assert int(end) == min(max(first + count, I64_MIN), I64_MAX), (first, count, ans)
    overflows += not I64_MIN <= first + count <= I64_MAX
  assert overflows > 0   # (first + count in int64 would have been undefined there)


def _plan(m, q):
  """lo, hi, g and the targets by the formulas of diag.pooled_quantile"""
  q = np.asarray(q, float)
  vi = (m - 1.) * q
  fl = np.floor(vi)
  lo = np.minimum(fl.astype(np.int64), m - 1)
  hi = np.minimum(lo + 1, m - 1)
  return lo, hi, vi - fl, sorted(set(lo.tolist()) | set(hi.tolist()) | {m - 1})


@pytest.mark.parametrize('m', [1, 2, 3, 2004 * 119, 65536 * 1250, 2**40 + 1])
def test_pooled_ranks(host, m):
  for q, ans in zip((QS, Q64), host(['plan {} {} {}'.format(m, len(q), hex_words(q))
                                    for q in (QS, Q64)])):
    word = ans.split()
    at = word.index('ranks')
    assert word[0] == 'plan' and at == 1 + 3 * len(q)
    lo, hi, g, targets = _plan(m, q)
    assert [int(w) for w in word[1:at:3]] == lo.tolist()
    assert [int(w) for w in word[2:at:3]] == hi.tolist()
    assert doubles(word[3:at:3]).tobytes() == g.tobytes()
    ranks = [int(w) for w in word[at + 1:]]
    assert ranks == targets and ranks == sorted(set(ranks)) and m - 1 in ranks


def _arrays():
  """[N, T, d] traces with ties, both zeros, both infinities, a = b = inf (a
  dim whose upper values are all inf) and a dim holding one NaN."""
  inf = np.inf
  a = np.array([[0., -0.], [1., 1.], [1., inf], [-inf, inf], [2.5, inf], [-0., 0.],
                [1., -3.], [7., inf]])
  b = np.random.RandomState(11).normal(size=(7, 3, 3))
  b[2, 1, 0] = b[5, 0, 0]          # a tie
  b[3, 2, 1] = np.nan              # the whole dim is NaN
  b[:, :, 2] = np.round(b[:, :, 2])   # many ties, zeros of both signs
  return [a.reshape(4, 2, 2), b, np.array([[[3., -0.]]])]


@pytest.mark.parametrize('i', range(3))
def test_interpolation_equals_pooled_quantile(host, i):
  x = _arrays()[i]
  m, d = x.shape[0] * x.shape[1], x.shape[2]
  # sorted as diag.pooled_quantile sorts (NaN last; equal zeros in its order)
  s = np.stack([np.sort(x[:, :, k], axis=None) for k in range(d)], axis=1)
  lines, wants = [], []
  for q in (QS, Q64, [.5]):
    lo, hi, _, targets = _plan(m, q)
    lines.append('interp {} {} {} {} {}'.format(m, d, len(q), hex_words(q), hex_words(s[targets].T)))
    wants.append((diag.pooled_quantile(x, q), np.stack([s[lo], s[hi]], axis=1)))
  for (want, stats), ans in zip(wants, host(lines)):
    word = ans.split()
    at = word.index('stats')
    assert doubles(word[1:at]).tobytes() == want.tobytes(), (i, ans)
    assert doubles(word[at + 1:]).tobytes() == stats.tobytes(), i
  if i == 1:
    assert np.isnan(wants[0][0][:, 1]).all() and np.isfinite(wants[0][0][:, 0]).all()
  if i == 0:   # inf - inf between the two infinite neighbours
    assert np.isnan(wants[0][0][:, 1]).any() and not np.isnan(x).any()


def test_quantile_list_messages(host):
  half = hex_words([.5])
  got = host(['qerr 0 1 ' + half, 'qerr 65 1 ' + half, 'qerr 2 2 ' + hex_words([.5, -0.1]),
              'qerr 1 1 ' + hex_words([1.5]), 'qerr 3 3 ' + hex_words([.25, .5, np.nan]),
              'qerr 64 64 ' + hex_words(Q64), 'qerr 10 10 ' + hex_words(QS)])
  assert got[0] == 'nq = 0 outside 1..64' and got[1] == 'nq = 65 outside 1..64'
  assert got[2] == 'q[1] = -0.1 is not a quantile in [0, 1]'
  assert got[3] == 'q[0] = 1.5 is not a quantile in [0, 1]'
  assert got[4] == 'q[2] = nan is not a quantile in [0, 1]'
  assert got[5] == got[6] == 'ok'
