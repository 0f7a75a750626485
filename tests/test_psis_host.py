"""The host side of the pointwise tail select (no GPU): pbh_trace_host.cpp's
tail_key, tail_pick and tail_finish, driven by the stand-alone program tests/
psis_host_main.cpp built with a host compiler alone, -ffp-contract=off and the
address and undefined-behaviour sanitizers, and run as a child process.

The device's part is played by NumPy here: the histograms of a count pass are
np.bincount of the keys under the prefix, the gather is a mask, and the
device's partial rows are log-sum-exp pairs of slices of the other terms.  The
tail must equal np.sort of the column bit for bit, the rest
diag.pointwise_tail's to 1e-12 with floor 1 (the two sum in different orders)."""
import os

import numpy as np
import pytest

from probayes_amd import diag
from host_program import CSRC, ROOT, build_sanitized, compiler, doubles, hex_words, runner

DIGIT, TILE = 10, 8
RTOL = 1e-12


@pytest.fixture(scope='module')
def host(tmp_path_factory):
  cxx = compiler()
  if cxx is None:
    pytest.skip('no host C++ compiler')
  tmp = tmp_path_factory.mktemp('psis_host')
  exe = str(tmp / 'psis_host_main')
  build_sanitized(cxx, [os.path.join(ROOT, 'tests', 'psis_host_main.cpp'),
                        os.path.join(CSRC, 'pbh_trace_host.cpp')], exe, ['-ffp-contract=off'])
  return runner(exe, tmp)


def keys_of(v):
  """the monotone 64-bit image of doubles: negative values reversed below the
  positive ones, either zero one image, every NaN the largest"""
  v = np.asarray(v, float)
  u = (v + 0.).view(np.uint64)
  k = np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))
  return np.where(np.isnan(v), np.uint64(2 ** 64 - 1), k).astype(np.uint64)


def test_keys_order_as_sorting_does(host):
  v = np.array([np.nan, -np.inf, -1e300, -1., -5e-324, -0., 0., 5e-324, 1., 1e300, np.inf,
                np.float64(np.nan).view(np.uint64).__or__(np.uint64(7)).view(np.float64)])
  got = np.array([int(a, 16) for a in host(['key ' + hex_words(x) for x in v])], np.uint64)
  assert np.array_equal(got, keys_of(v))
  assert got[0] == got[-1] == 2 ** 64 - 1 and got[5] == got[6]
  assert np.all(np.diff(got[1:11].astype(object)) >= 0)
  back = doubles(host(['value {:016x}'.format(int(k)) for k in got]))
  want = np.where(np.isnan(v), np.nan, v + 0.)
  assert back.tobytes() == want.tobytes()   # +0.0 for either zero, one NaN


def _pair(neg):
  """the log-sum-exp pair of the values neg (the empty set: (-inf, 0))"""
  if neg.size == 0:
    return -np.inf, 0.
  with np.errstate(all='ignore'):
    m = neg.max()
    if np.isnan(m):
      return np.nan, np.nan
    return m, float(np.where(neg == m, 1., np.exp(neg - m)).sum())


def select(host, col, k, capacity, rows=3):
  """(tail, rest_lse, passes) of one column through tail_pick and tail_finish"""
  keys = keys_of(col)
  S = keys.size
  prefix, rank, below, under = 0, k - 1, 0, S
  done = passes = 0
  while done < 64 and below + under > capacity:
    bits = min(DIGIT, 64 - done)
    hit = keys if done == 0 else keys[(keys >> np.uint64(64 - done)) == np.uint64(prefix)]
    assert hit.size == under
    digit = (hit >> np.uint64(64 - done - bits)) & np.uint64((1 << bits) - 1)
    hist = np.bincount(digit.astype(np.int64), minlength=1 << bits)
    ans = host(['pick {} {:016x} {} {} {} {}'.format(bits, prefix, rank, below, under,
                                                     ' '.join(str(h) for h in hist))])[0].split()
    prefix, rank, below, under = int(ans[0], 16), int(ans[1]), int(ans[2]), int(ans[3])
    done += bits
    passes += 1
    assert rank < under and below + rank == k - 1
  if done == 64:
    cand, other = keys[keys < np.uint64(prefix)], col[keys > np.uint64(prefix)]
    assert np.count_nonzero(keys == np.uint64(prefix)) == under
  else:
    hi = keys >> np.uint64(64 - done) if done else np.zeros(S, np.uint64)
    cand, other = keys[hi <= np.uint64(prefix)], col[hi > np.uint64(prefix)]
    assert cand.size == below + under
  assert cand.size <= capacity
  cand = cand[np.random.default_rng(5).permutation(cand.size)]   # any order
  pairs = [_pair(-part) for part in np.array_split(other, rows)]
  line = 'finish {} {} {:016x} {} {} {} {} {} {} {}'.format(
      k, done, prefix, rank, below, under, cand.size,
      ' '.join('{:016x}'.format(int(c)) for c in cand), rows,
      ' '.join(hex_words(np.array(p)) for p in pairs))
  out = doubles(host([line])[0].split())
  return out[:k], out[k], passes


def check(host, col, k, capacity):
  tail, rest, passes = select(host, col, k, capacity)
  want_tail, want_rest = diag.pointwise_tail(col[:, None], k)
  assert tail.tobytes() == want_tail[0].tobytes()
  want = want_rest[0]
  if np.isfinite(want):
    assert abs(rest - want) <= RTOL * max(abs(want), 1.), (rest, want)
  else:
    assert np.array_equal([rest], [want], equal_nan=True), (rest, want)
  return passes


def _columns():
  rng = np.random.default_rng(17)
  base = -0.5 * rng.normal(0., 3., 3120) ** 2 - 1.2
  few = rng.choice(base[:9], 3120)                  # nine values, heavy ties
  ties = base.copy()
  ties[:900] = np.sort(base)[100]                   # 900 copies of one value, rank k - 1 among them
  zeros = base.copy()
  zeros[:40], zeros[40:80] = -0., 0.
  zeros[80:700] = np.abs(zeros[80:700])             # the zeros are the smallest but 2 420
  nans = base.copy()
  nans[::7] = np.nan
  infs = base.copy()
  infs[:5], infs[5:9] = -np.inf, np.inf
  return {'loglik': base, 'few values': few, 'ties across the cut': ties,
          'all equal': np.full(780, -3.25), 'all equal zero': np.full(780, -0.),
          'zeros': zeros, 'nans': nans, 'mostly nan': np.where(np.arange(910) % 3, np.nan, base[:910]),
          'all nan': np.full(780, np.nan), 'infinities': infs,
          'last ulps': 1. + np.arange(780) % 13 * 2.220446049250313e-16}


@pytest.mark.parametrize('name', sorted(_columns()))
def test_select_equals_sorting(host, name):
  col = _columns()[name]
  S = col.size
  k = diag.psis_tail_length(S) + 1
  loose = check(host, col, k, max(2 * k, 65536))
  assert loose == 0                                  # every draw fits the default capacity
  tight = check(host, col, k, k)                     # capacity == k: the cut is isolated
  assert tight >= 1
  if name.startswith('all') or name in ('few values', 'ties across the cut', 'last ulps'):
    assert tight == 7                                # ties at the cut: all 64 bits fixed
  check(host, col, k, k + 50)
  check(host, col, 1, 1)
  check(host, col, S - 1, S - 1)


def test_zeros_come_out_positive(host):
  col = _columns()['zeros']
  tail, _, _ = select(host, col, 2500, 2500)
  zero = tail == 0
  assert zero.sum() == 80 and not np.signbit(tail[zero]).any()


def test_a_long_column(host):
  rng = np.random.default_rng(3)
  col = rng.standard_t(3, 32064) * 4. - 2.
  k = diag.psis_tail_length(col.size) + 1
  assert check(host, col, k, k) >= 2 and check(host, col, k, 2 * k) >= 1


def test_layout_and_batches(host):
  for tiles, cap in ((1, 65536), (18, 65536), (3, 7), (64, 4194304)):
    npad, prefix, cursor, hist, lists, words = (int(v) for v in
                                                host(['layout {} {}'.format(tiles, cap)])[0].split())
    assert npad == TILE * tiles and (prefix, cursor, hist) == (0, npad, 2 * npad)
    assert lists == hist + npad * 1024 and words == lists + npad * cap
  for cap in (1, 65536, 100000, 4194304, 4194305, 2 ** 40):
    tiles, _, top = (int(v) for v in host(['batch {}'.format(cap)])[0].split())
    assert top == 4194304 and tiles >= 1
    assert tiles * TILE * cap * 8 <= 256 << 20 or (tiles == 1 and cap > top)
    assert (tiles + 1) * TILE * cap * 8 > 256 << 20
  for k, want in ((1, 65536), (32768, 65536), (32769, 65538), (10 ** 6, 2 * 10 ** 6)):
    assert int(host(['batch {}'.format(k)])[0].split()[1]) == want
