"""The host side of the rank-normalised R-hat (no GPU).

diag.average_ranks against scipy's rankdata, exactly; diag.rank_rhat against
the longdouble restatement of rank_reference.py within 64 eps (rhat_reference.
device_bound's floor: diag-style fp64 with AS241 measured 4e-17 .. 1.3e-16 from
it on these inputs, and AS241 is within 7 ulp of scipy's ndtri per score);
diag.normal_scores against CPython's statistics.NormalDist.inv_cdf over every
possible half-integer rank at M = 4 096.

And probayes_amd/csrc/pbh_rank_impl.h, the header the device kernels include,
with pbh_trace_host.cpp's rank_layout, driven by the stand-alone program
tests/trace_host_main.cpp built with a host compiler alone, -ffp-contract=off
and the address and undefined-behaviour sanitizers, and run as a child
process (host_program.py): its AS241 equals inv_cdf bit for bit everywhere (the same libm, the
same order), its run search equals np.searchsorted, and the refusal of M >=
2^32 and the scratch geometry are right at the edges."""
import statistics

import numpy as np
import pytest

from probayes_amd import diag
from host_program import doubles, hex_words, host
from rank_reference import ndtri, ref_rank_rhat, ref_ranks
from rhat_reference import EPS, ar1_with_repeats, rel_dist

M_SCORES = 4096
INV = statistics.NormalDist().inv_cdf


def _big():
  x = ar1_with_repeats(2004, 160, 2, 5, loc=[0.3, -2.], sd=[1., 3.])
  x[:, :, 1] = np.round(x[:, :, 1], 1)   # heavy ties
  return x


def _zeros():
  """both zeros, ties and a few other values: [4, 6, 2]"""
  a = np.array([0., -0., 1., -1., 0., -0., 5e-324, -5e-324, 2., 0., -0., 2.,
                -0., -0., 0., 3., -3., 0., 0., 1., 1., -0., 7., -7.])
  return np.stack([a.reshape(4, 6), a[::-1].reshape(4, 6)], axis=2)


def _nan():
  x = ar1_with_repeats(7, 12, 2, 9)
  x[3, 5, 1] = np.nan
  return x


CASES = {
    'big (40, 120)': (_big, 40, 120),
    'big (40, 119)': (_big, 40, 119),
    'big (0, 4)': (_big, 0, 4),
    'N = 6': (lambda: ar1_with_repeats(6, 40, 2, 3), 3, 37),
    'N = 1': (lambda: ar1_with_repeats(1, 40, 2, 4), 0, 40),
    'zeros': (_zeros, 0, 6),
    'zeros (1, 4)': (_zeros, 1, 4),
    'NaN dim': (_nan, 0, 12),
}
_CACHE = {}


def _case(name):
  make, first, count = CASES[name]
  if make not in _CACHE:
    _CACHE[make] = make()
  return _CACHE[make], first, count


@pytest.mark.parametrize('fold', [False, True])
@pytest.mark.parametrize('name', list(CASES))
def test_average_ranks_equal_scipy(name, fold):
  x, first, count = _case(name)
  got = diag.average_ranks(x, first, count, fold=fold)
  med = diag.pooled_quantile(x, [.5], first, count)[0] if fold else None
  want = ref_ranks(x, first, count, med)
  assert got.shape == want.shape == (x.shape[0], count, x.shape[2])
  assert np.array_equal(got, want, equal_nan=True), name
  m = x.shape[0] * count
  for k in range(x.shape[2]):
    if np.isnan(want[:, :, k]).any():
      assert np.isnan(got[:, :, k]).all()
    else:   # multiples of 1/2 that sum as 1 .. M do
      assert np.array_equal(got[:, :, k] * 2, np.round(got[:, :, k] * 2))
      assert got[:, :, k].sum() == m * (m + 1) / 2
  if name == 'NaN dim':
    assert np.isnan(got[:, :, 1]).all() and np.isfinite(got[:, :, 0]).all()
  if name.startswith('big'):
    ties = [np.unique(want[:, :, k]).size for k in range(2)]
    print(name, 'distinct ranks per dim', ties, 'of', m)
    assert ties[1] < ties[0] < m   # MH-style repeats in dim 0, heavy ties in dim 1


@pytest.mark.parametrize('name', list(CASES))
def test_rank_rhat_against_longdouble(name):
  x, first, count = _case(name)
  got = diag.rank_rhat(x, first, count)
  ref = ref_rank_rhat(x, first, count, diag.pooled_quantile(x, [.5], first, count)[0])
  for key in ('bulk', 'folded'):
    dist = rel_dist(got[key], ref[key])
    print('{} {}: diag.py - longdouble {:.3g} (bound {:.3g})'.format(name, key, dist, 64 * EPS))
    assert got[key].shape == (x.shape[2],)
    assert dist <= 64 * EPS, (name, key, got[key], ref[key])
  assert got['rhat'].tobytes() == np.maximum(got['bulk'], got['folded']).tobytes()
  if name == 'NaN dim':
    assert np.isnan(got['rhat'][1]) and np.isfinite(got['rhat'][0])


def test_rank_rhat_argument_checks():
  x = ar1_with_repeats(5, 12, 2, 1)
  with pytest.raises(ValueError, match='count = 3'):
    diag.rank_rhat(x, 0, 3)
  with pytest.raises(ValueError, match='outside'):
    diag.rank_rhat(x, 5, 8)
  with pytest.raises(ValueError, match='outside'):
    diag.rank_rhat(x, -1, 8)
  with pytest.raises(ValueError, match='a trace'):
    diag.rank_rhat(x[0])
  with pytest.raises(ValueError, match='outside'):
    diag.average_ranks(x, 0, 13)
  assert diag.rank_rhat(x, 2)['rhat'].shape == (2,)


def _half_ranks():
  """every possible average rank among M_SCORES values, and its p"""
  r = np.arange(2, 2 * M_SCORES + 1) / 2.
  assert r.size == 8191 and r[0] == 1. and r[-1] == M_SCORES
  return r, (r - 0.375) / (M_SCORES + 0.25)


def test_normal_scores_equal_inv_cdf():
  r, p = _half_ranks()
  got = diag.normal_scores(r, M_SCORES)
  want = np.array([INV(v) for v in p])
  mid = np.abs(p - 0.5) <= 0.425
  assert mid.any() and not mid.all()
  # no libm call in the central branch: the same bits
  assert got[mid].tobytes() == want[mid].tobytes()
  # in the tails np.log may differ from math.log in the last bit
  differ = int((got != want).sum())
  dist = rel_dist(got[~mid], want[~mid])
  print('tails: {} of {} scores differ from inv_cdf, largest distance {:.3g} ({:.2f} eps)'
        .format(differ, int((~mid).sum()), dist, dist / EPS))
  assert dist <= 64 * EPS
  # the same function the reference uses, to its own accuracy
  assert rel_dist(got, ndtri(p)) <= 64 * EPS
  assert np.isnan(diag.normal_scores(np.nan, 10))


# ---- the header and the geometry, through the stand-alone program -----------
def test_header_scores_equal_inv_cdf_bit_for_bit(host):
  r, p = _half_ranks()
  # the ends of (0, 1) and the two sides of each branch boundary: |q| = 0.425,
  # and r = sqrt(-log(p)) = 5 at p = exp(-25)
  edge = [1e-300, 1. - 2.**-53, 0.075, np.nextafter(0.075, 0.), 0.925, np.nextafter(0.925, 1.),
          np.exp(-25.), np.nextafter(np.exp(-25.), 0.), np.nextafter(np.exp(-25.), 1.),
          1. - np.exp(-25.), 0.5]
  p_all = np.concatenate([p, edge])
  want = np.array([INV(float(v)) for v in p_all])
  got, scored = host(['ndtri ' + hex_words(p_all), 'score {} {}'.format(M_SCORES, hex_words(r))])
  got = doubles(got.split())
  assert got.tobytes() == want.tobytes(), np.flatnonzero(got != want)
  assert doubles(scored.split()).tobytes() == want[:r.size].tobytes()
  # each branch was taken
  q = np.abs(p_all - 0.5)
  rr = np.sqrt(-np.log(np.minimum(p_all, 1. - p_all)))
  assert (q <= 0.425).any() and ((q > 0.425) & (rr <= 5.)).any() and (rr > 5.).any()
  assert np.isfinite(want).all()


def _key_arrays():
  top = np.uint64(2**64 - 1)
  rng = np.random.default_rng(2)
  alt = np.repeat(np.arange(40, dtype=np.uint64), np.tile([1, 2], 20))   # runs of 1 and 2
  return {
      'run at the start': np.array([3, 3, 3, 3, 3, 7, 9, 11], np.uint64),
      'run at the end': np.array([1, 2, 5, top, top, top, top, top, top], np.uint64),
      'one run': np.full(37, 1 << 63, np.uint64),
      'M = 1': np.array([0], np.uint64),
      'runs of 1 and 2': alt,
      'distinct': np.arange(0, 66, 2, dtype=np.uint64),
      'random runs': np.sort(rng.integers(0, 12, 200).astype(np.uint64) << np.uint64(56)),
  }


@pytest.mark.parametrize('name', list(_key_arrays()))
def test_run_search_equals_searchsorted(host, name):
  keys = _key_arrays()[name]
  ans = host(['run ' + ' '.join('{:016x}'.format(int(k)) for k in keys)])[0].split()
  at = ans.index('ranks')
  got = np.array([int(w) for w in ans[:at]]).reshape(-1, 2)
  lo = np.searchsorted(keys, keys, 'left')
  hi = np.searchsorted(keys, keys, 'right')
  assert got.shape == (keys.size, 2)
  assert np.array_equal(got[:, 0], lo) and np.array_equal(got[:, 1], hi), name
  assert np.array_equal(doubles(ans[at + 1:]), (lo + hi + 1) / 2.)


def _layout(ans):
  word = ans.split()
  if word[0] == 'bad':
    return None
  names = ('M tiles chunk_tiles chunks select med res state chunk hist stats key0 key1 idx0 '
           'idx1 z r bytes').split()
  assert word[0] == 'ok' and len(word) == 1 + len(names)
  return dict(zip(names, (int(w) for w in word[1:])))


def test_layout_geometry_and_refusal(host):
  tile, most = 2048, 256
  sizes = [1, tile - 1, tile, tile + 1, most * tile, most * tile + 1, 2 * most * tile + 1,
           2**32 - 1]
  lines = ['rank_layout {} 1 3 100 1'.format(m) for m in sizes]
  lines += ['rank_layout {} 1 3 100 1'.format(2**32), 'rank_layout 65536 65536 3 100 1',
            'rank_layout {} {} 1 0 0'.format(2**40, 2**40), 'rank_layout 0 4 1 0 0',
            'rank_layout 4 0 1 0 0', 'rank_layout 4 4 0 0 0', 'rank_layout 2004 119 10 0 0',
            'rank_layout 65535 65537 2 7 1']
  ans = [_layout(a) for a in host(lines)]
  for m, l in zip(sizes, ans):
    assert l is not None and l['M'] == m
    assert l['tiles'] == -(-m // tile)                       # every element in one tile
    assert l['chunks'] <= most and l['chunk_tiles'] >= 1
    assert l['chunks'] == -(-l['tiles'] // l['chunk_tiles'])   # every tile in one chunk,
    assert (l['chunks'] - 1) * l['chunk_tiles'] < l['tiles']   # and no chunk empty
    if l['tiles'] <= most:
      assert l['chunk_tiles'] == 1
    # the regions in order, 256-byte aligned, each as large as what it holds
    order = ['select', 'med', 'res', 'state', 'chunk', 'hist', 'stats', 'key0', 'key1', 'idx0',
             'idx1', 'z', 'r', 'bytes']
    need = [100 * 8, 3 * 8, 2 * 3 * 8, 8 * 4, l['chunks'] * 256 * 4, l['tiles'] * 256 * 4,
            6 * m * 8, m * 8, m * 8, m * 4, m * 4, m * 8, m * 8]
    assert l['select'] == 0
    for a, b, size in zip(order, order[1:], need):
      assert l[a] % 256 == 0 and l[b] - l[a] >= size, (m, a)
      assert l[b] - l[a] < size + 256
  assert [l['chunk_tiles'] for l in ans[4:7]] == [1, 2, 3]
  assert ans[8] is None and ans[9] is None and ans[10] is None      # M >= 2^32
  assert ans[11] is None and ans[12] is None and ans[13] is None    # an argument out of range
  l = ans[14]   # without ranks the r buffer takes nothing
  assert l['M'] == 2004 * 119 and l['r'] == l['bytes'] and l['select'] == l['med'] == 0
  l = ans[15]
  assert l['M'] == 65535 * 65537 == 2**32 - 1 and l['tiles'] == 2**21
