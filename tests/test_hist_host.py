"""The host side of the pooled histograms (no GPU): pbh_trace_host.cpp's edge
and pair checks, layouts and choice of lookup, and pbh_hist_bin.h's lookup --
the header the kernels of pbh_hist.hip include, so the functions run here are
the ones the device runs -- driven by the stand-alone program tests/
hist_host_main.cpp, built with a host compiler alone, -ffp-contract=off and the
address and undefined-behaviour sanitizers, and run as a child process.

Both lookups must equal diag.hist_bin for every value sent: every edge, its two
neighbouring doubles, the zeros, the infinities, NaN, +-1e308, 5e-324 and 10 000
random values per edge set.  The search is run on every set, the guess only on
the sets hist_guess_ok passes."""
import os

import numpy as np
import pytest

from probayes_amd import diag
from host_program import CSRC, ROOT, build_sanitized, compiler, hex_words, runner

LANES, GROUPS, MAX_BINS, MAX_CELLS, BUDGET = 256, 1024, 4096, 16384, 64 * 1024
SHAPES = [(1, 2, 1), (6, 37, 2), (130, 40, 32), (2004, 160, 10), (33000, 8, 10),
          (65536, 1250, 10)]


@pytest.fixture(scope='module')
def host(tmp_path_factory):
  cxx = compiler()
  if cxx is None:
    pytest.skip('no host C++ compiler')
  tmp = tmp_path_factory.mktemp('hist_host')
  exe = str(tmp / 'hist_host_main')
  build_sanitized(cxx, [os.path.join(ROOT, 'tests', 'hist_host_main.cpp'),
                        os.path.join(CSRC, 'pbh_trace_host.cpp')], exe, ['-ffp-contract=off'])
  return runner(exe, tmp)


def _ladder130():
  v = np.empty(130)
  v[0] = 1.
  for i in range(1, 130):
    v[i] = np.nextafter(v[i - 1], 2.)
  return v


# the edge sets of the issue, by whether the guess is right for them
GUESS_OK = {'linspace(-1, 7, 51)': np.linspace(-1., 7., 51),
            'linspace(-4, 4, 4097)': np.linspace(-4., 4., 4097),
            'linspace(2.9, 3.1, 1001)': np.linspace(2.9, 3.1, 1001),
            'linspace(-1e300, 1e300, 8)': np.linspace(-1e300, 1e300, 8),
            '130 consecutive doubles': _ladder130()}
GUESS_FAILS = {'linspace(0, 5e-323, 11)': np.linspace(0., 5e-323, 11),
               'a span that overflows': np.array([-1.5e308, 0., 1.5e308]),
               'a span that overflows, 64 bins': np.arange(-32., 33.) * (1.7e308 / 32.)}
# sets of other looks: the choice is by the property, whatever it turns out
OTHER = {'geometric': np.geomspace(1e-3, 1e3, 101), 'one bin': np.array([-0.5, 2.]),
         'two bins': np.array([0., 1., 1.5]), 'uneven': np.array([-3., -2.9, 0., 0.1, 50.]),
         'geometric, 4 096 bins': np.geomspace(1e-6, 1e6, 4097),
         'about zero': np.array([-1e-300, -5e-324, 0., 5e-324, 1e-300])}
EDGE_SETS = dict(GUESS_OK, **GUESS_FAILS, **OTHER)


def _values(e, seed):
  rng = np.random.RandomState(seed)
  inf = np.inf
  lo, hi = e[0], e[-1]
  with np.errstate(over='ignore', invalid='ignore'):
    span = hi - lo
    parts = [e, np.nextafter(e, -inf), np.nextafter(e, inf),
             [0., -0., inf, -inf, np.nan, 1e308, -1e308, 5e-324, -5e-324],
             # inside the edges, a little outside them, and anywhere
             lo / 2 + hi / 2 + (rng.uniform(-0.55, 0.55, 6000) * span if np.isfinite(span)
                                else rng.uniform(-0.55, 0.55, 6000) * hi * 2),
             rng.choice(e, 2000) * (1. + rng.choice([-1e-16, 0., 1e-16, 3e-16], 2000)),
             rng.standard_cauchy(2000) * max(abs(lo), abs(hi), 5e-324)]
  return np.concatenate([np.asarray(p, float) for p in parts])


def _bins(host, how, e, x):
  ans = host(['bins {} {} {} {} {}'.format(how, e.size - 1, hex_words(e), x.size,
                                           hex_words(x))])[0].split()
  if ans[0] == 'refused':
    return None, None
  return int(ans[0]), np.array([int(v) for v in ans[1:]], np.int64)


def test_the_values_cover_what_the_issue_lists():
  x = _values(GUESS_OK['linspace(-1, 7, 51)'], 0)
  assert x.size >= 10000 + 3 * 51 + 9 and np.isnan(x).sum() >= 1
  assert np.isin(np.linspace(-1., 7., 51), x).all()
  assert ((x > -1.) & (x < 7.)).sum() > 5000 and (x < -1.).sum() > 100 and (x > 7.).sum() > 100


@pytest.mark.parametrize('name', sorted(EDGE_SETS))
def test_guess_ok_decides_by_the_property(host, name):
  e = EDGE_SETS[name]
  got = int(host(['guess_ok {} {}'.format(e.size - 1, hex_words(e))])[0])
  if name in GUESS_OK:
    assert got == 1
  if name in GUESS_FAILS:
    assert got == 0
  # the property itself, restated: the raw guess within one of i at both ends of bin i
  nb = e.size - 1
  with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
    s = nb / (e[nb] - e[0])
    want = bool(np.isfinite(s) and s > 0)
    if want:
      i = np.arange(nb)
      for x in (e[:-1], np.nextafter(e[1:], -np.inf)):
        g = np.minimum((x - e[0]) * s, nb - 1.).astype(np.int64)
        want = want and bool((np.abs(g - i) <= 1).all())
  assert got == int(want), name


@pytest.mark.parametrize('name', sorted(EDGE_SETS))
def test_the_lookup_equals_the_definition(host, name):
  e = EDGE_SETS[name]
  x = _values(e, len(name))
  ref = diag.hist_bin(x, e)
  assert {-1, -2, -3} <= set(ref.tolist()) and (ref >= 0).sum() > 1000
  mode, got = _bins(host, 'search', e, x)
  depth = int(np.ceil(np.log2(e.size - 1))) if e.size > 2 else 0
  assert mode == depth and 2 ** depth >= e.size - 1
  assert np.array_equal(got, ref), x[got != ref][:5]
  mode, got = _bins(host, 'guess', e, x)
  if name in GUESS_OK:
    assert mode == -1
  if name in GUESS_FAILS:
    assert mode is None
  if mode is not None:
    assert np.array_equal(got, ref), x[got != ref][:5]
  # what the library picks
  picked, got = _bins(host, 'plan', e, x)
  assert picked == (depth if mode is None else -1)
  assert np.array_equal(got, ref)


def test_every_depth_of_the_search(host):
  """B = 1 .. 33, the powers of two to 4 096 and their neighbours: every depth,
  tables with and without padding."""
  rng = np.random.RandomState(5)
  sizes = sorted(set(list(range(1, 34)) + [2 ** k + j for k in range(6, 13) for j in (-1, 0, 1)
                                           if 2 ** k + j <= MAX_BINS]))
  depths = set()
  for nb in sizes:
    e = np.sort(rng.normal(size=nb + 1)) * 3.
    assert (np.diff(e) > 0).all()
    x = np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf),
                        rng.normal(size=300) * 4., [np.nan, np.inf, -np.inf]])
    mode, got = _bins(host, 'search', e, x)
    depths.add(mode)
    assert np.array_equal(got, diag.hist_bin(x, e)), nb
  assert depths == set(range(13))


def _check(host, n_bins, edges):
  flat = np.concatenate([np.asarray(e, float) for e in edges]) if edges else np.zeros(0)
  return host(['check {} {} {}'.format(len(n_bins), ' '.join(str(b) for b in n_bins),
                                       hex_words(flat))])[0]


def test_check_edges_refusals(host):
  ok = [0., 1., 2.]
  assert _check(host, [2, 0, 2], [ok, ok]) == 'ok'
  assert _check(host, [MAX_BINS], [np.arange(MAX_BINS + 1.)]) == 'ok'
  assert _check(host, [1], [[-1e308, 1e308]]) == 'ok'
  for n_bins, edges, words in (
      ([0, 0, 0], [], ('every n_bins', '3 dims')),
      ([2, -1], [ok], ('dim 1', 'n_bins = -1')),
      ([2, MAX_BINS + 1], [ok], ('dim 1', 'n_bins = 4097')),
      ([2, 0, 2], [ok, [0., np.inf, 2.]], ('dim 2', 'edge 1', 'not finite')),
      ([2, 2], [ok, [np.nan, 1., 2.]], ('dim 1', 'edge 0', 'not finite')),
      ([2, 2], [[0., 1., -np.inf], ok], ('dim 0', 'edge 2', 'not finite')),
      ([2, 3], [ok, [0., 1., 1., 2.]], ('dim 1', 'edge 2', 'strictly increase')),
      ([2], [[0., -0., 1.]], ('dim 0', 'edge 1', 'strictly increase')),
      ([3], [[3., 2., 2.5, 4.]], ('dim 0', 'edge 1', 'strictly increase'))):
    msg = _check(host, n_bins, edges)
    for w in words:
      assert w in msg, (msg, w)


def test_check_pairs_refusals(host):
  def ask(n_bins, pairs, n_pairs=None):
    n_pairs = len(pairs) if n_pairs is None else n_pairs
    return host(['pairs {} {} {} {}'.format(len(n_bins), ' '.join(str(b) for b in n_bins), n_pairs,
                                            ' '.join('{} {}'.format(a, b) for a, b in pairs))])[0]
  assert ask([64, 0, 64], [(0, 2), (2, 0), (0, 0)]) == 'ok'
  assert ask([128, 128], [(0, 1)]) == 'ok'                 # the cell limit
  assert ask([MAX_BINS, 4], [(0, 1), (1, 0)]) == 'ok'
  for n_bins, pairs, n_pairs, words in (
      ([4, 4], [], 0, ('n_pairs = 0',)),
      ([4, 4], [], -2, ('n_pairs = -2',)),
      ([4, 4], [], 65536, ('n_pairs = 65536',)),
      ([4, 4], [(0, 1), (0, 2)], None, ('pair 1', 'dim 2', 'outside')),
      ([4, 4], [(-1, 1)], None, ('pair 0', 'dim -1', 'outside')),
      ([4, 0, 4], [(0, 2), (2, 1)], None, ('pair 1', 'dim 1', 'no edges')),
      ([129, 128], [(0, 0), (1, 0)], None, ('pair 0', '129 x 129', 'cells')),
      ([129, 128], [(1, 1), (1, 0)], None, ('pair 1', '128 x 129', '16512'))):
    msg = ask(n_bins, pairs, n_pairs)
    for w in words:
      assert w in msg, (msg, w)


def _table_len(nb):
  depth = 0
  while 2 ** depth < nb:
    depth += 1
  return 2 ** depth + 1


def _dim_lds(nb):
  return -(-(8 * _table_len(nb) + 4 * (nb + 3)) // 8) * 8


def layout(host, n, count, n_bins):
  ans = host(['layout {} {} {} {}'.format(n, count, len(n_bins),
                                          ' '.join(str(b) for b in n_bins))])[0].split()
  if ans[0] == 'refused':
    return None
  v = [int(a) for a in ans[1:]]
  keys = ('dims', 'groups', 'lds_bytes', 'chain_blocks', 'slices', 'slice_len', 'n_tab', 'n_ctr',
          'tables', 'counts', 'bytes')
  l = dict(zip(keys, v))
  rest = v[len(keys):]
  l['listed'] = [tuple(rest[3 * j:3 * j + 3]) for j in range(l['dims'])]
  rest = rest[3 * l['dims']:]
  assert len(rest) == 5 * l['groups']
  l['group'] = [tuple(rest[5 * g:5 * g + 5]) for g in range(l['groups'])]
  return l


def _check_slices(l, n, count, jobs):
  assert l['chain_blocks'] == -(-n // LANES)
  # the slices cover the count exactly, the last one not empty
  assert 1 <= l['slices'] <= count
  assert (l['slices'] - 1) * l['slice_len'] < count <= l['slices'] * l['slice_len']
  # a workgroup's uint32 counter: fewer than 2^32 elements
  assert LANES * l['slice_len'] < 2 ** 32
  groups = l['chain_blocks'] * jobs
  grid = groups * l['slices']
  assert grid >= min(GROUPS, groups * count) // 2 and grid < max(groups, GROUPS) + groups


def _check_layout(l, n, count, n_bins):
  listed = [k for k, b in enumerate(n_bins) if b > 0]
  assert [j[0] for j in l['listed']] == listed and l['dims'] == len(listed)
  _check_slices(l, n, count, l['groups'])
  firsts = [g[0] for g in l['group']] + [l['dims']]
  assert firsts[0] == 0 and all(a < b for a, b in zip(firsts, firsts[1:]))
  tab_at = ctr_at = 0
  biggest = 0
  for g, (first, tab_off, tab_len, ctr_off, ctr_len) in enumerate(l['group']):
    assert (tab_off, ctr_off) == (tab_at, ctr_at)
    t = c = lds = 0
    members = range(first, firsts[g + 1])
    for j in members:
      nb = n_bins[l['listed'][j][0]]
      assert l['listed'][j][1:] == (t, c)
      t += _table_len(nb)
      c += nb + 3
      lds += _dim_lds(nb)
    assert (tab_len, ctr_len) == (t, c)
    # within the budget; a dim above half of it alone
    assert lds <= BUDGET and 8 * t + 4 * c <= BUDGET
    for j in members:
      if _dim_lds(n_bins[l['listed'][j][0]]) > BUDGET // 2:
        assert len(members) == 1
    biggest = max(biggest, -(-(8 * t + 4 * c) // 8) * 8)
    tab_at += t
    ctr_at += c
  assert (l['n_tab'], l['n_ctr'], l['lds_bytes']) == (tab_at, ctr_at, biggest)
  regions = [(l['tables'], l['n_tab'] * 8), (l['counts'], l['n_ctr'] * 8)]
  end = 0
  for at, size in regions:
    assert at % 256 == 0 and at >= end
    end = at + size
  assert l['bytes'] >= end and l['bytes'] % 256 == 0


def _bin_lists(d):
  rng = np.random.RandomState(d)
  mixed = [int(b) for b in rng.choice([0, 1, 7, 100, 300, 1000, MAX_BINS], d)]
  if not any(mixed):
    mixed[0] = 5
  big = [100] * d
  big[d // 2] = MAX_BINS
  return [[100] * d, [300] * d, mixed, big, [MAX_BINS] * d, [1] * d]


@pytest.mark.parametrize('n,count,d', SHAPES)
def test_layout(host, n, count, d):
  for n_bins in _bin_lists(d):
    l = layout(host, n, count, n_bins)
    assert l is not None, n_bins
    _check_layout(l, n, count, n_bins)


def test_layout_of_known_shapes(host):
  # d = 10 at 100 bins: one group, one read of the window
  l = layout(host, 65536, 1250, [100] * 10)
  assert (l['groups'], l['slices'], l['slice_len']) == (1, 4, 313)
  assert l['lds_bytes'] == 10 * (8 * 129 + 4 * 103) and l['lds_bytes'] <= BUDGET
  # a 4 096-bin dim is a group of its own, also beside dims that would fit with it
  l = layout(host, 2004, 160, [1, MAX_BINS, 1, 0, 50])
  assert [g[0] for g in l['group']] == [0, 1, 2] and l['groups'] == 3
  assert l['lds_bytes'] == -(-(8 * 4097 + 4 * 4099) // 8) * 8
  # d = 32 at 300 bins: the groups split
  l = layout(host, 130, 40, [300] * 32)
  assert [g[0] for g in l['group']] == [0, 12, 24]
  assert (l['chain_blocks'], l['slices'], l['slice_len']) == (1, 40, 1)
  l = layout(host, 1, 2, [1])
  assert (l['tables'], l['counts'], l['bytes'], l['n_tab'], l['n_ctr']) == (0, 256, 512, 2, 4)
  # a window of 2^26 records: the slices are held to 2^24 - 1 records
  l = layout(host, 65536, 2 ** 26, [8])
  assert l['slice_len'] == 2 ** 24 - 1 and l['slices'] == 5


def test_layout_refusals(host):
  for n, count, n_bins in ((0, 4, [2]), (-1, 4, [2]), (4, 0, [2]), (4, -3, [2]), (4, 4, []),
                           (4, 4, [2] * 33), (4, 4, [0, 0]), (4, 4, [2, -1]),
                           (4, 4, [MAX_BINS + 1]), (2 ** 62, 4, [2]), (2 ** 33, 2 ** 31, [2]),
                           (2 ** 40, 1, [2]), (256, 2 ** 41, [2])):
    assert layout(host, n, count, n_bins) is None, (n, count, n_bins)
  assert layout(host, 4, 4, [MAX_BINS] * 32) is not None


def layout2d(host, n, count, n_bins, pairs):
  ans = host(['layout2d {} {} {} {} {} {}'.format(
      n, count, len(n_bins), ' '.join(str(b) for b in n_bins), len(pairs),
      ' '.join('{} {}'.format(a, b) for a, b in pairs))])[0].split()
  if ans[0] == 'refused':
    return None
  v = [int(a) for a in ans[1:]]
  keys = ('lds_bytes', 'chain_blocks', 'slices', 'slice_len', 'n_tab', 'n_ctr', 'tables', 'pairs',
          'counts', 'bytes')
  l = dict(zip(keys, v))
  d = len(n_bins)
  l['tab_off'] = v[len(keys):len(keys) + d]
  l['out'] = v[len(keys) + d:]
  assert len(l['out']) == len(pairs)
  return l


@pytest.mark.parametrize('n,count,d', SHAPES)
def test_layout2d(host, n, count, d):
  n_bins = [64] * d
  if d > 2:
    n_bins[1], n_bins[2] = 0, MAX_BINS
  with_edges = [k for k in range(d) if n_bins[k] and n_bins[k] <= 256]
  pairs = [(a, b) for a in with_edges for b in with_edges if a <= b][:45] + [(0, 0)]
  l = layout2d(host, n, count, n_bins, pairs)
  assert l is not None
  _check_slices(l, n, count, len(pairs))
  at = 0
  for k, nb in enumerate(n_bins):
    assert l['tab_off'][k] == (at if nb else -1)
    at += _table_len(nb) if nb else 0
  assert l['n_tab'] == at
  cells = [n_bins[a] * n_bins[b] for a, b in pairs]
  assert l['out'] == [sum(cells[:p]) for p in range(len(pairs))] and l['n_ctr'] == sum(cells)
  assert l['lds_bytes'] == max(8 * (_table_len(n_bins[a]) + _table_len(n_bins[b])) +
                               4 * n_bins[a] * n_bins[b] for a, b in pairs)
  regions = [(l['tables'], l['n_tab'] * 8), (l['pairs'], len(pairs) * 32),
             (l['counts'], l['n_ctr'] * 8)]
  end = 0
  for at, size in regions:
    assert at % 256 == 0 and at >= end
    end = at + size
  assert l['bytes'] >= end and l['bytes'] % 256 == 0


def test_layout2d_limits(host):
  # the cell limit, and the widest tables a pair can bring: within a CU's 160 KiB
  l = layout2d(host, 2004, 160, [128, 128], [(0, 1)])
  assert l['lds_bytes'] == 2 * 8 * 129 + 4 * MAX_CELLS
  l = layout2d(host, 2004, 160, [MAX_BINS, 4], [(0, 1), (1, 0), (1, 1)])
  assert l['lds_bytes'] == 8 * (4097 + 5) + 4 * MAX_CELLS and l['lds_bytes'] <= 160 * 1024
  for n_bins, pairs in (([129, 128], [(0, 1)]), ([4, 0], [(0, 1)]), ([4, 4], [(0, 2)]),
                        ([4, 4], []), ([4, -1], [(0, 0)])):
    assert layout2d(host, 2004, 160, n_bins, pairs) is None, (n_bins, pairs)
  assert layout2d(host, 0, 160, [4, 4], [(0, 1)]) is None
  assert layout2d(host, 2004, 0, [4, 4], [(0, 1)]) is None
