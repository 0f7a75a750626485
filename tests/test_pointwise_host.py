"""The host side of the pointwise reduction (no GPU): pbh_trace_host.cpp's
pointwise_layout, the pointwise-shape check of pbh_expr_host.cpp, and the two
merges of pbh_pointwise_merge.h -- the header the kernels include -- folded in
the device's order, driven by the stand-alone program
tests/pointwise_host_main.cpp built with a host compiler alone, -ffp-contract=
off and the address and undefined-behaviour sanitizers, and run as a child
process.

The merges against diag.pointwise_stats of the same terms: the error of each
is measured against a two-pass np.longdouble value, and the device order's must
lie within 8x the error of NumPy's own fp64 (diag.pointwise_stats) against that
value -- the factor allows for the different tree shape -- or within 1e-12
relative where NumPy's is smaller than that.  Measured:
over the cases below at most 3.0e-15 for the device order (the mean of terms
spread over -745 .. 709) and 6.0e-14 for NumPy's (the variance of terms at 1e6
+- 1e-3, where the device order's shifted moments keep 1.3e-16)."""
import os

import numpy as np
import pytest

from probayes_amd import diag, expr
from host_program import CSRC, ROOT, build_sanitized, compiler, doubles, hex_words, runner

LANES, TILE, GROUPS = 256, 8, 1024


@pytest.fixture(scope='module')
def host(tmp_path_factory):
  cxx = compiler()
  if cxx is None:
    pytest.skip('no host C++ compiler')
  tmp = tmp_path_factory.mktemp('pointwise_host')
  exe = str(tmp / 'pointwise_host_main')
  build_sanitized(cxx, [os.path.join(ROOT, 'tests', 'pointwise_host_main.cpp'),
                        os.path.join(CSRC, 'pbh_trace_host.cpp'),
                        os.path.join(CSRC, 'pbh_expr_host.cpp')], exe, ['-ffp-contract=off'])
  return runner(exe, tmp)


# ---------------------------------------------------------------------------
# the layout
# ---------------------------------------------------------------------------
SHAPES = [(130, 24, 137), (130, 7, 40), (130, 1, 7), (1, 24, 137), (2004, 16, 137),
          (257, 64, 9), (65536, 1250, 137), (1, 100000, 1), (256, 3, 65536), (3, 5, 8)]


def _layout(host, n, count, n_obs, sel=0, prog=777):
  ans = host(['layout {} {} {} {} {}'.format(n, count, n_obs, sel, prog)])[0].split()
  if ans[0] != 'ok':
    return ' '.join(ans)
  keys = ('chain_blocks', 'tiles', 'npad', 'slices', 'slice_len', 'rows', 'select', 'prog',
          'part', 'res', 'bytes')
  return dict(zip(keys, (int(v) for v in ans[1:])))


@pytest.mark.parametrize('shape', SHAPES)
def test_layout_partition_and_offsets(host, shape):
  n, count, n_obs = shape
  sel, prog = 40, 777
  l = _layout(host, n, count, n_obs, sel, prog)
  assert l['chain_blocks'] == -(-n // LANES) and l['tiles'] == -(-n_obs // TILE)
  assert l['npad'] == TILE * l['tiles'] and l['rows'] == l['chain_blocks'] * l['slices']
  # the record slices: consecutive, none empty, together the window
  assert 1 <= l['slices'] <= count and l['slice_len'] >= 1
  assert (l['slices'] - 1) * l['slice_len'] < count <= l['slices'] * l['slice_len']
  # they are there to fill the device, not beyond it
  groups = l['chain_blocks'] * l['tiles']
  assert l['slices'] == 1 or groups * (l['slices'] - 1) < GROUPS + groups
  # the regions: 256-aligned, in order, disjoint
  sizes = [('select', sel * 8), ('prog', prog * 8), ('part', 6 * l['rows'] * l['npad'] * 8),
           ('res', 3 * l['npad'] * 8)]
  at = 0
  for key, size in sizes:
    assert l[key] % 256 == 0 and l[key] >= at, key
    at = l[key] + size
  assert l['bytes'] % 256 == 0 and l['bytes'] >= at


@pytest.mark.parametrize('shape', [(130, 24, 137), (300, 7, 9), (1, 5, 7), (513, 3, 16)])
def test_layout_covers_every_term_once(host, shape):
  n, count, n_obs = shape
  l = _layout(host, n, count, n_obs)
  seen = np.zeros((n, count, n_obs), np.int64)
  rows = set()
  for block in range(l['chain_blocks']):
    c = np.arange(block * LANES, min((block + 1) * LANES, n))
    for s in range(l['slices']):
      r = np.arange(s * l['slice_len'], min((s + 1) * l['slice_len'], count))
      assert r.size
      rows.add(block * l['slices'] + s)
      for tile in range(l['tiles']):
        j = np.arange(tile * TILE, min((tile + 1) * TILE, n_obs))
        seen[np.ix_(c, r, j)] += 1
  assert np.all(seen == 1) and rows == set(range(l['rows']))


def test_layout_refusals_leave_out_untouched(host):
  bad = [(0, 4, 7, 0, 9), (4, 0, 7, 0, 9), (4, 4, 0, 0, 9), (4, 4, 65537, 0, 9), (4, 4, 7, -1, 9),
         (4, 4, 7, 0, 0), (-3, 4, 7, 0, 9), (2 ** 62, 4, 7, 0, 9), (2 ** 40, 2 ** 30, 7, 0, 9),
         (65535 * 256 + 1, 1, 7, 0, 9)]
  for args in bad:
    assert _layout(host, *args) == 'bad untouched', args
  assert _layout(host, 65535 * 256, 1, 7, 0, 9)['chain_blocks'] == 65535


# ---------------------------------------------------------------------------
# the pointwise shape
# ---------------------------------------------------------------------------
def _shape(host, code, d=2, depth=2, n_consts=2, n_cols=2, n_obs=9):
  return host(['shape {} {} {} {} {} {}'.format(d, depth, n_consts, n_cols, n_obs,
                                                ' '.join(str(int(w)) for w in code))])[0]


def test_pointwise_shape_check(host):
  E, col, var = expr.encode, (expr.VAR, expr.BODY_BASE), (expr.VAR, 0)
  acc, c0 = (expr.ACC, 0), (expr.CONST, 0)
  body = [E(expr.MUL, col, var), E(expr.ADD, acc, c0)]
  region = [E(expr.LOOP, (expr.SLOT, len(body)))] + body + [E(expr.SUM, acc)]
  assert _shape(host, region) == 'ok 0'
  prefix = [E(expr.LOG, var, dst=0, store=True), E(expr.EXP, (expr.VAR, 1), dst=1, store=True)]
  assert _shape(host, prefix + region) == 'ok 2'
  # a traced program
  tg = expr.trace_pointwise(lambda **kw: kw['a'] * np.arange(9.) - np.log(kw['b']), ['a', 'b'])
  at = [expr.decode(w)[0] for w in tg['code']].index(expr.LOOP)
  assert _shape(host, tg['code'], 2, tg['depth'], len(tg['consts']), *tg['data'].shape) == \
      'ok {}'.format(at)
  # two regions; SUM not last; no region
  two = region[:-1] + [E(expr.SUM, acc, dst=0, store=True)] + region
  assert _shape(host, two).startswith('shape ') and 'several' in _shape(host, two)
  tail = region + [E(expr.NEG, acc)]
  assert _shape(host, tail).startswith('shape ') and 'SUM' in _shape(host, tail)
  none = [E(expr.MUL, var, var)]
  assert _shape(host, none).startswith('shape ') and 'none' in _shape(host, none)
  # and what the existing checker refuses stays refused, with its place
  assert _shape(host, region[:-1]).startswith('check 0 ')
  assert _shape(host, [E(expr.MUL, (expr.VAR, 2), var)] + region).startswith('check 0 ')
  assert _shape(host, region[:1] + [E(63, col)] + region[2:]).startswith('check 1 ')
  # a body word whose low bits read LOOP is not a second region: the checker
  # refuses it before the shape is asked
  assert _shape(host, region[:1] + [E(expr.LOOP, col)] + region[2:]).startswith('check ')


# ---------------------------------------------------------------------------
# the merges, in the device's order
# ---------------------------------------------------------------------------
def _reduce(host, T):
  """T [rows, live, len] -> (lse, mean, var) of the rows * live * len terms"""
  rows, live, length = T.shape
  ans = host(['reduce {} {} {} {}'.format(rows, live, length, hex_words(T))])[0].split()
  return doubles(ans)


def _truth(t):
  t = t.astype(np.longdouble)
  top = t.max()
  lse = np.log(np.exp(t - top).sum()) + top
  mean = t.sum() / t.size
  return lse, mean, ((t - mean) ** 2).sum() / (t.size - 1)


MERGE_SHAPES = [(1, 1, 2), (1, 2, 1), (1, 130, 24), (3, 256, 5), (8, 212, 2), (24, 130, 1),
                (2, 7, 125), (5, 33, 17)]


@pytest.mark.parametrize('kind', ['loglik', 'spread', 'offset'])
@pytest.mark.parametrize('shape', MERGE_SHAPES)
def test_merges_against_the_host_definition(host, shape, kind):
  rng = np.random.default_rng(sum(shape))
  T = {'loglik': lambda: -0.5 * rng.normal(0., 3., shape) ** 2 - 1.2,
       'spread': lambda: rng.uniform(-745., 709., shape),
       'offset': lambda: 1e6 + rng.normal(0., 1e-3, shape)}[kind]()
  got = _reduce(host, T)
  flat = T.reshape(-1, 1)
  own = [v[0] for v in diag.pointwise_stats(flat)]
  truth = _truth(flat[:, 0])
  for name, g, o, t in zip(('lse', 'mean', 'var'), got, own, truth):
    if name == 'var' and t == 0:
      assert g == 0 and o == 0
      continue
    floor = abs(t) if name == 'var' else max(abs(t), 1)
    e_dev, e_np = float(abs(g - t) / floor), float(abs(o - t) / floor)
    print('{} {} {}: device order {:.3g}, numpy {:.3g}'.format(kind, shape, name, e_dev, e_np))
    assert e_dev <= max(8. * e_np, 1e-12), (name, e_dev, e_np)


def _same(a, b):
  a, b = np.asarray(a, float), np.asarray(b, float)
  return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize('shape', [(1, 130, 3), (3, 40, 2), (2, 256, 1)])
def test_infinities_and_nans_as_the_host_definition(host, shape):
  rng = np.random.default_rng(11)
  base = rng.normal(-2., 1., shape)
  inf = np.inf
  cases = {}
  for where in ((0, 0, 0), (shape[0] - 1, shape[1] - 1, shape[2] - 1), (0, shape[1] // 2, 0)):
    for v in (-inf, inf, np.nan):
      T = base.copy()
      T[where] = v
      cases[(where, v)] = T
  cases['all -inf'] = np.full(shape, -inf)
  both = base.copy()
  both[0, 0, 0], both[-1, -1, -1] = inf, -inf
  cases['both'] = both
  two = base.copy()
  two[0, 1, 0] = two[-1, 3, 0] = inf
  cases['two +inf'] = two
  rowful = base.copy()
  rowful[0] = -inf            # a whole workgroup at -inf
  cases['a row of -inf'] = rowful
  for key, T in cases.items():
    got = _reduce(host, T)
    with np.errstate(all='ignore'):
      want = [v[0] for v in diag.pointwise_stats(T.reshape(-1, 1))]
    for name, g, w in zip(('lse', 'mean', 'var'), got, want):
      if np.isfinite(w):
        assert abs(g - w) <= 1e-12 * max(abs(w), 1), (key, name, g, w)
      else:
        assert _same(g, w), (key, name, g, w)


def test_merge_identities(host):
  inf = np.inf
  def lse(*v):
    return doubles(host(['lse ' + hex_words(np.array(v))])[0].split())
  def mom(*v):
    return doubles(host(['mom ' + hex_words(np.array(v))])[0].split())
  # the empty set on either side leaves the other as it is, bit for bit
  assert _same(lse(-inf, 0., 1.5, 3.), [1.5, 3., 1.5 + np.log(3.)])
  assert _same(lse(1.5, 3., -inf, 0.), [1.5, 3., 1.5 + np.log(3.)])
  assert _same(lse(-inf, 0., -inf, 0.), [-inf, 0., -inf])
  assert _same(lse(-inf, 2., -inf, 1.), [-inf, 3., -inf])     # terms all -inf
  assert _same(lse(inf, 1., inf, 2.), [inf, 3., inf])
  assert _same(lse(inf, 1., 0., 2.), [inf, 1., inf])
  assert _same(lse(0., 1., 0., 1.), [0., 2., np.log(2.)])
  assert _same(lse(0., 1., -1., 1.), [0., 1. + np.exp(-1.), np.log(1. + np.exp(-1.))])
  assert np.all(np.isnan(lse(np.nan, np.nan, 0., 1.))) and np.all(np.isnan(lse(0., 1., np.nan, 1.)))
  # (count, shift, mean - shift, M2) -> the same and the mean
  assert _same(mom(0., 0., 0., 0., 3., 0., -inf, np.nan), [3., 0., -inf, np.nan, -inf])
  assert _same(mom(3., 0., -inf, np.nan, 0., 0., 0., 0.), [3., 0., -inf, np.nan, -inf])
  assert _same(mom(2., 1., 0., 0.5, 2., 3., 0., 0.5), [4., 1., 1., 5., 2.])
  assert _same(mom(2., 7., -6., 0.5, 2., 1., 2., 0.5), [4., 7., -5., 5., 2.])
  assert _same(mom(2., 0., -inf, np.nan, 2., 3., 0., 0.5), [4., 0., -inf, np.nan, -inf])
  assert _same(mom(2., 3., 0., 0.5, 2., 0., -inf, np.nan), [4., 3., -inf, np.nan, -inf])
  assert _same(mom(2., 0., -inf, np.nan, 2., 0., inf, np.nan), [4., 0., np.nan, np.nan, np.nan])
