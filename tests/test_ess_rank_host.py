"""The host side of the bulk- and tail-ESS across chains (no GPU).

diag.rank_ess (split_chain_acov by FFT, multi_chain_ess) against the
longdouble restatement by direct sums of ess_reference.py.  The bound is
rhat_reference.device_bound's floor, 64 eps (measured on these inputs: 0.4 .. 40
eps), raised to 512 eps for the two indicator series of the window (0, 4) alone:
at h = 2 there is one pair, tau = 1 + 2 rho[1] is a difference near 0.2, and the
FFT's rounding of A[0] and A[1] -- a few eps each, of 0 / 1 series whose A is
small against their means' variance -- is amplified by 1 / tau and by the
cancellation in mean_var - A[1] (measured: 55 and 179 eps).  Every distance is
printed.  Every decision of Geyer's scan must be
clear of rounding (ess_reference.clear), which is asserted, not assumed.

And pbh_trace_host.cpp's multi_chain_ess and ess_layout, driven by the
stand-alone program tests/trace_host_main.cpp built with a host compiler alone,
-ffp-contract=off and the address and undefined-behaviour sanitizers, and run
as a child process (host_program.py): its ESS equals diag.multi_chain_ess bit for bit on the same
means and autocovariances, and the scratch geometry is right at the edges."""
import numpy as np
import pytest

from probayes_amd import diag
from host_program import hex_words, host
from ess_reference import VARIANTS, clear, ref_acov, ref_ess, ref_rank_ess
from rhat_reference import EPS, ar1_with_repeats, rel_dist

BOUND = 64 * EPS
BOUND_H2_INDICATOR = 512 * EPS   # (see above; never above 1e-9)
assert BOUND <= BOUND_H2_INDICATOR <= 1e-9


def _bound(name, key):
  return BOUND_H2_INDICATOR if name == 'big (0, 4)' and key.startswith('tail') else BOUND


def _big():
  x = ar1_with_repeats(2004, 160, 2, 5, loc=[0.3, -2.], sd=[1., 3.])
  x[:, :, 1] = np.round(x[:, :, 1], 1)   # heavy ties
  return x


CASES = {
    'big (40, 120)': (_big, 40, 120),
    'big (40, 119)': (_big, 40, 119),
    'big (0, 4)': (_big, 0, 4),
    'N = 6': (lambda: ar1_with_repeats(6, 40, 2, 3), 3, 37),
    'N = 1': (lambda: ar1_with_repeats(1, 40, 2, 4), 0, 40),
}
_CACHE = {}


def _case(name):
  """(x, first, count, diag.rank_ess, the reference): computed once"""
  if name not in _CACHE:
    make, first, count = CASES[name]
    if make not in _CACHE:
      _CACHE[make] = make()
    x = _CACHE[make]
    _CACHE[name] = (x, first, count, diag.rank_ess(x, first, count),
                    ref_rank_ess(x, first, count))
  return _CACHE[name]


@pytest.mark.parametrize('name', list(CASES))
def test_rank_ess_against_longdouble(name):
  x, first, count, got, ref = _case(name)
  assert sorted(got) == sorted(VARIANTS + ('tail',))
  for key in VARIANTS:
    assert all(clear(r) for r in ref[key]), (name, key)   # the precondition, every dim
    want = np.array([r['ess'] for r in ref[key]])
    dist, bound = rel_dist(got[key], want), _bound(name, key)
    print('{} {}: diag.py - longdouble {:.3g} ({:.1f} eps; bound {:.0f} eps), k* {} of K {}'.format(
        name, key, dist, dist / EPS, bound / EPS, [r['k_star'] for r in ref[key]],
        ref[key][0]['K']))
    assert got[key].shape == (x.shape[2],)
    assert dist <= bound, (name, key, got[key], want)
  assert got['tail'].tobytes() == np.minimum(got['tail_lower'], got['tail_upper']).tobytes()


def test_split_chain_acov_against_direct_sums():
  x, first, count, _, _ = _case('big (40, 119)')
  y = x[:, :, 0]
  m, a = diag.split_chain_acov(y, first, count)
  rm, ra = ref_acov(y, first, count)
  assert m.shape == (2 * y.shape[0],) and a.shape == (count // 2,)
  dm = rel_dist(m, rm)
  da = float(np.max(np.abs(np.asarray(a, np.longdouble) - ra)) / ra[0])
  print('means {:.3g}, max_t |A - A_ref| / A_ref[0] {:.3g}'.format(dm, da))
  assert da <= BOUND
  # (a mean near zero keeps only its absolute accuracy: eps of the values' size)
  assert np.max(np.abs(np.asarray(m, np.longdouble) - rm)) <= 64 * EPS * np.abs(y).max()
  # the split chains in split_rhat's order: first halves, then second halves
  assert abs(m[3] - y[3, first:first + count // 2].mean()) < 1e-12
  assert abs(m[y.shape[0] + 3] - y[3, first + count - count // 2:first + count].mean()) < 1e-12


def test_the_inputs_reach_every_branch_of_the_scan():
  refs = [r for name in CASES for key in VARIANTS for r in _case(name)[4][key]]
  assert all(clear(r) for r in refs)
  assert any(r['k_star'] == r['K'] and r['K'] > 1 for r in refs)   # the scan never stops
  assert any(r['k_star'] < r['K'] for r in refs)
  assert any(r['min_changed'] for r in refs)   # the running minimum replaces a pair
  assert any(r['added'] for r in refs)         # the rho[2 k*] > 0 term
  assert any(r['k_star'] < r['K'] and not r['added'] for r in refs)


def test_independent_draws_give_the_number_of_draws():
  x = np.random.RandomState(11).normal(size=(500, 80, 2))
  got = diag.rank_ess(x)
  for key in ('bulk', 'basic'):
    print(key, got[key] / (500 * 80))
    assert np.all(np.abs(got[key] / (500 * 80) - 1.) <= 0.1), (key, got[key])


def test_constant_chains():
  same = np.full((40, 12, 2), 1.7)
  got = diag.rank_ess(same)
  for key in VARIANTS + ('tail',):
    assert np.isnan(got[key]).all(), key
  # (40 chains: some lie on either side of the 5 % and of the 95 % quantile,
  # so the indicator series are constant and different too)
  differ = same * np.arange(1., 41.)[:, None, None]
  got = diag.rank_ess(differ)
  for key in VARIANTS + ('tail',):
    assert np.isfinite(got[key]).all(), (key, got[key])


def test_a_nan_record_makes_its_dim_nan():
  x = ar1_with_repeats(7, 12, 2, 9)
  x[3, 5, 1] = np.nan
  got = diag.rank_ess(x)
  for key in VARIANTS + ('tail',):
    assert np.isnan(got[key][1]) and np.isfinite(got[key][0]), key
  m, a = diag.split_chain_acov(x[:, :, 1])
  assert np.isnan(a).all()


def test_argument_checks():
  x = ar1_with_repeats(5, 12, 2, 1)
  with pytest.raises(ValueError, match='count = 3'):
    diag.rank_ess(x, 0, 3)
  with pytest.raises(ValueError, match='outside'):
    diag.rank_ess(x, 5, 8)
  with pytest.raises(ValueError, match='outside'):
    diag.rank_ess(x, -1, 8)
  with pytest.raises(ValueError, match='a trace'):
    diag.rank_ess(x[0])
  with pytest.raises(ValueError, match='a series'):
    diag.split_chain_acov(x)
  with pytest.raises(ValueError, match='outside'):
    diag.split_chain_acov(x[:, :, 0], 0, 13)
  with pytest.raises(ValueError, match='multi_chain_ess'):
    diag.multi_chain_ess(np.zeros(3), np.ones(4), 4, 4)
  with pytest.raises(ValueError, match='multi_chain_ess'):
    diag.multi_chain_ess(np.zeros(1), np.ones(4), 1, 4)
  assert diag.rank_ess(x, 2)['bulk'].shape == (2,)


# ---- the host stage of the library, through the stand-alone program ---------
def _same_bits(a, b):
  return (np.isnan(a) and np.isnan(b)) or np.float64(a).tobytes() == np.float64(b).tobytes()


def _host_inputs():
  """(label, m, A): diag's own means and autocovariances of the cases, and
  the edges -- h = 2, h = 2 048, C = 2, a NaN, all zero, constant chains"""
  out = []
  for name in CASES:
    x, first, count, _, _ = _case(name)
    for k in range(x.shape[2]):
      out.append((name + ' values', ) + diag.split_chain_acov(x[:, :, k], first, count))
      ind = (x[:, :, k] <= np.median(x[:, first:first + count, k])).astype(float)
      out.append((name + ' indicator', ) + diag.split_chain_acov(ind, first, count))
  slow = ar1_with_repeats(3, 4096, 1, 8, rho=0.995)[:, :, 0]
  out.append(('h = 2048',) + diag.split_chain_acov(slow))
  out.append(('h = 2048, independent',) + diag.split_chain_acov(
      np.random.RandomState(2).normal(size=(3, 4096))))
  m, a = diag.split_chain_acov(ar1_with_repeats(4, 9, 1, 6)[:, :, 0])
  out.append(('NaN in A', m, np.where(np.arange(a.size) == 2, np.nan, a)))
  out.append(('NaN in A[0]', m, np.where(np.arange(a.size) == 0, np.nan, a)))
  out.append(('NaN mean', np.where(np.arange(m.size) == 1, np.nan, m), a))
  out.append(('all equal', np.full(6, 1.7), np.zeros(5)))
  out.append(('constant, different', np.arange(6.) * 0.3, np.zeros(5)))
  return out


def test_host_stage_equals_diag_bit_for_bit(host):
  inputs = _host_inputs()
  lines = ['ess {} {} {} {}'.format(m.size, a.size, hex_words(m), hex_words(a)) for _, m, a in inputs]
  seen_full = seen_nan = seen_stop = False
  for (label, m, a), ans in zip(inputs, host(lines)):
    word = ans.split()
    got = np.array([int(word[0], 16)], np.uint64).view(np.float64)[0]
    want = diag.multi_chain_ess(m, a, m.size, a.size)
    ref = ref_ess(m, a)
    assert _same_bits(got, want), (label, got, want)
    if not np.isnan(want) and clear(ref):
      assert int(word[1]) == ref['k_star'], label
      seen_full |= ref['k_star'] == ref['K'] and ref['K'] > 1
      seen_stop |= ref['k_star'] < ref['K']
    seen_nan |= bool(np.isnan(want))
  assert seen_full and seen_nan and seen_stop
  by = {label: diag.multi_chain_ess(m, a, m.size, a.size) for label, m, a in inputs}
  assert np.isnan(by['all equal']) and np.isnan(by['NaN in A[0]']) and np.isnan(by['NaN mean'])
  # (a NaN at a later lag stops the scan there, as the definition says)
  assert np.isfinite(by['NaN in A'])
  assert np.isfinite(by['constant, different'])


def _layout(ans):
  word = ans.split()
  if word[0] == 'bad':
    return ' '.join(word)
  names = 'base h pairs run groups select thr part acov means stats bytes'.split()
  assert word[0] == 'ok' and len(word) == 1 + len(names)
  return dict(zip(names, (int(w) for w in word[1:])))


def test_layout_geometry_and_refusals(host):
  most, points = 512, 4096
  shapes = [(1, 4, 1, 0, 0), (1, 4, 1, 1, 9), (2, 5, 3, 1, 100), (33, 37, 2, 1, 100),
            (2004, 119, 10, 1, 100), (2 * most, 4096, 2, 0, 7), (2 * most + 1, 4097, 2, 1, 7),
            (33000, 16, 2, 1, 50), (2**20, 4096, 32, 0, 1000)]
  lines = ['ess_layout {} {} {} {} {}'.format(*s) for s in shapes]
  lines += ['ess_layout 8 4098 2 1 0', 'ess_layout 8 3 2 1 0', 'ess_layout 0 8 2 0 0',
            'ess_layout 8 8 0 0 0', 'ess_layout 8 8 2 0 -1', 'ess_layout {} 4096 1 1 0'.format(2**20),
            'ess_layout {} 4096 1 0 0'.format(2**20)]
  ans = [_layout(a) for a in host(lines)]
  for (n, count, d, bulk, sel), l in zip(shapes, ans):
    assert isinstance(l, dict), (n, count, l)
    h = count // 2
    assert l['h'] == h and l['pairs'] == -(-n // 2)
    assert l['groups'] <= most and l['run'] >= 1
    assert l['groups'] == -(-l['pairs'] // l['run'])      # every pair in one run,
    assert (l['groups'] - 1) * l['run'] < l['pairs']      # and no workgroup without one
    if l['pairs'] <= most:
      assert l['run'] == 1
    # behind the sort's scratch, in order, 256-byte aligned, disjoint, each as
    # large as what it holds
    assert (l['base'] > 0) == bool(bulk) and l['select'] == l['base']
    order = ['select', 'thr', 'part', 'acov', 'means', 'stats', 'bytes']
    need = [sel * 8, 2 * d * 8, l['groups'] * points * 8, 4 * d * h * 8, 8 * d * n * 8,
            6 * d * n * 8]
    for a, b, size in zip(order, order[1:], need):
      assert l[a] % 256 == 0 and l[b] - l[a] >= size, (n, count, a)
      assert l[b] - l[a] < size + 256
  assert ans[7]['run'] == 33 and ans[7]['groups'] == 500   # 16 500 pairs
  assert ans[9] == 'bad'        # h = 2 049
  assert ans[10] == 'bad rank' or ans[10] == 'bad'   # count = 3
  assert ans[11].startswith('bad') and ans[12].startswith('bad') and ans[13] == 'bad'
  assert ans[14] == 'bad rank'  # M = 2^32: the sort's refusal, for the bulk variant only
  assert isinstance(ans[15], dict) and ans[15]['base'] == 0
