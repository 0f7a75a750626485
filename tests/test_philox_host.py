"""The host restatement of the Philox draw contracts (tests/philox_host.py):
known answers of the generator, no block drawn twice by any contract, and
the threshold's bits disjoint from the proposal's bits.  For the CondCov Gibbs
kernels: the block sets of the normals, the inversion uniforms and the ndtri
kernel's uniforms are disjoint and serve every coordinate once, the lane rule
is launch_gibbs_d's, and the host model of tests/test_gpu_gibbs_pin.py equals
oracle.gibbs.run_gibbs over whole chains; its checker bites."""
import numpy as np
import pytest

import philox_host as ph

# Random123's published known-answer vectors for philox4x32-10 (kat_vectors)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2,
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize('ctr,key,want', KAT)
def test_philox_known_answers(ctr, key, want):
  got = ph.philox4x32_10([np.array([c], np.uint64) for c in ctr], *key)
  assert tuple(int(w[0]) for w in got) == want
  # vectorised: the three vectors at once give the same words
  allc = [np.array([k[0][i] for k in KAT], np.uint64) for i in range(4)]
  if key == KAT[0][1]:
    got = ph.philox4x32_10(allc, *key)
    assert tuple(int(w[0]) for w in got) == want


def test_counter_and_key_layout():
  g, chain = (1 << 32) + 7, (3 << 32) + 9
  j, w1, w2, w3 = [int(np.ravel(v)[0]) for v in ph.ctr(5, g, chain)]
  assert (j, w1, w2, w3) == (5, 7, 9, 3 ^ (1 << 16))
  assert ph.key(0x0123456789ABCDEF) == (0x89ABCDEF, 0x01234567)
  # u01: NumPy's legacy random_sample construction, in [0, 1)
  assert ph.u01(np.uint64(0xFFFFFFFF), np.uint64(0xFFFFFFFF)) == 1. - 2. ** -53
  assert ph.u01(np.uint64(31), np.uint64(63)) == 0.


def _contracts(d):
  """(name, draw function) of every contract the kernels instantiate at d."""
  out = [('step_draws', lambda *a: ph.step_draws(*a)),
         ('uniform', lambda *a: ph.uniform_draws(*a)),
         ('f64 gauss', lambda *a: ph.f64_draws(*a, kind='gauss')),
         ('f64 uniform', lambda *a: ph.f64_draws(*a, kind='uniform'))]
  if d % 2 == 0 and d >= 4:
    out += [('pair', lambda *a: ph.pair_draws(*a)),
            ('f64 pair', lambda *a: ph.f64_draws(*a, pair=True))]
  return out


# 4 consecutive steps x 3 chains: a step pair and a chain pair straddling 2^32
G0 = (1 << 32) - 2
CHAINS = [5, (1 << 32) - 1, 1 << 32]


@pytest.mark.parametrize('d', range(1, 17))
def test_no_block_is_drawn_twice(d):
  for name, fn in _contracts(d):
    counters = {}
    n_blocks = 0
    for chain in CHAINS:
      _, _, blocks = fn(0x1234567 + (9 << 40), d, G0, 4, chain, 1)
      assert len(set(blocks)) == len(blocks)
      # a (j, slot) is consumed under one role only
      assert len({(j, s) for j, s, _ in blocks}) == len(blocks), (name, d)
      for j, slot, role in blocks:
        words = tuple(int(np.ravel(w)[0]) for w in ph.ctr(j, slot, chain))
        assert words not in counters, \
            '{} d={}: {} of chain {} and {} share counter {}'.format(
                name, d, (j, slot, role), chain, counters.get(words), words)
        counters[words] = (j, slot, role, chain)
        n_blocks += 1
    assert len(counters) == n_blocks
    # every step has a threshold block of its own, every role is present
    roles = {r for _, _, r, _ in counters.values()}
    assert any('threshold' in r for r in roles), (name, roles)
    assert sum('threshold' in v[2] for v in counters.values()) == 4 * len(CHAINS)


def test_block_lists_match_the_words_drawn():
  """The block list is what the draw function read: a draw computed from
  the listed blocks alone reproduces r and thr (step_draws at d = 3, the
  pair form at d = 10)."""
  seed, chain = 77, 12345
  r, thr, blocks = ph.step_draws(seed, 3, 9, 1, chain, 1)
  assert [(j, s) for j, s, _ in blocks] == [(0, 9), (1, 9), (0x40, 9)]
  w = [int(np.ravel(v)[0]) for j in (0, 1) for v in ph.block(seed, j, 9, chain)]
  z0, z1, _ = ph.bm96(w[0], w[1], w[2])
  z2, _, _ = ph.bm96(w[3], w[4], w[5])
  assert np.array_equal(r[0, :, 0], [z0, z1, z2])
  t = [int(np.ravel(v)[0]) for v in ph.block(seed, 0x40, 9, chain)]
  lead = w[6] >> 8
  assert thr[0, 0] == ph.u01(np.uint64((lead << 8) | (t[0] >> 24)), np.uint64(t[1]))
  # pair form, d = 10: steps 8, 9 share pair 4; half h's blocks 16 h .. 16 h + 3
  r, thr, blocks = ph.pair_draws(seed, 10, 8, 2, chain, 1)
  assert sorted((j, s) for j, s, _ in blocks) == sorted(
      [(q + 16 * h, 4) for h in range(2) for q in range(4)] + [(0x50, 8), (0x50, 9)])
  for h in range(2):
    w = [int(np.ravel(v)[0]) for q in range(4)
         for v in ph.block(seed, q + 16 * h, 4, chain)]
    z = []
    for q in range(5):
      z0, z1, _ = ph.bm96(w[3 * q], w[3 * q + 1], w[3 * q + 2])
      z += [z0, z1]
    assert np.array_equal(r[0, 5 * h:5 * h + 5, 0], z[:5])
    assert np.array_equal(r[1, 5 * h:5 * h + 5, 0], z[5:])
    if h == 1:
      for step, lead in ((0, w[15] >> 16), (1, w[15] & 0xFFFF)):
        t = [int(np.ravel(v)[0]) for v in ph.block(seed, 0x50, 8 + step, chain)]
        assert thr[step, 0] == ph.u01(np.uint64((lead << 16) | (t[0] >> 16)),
                                      np.uint64(t[1]))


@pytest.mark.parametrize('d', range(1, 17))
def test_threshold_bits_are_disjoint_from_the_proposal_bits(d):
  # uniform contract: the lead's 22 bits use none of the bits u01 keeps of
  # the words that feed a uniform at this d (block 0: x, y; z, w from d = 2)
  fields = ph.uniform_lead_fields(d)
  used = [0, 1] + ([2, 3] if d >= 2 else [])
  keep = {0: ph.U01_KEEP[0], 1: ph.U01_KEEP[1], 2: ph.U01_KEEP[0], 3: ph.U01_KEEP[1]}
  bits, dest = 0, 0
  for word, mask, sh in fields:
    if word in used:
      assert mask & keep[word] == 0, (d, word)
    n = bin(mask).count('1')
    bits += n
    placed = (mask << sh) if sh >= 0 else (mask >> -sh)
    assert placed & dest == 0 and placed < (1 << ph.UNIFORM_LEAD)
    dest |= placed
  assert bits == ph.UNIFORM_LEAD and dest == (1 << ph.UNIFORM_LEAD) - 1
  # the lead is really made of those fields
  rs = np.random.RandomState(d)
  w = [rs.randint(0, 2 ** 32, 64, dtype=np.uint64) for _ in range(4)]
  lead = ph.uniform_lead(w, d)
  w2 = [v.copy() for v in w]
  for word in used:
    w2[word] = (w2[word] & np.uint64(keep[word])) | (rs.randint(0, 64, 64, dtype=np.uint64)
                                                     & np.uint64(~keep[word] & 0xFFFFFFFF))
  if d >= 2:   # the uniforms do not see the lead's bits, and the other way round
    assert np.array_equal(ph.u01(w[0], w[1]), ph.u01(w2[0], w2[1]))
    assert np.array_equal(ph.u01(w[2], w[3]), ph.u01(w2[2], w2[3]))
    w3 = [v | np.uint64(keep[i]) for i, v in enumerate(w)]
    assert np.array_equal(ph.uniform_lead(w3, d), lead)
  # step_draws / PairDraw: the lead's word is no word of a normal pair, and
  # the words fit the blocks drawn
  layouts = [ph.step_layout(d)] + ([ph.pair_layout(d)] if d % 2 == 0 and d >= 4 else [])
  for pairs, lead_word, nb in layouts:
    words = [w for p in pairs for w in p]
    assert len(set(words)) == len(words) and lead_word not in words
    assert max(words + [lead_word]) < 4 * nb <= max(words + [lead_word]) + 4


def test_box_muller_host_form():
  """The quadrant-reduced host Box-Muller equals the plain construction to
  rounding, and is exact at the quadrant edges."""
  rs = np.random.RandomState(4)
  blk = [rs.randint(0, 2 ** 32, 4096, dtype=np.uint64) for _ in range(4)]
  blk[2][:4] = [0, 0x40000000, 0x80000000, 0xC0000000]
  blk[3][:4] = 0
  z0, z1 = ph.box_muller(blk)
  u1, u2 = 1. - ph.u01(blk[0], blk[1]), ph.u01(blk[2], blk[3])
  r = np.sqrt(-2. * np.log(u1))
  assert np.max(np.abs(z0 - r * np.cos(2 * np.pi * u2)) / np.maximum(1., r)) < 1e-15
  assert np.max(np.abs(z1 - r * np.sin(2 * np.pi * u2)) / np.maximum(1., r)) < 1e-15
  assert np.array_equal(z0[:4], r[:4] * [1, 0, -1, 0])
  assert np.array_equal(z1[:4], r[:4] * [0, 1, 0, -1])


def test_checker_accepts_the_oracle_chain_and_bites():
  """check_steps (tests/test_gpu_philox_pin.py) on a trace the oracle made
  from the host streams passes with zero error; the same trace against a
  stream with two normals swapped, or a threshold lead one bit off, fails."""
  import oracle
  from test_gpu_philox_pin import check_steps, _diag_spec, _spread, _norm, SEED
  spec = _norm(_diag_spec(4, 0.5))
  n, t = 33, 24
  init = _spread(spec, n, 3)
  r, thr, _ = ph.pair_draws(SEED, 4, 0, t, 0, n)
  ref = oracle.run_mh(spec, init, ph.streams(r, thr))
  trace = {k: ref[k] for k in ('v_x', 'v_p', 'u', 'p_x', 'p_p', 's')}
  trace['n_acc'] = ref['u'].sum(axis=1)
  out = check_steps(spec, trace, r, thr, init)
  assert out['ties'] == 0 and out['v_x'] == 0. and out['v_p'] == 0.
  with pytest.raises(AssertionError):
    check_steps(spec, trace, r[:, [1, 0, 2, 3]], thr, init)
  with pytest.raises(AssertionError):
    check_steps(spec, trace, r, thr * 0.5, init)
  bad = dict(trace, n_acc=trace['n_acc'] + 1)
  with pytest.raises(AssertionError):
    check_steps(spec, bad, r, thr, init)
  moved = dict(trace, v_p=np.where(ref['u'] == 0, np.nextafter(ref['v_p'], 0.), ref['v_p']))
  with pytest.raises(AssertionError):     # a rejected step must keep its record's bits
    check_steps(spec, moved, r, thr, init)


# ---------------------------------------------------------------------------
# the CondCov Gibbs kernels' contract
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('d', range(1, 17))
def test_gibbs_blocks_are_disjoint_and_serve_every_coordinate_once(d):
  for L in ph.gibbs_lane_choices(d):
    normals, invert = ph.gibbs_layout(d, L)
    # every coordinate has a (block, component) and an inversion block of its own
    assert len(normals) == d and len(set(normals)) == d
    assert all(c in (0, 1) for _, c in normals)
    assert invert == [ph.GIBBS_INVERT + k for k in range(d)]
    M = d // L
    for k, (j, c) in enumerate(normals):
      assert (j, c) == (ph.GIBBS_NORMALS + 16 * (k // M) + (k % M) // 2, (k % M) % 2)
    # a part's pairs stay below the next part's base
    assert (M + 1) // 2 <= 16
    for tsteps in range(1, d + 1):
      a, b, c = ph.gibbs_blocks(d, L, tsteps)
      assert not (a & b) and not (a & c) and not (b & c), (d, L, tsteps)
      assert len(b) == d and len(c) == tsteps and len(a) == L * ((M + 1) // 2)
  # d = 1 .. 16 never meets the MH kernels' tail blocks either
  assert ph.TAIL_STEP not in a | b and ph.TAIL_PAIR not in a | b


def test_gibbs_lanes_rule():
  for d in range(1, 17):
    want = 1 if d % 2 else (2 if d <= 12 else (4 if d % 4 == 0 else 2))
    assert ph.gibbs_lanes(d, {}) == want
    for L in (1, 2, 4):
      got = ph.gibbs_lanes(d, {'PBH_GIBBS_LANES': str(L)})
      assert got == (L if d % L == 0 else want)
    for bad in ('3', '8', '0', '-2', 'x', ''):
      assert ph.gibbs_lanes(d, {'PBH_GIBBS_LANES': bad}) == want
  assert [ph.gibbs_lanes(d, {}) for d in (8, 14, 16)] == [2, 2, 4]


def test_gibbs_draws_are_keyed_by_the_cycle_start():
  """Steps of one cycle share the cycle's draws, whatever step a window starts
  at; the uniforms of gibbs_kernel are keyed by the step itself."""
  seed, d, L, n = 99, 6, 2, 3
  z, u = ph.gibbs_fast_draws(seed, d, L, 1, 0, 18, 7, n)
  assert np.array_equal(z[0], z[5]) and np.array_equal(u[6], u[11])
  assert not np.array_equal(z[5], z[6])
  z2, u2 = ph.gibbs_fast_draws(seed, d, L, 1, 4, 9, 7, n)      # a mid-cycle origin
  assert np.array_equal(z2, z[4:13]) and np.array_equal(u2, u[4:13])
  # tsteps = 4: nblk = 2, cycles start at even steps
  z4, _ = ph.gibbs_fast_draws(seed, d, L, 4, 0, 4, 7, n)
  assert np.array_equal(z4[0], z4[1]) and np.array_equal(z4[0], z[0])
  assert np.array_equal(z4[2], z4[3]) and not np.array_equal(z4[2], z4[0])
  # by hand: coordinate 4 = part 1, ii = 1 -> component 1 of block 0x100 + 16
  chain = np.array([[7, 8, 9]], np.uint64)
  z0, z1 = ph.box_muller(ph.block(seed, 0x110, np.array([[6]], np.uint64), chain))
  assert np.array_equal(z[6, 4], z1[0]) and np.array_equal(z[6, 3], z0[0])
  w = ph.block(seed, 0x204, np.array([[6]], np.uint64), chain)
  assert np.array_equal(u[8, 4], ph.u01(w[0], w[1])[0])
  s = ph.gibbs_uniform_streams(seed, d, 4, 5, 3, 7, n)
  w = ph.block(seed, 2, np.array([[6]], np.uint64), chain)
  assert s.shape == (3, 4, n) and np.array_equal(s[1, 2], ph.u01(w[0], w[1])[0])


def _anchor_spec(d, tsteps, lo, hi):
  from test_gpu_gibbs_fast import _spec_d
  from test_gpu_gibbs_pin import _norm2d
  if d == 2:
    return _norm2d(lo, hi, tsteps)
  spec = _spec_d(d, 7, lo, hi)
  spec['proposal']['tsteps'] = tsteps
  return spec


ANCHOR = [(3, 1, 1, -1., 1.5), (2, 2, 2, -0.5, 1.), (8, 2, 1, -1.5, 2.), (4, 4, 3, -1.5, 2.)]


@pytest.mark.parametrize('d,L,tsteps,lo,hi', ANCHOR)
def test_gibbs_host_model_equals_the_oracle(d, L, tsteps, lo, hi):
  """Whole chains of the host model (tests/test_gpu_gibbs_pin.py) equal
  oracle.gibbs.run_gibbs on the equivalent uniforms: (ndtr(z) - cdf_lo) /
  (cdf_hi - cdf_lo) where the normal lies inside the limits, the inversion
  uniform where it does not.  1e-12 absolute at |x| = O(1); the round trip
  ndtri(ndtr(z)) costs under eps / phi(2.8) = 3e-14 with every |zlim| <= 2.8.
  Measured: 3.6e-15, 1.1e-15, 4.0e-15, 9.3e-15 with 263, 1 002, 154, 205
  inversion draws."""
  import oracle.gibbs
  import scipy.stats
  from test_gpu_gibbs_pin import host_chain, tables, _init
  spec = _anchor_spec(d, tsteps, lo, hi)
  tb = tables(spec)
  # (d = 4 has one limit at 3.06: eps / phi(3.06) = 6e-14, still a tenth of the bar)
  zmax = max(np.abs(tb.zlo).max(), np.abs(tb.zhi).max())
  assert np.finfo(float).eps / scipy.stats.norm.pdf(zmax) <= 1e-13, zmax
  n, t = 24, 40
  init = _init(spec, n, d)
  vx, streams, n_inv = host_chain(spec, L, init, t)
  assert 0 < n_inv < streams.size and np.all((streams >= 0) & (streams < 1))
  ref = oracle.gibbs.run_gibbs(spec, init, streams)
  err = float(np.max(np.abs(vx - ref['v_x'])))
  print('d {} L {} tsteps {}: {} inversion draws, max abs err {:.3g}'.format(
      d, L, tsteps, n_inv, err))
  assert err <= 1e-12, err


def test_gibbs_checker_accepts_the_host_chain_and_bites():
  """check_gibbs_steps on a trace the host model made passes with zero
  error; a trace made with another lane layout, with a pair's components
  swapped, with the step in place of the cycle start, or with a moved v_p,
  accept word or untouched coordinate fails."""
  from test_gpu_gibbs_fast import _spec_d
  import scipy.special
  from test_gpu_gibbs_pin import check_gibbs_steps, host_trace, ndtri_mp, _init
  for p in (1e-3, 0.0668, 0.3, 0.5, 0.77, 0.9772, 0.997):
    z = ndtri_mp(p)
    assert abs(z - scipy.special.ndtri(p)) <= 1e-15 * max(1., abs(z)), p
  spec = _spec_d(8, 7, -1.5, 2.)
  n, t = 37, 48
  init = _init(spec, n, 8)
  trace = host_trace(spec, 2, init, t)
  out = check_gibbs_steps(spec, trace, 2, init)
  assert out['ties'] == 0 and out['v_x_bm'] == 0. and out['v_x_inv'] == 0.
  assert out['v_p'] == 0. and 0.02 <= out['share'][0] <= out['share'][1] <= 0.98
  for L in (1, 4):                                   # another routing of the same draws
    with pytest.raises(AssertionError):
      check_gibbs_steps(spec, trace, L, init)
  orig = ph.box_muller
  try:
    ph.box_muller = lambda blk: orig(blk)[::-1]      # z0 and z1 swapped
    with pytest.raises(AssertionError):
      check_gibbs_steps(spec, trace, 2, init)
  finally:
    ph.box_muller = orig
  starts = ph.gibbs_cycle_starts
  try:                                               # keyed by the step, not the cycle start
    ph.gibbs_cycle_starts = lambda d, ts, g0, T: (-(-d // ts), list(range(g0, g0 + T)))
    with pytest.raises(AssertionError):
      check_gibbs_steps(spec, trace, 2, init)
  finally:
    ph.gibbs_cycle_starts = starts
  bad = dict(trace, v_p=trace['v_p'] * (1 + 3e-9))
  with pytest.raises(AssertionError):
    check_gibbs_steps(spec, bad, 2, init)
  words = trace['acc_words'].copy()
  words[5, 0] |= np.uint64(1) << np.uint64(n)        # a bit past the last chain
  with pytest.raises(AssertionError):
    check_gibbs_steps(spec, dict(trace, acc_words=words), 2, init)
  vx = trace['v_x'].copy()
  vx[3, 9, 5] = np.nextafter(vx[3, 9, 5], 9.)        # step 9 updates coordinate 1 only
  with pytest.raises(AssertionError):
    check_gibbs_steps(spec, dict(trace, v_x=vx), 2, init)
  mom = dict(trace['moments'], n_acc=trace['moments']['n_acc'] - 1)
  with pytest.raises(AssertionError):
    check_gibbs_steps(spec, dict(trace, moments=mom), 2, init)
