"""The lane-pair kernel's factored Philox rounds (pbh_philox.h) around a
change of the pair index's high word, P = step / 2 = 2^32, i.e. step 2^33.

The steady-state (FULL) form builds per-lane words for one value of that high
word, so a launch or server command that crosses the boundary must take the
general form (pair_full_form, pbh_run's server checks), and FULL itself must
be right on either side of it:

 * the production draws pinned to the oracle across the boundary
   (tests/test_gpu_philox_pin.py's helpers, its RTOL), even and odd origin,
   and chain ids straddling 2^32 at the same time;
 * FULL bit-equal to the general form (PBH_PAIR_FULL=0) for launch splits that
   cross the boundary, lie wholly below it (P_hi = 0) and wholly above it
   (P_hi = 1);
 * the resident server bit-equal to launches: a command that crosses is a
   launch, a command that starts exactly at the boundary (the server has seen
   only P_hi = 0 until then) rebuilds the words inside the resident kernel.

A run right after Engine.set_step has no predecessor and takes the general
form whatever its shape, so every plan below starts with a short run and the
runs after it are the ones under test."""
import numpy as np
import pytest

from test_gpu_philox_pin import RTOL, _pin, _wide_case

pytestmark = pytest.mark.gpu

B = 2 ** 33          # the first step of pair 2^32
SEED = 77


def _crosses(g, n):
  return g < B <= g + n - 1


# ---------------------------------------------------------------------------
# 1: the oracle across the boundary
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('step0,chain_offset', [(B - 30, 0), (B - 29, 0), (B - 30, 2 ** 32 - 40)])
def test_oracle_pin_across_the_pair_boundary(step0, chain_offset):
  """96 chains of the normalised cfg2 spec; launches 1, 4 x 1, then 56 steps
  in launches of 13: the second of those holds steps 2^33 - 1 and 2^33, the
  first is FULL below the boundary and the later ones FULL above it."""
  assert RTOL == 1e-12
  spec, init, contract, kw = _wide_case('pair')
  assert init.shape[0] == 96
  launches = ((1, 0), (4, 1), (56, 13))
  g = step0 + 5
  spans = [(g + 13 * i, min(13, 56 - 13 * i)) for i in range(5)]
  assert sum(_crosses(a, n) and n > 1 for a, n in spans) == 1
  assert spans[0][0] + spans[0][1] <= B and spans[2][0] > B
  _pin(spec, init, contract, launches=launches, step0=step0, chain_offset=chain_offset, **kw)


# ---------------------------------------------------------------------------
# 2: FULL equals the general form
# ---------------------------------------------------------------------------
def _trace(monkeypatch, env, n, step0, plan, cap):
  import bench
  from probayes_amd import Engine
  for k, v in env.items():
    monkeypatch.setenv(k, v)
  eng = Engine(bench.cfg2_spec())
  eng.init_chains(np.random.RandomState(3).normal(size=(n, bench.D)))
  eng.set_step(step0)
  eng.set_rng('philox', seed=SEED)
  eng.set_collect(moments=False)
  eng.alloc_trace(cap, 1)
  infos = []
  for k in plan:
    eng.run(k, steps_per_launch=k)
    infos.append(eng.server_info())
  tr, st = eng.trace(), eng.state()
  eng.close()
  return tr, st, infos


def _same(a, b):
  (ta, sa), (tb, sb) = a, b
  for k in ('v_x', 'v_p', 'u'):
    assert np.array_equal(ta[k], tb[k]), k
  assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])
  assert 0.05 < ta['u'].mean() < 0.95


# the issue's splits (40), (7, 33), (1, 39) from both origins: the run that
# crosses is general either way; (1, 9, 30) and (1, 25, 14) add a FULL launch
# just below and just above the crossing one
CROSSING = [(g0, plan) for g0 in (B - 20, B - 21)
            for plan in ((40,), (7, 33), (1, 39), (1, 9, 30), (1, 25, 14))]
# wholly below (P_hi = 0, the last pair of it included) and wholly above
ONE_SIDE = [(B - 40, (1, 39)), (B - 41, (1, 39)), (B + 2, (1, 39)), (B + 1, (1, 39))]


@pytest.mark.parametrize('g0,plan', CROSSING + ONE_SIDE)
def test_full_form_equals_general_form_at_the_boundary(monkeypatch, g0, plan):
  assert sum(plan) == 40
  out = {}
  for full in ('1', '0'):
    tr, st, _ = _trace(monkeypatch, {'PBH_PAIR_FULL': full, 'PBH_SERVER': '0'}, 64, g0, plan, 40)
    out[full] = (tr, st)
  _same(out['1'], out['0'])


# ---------------------------------------------------------------------------
# 3: the server
# ---------------------------------------------------------------------------
# (origin, commands).  B - 45: the issue's 3, 20, 17 end at B - 5 without
# crossing, so 5 more steps end exactly at the boundary and the next command
# starts on it -- the resident kernel rebuilds its words.  B - 25: the 17
# crosses.  B + 2: wholly above.
SERVER = [(B - 45, (3, 20, 17, 5, 10)), (B - 25, (3, 20, 17, 6)), (B + 2, (3, 20, 17))]


@pytest.mark.parametrize('g0,plan', SERVER)
def test_server_commands_equal_launches_at_the_boundary(monkeypatch, g0, plan):
  n, cap = 512, sum(plan)
  tr_ref, st_ref, _ = _trace(monkeypatch, {'PBH_SERVER': '0'}, n, g0, plan, cap)
  tr, st, infos = _trace(monkeypatch, {'PBH_SERVER': '1'}, n, g0, plan, cap)
  _same((tr, st), (tr_ref, st_ref))
  g, commands = g0, 0
  for i, (k, info) in enumerate(zip(plan, infos)):
    # the first run has no predecessor; a crossing run is a launch that stops
    # the server; every other run is a command to it
    launch = i == 0 or _crosses(g, k)
    commands += 0 if launch else 1
    assert info['commands'] == commands, (i, info)
    assert info['active'] == (not launch), (i, info)
    g += k
  if g0 == B - 25:
    assert [_crosses(g0 + sum(plan[:i]), k) for i, k in enumerate(plan)] == \
        [False, False, True, False]
    assert infos[-1]['launches'] == 2, infos      # relaunched after the crossing run
  else:
    assert infos[-1]['launches'] == 1, infos
