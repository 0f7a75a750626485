"""The host side of the pooled covariance (no GPU): pbh_trace_host.cpp's
cov_layout and cov_finish, driven by the stand-alone program tests/
cov_host_main.cpp built with a host compiler alone, -ffp-contract=off and the
address and undefined-behaviour sanitizers, and run as a child process.

cov_finish must equal diag.pooled_cov_finish bit for bit: the ABI's last step
is the definition's, operation for operation."""
import os

import numpy as np
import pytest

from probayes_amd import diag
from host_program import CSRC, ROOT, build_sanitized, compiler, doubles, hex_words, runner

LANES, TILE, HALF, GROUPS, MAX_DIM = 256, 16, 8, 1024, 32
SHAPES = [(1, 2, 1), (6, 37, 2), (130, 40, 32), (2004, 160, 10), (33000, 8, 10),
          (65536, 1250, 17)]


@pytest.fixture(scope='module')
def host(tmp_path_factory):
  cxx = compiler()
  if cxx is None:
    pytest.skip('no host C++ compiler')
  tmp = tmp_path_factory.mktemp('cov_host')
  exe = str(tmp / 'cov_host_main')
  build_sanitized(cxx, [os.path.join(ROOT, 'tests', 'cov_host_main.cpp'),
                        os.path.join(CSRC, 'pbh_trace_host.cpp')], exe, ['-ffp-contract=off'])
  return runner(exe, tmp)


def layout(host, n, count, d):
  ans = host(['layout {} {} {}'.format(n, count, d)])[0].split()
  if ans[0] == 'refused':
    return None
  keys = ('pairs', 'chain_blocks', 'slices', 'slice_len', 'rows', 'cols', 'K', 'part', 'res',
          'bytes')
  return dict(zip(keys, (int(v) for v in ans[1:])))


@pytest.mark.parametrize('n,count,d', SHAPES)
def test_layout(host, n, count, d):
  l = layout(host, n, count, d)
  assert l is not None
  assert l['chain_blocks'] == -(-n // LANES)
  # one tile up to 16 dims; above, two diagonal tiles and, per 8 dims of the
  # second, a rectangle for either half of the first
  assert l['pairs'] == (1 if d <= TILE else 2 + 2 * -(-(d - TILE) // HALF))
  assert l['cols'] == d + d * (d + 1) // 2
  # the slices cover the count exactly, the last one not empty
  assert 1 <= l['slices'] <= count
  assert (l['slices'] - 1) * l['slice_len'] < count <= l['slices'] * l['slice_len']
  assert l['rows'] == l['chain_blocks'] * l['slices']
  # about kPointwiseGroups workgroups when the records allow it, never many more
  groups = l['chain_blocks'] * l['pairs']
  grid = groups * l['slices']
  assert grid >= min(GROUPS, groups * count) // 2 and grid < max(groups, GROUPS) + groups
  # the regions: multiples of 256, in order, disjoint, inside bytes
  regions = [(l['K'], d * 8), (l['part'], l['rows'] * l['cols'] * 8), (l['res'], l['cols'] * 8)]
  end = 0
  for at, size in regions:
    assert at % 256 == 0 and at >= end
    end = at + size
  assert l['bytes'] >= end and l['bytes'] % 256 == 0


def test_layout_of_known_shapes(host):
  assert layout(host, 1, 2, 1) == dict(pairs=1, chain_blocks=1, slices=2, slice_len=1, rows=2,
                                       cols=2, K=0, part=256, res=512, bytes=768)
  l = layout(host, 65536, 1250, 17)
  assert (l['pairs'], l['chain_blocks'], l['slices'], l['slice_len']) == (4, 256, 1, 1250)
  l = layout(host, 65536, 1250, 10)
  assert (l['pairs'], l['slices'], l['slice_len'], l['rows']) == (1, 4, 313, 1024)
  l = layout(host, 130, 40, 32)
  assert (l['pairs'], l['chain_blocks'], l['slices'], l['slice_len']) == (6, 1, 40, 1)
  l = layout(host, 33000, 8, 10)
  assert (l['chain_blocks'], l['slices'], l['rows']) == (129, 8, 1032)


def test_layout_refusals(host):
  for n, count, d in ((0, 4, 2), (-1, 4, 2), (4, 0, 2), (4, -3, 2), (4, 4, 0), (4, 4, -1),
                      (4, 4, MAX_DIM + 1), (2 ** 62, 4, 2), (2 ** 33, 2 ** 31, 2),
                      (2 ** 40, 1, 2)):
    assert layout(host, n, count, d) is None, (n, count, d)
  assert layout(host, 4, 4, MAX_DIM) is not None


def test_the_packed_triangle(host):
  for d in (1, 2, 16, 17, 32):
    ia, ib = np.triu_indices(d)
    got = host(['tri {} {} {}'.format(a, b, d) for a, b in zip(ia, ib)])
    assert [int(v) for v in got] == list(range(d * (d + 1) // 2))


@pytest.mark.parametrize('d', [1, 2, 16, 17, 32])
def test_finish_equals_the_definition_bit_for_bit(host, d):
  rng = np.random.RandomState(100 + d)
  nt = d * (d + 1) // 2
  lines, want = [], []
  for case in range(6):
    M = int(rng.randint(2, 10 ** 9)) if case else 2
    K = rng.normal(size=d) * 10. ** rng.randint(-3, 7)
    v = rng.normal(size=(d + 3, d)).dot(rng.normal(size=(d, d)))
    S = v.sum(axis=0) * np.sqrt(M)
    full = v.T.dot(v) * M
    if case == 3:
      S[0], full[0, :] = 0., 0.          # a dim that never moved: 0 / 0 on its row
    if case == 4:
      S[d - 1] = np.nan                  # a NaN record in the last dim
    if case == 5:
      full = -full                       # a negative variance: sqrt gives NaN
    P = full[np.triu_indices(d)]
    assert P.size == nt
    lines.append('finish {} {} {} {} {}'.format(d, M, hex_words(K), hex_words(S), hex_words(P)))
    want.append(diag.pooled_cov_finish(K, S, P, M))
  for ans, ref in zip(host(lines), want):
    got = doubles(ans.split())
    assert got.size == d + 2 * d * d
    assert got[:d].tobytes() == ref['mean'].tobytes()
    assert got[d:d + d * d].tobytes() == ref['cov'].tobytes()
    assert got[d + d * d:].tobytes() == ref['corr'].tobytes()
  # the outputs are optional
  alone = doubles(host([lines[0].replace('finish', 'finish_cov', 1)])[0].split())
  assert alone.tobytes() == want[0]['cov'].tobytes()
