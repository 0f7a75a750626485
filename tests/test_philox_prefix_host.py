"""pbh_philox.h on the CPU: the factored rounds 1-3 of several Philox blocks
of one (step pair, chain) must give the plain ten-round function's words.

tests/philox_prefix_main.cpp is built as a stand-alone program with the
address and undefined-behaviour sanitizers and run as a child process.  It
compares NB = 2, 4 and 7 blocks (the lane-pair kernel's d = 4, 10, 16), every
first block Q0 < NB, on the corners of the pair index and the chain id
(P_lo = 0 and 0xFFFFFFFF, P_hi and chain_hi zero and not) and on 10^5 random
(seed, h, P, chain); its own reference is checked against the published
known-answer vector."""
import os
import subprocess

import pytest

from host_program import compiler as _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'probayes_amd', 'csrc')
DRAWS = 100000
BLOCKS_PER_DRAW = 3 + 10 + 28        # sum over Q0 of NB - Q0, NB = 2, 4, 7
CORNERS = 4 * 4 * 6 * 2


@pytest.fixture(scope='module')
def program(tmp_path_factory):
  cxx = _compiler()
  if cxx is None:
    pytest.skip('no host C++ compiler')
  exe = str(tmp_path_factory.mktemp('philox_prefix') / 'philox_prefix_main')
  version = subprocess.run([cxx, '--version'], capture_output=True, text=True).stdout
  static = [] if 'clang' in version else ['-static-libasan', '-static-libubsan']
  subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-Wall',
                         '-fsanitize=address,undefined', '-fno-sanitize-recover=all'] + static +
                        ['-I', CSRC, os.path.join(ROOT, 'tests', 'philox_prefix_main.cpp'),
                         '-o', exe])
  return exe


def test_factored_rounds_equal_the_plain_function(program):
  r = subprocess.run([program, str(DRAWS)], capture_output=True, text=True)
  assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
  word = r.stdout.split()
  assert word[0] == 'ok'
  assert int(word[1]) == (DRAWS + CORNERS) * BLOCKS_PER_DRAW
  assert DRAWS >= 10 ** 5
