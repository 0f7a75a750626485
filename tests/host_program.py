"""What the CPU tests that drive a stand-alone C++ program share: the search
for a host compiler, the build with the address and undefined-behaviour
sanitizers, the request/answer runner, and the words a double travels as.

The program of the trace reductions (tests/trace_host_main.cpp with
probayes_amd/csrc/pbh_trace_host.cpp, -ffp-contract=off as the library builds
the unit) is the `host` fixture: test_trace_host.py, test_rank_host.py and
test_ess_rank_host.py import it, and each builds the program once and sends
its own requests.  test_expr_host.py and test_philox_prefix_host.py take the
compiler search."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'probayes_amd', 'csrc')


def compiler():
  for name in ('c++', 'g++', 'clang++', '/opt/rocm/lib/llvm/bin/clang++'):
    path = shutil.which(name)
    if path:
      return path
  return None


def build_sanitized(cxx, sources, exe, flags=()):
  """sources -> exe, a program of its own with nothing preloaded"""
  # the sanitizer runtimes linked into the program (clang's default), so that
  # it runs whatever else the loader brings in first
  version = subprocess.run([cxx, '--version'], capture_output=True, text=True).stdout
  static = [] if 'clang' in version else ['-static-libasan', '-static-libubsan']
  subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-Wall'] + list(flags) +
                        ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'] + static +
                        list(sources) + ['-o', exe])


def runner(exe, tmp):
  """run(lines) -> the program's answers, one per request line"""
  def run(lines):
    req = tmp / 'requests.txt'
    req.write_text(''.join(l + '\n' for l in lines))
    r = subprocess.run([exe, str(req)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out
  return run


@pytest.fixture(scope='module')
def host(tmp_path_factory):
  """run(lines) of the trace reductions' program"""
  cxx = compiler()
  if cxx is None:
    pytest.skip('no host C++ compiler')
  tmp = tmp_path_factory.mktemp('trace_host')
  exe = str(tmp / 'trace_host_main')
  build_sanitized(cxx, [os.path.join(ROOT, 'tests', 'trace_host_main.cpp'),
                        os.path.join(CSRC, 'pbh_trace_host.cpp')], exe, ['-ffp-contract=off'])
  return runner(exe, tmp)


def hex_words(a):
  return ' '.join('{:016x}'.format(int(b)) for b in
                  np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64))


def doubles(words):
  return np.array([int(w, 16) for w in words], np.uint64).view(np.float64)
