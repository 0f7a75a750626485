"""pbh_trace_hist and pbh_trace_hist2d at the ABI level (CPU): the symbols, their
signatures in _lib.py and in include/pbhip.h, the argument checks that need no
device, the revision they leave alone, and the facade's refusals that need no
engine -- those of Sampler.trace_hist, trace_hist2d and trace_corner."""
import ctypes
import os
import re

import pytest

import probayes_amd as pb
from probayes_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP, IP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
I64P, I64, I32 = ctypes.POINTER(ctypes.c_int64), ctypes.c_int64, ctypes.c_int32
ARGTYPES = {'pbh_trace_hist': [ctypes.c_void_p, I64, I64, IP, DP, I64P, I64P],
            'pbh_trace_hist2d': [ctypes.c_void_p, I64, I64, IP, DP, I32, IP, I64P]}
PARAMS = {'pbh_trace_hist': ['pbh_engine *eng', 'int64_t first', 'int64_t count',
                             'const int32_t *n_bins', 'const double *edges', 'int64_t *counts',
                             'int64_t *outside'],
          'pbh_trace_hist2d': ['pbh_engine *eng', 'int64_t first', 'int64_t count',
                               'const int32_t *n_bins', 'const double *edges', 'int32_t n_pairs',
                               'const int32_t *pairs', 'int64_t *counts']}
NAMES = sorted(ARGTYPES)


def _header():
  with open(os.path.join(ROOT, 'include', 'pbhip.h')) as f:
    return f.read()


@pytest.mark.parametrize('name', NAMES)
def test_library_exports(name):
  lib = _lib.load()
  assert hasattr(lib, name) and name in _lib.SIGNATURES
  restype, argtypes = _lib.SIGNATURES[name]
  assert restype is ctypes.c_int
  assert argtypes == ARGTYPES[name]
  assert list(getattr(lib, name).argtypes) == list(argtypes)


@pytest.mark.parametrize('name', NAMES)
def test_signature_is_the_headers(name):
  m = re.search(r'int {}\(([^)]*)\);'.format(name), _header())
  assert m is not None
  assert [' '.join(p.split()) for p in m.group(1).split(',')] == PARAMS[name]


def test_the_limits_are_the_headers():
  text = _header()
  assert re.search(r'#define PBH_HIST_MAX_BINS 4096\b', text)
  assert re.search(r'#define PBH_HIST2D_MAX_CELLS 16384\b', text)
  # the rule is stated in full, and what the calls leave alone
  comment = text[text.index('Posterior histograms'):text.index('#define PBH_HIST_MAX_BINS')]
  for words in ('e[i] <= x < e[i + 1]', 'x == e[B]', 'below', 'above', 'NaN', '-0.0 and +0.0',
                '-inf', 'np.histogram2d', 'Changes nothing in the engine'):
    assert words in comment, words


def test_the_revision_and_the_version_stay():
  # added within revision 2: a caller finds them by the symbol, not the number
  lib = _lib.load()
  assert lib.pbh_abi_revision() == _lib.ABI_REVISION == 2
  assert lib.pbh_abi_version() == _lib.ABI_VERSION == 7
  text = _header()
  assert '#define PBH_ABI_REVISION 2' in text and '#define PBH_ABI_VERSION 7' in text


def _args(name, counts):
  n_bins = (ctypes.c_int32 * 2)(2, 2)
  edges = (ctypes.c_double * 6)(0., 1., 2., 0., 1., 2.)
  if name == 'pbh_trace_hist':
    return [n_bins, edges, counts, None]
  return [n_bins, edges, 1, (ctypes.c_int32 * 2)(0, 1), counts]


@pytest.mark.parametrize('name', NAMES)
def test_null_engine_is_refused_with_a_message(name):
  lib = _lib.load()
  out = (ctypes.c_int64 * 8)()
  assert getattr(lib, name)(None, 0, 4, *_args(name, out)) == -1   # PBH_ERR_ARG
  assert b'engine' in lib.pbh_last_error()


@pytest.mark.parametrize('name', NAMES)
def test_no_output_is_refused_with_a_message(name):
  lib = _lib.load()
  assert getattr(lib, name)(None, 0, 4, *_args(name, None)) == -1   # PBH_ERR_ARG
  msg = lib.pbh_last_error()
  assert b'no output' in msg and b'NULL' in msg and name.encode() in msg


CALLS = [('trace_hist', ()), ('trace_hist2d', ('x', 'x')), ('trace_corner', ())]


@pytest.mark.parametrize('method,args', CALLS)
def test_sampler_without_an_engine_refuses(method, args):
  x = pb.RV('x', vtype=float, vset=(-1., 1.))
  process = pb.SP(x)
  batched = process.sampler({'x': 0.}, stop=8, chains=4, rng='philox')
  with pytest.raises(ValueError, match='no engine'):
    getattr(batched, method)(*args)
  single = process.sampler({'x': 0.}, stop=8)
  with pytest.raises(ValueError, match='batched'):
    getattr(single, method)(*args)
