"""pbh_trace_cov at the ABI level (CPU): the symbol, its signature in _lib.py
and in include/pbhip.h, the argument checks that need no device, the revision
it leaves alone, and the facade's refusals that need no engine -- those of
Sampler.trace_cov and of Sampler.trace_tran, which also names why a lowered
proposal takes no covariance."""
import ctypes
import os
import re

import pytest

import probayes_amd as pb
from probayes_amd import _lib
from mcmc_examples import DELTA_WORKLOADS, WORKLOADS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP, I64 = ctypes.POINTER(ctypes.c_double), ctypes.c_int64
NAME = 'pbh_trace_cov'


def test_library_exports():
  lib = _lib.load()
  assert hasattr(lib, NAME) and NAME in _lib.SIGNATURES
  restype, argtypes = _lib.SIGNATURES[NAME]
  assert restype is ctypes.c_int
  assert argtypes == [ctypes.c_void_p, I64, I64, DP, DP, DP]
  assert list(getattr(lib, NAME).argtypes) == list(argtypes)


def test_signature_is_the_headers():
  with open(os.path.join(ROOT, 'include', 'pbhip.h')) as f:
    text = f.read()
  m = re.search(r'int {}\(([^)]*)\);'.format(NAME), text)
  assert m is not None
  params = [' '.join(p.split()) for p in m.group(1).split(',')]
  assert params == ['pbh_engine *eng', 'int64_t first', 'int64_t count', 'double *mean',
                    'double *cov', 'double *corr']


def test_the_revision_and_the_version_stay():
  # added within revision 2: a caller finds it by the symbol, not the number
  lib = _lib.load()
  assert lib.pbh_abi_revision() == _lib.ABI_REVISION == 2
  assert lib.pbh_abi_version() == _lib.ABI_VERSION == 7
  with open(os.path.join(ROOT, 'include', 'pbhip.h')) as f:
    text = f.read()
  assert '#define PBH_ABI_REVISION 2' in text and '#define PBH_ABI_VERSION 7' in text


def test_null_engine_is_refused_with_a_message():
  lib = _lib.load()
  out = (ctypes.c_double * 4)()
  assert getattr(lib, NAME)(None, 0, 4, out, None, None) == -1   # PBH_ERR_ARG
  assert b'engine' in lib.pbh_last_error()


def test_no_output_is_refused_with_a_message():
  lib = _lib.load()
  assert getattr(lib, NAME)(None, 0, 4, None, None, None) == -1   # PBH_ERR_ARG
  msg = lib.pbh_last_error()
  assert b'no output' in msg and b'NULL' in msg


@pytest.mark.parametrize('method', ['trace_cov', 'trace_tran'])
def test_sampler_without_an_engine_refuses(method):
  x = pb.RV('x', vtype=float, vset=(-1., 1.))
  process = pb.SP(x)
  batched = process.sampler({'x': 0.}, stop=8, chains=4, rng='philox')
  with pytest.raises(ValueError, match='no engine'):
    getattr(batched, method)()
  single = process.sampler({'x': 0.}, stop=8)
  with pytest.raises(ValueError, match='batched'):
    getattr(single, method)()


def _lowered(name):
  """A batched sampler of the example, lowered through SP.lower, no engine."""
  table = WORKLOADS if name in WORKLOADS else DELTA_WORKLOADS
  builder, params = table[name][:2]
  process, init, extra, kwds, _ = builder(pb, params)
  sampler = process.sampler(init, extra, stop=8, chains=4, rng='philox', **kwds)
  sampler._lower()
  assert sampler.spec is not None and sampler._eng is None
  return sampler


@pytest.mark.parametrize('name,why', [('randint2', 'is an int'), ('bound_sphere2', 'bounded'),
                                      ('bound_list3', 'bounded'), ('gibbs_norm2d', 'Gibbs'),
                                      ('metrohast_norm1d', 'ufun')])
def test_trace_tran_names_why_a_proposal_takes_no_covariance(name, why):
  sampler = _lowered(name)
  with pytest.raises(ValueError, match=why):
    sampler.trace_tran()
  # the covariance itself is still on offer: only the engine is missing
  with pytest.raises(ValueError, match='no engine'):
    sampler.trace_cov()


def test_trace_tran_accepts_an_additive_gaussian_walk():
  for name in ('covrw5', 'diag10'):
    sampler = _lowered(name)
    assert sampler._tran_refusal() is None
    with pytest.raises(ValueError, match='no engine'):
      sampler.trace_tran()
