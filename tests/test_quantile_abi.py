"""pbh_trace_quantile at the ABI level (CPU): the symbol, its argument
checks that need no device, the revision it bumps, and the facade's refusals
that need no engine."""
import ctypes

import pytest

import probayes_amd as pb
from probayes_amd import _lib


def test_library_exports_trace_quantile():
  lib = _lib.load()
  assert hasattr(lib, 'pbh_trace_quantile')
  assert 'pbh_trace_quantile' in _lib.SIGNATURES


def test_abi_revision_is_2():
  assert _lib.load().pbh_abi_revision() == 2
  assert _lib.ABI_REVISION == 2
  assert _lib.load().pbh_abi_version() == 7


def test_null_engine_is_refused_with_a_message():
  lib = _lib.load()
  q = (ctypes.c_double * 1)(0.5)
  out = (ctypes.c_double * 1)()
  rc = lib.pbh_trace_quantile(None, 0, 1, 1, q, 0, out)
  assert rc == -1   # PBH_ERR_ARG
  assert b'engine' in lib.pbh_last_error()


def test_sampler_without_an_engine_refuses():
  x = pb.RV('x', vtype=float, vset=(-1., 1.))
  process = pb.SP(x)
  batched = process.sampler({'x': 0.}, stop=8, chains=4, rng='philox')
  with pytest.raises(ValueError, match='no engine'):
    batched.trace_quantile(0.5)
  single = process.sampler({'x': 0.}, stop=8)
  with pytest.raises(ValueError, match='batched'):
    single.trace_quantile(0.5)
