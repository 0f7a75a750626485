"""pbh_trace_rhat at the ABI level (CPU): the symbol, the argument check that
needs no device, the revision it leaves alone, and the facade's refusals that
need no engine."""
import ctypes

import pytest

import probayes_amd as pb
from probayes_amd import _lib


def test_library_exports_trace_rhat():
  lib = _lib.load()
  assert hasattr(lib, 'pbh_trace_rhat')
  assert 'pbh_trace_rhat' in _lib.SIGNATURES
  # added within revision 2: a caller finds it by the symbol, not the number
  assert lib.pbh_abi_revision() == _lib.ABI_REVISION == 2


def test_null_engine_is_refused_with_a_message():
  lib = _lib.load()
  out = (ctypes.c_double * 1)()
  rc = lib.pbh_trace_rhat(None, 0, 4, 1, out, None, None)
  assert rc == -1   # PBH_ERR_ARG
  assert b'engine' in lib.pbh_last_error()


def test_sampler_without_an_engine_refuses():
  x = pb.RV('x', vtype=float, vset=(-1., 1.))
  process = pb.SP(x)
  batched = process.sampler({'x': 0.}, stop=8, chains=4, rng='philox')
  with pytest.raises(ValueError, match='no engine'):
    batched.trace_rhat()
  single = process.sampler({'x': 0.}, stop=8)
  with pytest.raises(ValueError, match='batched'):
    single.trace_rhat()
