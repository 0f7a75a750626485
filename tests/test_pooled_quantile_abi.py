"""pbh_trace_quantile_pooled at the ABI level (CPU): the symbol, the argument
check that needs no device, the revision it leaves alone, and the facade's
refusals that need no engine."""
import ctypes

import pytest

import probayes_amd as pb
from probayes_amd import _lib


def test_library_exports_trace_quantile_pooled():
  lib = _lib.load()
  assert hasattr(lib, 'pbh_trace_quantile_pooled')
  restype, argtypes = _lib.SIGNATURES['pbh_trace_quantile_pooled']
  assert restype is ctypes.c_int and len(argtypes) == 7
  assert list(lib.pbh_trace_quantile_pooled.argtypes) == list(argtypes)
  # added within revision 2: a caller finds it by the symbol, not the number
  assert lib.pbh_abi_revision() == _lib.ABI_REVISION == 2


def test_null_engine_is_refused_with_a_message():
  lib = _lib.load()
  q = (ctypes.c_double * 1)(0.5)
  out = (ctypes.c_double * 1)()
  rc = lib.pbh_trace_quantile_pooled(None, 0, 4, 1, q, out, None)
  assert rc == -1   # PBH_ERR_ARG
  assert b'engine' in lib.pbh_last_error()


def test_sampler_without_an_engine_refuses():
  x = pb.RV('x', vtype=float, vset=(-1., 1.))
  process = pb.SP(x)
  batched = process.sampler({'x': 0.}, stop=8, chains=4, rng='philox')
  with pytest.raises(ValueError, match='no engine'):
    batched.trace_quantile_pooled([.5])
  single = process.sampler({'x': 0.}, stop=8)
  with pytest.raises(ValueError, match='batched'):
    single.trace_quantile_pooled([.5])
