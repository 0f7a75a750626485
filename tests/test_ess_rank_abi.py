"""pbh_trace_ess_rank at the ABI level (CPU): the symbol, the signature, the
argument checks that need no device, the revision it leaves alone, and the
facade's refusals that need no engine."""
import ctypes
import os
import re

import pytest

import probayes_amd as pb
from probayes_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_trace_ess_rank():
  lib = _lib.load()
  assert hasattr(lib, 'pbh_trace_ess_rank')
  # added within revision 2: a caller finds it by the symbol, not the number
  assert lib.pbh_abi_revision() == _lib.ABI_REVISION == 2


def test_signature_is_the_headers():
  res, args = _lib.SIGNATURES['pbh_trace_ess_rank']
  dp = ctypes.POINTER(ctypes.c_double)
  assert res is ctypes.c_int
  assert args == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, dp, dp, dp, dp, dp]
  with open(os.path.join(ROOT, 'include', 'pbhip.h')) as f:
    text = f.read()
  m = re.search(r'int pbh_trace_ess_rank\(([^)]*)\);', text)
  assert m is not None
  params = [' '.join(p.split()) for p in m.group(1).split(',')]
  assert params == ['pbh_engine *eng', 'int64_t first', 'int64_t count', 'double *bulk',
                    'double *tail', 'double *tail_parts', 'double *basic', 'double *mean_acov']
  assert '#define PBH_ABI_REVISION 2' in text
  assert '#define PBH_ESS_RANK_MAX_HALF 2048' in text


def test_null_engine_is_refused_with_a_message():
  lib = _lib.load()
  out = (ctypes.c_double * 1)()
  rc = lib.pbh_trace_ess_rank(None, 0, 4, out, None, None, None, None)
  assert rc == -1   # PBH_ERR_ARG
  assert b'engine' in lib.pbh_last_error()


def test_no_output_is_refused_with_a_message():
  lib = _lib.load()
  rc = lib.pbh_trace_ess_rank(None, 0, 4, None, None, None, None, None)
  assert rc == -1   # PBH_ERR_ARG
  msg = lib.pbh_last_error()
  assert b'no output' in msg and b'NULL' in msg


def test_sampler_without_an_engine_refuses():
  x = pb.RV('x', vtype=float, vset=(-1., 1.))
  process = pb.SP(x)
  batched = process.sampler({'x': 0.}, stop=8, chains=4, rng='philox')
  with pytest.raises(ValueError, match='no engine'):
    batched.trace_ess_rank()
  single = process.sampler({'x': 0.}, stop=8)
  with pytest.raises(ValueError, match='batched'):
    single.trace_ess_rank()
