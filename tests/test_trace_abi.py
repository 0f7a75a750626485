"""The trace reductions at the ABI level (CPU), one row of SYMBOLS per entry
point (pbh_trace_rhat's three tests stay in test_rhat_abi.py): the symbol, its
signature in _lib.py and in include/pbhip.h, the argument checks that need no
device, the revision it leaves alone, and the facade's refusals that need no
engine."""
import ctypes
import os
import re

import pytest

import probayes_amd as pb
from probayes_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP, I64, I32 = ctypes.POINTER(ctypes.c_double), ctypes.c_int64, ctypes.c_int32
WINDOW = [ctypes.c_void_p, I64, I64]
WINDOW_PARAMS = ['pbh_engine *eng', 'int64_t first', 'int64_t count']

# per symbol: the ctypes arguments and the header's parameters behind (eng,
# first, count); the #defines the header must carry; the arguments behind a
# null engine of a call that asks for an output, and of one that asks for none
# where the symbol refuses that (None: it has no such check); the Sampler
# method and its arguments
SYMBOLS = {
    'pbh_trace_quantile': dict(
        args=[I32, DP, I32, DP],
        params=['int32_t nq', 'const double *q', 'int32_t weighted', 'double *out'],
        defines=['PBH_ABI_REVISION 2', 'PBH_QUANTILE_MAX_RECORDS 2048', 'PBH_QUANTILE_MAX_Q 64'],
        null_engine=lambda q, out: (0, 1, 1, q, 0, out), no_output=None,
        method=('trace_quantile', (0.5,))),
    'pbh_trace_quantile_pooled': dict(
        args=[I32, DP, DP, DP],
        params=['int32_t nq', 'const double *q', 'double *out', 'double *order_stats'],
        defines=['PBH_ABI_REVISION 2', 'PBH_QUANTILE_MAX_Q 64'],
        null_engine=lambda q, out: (0, 4, 1, q, out, None), no_output=None,
        method=('trace_quantile_pooled', ([.5],))),
    'pbh_trace_rhat_rank': dict(
        args=[DP, DP, DP, DP],
        params=['double *bulk', 'double *folded', 'double *ranks', 'double *folded_ranks'],
        defines=['PBH_ABI_REVISION 2'],
        null_engine=lambda q, out: (0, 4, out, None, None, None),
        no_output=(0, 4, None, None, None, None),
        method=('trace_rhat_rank', ())),
    'pbh_trace_ess_rank': dict(
        args=[DP, DP, DP, DP, DP],
        params=['double *bulk', 'double *tail', 'double *tail_parts', 'double *basic',
                'double *mean_acov'],
        defines=['PBH_ABI_REVISION 2', 'PBH_ESS_RANK_MAX_HALF 2048'],
        null_engine=lambda q, out: (0, 4, out, None, None, None, None),
        no_output=(0, 4, None, None, None, None, None),
        method=('trace_ess_rank', ())),
}
symbols = pytest.mark.parametrize('name', list(SYMBOLS))


@symbols
def test_library_exports(name):
  lib = _lib.load()
  assert hasattr(lib, name)
  assert name in _lib.SIGNATURES
  restype, argtypes = _lib.SIGNATURES[name]
  assert restype is ctypes.c_int and len(argtypes) == 3 + len(SYMBOLS[name]['args'])
  assert list(getattr(lib, name).argtypes) == list(argtypes)
  # added within revision 2: a caller finds it by the symbol, not the number
  assert lib.pbh_abi_revision() == _lib.ABI_REVISION == 2


def test_abi_revision_is_2():
  assert _lib.load().pbh_abi_revision() == 2
  assert _lib.ABI_REVISION == 2
  assert _lib.load().pbh_abi_version() == 7


@symbols
def test_signature_is_the_headers(name):
  row = SYMBOLS[name]
  res, args = _lib.SIGNATURES[name]
  assert res is ctypes.c_int
  assert args == WINDOW + row['args']
  with open(os.path.join(ROOT, 'include', 'pbhip.h')) as f:
    text = f.read()
  m = re.search(r'int {}\(([^)]*)\);'.format(name), text)
  assert m is not None
  params = [' '.join(p.split()) for p in m.group(1).split(',')]
  assert params == WINDOW_PARAMS + row['params']
  for define in row['defines']:
    assert '#define ' + define in text


@symbols
def test_null_engine_is_refused_with_a_message(name):
  lib = _lib.load()
  q = (ctypes.c_double * 1)(0.5)
  out = (ctypes.c_double * 1)()
  rc = getattr(lib, name)(None, *SYMBOLS[name]['null_engine'](q, out))
  assert rc == -1   # PBH_ERR_ARG
  assert b'engine' in lib.pbh_last_error()


@pytest.mark.parametrize('name', [n for n, row in SYMBOLS.items() if row['no_output']])
def test_no_output_is_refused_with_a_message(name):
  lib = _lib.load()
  rc = getattr(lib, name)(None, *SYMBOLS[name]['no_output'])
  assert rc == -1   # PBH_ERR_ARG
  msg = lib.pbh_last_error()
  assert b'no output' in msg and b'NULL' in msg


@symbols
def test_sampler_without_an_engine_refuses(name):
  method, args = SYMBOLS[name]['method']
  x = pb.RV('x', vtype=float, vset=(-1., 1.))
  process = pb.SP(x)
  batched = process.sampler({'x': 0.}, stop=8, chains=4, rng='philox')
  with pytest.raises(ValueError, match='no engine'):
    getattr(batched, method)(*args)
  single = process.sampler({'x': 0.}, stop=8)
  with pytest.raises(ValueError, match='batched'):
    getattr(single, method)(*args)
