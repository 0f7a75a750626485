"""bench.py as a program on the GPU: a plain run (no --full) prints the
headline line alone, really times --steps steps, and --dump-outputs writes
the last timed step's records, which must be bit-for-bit those of the same
seeded chains run through an engine in this process (ordinary launches)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

N, STEPS, WARMUP = 8192, 8, 4   # 32 eight-wave workgroups: the headline's form


def test_plain_run_line_and_dump_equal_the_engine(tmp_path, monkeypatch):
  import bench
  from probayes_amd import Engine
  dump = tmp_path / 'dump'
  p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1',
                      '--steps', str(STEPS), '--warmup', str(WARMUP),
                      '--chains', str(N), '--dump-outputs', str(dump)],
                     stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                     timeout=120, cwd=str(tmp_path))
  assert p.returncode == 0, p.stderr
  lines = [l for l in p.stdout.splitlines() if l.strip()]
  assert len(lines) == 1, p.stdout
  line = json.loads(lines[0])
  assert line['metric'] == bench.METRIC and line['unit'] == 'chain-steps/s'
  assert line['higher_is_better'] is True and line['dtype'] == 'f64'
  assert line['steps'] == STEPS and line['n_gpus'] == 1
  assert line['ms_per_step'] > 0
  assert abs(line['value'] * line['ms_per_step'] * STEPS / 1e3 / (N * STEPS) - 1) < 1e-9
  for k in ('cpu_baseline', 'launched', 'launched_chain_steps_per_s',
            'replay_chain_steps_per_s', 'rccl_allgather_ms'):
    assert k not in line, k
  assert line['dumped'] == {'x': [N, bench.D], 'logp': [N], 'accept': [N]}
  got = {f[:-4]: np.load(str(dump / f)) for f in sorted(os.listdir(str(dump)))}
  assert sorted(got) == ['accept', 'logp', 'x']
  assert got['x'].dtype == np.float64 and got['logp'].dtype == np.float64
  assert got['accept'].dtype == np.float32

  # the same chains by ordinary launches: bench.run_rank's sequence
  monkeypatch.setenv('PBH_SERVER', '0')
  eng = Engine(bench.cfg2_spec())
  eng.init_chains(np.zeros((N, bench.D)))
  eng.set_rng('philox', seed=bench.SEED)
  eng.set_collect(moments=False)
  eng.alloc_trace(WARMUP + STEPS, 1)
  for _ in range(WARMUP):
    eng.run(1)
  eng.run(STEPS, steps_per_launch=250, sync=True)
  assert eng.trace_len() == WARMUP + STEPS
  rec = eng.trace(first=WARMUP + STEPS - 1, count=1)
  eng.close()
  assert np.array_equal(got['x'], rec['v_x'][:, 0, :])
  assert np.array_equal(got['logp'], rec['v_p'][:, 0])
  assert np.array_equal(got['accept'], rec['u'][:, 0])
  assert 0.05 < got['accept'].mean() < 0.95
