"""``bench.py`` on its default path (c3, resident) on one GPU: a plain run prints the headline line and nothing it would need
runs of its own for; ``--full`` adds the per-kernel breakdown and roofline and checks the batch against the oracle."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step')


def _bench(extra):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--batch', '4', '--steps', '3', '--warmup', '1'] + extra,
                         cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert all(k in rec for k in HEADLINE)
    assert rec['unit'] == 'Mpixels/s' and rec['steps'] == 3 and rec['warmup'] == 1 and rec['n_gpus'] == 1
    assert abs(rec['value'] - 4 * 2048 * 2048 / (rec['ms_per_step'] / 1e3) / 1e6) < 1e-6 * rec['value']     # source pixels
    return rec


def test_plain_run_is_the_headline_alone():
    rec = _bench([])
    for leg in ('roofline', 'noise_stream', 'cpu_baseline', 'state_construction', 'other_configs'):
        assert leg not in rec
    assert rec['config']['verified'] is None and rec['config']['verified_against_oracle'] == 0


def test_full_run_adds_the_breakdown_and_the_checks():
    rec = _bench(['--full', '--verify', '2', '--extra-legs', '0', '--cpu-sample', '0'])
    assert rec['config']['verified'] is True and rec['config']['verified_against_oracle'] == 2
    assert 'k_chain_fused' in rec['roofline']['kernels_ms_per_step'] and rec['noise_stream']['kernels_ms_per_step']
    assert rec['state_construction']['lattices_equal_host_operator'] == '4 of 4 checked'
    assert rec['cpu_baseline'] is None
