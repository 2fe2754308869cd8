"""GPU: a plain `bench.py` run (no `--full`) is the headline alone -- the detect leg, its outputs and the line, none of the
other legs -- in a process of its own, as the benchmark is run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_LEGS = ('roofline', 'split_bf16', 'frontend', 'dense_finest_map', 'bulk_inference', 'train_step', 'cpu_baseline')


def test_plain_run_is_the_headline_only(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '2', '--warmup', '1', '--spin-up', '0',
                        '--dump-outputs', str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['full'] is False and not [k for k in FULL_LEGS if k in d]
    assert d['metric'] == 'clips/sec (3 s @ 22.05 kHz) detect fwd' and d['unit'] == 'clips/s' and d['higher_is_better'] is True
    assert d['dtype'] == 'f32' and d['steps'] == 2 and d['warmup'] == 1
    assert d['value'] > 0 and abs(d['value'] - 2 * 64 * 1e3 / (d['ms_per_step'] * 2)) < 1e-6 * d['value']
    assert d['single_lane_graph_replay'] is not None and d['config']['launch_note'] is None
    rows = np.load(tmp_path / 'detections.npy')
    assert rows.dtype == np.float64 and rows.shape[1] == 7 and len(rows) > 0
    assert set(np.unique(rows[:, 0]).astype(int)) <= set(range(64))
