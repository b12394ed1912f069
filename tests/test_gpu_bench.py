"""bench.py end to end on the GPU at a small batch, in a process of its own: a plain run reports the headline figure and what it
computed, and nothing beyond it; --full adds the per-kernel launches and roofline objects."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(tmp_path, *args):
    detail = tmp_path / 'detail.json'
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--reads', '3000', '--steps', '2', '--warmup', '1',
                        '--detail', str(detail)] + list(args), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.split('\n') if ln]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0]), json.loads(detail.read_text())


def test_plain_run_reports_the_headline_and_nothing_else(tmp_path):
    line, full = _bench(tmp_path, '--dump-outputs', str(tmp_path / 'out'))
    assert line['metric'].startswith('reads/s through CCS+SSW+BSJ') and line['unit'] == 'reads/s' and line['higher_is_better'] is True
    assert line['dtype'] == 'int16' and line['steps'] == 2 and line['warmup'] == 1
    assert line['value'] > 0 and abs(line['value'] - 3000 / (line['ms_per_step'] * 1e-3)) / line['value'] < 1e-3
    assert line['cpu_baseline'] is None and line['roofline'] is None and 'valu_roofline_k3' not in line
    assert 'extra' not in full and 'launches' not in full and full['counters']['total'] == 3000
    names = sorted(os.listdir(str(tmp_path / 'out')))
    assert names == sorted(n + '.npy' for n in ('consensus_rows', 'consensus_segments', 'consensus_sample_reads', 'consensus_sample_lengths',
                                                 'consensus_sample_bases', 'window_n_count', 'ssw_rows', 'splice_signals'))
    rows = np.load(str(tmp_path / 'out' / 'ssw_rows.npy'))
    assert rows.shape == (full['config']['reads_with_consensus'], 6)


def test_full_run_adds_launches_and_rooflines(tmp_path):
    line, full = _bench(tmp_path, '--full', '--no-cpu', '--no-extra')
    assert line['roofline']['bound'] == 'hbm' and line['roofline']['frac'] > 0
    assert line['valu_roofline_k3']['kernel'] == 'poa_consensus_kernel'
    assert any(x['kernel'] == 'poa_consensus_kernel' for x in full['launches'])
