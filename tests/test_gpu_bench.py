"""-m gpu: bench.py end to end (1 GPU), on a scaled-down matrix (the sub-blocks are full-size only).  With --full (incl. the
CPU baseline and the adversarial catalogues) the LAST stdout line must be the compact JSON record — parseable, under 3 KB,
with `roofline` and `cpu_baseline`, the lists of the sample identical to the CPU path's; a plain run prints the headline
fields only, and --dump-outputs writes the lists of the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_default_bench_prints_one_compact_parseable_line(tmp_path):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--scale', '0.05',
                        '--full', '--dump-outputs', str(tmp_path / 'out')],
                       capture_output=True, text=True, env=env, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    last = r.stdout.strip().splitlines()[-1]
    assert len(last.encode()) <= 3000
    d = json.loads(last)
    for key in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
                'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
        assert key in d, key
    assert d['n_gpus'] == 1 and d['steps'] == 3 and d['warmup'] == 1 and d['value'] > 0 and d['higher_is_better'] is True
    assert d['config']['workload'] and d['config']['scale'] == 0.05 and 'model' not in d['config']
    assert {'bound', 'achieved', 'peak', 'unit', 'frac', 'traffic'} <= set(d['roofline']) and d['roofline']['bound'] in ('hbm', 'mfma')
    assert abs(d['roofline']['frac'] - d['roofline']['achieved'] / d['roofline']['peak']) < 1e-3
    assert {'value', 'unit', 'cores', 'kind', 'sample'} <= set(d['cpu_baseline']) and d['cpu_baseline']['kind'] in ('port', 'reference')
    assert d['cpu_baseline']['identical_rows'] == 1.0                      # the GPU lists against the CPU path's on the sample
    assert 'adversarial_users_per_s' not in d['config']     # those three catalogues only ride along at full size (scale 1.0)
    # a pass over 7 K users is shorter on the device than on the host: the loop must have calibrated the replayed form
    # (scoring.RecordedPass) next to the launched ones, and whichever ran, the lists above came out of it
    detail = json.load(open(os.path.join(ROOT, 'bench_detail.json')))
    cal = detail['warmup_calibration_ms_per_step']
    assert cal['python_launch'] > 0 and cal.get('recorded_replay') is not None and cal['recorded_replay'] > 0, cal
    assert d['config']['launch'] in ('python', 'hipGraph', 'python, passes on 2 streams') or d['config']['launch'].startswith('recorded calls'), d['config']['launch']
    # the lists the CPU baseline was compared with are the dumped ones (external item ids, every user)
    recs = np.load(str(tmp_path / 'out' / 'recommendations.npy'))
    assert recs.dtype == np.float64 and recs.shape == (d['config']['n_users'], d['config']['topk'])


def test_plain_bench_measures_the_headline_only_and_dumps_the_last_step(tmp_path):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '4', '--warmup', '1', '--scale', '0.05',
                        '--dump-outputs', str(tmp_path / 'out')],
                       capture_output=True, text=True, env=env, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    for key in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step', 'build_s', 'config'):
        assert key in d, key
    assert d['steps'] == 4 and d['value'] > 0 and d['ms_per_step'] > 0 and d['unit'] == 'users/s' and d['dtype'] == 'bf16x3'
    assert abs(d['value'] * d['ms_per_step'] * 1e-3 - d['config']['n_users']) < 1e-3 * d['config']['n_users']
    for key in ('roofline', 'cpu_baseline', 'cold', 'roofline_build', 'roofline_foldin'):      # --full only
        assert key not in d, key
    assert d['ms_per_step_long_region'] is None and 'adversarial_users_per_s' not in d['config']
    recs = np.load(str(tmp_path / 'out' / 'recommendations.npy'))
    n_users, topk, n_items = d['config']['n_users'], d['config']['topk'], d['config']['n_items']
    assert recs.dtype == np.float64 and recs.shape == (n_users, topk)
    assert (recs >= 0).all() and (recs < n_items).all() and (recs == np.round(recs)).all()
    assert all(len(set(row)) == topk for row in recs.astype(np.int64))
