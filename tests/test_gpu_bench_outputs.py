"""bench.py's plain run and --dump-outputs on the GPU: the line says how many steps were timed and what one took,
runs none of the --full legs, and DIR/<name>.npy hold what the last timed step computed (fitness of the whole
population, the weighted noise sum, theta after Adam, the update ratio) in float32 / float64."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 2865808          # parameters of the default fc_caption model (bench.iteration_algorithmic_bytes)


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_outputs(tmp_path):
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    out = tmp_path / 'dump'
    p = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
                        '--population', '64', '--noise-len', str(1 << 25), '--dump-outputs', str(out)], env=env,
                       cwd=REPO, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, p.stdout
    rec = json.loads(lines[0])
    assert rec['steps'] == 3 and rec['warmup'] == 1 and rec['n_gpus'] == 1 and rec['dtype'] == 'fp32'
    assert rec['ms_per_step'] > 0 and rec['unit'] == 'members/s' and rec['higher_is_better'] is True
    # value = P / time per step
    assert abs(rec['value'] - 64 / (rec['ms_per_step'] / 1e3)) <= 1e-3 * rec['value']
    # a plain run: no CPU leg, no PMC profile lookup
    assert rec['full'] is False and rec['cpu_baseline'] is None
    assert rec['roofline']['traffic_looked_up'] is False and rec['roofline']['traffic'] is None
    assert sorted(os.listdir(out)) == ['fitness.npy', 'noise_sum.npy', 'theta.npy', 'update_ratio.npy']
    got = {n[:-4]: np.load(out / n) for n in os.listdir(out)}
    assert got['fitness'].shape == (64, 2) and got['fitness'].dtype == np.float64
    assert got['noise_sum'].shape == (D,) and got['noise_sum'].dtype == np.float32
    assert got['theta'].shape == (D,) and got['theta'].dtype == np.float64
    assert got['update_ratio'].shape == (1,) and got['update_ratio'].dtype == np.float64
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    for a in got.values():
        assert np.isfinite(a).all()
    assert (got['fitness'] >= 0).all() and got['fitness'].max() > 0 and np.abs(got['noise_sum']).max() > 0
    assert got['update_ratio'][0] == rec['update_ratio']
