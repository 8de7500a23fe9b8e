"""bench.py's command line: a plain run times the headline only and prints its line;
`--dump-outputs DIR` writes what the last timed step computed.

The dumped points are the GPU solution of the configs[1] problem, so they are held to the
bounds of tests/test_gpu_core.py against the reference's own solution of that problem
(tests/golden/sba_cfg2.npz `pts_out`: scipy TRF, stops at xtol = 1e-8): 1e-5 m max,
1e-6 m RMS."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, golden

pytestmark = pytest.mark.gpu

STEPS, WARMUP = 3, 1


@pytest.fixture(scope='module')
def plain_run(tmp_path_factory):
    """One plain run of the benchmark (its own process, as it is used) with a dump."""
    out = tmp_path_factory.mktemp('dump')
    p = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', str(STEPS),
                        '--warmup', str(WARMUP), '--dump-outputs', str(out)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0]), out


def test_plain_line_is_the_headline_only(plain_run):
    line, _ = plain_run
    assert line['unit'] == 'frames/s' and line['higher_is_better'] is True and line['dtype'] == 'f64'
    assert 'configs[1]' in line['metric']
    assert line['steps'] == STEPS and line['warmup'] == WARMUP
    assert line['ms_per_step'] > 0
    # value = frames solved per second: one step solves the problem's frames (100) on one GPU
    n_frames = int(golden('sba_cfg2')['n_frames'])
    np.testing.assert_allclose(line['value'], n_frames * 1e3 / line['ms_per_step'], rtol=1e-9)
    # what --full adds is absent from a plain run
    for k in ('roofline', 'convergence', 'stream_launch', 'cpu_baseline', 'fte', 'ekf', 'sba_ekf_pipeline',
              'fte_window', 'sba_at_scale'):
        assert k not in line, k


def test_dump_is_the_solution_of_the_timed_step(plain_run):
    _, out = plain_run
    assert sorted(os.listdir(out)) == ['points_3d.npy']
    pts = np.load(out / 'points_3d.npy')
    g = golden('sba_cfg2')
    assert pts.dtype == np.float64 and pts.shape == g['pts_out'].shape
    d = np.linalg.norm(pts - g['pts_out'], axis=1)
    print(f'dump vs reference solution: rms {np.sqrt(np.mean(d ** 2)):.3e} m, max {d.max():.3e} m')
    assert np.sqrt(np.mean(d ** 2)) < 1e-6 and d.max() < 1e-5
