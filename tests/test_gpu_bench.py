"""-m gpu: a plain bench.py run measures the headline only and --dump-outputs writes what its
last timed step computed; two runs with the same arguments see the same inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain(dump):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--config', 'cfg2',
           '--steps', '2', '--warmup', '1', '--dump-outputs', dump]
    out = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=280, stdin=subprocess.DEVNULL)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = [ln for ln in out.stdout.decode().splitlines() if ln.startswith('{')]
    assert len(lines) == 1, out.stdout.decode()[-2000:]
    arrays = {f[:-4]: np.load(os.path.join(dump, f)) for f in os.listdir(dump)}
    return json.loads(lines[0]), arrays


@pytest.mark.timeout(600)
def test_plain_run_dumps_the_last_step_and_is_reproducible(tmp_path):
    line, got = _plain(str(tmp_path / 'a'))
    assert line['steps'] == 2 and line['warmup'] == 1 and line['ms_per_step'] > 0
    assert line['value'] > 0 and line['fallbacks'] == 0
    assert line['config']['workload'].startswith('cfg2')
    for k in ('cfg2', 'cfg2_n128', 'exact_fp32', 'cpu_baseline', 'predict_ms', 'beam_s',
              'dataset_build_audio_s_per_s'):
        assert k not in line, k                   # companion measurements: --full only
    N = line['config']['global_batch']
    assert got['ctc_loss'].shape == (N,) and np.all(np.isfinite(got['ctc_loss']))
    assert got['greedy_decode'].shape[0] == N and got['greedy_decode_len'].shape == (N,)
    assert got['params_sample'].shape == got['grads_sample'].shape == got['sample_index'].shape
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.abs(got['grads_sample']).max() > 0
    _, again = _plain(str(tmp_path / 'b'))
    assert np.array_equal(got['sample_index'], again['sample_index'])
    np.testing.assert_allclose(again['ctc_loss'], got['ctc_loss'], rtol=1e-4)
    np.testing.assert_allclose(again['params_sample'], got['params_sample'], rtol=0, atol=1e-5)
    gmax = np.abs(got['grads_sample']).max()
    np.testing.assert_allclose(again['grads_sample'], got['grads_sample'], rtol=0, atol=1e-3 * gmax)
