"""GPU tier: a plain `bench.py` run (no --full) times the headline and nothing else, and what it dumps is the convolution of
its seeded pool."""
import json
import pathlib
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = pathlib.Path(__file__).resolve().parents[1]


def test_a_plain_run_times_the_headline_alone(tmp_path):
    import torch
    from oracle import c_oracle
    import vndecorrelate_amd.decorrelation as vnd
    from vndecorrelate_amd.taps import function_path_arrays
    pool, n = 16, 480000
    detail, out = tmp_path / 'detail.json', tmp_path / 'out'
    cmd = [sys.executable, str(REPO / 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--pool', str(pool),
           '--min-warmup-ms', '10', '--detail', str(detail), '--dump-outputs', str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(REPO))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith('{"metric"'), r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line['steps'] == 3 and line['value'] > 0 and line['ms_per_step'] > 0 and line['unit'] == 'Msamples/s'
    assert line['roofline']['kernel_ms'] > 0 and line['roofline']['copy_GBs'] is None and line['config']['parity'] is None
    assert 'cpu_baseline' not in line
    full = json.loads(detail.read_text())
    assert full['exact_mode'] is None and full['roofline']['power'] is None and full['config']['single_launch_us'] is None
    assert not {'secondary', 'next_rows', 'audio', 'end_to_end', 'cfg4_strong', 'cpu_baseline'} & set(full)
    # the dump: every stream of a 16-stream pool, against the C oracle on the pool's own seeded input (generator 1234 + rank)
    y = np.load(out / 'convolved.npy')
    assert y.dtype == np.float32 and y.shape == (pool, n, 2)
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1234)
    x = torch.empty((pool, n, 2), dtype=torch.float32, device='cuda').uniform_(-1.0, 1.0, generator=gen).cpu().numpy()
    a = function_path_arrays(vnd.generate_velvet_noise(duration_seconds=0.03, num_impulses=30, num_outs=2, sample_rate_hz=48000, seed=1))
    for b in (0, pool - 1):
        want = c_oracle.convolve(x[b], a.tap_offsets, a.tap_index, a.tap_weight, threads=8)
        err = float(np.max(np.abs(y[b].astype(np.float64) - want)) / np.max(np.abs(want)))
        assert err <= 1e-6, (b, err)
