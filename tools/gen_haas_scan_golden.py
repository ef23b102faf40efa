#!/usr/bin/env python3
"""Write tests/golden/haas_scan.npz and haas_scan_manifest.json from the reference's own code.

Usage:  python tools/gen_haas_scan_golden.py <reference checkout>

Runs the reference's ``optimization.py`` ``grid_scan`` over ``HaasEffect`` candidates (LR and MS, both delayed
channels, with and without width, mono and stereo input, a signal with silent stretches and signed zeros, a grid
fine enough to round many delays to the same integer), the local minima of each scan, and the reference's
``optimize_haas_delay`` on three signals.  Only outputs are stored; the manifest keeps each case's parameters, its
input recipe (``fixture_input`` rebuilds the input from it; the tests use that function) and the sha256 of every
stored array.  The reference is loaded as ``tools/gen_correlogram_golden.py`` loads it.
"""
from __future__ import annotations

import contextlib
import io
import json
import pathlib
import sys

import numpy as np

REPO = pathlib.Path(__file__).resolve().parents[1]
OUT = REPO / 'tests' / 'golden'
sys.path.insert(0, str(REPO / 'tools'))
from gen_correlogram_golden import load_reference, sha  # noqa: E402

WEIGHTS = dict(angle_limit=float(np.pi / 4), lambda_mean=5.0, lambda_skew=2.0, lambda_correlation=15.0,
               lambda_penalty=1e3)


def fixture_input(recipe: dict) -> np.ndarray:
    """The float32 input signal of a case from its manifest recipe."""
    n = recipe['n']
    r = np.random.default_rng(recipe['seed'])
    if recipe['kind'] == 'mono':
        return r.uniform(-1, 1, n).astype(np.float32)
    x = r.uniform(-1, 1, (n, 2)).astype(np.float32)
    if recipe['kind'] == 'stereo':
        return x
    if recipe['kind'] == 'stereo_zeros':                  # silent stretches and signed zeros in both channels
        for a, b in recipe['silent']:
            x[a:b] = 0.0
        for a, b in recipe['negative_zero']:
            x[a:b] = -0.0
        for a, b in recipe['mixed_zero']:                 # L = -0, R = +0 and the other way round
            x[a:b, 0], x[a:b, 1] = -0.0, 0.0
            x[b:2 * b - a, 0], x[b:2 * b - a, 1] = 0.0, -0.0
        return x
    raise ValueError(f'unknown input kind {recipe["kind"]!r}')


def scan_cases():
    """(name, input recipe, sample rate, max delay seconds, grid size, HaasEffect configuration)."""
    stereo = dict(kind='stereo', seed=1, n=3000)
    mono = dict(kind='mono', seed=2, n=2500)
    zeros = dict(kind='stereo_zeros', seed=3, n=3000, silent=[[0, 200], [1200, 1700], [2900, 3000]],
                 negative_zero=[[300, 340]], mixed_zero=[[400, 420]])
    yield 'lr_c0_stereo', stereo, 16000, 0.01, 64, dict(delayed_channel=0, mode='LR', width=None)
    yield 'lr_c1_stereo', stereo, 16000, 0.01, 64, dict(delayed_channel=1, mode='LR', width=None)
    yield 'lr_c0_mono', mono, 16000, 0.01, 64, dict(delayed_channel=0, mode='LR', width=None)
    yield 'lr_c1_mono_width', mono, 16000, 0.01, 48, dict(delayed_channel=1, mode='LR', width=0.3)
    yield 'lr_c0_stereo_width', stereo, 16000, 0.01, 48, dict(delayed_channel=0, mode='LR', width=0.7)
    yield 'ms_c0_stereo', stereo, 16000, 0.01, 64, dict(delayed_channel=0, mode='MS', width=None)
    yield 'ms_c1_stereo', stereo, 16000, 0.01, 64, dict(delayed_channel=1, mode='MS', width=None)
    yield 'ms_c0_mono', mono, 16000, 0.01, 48, dict(delayed_channel=0, mode='MS', width=None)
    yield 'ms_c1_mono_width', mono, 16000, 0.01, 48, dict(delayed_channel=1, mode='MS', width=0.6)
    yield 'ms_c1_stereo_width', stereo, 16000, 0.01, 48, dict(delayed_channel=1, mode='MS', width=0.25)
    yield 'lr_c0_zeros', zeros, 16000, 0.015, 64, dict(delayed_channel=0, mode='LR', width=None)
    yield 'ms_c1_zeros_width', zeros, 16000, 0.015, 64, dict(delayed_channel=1, mode='MS', width=0.5)
    yield 'lr_c0_duplicates', stereo, 8000, 0.005, 300, dict(delayed_channel=0, mode='LR', width=None)


def optimize_cases():
    """(name, input recipe, sample rate, max delay seconds, grid size) of optimize_haas_delay."""
    yield 'opt_stereo', dict(kind='stereo', seed=4, n=4000), 16000, 0.01, 40
    yield 'opt_mono', dict(kind='mono', seed=5, n=3000), 16000, 0.008, 32
    yield 'opt_zeros', dict(kind='stereo_zeros', seed=6, n=3000, silent=[[500, 1500]], negative_zero=[[100, 150]],
                            mixed_zero=[[200, 230]]), 8000, 0.02, 64


def main(argv):
    if len(argv) != 2:
        sys.exit(__doc__)
    root = pathlib.Path(argv[1]).resolve()
    _, dec = load_reference(root)
    sys.path.insert(0, str(root / 'src'))                 # optimization.py imports vndecorrelate.* (already loaded)
    import importlib
    opt = importlib.import_module('vndecorrelate.optimization')
    arrays, manifest = {}, {'numpy': np.__version__, 'weights': WEIGHTS, 'scans': {}, 'optimize': {}}
    quiet = contextlib.redirect_stdout(io.StringIO())
    for name, recipe, fs, max_delay, grid, cfg in scan_cases():
        x = fixture_input(recipe)
        taus = np.linspace(0.0, max_delay, grid)
        cands = [dec.HaasEffect(sample_rate_hz=fs, delay_time_seconds=tau, **cfg) for tau in taus]
        with quiet:
            scores = np.asarray(opt.grid_scan(x, cands, **WEIGHTS), np.float64)
        minima = np.asarray(opt.get_local_minima(scores, grid), np.int64)
        delays = [round(tau * fs) for tau in taus]
        arrays[f'{name}__scores'], arrays[f'{name}__minima'] = scores, minima
        manifest['scans'][name] = {'input': recipe, 'sample_rate_hz': fs, 'max_delay_seconds': max_delay,
                                   'grid_size': grid, 'config': cfg, 'distinct_delays': len(set(delays)),
                                   'sha256': {'scores': sha(scores), 'minima': sha(minima)}}
    for name, recipe, fs, max_delay, grid in optimize_cases():
        x = fixture_input(recipe)
        with quiet:
            tau = float(opt.optimize_haas_delay(input_signal=x, sample_rate_hz=fs, max_delay_seconds=max_delay,
                                                grid_size=grid, **WEIGHTS))
        manifest['optimize'][name] = {'input': recipe, 'sample_rate_hz': fs, 'max_delay_seconds': max_delay,
                                      'grid_size': grid, 'tau': tau, 'tau_hex': tau.hex()}
    OUT.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(OUT / 'haas_scan.npz', **arrays)
    (OUT / 'haas_scan_manifest.json').write_text(json.dumps(manifest, indent=1) + '\n')
    print(f'{len(manifest["scans"])} scans, {len(manifest["optimize"])} optimisations -> {OUT / "haas_scan.npz"} '
          f'({(OUT / "haas_scan.npz").stat().st_size} bytes)')


if __name__ == '__main__':
    main(sys.argv)
