"""The batched velvet-noise optimiser on the device (optimize_velvet_noise_batched, vnd_velvet_pairs_f32_dev): time
host to result, rounds, pairs and distinct tables per round, host time building banks, and the kernel's (frame, pair)
rate in the grid and in the refinement.  Prints one JSON line.

Signals are 44.1 kHz stereo noise of 10 s; the search is ``optimize_velvet_noise``'s default: a 400-point kappa grid,
30 ms / 30 impulses, seed 1.
- ``single``: B = 1.  ``optimize_velvet_noise`` (device grid, host refinement: the only way to do this work without the
  batched form) is timed once; the batched call is the median of --runs wall times, host array to result.  Both kappa
  and the host objective at each are reported.
- ``pools``: B = 64 and 256.  Median of --runs wall times, seconds per signal, rounds, pairs and distinct tables per
  round, and the host seconds spent building banks.  Kernel times are the device events the scorer records around
  every launch (``VelvetSearchStats.launch_ms``); (frame, pair) pairs/s = n * pairs of the launch / kernel time, for
  the grid launches and the refinement launches apart.
- ``scan_moments``: the single-signal scan (``vnd_scan_bank_f32_host``) on the same signal and grid, median of --runs
  wall times of ``scan_moments`` - bank build, table and signal upload, kernels and download - as (frame, pair)
  pairs/s.  Like against like beside it: ``pairs_host_*`` is the new kernel over the same 400 candidates with the same
  scope on the host clock (``velvet_bank_arrays``, ``TapTable.create``, ``velvet_pairs_host``: signal and pairs up,
  kernels, moments down).  ``grid_kernel_pairs_per_s_b1`` is the batched form's grid launch on that one signal by
  device events (its distinct tables only): a kernel rate, not to be set against the two wall-clock rates.

    python tools/velvet_search_rate.py [--runs 5] [--pools 64,256] [--out FILE]
"""
import argparse
import contextlib
import io
import json
import pathlib
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

FS, GRID, DURATION, IMPULSES, SEED, SECONDS = 44100, 400, 0.03, 30, 1, 10
WEIGHTS = dict(angle_limit=float(np.pi / 4), lambda_mean=5.0, lambda_skew=2.0, lambda_correlation=15.0,
               lambda_penalty=1e3)
KW = dict(sample_rate_hz=FS, duration_seconds=DURATION, num_impulses=IMPULSES, seed=SEED, grid_size=GRID, **WEIGHTS)


def quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kwargs)


def pool_of(batch, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (batch, SECONDS * FS, 2)).astype(np.float32)


def rates(stats, n):
    """(grid, refinement) (frame, pair) pairs per second and kernel seconds of one call, from its device events."""
    g = stats.grid_launches
    grid_s, ref_s = sum(stats.launch_ms[:g]) * 1e-3, sum(stats.launch_ms[g:]) * 1e-3
    return (n * sum(stats.launch_pairs[:g]) / grid_s, n * sum(stats.launch_pairs[g:]) / ref_s, grid_s, ref_s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--pools', default='64,256')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    runs = max(args.runs, 5)
    from vndecorrelate_amd import _native
    from vndecorrelate_amd import optimization as opt
    from vndecorrelate_amd.decorrelation import VelvetNoise
    ctx = _native.default_context()
    opt.set_velvet_search_device(True)
    n = SECONDS * FS
    result = dict(tool='velvet_search_rate', device=ctx.info()['name'], runs=runs, grid=GRID, duration_seconds=DURATION,
                  num_impulses=IMPULSES, seed=SEED, seconds=SECONDS, sample_rate_hz=FS)

    def make(kappa):
        return VelvetNoise(sample_rate_hz=FS, duration_seconds=DURATION, num_impulses=IMPULSES,
                           log_distribution_strength=kappa, normalizer=None, filtered_channels=(0,), mode='LR', seed=SEED)

    x = pool_of(1, 10)
    quiet(opt.optimize_velvet_noise_batched, input_signals=x, **KW)            # warm-up
    wall, grid_rate = [], []
    for _ in range(runs):
        t = time.perf_counter()
        kappa_b = quiet(opt.optimize_velvet_noise_batched, input_signals=x, **KW)
        wall.append(time.perf_counter() - t)
        grid_rate.append(rates(opt.last_velvet_search, n)[0])
    stats = opt.last_velvet_search
    t = time.perf_counter()
    kappa_h = quiet(opt.optimize_velvet_noise, input_signal=x[0], **KW)
    host_s = time.perf_counter() - t
    result['single'] = dict(
        batched_ms=round(statistics.median(wall) * 1e3, 2), batched_min_ms=round(min(wall) * 1e3, 2),
        optimize_velvet_noise_s=round(host_s, 2), kappa_batched=float(kappa_b[0]), kappa_host=float(kappa_h),
        host_score_at_kappa_batched=float(opt.symmetry_aware_objective(x[0], make(float(kappa_b[0])), **WEIGHTS)),
        host_score_at_kappa_host=float(opt.symmetry_aware_objective(x[0], make(float(kappa_h)), **WEIGHTS)),
        rounds=stats.rounds, minima=int(stats.minimum_nfev.size), evaluations=int(stats.evaluations.sum()),
        grid_tables=stats.grid_tables, bank_build_s=round(stats.bank_seconds, 4))

    print(f'single: {result["single"]}', file=sys.stderr, flush=True)
    candidates = [make(k) for k in np.linspace(0.0, 1.0, GRID)]
    opt.scan_moments(x[0], candidates, mode=_native.MODE_EXACT)                # warm-up
    scan = []
    for _ in range(runs):
        t = time.perf_counter()
        opt.scan_moments(x[0], candidates, mode=_native.MODE_EXACT)
        scan.append(time.perf_counter() - t)
    kappas = np.linspace(0.0, 1.0, GRID)

    def pairs_grid():
        arrays = opt.velvet_bank_arrays(kappas, sample_rate_hz=FS, duration_seconds=DURATION, num_impulses=IMPULSES, seed=SEED)
        table = _native.TapTable.create(ctx, arrays.tap_offsets, arrays.tap_index, arrays.tap_weight, **arrays.kwargs())
        try:
            return _native.velvet_pairs_host(ctx, table, x, np.zeros(GRID, np.int64), np.arange(GRID))
        finally:
            table.close()
    pairs_grid()                                                                # warm-up
    host = []
    for _ in range(runs):
        t = time.perf_counter()
        pairs_grid()
        host.append(time.perf_counter() - t)
    result['scan_moments'] = dict(wall_ms=round(statistics.median(scan) * 1e3, 2),
                                  pairs_per_s=float(f'{n * GRID / statistics.median(scan):.4g}'),
                                  pairs_host_wall_ms=round(statistics.median(host) * 1e3, 2),
                                  pairs_host_pairs_per_s=float(f'{n * GRID / statistics.median(host):.4g}'),
                                  grid_kernel_pairs_per_s_b1=float(f'{statistics.median(grid_rate):.4g}'))
    print(f'scan: {result["scan_moments"]}', file=sys.stderr, flush=True)

    result['pools'] = {}
    for batch in (int(b) for b in args.pools.split(',')):
        x = pool_of(batch, batch)
        quiet(opt.optimize_velvet_noise_batched, input_signals=x, **KW)         # warm-up
        wall, grid_rate, ref_rate = [], [], []
        for _ in range(runs):
            t = time.perf_counter()
            quiet(opt.optimize_velvet_noise_batched, input_signals=x, **KW)
            wall.append(time.perf_counter() - t)
            stats = opt.last_velvet_search
            g, r, grid_kernel_s, ref_kernel_s = rates(stats, n)
            grid_rate.append(g)
            ref_rate.append(r)
        w = statistics.median(wall)
        ppr, tpr = stats.pairs_per_round, stats.tables_per_round
        result['pools'][f'B{batch}'] = dict(
            wall_s=round(w, 3), seconds_per_signal=float(f'{w / batch:.4g}'), rounds=stats.rounds,
            grid_launches=stats.grid_launches, grid_pairs=stats.grid_pairs, grid_tables=stats.grid_tables,
            pairs_per_round_max=max(ppr), pairs_per_round_median=float(statistics.median(ppr)), pairs_per_round_last=ppr[-1],
            tables_per_round_max=max(tpr), tables_per_round_median=float(statistics.median(tpr)),
            evaluations_per_signal=float(stats.evaluations.mean()), minima_per_signal=float(stats.minimum_nfev.size / batch),
            bank_build_s=round(stats.bank_seconds, 4),
            grid_kernel_s=round(grid_kernel_s, 4), refinement_kernel_s=round(ref_kernel_s, 4),
            grid_pairs_per_s=float(f'{statistics.median(grid_rate):.4g}'),
            refinement_pairs_per_s=float(f'{statistics.median(ref_rate):.4g}'))
        print(f'B{batch}: {result["pools"][f"B{batch}"]}', file=sys.stderr, flush=True)
    opt.set_velvet_search_device(None)
    line = json.dumps(result)
    print(line)
    if args.out:
        pathlib.Path(args.out).write_text(line + '\n')


if __name__ == '__main__':
    main()
