"""The batched Haas-delay optimiser on the device (optimize_haas_delay_batched, vnd_haas_pairs_f64_dev): time host to
result, rounds and pairs per round, and the kernel's (frame, pair) rate in the grid and in the refinement.  Prints
one JSON line.

Signals are 44.1 kHz stereo noise of 10 s, the grid ``optimize_haas_delay``'s default (400 delays up to 30 ms, LR,
delayed channel 0).
- ``single``: B = 1.  ``optimize_haas_delay`` (device grid, host refinement) is timed once; the batched call is the
  median of --runs wall times, host array to result.  Both taus are reported, and whether they are equal.
- ``pools``: B = 64 and 256.  Median of --runs wall times, seconds per signal, rounds and pairs per round.  Kernel
  times are hipEvents around every launch on its stream; (frame, pair) pairs/s = sum of (n + d) over the launch's
  pairs / kernel time, for the grid launches and the refinement launches apart (the single-signal scan kernel
  reached 1.8e11 on the 400-delay grid).

    python tools/haas_search_rate.py [--runs 5] [--pools 64,256] [--out FILE]
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

FS, GRID, MAX_DELAY, SECONDS = 44100, 400, 0.03, 10
WEIGHTS = dict(angle_limit=float(np.pi / 4), lambda_mean=5.0, lambda_skew=2.0, lambda_correlation=15.0,
               lambda_penalty=1e3)
KW = dict(sample_rate_hz=FS, max_delay_seconds=MAX_DELAY, grid_size=GRID, **WEIGHTS)


def quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kwargs)


def pool_of(batch, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (batch, SECONDS * FS, 2)).astype(np.float32)


class KernelClock:
    """hipEvents around every vnd_haas_pairs_f64_dev launch, and each launch's (frame, pair) count."""

    def __init__(self, torch, opt, native):
        self.torch, self.launches = torch, []
        real_launch, real_dev = opt._DevicePairScorer._launch, native.haas_pairs_device
        clock = self

        def launch(scorer, signals, delays):
            clock.frames = int(np.sum(scorer.n + delays.astype(np.int64)))
            return real_launch(scorer, signals, delays)

        def dev(*args, **kwargs):
            s = torch.cuda.current_stream()                  # the stream the scorer launches on
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            real_dev(*args, **kwargs)
            b.record(s)
            clock.launches.append((a, b, clock.frames))
        opt._DevicePairScorer._launch = launch
        native.haas_pairs_device = dev

    def take(self):
        self.torch.cuda.synchronize()
        out = [(a.elapsed_time(b) * 1e-3, f) for a, b, f in self.launches]
        self.launches = []
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--pools', default='64,256')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    runs = max(args.runs, 5)
    import torch
    from vndecorrelate_amd import _native
    from vndecorrelate_amd import optimization as opt
    ctx = _native.default_context()
    opt.set_haas_scan_device(True)
    result = dict(tool='haas_search_rate', device=ctx.info()['name'], runs=runs, grid=GRID,
                  max_delay_seconds=MAX_DELAY, seconds=SECONDS, sample_rate_hz=FS,
                  single_signal_scan_pairs_per_s=1.8e11)

    x = pool_of(1, 10)
    quiet(opt.optimize_haas_delay_batched, input_signals=x, **KW)              # warm-up
    wall = []
    for _ in range(runs):
        t = time.perf_counter()
        tau_b = quiet(opt.optimize_haas_delay_batched, input_signals=x, **KW)
        wall.append(time.perf_counter() - t)
    stats = opt.last_haas_search
    t = time.perf_counter()
    tau_h = quiet(opt.optimize_haas_delay, input_signal=x[0], **KW)
    host_s = time.perf_counter() - t
    result['single'] = dict(batched_ms=round(statistics.median(wall) * 1e3, 2), batched_min_ms=round(min(wall) * 1e3, 2),
                            host_refinement_s=round(host_s, 2), tau_batched=float(tau_b[0]), tau_host=float(tau_h),
                            equal=bool(float(tau_b[0]) == float(tau_h)), rounds=stats.rounds,
                            minima=int(stats.minimum_nfev.size), evaluations=int(stats.evaluations.sum()),
                            host_evaluations=opt.last_haas_memo.calls)

    clock = KernelClock(torch, opt, _native)
    result['pools'] = {}
    for batch in (int(b) for b in args.pools.split(',')):
        x = pool_of(batch, batch)
        quiet(opt.optimize_haas_delay_batched, input_signals=x, **KW)           # warm-up
        clock.take()
        wall, grid_rate, ref_rate = [], [], []
        for _ in range(runs):
            t = time.perf_counter()
            quiet(opt.optimize_haas_delay_batched, input_signals=x, **KW)
            wall.append(time.perf_counter() - t)
            stats = opt.last_haas_search
            timed = clock.take()
            launches = len(timed) - stats.rounds                 # the grid's launches come first, then one per round
            g, r = timed[:launches], timed[launches:]
            grid_rate.append(sum(f for _, f in g) / sum(s for s, _ in g))
            ref_rate.append(sum(f for _, f in r) / sum(s for s, _ in r))
            ref_kernel_s = sum(s for s, _ in r)
            grid_kernel_s = sum(s for s, _ in g)
        w = statistics.median(wall)
        ppr = stats.pairs_per_round
        result['pools'][f'B{batch}'] = dict(
            wall_s=round(w, 3), seconds_per_signal=float(f'{w / batch:.4g}'), rounds=stats.rounds,
            grid_launches=launches, grid_pairs=stats.grid_pairs, pairs_per_round_max=max(ppr),
            pairs_per_round_median=float(statistics.median(ppr)), pairs_per_round_last=ppr[-1],
            evaluations_per_signal=float(stats.evaluations.mean()),
            grid_kernel_s=round(grid_kernel_s, 4), refinement_kernel_s=round(ref_kernel_s, 4),
            grid_pairs_per_s=float(f'{statistics.median(grid_rate):.4g}'),
            refinement_pairs_per_s=float(f'{statistics.median(ref_rate):.4g}'))
    opt.set_haas_scan_device(None)
    line = json.dumps(result)
    print(line)
    if args.out:
        pathlib.Path(args.out).write_text(line + '\n')


if __name__ == '__main__':
    main()
