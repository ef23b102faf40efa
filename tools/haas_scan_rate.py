"""The Haas-delay scan on the device (vnd_haas_scan_f64_dev): kernel time, (frame, candidate) pairs per second and
host-to-scores time of ``grid_scan`` on three signals, against NumPy's time per candidate.  Prints one JSON line.

Signals: 10 s and 60 s of 44.1 kHz stereo noise and 10 s of mono, each with the 400 delays of ``optimize_haas_delay``'s
default grid up to 30 ms (LR, delayed channel 0).  Kernel times are hipEvents on the launch stream after a warm-up,
the median of --runs (>= 5).  ``host_to_scores_ms`` is ``grid_scan`` from the host array to the scores, median of
--runs.  NumPy (the reference's ``symmetry_aware_objective``, one core) is timed on 3 candidates and EXTRAPOLATED to
the grid.  The scores of 8 spread candidates are checked against NumPy's.

``--memo`` instead runs ``optimize_haas_delay`` on the 10 s stereo signal with the host scan (no device needed) and
reports how many refinement evaluations the integer-delay memo saved.

    python tools/haas_scan_rate.py [--runs 7] [--out FILE]
    python tools/haas_scan_rate.py --memo
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

FS, GRID, MAX_DELAY = 44100, 400, 0.03
SIGNALS = [dict(name='stereo_10s_44k1', seconds=10, channels=2), dict(name='stereo_60s_44k1', seconds=60, channels=2),
           dict(name='mono_10s_44k1', seconds=10, channels=1)]
WEIGHTS = dict(angle_limit=float(np.pi / 4), lambda_mean=5.0, lambda_skew=2.0, lambda_correlation=15.0,
               lambda_penalty=1e3)


def signal(spec):
    n = spec['seconds'] * FS
    x = np.random.default_rng(spec['seconds'] + spec['channels']).uniform(-1, 1, (n, spec['channels']))
    x = x.astype(np.float32)
    return x[:, 0].copy() if spec['channels'] == 1 else x


def quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kwargs)


def memo_count():
    from vndecorrelate_amd import optimization as opt
    opt.set_haas_scan_device(False)
    x = signal(SIGNALS[0])
    t = time.perf_counter()
    tau = quiet(opt.optimize_haas_delay, input_signal=x, sample_rate_hz=FS, max_delay_seconds=MAX_DELAY,
                grid_size=GRID, **WEIGHTS)
    memo = opt.last_haas_memo
    return dict(tool='haas_scan_rate', memo=dict(signal=SIGNALS[0]['name'], tau=float(tau), objective_calls=memo.calls,
                                                 host_evaluations=memo.evaluations,
                                                 saved=memo.calls - memo.evaluations,
                                                 wall_s=round(time.perf_counter() - t, 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--out', default=None)
    ap.add_argument('--memo', action='store_true')
    args = ap.parse_args()
    if args.memo:
        result = memo_count()
    else:
        result = rates(max(args.runs, 5))
    line = json.dumps(result)
    print(line)
    if args.out:
        pathlib.Path(args.out).write_text(line + '\n')


def rates(runs):
    import torch
    from vndecorrelate_amd import _native
    from vndecorrelate_amd import optimization as opt
    from vndecorrelate_amd.decorrelation import HaasEffect
    ctx = _native.default_context()
    dev = torch.device('cuda', ctx.device)
    stream = torch.cuda.current_stream(dev)
    taus = np.linspace(0.0, MAX_DELAY, GRID)
    cands = [HaasEffect(sample_rate_hz=FS, delay_time_seconds=t, mode='LR') for t in taus]
    delays = np.unique([round(t * FS) for t in taus]).astype(np.int32)
    result = dict(tool='haas_scan_rate', device=ctx.info()['name'], runs=runs, grid=GRID, max_delay_seconds=MAX_DELAY,
                  distinct_delays=int(delays.size), signals={})
    for spec in SIGNALS:
        x = signal(spec)
        x2 = np.ascontiguousarray(x.reshape(x.shape[0], -1))
        n, channels = x2.shape
        xd = torch.from_numpy(x2).to(dev)
        dd = torch.from_numpy(delays).to(dev)
        md = torch.empty((delays.size, _native.MOMENTS), dtype=torch.float64, device=dev)
        ws = _native.haas_scan_workspace_bytes(n, delays.size, int(delays.max()))
        wd = torch.empty(ws, dtype=torch.uint8, device=dev)

        def launch():
            _native.haas_scan_device(ctx, xd.data_ptr(), n, channels, dd.data_ptr(), delays.size, md.data_ptr(),
                                     delayed_channel=0, ms_mode=False, width=None, workspace_ptr=wd.data_ptr(),
                                     workspace_bytes=ws, stream=stream.cuda_stream)
        launch()
        torch.cuda.synchronize(dev)
        kernel_ms = []
        for _ in range(runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            launch()
            b.record(stream)
            b.synchronize()
            kernel_ms.append(a.elapsed_time(b))
        host_ms = []
        for _ in range(runs):
            t = time.perf_counter()
            scores = quiet(opt.grid_scan, x, cands, **WEIGHTS)
            host_ms.append((time.perf_counter() - t) * 1e3)
        pairs = int(np.sum(n + delays.astype(np.int64)))        # (frame, candidate) pairs of the distinct delays
        pick = np.linspace(0, GRID - 1, 8).astype(int)
        check = max(abs(scores[i] - opt.symmetry_aware_objective(x, cands[i], **WEIGHTS))
                    / max(1.0, abs(scores[i])) for i in pick)
        t = time.perf_counter()
        for i in (0, GRID // 2, GRID - 1):
            opt.symmetry_aware_objective(x, cands[i], **WEIGHTS)
        numpy_per = (time.perf_counter() - t) / 3
        k = statistics.median(kernel_ms)
        result['signals'][spec['name']] = dict(
            frames=n, channels=channels, kernel_ms=round(k, 3), kernel_min_ms=round(min(kernel_ms), 3),
            pairs_per_s=float(f'{pairs / (k * 1e-3):.4g}'), host_to_scores_ms=round(statistics.median(host_ms), 2),
            host_to_scores_min_ms=round(min(host_ms), 2), worst_score_error_of_8=float(f'{check:.3g}'),
            numpy_per_candidate_ms=round(numpy_per * 1e3, 1), numpy_grid_extrapolated_s=round(numpy_per * GRID, 1))
    return result


if __name__ == '__main__':
    main()
