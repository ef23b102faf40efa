"""Cross-correlograms on the device (vnd_correlogram_f32_dev): time, FP64 rate and output bandwidth on three pools, and
NumPy's time for the same work.  Prints one JSON line.

Before timing, stream 0 of each pool is compared with the reference's NumPy loop (``cross_correlogram`` with the device
off): the worst absolute distance and the count of identical outputs.  Device times are hipEvents on the launch stream
after a warm-up, the median of --runs.  NumPy is timed on one stream and EXTRAPOLATED to the pool (one core).  Useful
FMAs are W^2 per window (the triangle of the full correlation) plus 2W for the energies.

    python tools/correlogram_rate.py [--runs 7] [--out FILE]
"""
import argparse
import json
import pathlib
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

FP64_VECTOR_SPEC_TFLOPS = 78.6          # AMD's published MI355X FP64 vector peak; not measured on these boards

POOLS = [
    dict(name='velvet_LR_256x10s_44k1', batch=256, fs=44100, seconds=10, lag=0.02, window=0.02, stride=0.01,
         source='velvet'),
    dict(name='noise_64x10s_96k_w50ms', batch=64, fs=96000, seconds=10, lag=0.05, window=0.05, stride=0.025,
         source='noise'),
    dict(name='sweep_2048x1s_16k', batch=2048, fs=16000, seconds=1, lag=0.02, window=0.02, stride=0.01, source='sweep'),
]


def make_pool(pool, torch, dev):
    """Device float32 (B, n, 2): channel 0 against channel 1, correlated in place."""
    b, n = pool['batch'], int(pool['fs'] * pool['seconds'])
    if pool['source'] == 'velvet':
        import vndecorrelate_amd.decorrelation as vnd
        mono = np.random.default_rng(1).uniform(-1, 1, (b, n)).astype(np.float32)
        st = vnd.VelvetNoise(sample_rate_hz=pool['fs'], seed=1, filtered_channels=(0,)).decorrelate_batched(
            np.repeat(mono[:, :, None], 2, axis=2))
        return torch.from_numpy(np.ascontiguousarray(st)).to(dev)
    if pool['source'] == 'sweep':
        from vndecorrelate_amd.utils.dsp import sine_sweep
        s = sine_sweep(20, 8000, pool['seconds'], pool['fs'])
        st = np.empty((b, n, 2), np.float32)
        st[:, :, 0] = s
        st[:, :, 1] = s + 0.05 * np.random.default_rng(2).standard_normal((b, n)).astype(np.float32)
        return torch.from_numpy(st).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    return torch.rand((b, n, 2), generator=gen, device=dev, dtype=torch.float32) * 2 - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    runs = max(args.runs, 5)

    import torch
    from vndecorrelate_amd import _native, analysis
    from vndecorrelate_amd.utils import dsp
    ctx = _native.default_context()
    dev = torch.device('cuda', ctx.device)
    stream = torch.cuda.current_stream(dev)
    result = dict(tool='correlogram_rate', device=ctx.info()['name'], fp64_vector_spec_tflops=FP64_VECTOR_SPEC_TFLOPS,
                  runs=runs, pools={})
    for pool in POOLS:
        x = make_pool(pool, torch, dev)
        b, n = x.shape[:2]
        W, hop, max_lag = dsp.correlogram_sizes(pool['fs'], pool['lag'], pool['window'], pool['stride'])
        lags = 2 * max_lag + 1
        kw = dict(sample_rate_hz=pool['fs'], max_lag_seconds=pool['lag'], window_size_seconds=pool['window'],
                  stride_seconds=pool['stride'])

        def launch():
            return analysis._launch(torch, ctx, x.data_ptr(), x.data_ptr() + 4, b, n, x.stride(0), x.stride(1), W, hop,
                                    lags, 1e-10, dev)

        out = launch()
        torch.cuda.synchronize(dev)
        got = out[0].cpu().numpy()
        x0 = x[0].cpu().numpy()
        analysis.set_correlogram_device(False)
        t = time.perf_counter()
        want = dsp.cross_correlogram(np.ascontiguousarray(x0[:, 0]), np.ascontiguousarray(x0[:, 1]), **kw)
        numpy_stream_s = time.perf_counter() - t
        analysis.set_correlogram_device(None)
        worst = float(np.max(np.abs(got.astype(np.float64) - want)))
        identical = int(np.count_nonzero(got == want))
        if not worst <= (2 * W + 4) * 2.0 ** -24:
            raise SystemExit(f'{pool["name"]}: stream 0 is {worst:.3g} from NumPy, outside (2W + 4) 2^-24')
        del out
        times = []
        for _ in range(runs):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record(stream)
            out = launch()
            stop.record(stream)
            stop.synchronize()
            times.append(start.elapsed_time(stop) / 1e3)
            del out
        med = statistics.median(times)
        windows = (n - W) // hop + 1
        fma = b * windows * (W * W + 2 * W)
        tflops = 2 * fma / med / 1e12
        out_bytes = b * windows * lags * 4
        result['pools'][pool['name']] = dict(
            batch=b, frames=n, window=W, hop=hop, lags=lags, windows=windows,
            check_stream0=dict(worst_abs=worst, identical=identical, outputs=int(got.size)),
            device_ms=round(med * 1e3, 3), device_min_ms=round(min(times) * 1e3, 3), useful_fma=fma,
            fp64_tflops=round(tflops, 2), share_of_fp64_spec=round(tflops / FP64_VECTOR_SPEC_TFLOPS, 3),
            output_gb=round(out_bytes / 1e9, 3), output_gb_per_s=round(out_bytes / med / 1e9, 1),
            numpy_one_stream_s=round(numpy_stream_s, 3), numpy_pool_extrapolated_s=round(numpy_stream_s * b, 1))
        del x
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(line + '\n')


if __name__ == '__main__':
    main()
