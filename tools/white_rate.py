"""WhiteNoise on the device (vnd_white_noise_f32_dev): time of the dense float64 FIR alone and of the whole stage on three
pools, its FP64 rate, and NumPy's time for the same work.  Prints one JSON line.

Before timing, stream 0 of each pool is checked against np.convolve under the per-output bound of include/vnd_amd.h
(one float32 ulp + 2^-40 * sum |h x|), and the outputs identical to NumPy's are counted.  Device times are hipEvents on
the launch stream after a warm-up, the median of --runs.  NumPy is timed on one 10 s stream and EXTRAPOLATED to the
pool (one core, as WhiteNoise.decorrelate runs it).

    python tools/white_rate.py [--runs 5] [--out FILE]
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
    dict(name='stereo_2048x10s_44k1', batch=2048, fs=44100, seconds=10, in_channels=2, channels=2, taps=1323),
    dict(name='mono_to_stereo_128x10s_44k1', batch=128, fs=44100, seconds=10, in_channels=1, channels=2, taps=1323),
    dict(name='8ch_16x10s_96k', batch=16, fs=96000, seconds=10, in_channels=8, channels=8, taps=2880),
]


def _numpy_conv(x, h):
    out = np.zeros((x.shape[0], h.shape[1]), np.float32)
    for c in range(h.shape[1]):
        out[:, c] = np.convolve(x[:, c % x.shape[1]], h[:, c], mode='same')
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    runs = max(args.runs, 5)

    import torch
    from vndecorrelate_amd import _native
    ctx = _native.default_context()
    dev = torch.device('cuda', ctx.device)
    stream = torch.cuda.current_stream(dev)
    gen = torch.Generator(device=dev)
    result = dict(tool='white_rate', device=ctx.info()['name'], fp64_vector_spec_tflops=FP64_VECTOR_SPEC_TFLOPS,
                  runs=runs, pools={})
    for pool in POOLS:
        b, n, cx, c, m = pool['batch'], pool['fs'] * pool['seconds'], pool['in_channels'], pool['channels'], pool['taps']
        gen.manual_seed(1234)
        x = torch.randn((b, n, cx), generator=gen, device=dev, dtype=torch.float32)
        h_host = np.random.default_rng(5).standard_normal((m, c))
        h = torch.from_numpy(h_host).to(dev)
        y = torch.empty((b, n, c), device=dev, dtype=torch.float32)
        ws = _native.decorrelate_workspace_bytes(b, n, c)
        work = torch.empty((ws,), device=dev, dtype=torch.uint8)

        def launch(normalize, width=None):
            _native.white_noise_device(ctx, x.data_ptr(), h.data_ptr(), y.data_ptr(), b, n, cx, c, m, width=width,
                                       normalize=normalize, workspace_ptr=work.data_ptr(), workspace_bytes=ws,
                                       stream=stream.cuda_stream)

        # correctness of stream 0 against np.convolve before any timing
        launch(_native.NORMALIZE_OFF)
        torch.cuda.synchronize(dev)
        x0 = x[0].cpu().numpy()
        got = y[0].cpu().numpy()
        t = time.perf_counter()
        want = _numpy_conv(x0, h_host)
        numpy_stream_s = time.perf_counter() - t
        abs_sums = np.stack([np.convolve(np.abs(x0[:, k % cx].astype(np.float64)), np.abs(h_host[:, k]), mode='same')
                             for k in range(c)], axis=1)
        bound = np.spacing(np.abs(want)).astype(np.float64) + 2.0 ** -40 * abs_sums
        worst = float(np.max(np.abs(got.astype(np.float64) - want) / bound))
        if not worst <= 1.0:
            raise SystemExit(f'{pool["name"]}: stream 0 outside the bound ({worst:.3f} of it)')
        identical = int(np.count_nonzero(got == want))

        def timed(normalize):
            launch(normalize)                                  # warm-up
            stream.synchronize()
            times = []
            for _ in range(runs):
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record(stream)
                launch(normalize)
                stop.record(stream)
                stop.synchronize()
                times.append(start.elapsed_time(stop) / 1e3)
            return statistics.median(times), min(times)

        conv_s, conv_min = timed(_native.NORMALIZE_OFF)
        stage_s, stage_min = timed(_native.NORMALIZE_RMS_REFERENCE_ORDER)
        fma = b * n * c * m
        tflops = 2 * fma / conv_s / 1e12
        result['pools'][pool['name']] = dict(
            batch=b, frames=n, in_channels=cx, channels=c, taps=m,
            check_stream0=dict(worst_of_bound=round(worst, 4), identical=identical, outputs=int(got.size)),
            conv_ms=round(conv_s * 1e3, 3), conv_min_ms=round(conv_min * 1e3, 3),
            stage_ms=round(stage_s * 1e3, 3), stage_min_ms=round(stage_min * 1e3, 3),
            conv_fp64_tflops=round(tflops, 2), conv_share_of_fp64_spec=round(tflops / FP64_VECTOR_SPEC_TFLOPS, 3),
            numpy_one_stream_s=round(numpy_stream_s, 3), numpy_pool_extrapolated_s=round(numpy_stream_s * b, 1))
        del x, y, work
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(line + '\n')


if __name__ == '__main__':
    main()
