"""The polar level envelope on resident pools (vnd_polar_level_f32_dev / _f64_dev) at the default 360 slices
and p = (95, 50), against the polar histogram on the same pool in the same run (vnd_polar_hist_*_dev, the default 240 x 150
grid: the yardstick for "one pass with atan2") and against the NumPy loop - the reference's mask and np.percentile per
slice - on one signal of the pool, scaled to the batch.  Prints one JSON line; nothing here is asserted but that two runs of a
call give the same bytes and that the frames per slice add up.

Cases, frames drawn on the device from a seed, each for float32 and float64 pools:
- ``gauss``: 256 x 480 000 frames of Gaussian noise (sigma 0.25), per-signal maximum;
- ``mono``: the same shape with every signal mono (L = R): one slice holds every frame - the contention case;
- ``quiet``: the Gaussian pool x 0.02 with a fixed ``radius_scale`` of 1: the keys crowd a few digits;
- ``block``: 2048 x 480, the per-block shape: launch-bound.
Every time is between two device events around ``reps`` back-to-back calls on the current stream, after two warm-up rounds;
the forms alternate in a rotating order; median and minimum of --runs, per call.

Each case is a child process under its own ``timeout``; the tool stops at the first case that fails.

    python tools/polar_level_rate.py [--runs 5] [--cases gauss,mono,quiet,block] [--out profiles/polar_level_rate.json]
"""
import argparse
import json
import pathlib
import statistics
import subprocess
import sys
import time

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

STEP_SECONDS = 300
CASES = ('gauss', 'mono', 'quiet', 'block')
BINS, PS = 360, (95.0, 50.0)


def timed(torch, fn):
    stream = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def fig(value):
    return float(f'{value:.4g}')


def measure(torch, forms, reps, runs):
    """forms: {name: callable}.  Median and minimum per call, the forms alternating in a rotating order."""
    names = list(forms)

    def run(name):
        for _ in range(reps):
            forms[name]()
    for _ in range(2):
        for name in names:
            run(name)
    torch.cuda.synchronize()
    times = {name: [] for name in names}
    for r in range(runs):
        for name in names[r % len(names):] + names[:r % len(names)]:
            times[name].append(timed(torch, lambda: run(name)) / reps)
    return {name: (statistics.median(t), min(t)) for name, t in times.items()}


def step(case, f64, runs):
    import numpy as np
    import torch
    from vndecorrelate_amd import _native, vectorscope
    ctx = _native.default_context()
    dev = torch.device('cuda', ctx.device)
    batch, frames = (2048, 480) if case == 'block' else (256, 480000)
    reps = 20 if case == 'block' else 3
    dtype = torch.float64 if f64 else torch.float32
    size = 8 if f64 else 4
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((batch, frames, 2), generator=gen, device=dev, dtype=torch.float32).to(dtype) * 0.25
    if case == 'mono':
        x[:, :, 1] = x[:, :, 0]
    if case == 'quiet':
        x *= 0.02
    scale = 1.0 if case == 'quiet' else 0.0
    stream = torch.cuda.current_stream().cuda_stream
    lp, rp = x.data_ptr(), x.data_ptr() + size
    edges, _ = vectorscope.level_edges(BINS)
    d_edges = torch.from_numpy(edges).to(dev)
    levels = torch.empty((batch, len(PS), BINS), dtype=dtype, device=dev)
    counts = torch.empty((batch, BINS), dtype=torch.int32, device=dev)
    need = _native.polar_level_work_bytes(batch, frames, BINS, len(PS), f64)
    work = torch.empty((need // 8,), dtype=torch.int64, device=dev)
    a0, a1 = vectorscope.polar_edges()
    d_a0, d_a1 = torch.from_numpy(a0).to(dev), torch.from_numpy(a1).to(dev)
    grid = torch.empty((batch, len(a0) - 1, len(a1) - 1), dtype=torch.int32, device=dev)
    hist_work = torch.empty((batch,), dtype=torch.int64, device=dev)

    def level():
        _native.polar_level_device(ctx, lp, rp, batch, frames, 2 * frames, 2, d_edges.data_ptr(), BINS, PS, levels.data_ptr(),
                                   counts.data_ptr(), work_ptr=work.data_ptr(), work_bytes=need, radius_scale=scale,
                                   float64=f64, stream=stream)

    def hist():
        _native.polar_hist_device(ctx, lp, rp, batch, frames, 2 * frames, 2, d_a0.data_ptr(), len(a0) - 1, d_a1.data_ptr(),
                                  len(a1) - 1, grid.data_ptr(), radius_scale=scale, work_ptr=0 if scale else hist_work.data_ptr(),
                                  work_bytes=0 if scale else 8 * batch, float64=f64, stream=stream)

    level()
    torch.cuda.synchronize()
    first = (levels.clone(), counts.clone())
    level()
    torch.cuda.synchronize()
    assert torch.equal(first[0].view(torch.int64 if f64 else torch.int32), levels.view(torch.int64 if f64 else torch.int32))
    assert torch.equal(first[1], counts), 'two runs of one call differ'
    kept = int(counts.to(torch.int64).sum())
    assert kept <= batch * frames
    got = measure(torch, {'level': level, 'hist': hist}, reps, runs)
    # the NumPy loop on signal 0, once
    host = x[0].cpu().numpy()
    vectorscope.set_scope_device(False)
    t0 = time.perf_counter()
    want = vectorscope.polar_level_batched(host, BINS, PS, radius_scale=scale or None)
    numpy_ms = (time.perf_counter() - t0) * 1e3
    vectorscope.set_scope_device(None)
    # (the NumPy loop's own atan2 may move a frame across an edge: the count of differing slices is recorded, not asserted)
    differing = int((want[1] != counts[0].cpu().numpy().view(np.uint32)).sum())
    total = batch * frames
    cells, digit = BINS * len(PS), 1                                # level_digit_bits of csrc/vnd_level.hpp
    while digit < 8 and cells * ((4 << (digit + 1)) + size) <= vectorscope.LDS_BYTES \
            and (cells << (digit + 1)) <= 8 * min(frames, vectorscope.LEVEL_SPAN_FRAMES):
        digit += 1
    passes = -(-8 * size // digit)
    row = {'case': case, 'dtype': 'float64' if f64 else 'float32', 'batch': batch, 'frames': frames, 'bins': BINS,
           'percentiles': list(PS), 'reps': reps, 'runs': runs, 'frames_in_a_slice': kept,
           'busiest_slice': int(counts.max()), 'digit_bits': digit, 'select_passes': passes, 'work_MiB': fig(need / 2 ** 20),
           'numpy_loop_one_signal_ms': fig(numpy_ms), 'numpy_loop_scaled_ms': fig(numpy_ms * batch),
           'slices_where_numpy_counts_differ_signal_0': differing}
    for form, (median, least) in got.items():
        row[form] = {'ms': fig(median), 'min_ms': fig(least), 'Gframes_per_s': fig(total / (median * 1e6)),
                     'input_GBps': fig(2 * size * total / (median * 1e6))}
    row['level_over_hist'] = fig(got['level'][0] / got['hist'][0])
    row['numpy_scaled_over_level'] = fig(numpy_ms * batch / got['level'][0])
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--cases', default=','.join(CASES))
    ap.add_argument('--step', default=None, help='run one case in this process: CASE:f32 or CASE:f64')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.step:
        case, kind = args.step.split(':')
        print(json.dumps(step(case, kind == 'f64', args.runs)))
        return
    rows = []
    for case in args.cases.split(','):
        for kind in ('f32', 'f64'):
            cmd = ['timeout', '-k', '10', str(STEP_SECONDS), sys.executable, __file__, '--step', f'{case}:{kind}', '--runs',
                   str(args.runs)]
            done = subprocess.run(cmd, capture_output=True, text=True)
            if done.returncode != 0:
                print(done.stdout + done.stderr, file=sys.stderr)
                raise SystemExit(f'case {case}:{kind} ended with status {done.returncode}: stopping')
            rows += json.loads(done.stdout.strip().splitlines()[-1])
    ratios = {}
    for kind in ('float32', 'float64'):
        by = {r['case']: r['level']['ms'] for r in rows if r['dtype'] == kind}
        if 'gauss' in by and 'mono' in by:
            ratios[kind] = fig(by['mono'] / by['gauss'])
    line = json.dumps({'tool': 'polar_level_rate', 'mono_over_gauss': ratios, 'rows': rows})
    print(line)
    if args.out:
        pathlib.Path(args.out).write_text(line + '\n')


if __name__ == '__main__':
    main()
