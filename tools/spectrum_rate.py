"""Short-time spectra on a resident pool (vnd_spectrogram_f32_dev, vnd_cross_spectra_f32_dev): a 256 x 480 000
stereo float32 pool through ``spectrogram_batched`` and ``coherence_batched`` at the SciPy defaults (``default``: nperseg 256,
the spectrogram's overlap an eighth, the coherence's a half) and at ``nperseg=4096`` (``wide``), against the SciPy loop on the
host on one signal of the pool, scaled to the batch.  Prints one JSON line; nothing here is asserted but that two runs of a
call give the same bytes.

Every device time is between two device events around ``reps`` back-to-back calls on the current stream, after two warm-up
rounds; the forms alternate in a rotating order; median and minimum of --runs, per call.  ``of_byte_bound`` is the time the
call's bytes - every frame read once, every output written once - take at 8 TB/s, over the measured time.

Each case is a child process under its own ``timeout``; the tool stops at the first case that fails.

    python tools/spectrum_rate.py [--runs 5] [--cases default,wide] [--out profiles/spectrum_rate.json]
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
CASES = {'default': 256, 'wide': 4096}
BATCH, FRAMES = 256, 480000
HBM_BYTES_PER_S = 8e12


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


def step(case, runs):
    import torch
    from scipy.signal import coherence, spectrogram
    from vndecorrelate_amd import _native, spectral
    ctx = _native.default_context()
    dev = torch.device('cuda', ctx.device)
    nperseg, reps = CASES[case], 3
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand((BATCH, FRAMES, 2), generator=gen, device=dev, dtype=torch.float32) * 2 - 1
    x[:, :, 1] = 0.6 * x[:, :, 0] + 0.8 * x[:, :, 1]
    spectral.set_spectrum_device(True)
    f, t, sxx = spectral.spectrogram_batched(x, nperseg=nperseg)
    out = torch.empty_like(sxx)
    forms = {'spectrogram': lambda: spectral.spectrogram_batched(x, nperseg=nperseg, out=out),
             'coherence': lambda: spectral.coherence_batched(x, nperseg=nperseg)}
    forms['spectrogram']()
    cxy = forms['coherence']()[1]
    torch.cuda.synchronize()
    assert torch.equal(sxx.view(torch.int32), out.view(torch.int32)), 'two runs of the spectrogram differ'
    assert torch.equal(cxy.view(torch.int32), forms['coherence']()[1].view(torch.int32)), 'two runs of the coherence differ'
    got = measure(torch, forms, reps, runs)
    # the SciPy loop on signal 0, once
    host = x[0].cpu().numpy()
    t0 = time.perf_counter()
    spectrogram(host[:, 0], nperseg=nperseg)
    spectrogram(host[:, 1], nperseg=nperseg)
    scipy_gram_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    coherence(host[:, 0], host[:, 1], nperseg=nperseg)
    scipy_coh_ms = (time.perf_counter() - t0) * 1e3
    in_bytes = 4 * 2 * BATCH * FRAMES
    hop = {'spectrogram': nperseg - nperseg // 8, 'coherence': nperseg // 2}
    work = _native.cross_spectra_work_bytes(BATCH, FRAMES, 2, nperseg, hop['coherence'], nperseg)
    out_bytes = {'spectrogram': 4 * sxx.numel(), 'coherence': 2 * work + 4 * 4 * BATCH * (nperseg // 2 + 1)}
    scipy_ms = {'spectrogram': scipy_gram_ms, 'coherence': scipy_coh_ms}
    row = {'case': case, 'dtype': 'float32', 'batch': BATCH, 'frames': FRAMES, 'channels': 2, 'nperseg': nperseg, 'nfft': nperseg,
           'reps': reps, 'runs': runs, 'columns': int(sxx.shape[-1]), 'floats_out_per_input_frame': fig(sxx.numel() / (2 * BATCH * FRAMES)),
           'run_length': {'spectrogram': spectral.run_length(nperseg, nperseg, hop['spectrogram']),
                          'coherence': spectral.run_length(nperseg, nperseg, hop['coherence'], cross_channels=2)}}
    for form, (median, least) in got.items():
        bound_ms = (in_bytes + out_bytes[form]) / HBM_BYTES_PER_S * 1e3
        row[form] = {'ms': fig(median), 'min_ms': fig(least), 'Gframes_per_s': fig(BATCH * FRAMES / (median * 1e6)),
                     'read_MB': fig(in_bytes / 1e6), 'written_MB': fig(out_bytes[form] / 1e6), 'byte_bound_ms': fig(bound_ms),
                     'of_byte_bound': fig(bound_ms / median), 'scipy_loop_one_signal_ms': fig(scipy_ms[form]),
                     'scipy_loop_scaled_ms': fig(scipy_ms[form] * BATCH), 'scipy_scaled_over_device': fig(scipy_ms[form] * BATCH / median)}
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--cases', default=','.join(CASES))
    ap.add_argument('--step', default=None, help='run one case in this process')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.step:
        print(json.dumps(step(args.step, args.runs)))
        return
    rows = []
    for case in args.cases.split(','):
        cmd = ['timeout', '-k', '10', str(STEP_SECONDS), sys.executable, __file__, '--step', case, '--runs', str(args.runs)]
        done = subprocess.run(cmd, capture_output=True, text=True)
        if done.returncode != 0:
            print(done.stdout + done.stderr, file=sys.stderr)
            raise SystemExit(f'case {case} ended with status {done.returncode}: stopping')
        rows += json.loads(done.stdout.strip().splitlines()[-1])
    line = json.dumps({'tool': 'spectrum_rate', 'rows': rows})
    print(line)
    if args.out:
        pathlib.Path(args.out).write_text(line + '\n')


if __name__ == '__main__':
    main()
