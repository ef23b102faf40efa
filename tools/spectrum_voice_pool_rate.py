"""The spectrum voice pool on resident blocks (vnd_spectrum_voice_stream_f32_dev, spectral.SpectrumVoicePool.process_dev)
beside the floor it can approach: the one-shot vnd_cross_spectra_f32_dev on an (S, M) pool of the same blocks - the same
frames through the same transform with no state, no ring and no history (it transforms the segments that lie inside one
block, ceil((M - nperseg + 1) / hop); the pool also transforms the ones that straddle two blocks, M / hop a call in steady
state).  Writes one JSON line to profiles/spectrum_voice_pool_rate.json (``--out``) and prints it.

Pools of S slots of stereo float32 noise at the coherence defaults (hann, nperseg 256, hop 128), every slot live and every
block full (M frames): S x M = 512 x 480, 2048 x 480 and 2048 x 4800.
- ``one_shot``: ``vnd_cross_spectra_f32_dev`` on the block, work memory allocated once.  The floor.
- ``means``: ``process_dev`` of a pool built with ``columns=False``, captured once with ``torch.cuda.graph`` and replayed.
- ``columns``: the same with the columns written.
Every time is between two device events on the current stream around --blocks back-to-back steady-state calls; the forms
alternate in a rotating order, median and minimum of --runs, reported per block.  Before any timing the means of the two
pools after the first calls are checked bit-equal with ``coherence_batched``'s three means of the frames pushed so far.

All shapes run in ONE child process under ``timeout``.

    python tools/spectrum_voice_pool_rate.py [--runs 5] [--shapes 512x480,2048x480,2048x4800] [--blocks 50] [--out FILE]
"""
import argparse
import json
import pathlib
import statistics
import subprocess
import sys

REPO = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

LIMIT_SECONDS = 600
FORMS = ('one_shot', 'means', 'columns')
NPERSEG, HOP = 256, 128


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


def shape_row(slots, frames, blocks, runs):
    import numpy as np
    import torch
    from vndecorrelate_amd import _native, spectral
    from vndecorrelate_amd.streaming import VOICE_START
    ctx = _native.default_context()
    dev = torch.device('cuda', ctx.device)
    gen = torch.Generator(device=dev).manual_seed(slots + frames)
    first = [torch.rand((slots, frames, 2), generator=gen, device=dev, dtype=torch.float32) * 2 - 1 for _ in range(3)]
    x = torch.empty_like(first[0])
    counts = torch.full((slots,), frames, dtype=torch.int32, device=dev)
    flags = torch.zeros(slots, dtype=torch.int32, device=dev)
    pools, graphs, outs = {}, {}, {}
    for name, columns in (('means', False), ('columns', True)):
        pool = spectral.spectrum_voice_pool(slots, frames, nperseg=NPERSEG, noverlap=NPERSEG - HOP, columns=columns)
        pool.reset()
        outs[name] = (torch.empty(pool._outputs[0][1], dtype=torch.float32, device=dev), torch.empty(slots, dtype=torch.int32, device=dev))
        graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
        with torch.cuda.graph(graph, stream=side):
            pool.process_dev(x, counts, flags, out=outs[name])
        pools[name], graphs[name] = pool, graph
    torch.cuda.synchronize(dev)
    # the first calls from position 0: the means equal the one-shot call on the frames so far, bit for bit
    for i, block in enumerate(first):
        x.copy_(block)
        flags.fill_(VOICE_START if i == 0 else 0)
        for g in graphs.values():
            g.replay()
        so_far = torch.cat(first[:i + 1], dim=1)
        want = (spectral.welch_batched(so_far, nperseg=NPERSEG)[1], torch.view_as_real(spectral.csd_batched(so_far, nperseg=NPERSEG)[1]))
        torch.cuda.synchronize(dev)
        for name, pool in pools.items():
            assert int(pool.segments[0]) == ((i + 1) * frames - NPERSEG) // HOP + 1
            assert torch.equal(pool.pxx.view(torch.int32), want[0][:, 0].contiguous().view(torch.int32)), (name, i, 'pxx')
            assert torch.equal(pool.pyy.view(torch.int32), want[0][:, 1].contiguous().view(torch.int32)), (name, i, 'pyy')
            assert torch.equal(pool.pxy.view(torch.int32), want[1].contiguous().view(torch.int32)), (name, i, 'pxy')
    flags.fill_(0)
    # the floor: the one-shot cross spectra of one block
    meter = pools['means']
    bins = meter.bins
    work_bytes = _native.cross_spectra_work_bytes(slots, frames, 2, NPERSEG, HOP, NPERSEG, False)
    work = torch.empty((max(1, work_bytes // 8),), dtype=torch.int64, device=dev)
    pxx, pyy = (torch.empty((slots, bins), dtype=torch.float32, device=dev) for _ in range(2))
    pxy = torch.empty((slots, bins, 2), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def one_shot():
        _native.cross_spectra_device(ctx, x.data_ptr(), slots, frames, 2 * frames, 2, 2, meter._win.data_ptr(), meter._tw.data_ptr(),
                                     NPERSEG, HOP, NPERSEG, pxx.data_ptr(), pyy.data_ptr(), pxy.data_ptr(), work_ptr=work.data_ptr(),
                                     work_bytes=work_bytes, detrend=True, scale=meter.scale, stream=stream)
    calls = {'one_shot': one_shot, 'means': graphs['means'].replay, 'columns': graphs['columns'].replay}

    def run(name):
        one = calls[name]
        for _ in range(blocks):
            one()
    names = list(FORMS)
    times = {n: [] for n in names}
    for n in names:
        run(n)                                                             # warm
    torch.cuda.synchronize(dev)
    for r in range(runs):
        for n in names[r % len(names):] + names[:r % len(names)]:
            times[n].append(timed(torch, lambda: run(n)) / blocks)
    plan = dict(f.split('=') for f in _native.describe_spectrum_voice_stream(slots, 2, NPERSEG, HOP, NPERSEG, frames).split()[1:])
    row = {'slots': slots, 'frames': frames, 'blocks': blocks, 'runs': runs, 'rows_per_call': int(plan['rows_per_call']),
           'run': int(plan['run']), 'workgroups': int(plan['nblocks']), 'steady_segments_per_call': fig(frames / HOP),
           'one_shot_segments_per_call': (frames - NPERSEG) // HOP + 1}
    for n in names:
        row[n + '_ms'] = fig(statistics.median(times[n]))
        row[n + '_min_ms'] = fig(min(times[n]))
    for n in ('means', 'columns'):
        row[f'{n}_over_one_shot'] = fig(statistics.median(times[n]) / statistics.median(times['one_shot']))
    assert np.isfinite([row[n + '_ms'] for n in names]).all()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--shapes', default='512x480,2048x480,2048x4800')
    ap.add_argument('--blocks', type=int, default=50)
    ap.add_argument('--child', action='store_true', help='run the shapes in this process')
    ap.add_argument('--out', default=str(REPO / 'profiles' / 'spectrum_voice_pool_rate.json'))
    args = ap.parse_args()
    if args.child:
        rows = [shape_row(*(int(v) for v in shape.split('x')), args.blocks, args.runs) for shape in args.shapes.split(',')]
        print(json.dumps({'tool': 'spectrum_voice_pool_rate', 'dtype': 'float32', 'channels': 2, 'window': 'hann', 'nperseg': NPERSEG,
                          'hop': HOP, 'rows': rows}))
        return
    cmd = ['timeout', '-k', '10', str(LIMIT_SECONDS), sys.executable, __file__, '--child', '--shapes', args.shapes, '--runs',
           str(args.runs), '--blocks', str(args.blocks)]
    done = subprocess.run(cmd, capture_output=True, text=True)
    if done.returncode != 0:
        print(done.stdout + done.stderr, file=sys.stderr)
        raise SystemExit(f'the measurement ended with status {done.returncode}')
    line = done.stdout.strip().splitlines()[-1]
    json.loads(line)
    print(line)
    pathlib.Path(args.out).write_text(line + '\n')


if __name__ == '__main__':
    main()
