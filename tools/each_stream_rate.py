"""decorrelate_each_stream on resident blocks (vnd_each_stream_f32_dev, vnd_haas_each_stream_f64_dev) against the other
ways to stream a pool, exact mode.  Prints one JSON line.

Pools of S = 64, 256 and 2048 streams of 44.1 kHz stereo noise fed in --blocks blocks of 480 frames, every block a
resident device tensor.  Velvet noise: every stream its own kappa (30 ms / 30 impulses / seed 1, MS mode, no normaliser);
Haas: every stream its own delay up to 20 ms (LR, delayed channel 0).
- (a) ``each``: ONE ``decorrelate_each_stream`` object for the pool: one launch per block.
- (b) ``loop``: S single-stream ``VelvetNoise.stream()`` / ``HaasEffect.stream()`` objects called in a loop: S launches
  per block - the only way to stream a table per voice without (a).
- (c) ``shared``: one ``Stream`` / ``HaasStream`` of the same pool with ONE shared table / delay - the ceiling.
Every time is between two device events on the current stream around a whole signal (every block's ``process`` and the
``flush``), Python included - a live host pays it too; the three forms alternate in a rotating order, median of --runs,
reported per block.
Before any timing the concatenated outputs of (a) are checked bit-equal to (b) stream by stream, and the stream of (c)
whose own table / delay is the shared one to the same stream of (a).

Each (kind, S) step is a child process under its own ``timeout``; the tool stops at the first step that fails.

    python tools/each_stream_rate.py [--runs 5] [--pools 64,256,2048] [--blocks 50] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/each_stream_rate.py --step velvet:2048 --forms each,shared   (a run of its own)
"""
import argparse
import json
import pathlib
import statistics
import subprocess
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

FS, BLOCK = 44100, 480
VELVET = dict(sample_rate_hz=FS, duration_seconds=0.03, num_impulses=30, seed=1, normalizer=None)
MAX_DELAY = round(0.02 * FS)
STEP_SECONDS = 420                     # a step's time limit: the S = 2048 loop form makes 2048 launches per block


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


def step(kind, streams, blocks, runs, wanted):
    import torch
    import vndecorrelate_amd.decorrelation as dec
    from vndecorrelate_amd import _native
    ctx = _native.default_context()
    dev = torch.device('cuda', ctx.device)
    gen = torch.Generator(device=dev).manual_seed(streams)
    feed = [torch.rand((streams, BLOCK, 2), generator=gen, device=dev, dtype=torch.float32) * 2 - 1 for _ in range(blocks)]
    n = blocks * BLOCK
    if kind == 'velvet':
        stages = [dec.VelvetNoise(log_distribution_strength=float(k), **VELVET) for k in np.linspace(0.0, 1.0, streams)]
        tails = [0] * streams
        shared_row = 0
        bytes_per_frame = 16                               # 8 read, 8 written
    else:
        delays = np.rint(np.linspace(0, MAX_DELAY, streams)).astype(int)
        stages = [dec.HaasEffect(sample_rate_hz=FS, delay_time_seconds=float(d) / FS) for d in delays]
        assert [round(h.delay_time_seconds * FS) for h in stages] == delays.tolist()
        tails = delays.tolist()
        shared_row = streams - 1                           # the last stream's delay is the largest: the shared one
        bytes_per_frame = 24                               # 8 read, 16 written as float64
    each = dec.decorrelate_each_stream(stages, max_frames_per_call=BLOCK)
    row = dict(kind=kind, streams=streams, blocks=blocks, block_frames=BLOCK, latency_frames=each.latency_frames,
               tail_frames=getattr(each, 'tail_frames', 0), algorithmic_bytes_per_frame=bytes_per_frame)
    if kind == 'velvet':
        row['distinct_tables'] = each.arrays.num_channels // 2

    def run_each():
        each.reset()
        return [each.process(x) for x in feed] + [each.flush()]
    own = [d.stream(num_streams=1, max_frames_per_call=BLOCK) for d in stages] if 'loop' in wanted else []
    shared = stages[shared_row].stream(num_streams=streams, max_frames_per_call=BLOCK) if 'shared' in wanted else None

    def run_loop():
        for s in own:
            s.reset()
        outs = [[s.process(x[b:b + 1]) for b, s in enumerate(own)] for x in feed]
        return outs + [[s.flush() for s in own]]

    def run_shared():
        shared.reset()
        return [shared.process(x) for x in feed] + [shared.flush()]
    forms = {k: fn for k, fn in (('each', run_each), ('loop', run_loop), ('shared', run_shared)) if k in wanted}
    if len(forms) == 3:                                    # warm-up, and the outputs the checks read
        got = torch.cat(run_each(), dim=1)
        loop = run_loop()
        ref = torch.cat(run_shared(), dim=1)
        torch.cuda.synchronize()
        equal = True
        for b in range(streams):
            mine = torch.cat([call[b] for call in loop], dim=1)[0]            # (n + own tail, 2)
            equal &= bool(torch.equal(got[b, :n + tails[b]], mine)) and not bool(got[b, n + tails[b]:].any())
        row['each_equals_loop'] = equal
        row['shared_row_equals_each'] = bool(torch.equal(ref[shared_row], got[shared_row]))
        if not (row['each_equals_loop'] and row['shared_row_equals_each']):
            raise SystemExit(f'outputs differ: {row}')
        del got, loop, ref, mine
    else:                                                  # (a trace run of some forms: warm-up only)
        for fn in forms.values():
            fn()
        torch.cuda.synchronize()
    times = {k: [] for k in forms}
    order = list(forms)
    for i in range(runs):                                  # the forms alternate, each run starting one form later: the
        for k in order[i % len(order):] + order[:i % len(order)]:      # loop form leaves the device idle for whoever follows it
            times[k].append(timed(torch, forms[k]))
    for k, t in times.items():
        per_block = statistics.median(t) / blocks
        row[f'{k}_ms_per_block'] = fig(per_block)
        row[f'{k}_min_ms_per_block'] = fig(min(t) / blocks)
        row[f'{k}_GBps'] = fig(streams * BLOCK * bytes_per_frame / (per_block * 1e-3) / 1e9)
        row[f'{k}_x_realtime'] = fig(BLOCK / FS * 1e3 / per_block)        # > 1: the pool keeps up with live audio
    row['device'] = ctx.info()['name']
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--pools', default='64,256,2048')
    ap.add_argument('--blocks', type=int, default=50)
    ap.add_argument('--forms', default='each,loop,shared', help='a subset skips the equality checks: for a kernel trace')
    ap.add_argument('--step', default=None, help='KIND:STREAMS - one step in this process (what the tool runs per step)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    runs = max(args.runs, 5)
    if args.step:
        kind, streams = args.step.split(':')
        print(json.dumps(step(kind, int(streams), args.blocks, runs, args.forms.split(','))))
        return
    result = dict(tool='each_stream_rate', runs=runs, sample_rate_hz=FS, mode='exact',
                  velvet={k: v for k, v in VELVET.items() if k != 'normalizer'}, max_delay_frames=MAX_DELAY, steps=[])
    for streams in (int(s) for s in args.pools.split(',')):
        for kind in ('velvet', 'haas'):
            cmd = ['timeout', '-k', '10', str(STEP_SECONDS), sys.executable, __file__, '--step', f'{kind}:{streams}',
                   '--runs', str(runs), '--blocks', str(args.blocks), '--forms', args.forms]
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if done.returncode != 0:                        # a fault, a hang or a mismatch: nothing more runs
                print(done.stdout, file=sys.stderr)
                raise SystemExit(f'step {kind}:{streams} ended with status {done.returncode}: stopping')
            row = json.loads(done.stdout.strip().splitlines()[-1])
            result.setdefault('device', row.pop('device'))
            row.pop('device', None)
            result['steps'].append(row)
    line = json.dumps(result)
    print(line)
    if args.out:
        pathlib.Path(args.out).write_text(line + '\n')


if __name__ == '__main__':
    main()
