"""The correlogram voice pool on resident blocks (vnd_correlogram_voice_stream_f32_dev,
analysis.CorrelogramVoicePool.process_dev) against the lockstep stream it grew out of (vnd_correlogram_stream_f32_dev).
Prints one JSON line.

Pools of S slots of 44.1 kHz stereo noise at the reference's default sizes (W = 882, H = 441, 1765 lags), every slot live
and every block full (M frames): S x M = 512 x 480, 2048 x 480 and 2048 x 4800.
- ``lockstep``: ``vnd_correlogram_stream_f32_dev``, the position held by the host: one launch per block, a grid sized by
  the call's rows.  The baseline.
- ``voice``: ``CorrelogramVoicePool.process_dev`` called from Python: two launches per block, a grid fixed by the pool
  (ceil(M / H) rows per slot), positions read from the device state.
- ``graph``: the same call captured once with ``torch.cuda.graph`` and replayed.
Every time is between two device events on the current stream around --blocks back-to-back steady-state calls (the
Python calls inside: a live host pays them too); the forms alternate in a rotating order, median and minimum of --runs,
reported per block.  Before any timing the three forms run the same first blocks from position 0 and their rows are
checked bit-equal, call by call; after the timed runs - in which voice and graph made the same calls - their last rows are
compared again.  ``idle_workgroups``: the workgroups of the fixed grid that hold no row in a steady-state call, counted
from the pool's plan and the rows a call returns (the smaller of the two row counts a slot alternates between).

Each shape is a child process under its own ``timeout``; the tool stops at the first shape that fails.

    python tools/correlogram_voice_pool_rate.py [--runs 5] [--shapes 512x480,2048x480,2048x4800] [--blocks 50] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/correlogram_voice_pool_rate.py --step 2048x4800 --forms lockstep,voice   (a run of its own)
"""
import argparse
import json
import pathlib
import statistics
import subprocess
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

FS = 44100
STEP_SECONDS = 300
FORMS = ('lockstep', 'voice', 'graph')


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


class Lockstep:
    """vnd_correlogram_stream_f32_dev on the pool's sizes: the host holds the position."""

    def __init__(self, torch, ctx, pool, dev):
        from vndecorrelate_amd import _native
        self.native, self.torch, self.ctx, self.pool = _native, torch, ctx, pool
        S, M = pool.slots, pool.max_frames_per_call
        self.bytes = _native.correlogram_stream_state_bytes(S, pool.window, M)
        self.state = torch.empty(self.bytes, dtype=torch.uint8, device=dev)
        self.out = torch.empty((S, pool.rows_per_call, pool.num_lags), dtype=torch.float32, device=dev)   # compact: (S, rows, L)
        self.position = 0

    def call(self, x):
        p = self.pool
        M = p.max_frames_per_call
        rows = self.native.correlogram_stream_device(
            self.ctx, self.state.data_ptr(), self.bytes, M, x.data_ptr(), x.data_ptr() + 4, 2 * M, 2, self.out.data_ptr(),
            p.slots, self.position, M, window=p.window, hop=p.hop, num_lags=p.num_lags, eps=float(p.epsilon),
            stream=self.torch.cuda.current_stream().cuda_stream)
        self.position += M
        return rows


def step(slots, frames, blocks, runs, wanted):
    import torch
    from vndecorrelate_amd import _native, analysis
    from vndecorrelate_amd.streaming import VOICE_START
    ctx = _native.default_context()
    dev = torch.device('cuda', ctx.device)
    gen = torch.Generator(device=dev).manual_seed(slots)
    x = torch.rand((slots, frames, 2), generator=gen, device=dev, dtype=torch.float32) * 2 - 1

    def make():
        pool = analysis.cross_correlogram_voice_pool(slots, sample_rate_hz=FS, max_frames_per_call=frames)
        pool.reset()
        return pool
    pool, captured = make(), make()
    W, H, L, rc = pool.window, pool.hop, pool.num_lags, pool.rows_per_call
    plan = dict(f.split('=') for f in _native.describe_correlogram_voice_stream(slots, W, H, L, frames).split()[1:])
    counts = torch.full((slots,), frames, dtype=torch.int32, device=dev)
    flags = torch.zeros(slots, dtype=torch.int32, device=dev)
    lock = Lockstep(torch, ctx, pool, dev)
    out = (torch.empty((slots, rc, L), dtype=torch.float32, device=dev), torch.empty(slots, dtype=torch.int32, device=dev))
    out_g = (torch.empty_like(out[0]), torch.empty_like(out[1]))
    pool.process_dev(x, counts, flags, out=out)                            # loads the kernels before the capture
    pool.reset()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
    with torch.cuda.graph(graph, stream=side):
        captured.process_dev(x, counts, flags, out=out_g)
    torch.cuda.synchronize(dev)
    # the same first calls from position 0 in the three forms, bit-equal call by call
    row_counts = []
    for i in range(6):
        flags.fill_(VOICE_START if i == 0 else 0)
        rows = lock.call(x)
        pool.process_dev(x, counts, flags, out=out)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert out[1].tolist() == [rows] * slots == out_g[1].tolist(), (i, rows, out[1][:4].tolist())
        want = lock.out.view(-1)[:slots * rows * L].view(slots, rows, L).view(torch.int32)
        for name, got in (('voice', out[0]), ('graph', out_g[0])):
            assert torch.equal(got[:, :rows].view(torch.int32), want), f'{name} differs from the lockstep stream in call {i}'
        row_counts.append(rows)
    flags.fill_(0)
    steady = row_counts[2:]
    groups, tiles = int(plan['groups']), int(plan['tiles'])
    busy = -(-min(steady) // 4)
    row = {'slots': slots, 'frames': frames, 'blocks': blocks, 'runs': runs, 'audio_ms_per_block': fig(1000.0 * frames / FS),
           'rows_per_call': rc, 'steady_rows': sorted(set(steady)), 'workgroups': int(plan['nblocks']),
           'idle_workgroups': slots * (groups - busy) * tiles}
    calls = {'lockstep': lambda: lock.call(x), 'voice': lambda: pool.process_dev(x, counts, flags, out=out),
             'graph': graph.replay}
    names = [n for n in FORMS if n in wanted]

    def run(name):
        one = calls[name]
        for _ in range(blocks):
            one()
    times = {n: [] for n in names}
    for n in names:
        run(n)                                                             # warm
    torch.cuda.synchronize(dev)
    for r in range(runs):
        for n in names[r % len(names):] + names[:r % len(names)]:
            times[n].append(timed(torch, lambda: run(n)) / blocks)
    if 'voice' in names and 'graph' in names:                              # both made the same calls: the same last rows
        torch.cuda.synchronize(dev)
        k = int(out[1][0])
        assert out[1].tolist() == [k] * slots == out_g[1].tolist()
        assert torch.equal(out[0][:, :k].view(torch.int32), out_g[0][:, :k].view(torch.int32)), 'voice and graph differ after the timed runs'
    assert captured._state is not None                                     # the graph holds pointers into that pool's state
    for n in names:
        row[n + '_ms'] = fig(statistics.median(times[n]))
        row[n + '_min_ms'] = fig(min(times[n]))
    for n in ('voice', 'graph'):
        if n in times and 'lockstep' in times:
            row[f'{n}_over_lockstep'] = fig(statistics.median(times[n]) / statistics.median(times['lockstep']))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--shapes', default='512x480,2048x480,2048x4800')
    ap.add_argument('--blocks', type=int, default=50)
    ap.add_argument('--forms', default=','.join(FORMS))
    ap.add_argument('--step', default=None, help='SLOTSxFRAMES: run one shape in this process')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    wanted = tuple(args.forms.split(','))
    if args.step:
        slots, frames = (int(v) for v in args.step.split('x'))
        print(json.dumps(step(slots, frames, args.blocks, args.runs, wanted)))
        return
    rows = []
    for shape in args.shapes.split(','):
        cmd = ['timeout', '-k', '10', str(STEP_SECONDS), sys.executable, __file__, '--step', shape, '--runs', str(args.runs),
               '--blocks', str(args.blocks), '--forms', args.forms]
        done = subprocess.run(cmd, capture_output=True, text=True)
        if done.returncode != 0:
            print(done.stdout + done.stderr, file=sys.stderr)
            raise SystemExit(f'shape {shape} ended with status {done.returncode}: stopping')
        rows.append(json.loads(done.stdout.strip().splitlines()[-1]))
    line = json.dumps({'tool': 'correlogram_voice_pool_rate', 'rows': rows})
    print(line)
    if args.out:
        pathlib.Path(args.out).write_text(line + '\n')


if __name__ == '__main__':
    main()
