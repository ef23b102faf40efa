"""The voice pool on resident blocks (vnd_voice_stream_f32_dev, streaming.VoicePool.process_dev) against the lockstep
pool it grew out of (vnd_each_stream_f32_dev), exact mode.  Prints one JSON line.

Pools of S slots of 44.1 kHz stereo noise, every slot active and every block full (M frames), a kappa per slot (30 ms /
30 impulses / seed 1, MS mode, no normaliser): S x M = 512 x 480, 2048 x 480 (bound by issuing from Python) and
2048 x 4800 (bound by the work).
- ``lockstep``: ``vnd_each_stream_f32_dev`` on the same bank and tables, the position held by the host: one launch per
  block, a grid sized by the call.
- ``voice``: ``VoicePool.process_dev`` called from Python: two launches per block, a grid fixed by the pool (M + H frames
  per row), positions read from the device state.
- ``graph``: the same call captured once with ``torch.cuda.graph`` and replayed.
Every time is between two device events on the current stream around --blocks back-to-back steady-state calls (the
Python calls inside: a live host pays them too); the forms alternate in a rotating order, median and minimum of --runs,
reported per block.  Before any timing the three forms run the same first blocks from position 0 and their outputs
are checked bit-equal, call by call.

Each shape is a child process under its own ``timeout``; the tool stops at the first shape that fails.

    python tools/voice_pool_rate.py [--runs 5] [--shapes 512x480,2048x480,2048x4800] [--blocks 50] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/voice_pool_rate.py --step 2048x4800 --forms lockstep,voice   (a run of its own)
"""
import argparse
import json
import pathlib
import statistics
import subprocess
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

FS = 44100
VELVET = dict(sample_rate_hz=FS, duration_seconds=0.03, num_impulses=30, seed=1, normalizer=None)
TABLES = 64                            # distinct kappas in the bank; slot b runs table b % TABLES
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
    """vnd_each_stream_f32_dev on the pool's bank: the host holds the position."""

    def __init__(self, torch, ctx, pool, tables, dev):
        from vndecorrelate_amd import _native
        self.native, self.torch, self.ctx, self.pool, self.tables = _native, torch, ctx, pool, tables
        S, M, H = pool.slots, pool.max_frames_per_call, pool.latency_frames
        self.bytes = _native.each_stream_state_bytes(pool._table, S, pool.in_channels, M)
        self.state = torch.empty(max(self.bytes, 1), dtype=torch.uint8, device=dev)
        self.y = torch.empty((S, M + H, 2), dtype=torch.float32, device=dev)           # compact: (S, n_out, 2) of a call
        self.position = 0

    def call(self, x, final=False):
        p = self.pool
        n_out = self.native.each_stream_device(
            self.ctx, p._table, self.tables.data_ptr(), self.state.data_ptr(), self.bytes, p.max_frames_per_call,
            x.data_ptr(), self.y.data_ptr(), p.slots, self.position, p.max_frames_per_call, p.in_channels, final=final,
            ms_encode=p.ms_encode, width=p.width, stream=self.torch.cuda.current_stream().cuda_stream)
        self.position = 0 if final else self.position + p.max_frames_per_call
        return n_out


def step(slots, frames, blocks, runs, wanted):
    import torch
    import vndecorrelate_amd.decorrelation as dec
    from vndecorrelate_amd import _native
    from vndecorrelate_amd.streaming import VOICE_END, VOICE_START
    ctx = _native.default_context()
    dev = torch.device('cuda', ctx.device)
    bank = [dec.VelvetNoise(log_distribution_strength=k, **VELVET) for k in np.linspace(0.0, 1.0, TABLES)]
    gen = torch.Generator(device=dev).manual_seed(slots)
    x = torch.rand((slots, frames, 2), generator=gen, device=dev, dtype=torch.float32) * 2 - 1

    def make():
        pool = dec.decorrelate_voice_pool(bank, slots=slots, in_channels=2, max_frames_per_call=frames)
        pool.reset()
        return pool
    pool, captured = make(), make()
    H = pool.latency_frames
    tables = torch.from_numpy(pool.bank_tables[np.arange(slots) % TABLES].astype(np.int32)).to(dev)
    counts = torch.full((slots,), frames, dtype=torch.int32, device=dev)
    flags = torch.zeros(slots, dtype=torch.int32, device=dev)
    lock = Lockstep(torch, ctx, pool, tables, dev)
    out = (torch.empty((slots, frames + H, 2), dtype=torch.float32, device=dev), torch.empty(slots, dtype=torch.int32, device=dev))
    out_g = (torch.empty_like(out[0]), torch.empty_like(out[1]))
    pool.process_dev(x, counts, flags, tables, out=out)                    # loads the kernels before the capture
    pool.reset()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
    with torch.cuda.graph(graph, stream=side):
        captured.process_dev(x, counts, flags, tables, out=out_g)
    torch.cuda.synchronize(dev)

    # the same first calls from position 0 in the three forms, bit-equal call by call: START, two plain blocks, END
    for i, f in enumerate((VOICE_START, 0, 0, VOICE_END)):
        flags.fill_(f)
        n_out = lock.call(x, final=f == VOICE_END)
        pool.process_dev(x, counts, flags, tables, out=out)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert out[1].tolist() == [n_out] * slots == out_g[1].tolist(), (i, n_out)
        want = lock.y.view(-1)[:slots * n_out * 2].view(slots, n_out, 2).view(torch.int32)
        for name, got in (('voice', out[0]), ('graph', out_g[0])):
            assert torch.equal(got[:, :n_out].view(torch.int32), want), f'{name} differs from the lockstep pool in call {i}'
    # into the steady state: every call returns `frames` frames per slot
    flags.fill_(0)
    while lock.position <= H:
        lock.call(x)
        pool.process_dev(x, counts, flags, tables, out=out)
        graph.replay()
    torch.cuda.synchronize(dev)

    def run_lockstep():
        for _ in range(blocks):
            lock.call(x)

    def run_voice():
        for _ in range(blocks):
            pool.process_dev(x, counts, flags, tables, out=out)

    def run_graph():
        for _ in range(blocks):
            graph.replay()
    forms = {'lockstep': run_lockstep, 'voice': run_voice, 'graph': run_graph}
    names = [n for n in FORMS if n in wanted]
    times = {n: [] for n in names}
    for n in names:
        forms[n]()                                                         # warm
    torch.cuda.synchronize(dev)
    for r in range(runs):
        for n in names[r % len(names):] + names[:r % len(names)]:
            times[n].append(timed(torch, forms[n]) / blocks)
    row = {'slots': slots, 'frames': frames, 'latency_frames': H, 'blocks': blocks, 'runs': runs,
           'audio_ms_per_block': fig(1000.0 * frames / FS)}
    for n in names:
        row[n + '_ms'] = fig(statistics.median(times[n]))
        row[n + '_min_ms'] = fig(min(times[n]))
    for n in ('voice', 'graph'):
        if n in times and 'lockstep' in times:
            row[n + '_over_lockstep'] = fig(statistics.median(times[n]) / statistics.median(times['lockstep']))
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
    line = json.dumps({'tool': 'voice_pool_rate', 'rows': rows})
    print(line)
    if args.out:
        pathlib.Path(args.out).write_text(line + '\n')


if __name__ == '__main__':
    main()
