"""The Haas voice pool and the chain voice pool on resident blocks (vnd_haas_voice_stream_f64_dev,
streaming.HaasVoicePool / ChainVoicePool .process_dev) against the lockstep pools they grew out of
(vnd_haas_each_stream_f64_dev, SignalChain.stream).  Prints one JSON line.

Pools of S slots of 44.1 kHz stereo noise, every slot active and every block full (M frames), 64 distinct delays up to
30 ms, slot b delayed by delay b % 64 (Haas LR, delayed channel 1): S x M = 512 x 480, 2048 x 480 and 2048 x 4800.
- ``lockstep``: ``vnd_haas_each_stream_f64_dev`` on the same delays, the position held by the host: one launch per block,
  a grid sized by the call.  The baseline.
- ``voice``: ``HaasVoicePool.process_dev`` called from Python: two launches per block, a grid fixed by the pool
  (M + max_delay frames per row), positions read from the device state.
- ``graph``: the same call captured once with ``torch.cuda.graph`` and replayed.
- ``chain_lockstep``: ``SignalChain.stream`` of VelvetNoise(MS, 30 ms / 30 impulses / seed 1, no normaliser) -> HaasEffect on
  device blocks, every stream through the chain of the largest delay: the baseline of the two chain forms.
- ``chain``: ``ChainVoicePool.process_dev`` from Python over the bank of that velvet filter with the 64 delays: four
  launches per block.
- ``chain_graph``: the same call captured and replayed.
Every time is between two device events on the current stream around --blocks back-to-back steady-state calls (the
Python calls inside: a live host pays them too); the forms alternate in a rotating order, median and minimum of --runs,
reported per block.  Before any timing the forms run the same first blocks from position 0 and their outputs are checked
bit-equal, call by call: the Haas forms against the lockstep entry over each stream's first n + d_b frames, the chain forms
against SignalChain.stream of three of the bank's chains on the slots that run them.

Each shape is a child process under its own ``timeout``; the tool stops at the first shape that fails.

    python tools/haas_voice_pool_rate.py [--runs 5] [--shapes 512x480,2048x480,2048x4800] [--blocks 50] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/haas_voice_pool_rate.py --step 2048x4800 --forms lockstep,voice   (a run of its own)
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
VELVET = dict(duration_seconds=0.03, num_impulses=30, seed=1, normalizer=None)
HAAS = dict(delayed_channel=1, mode='LR')
ENTRIES = 64                           # distinct delays in the bank; slot b runs entry b % ENTRIES
DELAYS = np.round(np.linspace(0, 0.03 * FS, ENTRIES)).astype(np.int32)
STEP_SECONDS = 300
FORMS = ('lockstep', 'voice', 'graph', 'chain_lockstep', 'chain', 'chain_graph')


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
    """vnd_haas_each_stream_f64_dev on the pool's delays: the host holds the position."""

    def __init__(self, torch, ctx, pool, delays, dev):
        from vndecorrelate_amd import _native
        self.native, self.torch, self.ctx, self.pool, self.delays = _native, torch, ctx, pool, delays
        S, M = pool.slots, pool.max_frames_per_call
        self.bytes = _native.haas_each_stream_state_bytes(S, pool.in_channels, pool.max_delay, M)
        self.state = torch.empty(max(self.bytes, 1), dtype=torch.uint8, device=dev)
        self.y = torch.empty((S, pool.row_frames, 2), dtype=torch.float64, device=dev)   # compact: (S, n_out, 2) of a call
        self.position = 0

    def call(self, x, final=False):
        p = self.pool
        n_out = self.native.haas_each_stream_device(
            self.ctx, self.state.data_ptr(), self.bytes, p.max_frames_per_call, x.data_ptr(), self.y.data_ptr(), p.slots,
            self.position, p.max_frames_per_call, p.in_channels, self.delays.data_ptr(), final=final, max_delay=p.max_delay,
            delayed_channel=p.delayed_channel, ms_mode=p.ms_mode, width=p.width,
            stream=self.torch.cuda.current_stream().cuda_stream)
        self.position = 0 if final else self.position + p.max_frames_per_call
        return n_out


def _captured(torch, dev, call):
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
    with torch.cuda.graph(graph, stream=side):
        call()
    torch.cuda.synchronize(dev)
    return graph


def replay(graph, pool):
    """One replay.  It names the pool the graph was captured on: the graph holds pointers into that pool's state and
    buffers, which must live as long as the graph is replayed."""
    assert pool._state is not None
    graph.replay()


def same_rows(torch, dev, out, out_g, frames, one, other):
    """After the timed runs, in which both forms made the same calls: the last steady-state call of either returned
    `frames` frames per slot, and the same ones."""
    torch.cuda.synchronize(dev)
    assert out[1].tolist() == [frames] * len(out[1]) == out_g[1].tolist(), \
        f'{one} and {other} after the timed runs: out_counts {out[1][:4].tolist()} and {out_g[1][:4].tolist()}, not {frames}'
    assert torch.equal(out[0][:, :frames].view(torch.int64), out_g[0][:, :frames].view(torch.int64)), \
        f'{one} and {other} differ after the timed runs'


def haas_forms(torch, dec, ctx, dev, x, slots, frames):
    """The three Haas forms, checked bit-equal and run into the steady state: ({name: one call}, max_delay)."""
    from vndecorrelate_amd.streaming import VOICE_END, VOICE_START
    bank = [dec.HaasEffect(sample_rate_hz=FS, delay_time_seconds=float(d) / FS, **HAAS) for d in DELAYS]

    def make():
        pool = dec.decorrelate_voice_pool(bank, slots=slots, in_channels=2, max_frames_per_call=frames)
        pool.reset()
        return pool
    pool, captured = make(), make()
    assert pool.bank_delays.tolist() == DELAYS.tolist()
    entry = np.arange(slots) % ENTRIES
    delays = torch.from_numpy(DELAYS[entry]).to(dev)
    counts = torch.full((slots,), frames, dtype=torch.int32, device=dev)
    flags = torch.zeros(slots, dtype=torch.int32, device=dev)
    lock = Lockstep(torch, ctx, pool, delays, dev)
    out = (torch.empty((slots, pool.row_frames, 2), dtype=torch.float64, device=dev),
           torch.empty(slots, dtype=torch.int32, device=dev))
    out_g = (torch.empty_like(out[0]), torch.empty_like(out[1]))
    pool.process_dev(x, counts, flags, delays, out=out)                    # loads the kernels before the capture
    pool.reset()
    graph = _captured(torch, dev, lambda: captured.process_dev(x, counts, flags, delays, out=out_g))
    # the same first calls from position 0 in the three forms, bit-equal call by call: START, two plain blocks, END
    for i, f in enumerate((VOICE_START, 0, 0, VOICE_END)):
        flags.fill_(f)
        n_out = lock.call(x, final=f == VOICE_END)
        pool.process_dev(x, counts, flags, delays, out=out)
        graph.replay()
        torch.cuda.synchronize(dev)
        own = frames + (DELAYS[entry] if f == VOICE_END else np.zeros(slots, np.int32))
        assert out[1].tolist() == own.tolist() == out_g[1].tolist(), (i, n_out)
        want = lock.y.view(-1)[:slots * n_out * 2].view(slots, n_out, 2).view(torch.int64)
        for name, got in (('voice', out[0]), ('graph', out_g[0])):
            for e in range(ENTRIES if f == VOICE_END else 1):               # each stream's first n + d_b frames
                rows = slice(e, None, ENTRIES) if f == VOICE_END else slice(None)
                k = frames + (int(DELAYS[e]) if f == VOICE_END else 0)
                assert torch.equal(got[rows, :k].view(torch.int64), want[rows, :k]), \
                    f'{name} differs from the lockstep pool in call {i}'
    flags.fill_(0)
    while lock.position <= pool.max_delay:                                  # into the steady state
        lock.call(x)
        pool.process_dev(x, counts, flags, delays, out=out)
        graph.replay()
    torch.cuda.synchronize(dev)
    return {'lockstep': lambda: lock.call(x), 'voice': lambda: pool.process_dev(x, counts, flags, delays, out=out),
            'graph': lambda: replay(graph, captured)}, pool.max_delay, \
        lambda: same_rows(torch, dev, out, out_g, frames, 'voice', 'graph')


def chain_forms(torch, dec, ctx, dev, x, slots, frames):
    """The three chain forms, checked bit-equal and run into the steady state: ({name: one call}, latency)."""
    from vndecorrelate_amd.streaming import VOICE_END, VOICE_START

    def chain(d):
        return (dec.SignalChain(sample_rate_hz=FS).velvet_noise(**VELVET)
                .haas_effect(delay_time_seconds=float(d) / FS, **HAAS))
    bank = [chain(d) for d in DELAYS]

    def make():
        pool = dec.decorrelate_voice_pool(bank, slots=slots, in_channels=2, max_frames_per_call=frames)
        pool.reset()
        return pool
    pool, captured = make(), make()
    H = pool.latency_frames
    entry = np.arange(slots) % ENTRIES
    tables = torch.from_numpy(pool.bank_tables[entry].astype(np.int32)).to(dev)
    delays = torch.from_numpy(pool.bank_delays[entry].astype(np.int32)).to(dev)
    counts = torch.full((slots,), frames, dtype=torch.int32, device=dev)
    flags = torch.zeros(slots, dtype=torch.int32, device=dev)
    out = (torch.empty((slots, pool.row_frames, 2), dtype=torch.float64, device=dev),
           torch.empty(slots, dtype=torch.int32, device=dev))
    out_g = (torch.empty_like(out[0]), torch.empty_like(out[1]))
    pool.process_dev(x, counts, flags, tables, delays, out=out)            # loads the kernels before the capture
    pool.reset()
    graph = _captured(torch, dev, lambda: captured.process_dev(x, counts, flags, tables, delays, out=out_g))
    # START, two plain blocks, END alone - against SignalChain.stream of three of the bank's chains, each on every stream:
    # the slots that run that chain are compared
    locks = {e: chain(DELAYS[e]).stream(num_streams=slots, in_channels=2, max_frames_per_call=frames) for e in (0, 31, ENTRIES - 1)}
    assert all(s.latency_frames == H for s in locks.values())
    for i, f in enumerate((VOICE_START, 0, 0, VOICE_END)):
        flags.fill_(f)
        counts.fill_(0 if f == VOICE_END else frames)                       # (the captured call reads these tensors)
        pool.process_dev(x, counts, flags, tables, delays, out=out)
        graph.replay()
        torch.cuda.synchronize(dev)
        for e, s in locks.items():
            want = s.flush() if f == VOICE_END else s.process(x)
            k = want.shape[1]
            rows = slice(e, None, ENTRIES)
            assert out[1][rows].tolist() == [k] * len(range(e, slots, ENTRIES)) == out_g[1][rows].tolist(), (i, e, k)
            for name, got in (('chain', out[0]), ('chain_graph', out_g[0])):
                assert torch.equal(got[rows, :k].view(torch.int64), want[rows].contiguous().view(torch.int64)), \
                    f'{name} differs from SignalChain.stream in call {i}, entry {e}'
    lock = locks[ENTRIES - 1]
    lock.reset()
    flags.fill_(0)
    counts.fill_(frames)
    for _ in range(H // frames + 2):                                        # into the steady state
        lock.process(x)
        pool.process_dev(x, counts, flags, tables, delays, out=out)
        graph.replay()
    torch.cuda.synchronize(dev)
    return {'chain_lockstep': lambda: lock.process(x),
            'chain': lambda: pool.process_dev(x, counts, flags, tables, delays, out=out),
            'chain_graph': lambda: replay(graph, captured)}, H, \
        lambda: same_rows(torch, dev, out, out_g, frames, 'chain', 'chain_graph')


def step(slots, frames, blocks, runs, wanted):
    import torch
    import vndecorrelate_amd.decorrelation as dec
    from vndecorrelate_amd import _native
    ctx = _native.default_context()
    dev = torch.device('cuda', ctx.device)
    gen = torch.Generator(device=dev).manual_seed(slots)
    x = torch.rand((slots, frames, 2), generator=gen, device=dev, dtype=torch.float32) * 2 - 1
    row = {'slots': slots, 'frames': frames, 'blocks': blocks, 'runs': runs, 'audio_ms_per_block': fig(1000.0 * frames / FS)}
    calls, checks = {}, []
    if any(n in wanted for n in FORMS[:3]):
        forms, row['max_delay'], check = haas_forms(torch, dec, ctx, dev, x, slots, frames)
        calls.update(forms)
        checks.append(('voice', 'graph', check))
    if any(n in wanted for n in FORMS[3:]):
        forms, row['latency_frames'], check = chain_forms(torch, dec, ctx, dev, x, slots, frames)
        calls.update(forms)
        checks.append(('chain', 'chain_graph', check))
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
    for one, other, check in checks:                                       # both made the same calls: the same last rows
        if one in names and other in names:
            check()
    for n in names:
        row[n + '_ms'] = fig(statistics.median(times[n]))
        row[n + '_min_ms'] = fig(min(times[n]))
    for n, base in (('voice', 'lockstep'), ('graph', 'lockstep'), ('chain', 'chain_lockstep'), ('chain_graph', 'chain_lockstep')):
        if n in times and base in times:
            row[f'{n}_over_{base}'] = fig(statistics.median(times[n]) / statistics.median(times[base]))
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
    line = json.dumps({'tool': 'haas_voice_pool_rate', 'rows': rows})
    print(line)
    if args.out:
        pathlib.Path(args.out).write_text(line + '\n')


if __name__ == '__main__':
    main()
