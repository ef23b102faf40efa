"""The polar-moments voice pool on resident blocks (vnd_polar_voice_stream_f32_dev, analysis.PolarVoicePool.process_dev)
against the one-shot reducer it streams (vnd_polar_moments_f32_dev with one pair).  Prints one JSON line.

Pools of S slots of stereo noise, every slot live and every block full (M frames): S x M = 512 x 480, 2048 x 480 and
2048 x 4800, and one ragged case (``2048x480r``) in which every second slot pushes one frame.
- ``voice``: ``PolarVoicePool.process_dev`` called from Python: two launches per block, a grid fixed by the pool
  (ceil(M / 512) + 1 chunk workgroups per slot, then one workgroup per slot), positions read from the device state.
- ``graph``: the same call captured once with ``torch.cuda.graph`` and replayed.
- ``oneshot_flat``: ``vnd_polar_moments_f32_dev`` once per block over the same S x M frames taken as ONE one-pair signal:
  two launches, the same frames read - the kernel work of the block without any pool, and no voice's answer.
- ``oneshot_each``: ``vnd_polar_moments_f32_dev`` per slot on that slot's block alone, S x 2 launches per block: what a
  server without the pool could issue per block (and it would still have only the block's moments, not the voice's).
Every time is between two device events on the current stream around --blocks back-to-back steady-state calls (the
Python calls inside: a live host pays them too); the forms alternate in a rotating order, median and minimum of --runs,
reported per block.  Before any timing voice and graph run the same first three calls from a START and every slot's
moments are checked bit-equal to the one-shot call on that voice's frames so far (every slot after the second call, 64
slots after the others); after the timed runs - in which voice and graph made the same calls - their rows are compared.

Steady state: a finish workgroup loads lane t's sums only when t < floor(p / 512), so a young voice loads fewer than
the 256 lanes a voice past 131 072 frames loads on every call.  After the checks both pools are therefore pushed
``prefill_calls`` further blocks, until every slot that pushes full blocks has 256 completed chunks, and only then
warmed and timed.  ``lanes_loaded`` is the mean number of lanes a slot's finish workgroup loaded over the TIMED calls,
computed from the positions those calls ran at ([full-block slots, one-frame slots] in the ragged case, whose one-frame
slots stay young: they never complete a chunk in the run).

``idle_workgroups``: the chunk workgroups of the fixed grid that leave at once in a steady-state call, a mean over the
positions k M, from the pool's plan.  ``state_bytes_per_call``: what a timed call moves besides the block, counted from
the code and the positions, not from a counter - 64 bytes for every lane sum loaded (``lanes_loaded``) and for every
chunk completed, the open chunk read from and written to the ring, the partials written and read, moments, valid and
positions - against ``block_bytes``, and ``copy_bytes`` = 2 x block_bytes, what a copy of the block moves.

Each shape is a child process under its own ``timeout``; the tool stops at the first shape that fails.

    python tools/polar_voice_pool_rate.py [--runs 5] [--shapes 512x480,2048x480,2048x4800,2048x480r] [--blocks 50] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/polar_voice_pool_rate.py --step 2048x4800 --forms voice   (a run of its own)
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
FORMS = ('voice', 'graph', 'oneshot_flat', 'oneshot_each')
CHUNK = 512


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


class OneShot:
    """vnd_polar_moments_f32_dev with one pair on a contiguous (n, 2) float32 device array."""

    def __init__(self, torch, ctx, dev, n_max):
        from vndecorrelate_amd import _native
        self.native, self.torch, self.ctx = _native, torch, ctx
        self.ws = _native.polar_moments_workspace_bytes(n_max, 1)
        self.work = torch.empty(self.ws, dtype=torch.uint8, device=dev)
        self.out = torch.empty((8,), dtype=torch.float64, device=dev)

    def call(self, y, n, out=None):
        out = self.out if out is None else out
        self.native.polar_moments_device(self.ctx, y.data_ptr(), n, 1, out.data_ptr(), self.work.data_ptr(), self.ws,
                                         self.torch.cuda.current_stream().cuda_stream)
        return out


def touched(p, n):
    """Chunks a call of n frames at position p has frames in."""
    return (p + n - 1) // CHUNK - p // CHUNK + 1 if n else 0


def step(slots, frames, ragged, blocks, runs, wanted):
    import torch
    from vndecorrelate_amd import _native, analysis
    from vndecorrelate_amd.streaming import VOICE_START
    ctx = _native.default_context()
    dev = torch.device('cuda', ctx.device)
    gen = torch.Generator(device=dev).manual_seed(slots)
    x = torch.rand((slots, frames, 2), generator=gen, device=dev, dtype=torch.float32) * 2 - 1

    def make():
        pool = analysis.stereo_image_voice_pool(slots, max_frames_per_call=frames)
        pool.reset()
        return pool
    pool, captured = make(), make()
    plan = dict(f.split('=') for f in _native.describe_polar_voice_stream(slots, frames).split()[1:])
    per_slot = [1 if ragged and b % 2 else frames for b in range(slots)]
    counts = torch.tensor(per_slot, dtype=torch.int32, device=dev)
    flags = torch.zeros(slots, dtype=torch.int32, device=dev)
    out = (torch.empty((slots, 8), dtype=torch.float64, device=dev), torch.empty(slots, dtype=torch.int32, device=dev))
    out_g = (torch.empty_like(out[0]), torch.empty_like(out[1]))
    pool.process_dev(x, counts, flags, out=out)                            # loads the kernels before the capture
    pool.reset()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
    with torch.cuda.graph(graph, stream=side):
        captured.process_dev(x, counts, flags, out=out_g)
    torch.cuda.synchronize(dev)
    # the same first calls from a START in both forms, every slot against the one-shot call on its frames so far
    one = OneShot(torch, ctx, dev, max(3 * frames, slots * frames))
    want = torch.empty((8,), dtype=torch.float64, device=dev)
    for i in range(3):
        flags.fill_(VOICE_START if i == 0 else 0)
        pool.process_dev(x, counts, flags, out=out)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert out[1].tolist() == [1] * slots == out_g[1].tolist(), i
        assert torch.equal(out[0].view(torch.int64), out_g[0].view(torch.int64)), f'voice and graph differ in call {i}'
        for b in (range(slots) if i == 1 else range(0, slots, max(1, slots // 64))):
            sofar = x[b, :per_slot[b]].repeat(i + 1, 1).contiguous()
            one.call(sofar, len(sofar), want)
            assert torch.equal(out[0][b].view(torch.int64), want.view(torch.int64)), \
                f'slot {b} differs from vnd_polar_moments_f32_dev after call {i}'
    flags.fill_(0)
    # to the steady state of a long-lived voice: 256 completed chunks in every slot that pushes full blocks
    prefill = -(-256 * CHUNK // frames) + 1
    for _ in range(prefill):
        pool.process_dev(x, counts, flags, out=out)
        graph.replay()
    torch.cuda.synchronize(dev)
    before = 3 + prefill + blocks                                          # calls of a pool before its first timed call
    timed_calls = runs * blocks

    def lanes(n):
        return statistics.mean(min(256, (k * n) // CHUNK) for k in range(before, before + timed_calls))
    loaded = {n: lanes(n) for n in set(per_slot)}
    assert loaded[frames] == 256
    G = int(plan['groups'])
    busy = sum(statistics.mean(touched(k * n, n) for k in range(2, 2 + CHUNK)) for n in per_slot)
    block_bytes = 8 * sum(per_slot)
    open_chunk = sum(statistics.mean((k * n) % CHUNK for k in range(2, 2 + CHUNK)) for n in per_slot)       # frames
    # lane sums loaded (64 B a lane that has a completed chunk) and stored (64 B a completed chunk); the open chunk read
    # from the ring and its new frames written; partials written and read; moments, valid, position
    completed = sum(n / CHUNK for n in per_slot)
    state_bytes = 64 * sum(loaded[n] for n in per_slot) + 64 * completed + 8 * 2 * open_chunk + 2 * 64 * busy \
        + slots * (64 + 4 + 16)
    row = {'slots': slots, 'frames': frames, 'ragged': bool(ragged), 'blocks': blocks, 'runs': runs,
           'audio_ms_per_block': fig(1000.0 * frames / FS), 'groups_per_slot': G, 'workgroups': int(plan['nblocks']),
           'finish_workgroups': int(plan['finish_groups']), 'idle_workgroups': fig(slots * G - busy),
           'block_bytes': block_bytes, 'copy_bytes': 2 * block_bytes, 'state_bytes_per_call': int(state_bytes),
           'pool_state_bytes': int(plan['state_bytes']), 'prefill_calls': prefill,
           'lanes_loaded': [fig(loaded[n]) for n in sorted(loaded, reverse=True)]}
    flat = x.view(slots * frames, 2)
    rows = [x[b, :per_slot[b]] for b in range(slots)]                      # contiguous (n, 2) views

    def each():
        for b in range(slots):
            one.call(rows[b], per_slot[b])
    calls = {'voice': lambda: pool.process_dev(x, counts, flags, out=out), 'graph': graph.replay,
             'oneshot_flat': lambda: one.call(flat, sum(per_slot)), 'oneshot_each': each}
    names = [n for n in FORMS if n in wanted]
    reps = {n: (max(1, blocks // 10) if n == 'oneshot_each' else blocks) for n in names}

    def run(name):
        fn = calls[name]
        for _ in range(reps[name]):
            fn()
    times = {n: [] for n in names}
    for n in names:
        run(n)                                                             # warm
    torch.cuda.synchronize(dev)
    for r in range(runs):
        for n in names[r % len(names):] + names[:r % len(names)]:
            times[n].append(timed(torch, lambda: run(n)) / reps[n])
    if 'voice' in names and 'graph' in names:                              # both made the same calls: the same rows
        torch.cuda.synchronize(dev)
        assert out[1].tolist() == [1] * slots == out_g[1].tolist()
        assert torch.equal(out[0].view(torch.int64), out_g[0].view(torch.int64)), 'voice and graph differ after the timed runs'
    assert captured._state is not None                                     # the graph holds pointers into that pool's state
    for n in names:
        row[n + '_ms'] = fig(statistics.median(times[n]))
        row[n + '_min_ms'] = fig(min(times[n]))
    for n in ('voice', 'graph'):
        if n in times:
            row[f'{n}_GBps_block'] = fig(block_bytes / (statistics.median(times[n]) * 1e6))
            row[f'{n}_GBps_all'] = fig((block_bytes + state_bytes) / (statistics.median(times[n]) * 1e6))
            for base in ('oneshot_flat', 'oneshot_each'):
                if base in times:
                    row[f'{n}_over_{base}'] = fig(statistics.median(times[n]) / statistics.median(times[base]))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--shapes', default='512x480,2048x480,2048x4800,2048x480r')
    ap.add_argument('--blocks', type=int, default=50)
    ap.add_argument('--forms', default=','.join(FORMS))
    ap.add_argument('--step', default=None, help='SLOTSxFRAMES[r]: run one shape in this process (r: every second slot pushes one frame)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    wanted = tuple(args.forms.split(','))
    if args.step:
        slots, frames = (int(v) for v in args.step.rstrip('r').split('x'))
        print(json.dumps(step(slots, frames, args.step.endswith('r'), args.blocks, args.runs, wanted)))
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
    line = json.dumps({'tool': 'polar_voice_pool_rate', 'rows': rows})
    print(line)
    if args.out:
        pathlib.Path(args.out).write_text(line + '\n')


if __name__ == '__main__':
    main()
