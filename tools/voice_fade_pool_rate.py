"""The crossfading voice pool on resident blocks (vnd_voice_fade_stream_f32_dev, streaming.FadeVoicePool.process_dev)
against the voice pool beside it (vnd_voice_stream_f32_dev), exact mode.  Prints one JSON line.

The shapes, the bank and the timing are tools/voice_pool_rate.py's: pools of S slots of 44.1 kHz stereo noise, every slot
active and every block full (M frames), a kappa per slot; S x M = 512 x 480, 2048 x 480 and 2048 x 4800.
- ``voice``: ``VoicePool.process_dev``, whose code the crossfading pool does not touch.
- ``fade_idle``: ``FadeVoicePool.process_dev`` with nobody switching: the steady state of a live pool.
- ``fade_all``: the same with every slot inside a fade on every call: fade_frames = 4 M, and every call carries
  VND_VOICE_SWITCH for every slot - ignored while the fade runs, accepted by the call after its last frame - so every tile
  of every call forms its frames twice and blends them.
Every time is between two device events on the current stream around --blocks back-to-back steady-state calls (the
Python calls inside); the forms alternate in a rotating order, median, minimum and maximum of --runs, reported per block.
Before any timing ``voice`` and ``fade_idle`` run the same first blocks from position 0 - START, two plain blocks, END -
and are checked byte-equal, call by call.

Each shape is a child process under its own ``timeout``; the tool stops at the first shape that fails.

    python tools/voice_fade_pool_rate.py [--runs 5] [--shapes 512x480,2048x480,2048x4800] [--blocks 50] [--out FILE]
"""
import argparse
import json
import pathlib
import statistics
import subprocess
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

from voice_pool_rate import FS, STEP_SECONDS, TABLES, VELVET, fig, timed  # noqa: E402

FORMS = ('voice', 'fade_idle', 'fade_all')
FADE_CALLS = 4                         # fade_frames = FADE_CALLS x M


def step(slots, frames, blocks, runs, wanted):
    import torch
    import vndecorrelate_amd.decorrelation as dec
    from vndecorrelate_amd import _native
    from vndecorrelate_amd.streaming import VOICE_END, VOICE_START, VOICE_SWITCH
    ctx = _native.default_context()
    dev = torch.device('cuda', ctx.device)
    bank = [dec.VelvetNoise(log_distribution_strength=k, **VELVET) for k in np.linspace(0.0, 1.0, TABLES)]
    gen = torch.Generator(device=dev).manual_seed(slots)
    x = torch.rand((slots, frames, 2), generator=gen, device=dev, dtype=torch.float32) * 2 - 1
    F = FADE_CALLS * frames

    def make(fade_frames):
        pool = dec.decorrelate_voice_pool(bank, slots=slots, in_channels=2, max_frames_per_call=frames, fade_frames=fade_frames)
        pool.reset()
        return pool
    pools = {'voice': make(None), 'fade_idle': make(F), 'fade_all': make(F)}
    H = pools['voice'].latency_frames
    entry = np.arange(slots) % TABLES
    tables = torch.from_numpy(pools['voice'].bank_tables[entry].astype(np.int32)).to(dev)
    other = torch.from_numpy(pools['voice'].bank_tables[(entry + 1) % TABLES].astype(np.int32)).to(dev)
    counts = torch.full((slots,), frames, dtype=torch.int32, device=dev)
    flags = torch.zeros(slots, dtype=torch.int32, device=dev)
    switch = torch.full((slots,), VOICE_SWITCH, dtype=torch.int32, device=dev)
    outs = {n: (torch.empty((slots, frames + H, 2), dtype=torch.float32, device=dev),
                torch.empty(slots, dtype=torch.int32, device=dev)) for n in FORMS}

    # the same first calls from position 0 in voice and fade_idle, byte-equal call by call: START, two plain blocks, END
    for i, f in enumerate((VOICE_START, 0, 0, VOICE_END)):
        flags.fill_(f)
        for n in ('voice', 'fade_idle'):
            pools[n].process_dev(x, counts, flags, tables, out=outs[n])
        torch.cuda.synchronize(dev)
        n_out = outs['voice'][1].tolist()
        assert n_out == outs['fade_idle'][1].tolist() and len(set(n_out)) == 1, (i, n_out)
        assert torch.equal(outs['voice'][0][:, :n_out[0]].view(torch.int32), outs['fade_idle'][0][:, :n_out[0]].view(torch.int32)), \
            f'fade_idle differs from the voice pool in call {i}'
        assert not pools['fade_idle'].fade_left_dev.any()
    # into the steady state: every call returns `frames` frames per slot; fade_all's slots are inside a fade from here on
    flags.fill_(VOICE_START)
    pools['fade_all'].process_dev(x, counts, flags, tables, out=outs['fade_all'])
    flags.fill_(0)
    for _ in range(H // frames + 2):
        for n in ('voice', 'fade_idle'):
            pools[n].process_dev(x, counts, flags, tables, out=outs[n])
        pools['fade_all'].process_dev(x, counts, switch, other, out=outs['fade_all'])
    for _ in range(2 * FADE_CALLS):                                        # past the first fade, which began below frame H
        pools['fade_all'].process_dev(x, counts, switch, other, out=outs['fade_all'])
    torch.cuda.synchronize(dev)
    left = []
    for _ in range(2 * FADE_CALLS):                                        # a fade is followed by the next without a gap:
        pools['fade_all'].process_dev(x, counts, switch, other, out=outs['fade_all'])
        seen = set(pools['fade_all'].fade_left_dev.tolist())               # after a call F - k M frames of it are left, k = 1 .. 4
        assert len(seen) == 1 and outs['fade_all'][1].tolist() == [frames] * slots, seen
        left.append(seen.pop())
    assert sorted(left) == sorted(2 * [k * frames for k in range(FADE_CALLS)]), left

    def runner(name, f, t):
        def run():
            for _ in range(blocks):
                pools[name].process_dev(x, counts, f, t, out=outs[name])
        return run
    forms = {'voice': runner('voice', flags, tables), 'fade_idle': runner('fade_idle', flags, tables),
             'fade_all': runner('fade_all', switch, other)}
    names = [n for n in FORMS if n in wanted]
    times = {n: [] for n in names}
    for n in names:
        forms[n]()                                                         # warm
    torch.cuda.synchronize(dev)
    for r in range(runs):
        for n in names[r % len(names):] + names[:r % len(names)]:
            times[n].append(timed(torch, forms[n]) / blocks)
    row = {'slots': slots, 'frames': frames, 'latency_frames': H, 'fade_frames': F, 'blocks': blocks, 'runs': runs,
           'audio_ms_per_block': fig(1000.0 * frames / FS)}
    for n in names:
        row[n + '_ms'] = fig(statistics.median(times[n]))
        row[n + '_min_ms'] = fig(min(times[n]))
        row[n + '_max_ms'] = fig(max(times[n]))
    for n in ('fade_idle', 'fade_all'):
        if n in times and 'voice' in times:
            row[n + '_over_voice'] = fig(statistics.median(times[n]) / statistics.median(times['voice']))
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
    line = json.dumps({'tool': 'voice_fade_pool_rate', 'rows': rows})
    print(line)
    if args.out:
        pathlib.Path(args.out).write_text(line + '\n')


if __name__ == '__main__':
    main()
