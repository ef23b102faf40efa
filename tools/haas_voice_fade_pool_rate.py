"""The crossfading Haas voice pool on resident blocks (vnd_haas_voice_fade_stream_f64_dev,
streaming.HaasFadeVoicePool.process_dev) against the Haas voice pool beside it (vnd_haas_voice_stream_f64_dev).  Prints one
JSON line.

The shapes, the bank and the timing are tools/haas_voice_pool_rate.py's: pools of S slots of 44.1 kHz stereo noise, every
slot active and every block full (M frames), 64 distinct delays up to 30 ms, slot b delayed by delay b % 64 (Haas LR,
delayed channel 1); S x M = 512 x 480, 2048 x 480 and 2048 x 4800.
- ``voice``: ``HaasVoicePool.process_dev``, whose code the crossfading pool does not touch.
- ``fade_idle``: ``HaasFadeVoicePool.process_dev`` with nobody switching: the steady state of a live pool.
- ``fade_all``: the same with every slot inside a fade on every call: fade_frames = 4 M, and every call carries
  VND_VOICE_SWITCH for every slot - ignored while the fade runs, accepted by the call after its last frame - so every lane
  of every call reads its delayed column twice and blends.
Every time is between two device events on the current stream around --blocks back-to-back steady-state calls (the
Python calls inside); the forms alternate in a rotating order, median, minimum and maximum of --runs, reported per block.
Before any timing ``voice`` and ``fade_idle`` run the same first blocks from position 0 - START, two plain blocks, END -
and are checked byte-equal, call by call.

EXPECTED, written before the first run: the kernel is memory-bound and an idle lane adds the record's 16 bytes per
workgroup and two compares to haas_voice_stream_kernel's work, so ``fade_idle`` over ``voice`` should lie within the
spread of the repeats around 1.0 - at most a few percent above, as the velvet pool's 1.03; ``fade_all``
reads one more input column per lane against two reads and one 16-byte store, so well below 1.5.

Each shape is a child process under its own ``timeout``; the tool stops at the first shape that fails.

    python tools/haas_voice_fade_pool_rate.py [--runs 5] [--shapes 512x480,2048x480,2048x4800] [--blocks 50] [--out FILE]
"""
import argparse
import json
import pathlib
import statistics
import subprocess
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

from haas_voice_pool_rate import DELAYS, ENTRIES, FS, HAAS, STEP_SECONDS, fig, timed  # noqa: E402

FORMS = ('voice', 'fade_idle', 'fade_all')
FADE_CALLS = 4                         # fade_frames = FADE_CALLS x M


def step(slots, frames, blocks, runs, wanted):
    import torch
    import vndecorrelate_amd.decorrelation as dec
    from vndecorrelate_amd import _native
    from vndecorrelate_amd.streaming import VOICE_END, VOICE_START, VOICE_SWITCH
    ctx = _native.default_context()
    dev = torch.device('cuda', ctx.device)
    bank = [dec.HaasEffect(sample_rate_hz=FS, delay_time_seconds=float(d) / FS, **HAAS) for d in DELAYS]
    gen = torch.Generator(device=dev).manual_seed(slots)
    x = torch.rand((slots, frames, 2), generator=gen, device=dev, dtype=torch.float32) * 2 - 1
    F = FADE_CALLS * frames

    def make(fade_frames):
        if fade_frames is None:
            pool = dec.decorrelate_voice_pool(bank, slots=slots, in_channels=2, max_frames_per_call=frames)
        else:
            pool = dec.decorrelate_fade_voice_pool(bank, slots=slots, in_channels=2, max_frames_per_call=frames,
                                                   fade_frames=fade_frames)
        pool.reset()
        return pool
    pools = {'voice': make(None), 'fade_idle': make(F), 'fade_all': make(F)}
    D = pools['voice'].max_delay
    entry = np.arange(slots) % ENTRIES
    delays = torch.from_numpy(DELAYS[entry]).to(dev)
    other = torch.from_numpy(DELAYS[(entry + 1) % ENTRIES]).to(dev)
    counts = torch.full((slots,), frames, dtype=torch.int32, device=dev)
    flags = torch.zeros(slots, dtype=torch.int32, device=dev)
    switch = torch.full((slots,), VOICE_SWITCH, dtype=torch.int32, device=dev)
    outs = {n: (torch.empty((slots, frames + D, 2), dtype=torch.float64, device=dev),
                torch.empty(slots, dtype=torch.int32, device=dev)) for n in FORMS}

    # the same first calls from position 0 in voice and fade_idle, byte-equal call by call: START, two plain blocks, END
    for i, f in enumerate((VOICE_START, 0, 0, VOICE_END)):
        flags.fill_(f)
        for n in ('voice', 'fade_idle'):
            outs[n][0].view(torch.int64).fill_(-1)                         # (rows have their own lengths at END)
            pools[n].process_dev(x, counts, flags, delays, out=outs[n])
        torch.cuda.synchronize(dev)
        assert outs['voice'][1].tolist() == outs['fade_idle'][1].tolist() == \
            (frames + (DELAYS[entry] if f == VOICE_END else 0 * entry)).tolist(), i
        assert torch.equal(outs['voice'][0].view(torch.int64), outs['fade_idle'][0].view(torch.int64)), \
            f'fade_idle differs from the Haas voice pool in call {i}'
        assert not pools['fade_idle'].fade_left_dev.any()
    # into the steady state: every call returns `frames` frames per slot; fade_all's slots are inside a fade from call 2 on
    flags.fill_(VOICE_START)
    for n in FORMS:
        pools[n].process_dev(x, counts, flags, delays, out=outs[n])
    flags.fill_(0)
    for _ in range(D // frames + 2):
        for n in ('voice', 'fade_idle'):
            pools[n].process_dev(x, counts, flags, delays, out=outs[n])
        pools['fade_all'].process_dev(x, counts, switch, other, out=outs['fade_all'])
    torch.cuda.synchronize(dev)
    left = []
    for _ in range(2 * FADE_CALLS):                                        # a fade is followed by the next without a gap:
        pools['fade_all'].process_dev(x, counts, switch, other, out=outs['fade_all'])
        seen = set(pools['fade_all'].fade_left_dev.tolist())               # after a call F - k M frames of it are left, k = 1 .. 4
        assert len(seen) == 1 and outs['fade_all'][1].tolist() == [frames] * slots, seen
        left.append(seen.pop())
    assert sorted(left) == sorted(2 * [k * frames for k in range(FADE_CALLS)]), left

    def runner(name, f, d):
        def run():
            for _ in range(blocks):
                pools[name].process_dev(x, counts, f, d, out=outs[name])
        return run
    forms = {'voice': runner('voice', flags, delays), 'fade_idle': runner('fade_idle', flags, delays),
             'fade_all': runner('fade_all', switch, other)}
    names = [n for n in FORMS if n in wanted]
    times = {n: [] for n in names}
    for n in names:
        forms[n]()                                                         # warm
    torch.cuda.synchronize(dev)
    for r in range(runs):
        for n in names[r % len(names):] + names[:r % len(names)]:
            times[n].append(timed(torch, forms[n]) / blocks)
    row = {'slots': slots, 'frames': frames, 'max_delay': D, 'fade_frames': F, 'blocks': blocks, 'runs': runs,
           'audio_ms_per_block': fig(1000.0 * frames / FS)}
    for n in names:
        row[n + '_ms'] = fig(statistics.median(times[n]))
        row[n + '_min_ms'] = fig(min(times[n]))
        row[n + '_max_ms'] = fig(max(times[n]))
    for n in ('fade_idle', 'fade_all'):
        if n in times and 'voice' in times:
            row[n + '_over_voice'] = fig(statistics.median(times[n]) / statistics.median(times['voice']))
            row[n + '_over_voice_min_max'] = [fig(min(times[n]) / max(times['voice'])), fig(max(times[n]) / min(times['voice']))]
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
    line = json.dumps({'tool': 'haas_voice_fade_pool_rate', 'rows': rows})
    print(line)
    if args.out:
        pathlib.Path(args.out).write_text(line + '\n')


if __name__ == '__main__':
    main()
