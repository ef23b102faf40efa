"""The Haas-delay scan voice pool (vnd_haas_scan_voice_stream_push_f32_dev, ..._pairs_f64_dev) in steady state, against what
a caller had to do without it: gather every voice's window out of a ring into a contiguous (slots, W, 2) tensor with torch,
then call the one-shot vnd_haas_pairs_f64_dev on it - in the same run.  Prints one JSON line; nothing here is asserted but
that the two routes leave the same moments, byte for byte.

Cases, float32 stereo frames drawn on the device from a seed (Gaussian, sigma 0.25, the right channel partly the left's),
every slot live with a full window, window_frames W = 48 000, blocks of M = 480 frames, the 400 delays of
``optimize_haas_delay``'s default grid up to 20 ms at 48 kHz (LR, delayed channel 0): ``16``, ``64`` and ``256`` slots.
Forms: ``push`` (one block into the rings), ``scan`` (scan_dev: every slot against the grid, from the state alone),
``gather`` (torch: the windows in time order out of the same rings, index arithmetic included), ``one_shot`` (the pairs entry
on the gathered tensor) and ``optimize`` (one HaasScanVoicePool.optimize call, host clock, grid and refinement).  The rings are
filled first (W / M + 3 pushes of fresh blocks, so the windows wrap).  Every device time is between two device events around
``reps`` back-to-back calls on the current stream, after a warm-up; the forms alternate in a rotating order; median, minimum
and maximum of --runs, per call.

``--embed name=FILE`` (repeatable) copies the JSON line of another tool's run into the result under ``one_shot_entry`` - the
one-shot scan's own times (tools/haas_scan_rate.py, tools/haas_search_rate.py) before and after the scan kernel was given its
frame loader.

Each case is a child process under its own ``timeout``; the tool stops at the first case that fails.

    python tools/haas_scan_voice_pool_rate.py [--runs 3] [--cases 16,64,256] [--out profiles/haas_scan_voice_pool_rate.json]
"""
import argparse
import contextlib
import io
import json
import pathlib
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

STEP_SECONDS = 300
CASES = ('16', '64', '256')
FS, WINDOW, BLOCK, GRID, MAX_DELAY_SECONDS = 48000, 48000, 480, 400, 0.02
REPS = {'push': 50, 'scan': 3, 'gather': 10, 'one_shot': 3}


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


class Bench:
    """One pool, every slot live: counts = M and no flag after a first call with START; and today's route beside it."""

    def __init__(self, slots, seed):
        import torch
        from vndecorrelate_amd import _native, optimization
        self.torch, self.native = torch, _native
        self.ctx = _native.default_context()
        self.dev = torch.device('cuda', self.ctx.device)
        self.slots = S = slots
        self.pool = optimization.haas_scan_voice_pool(S, in_channels=2, max_frames_per_call=BLOCK, window_frames=WINDOW,
                                                      max_delay_seconds=MAX_DELAY_SECONDS, sample_rate_hz=FS)
        self.pool.reset()
        gen = torch.Generator(device=self.dev).manual_seed(seed)
        self.counts = torch.full((S,), BLOCK, dtype=torch.int32, device=self.dev)
        self.idle = torch.zeros(S, dtype=torch.int32, device=self.dev)
        for call in range(WINDOW // BLOCK + 3):
            left = torch.randn((S, BLOCK, 1), generator=gen, device=self.dev, dtype=torch.float32) * 0.25
            other = torch.randn((S, BLOCK, 1), generator=gen, device=self.dev, dtype=torch.float32) * 0.25
            self.x = torch.cat([left, 0.6 * left + 0.4 * other], dim=2).contiguous()
            self.pool.process_dev(self.x, self.counts, torch.ones_like(self.idle) if call == 0 else self.idle)
        delays = np.unique(optimization.haas_delays(np.linspace(0.0, MAX_DELAY_SECONDS, GRID), FS)).astype(np.int32)
        self.delays = torch.from_numpy(delays).to(self.dev)
        self.D = D = int(delays.size)
        self.frame_pairs = int(np.sum(WINDOW + delays.astype(np.int64))) * S
        # today's route: the caller's own ring (here the pool's, so both routes read the same frames), its gather, the pairs
        state = self.pool._state[0]
        fill_at = (8 * S + 15) & ~15
        head_at = fill_at + ((4 * S + 15) & ~15)
        ring_at = head_at + ((4 * S + 15) & ~15)
        self.ring = state[ring_at:ring_at + S * WINDOW * 8].view(torch.float32).view(S, WINDOW, 2)
        self.head = state[head_at:head_at + 4 * S].view(torch.int32)
        self.frames = torch.arange(WINDOW, dtype=torch.int64, device=self.dev)
        self.signals = torch.arange(S, dtype=torch.int32, device=self.dev).repeat_interleave(D)
        self.tiled = self.delays.repeat(S)
        self.moments = torch.empty((S * D, _native.MOMENTS), dtype=torch.float64, device=self.dev)
        self.ws_bytes = _native.haas_pairs_workspace_bytes(WINDOW, S * D, int(delays.max()))
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.dev)
        self.gather()

    def push(self):
        self.pool.process_dev(self.x, self.counts, self.idle)

    def scan(self):
        return self.pool.scan_dev(self.delays)

    def gather(self):
        entry = (self.head.to(self.torch.int64)[:, None] + self.frames[None, :]) % WINDOW          # full windows: first = head
        self.windows = self.torch.take_along_dim(self.ring, entry[:, :, None].expand(self.slots, WINDOW, 2), dim=1)

    def one_shot(self):
        torch = self.torch
        self.native.haas_pairs_device(self.ctx, self.windows.data_ptr(), self.slots, WINDOW, 2, self.signals.data_ptr(),
                                      self.tiled.data_ptr(), self.slots * self.D, self.moments.data_ptr(), delayed_channel=0,
                                      ms_mode=False, width=None, workspace_ptr=self.ws.data_ptr(), workspace_bytes=self.ws_bytes,
                                      stream=torch.cuda.current_stream().cuda_stream)


def measure(torch, forms, runs):
    """forms: {name: callable}.  The per-call times of every form, the forms alternating in a rotating order."""
    names = list(forms)

    def run(name):
        for _ in range(REPS[name]):
            forms[name]()
    for name in names:
        run(name)
    torch.cuda.synchronize()
    times = {name: [] for name in names}
    for r in range(runs):
        for name in names[r % len(names):] + names[:r % len(names)]:
            times[name].append(timed(torch, lambda: run(name)) / REPS[name])
    return times


def step(case, runs):
    slots = int(case)
    bench = Bench(slots, seed=1)
    torch = bench.torch
    got = bench.scan()
    bench.gather()
    bench.one_shot()
    torch.cuda.synchronize()
    assert torch.equal(got.view(-1, 8).view(torch.int64), bench.moments.view(torch.int64)), 'the two routes differ in a moment'
    # the gather moves nothing of the state, the scan neither: push last in every rotation would change the windows, so the
    # pushes are timed on their own first and the three read-only forms alternate afterwards
    times = measure(torch, {'push': bench.push}, runs)
    times.update(measure(torch, {'scan': bench.scan, 'gather': bench.gather, 'one_shot': bench.one_shot}, runs))
    wall = []
    with contextlib.redirect_stdout(io.StringIO()):
        bench.pool.optimize()                                          # warm-up
        for _ in range(runs):
            torch.cuda.synchronize()
            t = time.perf_counter()
            taus = bench.pool.optimize()
            wall.append((time.perf_counter() - t) * 1e3)
    stats = bench.pool.last_search
    row = {'case': case, 'slots': slots, 'window_frames': WINDOW, 'max_frames_per_call': BLOCK, 'delays': bench.D,
           'max_delay': bench.pool.max_delay, 'pairs': slots * bench.D, 'reps': REPS, 'runs': runs,
           'state_bytes': bench.pool._state[1], 'workspace_bytes': slots * bench.D * bench.pool.chunks_per_pair * 64,
           'one_shot_workspace_bytes': bench.ws_bytes}
    for form, t in times.items():
        row[form] = {'ms': fig(statistics.median(t)), 'min_ms': fig(min(t)), 'max_ms': fig(max(t))}
    row['scan']['frame_pairs_per_s'] = fig(bench.frame_pairs / (statistics.median(times['scan']) * 1e-3))
    row['one_shot']['frame_pairs_per_s'] = fig(bench.frame_pairs / (statistics.median(times['one_shot']) * 1e-3))
    row['optimize'] = {'ms': fig(statistics.median(wall)), 'min_ms': fig(min(wall)), 'max_ms': fig(max(wall)),
                       'rounds': stats.rounds, 'grid_pairs': stats.grid_pairs, 'pairs_per_round_max': max(stats.pairs_per_round),
                       'evaluations_per_slot': float(stats.evaluations.mean()), 'distinct_taus': int(np.unique(taus).size)}
    row['scan_over_one_shot'] = fig(statistics.median(times['scan']) / statistics.median(times['one_shot']))
    row['scan_over_gather_plus_one_shot'] = fig(statistics.median(times['scan'])
                                                / (statistics.median(times['gather']) + statistics.median(times['one_shot'])))
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--cases', default=','.join(CASES))
    ap.add_argument('--step', default=None, help='run one case in this process')
    ap.add_argument('--embed', action='append', default=[], metavar='NAME=FILE')
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
    result = {'tool': 'haas_scan_voice_pool_rate', 'rows': rows}
    if args.embed:
        result['one_shot_entry'] = {}
        for item in args.embed:
            name, _, path = item.partition('=')
            result['one_shot_entry'][name] = json.loads(pathlib.Path(path).read_text().strip().splitlines()[-1])
    line = json.dumps(result)
    print(line)
    if args.out:
        pathlib.Path(args.out).write_text(line + '\n')


if __name__ == '__main__':
    main()
