"""The level-envelope voice pool (vnd_polar_level_voice_stream_push_f32_dev, ..._levels_f32_dev) in steady state, against the
one-shot entry it shares its select with: vnd_polar_level_f32_dev on a (slots, W, 2) pool with the same radius_scale, in the
same run.  Minus its stage kernel, that one-shot is what the levels entry should cost.  Prints one JSON line; nothing here is
asserted but that the pool and the one-shot entry leave the same levels and slice counts.

Cases, float32 frames drawn on the device from a seed (Gaussian, sigma 0.25), every slot live, window_frames W = 48 000,
blocks of M = 480 frames, 360 slices, percentiles (95, 50):
- ``256``: 256 slots;
- ``2048``: 2048 slots.
Forms: ``push`` (one block into the rings), ``levels`` (the envelope of every slot from the state alone), ``push_levels``
(both, as process_dev enqueues them) and ``one_shot``.  The rings are filled first (W / M pushes of the same block, so the
window is that block W / M times over and the one-shot's pool is its tiling).  Every time is between two device events around
``reps`` back-to-back calls on the current stream, after a warm-up; the forms alternate in a rotating order; median and
minimum of --runs, per call.

Each case is a child process under its own ``timeout``; the tool stops at the first case that fails.

    python tools/level_voice_pool_rate.py [--runs 5] [--cases 256,2048] [--out profiles/level_voice_pool_rate.json]
"""
import argparse
import json
import pathlib
import statistics
import subprocess
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

STEP_SECONDS = 300
CASES = ('256', '2048')
WINDOW, BLOCK, BINS, PERCENTILES = 48000, 480, 360, (95.0, 50.0)
REPS = {'push': 50, 'levels': 5, 'push_levels': 5, 'one_shot': 5}


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
    """One pool at the C binding, every slot live: counts = M and no flag after a first call with START."""

    def __init__(self, slots, seed):
        import torch
        from vndecorrelate_amd import _native, vectorscope
        self.torch, self.native = torch, _native
        self.ctx = _native.default_context()
        self.dev = torch.device('cuda', self.ctx.device)
        self.slots = S = slots
        gen = torch.Generator(device=self.dev).manual_seed(seed)
        self.x = torch.randn((S, BLOCK, 2), generator=gen, device=self.dev, dtype=torch.float32) * 0.25
        self.edges = torch.from_numpy(vectorscope.level_edges(BINS)[0]).to(self.dev)
        self.counts = torch.full((S,), BLOCK, dtype=torch.int32, device=self.dev)
        self.idle = torch.zeros(S, dtype=torch.int32, device=self.dev)
        self.start = torch.ones(S, dtype=torch.int32, device=self.dev)
        self.valid = torch.empty(S, dtype=torch.int32, device=self.dev)
        self.need = _native.level_voice_stream_state_bytes(S, BLOCK, WINDOW)
        self.state = torch.empty(self.need, dtype=torch.uint8, device=self.dev)
        self.levels = torch.zeros((S, len(PERCENTILES), BINS), dtype=torch.float32, device=self.dev)
        self.bin_counts = torch.zeros((S, BINS), dtype=torch.int32, device=self.dev)
        self.work_bytes = _native.level_voice_stream_work_bytes(S, WINDOW, BINS, len(PERCENTILES))
        self.work = torch.empty((self.work_bytes + 7) // 8, dtype=torch.int64, device=self.dev)
        _native.level_voice_stream_reset_device(self.ctx, self.state.data_ptr(), self.need, S, BLOCK, WINDOW, stream=self.stream())
        self.push(self.start)
        for _ in range(WINDOW // BLOCK - 1):
            self.push()
        # the one-shot's side: the window as a pool of its own, and its work memory
        self.pool = self.x.repeat(1, WINDOW // BLOCK, 1).contiguous()
        self.one_levels, self.one_counts = torch.zeros_like(self.levels), torch.zeros_like(self.bin_counts)
        self.one_work_bytes = _native.polar_level_work_bytes(S, WINDOW, BINS, len(PERCENTILES))
        self.one_work = torch.empty((self.one_work_bytes + 7) // 8, dtype=torch.int64, device=self.dev)

    def stream(self):
        return self.torch.cuda.current_stream().cuda_stream

    def push(self, flags=None):
        x = self.x
        self.native.level_voice_stream_push_device(
            self.ctx, self.state.data_ptr(), self.need, BLOCK, WINDOW, x.data_ptr(), x.data_ptr() + 4, 2 * BLOCK, 2,
            self.counts.data_ptr(), (self.idle if flags is None else flags).data_ptr(), self.edges.data_ptr(), BINS,
            self.valid.data_ptr(), self.slots, radius_scale=1.0, stream=self.stream())

    def read(self):
        self.native.level_voice_stream_levels_device(
            self.ctx, self.state.data_ptr(), self.need, BLOCK, WINDOW, BINS, PERCENTILES, self.levels.data_ptr(),
            self.bin_counts.data_ptr(), self.slots, work_ptr=self.work.data_ptr(), work_bytes=self.work_bytes,
            stream=self.stream())

    def push_read(self):
        self.push()
        self.read()

    def one_shot(self):
        p = self.pool
        self.native.polar_level_device(
            self.ctx, p.data_ptr(), p.data_ptr() + 4, self.slots, WINDOW, 2 * WINDOW, 2, self.edges.data_ptr(), BINS,
            PERCENTILES, self.one_levels.data_ptr(), self.one_counts.data_ptr(), work_ptr=self.one_work.data_ptr(),
            work_bytes=self.one_work_bytes, radius_scale=1.0, stream=self.stream())


def measure(torch, forms, runs):
    """forms: {name: callable}.  Median and minimum per call, the forms alternating in a rotating order."""
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
    return {name: (statistics.median(t), min(t)) for name, t in times.items()}


def step(case, runs):
    slots = int(case)
    bench = Bench(slots, seed=1)
    torch = bench.torch
    bench.read()
    bench.one_shot()
    torch.cuda.synchronize()
    assert torch.equal(bench.levels, bench.one_levels), 'the pool and the one-shot entry differ in a level'
    assert torch.equal(bench.bin_counts, bench.one_counts), 'the pool and the one-shot entry differ in a slice count'
    assert int(bench.bin_counts.to(torch.int64).sum()) == slots * WINDOW
    got = measure(torch, {'push': bench.push, 'levels': bench.read, 'push_levels': bench.push_read, 'one_shot': bench.one_shot},
                  runs)
    row = {'case': case, 'slots': slots, 'window_frames': WINDOW, 'max_frames_per_call': BLOCK, 'num_bins': BINS,
           'percentiles': list(PERCENTILES), 'reps': REPS, 'runs': runs, 'state_bytes': bench.need, 'work_bytes': bench.work_bytes,
           'one_shot_work_bytes': bench.one_work_bytes}
    for form, (median, least) in got.items():
        row[form] = {'ms': fig(median), 'min_ms': fig(least)}
    row['levels_over_one_shot'] = fig(got['levels'][0] / got['one_shot'][0])
    row['push_levels_over_one_shot'] = fig(got['push_levels'][0] / got['one_shot'][0])
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
    line = json.dumps({'tool': 'level_voice_pool_rate', 'rows': rows})
    print(line)
    if args.out:
        pathlib.Path(args.out).write_text(line + '\n')


if __name__ == '__main__':
    main()
