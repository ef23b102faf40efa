"""The count-grid voice pool (vnd_polar_hist_voice_stream_f32_dev, vnd_lissajous_hist_voice_stream_f32_dev) in steady state,
against the lockstep entry it grew out of: vnd_polar_hist_f32_dev / vnd_lissajous_hist_f32_dev with accumulate = 1, n_each_dev
and (polar) radius_scale = 1 at the same shape, in the same run.  Prints one JSON line; nothing here is asserted but that the
whole-voice pool and the lockstep entry leave the same grid.

Cases, float32 frames drawn on the device from a seed (Gaussian, sigma 0.25), every slot live and pushing a full block:
- ``block``: 2048 slots x 480 frames on the default 240 x 150 polar grid;
- ``long``: 256 slots x 4800 frames on the same grid;
- ``lissajous``: 2048 slots x 480 frames on the 512 x 512 L/R grid, the window form alone against the lockstep entry.
Forms: ``whole`` (window_frames 0), ``window`` (window_frames 48 000, warmed up past the window, so that every frame takes a
count out as well) and ``lockstep``.  Every time is between two device events around ``reps`` back-to-back calls on the
current stream, after the warm-up; the forms alternate in a rotating order; median and minimum of --runs, per call.

Each case is a child process under its own ``timeout``; the tool stops at the first case that fails.

    python tools/scope_voice_pool_rate.py [--runs 5] [--cases block,long,lissajous] [--out profiles/scope_voice_pool_rate.json]
"""
import argparse
import json
import pathlib
import statistics
import subprocess
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

STEP_SECONDS = 300
CASES = ('block', 'long', 'lissajous')
WINDOW = 48000
SHAPES = {'block': (2048, 480, True, 50), 'long': (256, 4800, True, 20), 'lissajous': (2048, 480, False, 20)}


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


class Pool:
    """One voice pool at the C binding, every slot live: counts = M and no flag after a first call with START."""

    def __init__(self, bench, window):
        torch, native = bench.torch, bench.native
        S, M = bench.slots, bench.frames
        self.bench, self.window = bench, window
        need = native.scope_voice_stream_state_bytes(S, M, window)
        self.state = torch.empty(max(need, 16), dtype=torch.uint8, device=bench.dev)
        self.need = need
        self.grid = torch.zeros((S,) + bench.bins, dtype=torch.int32, device=bench.dev)
        self.valid = torch.empty(S, dtype=torch.int32, device=bench.dev)
        native.scope_voice_stream_reset_device(bench.ctx, self.state.data_ptr(), need, S, M, window,
                                               stream=torch.cuda.current_stream().cuda_stream)
        self.call(bench.start)

    def call(self, flags=None):
        b = self.bench
        x = b.x
        b.native.scope_voice_stream_device(
            b.ctx, self.state.data_ptr(), self.need, b.frames, self.window, x.data_ptr(), x.data_ptr() + 4, 2 * b.frames, 2,
            b.counts.data_ptr(), (b.idle if flags is None else flags).data_ptr(), b.e0.data_ptr(), b.bins[0], b.e1.data_ptr(),
            b.bins[1], self.grid.data_ptr(), self.valid.data_ptr(), b.slots, polar=b.polar, radius_scale=1.0,
            stream=b.torch.cuda.current_stream().cuda_stream)


class Bench:
    def __init__(self, slots, frames, polar, seed):
        import torch
        from vndecorrelate_amd import _native, vectorscope
        self.torch, self.native = torch, _native
        self.ctx = _native.default_context()
        self.dev = torch.device('cuda', self.ctx.device)
        self.slots, self.frames, self.polar = slots, frames, polar
        gen = torch.Generator(device=self.dev).manual_seed(seed)
        self.x = torch.randn((slots, frames, 2), generator=gen, device=self.dev, dtype=torch.float32) * 0.25
        e0, e1 = vectorscope.polar_edges() if polar else vectorscope.lissajous_edges()
        self.e0, self.e1 = torch.from_numpy(e0).to(self.dev), torch.from_numpy(e1).to(self.dev)
        self.bins = (len(e0) - 1, len(e1) - 1)
        self.counts = torch.full((slots,), frames, dtype=torch.int32, device=self.dev)
        self.idle = torch.zeros(slots, dtype=torch.int32, device=self.dev)
        self.start = torch.ones(slots, dtype=torch.int32, device=self.dev)
        self.lock_grid = torch.zeros((slots,) + self.bins, dtype=torch.int32, device=self.dev)

    def lockstep(self):
        x = self.x
        args = (self.ctx, x.data_ptr(), x.data_ptr() + 4, self.slots, self.frames, 2 * self.frames, 2, self.e0.data_ptr(),
                self.bins[0], self.e1.data_ptr(), self.bins[1], self.lock_grid.data_ptr())
        kw = dict(n_each_ptr=self.counts.data_ptr(), accumulate=True, stream=self.torch.cuda.current_stream().cuda_stream)
        if self.polar:
            self.native.polar_hist_device(*args, radius_scale=1.0, **kw)
        else:
            self.native.lissajous_hist_device(*args, **kw)


def measure(torch, forms, reps, runs):
    """forms: {name: callable}.  Median and minimum per call, the forms alternating in a rotating order."""
    names = list(forms)

    def run(name):
        for _ in range(reps):
            forms[name]()
    for _ in range(2):
        for name in names:
            run(name)
    torch.cuda.synchronize()
    times = {name: [] for name in names}
    for r in range(runs):
        for name in names[r % len(names):] + names[:r % len(names)]:
            times[name].append(timed(torch, lambda: run(name)) / reps)
    return {name: (statistics.median(t), min(t)) for name, t in times.items()}


def step(case, runs):
    slots, frames, polar, reps = SHAPES[case]
    bench = Bench(slots, frames, polar, seed=1)
    torch = bench.torch
    forms, pools = {}, {}
    if polar:
        pools['whole'] = Pool(bench, 0)
        bench.lockstep()                                              # one block each: the two must agree
        torch.cuda.synchronize()
        assert torch.equal(pools['whole'].grid, bench.lock_grid), 'the whole-voice pool and the lockstep entry differ'
        forms['whole'] = pools['whole'].call
    pools['window'] = Pool(bench, WINDOW)
    for _ in range(WINDOW // frames + 2):                             # past the window: every frame takes a count out too
        pools['window'].call()
    torch.cuda.synchronize()
    assert int(pools['window'].grid.to(torch.int64).sum()) <= slots * WINDOW
    forms['window'] = pools['window'].call
    forms['lockstep'] = bench.lockstep
    got = measure(torch, forms, reps, runs)
    total = slots * frames
    row = {'case': case, 'grid': 'polar' if polar else 'lissajous', 'slots': slots, 'frames': frames, 'bins': list(bench.bins),
           'window_frames': WINDOW, 'reps': reps, 'runs': runs}
    for form, (median, least) in got.items():
        row[form] = {'ms': fig(median), 'min_ms': fig(least), 'Gframes_per_s': fig(total / (median * 1e6))}
    for form in ('whole', 'window'):
        if form in got:
            row[form + '_over_lockstep'] = fig(got[form][0] / got['lockstep'][0])
    if 'whole' in got:
        row['window_over_whole'] = fig(got['window'][0] / got['whole'][0])
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
    line = json.dumps({'tool': 'scope_voice_pool_rate', 'rows': rows})
    print(line)
    if args.out:
        pathlib.Path(args.out).write_text(line + '\n')


if __name__ == '__main__':
    main()
