"""The vectorscope's histogram entries on resident pools (vnd_polar_hist_f32_dev, vnd_lissajous_hist_f32_dev) under each
route, against the moments reducer as the yardstick (vnd_polar_moments_f32_dev: the same atan2f and sqrtf per frame, DESIGN.md
§3.19).  Prints one JSON line; nothing here is asserted but that the routes give the same grid.

Cases, float32 frames drawn on the device from a seed:
- ``polar``: the default 240 x 150 polar grid, per-signal maximum (two kernels: the maximum, then the grid);
- ``polar_fixed``: the same grid with ``radius_scale`` 1 (one kernel) - on the quiet pool every frame lands in the first few
  radius bins, the centre-heavy case of the polar grid (normalised by its own maximum a quiet pool is the loud one again);
- ``lissajous``: the 512 x 512 L/R grid on [-1.1, 1.1]^2 - 1 MiB a signal, the direct route whatever is pinned;
- ``moments``: ``vnd_polar_moments_f32_dev`` on the same pool taken as one one-pair signal.
Pools: 256 x 480 000 frames of Gaussian noise (sigma 0.25, ``gauss``) and of the same noise x 0.02 (``quiet``), and 2048 x 480
(``block``, the per-block shape).  ``sweep``: the polar_fixed grid at a constant 2^22 frames cut into signals of 480 ... 65 536
frames, LDS-private against direct - where the auto choice's crossover comes from.
Each histogram case is timed with VND_SCOPE_ROUTE pinned to 1 (LDS-private), to 2 (direct) and unset (``auto``); ``route`` is
what vnd_scope_route answered.  Every time is between two device events around ``reps`` back-to-back calls on the current
stream, after two warm-up rounds; the forms alternate in a rotating order; median and minimum of --runs, per call.

Each case is a child process under its own ``timeout``; the tool stops at the first case that fails.

    python tools/scope_hist_rate.py [--runs 5] [--cases gauss,quiet,block,sweep] [--out profiles/scope_hist_rate.json]
"""
import argparse
import json
import os
import pathlib
import statistics
import subprocess
import sys

os.environ.setdefault('VND_TUNING', '1')          # VND_SCOPE_ROUTE is a tuning variable: read at the call in a tuning session
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

STEP_SECONDS = 300
CASES = ('gauss', 'quiet', 'block', 'sweep')
ROUTES = (('lds', '1'), ('direct', '2'), ('auto', None))
SWEEP_FRAMES = (480, 1200, 2400, 4800, 9600, 19200, 65536)


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


def pin(value):
    if value is None:
        os.environ.pop('VND_SCOPE_ROUTE', None)
    else:
        os.environ['VND_SCOPE_ROUTE'] = value


class Bench:
    def __init__(self, batch, frames, sigma, seed):
        import torch
        from vndecorrelate_amd import _native, vectorscope
        self.torch, self.native, self.vs = torch, _native, vectorscope
        self.ctx = _native.default_context()
        self.dev = torch.device('cuda', self.ctx.device)
        gen = torch.Generator(device=self.dev).manual_seed(seed)
        self.x = torch.randn((batch, frames, 2), generator=gen, device=self.dev, dtype=torch.float32) * sigma
        self.batch, self.frames = batch, frames
        self.work = torch.empty(batch, dtype=torch.int64, device=self.dev)
        self.edges = {}
        for name, (e0, e1) in (('polar', vectorscope.polar_edges()), ('lissajous', vectorscope.lissajous_edges())):
            self.edges[name] = (torch.from_numpy(e0).to(self.dev), torch.from_numpy(e1).to(self.dev), len(e0) - 1, len(e1) - 1)
        self.counts = {}

    def grid(self, name):
        _, _, b0, b1 = self.edges['lissajous' if name == 'lissajous' else 'polar']
        if name not in self.counts:
            self.counts[name] = self.torch.empty((self.batch, b0, b1), dtype=self.torch.int32, device=self.dev)
        return self.counts[name]

    def call(self, name):
        x, n = self.x, self.frames
        stream = self.torch.cuda.current_stream().cuda_stream
        lp, rp = x.data_ptr(), x.data_ptr() + 4
        out = self.grid(name)
        if name == 'lissajous':
            e0, e1, b0, b1 = self.edges['lissajous']
            self.native.lissajous_hist_device(self.ctx, lp, rp, self.batch, n, 2 * n, 2, e0.data_ptr(), b0, e1.data_ptr(), b1,
                                              out.data_ptr(), stream=stream)
        else:
            e0, e1, b0, b1 = self.edges['polar']
            fixed = name == 'polar_fixed'
            self.native.polar_hist_device(self.ctx, lp, rp, self.batch, n, 2 * n, 2, e0.data_ptr(), b0, e1.data_ptr(), b1,
                                          out.data_ptr(), radius_scale=1.0 if fixed else 0.0,
                                          work_ptr=0 if fixed else self.work.data_ptr(), work_bytes=0 if fixed else 8 * self.batch,
                                          stream=stream)

    def route(self, name):
        _, _, b0, b1 = self.edges['lissajous' if name == 'lissajous' else 'polar']
        return {1: 'lds', 2: 'direct'}[self.native.scope_route(b0, b1, self.frames)]


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


def histogram_rows(bench, names, reps, runs, label):
    torch = bench.torch
    rows = []
    for name in names:
        grids = {}
        for form, value in ROUTES:                                          # the routes agree before anything is timed
            pin(value)
            bench.call(name)
            torch.cuda.synchronize()
            grids[form] = bench.grid(name).clone()
        assert torch.equal(grids['lds'], grids['direct']) and torch.equal(grids['lds'], grids['auto']), f'{name}: the routes differ'
        kept = int(grids['auto'].to(torch.int64).sum())
        forms, taken = {}, {}
        for form, value in ROUTES:
            pin(value)
            taken[form] = bench.route(name)

            def fn(value=value, name=name):
                pin(value)
                bench.call(name)
            forms[form] = fn
        got = measure(torch, forms, reps, runs)
        pin(None)
        frames = bench.batch * bench.frames
        row = {'case': label, 'grid': name, 'batch': bench.batch, 'frames': bench.frames, 'reps': reps, 'runs': runs,
               'frames_kept': kept, 'busiest_cell': int(grids['auto'].max())}
        for form, (median, least) in got.items():
            row[form] = {'route': taken[form], 'ms': fig(median), 'min_ms': fig(least),
                         'Gframes_per_s': fig(frames / (median * 1e6)), 'input_GBps': fig(8 * frames / (median * 1e6))}
        faster = 'lds' if got['lds'][0] <= got['direct'][0] else 'direct'
        row['faster_pinned'] = row[faster]['route']
        row['lds_over_direct'] = fig(got['lds'][0] / got['direct'][0])
        rows.append(row)
    return rows


def moments_row(bench, reps, runs, label):
    torch, native = bench.torch, bench.native
    n = bench.batch * bench.frames
    ws = native.polar_moments_workspace_bytes(n, 1)
    work = torch.empty(ws, dtype=torch.uint8, device=bench.dev)
    out = torch.empty(8, dtype=torch.float64, device=bench.dev)

    def call():
        native.polar_moments_device(bench.ctx, bench.x.data_ptr(), n, 1, out.data_ptr(), work.data_ptr(), ws,
                                    torch.cuda.current_stream().cuda_stream)
    median, least = measure(torch, {'moments': call}, reps, runs)['moments']
    return {'case': label, 'grid': 'moments', 'batch': bench.batch, 'frames': bench.frames, 'reps': reps, 'runs': runs,
            'ms': fig(median), 'min_ms': fig(least), 'Gframes_per_s': fig(n / (median * 1e6)),
            'input_GBps': fig(8 * n / (median * 1e6))}


def step(case, runs):
    if case in ('gauss', 'quiet'):
        bench = Bench(256, 480000, 0.25 * (0.02 if case == 'quiet' else 1.0), seed=1)
        rows = histogram_rows(bench, ('polar', 'polar_fixed', 'lissajous'), 10, runs, case)
        rows.append(moments_row(bench, 10, runs, case))
        base = rows[-1]['ms']
        for row in rows[:-1]:
            row['auto_over_moments'] = fig(row['auto']['ms'] / base)
        return rows
    if case == 'block':
        bench = Bench(2048, 480, 0.25, seed=2)
        return histogram_rows(bench, ('polar', 'polar_fixed'), 50, runs, case)
    if case == 'sweep':
        rows = []
        for frames in SWEEP_FRAMES:
            bench = Bench((1 << 22) // frames, frames, 0.25, seed=3)
            rows += histogram_rows(bench, ('polar_fixed',), 20, runs, 'sweep')
            del bench
        return rows
    raise SystemExit(f'unknown case {case}')


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
    line = json.dumps({'tool': 'scope_hist_rate', 'rows': rows})
    print(line)
    if args.out:
        pathlib.Path(args.out).write_text(line + '\n')


if __name__ == '__main__':
    main()
