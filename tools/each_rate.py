"""decorrelate_each on a resident pool (vnd_decorrelate_each_f32_dev, vnd_haas_each_f64_dev) against today's
alternatives, exact mode.  Prints one JSON line.

Pools of B = 64 and 256 signals of 10 s 44.1 kHz stereo noise.  Velvet noise: every signal its own kappa (30 ms / 30
impulses / seed 1, MS mode, RMS normaliser); Haas: every signal its own delay up to 20 ms (LR, delayed channel 0).
- (a) ``each``: ``decorrelate_each`` of the device tensor (``each_api_ms``: the Python call, bank lookup included) and
  the C entry alone on the same buffers (``each_dev_ms``).
- (b) ``loop``: the warm loop of per-signal ``vnd_decorrelate_f32_dev`` / ``vnd_haas_f64_dev`` calls on the resident
  pool, one table per signal built (and its launch prepared) beforehand.
- (c) ``shared``: ``vnd_decorrelate_f32_dev`` / ``vnd_haas_f64_dev`` of the whole pool with ONE shared table / delay -
  the ceiling: the velvet launch runs the per-table window form.
Every time is between two device events on the current stream around the enqueues; the three forms alternate, median
of --runs.  Before any timing (a) is checked bit-equal to (b) row by row, and row 0 of (c) to row 0 of (a) with signal
0's table / delay shared.  GB/s are algorithmic: 16 B per stereo frame (8 read, 8 written) for velvet noise, 24 B for
Haas (8 read, 16 written as float64); ``read_bytes_per_frame`` adds the halo each_kernel stages per 2048-frame tile.

    python tools/each_rate.py [--runs 5] [--pools 64,256] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/each_rate.py --only-each --pools 64     (a run of its own)
"""
import argparse
import json
import pathlib
import statistics
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

FS, SECONDS, TILE = 44100, 10, 2048
VELVET = dict(sample_rate_hz=FS, duration_seconds=0.03, num_impulses=30, seed=1)
MAX_DELAY = round(0.02 * FS)


def timed(torch, fn):
    stream = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def med(values):
    return float(f'{statistics.median(values):.4g}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--pools', default='64,256')
    ap.add_argument('--only-each', action='store_true', help='form (a) alone, for a kernel trace')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    runs = max(args.runs, 5)
    import torch
    import vndecorrelate_amd.decorrelation as dec
    from vndecorrelate_amd import _native
    from vndecorrelate_amd.taps import class_path_bank_arrays
    ctx = _native.default_context()
    dev = torch.device('cuda', ctx.device)
    dec.set_each_device(True)
    n = FS * SECONDS
    result = dict(tool='each_rate', device=ctx.info()['name'], runs=runs, seconds=SECONDS, sample_rate_hz=FS,
                  mode='exact', velvet=dict(VELVET, layout='MS', normalizer='rms'), max_delay_frames=MAX_DELAY, pools={})
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream                       # noqa: E731
    stage = dict(ms_encode=True, width=None, normalize=_native.NORMALIZE_RMS_REFERENCE_ORDER)

    for batch in (int(b) for b in args.pools.split(',')):
        gen = torch.Generator(device=dev).manual_seed(batch)
        x = torch.rand((batch, n, 2), generator=gen, device=dev, dtype=torch.float32) * 2 - 1
        row = dict(frames=batch * n)

        # ---- velvet noise ----
        stages = [dec.VelvetNoise(log_distribution_strength=float(k), **VELVET) for k in np.linspace(0.0, 1.0, batch)]
        members, tables = dec.each_velvet_members(stages)
        arrays = class_path_bank_arrays(members)
        bank = _native.TapTable.create(ctx, arrays.tap_offsets, arrays.tap_index, arrays.tap_weight, **arrays.kwargs())
        index = torch.from_numpy(tables).to(dev)
        ws = _native.decorrelate_workspace_bytes(batch, n, 2)
        work = torch.empty(ws, dtype=torch.uint8, device=dev)
        y_each, y_loop, y_shared = (torch.empty((batch, n, 2), dtype=torch.float32, device=dev) for _ in range(3))
        halo = (bank.max_index + 2 + 15) & ~15
        row['velvet'] = v = dict(distinct_tables=len(members), bank_max_index=bank.max_index, halo_frames=halo,
                                 algorithmic_bytes_per_frame=16,
                                 read_bytes_per_frame=float(f'{8 * (1 + halo / TILE):.4g}'), written_bytes_per_frame=8)

        def each_api():
            return dec.decorrelate_each(x, stages)

        def each_dev():
            _native.decorrelate_each_device(ctx, bank, x.data_ptr(), index.data_ptr(), y_each.data_ptr(), batch, n, 2,
                                            workspace_ptr=work.data_ptr(), workspace_bytes=ws, stream=stream(), **stage)
        if not args.only_each:
            own = [d._device_table() for d in stages]
            ws1 = _native.decorrelate_workspace_bytes(1, n, 2)
            for t in own:
                t.prepare(1, n, 2, _native.MODE_EXACT)
            own[0].prepare(batch, n, 2, _native.MODE_EXACT)

            def loop():
                for b, t in enumerate(own):
                    t.decorrelate_device(x[b].data_ptr(), y_loop[b].data_ptr(), 1, n, 2, mode=_native.MODE_EXACT,
                                         workspace_ptr=work.data_ptr(), workspace_bytes=ws1, stream=stream(), **stage)

            def shared():
                own[0].decorrelate_device(x.data_ptr(), y_shared.data_ptr(), batch, n, 2, mode=_native.MODE_EXACT,
                                          workspace_ptr=work.data_ptr(), workspace_bytes=ws, stream=stream(), **stage)
            v['shared_launch'] = own[0].describe(batch, n, 2, _native.MODE_EXACT).split(' ')[0]
            v['loop_launch'] = own[0].describe(1, n, 2, _native.MODE_EXACT).split(' ')[0]
            each_dev(), loop(), shared()                   # warm-up, and the outputs the checks read
            y_api = each_api()
            torch.cuda.synchronize()
            v['each_equals_loop'] = bool(torch.equal(y_each, y_loop)) and bool(torch.equal(y_api, y_loop))
            v['shared_row0_equals_each_row0'] = bool(torch.equal(y_shared[0], y_each[0]))
            if not (v['each_equals_loop'] and v['shared_row0_equals_each_row0']):
                raise SystemExit(f'outputs differ: {v}')
            del y_api
            forms = dict(each_api=each_api, each_dev=each_dev, loop=loop, shared=shared)
        else:
            each_dev()
            forms = dict(each_api=each_api, each_dev=each_dev)
        times = {k: [] for k in forms}
        for _ in range(runs):                              # the forms alternate
            for k, fn in forms.items():
                times[k].append(timed(torch, fn))
        for k, t in times.items():
            v[f'{k}_ms'] = med(t)
            v[f'{k}_min_ms'] = float(f'{min(t):.4g}')
            v[f'{k}_GBps'] = float(f'{batch * n * 16 / (statistics.median(t) * 1e-3) / 1e9:.4g}')
        del y_each, y_loop, y_shared, work
        bank.close()

        # ---- Haas ----
        delays = np.rint(np.linspace(0, MAX_DELAY, batch)).astype(np.int32)
        haas = [dec.HaasEffect(sample_rate_hz=FS, delay_time_seconds=float(d) / FS) for d in delays]
        assert [round(h.delay_time_seconds * FS) for h in haas] == delays.tolist()
        frames = torch.from_numpy(delays).to(dev)
        rows = n + MAX_DELAY
        h_each = torch.empty((batch, rows, 2), dtype=torch.float64, device=dev)
        settings = dict(delayed_channel=0, ms_mode=False, width=None)
        row['haas'] = h = dict(algorithmic_bytes_per_frame=24)

        def haas_api():
            return dec.decorrelate_each(x, haas)

        def haas_dev():
            _native.haas_each_device(ctx, x.data_ptr(), h_each.data_ptr(), batch, n, 2, frames.data_ptr(),
                                     max_delay=MAX_DELAY, stream=stream(), **settings)
        if not args.only_each:
            h_loop = torch.zeros((batch, rows, 2), dtype=torch.float64, device=dev)     # signal b's (n + d_b, 2) at the row's start
            h_shared = torch.empty((batch, rows, 2), dtype=torch.float64, device=dev)

            def haas_loop():
                for b, d in enumerate(delays.tolist()):
                    _native.haas_device(ctx, x[b].data_ptr(), h_loop[b].data_ptr(), 1, n, 2, delay=d, stream=stream(), **settings)

            def haas_shared():
                _native.haas_device(ctx, x.data_ptr(), h_shared.data_ptr(), batch, n, 2, delay=MAX_DELAY, stream=stream(),
                                    **settings)
            haas_dev(), haas_loop(), haas_shared()
            got = haas_api()
            torch.cuda.synchronize()
            h['each_equals_loop'] = bool(torch.equal(h_each, h_loop)) and \
                all(bool(torch.equal(g, h_loop[b, :n + int(d)])) for b, (g, d) in enumerate(zip(got, delays)))
            h['shared_last_row_equals_each'] = bool(torch.equal(h_shared[-1], h_each[-1]))   # the last signal's delay is the shared one
            if not (h['each_equals_loop'] and h['shared_last_row_equals_each']):
                raise SystemExit(f'outputs differ: {h}')
            del got
            forms = dict(each_api=haas_api, each_dev=haas_dev, loop=haas_loop, shared=haas_shared)
        else:
            haas_dev()
            forms = dict(each_api=haas_api, each_dev=haas_dev)
        times = {k: [] for k in forms}
        for _ in range(runs):
            for k, fn in forms.items():
                times[k].append(timed(torch, fn))
        for k, t in times.items():
            h[f'{k}_ms'] = med(t)
            h[f'{k}_min_ms'] = float(f'{min(t):.4g}')
            h[f'{k}_GBps'] = float(f'{batch * n * 24 / (statistics.median(t) * 1e-3) / 1e9:.4g}')
        result['pools'][f'B{batch}'] = row
        del x, h_each
        if not args.only_each:
            del h_loop, h_shared
        torch.cuda.empty_cache()
    dec.set_each_device(None)
    line = json.dumps(result)
    print(line)
    if args.out:
        pathlib.Path(args.out).write_text(line + '\n')


if __name__ == '__main__':
    main()
