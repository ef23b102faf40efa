#!/usr/bin/env python3
"""The chunked stream call (vnd_stream_f32_dev) against the composed baseline made of existing calls, per pushed block.

Table: the 30 ms / 30-tap function-path filter at 48 kHz, stereo (H = its largest tap index).  Shapes: S streams x B
frames per call, S in {64, 512, 2048}, B in {64, 480, 4800}.  Baseline: torch.cat of the H-frame history and the chunk
on the device, vnd_convolve_f32_dev over H + B frames, keep the first B outputs (the history of the next call is a view
of the cat's last H frames).  Both run in steady state (position >= H, B outputs per call), exact mode, alternated in one
process; time per call is the median over rounds of device-event time over N back-to-back calls issued from Python.
Before timing, the two outputs are checked bit-equal at every shape.  Algorithmic bytes of a stream call: the chunk read,
the H-frame halo read from the ring, the outputs written, min(B, H) frames written to the ring.  One JSON line at the end.
"""
import argparse
import ctypes
import json
import pathlib
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
import numpy as np
import torch

import vndecorrelate_amd.decorrelation as vnd
from vndecorrelate_amd import _native
from vndecorrelate_amd.taps import function_path_arrays

PEAK_BPS = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, nargs='*', default=[64, 512, 2048])
    ap.add_argument('--frames', type=int, nargs='*', default=[64, 480, 4800])
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()

    ctx = _native.default_context()
    dev = torch.device('cuda', ctx.device)
    fir = vnd.generate_velvet_noise(duration_seconds=0.03, num_impulses=30, num_outs=2, sample_rate_hz=48000, seed=1)
    arr = function_path_arrays(fir)
    table = _native.TapTable.create(ctx, arr.tap_offsets, arr.tap_index, arr.tap_weight)
    lib, H, C = table._lib, table.max_index, 2
    stream = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    rows = []
    for S in args.streams:
        for B in args.frames:
            need = ctypes.c_int64()
            _native._check(lib.vnd_stream_state_bytes(table.handle, S, C, B, ctypes.byref(need)), 'vnd_stream_state_bytes')
            state = torch.empty(need.value, dtype=torch.uint8, device=dev)
            gen = torch.Generator(device=dev).manual_seed(S * 7 + B)
            calls_warm = (H + B - 1) // B + 2                 # until position >= H, then a couple more
            chunks = [torch.rand((S, B, C), generator=gen, device=dev) * 2 - 1 for _ in range(calls_warm + 3)]
            y_s = torch.empty((S, B, C), dtype=torch.float32, device=dev)
            y_b = torch.empty((S, H + B, C), dtype=torch.float32, device=dev)
            n_out = ctypes.c_int64()
            pos = [0]
            hist = [torch.zeros((S, H, C), dtype=torch.float32, device=dev)]

            def stream_call(chunk):
                _native._check(lib.vnd_stream_f32_dev(ctx.handle, table.handle, ctypes.c_void_p(state.data_ptr()),
                                                      need.value, B, ctypes.c_void_p(chunk.data_ptr()),
                                                      ctypes.c_void_p(y_s.data_ptr()), S, pos[0], B, C, 0,
                                                      vnd.MODE_EXACT, 0, 0, 0.0, ctypes.byref(n_out), sp),
                               'vnd_stream_f32_dev')
                pos[0] += B

            def baseline_call(chunk):
                cat = torch.cat((hist[0], chunk), dim=1)
                table.convolve_device(cat.data_ptr(), y_b.data_ptr(), S, H + B, C, vnd.MODE_EXACT, stream.cuda_stream)
                hist[0] = cat[:, B:]
                return y_b[:, :B]

            # bit-equality in steady state (output frames [pos - H, pos - H + B) of both)
            checked = 0
            for k, chunk in enumerate(chunks):
                before = pos[0]
                stream_call(chunk)
                kept = baseline_call(chunk)
                if before >= H:
                    assert n_out.value == B
                    torch.cuda.synchronize(dev)
                    assert torch.equal(y_s, kept), (S, B, k)
                    checked += 1
            assert checked >= 3
            n_calls = int(max(20, min(400, 4e8 / (S * (H + B) * C * 4))))
            t_s, t_b = [], []
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            for _ in range(args.rounds):
                ev[0].record(stream)
                for k in range(n_calls):
                    stream_call(chunks[k % len(chunks)])
                ev[1].record(stream)
                ev[2].record(stream)
                for k in range(n_calls):
                    baseline_call(chunks[k % len(chunks)])
                ev[3].record(stream)
                torch.cuda.synchronize(dev)
                t_s.append(ev[0].elapsed_time(ev[1]) / n_calls)
                t_b.append(ev[2].elapsed_time(ev[3]) / n_calls)
            ms_s, ms_b = float(np.median(t_s)), float(np.median(t_b))
            algo = S * C * 4 * (B + H + B + min(B, H))
            row = dict(streams=S, frames_per_call=B, latency=H, stream_ms=round(ms_s, 5), baseline_ms=round(ms_b, 5),
                       speedup=round(ms_b / ms_s, 3), stream_frames_per_s=round(S * B / (ms_s * 1e-3)),
                       stream_bytes_per_call=algo, stream_share_of_8TBps=round(algo / (ms_s * 1e-3) / PEAK_BPS, 4),
                       bit_equal_calls=checked)
            rows.append(row)
            print(f'S={S:5d} B={B:5d}: stream {ms_s*1e3:9.1f} us  baseline {ms_b*1e3:9.1f} us  x{ms_b/ms_s:5.2f}  '
                  f'{S*B/(ms_s*1e-3)/1e6:9.1f} Mframes/s  {algo/(ms_s*1e-3)/1e12:6.3f} TB/s '
                  f'({100*algo/(ms_s*1e-3)/PEAK_BPS:5.1f} % of 8)  bit-equal on {checked} calls', flush=True)
            del state, chunks, y_s, y_b, hist
            torch.cuda.empty_cache()
    table.close()
    print(json.dumps({'tool': 'stream_rate', 'table': '48k 30ms 30 taps stereo', 'rows': rows}))


if __name__ == '__main__':
    main()
