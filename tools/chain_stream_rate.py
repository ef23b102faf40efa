#!/usr/bin/env python3
"""The chain stream call (ChainStream.process on device tensors) against a baseline made of existing calls, per pushed block.

Chain: the README chain without its normaliser - VelvetNoise at 48 kHz, 30 ms / 30 taps, MS mode, normalizer=None, then
HaasEffect 20 ms (d = 960 frames), delayed channel 1, LR.  Shapes: S streams x B frames per call, S in {64, 512, 2048},
B in {64, 480, 4800}.  Baseline: the velvet stream call (vnd_stream_f32_dev), then torch.cat of the Haas stage's last d
input frames with the velvet block on the device, vnd_haas_f64_dev over those d + B frames, keep output frames [d, d + B).
Both run in steady state (position >= H + d, B outputs per call), exact mode, alternated in one process; time per call is
the median over rounds of device-event time over N back-to-back calls issued from Python.  Before timing, the two outputs
are checked bit-equal at every shape.  Algorithmic bytes of a chain call: the velvet stream's (chunk, H-frame halo, float32
outputs, ring writes) plus the Haas stream's (its float32 input read, the delayed column's halo, float64 outputs, min(B, d)
frames to its ring).  One JSON line at the end.
"""
import argparse
import json
import pathlib
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
import numpy as np
import torch

import vndecorrelate_amd.decorrelation as vnd
from vndecorrelate_amd import _native

PEAK_BPS = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, nargs='*', default=[64, 512, 2048])
    ap.add_argument('--frames', type=int, nargs='*', default=[64, 480, 4800])
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()

    ctx = _native.default_context()
    dev = torch.device('cuda', ctx.device)
    stream = torch.cuda.current_stream(dev)
    C, rows = 2, []

    def make_chain():
        return (vnd.SignalChain(sample_rate_hz=48000)
                .velvet_noise(duration_seconds=0.03, num_impulses=30, seed=1, normalizer=None)
                .haas_effect(delay_time_seconds=0.02, delayed_channel=1, mode='LR'))

    for S in args.streams:
        for B in args.frames:
            chain = make_chain()
            cs = chain.stream(num_streams=S, max_frames_per_call=B)
            vel = chain._decorrelators[0].stream(num_streams=S, max_frames_per_call=B)
            H, d = cs.latency_frames, cs.tail_frames
            gen = torch.Generator(device=dev).manual_seed(S * 7 + B)
            calls_warm = (H + d + B - 1) // B + 2                 # until both stages are in steady state
            chunks = [torch.rand((S, B, C), generator=gen, device=dev) * 2 - 1 for _ in range(calls_warm + 3)]
            y_b = torch.empty((S, d + B + d, 2), dtype=torch.float64, device=dev)
            hist = [torch.zeros((S, d, C), dtype=torch.float32, device=dev)]

            def chain_call(chunk):
                return cs.process(chunk)

            def baseline_call(chunk):
                v = vel.process(chunk)
                cat = torch.cat((hist[0], v), dim=1)
                _native.haas_device(ctx, cat.data_ptr(), y_b.data_ptr(), S, d + v.shape[1], C, delay=d,
                                    delayed_channel=1, ms_mode=False, width=None, stream=stream.cuda_stream)
                hist[0] = cat[:, v.shape[1]:]
                return y_b[:, d:d + v.shape[1]]

            checked, pushed = 0, 0
            for k, chunk in enumerate(chunks):
                got = chain_call(chunk)
                kept = baseline_call(chunk)
                pushed += B
                if pushed - B >= H + d:
                    assert got.shape[1] == B
                    torch.cuda.synchronize(dev)
                    assert torch.equal(got, kept), (S, B, k)
                    checked += 1
            assert checked >= 3
            n_calls = int(max(20, min(400, 4e8 / (S * (H + B) * C * 12))))
            t_s, t_b = [], []
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            for _ in range(args.rounds):
                ev[0].record(stream)
                for k in range(n_calls):
                    chain_call(chunks[k % len(chunks)])
                ev[1].record(stream)
                ev[2].record(stream)
                for k in range(n_calls):
                    baseline_call(chunks[k % len(chunks)])
                ev[3].record(stream)
                torch.cuda.synchronize(dev)
                t_s.append(ev[0].elapsed_time(ev[1]) / n_calls)
                t_b.append(ev[2].elapsed_time(ev[3]) / n_calls)
            ms_s, ms_b = float(np.median(t_s)), float(np.median(t_b))
            algo = S * C * 4 * (B + H + B + min(B, H)) + S * (C * 4 * (B + min(B, d)) + 2 * 8 * B + C * 4 * min(B, d))
            row = dict(streams=S, frames_per_call=B, latency=H, delay=d, chain_ms=round(ms_s, 5),
                       baseline_ms=round(ms_b, 5), speedup=round(ms_b / ms_s, 3),
                       chain_frames_per_s=round(S * B / (ms_s * 1e-3)), chain_bytes_per_call=algo,
                       chain_share_of_8TBps=round(algo / (ms_s * 1e-3) / PEAK_BPS, 4), bit_equal_calls=checked)
            rows.append(row)
            print(f'S={S:5d} B={B:5d}: chain {ms_s*1e3:9.1f} us  baseline {ms_b*1e3:9.1f} us  x{ms_b/ms_s:5.2f}  '
                  f'{S*B/(ms_s*1e-3)/1e6:9.1f} Mframes/s  {algo/(ms_s*1e-3)/1e12:6.3f} TB/s '
                  f'({100*algo/(ms_s*1e-3)/PEAK_BPS:5.1f} % of 8)  bit-equal on {checked} calls', flush=True)
            del cs, vel, chunks, y_b, hist
            torch.cuda.empty_cache()
    print(json.dumps({'tool': 'chain_stream_rate', 'chain': '48k velvet 30ms 30 taps MS -> Haas 20 ms ch1 LR',
                      'rows': rows}))


if __name__ == '__main__':
    main()
