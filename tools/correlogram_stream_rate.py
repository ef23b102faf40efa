"""The streamed cross-correlogram (vnd_correlogram_stream_f32_dev) against its baseline, on pools of S streams pushed B
frames per call.  Prints one JSON line.

44.1 kHz with the reference's defaults: W = 882, H = 441, 1765 lags.  Blocks are device (S, B, 2) float32 slices of one
resident signal, correlated in place.  Baseline: a device ``torch.cat`` of the retained history (the frames from the
first incomplete window on, at most W - 1) and the block, then ``vnd_correlogram_f32_dev`` over it.  Before timing, both
forms run the same calls from position 0 and their rows are compared bit for bit.  Then, per round, each form pushes the
next K blocks back to back between two device events; the forms alternate, and the time is the median over rounds, per
call.  Useful FMAs are W^2 + 2W per window completed in the timed calls; their rate is given as a share of the FP64
vector spec (78.6 TF).  The time includes issuing the calls from Python.

    python tools/correlogram_stream_rate.py [--rounds 5] [--out FILE]
"""
import argparse
import json
import math
import pathlib
import statistics
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

FP64_VECTOR_SPEC_TFLOPS = 78.6          # AMD's published MI355X FP64 vector peak; not measured on these boards
POOLS = (64, 512, 2048)
BLOCKS = (64, 480, 4800)
FS, W, H, LAGS, EPS = 44100, 882, 441, 1765, 1e-10


class Baseline:
    """The history-buffer form: cat(history, block), the one-shot call, keep the frames from the next incomplete
    window on."""

    def __init__(self, torch, ctx, dev, S):
        self.torch, self.ctx, self.dev = torch, ctx, dev
        self.hist = torch.empty((S, 0, 2), dtype=torch.float32, device=dev)
        self.start = 0                                 # absolute frame of hist[:, 0]
        self.position = 0

    def process(self, block):
        from vndecorrelate_amd import analysis
        torch = self.torch
        buf = torch.cat([self.hist, block], dim=1)
        S, n = buf.shape[:2]
        out = analysis._launch(torch, self.ctx, buf.data_ptr(), buf.data_ptr() + 4, S, n, n * 2, 2, W, H, LAGS, EPS,
                               self.dev)
        self.position += block.shape[1]
        keep = (out.shape[1] * H)                      # the first window not yet complete starts here, within buf
        self.hist = buf[:, keep:]
        self.start += keep
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    rounds = max(args.rounds, 3)

    import torch
    from vndecorrelate_amd import _native, analysis
    ctx = _native.default_context()
    dev = torch.device('cuda', ctx.device)
    cur = torch.cuda.current_stream(dev)
    result = dict(tool='correlogram_stream_rate', device=ctx.info()['name'], fp64_vector_spec_tflops=FP64_VECTOR_SPEC_TFLOPS,
                  sample_rate_hz=FS, window=W, hop=H, lags=LAGS, rounds=rounds, grid={})
    for S in POOLS:
        for B in BLOCKS:
            K = max(8, math.ceil(8 * H / B))           # calls per timed round: at least 8 windows
            warm = math.ceil(2 * W / B) + K            # untimed calls from position 0, compared bit for bit
            total = (warm + rounds * K) * B
            gen = torch.Generator(device=dev)
            gen.manual_seed(S * 10007 + B)
            x = torch.rand((S, total, 2), generator=gen, device=dev, dtype=torch.float32) * 2 - 1
            stream = analysis.cross_correlogram_stream(S, sample_rate_hz=FS, max_frames_per_call=B)
            base = Baseline(torch, ctx, dev, S)
            assert (stream.window, stream.hop, stream.num_lags) == (W, H, LAGS)
            got, want = [], []
            for c in range(warm):
                blk = x[:, c * B:(c + 1) * B]
                got.append(stream.process(blk))
                want.append(base.process(blk))
            got, want = torch.cat(got, dim=1), torch.cat(want, dim=1)
            if not (got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32))):
                raise SystemExit(f'S={S} B={B}: the stream and the baseline differ')
            checked_rows = int(got.shape[1])
            del got, want
            times = {'stream': [], 'baseline': []}
            rows = {'stream': 0, 'baseline': 0}
            pos = warm * B
            for r in range(rounds):
                order = (('stream', stream), ('baseline', base)) if r % 2 == 0 else (('baseline', base), ('stream', stream))
                for name, form in order:
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record(cur)
                    n_rows = 0
                    for c in range(K):
                        out = form.process(x[:, pos + c * B:pos + (c + 1) * B])
                        n_rows += int(out.shape[1])
                    stop.record(cur)
                    stop.synchronize()
                    del out
                    times[name].append(start.elapsed_time(stop) / 1e3 / K)
                    rows[name] += n_rows
                pos += K * B
            assert rows['stream'] == rows['baseline']
            t_s, t_b = statistics.median(times['stream']), statistics.median(times['baseline'])
            fma_per_call = S * (rows['stream'] / (rounds * K)) * (W * W + 2 * W)
            tflops = 2 * fma_per_call / t_s / 1e12
            result['grid'][f'{S}x{B}'] = dict(
                streams=S, block=B, calls_per_round=K, checked_rows=checked_rows,
                stream_us=round(t_s * 1e6, 1), stream_min_us=round(min(times['stream']) * 1e6, 1),
                baseline_us=round(t_b * 1e6, 1), baseline_min_us=round(min(times['baseline']) * 1e6, 1),
                ratio=round(t_b / t_s, 2), windows_per_call=round(rows['stream'] / (rounds * K) * S, 1),
                fp64_tflops=round(tflops, 2), share_of_fp64_spec=round(tflops / FP64_VECTOR_SPEC_TFLOPS, 3))
            del x, stream, base
            torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if args.out:
        pathlib.Path(args.out).write_text(line + '\n')


if __name__ == '__main__':
    main()
