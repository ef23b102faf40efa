#!/usr/bin/env python3
"""What one call through ``_native.py`` costs on the host, this tree's binding against another checkout's.  No GPU.

    python tools/native_binding_rate.py <other checkout> [--calls 200000] [--rounds 5]

Times ``level_voice_stream_push_device`` and ``voice_stream_device`` - the per-block calls of the voice pools - against two
stand-ins for the library: ``null``, whose functions are Python callables that return 0 (the wrapper's own Python work), and
``c_noop``, where every bound name is libc's ``ffs`` under the binding's own ``argtypes`` (a context handle of 0 makes it
return 0, the other arguments are ignored: the wrapper and ctypes' conversion of every argument, no work behind them).  The
two trees alternate round by round; ns per call, median and minimum of the rounds.  Prints one JSON line.
"""
import argparse
import ctypes
import importlib.util
import json
import pathlib
import statistics
import sys
import time

REPO = pathlib.Path(__file__).resolve().parents[1]
spec = importlib.util.spec_from_file_location('gen_native_calls_golden', REPO / 'tools' / 'gen_native_calls_golden.py')
gen = importlib.util.module_from_spec(spec)
spec.loader.exec_module(gen)


class Null:
    def __getattr__(self, name):
        fn = lambda *args: 0                                                      # noqa: E731
        setattr(self, name, fn)
        return fn


class CNoop:
    def __init__(self, native):
        libc = ctypes.CDLL(None)
        for name, (_, argtypes) in gen.signature_tables(native).items():
            setattr(self, name, ctypes.CFUNCTYPE(ctypes.c_int, *argtypes)(('ffs', libc)))


def calls(native, lib):
    ctx, bank = gen.Handle(lib, 0), gen.Handle(lib, 0)
    a = list(range(4096, 4096 + 64 * 16, 64))

    def push():
        native.level_voice_stream_push_device(ctx, a[0], 1 << 20, 480, 48000, a[1], a[2], 960, 2, a[3], a[4], a[5], 360, a[6],
                                              256, radius_scale=1.0, stream=a[7])

    def voice():
        native.voice_stream_device(ctx, bank, a[0], 1 << 20, 480, a[1], a[2], a[3], a[4], a[5], a[6], 256, 2, ms_encode=True,
                                   width=None, stream=a[7])
    return {'level_voice_stream_push_device': push, 'voice_stream_device': voice}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('other')
    ap.add_argument('--calls', type=int, default=200000)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    trees = {'other': gen.load_native(pathlib.Path(args.other).resolve()), 'this': gen.load_native(REPO)}
    forms = {}
    for tree, native in trees.items():
        for stand_in, lib in (('null', Null()), ('c_noop', CNoop(native))):
            for wrapper, fn in calls(native, lib).items():
                fn()
                forms[(wrapper, stand_in, tree)] = fn
    times = {key: [] for key in forms}
    for r in range(args.rounds):
        order = list(forms)
        for key in order[r % len(order):] + order[:r % len(order)]:
            fn = forms[key]
            t0 = time.perf_counter_ns()
            for _ in range(args.calls):
                fn()
            times[key].append((time.perf_counter_ns() - t0) / args.calls)
    rows = [{'wrapper': w, 'stand_in': s, 'tree': t, 'ns_per_call': round(statistics.median(v), 1), 'min_ns': round(min(v), 1)}
            for (w, s, t), v in times.items()]
    print(json.dumps({'tool': 'native_binding_rate', 'calls': args.calls, 'rounds': args.rounds, 'rows': rows}))


if __name__ == '__main__':
    main()
