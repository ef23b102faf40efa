"""GPU tier: every one-shot `*_dev` entry held to its exact memory footprint (include/vnd_amd.h: "caller-owned buffers", "`*_dev`
calls only enqueue ... and allocate nothing", "`workspace` is device memory of >= ... bytes").

Each case runs through tests/arena.py - one device tensor [guard | x | guard | y | guard | workspace | guard | aux | guard], y
poisoned, the workspace of exactly the declared size and poisoned too - and asserts, besides the values against the oracle the
entry's own tests use, at their bars: every guard intact (in front as behind), x and every further input unchanged, no element
of y unwritten.  The stage's cases run twice, the second time with the workspace's bits inverted: the same output bits.  Each
case names the form it asked for from the launch description (a form that was asked for and not taken fails) and the file prints
the forms it reached when it ends (-s); the stage cases hold the description and vnd_debug_decorrelate_f32_dev's report to
csrc/vnd_stage.hpp's rules restated (`_stage_plan`).  Lengths are laid around the form's own tile T and run M (read from the
description):
1, 2, M - 1, M, M + 1, T - 1, T, T + 1, 2 T + 3, 3 T, with pools of 1 and 3 distinct streams - 2 T + 3 is odd, so streams 1 and 2
of its pool start 8-byte aligned.  The `*_host` entries stage into buffers of the library's own: for them, one test per staging
route, each after a call that left NaNs in that staging."""
import collections
import re
import time

import numpy as np
import pytest

from arena import GUARD_BYTES, POISON, POISON64, SENTINEL, Arena
from oracle import c_oracle
from oracle import vnd_oracle as O
from test_gpu_correlogram import exact_R, ulps
from test_gpu_each import _class_bank, _taps
from test_gpu_fast_stage import _Env, _expect, _partial_len
from test_gpu_fuzz import random_fir
from test_gpu_haas_scan import check_row
from test_gpu_optimization import _moments64
from test_gpu_white_noise import _check_bound, _numpy_conv

pytestmark = pytest.mark.gpu

EXACT, FMA, FAST = 0, 1, 2
MODES = (EXACT, FMA, FAST)
OFF, RMS, REF = 0, 1, 2                              # NORMALIZE_*
DIRECT, SPEC_EXACT, PAR_SUMS, NO_PAR_SUMS, FORCE, NOFUSE, GENERIC = 1 << 12, 1 << 15, 1 << 17, 1 << 19, 1 << 23, 1 << 24, 1 << 25
WIN = {0: 1 << 5, 16: 2 << 5, 32: 3 << 5, 64: 4 << 5}
R4 = 4                                               # bits 0-4: frame pairs per lane of the generic plan (the fused fast stage needs 2, 4 or 8)
TOL_PEAK = 1e-6
FORMS = collections.defaultdict(set)                 # case -> the forms its launches took
STARTED = time.time()


def span_bits(min_span, rounds):
    return (min_span << 20) | (rounds << 28)


class Env:
    def __init__(self, golden):
        import torch
        import vndecorrelate_amd.decorrelation as d
        from vndecorrelate_amd import _native
        self.torch, self.d, self.native, self.golden = torch, d, _native, golden
        self.ctx = _native.default_context()
        assert 'gfx950' in self.ctx.info()['name']
        self.dev = torch.device('cuda', self.ctx.device)
        self.tables = {}

    @property
    def stream(self):
        return self.torch.cuda.current_stream(self.dev).cuda_stream

    def arrays(self, key):
        """The tap tables of the file: the golden ones, the fuzz cases' cut-ring ones, the class path's."""
        from vndecorrelate_amd.taps import TapArrays, function_path_arrays
        d, golden = self.d, self.golden
        if key == 'k30':
            return function_path_arrays(golden.fir('g48k_k30'))
        if key == 'mono':
            return function_path_arrays(np.ascontiguousarray(golden.fir('g48k_k30')[:, :1]))
        if key.startswith('wide'):                               # wide4, wide6, ...: the 8-channel table cut or doubled
            wide = golden.fir('g96k_k64_c8')
            return function_path_arrays(np.ascontiguousarray(np.concatenate([wide, wide[:, ::-1]], axis=1)[:, :int(key[4:])]))
        if key.startswith('fuzz'):                               # fuzz10, fuzz14: rings cut with a tail (test_gpu_fuzz.CASES)
            seed = int(key[4:])
            return function_path_arrays(random_fir(seed, np.random.default_rng(1000 + seed)))
        if key == 'cls':
            return d.VelvetNoise(sample_rate_hz=48000, seed=1)._tap_arrays()
        if key == 'lr8':
            return d.VelvetNoise(sample_rate_hz=48000, num_outs=8, num_impulses=30, filtered_channels=tuple(range(8)), mode='LR',
                                 seed=3)._tap_arrays()
        if key == 'huge':                                        # a halo that fits no LDS tile: the gather kernel
            return TapArrays(np.array([0, 2, 3], np.int32), np.array([3, (1 << 29) + 5, 0], np.int32),
                             np.array([0.5, 2.0, -1.0], np.float32))
        raise KeyError(key)

    def table(self, key):
        if key not in self.tables:
            arr = self.arrays(key)
            self.tables[key] = (self.native.TapTable.create(self.ctx, arr.tap_offsets, arr.tap_index, arr.tap_weight, **arr.kwargs()), arr)
        return self.tables[key]


@pytest.fixture(scope='module')
def env(golden):
    e = Env(golden)
    yield e
    e.ctx.set_variant(-1)
    for table, _ in e.tables.values():
        table.close()
    print(f'\nforms reached by tests/test_gpu_footprint.py ({time.time() - STARTED:.1f} s of wall time):')
    for case in sorted(FORMS):
        for text in sorted(FORMS[case]):
            print(f'    {case}: {text}')


# ---- shared pieces ---------------------------------------------------------------------------------------------------
def _short(text):
    """A launch description without the fields that follow the shape."""
    keep = ('frames_per_lane=', 'pairs_per_lane=', 'cg=', 'nt_stores=', 'threads=', 'store_phase=', 'pieces=', 'waves=', 'taps=')
    split = ['a chunk per CU'] if 'a chunk of' in text else ['balanced ranges'] if 'balanced ranges' in text else []
    return ' '.join([text.split()[0]] + [t for t in text.split() if t.startswith(keep)] + split)


def _tile(text):
    """(T, M): the tile in frames and a lane's run, from a launch description (the direct kernel has neither: a workgroup's frames)."""
    t = re.search(r'tile=(\d+)', text)
    m = re.search(r'frames_per_lane=(\d+)', text)
    p = re.search(r'pairs_per_lane=(\d+)', text)
    T = int(t.group(1)) if t else int(re.search(r'threads=(\d+)', text).group(1))
    return T, int(m.group(1)) if m else 2 * int(p.group(1)) if p else 2


def _lengths(T, M):
    return sorted({1, 2, M - 1, M, M + 1, T - 1, T, T + 1, 2 * T + 3, 3 * T} - {0})


def _pools(T, M):
    return [(batch, n) for n in _lengths(T, M) for batch in (1, 3)]


def _signals(seed, batch, n, cx):
    return np.random.default_rng(seed).uniform(-1, 1, (batch, n, cx)).astype(np.float32)


def _fan(x, C):
    return np.ascontiguousarray(np.tile(x, (1, 1, C // x.shape[-1])))


def _oracle(arr, x, mode):
    """(S, n, C): output channel c from input channel c % Cx, in the mode's arithmetic (the fast mode is held to the exact one)."""
    fn = c_oracle.convolve_fma if mode == FMA else c_oracle.convolve
    return fn(_fan(x, arr.num_channels), arr.tap_offsets, arr.tap_index, arr.tap_weight, seg_off=arr.seg_offsets,
              seg_end=arr.seg_end, seg_gain=arr.seg_gain, chan_flags=arr.chan_flags, apply_gain=arr.apply_gain, threads=8)


def _first_diff(got, want):
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    return None if not len(bad) else (tuple(int(i) for i in bad[0]), len(bad), float(got[tuple(bad[0])]), float(want[tuple(bad[0])]))


def _values(got, want, mode, where):
    assert got.shape == want.shape, where
    if mode != FAST:
        assert np.array_equal(got, want, equal_nan=True), (where, _first_diff(got, want))
        return
    peak = float(np.max(np.abs(want))) or 1.0
    err = float(np.max(np.abs(got.astype(np.float64) - want))) / peak
    assert err <= TOL_PEAK, f'{where}: {err:.2e} of peak'


def _aligned(batch, n, C, cx):
    """Whether the per-table kernels take the pool: every stream of x and y on their access boundary (make_spec_plan)."""
    return batch == 1 or C != 2 or n % 2 == 0


def _convolve(env, table, arr, x, mode, where, skew=None):
    batch, n, cx = x.shape
    a = Arena(env.torch, env.dev, x=x, y=((batch, n, arr.num_channels), np.float32), skew=skew)
    table.convolve_device(a.ptr('x'), a.ptr('y'), batch, n, cx, mode, env.stream)
    return a.check(where)[0]


GENERIC_NAMES = ('conv_ordered', 'conv_fast', 'conv_direct')


def _conv_form(env, case, key, *, variant, modes, expect, tuning=None, cx=None, pools=_pools, seed=0):
    """One form of vnd_convolve_f32_dev / vnd_convolve_fanout_f32_dev: `expect(text, mode)` holds the description of every launch
    the per-table kernels can take to the form asked for; a pool they cannot take (8-byte aligned streams) must say a generic one."""
    table, arr = env.table(key)
    C = arr.num_channels
    cx = cx or C
    with _Env(tuning):
        env.ctx.set_variant(variant)
        try:
            for mode in modes:
                T, M = _tile(table.describe(1, 4096, cx, mode))
                for batch, n in pools(T, M):
                    where = f'{case} {key} mode={mode} batch={batch} n={n} (T={T} M={M})'
                    text = table.describe(batch, n, cx, mode)
                    if _aligned(batch, n, C, cx):
                        expect(text, mode)
                    else:
                        assert text.startswith(GENERIC_NAMES), (where, text)
                    FORMS[case].add(_short(text))
                    x = _signals(seed * 1000003 + n * 7 + batch, batch, n, cx)
                    _values(_convolve(env, table, arr, x, mode, where), _oracle(arr, x, mode), mode, where)
        finally:
            env.ctx.set_variant(-1)


def _has(*tokens, exact_prefix='conv_spec_exact', fast_prefix='conv_spec', absent=()):
    def expect(text, mode):
        prefix = fast_prefix if mode == FAST else exact_prefix
        assert text.startswith(prefix) and all(t in text for t in tokens) and not any(t in text for t in absent), (mode, tokens, text)
    return expect


# ---- 0. the harness itself: both assertions can fail (no project kernel runs) -----------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_the_arena_sees_a_store_into_a_guard_and_a_hole_in_y(env, dtype):
    torch = env.torch
    x = _signals(1, 3, 50, 2)
    a = Arena(torch, env.dev, x=x, y=((3, 50, 2), dtype), workspace_bytes=100, aux={'table': np.arange(3, dtype=np.int32)},
              skew={'y': 8, 'table': 4})
    y = a.tensor('y')
    with pytest.raises(AssertionError, match='never written'):
        a.check('untouched')                                     # nothing wrote y at all
    y[...] = 1.0
    got, ws = a.check('filled')
    assert (got == 1.0).all() and got.dtype == dtype and len(ws) == 100
    y[1, 7, 1] = torch.tensor(np.array([POISON64 if a.wide else POISON], np.uint64 if a.wide else np.uint32).view(dtype))[0]
    with pytest.raises(AssertionError, match=r'never written, the first at index \(1, 7, 1\)'):
        a.check('a hole')
    a.reset()
    y[...] = 1.0
    words = y.numel() * (2 if a.wide else 1)
    flat = a.buf[a.offset['y'] // 4:]                            # from y's first word to the end of the arena
    flat[words:words + 4] = 0                                    # a slice assignment one frame past y
    with pytest.raises(AssertionError, match='a guard was written.*past the end of y'):
        a.check('past y')
    a.reset()
    y[...] = 1.0
    a.buf[a.offset['y'] // 4 - 1] = 0                            # ... and one word in front of it
    with pytest.raises(AssertionError, match='a guard was written.*in front of y'):
        a.check('in front of y')
    a.reset()
    y[...] = 1.0
    a.buf[(a.offset['ws'] + 100) // 4] = 0                       # the first word past the workspace's declared bytes
    with pytest.raises(AssertionError, match='a guard was written.*past the end of ws'):
        a.check('past the workspace')
    a.reset()
    y[...] = 1.0
    a.buf[a.offset['x'] // 4 + 5] = 0
    with pytest.raises(AssertionError, match='input x was changed'):
        a.check('x')
    assert GUARD_BYTES >= 2 * 128 * 1024 and SENTINEL != POISON


# ---- 1. vnd_convolve_f32_dev: every form -----------------------------------------------------------------------------------------
def _generic(text, mode):
    assert text.startswith('conv_fast' if mode == FAST else 'conv_ordered'), (mode, text)


def _direct(text, mode):
    assert text.startswith('conv_direct'), (mode, text)


def _adds(on):
    def expect(text, mode):
        assert text.startswith('conv_spec_window') and text.endswith('taps=adds-per-segment') == on, (on, text)
    return expect


def _ragged(streams):
    """Ragged pools for the balanced cut: ranges of a tile or two that run from one stream into the next, tails inside a tile."""
    def pools(T, M):
        return [(streams, 2 * T + 50), (streams, T + 2 * M + 2), (streams, 3 * T)]
    return pools


def _chunked(T, M):
    """One CU chunk per 1 / 256 (1 / 128) of a stream: the smallest pools whose chunks are two tiles, the last one ragged."""
    return [(1, 511 * T + 10), (2, 255 * T + 2 * M + 6)]


def _paced(T, M):
    return [(3, 100 * T + 2 * M)]                                # 300 one-tile spans: more than one workgroup per CU, fewer than two


WINDOW = _has('_window', 'frames_per_lane=')
CONV_FORMS = [
    # case, table, variant, tuning, input channels (None: the table's), modes, expectation, pools
    ('generic', 'k30', GENERIC, None, None, MODES, _generic, _pools),
    ('generic, 4 pairs per lane', 'k30', GENERIC | R4, None, None, MODES, _generic, _pools),
    ('generic C=8', 'wide8', GENERIC, None, None, MODES, _generic, _pools),
    ('generic C=8, a channel per workgroup', 'wide8', GENERIC | (1 << 8), None, None, MODES, _generic, _pools),
    ('generic C=8, four channels per workgroup', 'wide8', GENERIC | (4 << 8), None, None, MODES, _generic, _pools),
    ('generic C=3 (odd channel count)', 'fuzz2', GENERIC, None, None, MODES, _generic, _pools),
    ('direct (halo fits no LDS tile)', 'huge', -1, None, None, MODES, _direct, _pools),
    ('direct (variant bit 12)', 'k30', DIRECT, None, None, MODES, _direct, _pools),
    ('pair-read', 'k30', FORCE | WIN[0] | span_bits(1, 3), None, None, (EXACT, FAST),
     _has('pairs_per_lane=', exact_prefix='conv_spec_exact (', fast_prefix='conv_spec ('), _pools),
    ('window 32', 'k30', FORCE | WIN[32] | span_bits(1, 7), {'VND_SPEC_NT': 128}, None, (EXACT, FAST),
     _has('_window', 'frames_per_lane=32 ', 'threads=128', absent=('split',)), _pools),
    ('window 16', 'k30', FORCE | WIN[16] | span_bits(2, 1), {'VND_SPEC_NT': 128}, None, (EXACT, FAST),
     _has('_window', 'frames_per_lane=16 ', 'threads=128', absent=('split',)), _pools),
    ('split 64', 'k30', FORCE | WIN[64] | span_bits(1, 3), {'VND_WIN_SPLIT': 2, 'VND_SPEC_NT': 256}, None, (EXACT, FAST),
     _has('_window', 'frames_per_lane=64 ', 'threads=256', 'waves=split-by-channel'), _pools),
    ('quads C=4', 'wide4', FORCE | WIN[32] | span_bits(1, 7), {'VND_SPEC_NT': 256, 'VND_WIN_OCTET': 0}, None, (EXACT, FAST),
     _has('_window', 'pieces=channel-quads waves=split-by-channel'), _pools),
    ('octets C=8', 'wide8', FORCE | WIN[32] | span_bits(2, 1), {'VND_SPEC_NT': 512, 'VND_WIN_OCTET': 1}, None, (EXACT, FAST),
     _has('_window', 'pieces=channel-octets waves=split-by-channel'), _pools),
    ('octets C=16', 'wide16', FORCE | WIN[32] | span_bits(1, 7), {'VND_SPEC_NT': 512, 'VND_WIN_OCTET': 1}, None, (EXACT,),
     _has('_window', 'pieces=channel-octets waves=split-by-channel'), _pools),
    ('4k+2 C=6', 'wide6', FORCE | WIN[32] | span_bits(1, 7), {'VND_SPEC_NT': 256, 'VND_WIN_OCTET': 0}, None, (EXACT, FAST),
     _has('_window', 'pieces=channel-quads'), _pools),
    ('4k+2 C=10', 'wide10', FORCE | WIN[16] | span_bits(2, 1), {'VND_SPEC_NT': 256, 'VND_WIN_OCTET': 0}, None, (EXACT, FAST),
     _has('_window', 'pieces=channel-quads'), _pools),
    ('cut ring C=8 (8, 2719)', 'fuzz10', FORCE | WIN[32] | span_bits(1, 3), None, None, (EXACT, FAST),
     _has('_window', 'pieces=channel-'), _pools),
    ('cut ring 4k+2 C=6 (6, 2719)', 'fuzz14', FORCE | WIN[32] | span_bits(1, 3), None, None, (EXACT, FAST),
     _has('_window', 'pieces=channel-quads'), _pools),
    ('exact window, class path: split', 'cls', FORCE, {'VND_SPEC_NT': 256}, None, (EXACT,),
     _has('_window', 'frames_per_lane=64 ', 'waves=split-by-channel'), _pools),
    ('exact window, class path: plain', 'cls', FORCE, {'VND_SPEC_NT': 256, 'VND_WIN_SPLIT_CLASS': 0}, None, (EXACT,),
     _has('_window', 'frames_per_lane=32 ', absent=('split',)), _pools),
    ('balanced cut, 3 streams', 'k30', FORCE, {'VND_SPEC_NT': 256, 'VND_WIN_BALANCE': 2}, None, (EXACT, FAST), _has('_window', 'balanced ranges'), _ragged(3)),
    ('balanced cut, 5 streams', 'cls', FORCE, {'VND_SPEC_NT': 256, 'VND_WIN_BALANCE': 2}, None, (EXACT, FAST), _has('_window', 'balanced ranges'), _ragged(5)),
    ('CU chunks', 'k30', FORCE | WIN[16], {'VND_SPEC_NT': 64, 'VND_WIN_CHUNKS': 1, 'VND_WIN_CHUNK_LEN0': 1}, None, (EXACT, FAST),
     _has('_window', 'a chunk of 2 tiles per CU as 1 + 1'), _chunked),
    ('CU chunks off', 'k30', FORCE | WIN[16], {'VND_SPEC_NT': 64, 'VND_WIN_CHUNKS': 0}, None, (FAST,),
     _has('_window', absent=('a chunk of',)), _chunked),
    ('pacing from the first tile', 'k30', FORCE | WIN[16] | span_bits(1, 1), {'VND_SPEC_NT': 64, 'VND_WIN_PACE_MIN_TILES': 1}, None,
     (EXACT, FAST), _has('_window', 'spans x 1 tiles'), _paced),
    ('non-temporal stores, stereo', 'k30', FORCE | WIN[32] | span_bits(1, 7), {'VND_SPEC_NT': 128, 'VND_FORCE_NT': 1, 'VND_NT_MIN_MB': 0},
     None, (EXACT, FAST), _has('_window', 'nt_stores=1'), _pools),
    ('non-temporal stores, octets C=16', 'wide16', FORCE | WIN[32] | span_bits(1, 7),
     {'VND_SPEC_NT': 512, 'VND_WIN_OCTET': 1, 'VND_FORCE_NT': 1, 'VND_NT_MIN_MB': 0}, None, (FAST,),
     _has('_window', 'pieces=channel-octets', 'nt_stores=1'), _pools),
    ('non-temporal stores, pair-read', 'k30', FORCE | WIN[0] | span_bits(1, 3), {'VND_FORCE_NT': 1, 'VND_NT_MIN_MB': 0}, None, (EXACT, FAST),
     _has('pairs_per_lane=', 'nt_stores=1'), _pools),
    ('adds per segment', 'cls', FORCE | WIN[32] | span_bits(1, 7), {'VND_WIN_ADDS': 1}, None, (FAST,), _adds(True), _pools),
    ('one FMA per tap', 'cls', FORCE | WIN[32] | span_bits(1, 7), {'VND_WIN_ADDS': 0}, None, (FAST,), _adds(False), _pools),
    # vnd_convolve_fanout_f32_dev
    ('fan-out mono -> stereo, merged reads', 'k30', FORCE, {'VND_SPEC_NT': 256}, 1, (EXACT, FAST),
     _has('_window', 'frames_per_lane=32 ', absent=('split',)), _pools),
    ('fan-out mono -> stereo, class path: split form, both plane sets', 'cls', FORCE, {'VND_SPEC_NT': 256}, 1, (EXACT,),
     _has('_window', 'frames_per_lane=64 ', 'waves=split-by-channel'), _pools),
    ('fan-out mono -> stereo, generic', 'k30', GENERIC, None, 1, MODES, _generic, _pools),
    ('fan-out two-filter bank, in_channels = 2', 'wide4', -1, None, 2, MODES, _generic, _pools),
    ('fan-out four-filter bank of a mono input', 'wide8', -1, None, 1, MODES, _generic, _pools),
]


@pytest.mark.parametrize('case, key, variant, tuning, cx, modes, expect, pools', CONV_FORMS, ids=[c[0] for c in CONV_FORMS])
def test_convolve_forms(env, case, key, variant, tuning, cx, modes, expect, pools):
    _conv_form(env, f'convolve: {case}', key, variant=variant, tuning=tuning, cx=cx, modes=modes, expect=expect, pools=pools,
               seed=len(case))


def _per_table_takes(C, cx, batch, n, skew):
    """make_spec_plan's access shape: 16 bytes per frame pair of a stereo signal (8 from a mono input), 8 per frame of a wider one,
    from every stream's first sample."""
    skew = skew or {}
    need_y = 16 if C == 2 else 8
    need_x = 8 if cx == 1 and C == 2 else need_y
    return skew.get('x', 0) % need_x == 0 and skew.get('y', 0) % need_y == 0 and _aligned(batch, n, C, cx)


def _route(env, table, arr, x, skew):
    """Which kernel takes a launch from these pointers: the plain convolution reports nothing, so the stage's hook is asked about the
    same pointers in the exact mode - the side-channel encode alone on a stereo table, the normaliser alone on a wider one.  The
    store phase of a per-table kernel says 1 or 2 there, a generic kernel 0."""
    batch, n, cx = x.shape
    C = arr.num_channels
    ws_bytes = env.native.decorrelate_workspace_bytes(batch, n, C)
    a = Arena(env.torch, env.dev, x=x, y=((batch, n, C), np.float32), workspace_bytes=ws_bytes, skew=skew)
    taken = table.decorrelate_device_taken(a.ptr('x'), a.ptr('y'), batch, n, cx, mode=EXACT, ms_encode=C == 2, width=None,
                                           normalize=OFF if C == 2 else RMS, workspace_ptr=a.ptr('ws'), workspace_bytes=ws_bytes,
                                           stream=env.stream)
    a.check(f'route of {skew}')
    return taken['conv_path']


@pytest.mark.parametrize('skew', [dict(x=4), dict(y=4), dict(x=8), dict(x=8, y=8), dict(x=4, y=8), dict(x=8, y=4)],
                         ids=lambda s: ' '.join(f'{k}+{v}' for k, v in s.items()))
@pytest.mark.parametrize('key, cx', [('k30', 2), ('k30', 1), ('wide8', 8)])
def test_convolve_from_bases_off_the_16_byte_boundary(env, key, cx, skew):
    """x or y 4 or 8 bytes past a 16-byte boundary, the window form asked for.  The description only knows the shape; the launch sees
    the pointers.  A stereo table needs both on 16 bytes: every skew here goes to a generic kernel.  Its mono input needs 8: x + 8
    alone keeps the per-table kernel (the one-plane staging from an 8-byte base).  An 8-channel table needs 8 on both sides: x + 8
    and x + 8, y + 8 keep the octet kernel (its 32-byte frames from an 8-byte base), every skew of 4 goes generic.  The route is
    asserted through the stage's hook on the same pointers."""
    table, arr = env.table(key)
    C = arr.num_channels
    env.ctx.set_variant(FORCE | WIN[32] | span_bits(1, 7))
    try:
        routes = set()
        for mode in MODES:
            T, M = _tile(table.describe(1, 4096, cx, mode))
            for batch, n in ((1, 1), (3, 2), (1, M + 1), (3, T - 1), (1, T), (3, T + 1), (3, 2 * T + 3), (1, 3 * T)):
                where = f'skew {skew} {key} cx={cx} mode={mode} batch={batch} n={n}'
                x = _signals(n + batch + cx, batch, n, cx)
                _values(_convolve(env, table, arr, x, mode, where, skew=skew), _oracle(arr, x, mode), mode, where)
                if mode == EXACT:
                    per_table = _per_table_takes(C, cx, batch, n, skew)
                    assert (_route(env, table, arr, x, skew) != 0) == per_table, (where, per_table)
                    routes.add('per-table' if per_table else 'generic')
        FORMS[f'convolve: bases off the 16-byte boundary ({key}, {cx} input channels)'].add(
            ' '.join(f'{k}+{v}' for k, v in skew.items()) + ': ' + ' and '.join(sorted(routes))
            + ' (generic where the pool is 3 streams of an odd length)' * (len(routes) == 2))
    finally:
        env.ctx.set_variant(-1)


# ---- 2. vnd_decorrelate_f32_dev / vnd_decorrelate_fanout_f32_dev: the stage, a workspace of exactly the declared bytes -----------------
STAGE_N = (1, 2, 2047, 2048, 2049, 8191, 8192, 8193, 3 * 2048 + 5)


def _stage_plan(variant, tuning, *, C, cx, batch, n, mode, ms, width, normalize, skew, fast_epi):
    """What decorrelate_dev does with a case, restated from csrc/vnd_stage.hpp for the tables of this file: (tokens of the launch
    description, branch, conv_path, numpy_order, blk_done).  The description knows the shape alone, the launch the pointers too.
      * kernel: the variant's - the window form (bits 5-7 = 3), the pair-read form (1), the octet form (8 channels, forced), the
        generic kernels (bit 25, or nothing forced at these sizes) - where the per-table kernels' access shape holds and the mode
        is not fma; else a generic one;
      * numpy_order: the normaliser's sums in NumPy's order - the exact mode, or VND_NORMALIZE_RMS_REFERENCE_ORDER;
      * fused (fast mode): the generic plan of the shape has an epilogue instantiation (2, 4 or 8 pairs per lane: pinned by the
        variant here, or a pool large enough), bit 24 (nofuse) is off, and the call is not NumPy-order sums alone;
      * conv_path (what the convolution's store phase did): 0 a generic kernel or a plain launch, 1 a per-table kernel that left
        the sums, 2 one that did not.  The exact and fma modes hand the store phase the pointwise steps, or the block sums alone;
        bit 24 hands it nothing (0).  Block sums exist for stereo NumPy-order sums unless bit 19 (no_par_sums) or
        VND_EPI_BLOCK_SUMS=0 (then 2); the pair-read form never leaves them (2);
      * blk_done: the block-parallel sums start from the store phase's block sums."""
    v = max(variant, 0)
    nofuse, no_par, generic, force = bool(v & NOFUSE), bool(v & NO_PAR_SUMS), bool(v & GENERIC), bool(v & FORCE)
    blk_on = str((tuning or {}).get('VND_EPI_BLOCK_SUMS', 1)) != '0'
    win, pairs = (v >> 5) & 7, v & 31
    kind = 'generic' if generic or not force else 'window' if win == 3 else 'pair' if win == 1 else 'octets' if C == 8 else None
    assert kind is not None, variant
    described = kind != 'generic' and mode != FMA and _aligned(batch, n, C, cx)
    per_table = described and _per_table_takes(C, cx, batch, n, skew)
    pointwise = bool(ms) or width is not None
    want_seq = bool(normalize) and (mode == EXACT or normalize == REF)
    par_ok = want_seq and C % 2 == 0 and (C == 2 or cx == C) and not no_par
    want_blk = par_ok and C == 2 and blk_on
    if described:
        exact = '_exact' if mode == EXACT else ''
        tokens = {'window': (f'conv_spec{exact}_window', 'frames_per_lane=32 '), 'pair': (f'conv_spec{exact} (', 'pairs_per_lane='),
                  'octets': (f'conv_spec{exact}_window', 'pieces=channel-octets')}[kind]
    else:
        tokens = (('conv_fast' if mode == FAST else 'conv_ordered') + ('_fanout' if cx == 1 and C != 1 else ''),)
        if pairs:
            tokens += (f'pairs_per_lane={pairs} ',)
    any_step = pointwise or bool(normalize)
    branch, conv_path = 'table-order', 0
    if mode == FAST and normalize and not want_seq and not pointwise and C % 4 == 0 and cx == C and not nofuse and blk_on and per_table:
        branch, conv_path = 'q_done', 1
    elif any_step and mode == FAST and not nofuse and fast_epi and not (want_seq and not pointwise):
        branch = 'fused'
        sums_in_store_phase = (want_blk and want_seq) or (not want_seq and bool(normalize) and C == 2 and blk_on)
        if per_table:
            conv_path = 2 if kind == 'pair' else 1 if sums_in_store_phase else 2 if want_seq or not normalize else 0
    elif mode != FAST:
        sums_only = not pointwise and want_blk and bool(normalize)
        if (pointwise or sums_only) and not nofuse and per_table and C == 2:
            conv_path = 1 if kind == 'window' and want_blk else 2
        elif kind == 'octets' and per_table and par_ok and normalize and mode == EXACT and not nofuse and blk_on:
            conv_path = 1
    blk_done = conv_path == 1 and (want_blk or kind == 'octets') and branch != 'q_done'
    return tokens, branch, conv_path, want_seq, blk_done


def _stage(env, case, key, x, mode, *, ms, width, normalize, variant=-1, tuning=None, skew=None, fast_epi=None):
    """One stage call through the arena, twice (the workspace poisoned, then its bits inverted: the same output), against NumPy's
    epilogue: on the oracle's convolution bit for bit in the exact and fma modes, on the kernel's own convolution in the fast one.
    The form that ran - the launch description and what vnd_debug_decorrelate_f32_dev reports - must be the one `_stage_plan`
    derives from the variant and the tuning variables of the case.  VND_NORMALIZE_RMS in the fma mode (float64 sums of float32
    partials on a convolution with no fast-mode twin) has no reference in this file: footprint and workspace independence only."""
    table, arr = env.table(key)
    C = arr.num_channels
    batch, n, cx = x.shape
    where = f'{case} {key} mode={mode} batch={batch} n={n} cx={cx} ms={ms} width={width} normalize={normalize}'
    ws_bytes = env.native.decorrelate_workspace_bytes(batch, n, C)
    if fast_epi is None:
        fast_epi = variant >= 0 and (variant & 31) in (2, 4, 8)
    with _Env(tuning):
        env.ctx.set_variant(variant)
        try:
            a = Arena(env.torch, env.dev, x=x, y=((batch, n, C), np.float32), workspace_bytes=ws_bytes, skew=skew)
            kw = dict(mode=mode, ms_encode=ms, width=width, normalize=normalize, workspace_ptr=a.ptr('ws'), workspace_bytes=ws_bytes,
                      stream=env.stream)
            table.decorrelate_device(a.ptr('x'), a.ptr('y'), batch, n, cx, **kw)
            y, ws = a.check(where)
            a.reset(invert_workspace=True)
            taken = table.decorrelate_device_taken(a.ptr('x'), a.ptr('y'), batch, n, cx, **kw)
            y2, _ = a.check(where + ' (workspace inverted)')
            assert np.array_equal(y.view(np.int32), y2.view(np.int32)), (where, 'the output depends on what the workspace held',
                                                                         _first_diff(y, y2))
            text = table.describe(batch, n, cx, mode)
            conv = _convolve(env, table, arr, x, mode, where + ' (convolution)', skew=skew) if mode == FAST else None
        finally:
            env.ctx.set_variant(-1)
    tokens, branch, conv_path, numpy_order, blk_done = _stage_plan(variant, tuning, C=C, cx=cx, batch=batch, n=n, mode=mode, ms=ms,
                                                                   width=width, normalize=normalize, skew=skew, fast_epi=fast_epi)
    assert text.startswith(tokens[0]) and all(t in text for t in tokens[1:]), (where, tokens, text)
    assert taken == dict(branch=branch, conv_path=conv_path, numpy_order=numpy_order, blk_done=blk_done), \
        (where, taken, dict(branch=branch, conv_path=conv_path, numpy_order=numpy_order, blk_done=blk_done), text)
    FORMS[case].add(f"{_short(text)} | branch={taken['branch']} conv_path={taken['conv_path']} numpy_order={int(taken['numpy_order'])} "
                    f"blk_done={int(taken['blk_done'])}")
    if mode == FMA and normalize == RMS:
        return
    x2 = _fan(x, C)
    with np.errstate(all='ignore'):
        if mode == FAST:
            _values(conv, _oracle(arr, x, mode), FAST, where + ' (convolution)')
            if normalize == REF and cx != C and C != 2:          # (a bank: the output alone - where its sums lie in the workspace is the library's)
                want = conv.copy()
                for b in range(batch):
                    O.rms_normalize(x2[b], want[b])
                assert np.array_equal(y, want, equal_nan=True), (where, _first_diff(y, want))
                return
            _expect(x, y, conv, ws[:len(ws) // 8 * 8].view(np.float64), taken, ms=ms, width=width, normalize=normalize,
                    k=_partial_len(taken, text) if normalize == RMS else None, tag=f'footprint/{case}')
            return
        want = _oracle(arr, x, mode)
        if ms or width is not None:
            want = np.stack([O.pointwise(x2[b], want[b], ms, width) for b in range(batch)])
        if normalize:
            for b in range(batch):
                O.rms_normalize(x2[b], want[b])
    assert np.array_equal(y, want, equal_nan=True), (where, _first_diff(y, want))


STEPS = [(True, None), (False, None), (True, 0.3), (False, 0.3)]            # MS and LR, width None and 0.3
STAGE_FORMS = [
    # case, table, input channels, variant, tuning, modes, normalisers
    ('automatic', 'cls', 2, -1, None, MODES, (OFF, RMS, REF)),
    ('automatic, mono input', 'cls', 1, -1, None, (EXACT, FAST), (OFF, RMS, REF)),
    ('store-phase epilogue (window 32)', 'cls', 2, FORCE | WIN[32], None, (EXACT, FAST), (OFF, RMS, REF)),
    ('store-phase epilogue (window 32), function path', 'k30', 2, FORCE | WIN[32], None, (EXACT, FAST), (RMS, REF)),
    ('store-phase epilogue (window 32), mono input', 'k30', 1, FORCE | WIN[32], None, (EXACT, FAST), (RMS, REF)),
    ('nofuse, window 32', 'cls', 2, NOFUSE | FORCE | WIN[32], None, (EXACT, FAST), (RMS, REF)),
    ('nofuse, generic, 4 pairs per lane', 'cls', 2, NOFUSE | GENERIC | R4, None, (FAST,), (OFF, RMS, REF)),
    ('generic fast kernel, 4 pairs per lane', 'cls', 2, GENERIC | R4, None, (FAST,), (OFF, RMS, REF)),
    # (bit 17, par_sums, forces the block-parallel sums that pools of up to 64 streams take anyway: nothing reports which sums kernel
    #  ran, so the switch is run for its footprint and is not confirmable; bit 19 shows - no block sums leave the store phase)
    ('par_sums (not confirmable)', 'cls', 2, FORCE | WIN[32] | PAR_SUMS, None, (EXACT,), (RMS,)),
    ('no_par_sums', 'cls', 2, FORCE | WIN[32] | NO_PAR_SUMS, None, (EXACT,), (RMS, REF)),
    ('block sums off', 'cls', 2, FORCE | WIN[32], {'VND_EPI_BLOCK_SUMS': 0}, (EXACT, FAST), (RMS, REF)),
    ('pair-read', 'k30', 2, FORCE | WIN[0], None, (EXACT, FAST), (RMS, REF)),
]


@pytest.mark.parametrize('case, key, cx, variant, tuning, modes, normalizers', STAGE_FORMS, ids=[c[0] for c in STAGE_FORMS])
def test_stage_forms(env, case, key, cx, variant, tuning, modes, normalizers):
    for mode in modes:
        for normalize in normalizers:
            for i, n in enumerate(STAGE_N):
                for batch in (1, 3):
                    ms, width = STEPS[(i + batch + normalize) % 4]
                    if normalize == OFF and not ms and width is None:
                        ms = True
                    x = _signals(n * 31 + batch + cx, batch, n, cx)
                    _stage(env, f'stage: {case}', key, x, mode, ms=ms, width=width, normalize=normalize, variant=variant, tuning=tuning)


@pytest.mark.parametrize('ms, width', STEPS)
@pytest.mark.parametrize('normalize', [OFF, RMS, REF])
def test_stage_every_step_at_the_block_seams(env, ms, width, normalize):
    """MS and LR, width None and 0.3, each normaliser: the exact mode on the lengths around a 2048-frame block and an odd pool."""
    if normalize == OFF and not ms and width is None:
        return                                                   # (the bare convolution: section 1)
    for n in (2047, 2049, 3 * 2048 + 5):
        for batch in (1, 3):
            x = _signals(n + batch, batch, n, 2)
            _stage(env, 'stage: every step, exact, automatic', 'cls', x, EXACT, ms=ms, width=width, normalize=normalize)
            _stage(env, 'stage: every step, exact, store phase', 'cls', x, EXACT, ms=ms, width=width, normalize=normalize,
                   variant=FORCE | WIN[32])


def test_stage_fused_fast_launch_of_a_pool(env):
    """The fast mode fuses the stage into one launch only where the generic plan of the shape has an epilogue instantiation: a pool of
    96 streams of 20012 frames (the last tile and the last block partial) - the window form's store phase, and the generic kernel."""
    x = _signals(5, 96, 20012, 2)
    for variant, name in ((FORCE | WIN[32], 'window 32'), (GENERIC | R4, 'generic')):
        for normalize, (ms, width) in ((RMS, (True, 0.3)), (REF, (False, 0.3))):
            _stage(env, f'stage: fused fast launch, {name}', 'cls', x, FAST, ms=ms, width=width, normalize=normalize, variant=variant,
                   fast_epi=True)


@pytest.mark.parametrize('mode', [EXACT, FMA])
def test_stage_mono_table_pairwise_sums(env, mode):
    """A single-channel table: NumPy sums an (n, 1) array pairwise in 8192-element chunks."""
    for n in (1, 2047, 2048, 2049, 8191, 8192, 8193, 3 * 8192 + 5):
        for batch in (1, 3):
            for normalize in (RMS, REF):
                x = _signals(n + batch, batch, n, 1)
                _stage(env, 'stage: mono table (pairwise sums)', 'mono', x, mode, ms=False, width=None, normalize=normalize)


@pytest.mark.parametrize('mode, normalize, variant', [(EXACT, RMS, FORCE), (EXACT, REF, -1), (FAST, RMS, FORCE), (FAST, REF, FORCE), (FMA, REF, -1),
                                                      (FMA, RMS, -1)])
def test_stage_eight_channel_octets(env, mode, normalize, variant):
    """LR mode on 8 channels: in the fast mode the normaliser's sums leave the octet kernel's store phase (q_done)."""
    for n in (1, 2047, 2048, 2050, 3 * 2048 + 6, 60078):
        for batch in (1, 3):
            x = _signals(n + batch, batch, n, 8)
            _stage(env, 'stage: 8-channel LR octets', 'lr8', x, mode, ms=False, width=None, normalize=normalize, variant=variant)


@pytest.mark.parametrize('key, cx', [('wide4', 2), ('wide8', 1)])
def test_stage_fanout_bank(env, key, cx):
    """vnd_decorrelate_fanout_f32_dev on a bank: the normaliser pairs output channel c with input channel c % in_channels."""
    for mode in MODES:
        for n in (1, 2049, 3 * 2048 + 5):
            for batch in (1, 3):
                x = _signals(n + batch + cx, batch, n, cx)
                _stage(env, f'stage: fan-out bank, in_channels = {cx}', key, x, mode, ms=False, width=None, normalize=REF)


@pytest.mark.parametrize('skew', [dict(x=8, y=8, ws=8), dict(x=4, y=4), dict(ws=8)], ids=lambda s: ' '.join(f'{k}+{v}' for k, v in s.items()))
def test_stage_from_skewed_buffers(env, skew):
    """(The workspace holds doubles: 8-byte alignment is the caller's to give, so its skew is 8 only.)"""
    for mode in (EXACT, FAST):
        for n, batch in ((2049, 3), (8193, 1), (3 * 2048 + 6, 3)):
            x = _signals(n + batch, batch, n, 2)
            _stage(env, 'stage: skewed buffers', 'cls', x, mode, ms=True, width=0.3, normalize=REF, variant=FORCE | WIN[32], skew=skew)


# ---- 3. vnd_haas_f64_dev ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cx', [1, 2])
@pytest.mark.parametrize('ms, width, dc', [(False, None, 0), (True, None, 1), (False, 0.3, 1), (True, 0.3, 0)])
def test_haas(env, cx, ms, width, dc):
    for n in (1, 255, 256, 257, 1001):
        for delay in sorted({0, 1, 255, 256, 257, n, n + 7}):
            for batch, skew in ((1, None), (3, dict(x=4, y=8))):
                where = f'haas n={n} delay={delay} batch={batch} cx={cx} ms={ms} width={width} dc={dc}'
                x = _signals(n + delay + batch, batch, n, cx)
                a = Arena(env.torch, env.dev, x=x, y=((batch, n + delay, 2), np.float64), skew=skew)
                env.native.haas_device(env.ctx, a.ptr('x'), a.ptr('y'), batch, n, cx, delay=delay, delayed_channel=dc, ms_mode=ms,
                                       width=width, stream=env.stream)
                y, _ = a.check(where)
                for b in range(batch):
                    want = O.haas_effect(x[b, :, 0] if cx == 1 else x[b], sample_rate_hz=1, delay_time_seconds=float(delay),
                                         delayed_channel=dc, mode='MS' if ms else 'LR', width=width)
                    assert y[b].tobytes() == want.tobytes(), (where, b, _first_diff(y[b], want))
    FORMS['haas: vnd_haas_f64_dev'].add('delays 0, 1, 255, 256, 257, n, n + 7; float64 poison and guards')


# ---- 4. vnd_white_noise_f32_dev ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cx, c', [(1, 1), (1, 2), (2, 2), (3, 3), (8, 8)])
def test_white_noise(env, cx, c):
    rng = np.random.default_rng(cx * 10 + c)
    for m in (1, 2, 63, 64, 65):
        for n in sorted({m, m + 1, 2047, 2048, 2049, 3 * 2048 + 5}):
            if n < m:
                continue
            for batch, skew in ((1, None), (3, dict(x=4, y=4, h=8))):
                for width, normalize in ((None, OFF), (0.3 if c == 2 else None, RMS)):
                    where = f'white noise M={m} n={n} batch={batch} cx={cx} c={c} width={width} normalize={normalize}'
                    x = rng.standard_normal((batch, n, cx)).astype(np.float32)
                    h = rng.standard_normal((m, c))
                    ws_bytes = env.native.decorrelate_workspace_bytes(batch, n, c)
                    outs = []
                    a = Arena(env.torch, env.dev, x=x, y=((batch, n, c), np.float32), workspace_bytes=ws_bytes, aux={'h': h}, skew=skew)
                    for invert in (False, True):
                        a.reset(invert_workspace=invert)
                        env.native.white_noise_device(env.ctx, a.ptr('x'), a.ptr('h'), a.ptr('y'), batch, n, cx, c, m, width=width,
                                                      normalize=normalize, workspace_ptr=a.ptr('ws'), workspace_bytes=ws_bytes,
                                                      stream=env.stream)
                        outs.append(a.check(where)[0])
                    assert outs[0].tobytes() == outs[1].tobytes(), (where, 'the output depends on what the workspace held')
                    if normalize == OFF:
                        for b in range(batch):
                            _check_bound(outs[0][b], _numpy_conv(x[b], h), x[b], h, where)
    FORMS['white noise: vnd_white_noise_f32_dev'].add(f'{cx} -> {c} channels, workspace of exactly vnd_decorrelate_workspace_bytes()')


def test_white_noise_stage_where_the_convolutions_agree(env):
    """Where the float32 convolution outputs agree with NumPy's the whole stage is bit-identical (include/vnd_amd.h): a FIR and a signal
    of small integers, whose float64 sums are exact in any order."""
    rng = np.random.default_rng(3)
    for n, batch in ((2049, 3), (8193, 1)):
        x = rng.integers(-8, 9, (batch, n, 2)).astype(np.float32)
        h = rng.integers(-4, 5, (65, 2)).astype(np.float64)
        ws_bytes = env.native.decorrelate_workspace_bytes(batch, n, 2)
        a = Arena(env.torch, env.dev, x=x, y=((batch, n, 2), np.float32), workspace_bytes=ws_bytes, aux={'h': h})
        env.native.white_noise_device(env.ctx, a.ptr('x'), a.ptr('h'), a.ptr('y'), batch, n, 2, 2, 65, width=0.3, normalize=RMS,
                                      workspace_ptr=a.ptr('ws'), workspace_bytes=ws_bytes, stream=env.stream)
        y, _ = a.check(f'white noise stage n={n}')
        for b in range(batch):
            want = O.pointwise(x[b], _numpy_conv(x[b], h), False, 0.3)
            O.rms_normalize(x[b], want)
            assert np.array_equal(y[b], want), (n, b, _first_diff(y[b], want))


# ---- 5. vnd_correlogram_f32_dev ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('W, hop, num_lags, n', [(1, 1, 1, 7), (16, 7, 31, 131), (64, 32, 127, 640), (255, 100, 509, 1500),
                                                 (257, 300, 513, 2000), (1025, 2000, 3000, 6000)])
def test_correlogram(env, W, hop, num_lags, n):
    rng = np.random.default_rng(W * 7919 + hop)
    windows = (n - W) // hop + 1
    for batch, pad, skew in ((1, 0, None), (3, 0, dict(x=4, y=8, ysig=4)), (3, 13, None)):
        # stream_stride = n + pad: the padding between two streams holds the guards' NaN, so a read past a stream's end shows
        xs = np.full((batch, n + pad), SENTINEL, np.uint32).view(np.float32)
        ys = xs.copy()
        xs[:, :n] = rng.uniform(-1, 1, (batch, n))
        ys[:, :n] = rng.standard_normal((batch, n))
        where = f'correlogram W={W} hop={hop} lags={num_lags} n={n} batch={batch} stride={n + pad}'
        a = Arena(env.torch, env.dev, x=xs, y=((batch, windows, num_lags), np.float32), aux={'ysig': ys}, skew=skew)
        env.native.correlogram_device(env.ctx, a.ptr('x'), a.ptr('ysig'), a.ptr('y'), batch, n, n + pad, 1, window=W, hop=hop,
                                      num_lags=num_lags, eps=1e-10, stream=env.stream)
        y, _ = a.check(where)
        for b in range(batch):
            R = exact_R(xs[b, :n], ys[b, :n], W, hop, num_lags, 1e-10)
            assert ulps(y[b], R).max(initial=0) <= 1, (where, b)
    FORMS['correlogram: vnd_correlogram_f32_dev'].add('(S, frames, lags) block; a pool with stream_stride > n whose padding is guard pattern')


# ---- 6. the scans and the pair scorers: moments rows, a workspace of exactly *_workspace_bytes() -----------------------------------
def _twice(a, call, where):
    """`call()` on the arena as it is and again with the workspace's bits inverted: the same rows."""
    call()
    first = a.check(where)[0]
    a.reset(invert_workspace=True)
    call()
    second = a.check(where + ' (workspace inverted)')[0]
    assert first.tobytes() == second.tobytes(), (where, 'the rows depend on what the workspace held')
    return first


@pytest.mark.parametrize('pairs, n', [(1, 1), (1, 777), (3, 2049), (63, 1025), (64, 1025), (100, 4099)])
def test_polar_moments(env, pairs, n):
    y = np.random.default_rng(pairs * 1000 + n).uniform(-1, 1, (n, 2 * pairs)).astype(np.float32)
    y[n // 2] = 0.0                                      # a silent frame: r = 0, theta = 0
    if n > 3:
        y[3, 0::2] = -y[3, 1::2]                         # L + R == 0: theta = +-pi/2 exactly, the largest |theta| of every pair
    ws = env.native.polar_moments_workspace_bytes(n, pairs)
    a = Arena(env.torch, env.dev, x=y, y=((pairs, 8), np.float64), workspace_bytes=ws, skew=dict(x=8) if pairs % 2 else None)
    got = _twice(a, lambda: env.native.polar_moments_device(env.ctx, a.ptr('x'), n, pairs, a.ptr('y'), a.ptr('ws'), ws, env.stream),
                 f'polar moments pairs={pairs} n={n}')
    for f in range(pairs):
        want = _moments64(y[:, 2 * f:2 * f + 2])
        scale = _moments64(np.abs(y[:, 2 * f:2 * f + 2]) * np.array([1.0, 0.5], np.float32))
        scale[1:4] = want[0] * np.array([np.pi / 2, (np.pi / 2) ** 2, (np.pi / 2) ** 3])
        assert np.all(np.abs(got[f] - want) <= 3e-8 * np.maximum(scale, 1.0)), (pairs, n, f, got[f], want)
        assert got[f][4] == want[4] or abs(got[f][4] - want[4]) <= 2.4e-7
    FORMS['moments: vnd_polar_moments_f32_dev'].add('lanes along time' if pairs < 64 else 'lanes along candidates (64 pairs and more)')


@pytest.mark.parametrize('n, cx', [(1, 1), (3, 2), (2047, 2), (2048, 1), (2049, 2), (3 * 2048 + 5, 1)])
def test_haas_scan(env, n, cx):
    from vndecorrelate_amd.decorrelation import HaasEffect
    x = _signals(n * 3 + cx, 1, n, cx)[0]
    delays = np.array(sorted({0, 1, 255, 256, 257, n, n + 9, 2000}), np.int32)
    for cfg in (dict(delayed_channel=0, mode='LR', width=None), dict(delayed_channel=1, mode='MS', width=0.35)):
        ws = env.native.haas_scan_workspace_bytes(n, delays.size, int(delays.max()))
        a = Arena(env.torch, env.dev, x=x, y=((delays.size, 8), np.float64), workspace_bytes=ws, aux={'delays': delays},
                  skew=dict(x=4, delays=4) if n % 2 else None)
        got = _twice(a, lambda: env.native.haas_scan_device(env.ctx, a.ptr('x'), n, cx, a.ptr('delays'), delays.size, a.ptr('y'),
                                                            delayed_channel=cfg['delayed_channel'], ms_mode=cfg['mode'] == 'MS',
                                                            width=cfg['width'], workspace_ptr=a.ptr('ws'), workspace_bytes=ws,
                                                            stream=env.stream), f'haas scan n={n} cx={cx} {cfg}')
        for row, d in zip(got, delays):
            want = HaasEffect(sample_rate_hz=1, delay_time_seconds=float(d), **cfg).decorrelate(x[:, 0] if cx == 1 else x)
            check_row(row, want, (n, cx, cfg, int(d)))
    FORMS['moments: vnd_haas_scan_f64_dev'].add('delays 0, 1, 255, 256, 257, n, n + 9, 2000')


@pytest.mark.parametrize('n, cx', [(1, 2), (2047, 1), (2049, 2), (3 * 2048 + 5, 2)])
def test_haas_pairs(env, n, cx):
    """Rows equal the single-signal scan's, bit for bit (tests/test_gpu_haas_search.py's reference), rows of bad pairs are NaN."""
    pool = _signals(n + cx, 3, n, cx)
    delays = np.array([0, 1, 255, 256, 257, n, n + 9, 0, 17, -3, 5], np.int32)
    sig = np.array([0, 1, 2, 0, 1, 2, 0, 1, 3, 2, -1], np.int32)              # pair 8: no such signal; 9: a negative delay; 10: signal -1
    bad = (8, 9, 10)
    kw = dict(delayed_channel=1, ms_mode=True, width=0.35)
    ws = env.native.haas_pairs_workspace_bytes(n, sig.size, n + 9)
    a = Arena(env.torch, env.dev, x=pool, y=((sig.size, 8), np.float64), workspace_bytes=ws, aux={'signals': sig, 'delays': delays},
              skew=dict(signals=4, delays=8))
    got = _twice(a, lambda: env.native.haas_pairs_device(env.ctx, a.ptr('x'), 3, n, cx, a.ptr('signals'), a.ptr('delays'), sig.size,
                                                         a.ptr('y'), workspace_ptr=a.ptr('ws'), workspace_bytes=ws, stream=env.stream,
                                                         **kw), f'haas pairs n={n} cx={cx}')
    for p in range(sig.size):
        if p in bad:
            assert np.isnan(got[p]).all(), (n, cx, p, got[p])
        else:
            want = env.native.haas_scan_host(env.ctx, np.ascontiguousarray(pool[sig[p]]), [int(delays[p])], **kw)[0]
            assert got[p].tobytes() == want.tobytes(), (n, cx, p, got[p], want)
    FORMS['moments: vnd_haas_pairs_f64_dev'].add('11 pairs of 3 signals, three of them out of contract (NaN rows)')


@pytest.mark.parametrize('n, cx', [(1, 2), (200, 1), (2047, 2), (2048, 1), (2049, 2), (3 * 2048 + 5, 1)])
def test_velvet_pairs(env, n, cx):
    """tests/test_gpu_velvet_search.py's two comparisons.  Integer samples and power-of-two gains: slots 5-7 equal NumPy's on the
    oracle's frames bit for bit - any wrong frame shows - and every slot is finite.  Uniform samples (777 frames and more, as there):
    every slot within the moments bound."""
    envelope = (1.0, 0.5, 0.25)
    members = [_taps(0.0, envelope=envelope), _taps(0.6, envelope=envelope), _taps(0.7, filtered=(0, 1), envelope=envelope, seed=5)]
    bank = _class_bank(env.ctx, members, envelope)
    sig = np.array([0, 1, 2, 2, 0, 1, 1], np.int32)
    cand = np.array([0, 1, 2, 0, 2, 0, 1], np.int32)
    ws = env.native.velvet_pairs_workspace_bytes(n, sig.size)
    rng = np.random.default_rng(n + cx)
    try:
        for kind in ('integers', 'uniform'):
            if kind == 'uniform' and n < 777:
                continue
            pool = rng.integers(-3, 4, (3, n, cx)).astype(np.float32) if kind == 'integers' else _signals(n + cx, 3, n, cx)
            a = Arena(env.torch, env.dev, x=pool, y=((sig.size, 8), np.float64), workspace_bytes=ws,
                      aux={'signals': sig, 'candidates': cand}, skew=dict(candidates=4))
            got = _twice(a, lambda: env.native.velvet_pairs_device(env.ctx, bank, a.ptr('x'), 3, n, cx, a.ptr('signals'),
                                                                   a.ptr('candidates'), sig.size, a.ptr('y'), workspace_ptr=a.ptr('ws'),
                                                                   workspace_bytes=ws, stream=env.stream),
                         f'velvet pairs n={n} cx={cx} {kind}')
            for p, (s, c) in enumerate(zip(sig, cand)):
                frames = O.class_convolve(np.repeat(pool[s], 2, axis=1) if cx == 1 else pool[s], members[c], envelope, 2)
                want = _moments64(frames)
                if kind == 'integers':
                    assert got[p][5:].tobytes() == want[5:].tobytes(), (n, cx, p, got[p][5:], want[5:])
                    assert np.all(np.isfinite(got[p])), (n, cx, p, got[p])
                else:
                    scale = _moments64(np.abs(frames) * np.array([1.0, 0.5], np.float32))
                    scale[1:4] = want[0] * np.array([np.pi / 2, (np.pi / 2) ** 2, (np.pi / 2) ** 3])
                    sums = [0, 1, 2, 3, 5, 6, 7]                       # (slot 4 is a maximum: its own bar, one float32 ulp)
                    assert np.all(np.abs(got[p] - want)[sums] <= (3e-8 * np.maximum(scale, 1.0))[sums]), (n, cx, p, got[p], want)
                    assert got[p][4] == want[4] or abs(got[p][4] - want[4]) <= 2.4e-7, (n, cx, p, got[p][4], want[4])
    finally:
        bank.close()
    FORMS['moments: vnd_velvet_pairs_f32_dev'].add('7 pairs of 3 signals and 3 candidates')


# ---- 7. the per-signal entries: vnd_convolve_each_f32_dev, vnd_decorrelate_each_f32_dev, vnd_haas_each_f64_dev -----------------------
EACH_N = (1, 200, 2047, 2048, 2049, 4097, 5001)
EACH_ENVELOPE = (1.0, 0.5, 0.25)


@pytest.fixture(scope='module')
def each_bank(env):
    members = [_taps(0.0, envelope=EACH_ENVELOPE), _taps(0.5, envelope=EACH_ENVELOPE),
               _taps(0.7, filtered=(0, 1), envelope=EACH_ENVELOPE, seed=5)]
    bank = _class_bank(env.ctx, members, EACH_ENVELOPE)
    yield bank, members
    bank.close()


@pytest.mark.parametrize('cx', [1, 2])
@pytest.mark.parametrize('stage', [None, dict(ms_encode=True, width=0.3, normalize=REF), dict(ms_encode=False, width=None, normalize=RMS)],
                         ids=['convolve', 'decorrelate MS width REF', 'decorrelate LR RMS'])
def test_each_velvet(env, each_bank, cx, stage):
    """Odd n with 2 and more signals (rows on 8-byte boundaries), the lengths around the 2048-frame tile, and one table index out
    of contract: that signal's rows NaN, its neighbours' the oracle's, every guard intact."""
    bank, members = each_bank
    for n in EACH_N:
        for tables in ([1], [2, 0, 1], [0, 7, 2], [-1, 1, 0, 2]):
            batch = len(tables)
            where = f'each n={n} cx={cx} tables={tables} stage={stage}'
            pool = _signals(n + batch + cx, batch, n, cx)
            t = np.asarray(tables, np.int32)
            ws = env.native.decorrelate_workspace_bytes(batch, n, 2) if stage else 0
            a = Arena(env.torch, env.dev, x=pool, y=((batch, n, 2), np.float32), workspace_bytes=ws, aux={'tables': t},
                      skew=dict(tables=4) if batch == 1 else dict(x=8, y=8, tables=4) if batch == 3 and 7 in tables else None)

            def call():
                if stage is None:
                    env.native.convolve_each_device(env.ctx, bank, a.ptr('x'), a.ptr('tables'), a.ptr('y'), batch, n, cx, stream=env.stream)
                else:
                    env.native.decorrelate_each_device(env.ctx, bank, a.ptr('x'), a.ptr('tables'), a.ptr('y'), batch, n, cx,
                                                       workspace_ptr=a.ptr('ws'), workspace_bytes=ws, stream=env.stream, **stage)
            got = _twice(a, call, where)
            for b, k in enumerate(tables):
                if not 0 <= k < len(members):
                    assert np.isnan(got[b]).all(), (where, b)
                    continue
                x2 = np.repeat(pool[b], 2, axis=1) if cx == 1 else pool[b]
                want = O.class_convolve(x2, members[k], EACH_ENVELOPE, 2)
                if stage is not None:
                    with np.errstate(all='ignore'):
                        want = O.pointwise(x2, want, stage['ms_encode'], stage['width'])
                        O.rms_normalize(x2, want)
                assert got[b].tobytes() == want.tobytes(), (where, b, _first_diff(got[b], want))
    FORMS['each: vnd_convolve_each_f32_dev' if stage is None else 'each: vnd_decorrelate_each_f32_dev'].add(
        f'{cx} input channels, pools of 1, 3 and 4 signals, one table index out of contract')


@pytest.mark.parametrize('cx', [1, 2])
@pytest.mark.parametrize('ms, width, dc', [(False, None, 0), (True, 0.3, 1)])
def test_each_haas(env, cx, ms, width, dc):
    for n in (1, 255, 256, 257, 2047, 2048, 2049, 4097):
        max_delay = n + 9
        for delays in ([0], [1, 255, 256], [257, n, max_delay], [0, max_delay + 1, 5, -1]):      # the last: two delays out of contract
            batch = len(delays)
            where = f'haas each n={n} cx={cx} delays={delays} ms={ms} width={width} dc={dc}'
            pool = _signals(n + batch + cx, batch, n, cx)
            a = Arena(env.torch, env.dev, x=pool, y=((batch, n + max_delay, 2), np.float64), aux={'delays': np.asarray(delays, np.int32)},
                      skew=dict(x=4, y=8, delays=4) if batch == 3 else None)
            env.native.haas_each_device(env.ctx, a.ptr('x'), a.ptr('y'), batch, n, cx, a.ptr('delays'), max_delay=max_delay,
                                        delayed_channel=dc, ms_mode=ms, width=width, stream=env.stream)
            got, _ = a.check(where)
            for b, d in enumerate(delays):
                if not 0 <= d <= max_delay:
                    assert np.isnan(got[b]).all(), (where, b)
                    continue
                want = O.haas_effect(pool[b, :, 0] if cx == 1 else pool[b], sample_rate_hz=1, delay_time_seconds=float(d),
                                     delayed_channel=dc, mode='MS' if ms else 'LR', width=width)
                assert got[b, :n + d].tobytes() == want.tobytes(), (where, b, _first_diff(got[b, :n + d], want))
                assert got[b, n + d:].tobytes() == np.zeros((max_delay - d, 2)).tobytes(), (where, b)       # padding: +0.0
    FORMS['each: vnd_haas_each_f64_dev'].add(f'{cx} input channels, delays 0, 1, 255, 256, 257, n, max_delay and two out of contract')


# ---- 8. the *_host entries: one test per staging route, after a call that left NaNs in that staging ---------------------------------
def _nan_like(x):
    return np.full_like(x, np.nan)


def test_host_stage_route(env):
    """HostCall::stage keeps the context's staging buffers from call to call: after a same-shape call on an all-NaN input (every
    frame of the staged output a NaN - the table has a tap at offset 0 in every channel) the checked call's output is the oracle's."""
    from vndecorrelate_amd.taps import function_path_arrays
    fir = random_fir(0, np.random.default_rng(1000))             # CASES[0]: a tap at offset 0 in every channel
    arr = function_path_arrays(fir)
    table = env.native.TapTable.create(env.ctx, arr.tap_offsets, arr.tap_index, arr.tap_weight)
    try:
        for cx in (2, 1):
            for batch, n in ((3, 5000), (1, 12345), (2, 2049)):
                x = _signals(n + cx, batch, n, cx)
                assert np.isnan(table.convolve_host(_nan_like(x), EXACT)).all()
                got = table.convolve_host(x, EXACT)
                assert np.array_equal(got, _oracle(arr, x, EXACT)), (cx, batch, n)
                assert np.isnan(table.decorrelate_host(_nan_like(x), EXACT, ms_encode=True, width=0.3, normalize=False)).all()
                got = table.decorrelate_host(x, EXACT, ms_encode=True, width=0.3, normalize=True)
                x2 = _fan(x, 2)
                want = _oracle(arr, x, EXACT)
                for b in range(batch):
                    want[b] = O.pointwise(x2[b], want[b], True, 0.3)
                    O.rms_normalize(x2[b], want[b])
                assert np.array_equal(got, want), ('decorrelate_host', cx, batch, n)
    finally:
        table.close()


def test_host_carve_route(env, each_bank):
    """HostCall::carve hands out x, y, the per-signal integers and the workspace as pieces of ONE buffer the context keeps."""
    bank, members = each_bank
    for cx in (2, 1):
        for batch, n in ((3, 5001), (4, 2048)):
            pool = _signals(n + cx + 50, batch, n, cx)
            tables = [k % 3 for k in range(batch)]
            stage = dict(ms_encode=True, width=0.3, normalize=REF)
            env.native.convolve_each_host(env.ctx, bank, _nan_like(pool), [2] * batch)              # table 2 filters both channels
            got = env.native.convolve_each_host(env.ctx, bank, pool, tables)
            env.native.decorrelate_each_host(env.ctx, bank, _nan_like(pool), [2] * batch, ms_encode=False, width=None, normalize=OFF)
            staged = env.native.decorrelate_each_host(env.ctx, bank, pool, tables, **stage)
            for b, k in enumerate(tables):
                x2 = np.repeat(pool[b], 2, axis=1) if cx == 1 else pool[b]
                want = O.class_convolve(x2, members[k], EACH_ENVELOPE, 2)
                assert got[b].tobytes() == want.tobytes(), ('convolve_each_host', cx, batch, n, b)
                want = O.pointwise(x2, want, True, 0.3)
                O.rms_normalize(x2, want)
                assert staged[b].tobytes() == want.tobytes(), ('decorrelate_each_host', cx, batch, n, b)
            delays = [(7 * b) % 40 for b in range(batch)]
            kw = dict(max_delay=40, delayed_channel=1, ms_mode=True, width=0.3)
            env.native.haas_each_host(env.ctx, _nan_like(pool), delays, **kw)
            rows = env.native.haas_each_host(env.ctx, pool, delays, **kw)
            for b, d in enumerate(delays):
                want = O.haas_effect(pool[b, :, 0] if cx == 1 else pool[b], sample_rate_hz=1, delay_time_seconds=float(d), delayed_channel=1,
                                     mode='MS', width=0.3)
                assert rows[b, :n + d].tobytes() == want.tobytes(), ('haas_each_host', cx, batch, n, b)
                assert not rows[b, n + d:].any()


def test_host_pipelined_routes(env, monkeypatch):
    """The chunked routes: a long stream cut in time (VND_HOST_TIME_PIECES), and a batch cut into groups of streams on two HIP
    streams (16 MB of traffic and more)."""
    from vndecorrelate_amd.taps import function_path_arrays
    fir = random_fir(0, np.random.default_rng(1000))
    arr = function_path_arrays(fir)
    table = env.native.TapTable.create(env.ctx, arr.tap_offsets, arr.tap_index, arr.tap_weight)
    try:
        monkeypatch.setenv('VND_HOST_TIME_PIECES', '3')
        for batch, n in ((1, 8 * 4096 + 77), (2, 10 * 4096 + 1)):
            x = _signals(n, batch, n, 2)
            assert np.isnan(table.convolve_host(_nan_like(x), EXACT)).all()
            assert np.array_equal(table.convolve_host(x, EXACT), _oracle(arr, x, EXACT)), ('time pieces', batch, n)
        monkeypatch.delenv('VND_HOST_TIME_PIECES')
        batch, n = 5, 210001                                     # 16.8 MB of traffic: two groups of streams
        x = _signals(n, batch, n, 2)
        assert np.isnan(table.convolve_host(_nan_like(x), EXACT)).all()
        assert np.array_equal(table.convolve_host(x, EXACT), _oracle(arr, x, EXACT)), ('stream groups', batch, n)
        table.decorrelate_host(_nan_like(x), EXACT, ms_encode=True, width=None, normalize=False)
        got = table.decorrelate_host(x, EXACT, ms_encode=True, width=None, normalize=True)
        want = _oracle(arr, x, EXACT)
        for b in range(batch):
            want[b] = O.pointwise(x[b], want[b], True, None)
            O.rms_normalize(x[b], want[b])
        assert np.array_equal(got, want), ('decorrelate_host, stream groups', batch, n)
    finally:
        table.close()
