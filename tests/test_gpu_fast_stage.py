"""GPU tier: the decorrelate stage in VND_MODE_FAST held BIT FOR BIT to NumPy's epilogue on the kernel's own convolution.

The fast convolution is not the reference's, but everything the stage does after it is (include/vnd_amd.h): for the convolution
``c`` the same table gives under the same variant word and tuning variables (``convolve_device``; an output is a function of the
table and of its position alone within one kernel form), the stage must equal ``pointwise(x, c)`` - the side-channel encode and
the width in the reference's float32 operations - and, under VND_NORMALIZE_RMS_REFERENCE_ORDER, ``rms_normalize(x, pointwise(x,
c))`` with NumPy's own sums of squares.  Every branch of the stage that runs in the fast mode: the window form (32 and 64 frames per
lane, adds per segment on and off, function- and class-path tables, stereo and a mono input fanned out, the balanced cut), the
pair-read kernel, the generic fast kernel at two thread counts and two pair counts, the separate passes, the quad / octet kernels'
sums, NumPy-order sums stitched from the store phase's block sums, ragged and tiny shapes, and the public API.

VND_NORMALIZE_RMS (float64 sums of float32 partials) cannot be NumPy's bits.  There every (stream, channel) must be exactly
``float32(p * s)`` for one float32 scale ``s``, and ``s`` must lie in the interval ``vnd_oracle.rms_scale_bounds`` derives from
the partial length the path's kernel uses (at most ``k`` squares per float32 partial: gamma_k of exact sums, through the
device's own formula) - on adversarial inputs too.

Each case names the branch and the convolution path it took (``vnd_debug_decorrelate_f32_dev``) and checks it is not vacuous:
its ``c`` differs from the exact oracle somewhere and stays within the fast mode's 1e-6 of peak of it."""
import os
import re

import numpy as np
import pytest

from oracle import c_oracle
from oracle import vnd_oracle as O

pytestmark = pytest.mark.gpu

TOL_PEAK = 1e-6
FORCE, NOFUSE, GENERIC = 1 << 23, 1 << 24, 1 << 25
WIN = {0: 1 << 5, 32: 3 << 5, 64: 4 << 5}      # variant bits 5-7: frames per lane (0: the pair-read kernel)
# bits 0-4, frame pairs per lane: the stage fuses its epilogue into the fast launch only where the GENERIC plan of that shape has an
# epilogue instantiation (decorrelate_dev: fast_epi_kernel - 256 threads, 2 / 4 / 8 pairs per lane, an exchange buffer that fits the
# halo), whichever kernel then takes the launch.  Small pools plan 1 pair per lane and large ones 8: both run the separate passes.  A pool
# of 96 streams of 20012 frames plans 2 or 4 and fuses; the pair-count bits would pin the generic plan but also the per-table one.
R4 = 4
POOL, N = 96, 20012                            # (N: the last tile and the last 2048-frame block are partial)
SOME = (0, 1, 2, 47, 95)                       # streams whose VND_NORMALIZE_RMS scales are recovered and bounded
OFF, RMS, REF = 0, 1, 2                        # NORMALIZE_*
STEPS = [(False, None), (True, None), (False, 0.35), (True, 0.35)]
WORST = {}                                     # path -> worst |s - exact| / half-width of its interval (printed at the end)


@pytest.fixture(scope='module')
def env():
    import vndecorrelate_amd.decorrelation as d
    from vndecorrelate_amd import _native
    ctx = _native.default_context()
    assert 'gfx950' in ctx.info()['name']
    yield d, _native, ctx
    ctx.set_variant(-1)
    d.set_default_mode(d.MODE_EXACT)
    if WORST:
        print('\nVND_NORMALIZE_RMS: worst scale error as a fraction of its bound: '
              + ', '.join(f'{k} {v:.3f}' for k, v in sorted(WORST.items())))


def _arrays(golden, kind, channels=2):
    from vndecorrelate_amd.taps import function_path_arrays
    import vndecorrelate_amd.decorrelation as d
    if kind == 'fn':
        return function_path_arrays(golden.fir('g48k_k30'))
    if kind == 'cls':
        return d.VelvetNoise(sample_rate_hz=48000, seed=1)._tap_arrays()
    return d.VelvetNoise(sample_rate_hz=48000, num_outs=channels, num_impulses=30, filtered_channels=tuple(range(channels)),
                         mode='LR', seed=3)._tap_arrays()


def _table(native, ctx, arr):
    return native.TapTable.create(ctx, arr.tap_offsets, arr.tap_index, arr.tap_weight, **arr.kwargs())


def _exact(x2, arr):
    return c_oracle.convolve(x2, arr.tap_offsets, arr.tap_index, arr.tap_weight, seg_off=arr.seg_offsets, seg_end=arr.seg_end,
                             seg_gain=arr.seg_gain, chan_flags=arr.chan_flags, apply_gain=arr.apply_gain, threads=8)


def _fanout(x, C):
    return np.ascontiguousarray(np.tile(x, (1, 1, C // x.shape[-1])))


class _Env:
    """Tuning variables for one launch (VND_TUNING=1 sessions read them live), restored afterwards."""

    def __init__(self, values):
        self.values, self.saved = values or {}, {}

    def __enter__(self):
        for k, v in self.values.items():
            self.saved[k] = os.environ.get(k)
            os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run(env, table, x, *, variant, ms=False, width=None, normalize=OFF, tuning=None):
    """The stage and the plain fast convolution of x ((batch, n, Cx) float32) under one variant word and tuning: (stage output,
    convolution, workspace as float64, taken, describe text)."""
    import torch
    d, native, ctx = env
    batch, n, cx = x.shape
    C = table.num_channels
    st = torch.cuda.current_stream().cuda_stream
    with _Env(tuning):
        ctx.set_variant(variant)
        try:
            xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
            y = torch.full((batch, n, C), float('nan'), dtype=torch.float32, device='cuda')
            c = torch.full((batch, n, C), float('nan'), dtype=torch.float32, device='cuda')
            ws_bytes = native.decorrelate_workspace_bytes(batch, n, C)
            ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device='cuda')        # exactly the declared size, and not zeroed
            taken = table.decorrelate_device_taken(xd.data_ptr(), y.data_ptr(), batch, n, cx, mode=d.MODE_FAST, ms_encode=ms,
                                                   width=width, normalize=normalize, workspace_ptr=ws.data_ptr(),
                                                   workspace_bytes=ws_bytes, stream=st)
            table.convolve_device(xd.data_ptr(), c.data_ptr(), batch, n, cx, d.MODE_FAST, st)
            text = table.describe(batch, n, cx, d.MODE_FAST)
            torch.cuda.synchronize()
        finally:
            ctx.set_variant(-1)
    return y.cpu().numpy(), c.cpu().numpy(), ws[:ws_bytes // 8 * 8].view(torch.float64).cpu().numpy(), taken, text


def _seq_sums(a):
    """NumPy's axis-0 float32 reduction for (n, C >= 2): a sequential recurrence per channel."""
    with np.errstate(all='ignore'):
        return np.cumsum(np.square(a), axis=0, dtype=np.float32)[-1] if len(a) else np.zeros(a.shape[1], np.float32)


def _nonvacuous(c, exact, tag):
    fin = np.isfinite(exact).all(axis=(1, 2))
    assert not np.array_equal(c, exact, equal_nan=True), ('the fast convolution is the exact one', tag)
    peak = float(np.max(np.abs(exact[fin]))) or 1.0
    err = float(np.max(np.abs(c[fin].astype(np.float64) - exact[fin]))) / peak
    assert err <= TOL_PEAK, (tag, err)


def _rms_check(x2, p, y, k, tag):
    """VND_NORMALIZE_RMS: y == float32(p * s) frame by frame for one float32 s per (stream, channel), s within the bound of
    float32 partials of at most k squares.  Returns the worst |s - exact| / half-width seen."""
    worst = 0.0
    for b in (SOME if len(x2) > max(SOME) else range(len(x2))):
        lo, exact, hi = O.rms_scale_bounds(x2[b], p[b], k)
        for ch in range(p.shape[-1]):
            pc, yc = p[b, :, ch], y[b, :, ch]
            use = (pc != 0) & np.isfinite(pc)
            if not use.any():
                s = np.float32(0.0)
            else:
                s = np.float32(np.median(yc[use].astype(np.float64) / pc[use]))
            found = None
            for step in (0, -1, 1, -2, 2, -3, 3):
                cand = np.float32(s)
                for _ in range(abs(step)):
                    cand = np.nextafter(cand, np.float32(np.inf if step > 0 else -np.inf))
                if np.array_equal((pc * cand).astype(np.float32), yc, equal_nan=True):
                    found = cand
                    break
            assert found is not None, (tag, b, ch, 'no one float32 scale gives the output')
            if use.any():
                assert lo[ch] <= found <= hi[ch], (tag, b, ch, float(found), float(lo[ch]), float(hi[ch]))
                half = max(float(hi[ch]) - float(exact[ch]), float(exact[ch]) - float(lo[ch]))
                if half > 0:
                    worst = max(worst, abs(float(found) - float(exact[ch])) / half)
    WORST[tag] = max(WORST.get(tag, 0.0), worst)
    return worst


def _expect(x, y, c, ws, taken, *, ms, width, normalize, k=None, tag=''):
    """The stage's output against NumPy's epilogue on the kernel's own convolution c."""
    C = c.shape[-1]
    x2 = _fanout(x, C)
    p = np.stack([O.pointwise(x2[b], c[b], ms, width) for b in range(len(x))]) if (ms or width is not None) else c
    if normalize == OFF:
        assert np.array_equal(y, p, equal_nan=True), tag
    elif normalize == REF:
        want = p.copy()
        with np.errstate(all='ignore'):
            for b in range(len(x)):
                O.rms_normalize(x2[b], want[b])
        bad = [b for b in range(len(x)) if not np.array_equal(y[b], want[b], equal_nan=True)]
        assert not bad, (tag, bad[:8])
        sums = ws[:2 * C * len(x)].reshape(len(x), 2 * C).astype(np.float32)
        for b in range(len(x)):
            assert np.array_equal(sums[b], np.concatenate([_seq_sums(x2[b]), _seq_sums(p[b])]), equal_nan=True), (tag, b)
    else:
        _rms_check(x2, p, y, k, tag)


def _partial_len(taken, text):
    """Squares per float32 partial of the path that formed VND_NORMALIZE_RMS's sums (csrc: the window kernel's store phase adds a
    lane's frames_per_lane outputs, the generic fast kernel 2 x pairs_per_lane per lane, epilogue_pointwise_kernel 16 per thread)."""
    if taken['branch'] == 'table-order' or taken['conv_path'] == 2:
        return 16
    if taken['conv_path'] == 1:
        return int(re.search(r'frames_per_lane=(\d+)', text).group(1))
    return 2 * int(re.search(r'pairs_per_lane=(\d+)', text).group(1))


def _signals(seed, batch, n, cx):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (batch, n, cx)).astype(np.float32)


# ---- the window form (conv_path 1 where it leaves the sums) ---------------------------------------------------------------
@pytest.mark.parametrize('kind,adds', [('fn', '1'), ('cls', '1'), ('cls', '0')])     # (adds per segment: class-path tables only)
@pytest.mark.parametrize('fpl', [32, 64])
@pytest.mark.parametrize('cx', [2, 1])
def test_window_form(env, golden, kind, fpl, adds, cx):
    d, native, ctx = env
    arr = _arrays(golden, kind)
    table = _table(native, ctx, arr)
    x = _signals(fpl + cx + (kind == 'fn'), POOL, N, cx)
    exact = _exact(_fanout(x, 2), arr)
    variant, tuning = FORCE | WIN[fpl], {'VND_WIN_ADDS': adds}
    try:
        for normalize in (OFF, REF, RMS):
            for ms, width in STEPS:
                if normalize == OFF and not ms and width is None:
                    continue
                tag = f'window{fpl}/{kind}/adds{adds}/cx{cx}/{normalize}/{ms}/{width}'
                y, c, ws, taken, text = _run(env, table, x, variant=variant, ms=ms, width=width, normalize=normalize, tuning=tuning)
                assert text.startswith('conv_spec_window') and f'frames_per_lane={fpl} ' in text, (tag, text)
                if kind == 'cls':
                    assert text.endswith('taps=adds-per-segment') == (adds == '1'), (tag, text)
                steps = ms or width is not None
                if normalize == REF and not steps:
                    assert taken['branch'] == 'table-order' and taken['conv_path'] == 0, (tag, taken)
                else:
                    assert taken['branch'] == 'fused', (tag, taken)
                    sums_here = (normalize == RMS) or (normalize == REF and taken['blk_done'])
                    assert taken['conv_path'] == (1 if sums_here and fpl == 32 else 2), (tag, taken)
                    if normalize == REF:
                        assert taken['numpy_order'] and taken['blk_done'] == (fpl == 32), (tag, taken)
                _nonvacuous(c, exact, tag)
                _expect(x, y, c, ws, taken, ms=ms, width=width, normalize=normalize, k=_partial_len(taken, text),
                        tag=f'window{fpl}' if normalize == RMS else tag)
    finally:
        table.close()


# ---- the balanced cut: same bits as the uniform spans, and NumPy's epilogue ---------------------------------------------------
@pytest.mark.parametrize('pool,n', [(7, 3 * 8192 + 50), (13, 8192 * 2), (5, 70000), (POOL, N), (192, N)])
def test_balanced_cut(env, golden, pool, n):
    d, native, ctx = env
    arr = _arrays(golden, 'cls')
    table = _table(native, ctx, arr)
    x = _signals(pool * 7 + n % 13, pool, n, 2)
    exact = _exact(x, arr)
    try:
        for normalize, ms, width in ((OFF, True, 0.35), (REF, True, None), (REF, False, 0.35), (RMS, True, 0.35), (RMS, False, None)):
            outs = {}
            for bal in ('2', '0'):
                tag = f'balanced/{pool}x{n}/{bal}/{normalize}/{ms}/{width}'
                y, c, ws, taken, text = _run(env, table, x, variant=FORCE | WIN[32], ms=ms, width=width, normalize=normalize,
                                             tuning={'VND_WIN_BALANCE': bal})
                assert ('balanced ranges' in text) == (bal == '2'), (tag, text)
                # (the small ragged pools plan 1 pair per lane: the window kernel's plain launch and the separate passes)
                if (pool, n) == (POOL, N):
                    assert taken['branch'] == 'fused', (tag, taken)
                if taken['branch'] == 'fused':
                    # (the sums leave the store phase: the fused float64 rows, or the block sums NumPy's order starts from)
                    assert taken['conv_path'] == (2 if normalize == OFF else 1) and taken['blk_done'] == (normalize == REF), (tag, taken)
                else:
                    assert taken['branch'] == 'table-order' and taken['conv_path'] == 0, (tag, taken)
                _nonvacuous(c, exact, tag)
                _expect(x, y, c, ws, taken, ms=ms, width=width, normalize=normalize, k=_partial_len(taken, text),
                        tag='window32-balanced' if normalize == RMS else tag)
                outs[bal] = (y, c)
            assert np.array_equal(outs['2'][1], outs['0'][1]) and np.array_equal(outs['2'][0], outs['0'][0]), tag
    finally:
        table.close()


# ---- the pair-read kernel (conv_path 2: the sums in one more pass) ---------------------------------------------------------
@pytest.mark.parametrize('cx', [2, 1])
def test_pair_read(env, golden, cx):
    d, native, ctx = env
    arr = _arrays(golden, 'fn')
    table = _table(native, ctx, arr)
    x = _signals(40 + cx, POOL, N, cx)
    exact = _exact(_fanout(x, 2), arr)
    try:
        for normalize in (OFF, REF, RMS):
            for ms, width in STEPS:
                if normalize == OFF and not ms and width is None:
                    continue
                tag = f'pair_read/cx{cx}/{normalize}/{ms}/{width}'
                y, c, ws, taken, text = _run(env, table, x, variant=FORCE | WIN[0], ms=ms, width=width, normalize=normalize)
                assert text.startswith('conv_spec (') and 'pairs_per_lane=' in text, (tag, text)
                if normalize == REF and not (ms or width is not None):
                    assert taken['branch'] == 'table-order' and taken['conv_path'] == 0, (tag, taken)
                else:
                    assert taken['branch'] == 'fused' and taken['conv_path'] == 2, (tag, taken)
                _nonvacuous(c, exact, tag)
                _expect(x, y, c, ws, taken, ms=ms, width=width, normalize=normalize, k=_partial_len(taken, text),
                        tag='pair_read' if normalize == RMS else tag)
    finally:
        table.close()


# ---- the generic fast kernel (conv_path 0, one row of sums per tile) --------------------------------------------------------
@pytest.mark.parametrize('nt', [0, 1])                 # bits 16-17: 256 / 128 threads (the epilogue instantiations have 256)
@pytest.mark.parametrize('pairs', [2, 4])              # bits 0-4: frame pairs per lane
def test_generic_fast_kernel(env, golden, nt, pairs):
    d, native, ctx = env
    arr = _arrays(golden, 'cls')
    table = _table(native, ctx, arr)
    batch, n = 4, 30011 + 1
    x = _signals(50 + nt * 10 + pairs, batch, n, 2)
    exact = _exact(x, arr)
    variant = GENERIC | (nt << 16) | pairs
    try:
        for normalize in (OFF, REF, RMS):
            for ms, width in STEPS:
                if normalize == OFF and not ms and width is None:
                    continue
                tag = f'generic/nt{nt}/r{pairs}/{normalize}/{ms}/{width}'
                y, c, ws, taken, text = _run(env, table, x, variant=variant, ms=ms, width=width, normalize=normalize)
                assert text.startswith('conv_fast ') and f'pairs_per_lane={pairs} ' in text, (tag, text)
                expect_branch = 'table-order' if (normalize == REF and not (ms or width is not None)) or nt else 'fused'
                assert taken['branch'] == expect_branch and taken['conv_path'] == 0, (tag, taken)
                _nonvacuous(c, exact, tag)
                _expect(x, y, c, ws, taken, ms=ms, width=width, normalize=normalize, k=_partial_len(taken, text),
                        tag=f'generic/r{pairs}' if normalize == RMS else tag)
    finally:
        table.close()


# ---- not fused: the plain launch and the separate passes --------------------------------------------------------------------
@pytest.mark.parametrize('conv', ['window', 'generic'])
def test_separate_passes(env, golden, conv):
    d, native, ctx = env
    arr = _arrays(golden, 'fn')
    table = _table(native, ctx, arr)
    batch, n = 3, 50000 + 74
    x = _signals(61, batch, n, 2)
    exact = _exact(x, arr)
    variant = NOFUSE | (FORCE | WIN[32] if conv == 'window' else GENERIC)
    try:
        for normalize in (OFF, REF, RMS):
            for ms, width in STEPS:
                if normalize == OFF and not ms and width is None:
                    continue
                tag = f'nofuse/{conv}/{normalize}/{ms}/{width}'
                y, c, ws, taken, text = _run(env, table, x, variant=variant, ms=ms, width=width, normalize=normalize)
                assert text.startswith('conv_spec_window' if conv == 'window' else 'conv_fast '), (tag, text)
                assert taken['branch'] == 'table-order' and taken['conv_path'] == 0, (tag, taken)
                _nonvacuous(c, exact, tag)
                _expect(x, y, c, ws, taken, ms=ms, width=width, normalize=normalize, k=16,
                        tag='nofuse' if normalize == RMS else tag)
    finally:
        table.close()


# ---- wider tables: the quad / octet kernels' sums (q_done), and NumPy-order sums in table order --------------------------------
@pytest.mark.parametrize('channels', [4, 6, 8, 16])
def test_wide_tables(env, golden, channels):
    d, native, ctx = env
    arr = _arrays(golden, 'lr', channels)
    table = _table(native, ctx, arr)
    batch, n = 3, 60000 + 78                              # even: 16-byte aligned streams
    x = _signals(70 + channels, batch, n, channels)
    x[1] = (np.round(x[1] * 20000) / 32768.0).astype(np.float32)      # 16-bit audio: ties in NumPy's sums
    x[2, :, channels - 1] = 0.0                                        # a silent channel
    exact = _exact(x, arr)
    try:
        for normalize in (REF, RMS):
            if normalize == RMS and channels % 4:
                continue
            tag = f'wide/c{channels}/{normalize}'
            y, c, ws, taken, text = _run(env, table, x, variant=FORCE, normalize=normalize)
            if normalize == RMS:
                assert 'pieces=channel-' in text, (tag, text)
                assert taken['branch'] == 'q_done' and taken['conv_path'] == 1, (tag, taken)
            else:
                assert taken['branch'] == 'table-order' and taken['conv_path'] == 0 and taken['numpy_order'], (tag, taken)
            _nonvacuous(c, exact, tag)
            _expect(x, y, c, ws, taken, ms=False, width=None, normalize=normalize, k=_partial_len(taken, text),
                    tag=f'q_done/c{channels}' if normalize == RMS else tag)
    finally:
        table.close()


# ---- NumPy-order sums stitched from the fast store phase's block sums -----------------------------------------------------------
@pytest.mark.parametrize('pool', [POOL, 255])
def test_numpy_order_sums_from_fast_block_sums(env, golden, pool):
    d, native, ctx = env
    arr = _arrays(golden, 'cls')
    table = _table(native, ctx, arr)
    n = 20000 + 37 * 2
    rng = np.random.default_rng(pool)
    x = rng.uniform(-1, 1, (pool, n, 2)).astype(np.float32)
    x[1] = np.round(x[1] * 32767) / 32768                          # ties in most blocks
    x[2, :9000] = 0                                                # silent start
    x[3] *= np.linspace(0.001, 40, n, dtype=np.float32)[:, None]   # binade crossings late in the signal
    x[4] *= 1e-4
    x[5, 12345, 0] = np.inf
    x[6, 4321, 1] = np.nan
    exact = _exact(x, arr)
    try:
        outs = {}
        for label, tuning in (('block sums', None), ('block sums off', {'VND_EPI_BLOCK_SUMS': '0'})):
            for ms, width in STEPS[1:]:
                tag = f'blk/{pool}/{label}/{ms}/{width}'
                with np.errstate(all='ignore'):
                    y, c, ws, taken, text = _run(env, table, x, variant=FORCE | WIN[32], ms=ms, width=width, normalize=REF,
                                                 tuning=tuning)
                assert text.startswith('conv_spec_window') and 'frames_per_lane=32 ' in text, (tag, text)
                on = tuning is None
                assert taken['branch'] == 'fused' and taken['numpy_order'] and taken['blk_done'] == on, (tag, taken)
                assert taken['conv_path'] == (1 if on else 2), (tag, taken)
                _nonvacuous(c, exact, tag)
                with np.errstate(all='ignore'):
                    _expect(x, y, c, ws, taken, ms=ms, width=width, normalize=REF, tag=tag)
                outs[(label, ms, width)] = y
        for ms, width in STEPS[1:]:
            assert np.array_equal(outs[('block sums', ms, width)], outs[('block sums off', ms, width)], equal_nan=True)
    finally:
        table.close()


# ---- shapes at the edges --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('batch,n,cx', [(2, 1, 2), (3, 500, 2), (2, 1999, 2), (3, 4001, 1), (4, 30011, 2), (1, 2048 * 3, 2)])
@pytest.mark.parametrize('variant', [-1, FORCE | WIN[32]])
def test_edge_shapes(env, golden, batch, n, cx, variant):
    d, native, ctx = env
    arr = _arrays(golden, 'fn')
    table = _table(native, ctx, arr)
    x = _signals(n + batch, batch, n, cx)
    exact = _exact(_fanout(x, 2), arr)
    try:
        for normalize, ms, width in ((OFF, True, 0.35), (REF, True, 0.35), (REF, False, None), (RMS, False, 0.35)):
            tag = f'edge/{batch}x{n}x{cx}/{variant}/{normalize}'
            y, c, ws, taken, text = _run(env, table, x, variant=variant, ms=ms, width=width, normalize=normalize)
            # (which branch these shapes take depends on the generic plan: named, and held to the same bits either way)
            assert taken['branch'] in ('fused', 'table-order'), (tag, taken)
            if normalize == REF and not (ms or width is not None):
                assert taken['branch'] == 'table-order', (tag, taken, text)
            if n > 1:
                _nonvacuous(c, exact, tag)
            _expect(x, y, c, ws, taken, ms=ms, width=width, normalize=normalize, k=_partial_len(taken, text),
                    tag='edges' if normalize == RMS else tag)
    finally:
        table.close()


def test_denormal_range_input(env, golden):
    d, native, ctx = env
    arr = _arrays(golden, 'fn')
    table = _table(native, ctx, arr)
    x = (_signals(81, POOL, N, 2).astype(np.float64) * 3e-38).astype(np.float32)
    assert np.any((np.abs(x) < np.finfo(np.float32).tiny) & (x != 0))
    try:
        for variant in (FORCE | WIN[32], GENERIC | R4):
            for normalize, ms, width in ((OFF, True, 0.35), (REF, True, 0.35)):
                tag = f'denormal/{variant}/{normalize}'
                y, c, ws, taken, text = _run(env, table, x, variant=variant, ms=ms, width=width, normalize=normalize)
                assert taken['branch'] == 'fused', (tag, taken)
                assert np.any((np.abs(c) < np.finfo(np.float32).tiny) & (c != 0)), tag
                _expect(x, y, c, ws, taken, ms=ms, width=width, normalize=normalize, tag=tag)
    finally:
        table.close()


# ---- VND_NORMALIZE_RMS on inputs that drive the float32 partials' rounding one way ------------------------------------------------
def _adversarial(n):
    one = np.float32(1 + 2.0 ** -12)
    pool = lambda a: np.ascontiguousarray(np.broadcast_to(a, (POOL,) + a.shape))     # (a pool that fuses: see R4)
    yield 'constant_magnitude', pool(np.tile(np.array([one, -one], np.float32), (n, 1)))
    dom = np.full((n, 2), np.float32(1 + 2.0 ** -11))
    dom[::16] = np.float32(4097.0)                        # one dominant sample in every run of 16, 32 or 64 frames
    yield 'dominant_per_run', pool(dom)
    alt = np.ones((n, 2), np.float32) * np.float32(1 + 2.0 ** -10)
    alt[1::2] *= np.float32(3.0)
    yield 'alternating', pool(alt)


@pytest.mark.parametrize('path,variant', [('window32', FORCE | WIN[32]), ('window64', FORCE | WIN[64]),
                                          ('pair_read', FORCE | WIN[0]), ('generic/r4', GENERIC | R4), ('nofuse', NOFUSE | GENERIC | R4)])
def test_rms_scale_bound_on_adversarial_inputs(env, golden, path, variant):
    d, native, ctx = env
    arr = _arrays(golden, 'fn')
    table = _table(native, ctx, arr)
    try:
        for name, x in _adversarial(N):
            for ms, width in ((False, None), (False, 0.35)):
                tag = f'{path}/{name}/{width}'
                y, c, ws, taken, text = _run(env, table, np.ascontiguousarray(x), variant=variant, ms=ms, width=width, normalize=RMS)
                assert taken['branch'] == ('table-order' if variant & NOFUSE else 'fused'), (tag, taken)
                _expect(x, y, c, ws, taken, ms=ms, width=width, normalize=RMS, k=_partial_len(taken, text), tag=path)
    finally:
        table.close()


# ---- the public API under set_default_mode(MODE_FAST) -----------------------------------------------------------------------------
def test_public_api(env):
    d, native, ctx = env
    x = _signals(91, 3, 48000 + 11, 2)
    d.set_default_mode(d.MODE_FAST)
    try:
        vn = d.VelvetNoise(sample_rate_hz=48000, seed=1, width=0.35)
        table = vn._device_table()
        ms = vn.mode == d.LayoutMode.MS
        c = table.convolve_host(x, d.MODE_FAST)
        want = np.stack([O.pointwise(x[b], c[b], ms, 0.35) for b in range(3)])
        for b in range(3):
            O.rms_normalize(x[b], want[b])
        assert np.array_equal(vn.decorrelate_batched(x), want)
        c1 = table.convolve_host(np.ascontiguousarray(x[0]), d.MODE_FAST)
        w1 = O.pointwise(x[0], c1, ms, 0.35)
        O.rms_normalize(x[0], w1)
        assert np.array_equal(vn.decorrelate(x[0]), w1)
        chain = d.SignalChain(sample_rate_hz=48000, device_resident=True).velvet_noise(seed=1, width=0.35)
        assert np.array_equal(chain(x[0]), w1)
        # mono: fanned out on the device, as the reference's mono_to_stereo
        xm = np.ascontiguousarray(x[1, :, 0])
        cm = table.convolve_host(np.ascontiguousarray(xm[:, None]), d.MODE_FAST)
        x2 = np.column_stack((xm, xm))
        wm = O.pointwise(x2, cm, ms, 0.35)
        O.rms_normalize(x2, wm)
        assert np.array_equal(vn.decorrelate(xm), wm)
    finally:
        d.set_default_mode(d.MODE_EXACT)
