"""GPU tier: VND_MODE_FMA against its definition (include/vnd_amd.h: ``acc = fma(x, w, acc)`` in table order, one rounding
per tap), BIT FOR BIT, on every kernel that runs the fma arithmetic - the generic ordered kernel (every tile size, mono
fan-out, the pointwise-epilogue form of the decorrelate stage), the direct kernel (long FIRs), the stream kernel and the
stream's direct variant.  The reference is ``oracle.c_oracle.convolve_fma`` (held to ``vnd_oracle.convolve_taps_fma`` and
to exact rational arithmetic on the CPU tier).  Each case also checks that its fma reference differs from the exact
oracle on its input - a kernel running the exact arithmetic under MODE_FMA must fail here - unless power-of-two weights,
an empty signal or a lone nonzero sample make the two arithmetics one by design; and it names the kernel that ran (never a per-table
``conv_spec*`` kernel: those have no fma form)."""
import json
import pathlib

import numpy as np
import pytest

from conftest import make_input
from oracle import c_oracle
from oracle import vnd_oracle as O

pytestmark = pytest.mark.gpu

MANIFEST = json.loads((pathlib.Path(__file__).parent / 'golden' / 'manifest.json').read_text())
FN_CASES = sorted(n for n, m in MANIFEST['fn'].items()
                  if 'f64' not in n and m['input'].get('dtype', 'float32') == 'float32')
# where the fma and exact arithmetics agree on every output by design: no outputs (n0), no tap inside the signal (n1), one
# nonzero input sample (impulse), +-1 weights (noenv), power-of-two weights (long_fir: 1, 0.5, 0.25 - every product exact)
FMA_IS_EXACT = {'fn_n0', 'fn_n1', 'fn_impulse', 'fn_noenv', 'fn_long_fir'}


@pytest.fixture(scope='module')
def vnd():
    import vndecorrelate_amd.decorrelation as d
    from vndecorrelate_amd import _native
    ctx = _native.default_context()
    assert 'gfx950' in ctx.info()['name']
    yield d
    ctx.set_variant(-1)
    d.set_default_mode(d.MODE_EXACT)


def _table(arr):
    from vndecorrelate_amd import _native
    return _native.TapTable.create(_native.default_context(), arr.tap_offsets, arr.tap_index, arr.tap_weight, **arr.kwargs())


def _refs(x, arr):
    """(fma reference, exact oracle) of a table's convolution of x ((n, C) or (B, n, C) float32)."""
    args = (x, arr.tap_offsets, arr.tap_index, arr.tap_weight)
    kw = dict(seg_off=arr.seg_offsets, seg_end=arr.seg_end, seg_gain=arr.seg_gain, chan_flags=arr.chan_flags,
              apply_gain=arr.apply_gain, threads=8)
    return c_oracle.convolve_fma(*args, **kw), c_oracle.convolve(*args, **kw)


def _generic(text, family='conv_'):
    assert text.startswith(family) and not text.startswith('conv_spec') and 'mode=1' in text, text
    return text


def _replicate(x, channels):
    return np.ascontiguousarray(np.tile(x, (1,) * (x.ndim - 1) + (channels // x.shape[-1],)))


# ---- a. every float32 function-path golden through convolve_velvet_noise --------------------------------------------
@pytest.mark.parametrize('name', FN_CASES)
def test_function_path_goldens(vnd, golden, name):
    from vndecorrelate_amd.taps import function_path_arrays
    meta = golden.manifest['fn'][name]
    x = make_input(meta['input'])
    fir = golden.fir(meta['generator'])
    arr = function_path_arrays(fir)
    want, exact = _refs(x.astype(np.float32), arr)
    if x.ndim == 3:
        got = vnd.convolve_velvet_noise_batched(x, fir, mode=vnd.MODE_FMA)
    else:
        got = vnd.convolve_velvet_noise(x, fir, mode=vnd.MODE_FMA)
    assert got.dtype == np.float32 and np.array_equal(got, want), name
    assert np.array_equal(want, exact) == (name in FMA_IS_EXACT), name
    if x.shape[-2]:
        table = _table(arr)
        batch = x.shape[0] if x.ndim == 3 else 1
        _generic(table.describe(batch, x.shape[-2], x.shape[-1], vnd.MODE_FMA))
        table.close()


# ---- f. long FIRs: the direct kernel (2 s) --------------------------------------------------------------------------
def test_long_fir_direct_kernel(vnd):
    from vndecorrelate_amd.taps import function_path_arrays
    fir = vnd.generate_velvet_noise(duration_seconds=2.0, num_impulses=40, sample_rate_hz=48000, seed=4)
    x = make_input(dict(seed=2, shape=[150000, 2]))
    arr = function_path_arrays(fir)
    table = _table(arr)
    _generic(table.describe(1, 150000, 2, vnd.MODE_FMA), 'conv_direct')
    want, exact = _refs(x, arr)
    assert not np.array_equal(want, exact)
    assert np.array_equal(vnd.convolve_velvet_noise(x, fir, mode=vnd.MODE_FMA), want)
    assert np.array_equal(table.convolve_host(x[None], vnd.MODE_FMA)[0], want)
    table.close()


# ---- g. non-finite weights: the direct kernel, finite outputs bit for bit ------------------------------------------------
def test_non_finite_weights_bit_exact_where_finite(vnd):
    """Irregular weights around the inf / NaN taps, so that the finite outputs hold several rounded terms."""
    from vndecorrelate_amd.taps import function_path_arrays
    fir = np.zeros((64, 2), np.float32)
    fir[[1, 3, 5, 9, 40, 44], 0] = [0.5, 0.3141, np.inf, -0.7071, -0.25, 0.1234]
    fir[[0, 2, 17, 30, 33], 1] = [1.0, -0.377, np.nan, 0.618, -0.45]
    x = np.random.default_rng(9).uniform(0.1, 1, (3000, 2)).astype(np.float32)
    arr = function_path_arrays(fir)
    table = _table(arr)
    _generic(table.describe(1, 3000, 2, vnd.MODE_FMA), 'conv_direct')
    with np.errstate(all='ignore'):
        want, exact = _refs(x, arr)
        ref = O.convolve_velvet_noise(x, fir)
    got = vnd.convolve_velvet_noise(x, fir, mode=vnd.MODE_FMA)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref))
    assert np.array_equal(got, want, equal_nan=True)
    assert fin[-5:].all() and not np.array_equal(want[fin], exact[fin])
    table.close()


# ---- f. 0.1-0.7 s FIRs: LDS windows past 64 KB, the ordered kernel ----------------------------------------------------
@pytest.mark.parametrize('seconds', [0.1, 0.25, 0.4, 0.7])
def test_mid_length_firs(vnd, seconds):
    from vndecorrelate_amd.taps import function_path_arrays
    fir = vnd.generate_velvet_noise(duration_seconds=seconds, num_impulses=40, sample_rate_hz=48000, seed=6)
    x = make_input(dict(seed=9, shape=[2, 90001, 2]))
    arr = function_path_arrays(fir)
    table = _table(arr)
    _generic(table.describe(2, 90001, 2, vnd.MODE_FMA), 'conv_ordered')
    want, exact = _refs(x, arr)
    assert not np.array_equal(want, exact)
    assert np.array_equal(table.convolve_host(x, vnd.MODE_FMA), want), seconds
    table.close()


# ---- e. mono fan-out: every tile size, misaligned device pointers ---------------------------------------------------------
def test_mono_fanout_every_tile_size(vnd, golden):
    from vndecorrelate_amd import _native
    from vndecorrelate_amd.taps import function_path_arrays
    ctx = _native.default_context()
    arr = function_path_arrays(golden.fir('g48k_k30'))
    table = _table(arr)
    x = make_input(dict(seed=41, shape=[5, 20011, 1]))
    want, exact = _refs(_replicate(x, 2), arr)
    assert not np.array_equal(want, exact)
    try:
        for pairs in (1, 2, 4, 8):
            ctx.set_variant(pairs)
            text = _generic(table.describe(5, 20011, 1, vnd.MODE_FMA), 'conv_ordered_fanout')
            assert f'pairs_per_lane={pairs} ' in text, text
            assert np.array_equal(table.convolve_host(x, vnd.MODE_FMA), want), pairs
        ctx.set_variant(1 << 12)
        _generic(table.describe(5, 20011, 1, vnd.MODE_FMA), 'conv_direct')
        assert np.array_equal(table.convolve_host(x, vnd.MODE_FMA), want)
    finally:
        ctx.set_variant(-1)
        table.close()


def test_mono_fanout_misaligned_device_pointers(vnd, golden):
    import torch
    from vndecorrelate_amd.taps import function_path_arrays
    arr = function_path_arrays(golden.fir('g48k_k30'))
    table = _table(arr)
    n, batch = 9001, 3
    x = make_input(dict(seed=46, shape=[batch, n, 1]))
    want, exact = _refs(_replicate(x, 2), arr)
    assert not np.array_equal(want, exact)
    _generic(table.describe(batch, n, 1, vnd.MODE_FMA), 'conv_ordered_fanout')
    stream = torch.cuda.current_stream().cuda_stream
    for shift in (0, 1, 2, 3):
        xin = torch.zeros(x.size + 8, dtype=torch.float32, device='cuda:0')
        yout = torch.full((want.size + 8,), 7.0, dtype=torch.float32, device='cuda:0')
        xin[shift:shift + x.size] = torch.from_numpy(x.ravel()).cuda()
        table.convolve_device(xin.data_ptr() + 4 * shift, yout.data_ptr() + 4 * shift, batch, n, 1, vnd.MODE_FMA, stream)
        torch.cuda.synchronize()
        got = yout.cpu().numpy()
        assert np.array_equal(got[shift:shift + want.size].reshape(want.shape), want), shift
        assert np.all(got[:shift] == 7.0) and np.all(got[shift + want.size:] == 7.0), shift
    table.close()


# ---- h. the decorrelate stage in fma mode on a function-path table ------------------------------------------------------
def _pointwise(x2, y, ms_encode, width):
    """The stage's pointwise steps on a (n, 2) convolution, in the reference's operations (utils/dsp.py)."""
    y = y.copy()
    if ms_encode:
        O.encode_side(x2, y)
    if width is not None:
        O.apply_stereo_width(y, width)
    return y


@pytest.mark.parametrize('cx', [2, 1])
def test_decorrelate_stage(vnd, golden, cx):
    from vndecorrelate_amd import _native
    from vndecorrelate_amd.taps import function_path_arrays
    ctx = _native.default_context()
    arr = function_path_arrays(golden.fir('g48k_k30'))
    table = _table(arr)
    batch, n = 3, 30011                                  # ragged: neither the tile nor the 2048-frame block divides it
    x = make_input(dict(seed=47 + cx, shape=[batch, n, cx]))
    x2 = _replicate(x, 2)
    conv, exact = _refs(x2, arr)
    assert not np.array_equal(conv, exact)
    family = 'conv_ordered_fanout' if cx == 1 else 'conv_ordered'
    try:
        for pairs in (-1, 1, 4):
            ctx.set_variant(pairs)
            text = _generic(table.describe(batch, n, cx, vnd.MODE_FMA), family)
            assert pairs < 0 or f'pairs_per_lane={pairs} ' in text, text
            for ms_encode in (False, True):
                for width in (None, 0.4):
                    tag = (cx, pairs, ms_encode, width)
                    got = table.decorrelate_host(x, vnd.MODE_FMA, ms_encode=ms_encode, width=width,
                                                 normalize=_native.NORMALIZE_RMS_REFERENCE_ORDER)
                    off = table.decorrelate_host(x, vnd.MODE_FMA, ms_encode=ms_encode, width=width,
                                                 normalize=_native.NORMALIZE_OFF)
                    rms = table.decorrelate_host(x, vnd.MODE_FMA, ms_encode=ms_encode, width=width,
                                                 normalize=_native.NORMALIZE_RMS)
                    for b in range(batch):
                        pw = _pointwise(x2[b], conv[b], ms_encode, width)
                        assert np.array_equal(off[b], pw), tag
                        ref = pw.copy()
                        O.rms_normalize(x2[b], ref)
                        assert np.array_equal(got[b], ref), tag
                        # float64 sums: the applied scale is the float64 RMS ratio to within 1e-6
                        scale = (np.sqrt(np.mean(x2[b].astype(np.float64) ** 2, axis=0))
                                 / np.sqrt(np.mean(pw.astype(np.float64) ** 2, axis=0) + 1e-10))
                        want = pw.astype(np.float64) * scale
                        assert np.max(np.abs(rms[b] - want)) <= 1e-6 * np.max(np.abs(want)), tag
    finally:
        ctx.set_variant(-1)
        table.close()


# ---- i. streams: the stream kernel and its direct variant ------------------------------------------------------------
def _run(stream, x, sched):
    outs, pos = [], 0
    for b in sched:
        outs.append(stream.process(x[..., pos:pos + b, :] if x.ndim == 3 else x[pos:pos + b]))
        pos += b
    outs.append(stream.flush())
    return np.concatenate(outs, axis=-2)


def _schedule(kind, n, latency, seed=0):
    if kind == 'random':
        rng, out, left = np.random.default_rng(seed), [], n
        while left > 0:
            b = int(min(left, rng.choice([0, 0, 1, 17, 480, max(1, latency // 2), latency + 3, 3 * latency + 11])))
            out.append(b)
            left -= b
        return out
    step = int(kind)
    return [step] * (n // step) + ([n % step] if n % step else [])


def test_stream_direct_variant_long_fir(vnd):
    from vndecorrelate_amd.streaming import convolve_velvet_noise_stream
    from vndecorrelate_amd.taps import function_path_arrays
    fir = vnd.generate_velvet_noise(duration_seconds=2.0, num_impulses=40, sample_rate_hz=48000, seed=4)
    x = make_input(dict(seed=2, shape=[150000, 2]))
    want, exact = _refs(x, function_path_arrays(fir))
    assert not np.array_equal(want, exact)
    for kind in ('4800', 'random'):
        s = convolve_velvet_noise_stream(fir, mode=vnd.MODE_FMA, max_frames_per_call=100000)
        assert s.latency_frames > 48000                    # the window does not fit LDS: the direct variant
        y = _run(s, x, _schedule(kind, len(x), s.latency_frames, seed=3))
        assert np.array_equal(y, want), kind
