"""GPU tier of the short-time spectra (include/vnd_spectrum.h, vndecorrelate_amd.spectral).

1. purity: every column of a spectrogram equals the one-segment call on its own segment of its own channel, bit for bit;
2. channel independence: a quiet left channel beside a loud right one has the bits it has alone;
3. parity: the device's distance from SciPy's float64 result is at most 4 x the distance of SciPy's own float32 call, with
   asymmetric windows, no detrend and 'spectrum' scaling too; the detrend held to its own contract, half a float32 ulp of the
   mean;
4. exact cases; 5. the Welch sums: the host's replay of the documented order bit for bit, parity with SciPy at every transform
   size in both types, exchanged channels, strided views; 6. the footprint between guard bands; 7. the plumbing (tensors,
   counts, one graph).
The grid (tests/spectrum_cases.py) holds every transform size, 64 to 4096 - radix-2 first stage and pure radix 4, 64 to 1
segments a pass - and an odd nperseg at every pass width.

Measured on one MI355X (profiles/spectrum_error.json holds every shape): on uniform noise the device's worst column is 1.6
to 2.3e-7 from SciPy's float64 result where SciPy's own float32 call is 1.4 to 2.2e-7 (5.9e-7 both on two-sample segments) -
at 512, 1024, 2048: 1.6, 1.7, 1.6e-7 against 1.6, 1.5, 1.5e-7 - the worst single column 2.4 x SciPy's (3.1 x with a decaying
window, no detrend, 'spectrum' scaling); float64 columns are within 6.4e-16 of SciPy's.  The offset input uses 0.76 to 0.91
of the half-ulp budget.  Welch over 25 segments: float32 Pxx, Pyy, Pxy 4.3 to 7.7e-8 where SciPy's float32 call has 8.7e-8 to
1.1e-7, float64 1.7 to 2.8e-16 from SciPy's float64 result (bound 1.2 to 2.1e-14)."""
import json
import os
import pathlib

import numpy as np
import pytest

import spectrum_cases as C
from spectrum_cases import GRID, IDS, column_errors as _column_errors, hops as _hops, inputs as _inputs, noise as _noise

pytestmark = pytest.mark.gpu

GUARD = 512                      # elements of sentinel either side of every output
DTYPES = [np.float32, np.float64]
ERRORS = {}                      # what test 3 measures, written to $VND_SPECTRUM_ERROR_JSON when that is set


@pytest.fixture(scope='module')
def gpu():
    import torch
    import __graft_entry__ as entry
    entry.build()
    from vndecorrelate_amd import _native, spectral
    ctx = _native.default_context()

    class G:
        pass
    g = G()
    g.torch, g.native, g.sp, g.ctx = torch, _native, spectral, ctx
    g.device = torch.device('cuda', ctx.device)
    spectral.set_spectrum_device(True)
    yield g
    spectral.set_spectrum_device(None)
    out = os.environ.get('VND_SPECTRUM_ERROR_JSON')
    if out and ERRORS:
        pathlib.Path(out).write_text(json.dumps(ERRORS, indent=1, sort_keys=True) + '\n')


def _up(g, a):
    a = np.ascontiguousarray(a)
    return g.torch.from_numpy(a if a.flags.writeable else a.copy()).to(g.device)      # (the shared references are read-only)


def _lengths(g, nfft, nperseg, hop, dtype, cross=0):
    """The signal lengths of the grid: one segment, one frame short of two, two, and R - 1, R, R + 1, 2R + 1 segments."""
    run = g.sp.run_length(nfft, nperseg, hop, dtype, cross)
    segs = sorted({s for s in (run - 1, run, run + 1, 2 * run + 1) if s >= 1})
    return run, sorted({nperseg, nperseg + hop - 1, nperseg + hop} | {nperseg + (s - 1) * hop for s in segs})


def _gram(g, pool, nfft, nperseg, hop, **kw):
    """spectrogram_batched on the device, through tensors: Sxx as NumPy."""
    kw.setdefault('window', ('tukey', 0.25))
    s = g.sp.spectrogram_batched(_up(g, pool), nperseg=nperseg, noverlap=nperseg - hop, nfft=nfft, **kw)[2]
    return s.cpu().numpy()


def _segments_pool(pool, nperseg, hop):
    """Every segment of every channel of a (B, n, C) pool as a signal of its own: (B * C * T, nperseg), T innermost."""
    view = np.lib.stride_tricks.sliding_window_view(pool, nperseg, axis=1)[:, ::hop]        # (B, T, C, nperseg)
    return np.ascontiguousarray(view.transpose(0, 2, 1, 3)).reshape(-1, nperseg)


# ---- 1. purity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
@pytest.mark.parametrize('nfft,nperseg', GRID, ids=IDS)
def test_a_column_is_the_one_segment_call(gpu, nfft, nperseg, dtype):
    g = gpu
    bins, case = nfft // 2 + 1, 0
    for hop in _hops(nperseg):
        run, lengths = _lengths(g, nfft, nperseg, hop, dtype)
        for n in lengths:
            batch, channels = ((3, 2), (1, 1), (1, 2), (3, 1))[case % 4]
            detrend = 'constant' if case % 3 else False
            scaling = 'density' if case % 2 else 'spectrum'
            case += 1
            pool = _noise((batch, n, channels), 1000 * nfft + case, dtype)
            kw = dict(detrend=detrend, scaling=scaling, fs=48000.0)
            got = _gram(g, pool, nfft, nperseg, hop, **kw)
            cols = (n - nperseg) // hop + 1
            assert got.shape == (batch, channels, bins, cols) and got.dtype == dtype
            alone = _gram(g, _segments_pool(pool, nperseg, hop), nfft, nperseg, hop, **kw)     # (B * C * T, F, 1)
            want = alone.reshape(batch, channels, cols, bins).transpose(0, 1, 3, 2)
            assert got.tobytes() == np.ascontiguousarray(want).tobytes(), (hop, n, run, batch, channels, detrend, scaling)
            assert np.isfinite(got).all() and (got >= 0).all() and got.any()
    assert case >= 6


def test_a_strided_mono_view_and_counts(gpu):
    g, sp = gpu, gpu.sp
    nfft, nperseg, hop, n = 256, 200, 175, 200 + 175 * 40
    pool = _noise((3, n, 2), 5)
    t = _up(g, pool)
    both = sp.spectrogram_batched(t, nperseg=nperseg, noverlap=nperseg - hop, nfft=nfft)[2].cpu().numpy()
    view = t[:, :, 1]
    assert not view.is_contiguous()
    right = sp.spectrogram_batched(view, nperseg=nperseg, noverlap=nperseg - hop, nfft=nfft)[2].cpu().numpy()
    assert right.shape == (3, 129, 41) and right.tobytes() == np.ascontiguousarray(both[:, 1]).tobytes()
    assert right.tobytes() == _gram(g, pool[:, :, 1], nfft, nperseg, hop).tobytes()
    # counts 0, nperseg - 1, nperseg and n, and the values outside [0, n]: the signal's own columns, then zeros
    wide = np.concatenate([pool, pool])[:6]
    counts = np.array([0, nperseg - 1, nperseg, n, -1, n + 1], np.int32)
    got = sp.spectrogram_batched(_up(g, wide), nperseg=nperseg, noverlap=nperseg - hop, nfft=nfft,
                                 counts=_up(g, counts))[2].cpu().numpy()
    assert not got[0].any() and not got[1].any() and not got[4].any() and not got[5].any()
    assert got[2, :, :, :1].tobytes() == both[2, :, :, :1].tobytes() and not got[2, :, :, 1:].any()
    assert got[3].tobytes() == both[0].tobytes()
    part = sp.spectrogram_batched(_up(g, wide), nperseg=nperseg, noverlap=nperseg - hop, nfft=nfft,
                                  counts=np.array([n, 200 + 175 * 17 + 174, 200 + 175 * 32, 0, 0, 0], np.int32))[2].cpu().numpy()
    assert part[1, :, :, :18].tobytes() == both[1, :, :, :18].tobytes() and not part[1, :, :, 18:].any()
    assert part[2, :, :, :33].tobytes() == both[2, :, :, :33].tobytes() and not part[2, :, :, 33:].any()


# ---- 2. channel independence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_a_quiet_channel_keeps_its_own_bits(gpu, dtype):
    g, sp = gpu, gpu.sp
    for nfft, nperseg, hop in ((256, 256, 224), (4096, 4096, 512), (128, 128, 128), (512, 512, 448), (2048, 1999, 1750)):
        n = nperseg + 37 * hop
        pool = _noise((2, n, 2), nfft, dtype)
        pool[:, :, 0] *= dtype(1e-4)                              # the side channel, 80 dB under full scale
        both = _gram(g, pool, nfft, nperseg, hop)
        left = _gram(g, pool[:, :, 0], nfft, nperseg, hop)
        assert both[:, 0].tobytes() == left.tobytes() and left.any()
        kw = dict(nperseg=nperseg, noverlap=nperseg - hop, nfft=nfft)
        pxx = sp.welch_batched(_up(g, pool), **kw)[1].cpu().numpy()
        alone = sp.welch_batched(_up(g, pool[:, :, 0]), **kw)[1].cpu().numpy()
        assert pxx.shape == (2, 2, nfft // 2 + 1) and pxx[:, 0].tobytes() == alone.tobytes() and alone.any()
        assert pxx[:, 1].tobytes() == sp.welch_batched(_up(g, pool)[:, :, 1], **kw)[1].cpu().numpy().tobytes()


# ---- 3. parity with SciPy ------------------------------------------------------------------------------------------------
def _signal_errors(got, ref):
    return np.linalg.norm(got.astype(ref.dtype) - ref, axis=-1) / np.linalg.norm(ref, axis=-1)


def _hold_to_scipy(g, label, name, x, ref, own, nfft, nperseg, hop, **kw):
    """The parity rules of one float32 pool: every device column within 4 x SciPy's float32 distance from SciPy's float64
    result, noise columns under the cap, and the float64 pool within 16 log2(nfft) 2^-53."""
    got = _gram(g, x, nfft, nperseg, hop, fs=48000.0, **kw)
    dev, sci = _column_errors(got, ref), _column_errors(own, ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = float(np.nanmax(np.where(dev > 0, dev / sci, 0.0)))
    ERRORS['spectrogram %s%s nfft %d nperseg %d' % (label, name, nfft, nperseg)] = dict(
        device_max=float(dev.max()), device_mean=float(dev.mean()), scipy_max=float(sci.max()), scipy_mean=float(sci.mean()),
        worst_ratio=ratio)
    print(label, name, nfft, nperseg, 'device', dev.max(), 'scipy float32', sci.max(), 'worst ratio', ratio)
    assert (dev <= 4 * sci).all(), (label, name, ratio)
    if name == 'noise':
        assert (dev <= 8 * np.log2(nfft) * 2.0 ** -24).all(), float(dev.max())
    # float64 pools against SciPy's float64 result
    got64 = _gram(g, x.astype(np.float64), nfft, nperseg, hop, fs=48000.0, **kw)
    dev64 = _column_errors(got64, ref)
    ERRORS['spectrogram float64 %s%s nfft %d nperseg %d' % (label, name, nfft, nperseg)] = dict(device_max=float(dev64.max()))
    print(label, name, nfft, nperseg, 'float64 device', dev64.max(), 'bound', 16 * np.log2(nfft) * 2.0 ** -53)
    assert (dev64 <= 16 * np.log2(nfft) * 2.0 ** -53).all(), (label, name, float(dev64.max()))
    return got


@pytest.mark.parametrize('nfft,nperseg', GRID, ids=IDS)
def test_spectrogram_parity_with_scipy(gpu, nfft, nperseg):
    hop = C.parity_case(nfft, nperseg)[0]
    for name, x, ref, own in C.parity_reference(nfft, nperseg):
        _hold_to_scipy(gpu, '', name, x, ref, own, nfft, nperseg, hop)


@pytest.mark.parametrize('nfft,nperseg', [(512, 401), (1024, 1024)], ids=['512-401', '1024-1024'])
def test_parity_beyond_the_defaults(gpu, nfft, nperseg):
    """Windows that a reversed index would change, no detrend, and the 'spectrum' scaling, under the same rules."""
    hop, n, seed = C.parity_case(nfft, nperseg)
    decay, ramp = (w for _, w in C.asymmetric_windows(nperseg))
    assert not np.allclose(decay, decay[::-1]) and not np.allclose(ramp, ramp[::-1])
    variants = (('decay ', dict(window=decay)), ('tukey-ramp ', dict(window=ramp)), ('no detrend ', dict(detrend=False)),
                ('spectrum ', dict(scaling='spectrum')), ('decay no detrend spectrum ', dict(window=decay, detrend=False,
                                                                                            scaling='spectrum')))
    for name, x in _inputs((2, n, 2), seed + 3):
        for label, kw in variants:
            ref, own = C.scipy_columns(x, nfft, nperseg, hop, **kw)
            _hold_to_scipy(gpu, label, name, x, ref, own, nfft, nperseg, hop, **kw)


@pytest.mark.parametrize('nfft,nperseg', C.NEW_SHAPES, ids=C.NEW_IDS)
def test_the_detrend_is_a_float64_mean_rounded_once(gpu, nfft, nperseg):
    """The contract, not relative to SciPy: a float32 column of 0.9 + 1e-3 x noise is within what half a float32 ulp of its
    segment's mean changes in the float64 column, plus the noise cap (tests/test_spectrum_cpu.py: the contract's model stays
    under it, a float32 running sum does not, and SciPy's pairwise float32 mean is 1.4 to 4 times it)."""
    from scipy.signal import get_window
    hop = C.parity_case(nfft, nperseg)[0]
    name, x, _, _ = C.parity_reference(nfft, nperseg)[1]
    assert name == 'offset'
    xs = np.ascontiguousarray(np.moveaxis(x, 2, 1))
    ref, budget = C.detrend_budget(xs, nfft, nperseg, hop, get_window(('tukey', 0.25), nperseg), 48000.0)
    dev = _column_errors(_gram(gpu, x, nfft, nperseg, hop, fs=48000.0), ref)
    assert dev.shape == budget.shape == (2, 2, 9)
    share = float((dev / budget).max())
    ERRORS['detrend budget nfft %d nperseg %d' % (nfft, nperseg)] = dict(device_share_of_budget=share,
                                                                        budget_max=float(budget.max()))
    print('detrend', nfft, nperseg, 'share of the half-ulp budget', share)
    assert (dev <= budget).all(), share


# ---- 4. exact cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_exact_cases(gpu, dtype):
    from scipy.signal import spectrogram
    g = gpu
    for nfft in (64, 128, 256, 512, 1024, 2048, 4096):
        n = nfft * 3 + 5
        half = np.full((2, n, 2), 0.5, dtype)
        kw = dict(window='boxcar', scaling='spectrum')
        got = _gram(g, half, nfft, nfft, nfft // 2, detrend=False, **kw)
        assert got.shape == (2, 2, nfft // 2 + 1, 5)
        assert (got[:, :, 0] == 0.25).all() and (got[:, :, 1:] == 0).all(), nfft
        want = spectrogram(half[0, :, 0], window='boxcar', scaling='spectrum', nperseg=nfft, noverlap=nfft // 2, detrend=False)[2]
        assert (want[0] == 0.25).all() and (want[1:] == 0).all()                          # SciPy gives the same
        assert (_gram(g, half, nfft, nfft, nfft // 2, detrend='constant', **kw) == 0).all(), nfft
        for detrend in (False, 'constant'):
            assert (_gram(g, np.zeros((1, n), dtype), nfft, nfft, nfft, detrend=detrend, **kw) == 0).all()
    # a segment shorter than the transform: the same DC as SciPy's, whose scale is no power of two
    got = _gram(g, np.full((1, 600), 0.5, dtype), 256, 200, 200, detrend=False, window='boxcar', scaling='spectrum')
    want = spectrogram(np.full(600, 0.5, dtype), window='boxcar', scaling='spectrum', nperseg=200, noverlap=0, nfft=256,
                       detrend=False)[2]
    assert (got[0, 0] == want[0]).all() and abs(float(got[0, 0, 0]) - 0.25) < 1e-7


# ---- 5. Welch, CSD, coherence --------------------------------------------------------------------------------------------
def _cross(g, pool, **kw):
    """(pxx, pyy, pxy) of a (B, n, 2) pool from the device, as NumPy."""
    t = _up(g, pool)
    counts = kw.pop('counts', None)
    counts = None if counts is None else _up(g, np.asarray(counts, np.int32))
    pxx = g.sp.welch_batched(t, counts=counts, **kw)[1].cpu().numpy()
    pxy = g.sp.csd_batched(t, counts=counts, **kw)[1].cpu().numpy()
    return pxx[:, 0], pxx[:, 1], pxy


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_a_signal_alone_and_in_a_pool_and_twice(gpu, dtype):
    g = gpu
    for nfft, nperseg, hop in ((256, 256, 128), (64, 64, 64), (4096, 4096, 2048), (256, 200, 25)):
        run = g.sp.run_length(nfft, nperseg, hop, dtype, 2)
        n = nperseg + (3 * run + 1) * hop
        m = nperseg + (2 * run) * hop + hop // 2                   # the signal's own frames: 2R + 1 segments and a rest
        kw = dict(nperseg=nperseg, noverlap=nperseg - hop, nfft=nfft)
        sig = _noise((1, n, 2), nfft + hop, dtype)
        alone = _cross(g, sig[:, :m], **kw)
        pool = np.concatenate([_noise((1, n, 2), 1, dtype), sig, _noise((1, n, 2), 2, dtype)])
        inside = _cross(g, pool, counts=[n, m, nperseg - 1], **kw)
        again = _cross(g, pool, counts=[n, m, nperseg - 1], **kw)
        for a, b, c in zip(alone, inside, again):
            assert a[0].tobytes() == b[1].tobytes() and b.tobytes() == c.tobytes() and a.any()
            assert not b[2].any()                                  # no whole segment: zeros
        # ... and the mean is over the signal's own segments: the spectrogram's columns, added in float64 in ascending t
        # in the documented order, so the host replays it: every bit
        cols = _gram(g, sig[:, :m], nfft, nperseg, hop, window='hann')
        assert cols.shape[-1] == 2 * run + 1
        want = C.replay_mean(cols, run, dtype)
        assert alone[0].tobytes() == np.ascontiguousarray(want[:, 0]).tobytes(), (nfft, nperseg, hop)
        assert alone[1].tobytes() == np.ascontiguousarray(want[:, 1]).tobytes(), (nfft, nperseg, hop)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
@pytest.mark.parametrize('nfft,nperseg,hop', C.WELCH_SHAPES, ids=['%d-%d-%d' % s for s in C.WELCH_SHAPES])
def test_the_sums_are_the_host_replay(gpu, nfft, nperseg, hop, dtype):
    """Pxx and Pyy at R - 1, R, R + 1, 2R and 2R + 1 segments are the spectrogram's columns added on the host in the
    documented order: a run in ascending t from 0.0, the runs in ascending order from 0.0, one division, one rounding."""
    g = gpu
    run = g.sp.run_length(nfft, nperseg, hop, dtype, 2)
    if dtype == np.float64 and (nfft, nperseg, hop) in C.SHORTEST_RUNS:
        assert run == 2048 // (nfft // 2)                          # the shortest run there is: one pass
    segs = sorted({s for s in (run - 1, run, run + 1, 2 * run, 2 * run + 1) if s >= 1})
    n = nperseg + 2 * run * hop + hop - 1
    sig = _noise((1, n, 2), 3 * nfft + hop, dtype)
    kw = dict(nperseg=nperseg, noverlap=nperseg - hop, nfft=nfft)
    cols = _gram(g, sig, nfft, nperseg, hop, window='hann')        # (1, 2, F, 2R + 1)
    assert cols.shape[-1] == 2 * run + 1 and cols.dtype == dtype
    for group in (segs[:3], segs[3:]):
        if not group:
            continue
        counts = [nperseg + (s - 1) * hop + (hop - 1) * (i % 2) for i, s in enumerate(group)]
        pool = np.repeat(sig, len(group), axis=0)
        pxx = g.sp.welch_batched(_up(g, pool), counts=_up(g, np.asarray(counts, np.int32)), **kw)[1].cpu().numpy()
        assert pxx.shape == (len(group), 2, nfft // 2 + 1) and pxx.dtype == dtype
        for i, s in enumerate(group):
            want = C.replay_mean(cols[0, :, :, :s], run, dtype)
            assert pxx[i].tobytes() == want.tobytes(), (s, run, float(np.abs(pxx[i] / want - 1).max()))
            assert want.all()


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_left_equal_to_right(gpu, dtype):
    g = gpu
    for nfft, nperseg, hop in ((256, 256, 128), (128, 100, 50), (4096, 4096, 4096)):
        mono = _noise((2, nperseg + 40 * hop), nfft, dtype)
        pxx, pyy, pxy = _cross(g, np.stack([mono, mono], axis=2), nperseg=nperseg, noverlap=nperseg - hop, nfft=nfft)
        assert pxx.tobytes() == pyy.tobytes() == np.ascontiguousarray(pxy.real).tobytes() and pxx.any()
        assert (pxy.imag == 0).all()


def test_two_thousand_segments_and_a_delay(gpu):
    from scipy.signal import csd, welch
    g = gpu
    # 2000 segments: the sum a float32 accumulator fails
    x = _noise((2, 128000, 2), 11)
    x[1] = np.float32(0.9) + np.float32(1e-3) * x[1]
    kw = dict(nperseg=64, noverlap=0)
    pxx, pyy, pxy = _cross(g, x, **kw)
    # R = L delayed by 3 frames: the conjugation
    a = _noise((3 + 256 * 40,), 12)
    d = np.stack([a[3:], a[:-3]], axis=1)[None]
    for name, pool, kw in (('2000 segments', x, kw), ('delay', d, dict(nperseg=256))):
        pxx, pyy, pxy = _cross(g, pool, **kw)
        for b in range(len(pool)):
            l, r = pool[b, :, 0], pool[b, :, 1]
            l64, r64 = l.astype(np.float64), r.astype(np.float64)
            for what, got, ref, own in (('pxx', pxx[b], welch(l64, **kw)[1], welch(l, **kw)[1]),
                                        ('pyy', pyy[b], welch(r64, **kw)[1], welch(r, **kw)[1]),
                                        ('pxy', pxy[b], csd(l64, r64, **kw)[1], csd(l, r, **kw)[1])):
                dev, sci = float(_signal_errors(got, ref)), float(_signal_errors(own, ref))
                ERRORS['%s %s signal %d' % (name, what, b)] = dict(device=dev, scipy=sci)
                print(name, what, b, 'device', dev, 'scipy float32', sci)
                assert dev <= 4 * sci, (name, what, b, dev, sci)
    assert np.abs(pxy.imag).max() > 0.1 * np.abs(pxy.real).max()   # the delay shows in the phase


def test_coherence_parity(gpu):
    from scipy.signal import coherence
    g = gpu
    a, b = _noise((2, 256 * 60), 13), _noise((2, 256 * 60), 14)
    pool = np.stack([a, np.float32(0.6) * a + np.float32(0.8) * b], axis=2)
    f, cxy = g.sp.coherence_batched(_up(g, pool))
    cxy = cxy.cpu().numpy()
    assert cxy.shape == (2, 129) and cxy.dtype == np.float32 and f.cpu().numpy().tobytes() == coherence(a[0], a[0])[0].tobytes()
    for s in range(2):
        ref = coherence(pool[s, :, 0].astype(np.float64), pool[s, :, 1].astype(np.float64))[1]
        own = coherence(pool[s, :, 0], pool[s, :, 1])[1]
        dev, sci = float(np.abs(cxy[s] - ref).max()), float(np.abs(own - ref).max())
        ERRORS['coherence signal %d' % s] = dict(device=dev, scipy=sci)
        print('coherence', s, 'device', dev, 'scipy float32', sci)
        assert dev <= 4 * sci and 0.2 < ref.mean() < 0.6
    host = g.sp.coherence_batched(pool)[1]                         # NumPy in, NumPy out: the same device sums
    assert isinstance(host, np.ndarray) and host.dtype == np.float32 and np.abs(host - cxy).max() <= 2.0 ** -22   # two hypots


@pytest.mark.parametrize('nfft,nperseg', C.WELCH_PARITY, ids=['%d-%d' % p for p in C.WELCH_PARITY])
def test_welch_and_csd_parity_at_every_size(gpu, nfft, nperseg):
    """25 half-overlapped segments of L = a, R = 0.6 a + 0.8 b: float32 within 4 x SciPy's float32 call, float64 within the
    column bound 16 log2(nfft) 2^-53 of SciPy's float64 result - a mean of columns inherits it when nothing cancels, and
    |Pxy| is 0.62 to 0.66 of sqrt(Pxx Pyy) here."""
    from scipy.signal import csd, welch
    g = gpu
    hop = nperseg // 2
    pool = C.coherent_pair(nperseg + 24 * hop, 100 + nfft)
    kw = dict(nperseg=nperseg, noverlap=nperseg - hop, nfft=nfft)
    l, r = pool[0, :, 0], pool[0, :, 1]
    l64, r64 = l.astype(np.float64), r.astype(np.float64)
    refs = (welch(l64, **kw)[1], welch(r64, **kw)[1], csd(l64, r64, **kw)[1])
    owns = (welch(l, **kw)[1], welch(r, **kw)[1], csd(l, r, **kw)[1])
    share = np.linalg.norm(refs[2]) / np.linalg.norm(np.sqrt(refs[0] * refs[1]))
    assert 0.5 < share < 0.75, share                               # the mean cross spectrum does not cancel
    bound = 16 * np.log2(nfft) * 2.0 ** -53
    for what, got, got64, ref, own in zip(('pxx', 'pyy', 'pxy'), _cross(g, pool, **kw), _cross(g, pool.astype(np.float64), **kw),
                                          refs, owns):
        assert got.dtype == own.dtype and got64.dtype == ref.dtype and got.shape == (1, nfft // 2 + 1)
        dev, sci, dev64 = float(_signal_errors(got[0], ref)), float(_signal_errors(own, ref)), float(_signal_errors(got64[0], ref))
        ERRORS['welch %s nfft %d nperseg %d' % (what, nfft, nperseg)] = dict(device=dev, scipy=sci, device_float64=dev64,
                                                                            bound_float64=bound)
        print('welch', what, nfft, nperseg, 'device', dev, 'scipy float32', sci, 'float64 device', dev64, 'bound', bound)
        assert dev <= 4 * sci, (what, dev, sci)
        assert dev64 <= bound, (what, dev64, bound)


def test_coherence_parity_at_2048(gpu):
    from scipy.signal import coherence
    g = gpu
    nfft, hop = 2048, 1024
    pool = C.coherent_pair(nfft + 24 * hop, 100 + nfft)
    l64, r64 = pool[0, :, 0].astype(np.float64), pool[0, :, 1].astype(np.float64)
    ref = coherence(l64, r64, nperseg=nfft)[1]
    own = coherence(pool[0, :, 0], pool[0, :, 1], nperseg=nfft)[1]
    assert 0.2 < ref.mean() < 0.6
    cxy = g.sp.coherence_batched(_up(g, pool), nperseg=nfft)[1].cpu().numpy()
    cxy64 = g.sp.coherence_batched(_up(g, pool.astype(np.float64)), nperseg=nfft)[1].cpu().numpy()
    assert cxy.dtype == np.float32 and cxy64.dtype == np.float64 and cxy.shape == cxy64.shape == (1, nfft // 2 + 1)
    dev, sci, dev64 = float(np.abs(cxy[0] - ref).max()), float(np.abs(own - ref).max()), float(np.abs(cxy64[0] - ref).max())
    bound = 32 * np.log2(nfft) * 2.0 ** -53                        # absolute: a quotient of three means, each within half of it
    ERRORS['coherence nfft 2048'] = dict(device=dev, scipy=sci, device_float64=dev64, bound_float64=bound)
    print('coherence 2048 device', dev, 'scipy float32', sci, 'float64 device', dev64, 'bound', bound)
    assert dev <= 4 * sci and dev64 <= bound


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_exchanged_channels_exchange_the_sums(gpu, dtype):
    """Of a stereo pool and the pool with L and R exchanged: Pxx and Pyy trade places and Pxy is conjugated, bit for bit -
    the products commute and a - b against b - a is an exact negation.  Shapes whose right channel is staged at an odd
    offset; one signal with no segment, one with R + 1."""
    g = gpu
    for nfft, nperseg, hop in C.ODD_ROOM:
        run = g.sp.run_length(nfft, nperseg, hop, dtype, 2)
        assert ((run - 1) * hop + nperseg) % 2 == 1
        n = nperseg + (2 * run + 1) * hop
        pool = _noise((3, n, 2), nfft + 17, dtype)
        pool[:, :, 1] *= dtype(0.25)                               # ... so that Pxx for Pyy cannot pass
        counts = [nperseg - 1, nperseg + run * hop, n]
        kw = dict(nperseg=nperseg, noverlap=nperseg - hop, nfft=nfft, counts=counts)
        pxx, pyy, pxy = _cross(g, pool, **kw)
        fxx, fyy, fxy = _cross(g, np.ascontiguousarray(pool[:, :, ::-1]), **kw)
        assert pxx.tobytes() == fyy.tobytes() and pyy.tobytes() == fxx.tobytes(), (nfft, nperseg, hop)
        assert pxy.real.tobytes() == fxy.real.tobytes(), (nfft, nperseg, hop)
        nonzero = pxy.imag != 0                                    # (an exact zero sum is +0.0 either way)
        assert np.array_equal(nonzero, fxy.imag != 0) and pxy.imag[nonzero].tobytes() == (-fxy.imag[nonzero]).tobytes()
        assert not pxx[0].any() and not pxy[0].any() and pxx[1:].all() and pyy[1:].all() and pxy.imag[1:].any()
        assert pxx.tobytes() != pyy.tobytes()


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_strided_views_are_their_contiguous_copies(gpu, dtype):
    """The kernels take a tensor's own strides: a stereo pair inside frames of four, every other signal, every other frame,
    one channel of four - and channels that are not adjacent, which are copied first.  Each gives the bits of the same view
    made contiguous, with and without counts."""
    g, sp = gpu, gpu.sp
    nfft, nperseg, hop = 512, 401, 351
    run = sp.run_length(nfft, nperseg, hop, dtype, 2)
    n = 2 * (nperseg + (2 * run + 1) * hop) + 3
    w = _up(g, _noise((4, n, 4), 31, dtype))
    kw = dict(nperseg=nperseg, noverlap=nperseg - hop, nfft=nfft)
    views = (('pair in frames of 4', w[:, :, 1:3]), ('every other signal', w[::2, :, :2]), ('every other frame', w[:, ::2, :2]),
             ('one channel of 4', w[:, :, 2]), ('channels not adjacent', w[:, :, ::2]))
    for name, v in views:
        assert not v.is_contiguous(), name
        flat = v.contiguous()
        m = v.shape[1]
        each = _up(g, np.array([m, nperseg + run * hop + 5, nperseg - 1, m - 1][:v.shape[0]], np.int32))
        for counts in (None, each):
            entries = [sp.spectrogram_batched, sp.welch_batched] + ([sp.csd_batched] if v.dim() == 3 else [])
            for fn in entries:
                got, want = fn(v, counts=counts, **kw)[-1], fn(flat, counts=counts, **kw)[-1]
                assert got.shape == want.shape and got.dtype == want.dtype
                assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), (name, fn.__name__, counts is not None)
                assert bool(got.abs().sum() > 0)
    # ... and the view is the signal it shows: against the host's own slice
    host = w.cpu().numpy()
    got = sp.welch_batched(w[:, ::2, :2], **kw)[1].cpu().numpy()
    assert got.tobytes() == sp.welch_batched(_up(g, host[:, ::2, :2]), **kw)[1].cpu().numpy().tobytes()


# ---- 6. footprint --------------------------------------------------------------------------------------------------------
class Guarded:
    """A device buffer of `count` elements between two guard bands of a sentinel."""

    def __init__(self, g, count, dtype, fill):
        self.fill, self.count = fill, count
        self.whole = g.torch.full((count + 2 * GUARD,), fill, dtype=dtype, device=g.device)
        self.view = self.whole[GUARD:GUARD + count]

    def ptr(self):
        return self.view.data_ptr()

    def check(self):
        w = self.whole.cpu().numpy()
        assert (w[:GUARD] == self.fill).all() and (w[GUARD + self.count:] == self.fill).all(), 'a guard band was written'
        return w[GUARD:GUARD + self.count]


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
@pytest.mark.parametrize('nfft,nperseg,hop', [(64, 2, 1), (64, 64, 56), (4096, 4096, 3584), (4096, 4096, 1),
                                               (1024, 513, 449), (2048, 2048, 1)])
def test_every_entry_between_guard_bands(gpu, nfft, nperseg, hop, dtype):
    g, sp, torch = gpu, gpu.sp, gpu.torch
    f64 = dtype == np.float64
    tdt = torch.float64 if f64 else torch.float32
    bins = nfft // 2 + 1
    run = sp.run_length(nfft, nperseg, hop, dtype, 0)
    n = nperseg + (2 * run) * hop + hop - 1                        # 2R + 1 segments and a rest
    cols = (n - nperseg) // hop + 1
    batch = 3
    pool = _noise((batch, n, 2), nfft + hop, dtype)
    frames = Guarded(g, pool.size, tdt, -777.0)
    frames.view.copy_(_up(g, pool).reshape(-1))
    win64 = np.hanning(nperseg) + 0.1
    win, tw = _up(g, win64.astype(dtype)), _up(g, sp.twiddle_table(nfft, dtype))
    each = _up(g, np.array([n, nperseg + run * hop, nperseg - 1], np.int32))
    scale = sp.spectrum_scale(win64, 1.0, 'density')
    stream = torch.cuda.current_stream(g.device).cuda_stream
    for channels in (1, 2):
        common = (g.ctx, frames.ptr(), batch, n, 2 * n, 2, channels, win.data_ptr(), tw.data_ptr(), nperseg, hop, nfft)
        sxx = Guarded(g, batch * channels * bins * cols, tdt, -555.0)
        g.native.spectrogram_device(*common, sxx.ptr(), detrend=False, scale=scale, n_each_ptr=each.data_ptr(), float64=f64,
                                    stream=stream)
        got = sxx.check().reshape(batch, channels, bins, cols)
        assert (got != -555.0).all() and not got[2].any() and not got[1, :, :, run + 1:].any() and got[1, :, :, :run + 1].all()
        want = _gram(g, pool[:, :, :channels], nfft, nperseg, hop, window=win64, counts=each, detrend=False)
        assert got.tobytes() == want.tobytes()
        need = g.native.cross_spectra_work_bytes(batch, n, channels, nperseg, hop, nfft, f64)
        results = []
        for garbage in (-1, 0x0123456789abcdef):
            pxx, pyy = Guarded(g, batch * bins, tdt, -555.0), Guarded(g, batch * bins, tdt, -555.0)
            pxy = Guarded(g, batch * bins * 2, tdt, -555.0)
            work = Guarded(g, need // 8, torch.int64, garbage)
            g.native.cross_spectra_device(*common, pxx.ptr(), pyy.ptr(), pxy.ptr(), work_ptr=work.ptr(), work_bytes=need,
                                          detrend=False, scale=scale, n_each_ptr=each.data_ptr(), float64=f64, stream=stream)
            work.check()
            rows = (pxx.check(), pyy.check(), pxy.check())
            assert (rows[0] != -555.0).all() and rows[0][:2 * bins].all() and not rows[0][2 * bins:].any()
            if channels == 2:
                assert (rows[1] != -555.0).all() and (rows[2] != -555.0).all() and not rows[2][4 * bins:].any()
            else:
                assert (rows[1] == -555.0).all() and (rows[2] == -555.0).all()          # one channel writes pxx alone
            results.append(b''.join(r.tobytes() for r in rows))
        assert results[0] == results[1]                            # whatever the work memory held
        assert frames.check().tobytes() == pool.tobytes()          # the inputs are as they were
    assert win.cpu().numpy().tobytes() == win64.astype(dtype).tobytes()


# ---- 7. plumbing ---------------------------------------------------------------------------------------------------------
def test_tensors_counts_of_a_voice_pool_and_one_graph(gpu):
    import vndecorrelate_amd.decorrelation as dec
    from scipy.signal import coherence
    g, sp, torch = gpu, gpu.sp, gpu.torch
    x = _noise((3, 4000, 2), 21)
    t = _up(g, x)
    f, tt, s = sp.spectrogram_batched(t)
    assert all(v.device == t.device for v in (f, tt, s)) and s.dtype == torch.float32 and tuple(s.shape) == (3, 2, 129, 17)
    out = torch.empty_like(s)
    assert sp.spectrogram_batched(t, out=out)[2] is out and out.cpu().numpy().tobytes() == s.cpu().numpy().tobytes()
    host = sp.spectrogram_batched(x)                               # NumPy in, NumPy out
    assert all(isinstance(v, np.ndarray) for v in host) and host[2].tobytes() == s.cpu().numpy().tobytes()
    assert sp.welch_batched(t.double())[1].dtype == torch.float64
    # set_spectrum_device(False) keeps the SciPy loop
    sp.set_spectrum_device(False)
    try:
        assert sp.coherence_batched(x)[1][1].tobytes() == coherence(x[1, :, 0], x[1, :, 1])[1].tobytes()
        assert sp.coherence_batched(t)[1].device == t.device
    finally:
        sp.set_spectrum_device(True)

    # decorrelate, then coherence: the pool's out_counts are the spectra's counts, all in device memory
    slots, frames = 3, 4000
    stage = dec.VelvetNoise(sample_rate_hz=48000, duration_seconds=0.005, num_impulses=12, seed=1, normalizer=None)
    pool = dec.decorrelate_voice_pool([stage], slots=slots, in_channels=2, max_frames_per_call=frames)
    xin = torch.empty((slots, frames, 2), dtype=torch.float32, device=g.device)
    counts = _up(g, np.array([frames, 2500, 0], np.int32))
    flags = _up(g, np.array([3, 3, 0], np.int32))                  # START | END: a whole voice a call
    tables = _up(g, np.full(slots, int(pool.bank_tables[0]), np.int32))
    y = torch.zeros((slots, pool.row_frames, 2), dtype=torch.float32, device=g.device)
    oc = torch.empty(slots, dtype=torch.int32, device=g.device)
    pool.reset()

    def chain():
        pool.process_dev(xin, counts, flags, tables, out=(y, oc))
        return sp.coherence_batched(y, counts=oc)[1]
    xin.copy_(_up(g, _noise((slots, frames, 2), 22)))
    eager = chain().cpu().numpy()                                  # the warm-up: tables uploaded, kernels loaded
    assert oc.cpu().numpy().tolist() == [frames, 2500, 0]
    yh = y.cpu().numpy()
    want = coherence(yh[1, :2500, 0].astype(np.float64), yh[1, :2500, 1].astype(np.float64))[1]
    assert np.abs(eager[1] - want).max() < 1e-4 and np.isnan(eager[2]).all() and np.isfinite(eager[:2]).all()
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(g.device)
    with torch.cuda.graph(graph, stream=side):
        captured = chain()
    torch.cuda.synchronize()
    fresh = _up(g, _noise((slots, frames, 2), 23))
    xin.copy_(fresh)
    captured.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    replayed = captured.cpu().numpy()
    xin.copy_(fresh)
    assert replayed.tobytes() == chain().cpu().numpy().tobytes() and replayed.tobytes() != eager.tobytes()
