"""CPU tier of the short-time spectra (include/vnd_spectrum.h, vndecorrelate_amd.spectral): the axes against SciPy's bit for
bit, the routing rule, the SciPy loop of the host path with and without counts, and the header against its binding and its
refusals - no device call."""
import ctypes
import pathlib
import re
import subprocess

import numpy as np
import pytest

import spectrum_cases as C
from spectrum_cases import GRID, hops as _hops        # (nfft, nperseg) of the device grid, and the hops of each

REPO = pathlib.Path(__file__).resolve().parents[1]
HEADER = REPO / 'include' / 'vnd_spectrum.h'
NAMES = ['vnd_cross_spectra_f32_dev', 'vnd_cross_spectra_f64_dev', 'vnd_cross_spectra_work_bytes', 'vnd_spectrogram_f32_dev',
         'vnd_spectrogram_f64_dev', 'vnd_spectrum_run_length']
INVALID, UNSUPPORTED = 1, 4

@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as entry
    entry.build()
    from vndecorrelate_amd import _native
    return _native.load_library()


@pytest.fixture
def sp():
    from vndecorrelate_amd import spectral
    spectral.set_spectrum_device(False)
    yield spectral
    spectral.set_spectrum_device(None)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the axes ------------------------------------------------------------------------------------------------------------
def test_f_and_t_are_scipys_bit_for_bit(sp):
    from scipy.signal import spectrogram
    checked = 0
    for nfft, nperseg in GRID:
        for hop in _hops(nperseg):
            for n in (nperseg, nperseg + hop - 1, nperseg + hop, nperseg + 7 * hop + 3):
                for fs in (1.0, 48000.0, 44100):
                    x = np.zeros(n, np.float32)
                    f, t, s = spectrogram(x, fs=fs, window='boxcar', nperseg=nperseg, noverlap=nperseg - hop, nfft=nfft)
                    assert _same_bits(sp.bin_frequencies(nfft, fs), f) and len(f) == nfft // 2 + 1
                    assert _same_bits(sp.segment_times(n, nperseg, nperseg - hop, fs), t)
                    assert s.shape == (nfft // 2 + 1, (n - nperseg) // hop + 1)
                    checked += 1
    assert checked == sum(len(_hops(p)) for _, p in GRID) * 4 * 3
    # ... and through the function, both axes of both forms
    x = np.random.default_rng(0).uniform(-1, 1, (2, 700, 2)).astype(np.float32)
    f, t, _ = sp.spectrogram_batched(x, fs=48000.0)
    want = spectrogram(x[0, :, 0], fs=48000.0)
    assert _same_bits(f, want[0]) and _same_bits(t, want[1])


# ---- the routing rule ----------------------------------------------------------------------------------------------------
def test_spectrum_covers_admits_and_refuses_the_list(sp):
    ok = dict(dtype=np.float32, batch=3, n_frames=1000, channels=2, nperseg=256, noverlap=32, nfft=256)
    covers = lambda **kw: sp.spectrum_covers(**{**ok, **kw})                                  # noqa: E731
    assert covers() and covers(dtype=np.float64) and covers(channels=1) and covers(batch=65535, n_frames=256)
    # nfft: a power of two in [64, 4096]
    for nfft in (64, 128, 256, 512, 1024, 2048, 4096):
        assert covers(nfft=nfft, nperseg=64, noverlap=0, n_frames=5000)
    for nfft in (32, 96, 100, 255, 257, 4095, 8192, 256.0, None):
        assert covers(nfft=nfft, nperseg=20, noverlap=0) is (nfft is None and False), nfft
    assert covers(nfft=None)                                                                  # nfft defaults to nperseg
    for nfft, nperseg in GRID:                                                                # every shape of the device grid
        for hop in _hops(nperseg):
            for dtype in (np.float32, np.float64):
                for channels in (1, 2):
                    assert covers(dtype=dtype, nfft=nfft, nperseg=nperseg, noverlap=nperseg - hop, channels=channels,
                                  n_frames=nperseg + 3 * hop), (nfft, nperseg, hop)
    assert len(GRID) == 15 and {n for n, _ in GRID} == {64, 128, 256, 512, 1024, 2048, 4096}
    assert sum(p % 2 for _, p in GRID) == 6                                                   # the odd segments
    # 2 <= nperseg <= nfft, 0 <= noverlap < nperseg, n >= nperseg
    assert covers(nperseg=2, noverlap=1) and covers(nperseg=2, noverlap=0) and covers(nperseg=200)
    assert not covers(nperseg=1, noverlap=0) and not covers(nperseg=257) and not covers(nperseg=0)
    assert covers(noverlap=0) and covers(noverlap=255) and covers(noverlap=None)
    assert not covers(noverlap=256) and not covers(noverlap=-1) and not covers(noverlap=1.5)
    assert covers(n_frames=256) and not covers(n_frames=255) and not covers(n_frames=2 ** 31)
    # detrend, scaling, window
    assert covers(detrend=False) and covers(detrend='constant')
    for bad in ('linear', True, None, lambda d: d):
        assert not covers(detrend=bad), bad
    assert covers(scaling='spectrum') and not covers(scaling='power') and not covers(scaling=None)
    assert covers(window=('tukey', 0.25)) and covers(window='boxcar') and covers(window=np.hanning(256))
    assert not covers(window=np.hanning(255)) and not covers(window=np.ones((2, 128)))
    assert not covers(window=np.ones(256, np.complex64))
    # dtypes, channels, batch, launch size
    for bad in (np.float16, np.complex64, np.int16, 'no dtype'):
        assert not covers(dtype=bad), bad
    assert not covers(channels=3) and not covers(channels=0) and not covers(batch=0) and not covers(batch=65536)
    assert not covers(batch=65535, n_frames=2 ** 20, nperseg=64, noverlap=63, nfft=64)       # above 2^23 workgroups
    assert not covers(batch=True) and not covers(n_frames=1000.0)


def test_uncovered_calls_keep_the_scipy_loop(sp):
    """With the device demanded, a call the device does not cover still takes the SciPy loop; a covered one needs a device."""
    from scipy.signal import coherence, spectrogram, welch
    x = np.random.default_rng(1).uniform(-1, 1, (2, 900, 2)).astype(np.float32)
    sp.set_spectrum_device(True)
    got = sp.spectrogram_batched(x, detrend='linear')[2]
    assert _same_bits(got[1, 0], spectrogram(x[1, :, 0], detrend='linear')[2])
    got = sp.welch_batched(x, nperseg=100)[1]                                               # nfft 100: no power of two
    assert _same_bits(got[0, 1], welch(x[0, :, 1], nperseg=100)[1])
    wide = np.random.default_rng(2).uniform(-1, 1, (1, 600, 3)).astype(np.float32)
    assert sp.spectrogram_batched(wide)[2].shape == (1, 3, 129, 2)                           # three channels
    halves = x.astype(np.float16)
    assert _same_bits(sp.coherence_batched(halves)[1][0], coherence(halves[0, :, 0], halves[0, :, 1])[1])
    cplx = (x[:, :, 0] + 1j * x[:, :, 1]).astype(np.complex64)
    with pytest.warns(UserWarning):                                                          # SciPy's own: two-sided
        assert sp.spectrogram_batched(cplx)[2].shape[1] == 256
    from vndecorrelate_amd.analysis import _gpu_present
    if not _gpu_present():
        with pytest.raises(RuntimeError, match='set_spectrum_device'):
            sp.spectrogram_batched(x)
        with pytest.raises(RuntimeError, match='set_spectrum_device'):
            sp.coherence_batched(x)
    with pytest.raises(TypeError):
        sp.set_spectrum_device(1)


# ---- the host path -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_the_host_path_is_the_scipy_loop(sp, dtype):
    from scipy.signal import coherence, csd, spectrogram, welch
    x = np.random.default_rng(3).uniform(-1, 1, (3, 1500, 2)).astype(dtype)
    for kw in (dict(), dict(fs=48000.0, window='hann', nperseg=128, noverlap=100, nfft=256, detrend=False, scaling='spectrum'),
               dict(window=np.hanning(64), nperseg=None), dict(nperseg=64, noverlap=0)):
        f, t, s = sp.spectrogram_batched(x, **kw)
        assert s.dtype == dtype and s.shape[:2] == (3, 2) and s.shape[2:] == (len(f), len(t))
        fw, pxx = sp.welch_batched(x, **kw)
        fc, pxy = sp.csd_batched(x, **kw)
        assert pxx.shape == (3, 2, len(f)) and pxy.shape == (3, len(f)) and np.iscomplexobj(pxy)
        for b in range(3):
            for c in range(2):
                want = spectrogram(x[b, :, c], **kw)
                assert _same_bits(s[b, c], want[2]) and _same_bits(f, want[0]) and _same_bits(t, want[1])
                assert _same_bits(pxx[b, c], welch(x[b, :, c], **kw)[1])
            assert _same_bits(pxy[b], csd(x[b, :, 0], x[b, :, 1], **kw)[1])
        ckw = {k: v for k, v in kw.items() if k != 'scaling'}
        fcoh, cxy = sp.coherence_batched(x, **ckw)
        assert cxy.dtype == dtype
        for b in range(3):
            assert _same_bits(cxy[b], coherence(x[b, :, 0], x[b, :, 1], **ckw)[1])
    # a 2-D pool is one channel, without the channel axis
    mono = sp.spectrogram_batched(x[:, :, 1])
    assert mono[2].shape == (3, 129, 6) and _same_bits(mono[2][2], spectrogram(x[2, :, 1])[2])
    assert sp.welch_batched(x[:, :, 1])[1].shape == (3, 129)
    # the defaults are SciPy's: spectrogram overlaps an eighth, the averages a half
    assert sp.spectrogram_batched(x)[2].shape[-1] == (1500 - 256) // 224 + 1


def test_counts_zero_the_columns_past_a_signals_own(sp):
    from scipy.signal import csd, spectrogram, welch
    x = np.random.default_rng(4).uniform(-1, 1, (5, 1200, 2)).astype(np.float32)
    counts = np.array([0, 255, 256, 700, 1200], np.int32)
    f, t, s = sp.spectrogram_batched(x, counts=counts)
    assert s.shape == (5, 2, 129, 5) and len(t) == 5
    assert not s[0].any() and not s[1].any()                      # no whole segment: zeros, where SciPy shortens nperseg
    for b, m in ((2, 256), (3, 700), (4, 1200)):
        own = (m - 256) // 224 + 1
        assert _same_bits(s[b, 1, :, :own], spectrogram(x[b, :m, 1])[2]) and not s[b, :, :, own:].any()
        assert s[b, :, :, :own].all()
    _, pxx = sp.welch_batched(x, counts=counts)
    _, pxy = sp.csd_batched(x, counts=counts)
    assert not pxx[:2].any() and not pxy[:2].any()
    assert _same_bits(pxx[3, 0], welch(x[3, :700, 0])[1]) and _same_bits(pxy[3], csd(x[3, :700, 0], x[3, :700, 1])[1])
    # a count outside [0, n] is no frame
    _, _, odd = sp.spectrogram_batched(x[:2], counts=np.array([-1, 1201], np.int32))
    assert not odd.any()
    with pytest.raises(ValueError, match='one entry per signal'):
        sp.spectrogram_batched(x, counts=counts[:2])
    assert 'shorten' in sp.spectrogram_batched.__doc__ and 'SciPy' in sp.spectrogram_batched.__doc__


def test_argument_errors_are_scipys(sp):
    x = np.zeros((2, 500, 2), np.float32)
    with pytest.raises(ValueError, match='noverlap must be less than nperseg'):
        sp.spectrogram_batched(x, nperseg=64, noverlap=64)
    with pytest.raises(ValueError, match='nfft must be greater than or equal to nperseg'):
        sp.welch_batched(x, nperseg=64, nfft=32)
    with pytest.raises(ValueError, match='Unknown scaling'):
        sp.csd_batched(x, scaling='power')
    for fn in (sp.csd_batched, sp.coherence_batched):
        with pytest.raises(ValueError, match=r'\(batch, n, 2\)'):
            fn(x[:, :, 0])
    with pytest.raises(ValueError, match='pool must be'):
        sp.spectrogram_batched(x[0, :, 0])


def test_tables_and_scale(sp):
    for nfft in (64, 4096):
        for dtype in (np.float32, np.float64):
            tw = sp.twiddle_table(nfft, dtype)
            assert tw.dtype == dtype and tw.shape == (nfft, 2)
            assert tuple(tw[0]) == (1, 0) and tuple(tw[nfft // 4]) == (0, -1) and tuple(tw[nfft // 2]) == (-1, 0)
            k = np.arange(nfft)
            want = np.exp(-2j * np.pi * k / nfft)
            assert np.max(np.abs(tw[:, 0].astype(np.float64) + 1j * tw[:, 1].astype(np.float64) - want)) <= np.finfo(dtype).eps
    win = np.hanning(200)
    assert sp.spectrum_scale(win, 48000.0, 'density') == 1.0 / (48000.0 * np.sum(win * win))
    assert sp.spectrum_scale(win, 48000.0, 'spectrum') == 1.0 / np.sum(win) ** 2
    assert sp.spectrum_scale(np.ones(64), 1.0, 'spectrum') == 2.0 ** -12


# ---- the references the GPU tier rests on --------------------------------------------------------------------------------
PARITY = [p for p in GRID if p != (64, 2)]     # two-sample segments: SciPy's own column error can be nearly zero


@pytest.mark.parametrize('nfft,nperseg', PARITY, ids=['%d-%d' % p for p in PARITY])
def test_scipys_float32_error_is_typical_in_every_column(nfft, nperseg):
    """The GPU tier holds every device column to 4 x the error of SciPy's float32 call in the same column, so that error must
    not be a lucky near-zero.  Noise: the smallest column error is at least a quarter of the shape's median (measured 0.68 to
    0.95 of it).  0.9 + 1e-3 x noise: there the condition does NOT hold - a column's error is the rounding of its segment's
    mean to float32, anywhere between nothing and half an ulp, and the smallest measured 0.015 to 0.063 of the median - and
    what carries the rule instead is that the device's contract rounds the same mean: a model of the contract (float64 mean
    rounded once, float32 subtract and multiply, exact transform) stays within 2 x SciPy's error in every column (measured
    1.000 to 1.018), which leaves the other factor of two of the four to the transform's own rounding."""
    from scipy.signal import get_window
    hop = C.parity_case(nfft, nperseg)[0]
    for name, x, ref, own in C.parity_reference(nfft, nperseg):
        sci = C.column_errors(own, ref)
        print(name, nfft, nperseg, 'smallest / median', sci.min() / np.median(sci))
        assert sci.shape == (2, 2, 9) and (sci > 0).all()
        if name == 'noise':
            assert sci.min() >= 0.25 * np.median(sci), (sci.min(), np.median(sci))
        else:
            xs = np.ascontiguousarray(np.moveaxis(x, 2, 1))
            model = C.column_errors(C.contract_model(xs, nfft, nperseg, hop, get_window(('tukey', 0.25), nperseg), 48000.0), ref)
            print(name, nfft, nperseg, 'contract model / scipy float32', (model / sci).max())
            assert (model <= 2 * sci).all(), float((model / sci).max())


def test_the_half_ulp_budget_of_the_detrend():
    """The detrend contract - float64 sum, divided and rounded once to the sample type - as a budget a column can be held
    to without SciPy's float32 call: the change of the float64 column when its mean moves half a float32 ulp, plus the noise
    cap.  The contract model stays under it at all nine new shapes (0.76 to 0.91 of it); a float32 running-sum mean does not
    (6 to 75 times it), and SciPy's own pairwise float32 mean reaches 1.4 to 4 times it: the GPU test has teeth."""
    from scipy.signal import get_window
    over = 0
    for nfft, nperseg in C.NEW_SHAPES:
        hop = C.parity_case(nfft, nperseg)[0]
        name, x, scipy_ref, own = C.parity_reference(nfft, nperseg)[1]
        assert name == 'offset'
        win = get_window(('tukey', 0.25), nperseg)
        xs = np.ascontiguousarray(np.moveaxis(x, 2, 1))
        ref, budget = C.detrend_budget(xs, nfft, nperseg, hop, win, 48000.0)
        assert ref.shape == scipy_ref.shape and np.allclose(ref, scipy_ref, rtol=1e-9, atol=0)   # the reference is SciPy's
        assert (budget > 8 * np.log2(nfft) * 2.0 ** -24).all()
        model = C.column_errors(C.contract_model(xs, nfft, nperseg, hop, win, 48000.0), ref)
        running = C.column_errors(C.contract_model(xs, nfft, nperseg, hop, win, 48000.0, mean='running'), ref)
        print(nfft, nperseg, 'share of the budget: contract', (model / budget).max(), 'running sum', (running / budget).max(),
              'scipy float32', (C.column_errors(own, ref) / budget).max())
        assert (model <= budget).all(), (nfft, nperseg, float((model / budget).max()))
        over += bool((running > budget).any())
    assert over >= 1


def test_replay_mean_is_the_documented_order():
    cols = np.random.default_rng(9).uniform(0, 1, (3, 5, 11)).astype(np.float32)
    one = C.replay_mean(cols, 32, np.float32)                      # one run: a plain ascending sum
    want = np.zeros((3, 5))
    for t in range(11):
        want = want + cols[..., t].astype(np.float64)
    assert _same_bits(one, (want / 11.0).astype(np.float32))
    parts = [cols[..., t0:t0 + 4].astype(np.float64) for t0 in (0, 4, 8)]
    want = ((parts[0][..., 0] + parts[0][..., 1] + parts[0][..., 2] + parts[0][..., 3])
            + (parts[1][..., 0] + parts[1][..., 1] + parts[1][..., 2] + parts[1][..., 3])
            + (parts[2][..., 0] + parts[2][..., 1] + parts[2][..., 2])) / 11.0
    assert _same_bits(C.replay_mean(cols, 4, np.float64), want)


def test_the_package_exports_it_and_the_module_stands_alone():
    import vndecorrelate_amd
    from vndecorrelate_amd import spectral
    for name in ('spectrogram_batched', 'welch_batched', 'csd_batched', 'coherence_batched', 'set_spectrum_device',
                 'spectrum_covers'):
        assert getattr(vndecorrelate_amd, name) is getattr(spectral, name) and name in spectral.__all__
    text = (REPO / 'vndecorrelate_amd' / 'spectral.py').read_text().lower()
    assert 'oracle' not in text
    assert re.search(r'^(from|import) scipy', text, flags=re.M) is None        # SciPy is imported where it is used


# ---- the header and its binding ------------------------------------------------------------------------------------------
def test_header_is_plain_c():
    src = '#include "vnd_spectrum.h"\nint main(void){return VND_SPECTRUM_MAX_NFFT == 4096 ? 0 : 1;}\n'
    r = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-fsyntax-only', '-I', str(REPO / 'include'), '-x', 'c', '-'],
                       input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_header_binding_and_library_agree(lib):
    from vndecorrelate_amd import _native, spectral
    text = re.sub(r'/\*.*?\*/', '', HEADER.read_text(), flags=re.S)
    assert sorted(set(re.findall(r'\b(vnd_[a-z0-9_]+)\s*\(', text))) == NAMES
    for name in NAMES:
        assert hasattr(lib, name)
    for define, value in (('VND_SPECTRUM_MIN_NFFT', spectral.MIN_NFFT), ('VND_SPECTRUM_MAX_NFFT', spectral.MAX_NFFT),
                          ('VND_SPECTRUM_RUN', spectral.RUN)):
        assert int(re.search(r'#define %s (\d+)' % define, text).group(1)) == value
    assert not set(NAMES) & set(_native.SIGNATURES)                # it stays out of vnd_amd.h


P = 1 << 24            # a made-up device address: nothing below reaches a device


def _common(batch, n, ss, fs, ch, win, tw, nperseg, hop, nfft, detrend, scale, each):
    return (batch, n, ss, fs, ch, win, tw, nperseg, hop, nfft, detrend, ctypes.c_double(scale), each)


def _gram(lib, f64=False, *, ctx=0, x=P, batch=3, n=1000, ss=2000, fs=2, ch=2, win=5 * P, tw=6 * P, nperseg=256, hop=224,
          nfft=256, detrend=1, scale=1e-3, each=0, sxx=2 * P):
    fn = lib.vnd_spectrogram_f64_dev if f64 else lib.vnd_spectrogram_f32_dev
    return fn(ctx, x, *_common(batch, n, ss, fs, ch, win, tw, nperseg, hop, nfft, detrend, scale, each), sxx, None)


def _cross(lib, f64=False, *, ctx=0, x=P, batch=3, n=1000, ss=2000, fs=2, ch=2, win=5 * P, tw=6 * P, nperseg=256, hop=128,
           nfft=256, detrend=1, scale=1e-3, each=0, pxx=2 * P, pyy=3 * P, pxy=4 * P, work=8 * P, work_bytes=None):
    if work_bytes is None:
        need = ctypes.c_int64()
        ok = lib.vnd_cross_spectra_work_bytes(batch, n, ch, nperseg, hop, nfft, int(f64), ctypes.byref(need))
        work_bytes = need.value if ok == 0 else 1 << 40
    fn = lib.vnd_cross_spectra_f64_dev if f64 else lib.vnd_cross_spectra_f32_dev
    return fn(ctx, x, *_common(batch, n, ss, fs, ch, win, tw, nperseg, hop, nfft, detrend, scale, each), pxx, pyy, pxy, work,
              work_bytes, None)


@pytest.mark.parametrize('f64', [False, True])
@pytest.mark.parametrize('entry', ['spectrogram', 'cross'])
def test_checks_that_need_no_device(lib, entry, f64):
    err = lib.vnd_last_error
    call = (lambda **kw: _gram(lib, f64, **kw)) if entry == 'spectrogram' else (lambda **kw: _cross(lib, f64, **kw))
    outs = ('sxx',) if entry == 'spectrogram' else ('pxx', 'pyy', 'pxy', 'work')
    size = 8 if f64 else 4
    # valid arguments reach the last check: the context
    assert call() == INVALID and b'null context' in err()
    assert call(each=7 * P, detrend=0, nfft=4096, nperseg=4096, hop=1, n=4200, ss=10000) == INVALID and b'null context' in err()
    assert call(nfft=64, nperseg=2, hop=2, ch=1, fs=1, ss=1, n=2, batch=65535) == INVALID and b'null context' in err()
    assert call(nperseg=200, hop=1) == INVALID and b'null context' in err()
    # null pointers
    for name in ('x', 'win', 'tw') + outs:
        assert call(**{name: 0}) == INVALID and b'null' in err() and b'context' not in err(), name
    if entry == 'cross':                                           # one channel writes pxx alone
        assert call(ch=1, pyy=0, pxy=0) == INVALID and b'null context' in err()
    # counts below 1
    for name in ('batch', 'n', 'ss', 'fs', 'hop'):
        for bad in (0, -1):
            assert call(**{name: bad}, **({} if entry == 'spectrogram' else {'work_bytes': 1 << 40})) == INVALID \
                and b'>= 1' in err(), (name, bad)
    for bad in (1, 0, -5):
        assert call(nperseg=bad, hop=1, **({} if entry == 'spectrogram' else {'work_bytes': 1 << 40})) == INVALID \
            and b'>= 1' in err(), bad
    for bad in (0, 3, -1):
        assert call(ch=bad, fs=4) == INVALID and b'channels' in err(), bad
    assert call(ch=2, fs=1) == INVALID and b'frame stride' in err()
    assert call(n=255) == INVALID and b'no whole segment' in err()
    # the scale
    assert call(scale=float('nan')) == INVALID and b'NaN' in err()
    for bad in (0.0, -1.0, float('inf')) + (() if f64 else (1e-60, 1e60)):
        assert call(scale=bad) == INVALID and b'scale' in err(), bad
    # what the kernels do not take
    for bad in (32, 96, 255, 257, 8192, 0, -256):
        assert call(nfft=bad, nperseg=16, hop=16) == UNSUPPORTED and b'power of two' in err(), bad
    assert call(nperseg=257, hop=1) == UNSUPPORTED and b'above nfft' in err()
    assert call(hop=257) == UNSUPPORTED and b'above nperseg' in err()
    assert call(batch=65536, ss=1, fs=2, n=256) == UNSUPPORTED and b'split the pool' in err()
    assert call(n=2 ** 31, ss=1) == UNSUPPORTED and b'2^31' in err()
    assert call(ss=2 ** 61) == UNSUPPORTED and b'overflow' in err()
    assert call(batch=65535, n=2 ** 20, ss=1, nfft=64, nperseg=64, hop=1) == UNSUPPORTED and b'workgroups' in err()
    # an invalid argument is reported before an unsupported shape
    assert call(nfft=100, scale=float('nan')) == INVALID and call(nfft=100, ch=3) == INVALID
    # overlapping buffers: the frames span 2 * 2000 + 999 * 2 + 2 samples from P
    inside = P + 100 * size
    for name in outs:
        assert call(**{name: inside}) == INVALID and b'overlap' in err(), name
        assert call(**{name: 5 * P + 254 * size}) == INVALID and b'window' in err(), name      # inside the window's end
        assert call(**{name: 6 * P + 510 * size}) == INVALID and b'twiddles' in err(), name    # inside the twiddles' end
        assert call(each=7 * P, **{name: 7 * P + 8}) == INVALID and b'n_each' in err(), name
    last = P + (2 * 2000 + 999 * 2 + 1) * size
    assert call(**{outs[0]: last}) == INVALID and b'overlap' in err()
    assert call(**{outs[0]: last + size + (8 - (last + size) % 8) % 8}) == INVALID and b'null context' in err()
    if entry == 'cross':
        need = ctypes.c_int64()
        assert lib.vnd_cross_spectra_work_bytes(3, 1000, 2, 256, 128, 256, int(f64), ctypes.byref(need)) == 0
        assert call(work_bytes=need.value - 1) == INVALID and b'work of' in err()
        assert call(work_bytes=need.value) == INVALID and b'null context' in err()
        assert call(work=8 * P + 4) == INVALID and b'aligned' in err()
        row = 3 * 129 * size
        assert call(pyy=2 * P + row - size) == INVALID and b'one another' in err()
        assert call(pyy=2 * P + row) == INVALID and b'null context' in err()
        assert call(pxy=3 * P + row - size) == INVALID and b'one another' in err()
        assert call(pxx=4 * P + 2 * row - size) == INVALID and b'one another' in err()
        assert call(pxx=8 * P + need.value - size) == INVALID and b'one another' in err()
        assert call(pxx=8 * P + need.value) == INVALID and b'null context' in err()
    else:
        sxx_bytes = 3 * 2 * 129 * 4 * size                         # (1000 - 256) // 224 + 1 = 4 columns
        assert call(x=2 * P + sxx_bytes - size) == INVALID and b'overlap' in err()
        assert call(x=2 * P + sxx_bytes) == INVALID and b'null context' in err()


def test_work_bytes_and_run_length(lib):
    from vndecorrelate_amd import _native, spectral
    got, run = ctypes.c_int64(-7), ctypes.c_int32(-7)
    for f64 in (0, 1):
        for ch in (1, 2):
            for nfft, nperseg in GRID:
                for hop in _hops(nperseg):
                    assert lib.vnd_spectrum_run_length(nfft, nperseg, hop, f64, ch, ctypes.byref(run)) == 0
                    r = run.value
                    assert 1 <= r <= 32 and r == C.spectrum_run(nfft, nperseg, hop, 8 if f64 else 4, ch), (nfft, nperseg, hop)
                    # the staged frames of a run fit 156 KiB beside the points (and, stereo, the left spectra of a pass)
                    points = 2 * 2368 * (2 if ch == 2 else 1)
                    assert (points + ch * ((r - 1) * hop + nperseg)) * (8 if f64 else 4) <= 156 * 1024
                    for n in (nperseg, nperseg + hop * r - 1, nperseg + hop * r, nperseg + 5 * hop * r + 1):
                        segments = (n - nperseg) // hop + 1
                        assert lib.vnd_cross_spectra_work_bytes(3, n, ch, nperseg, hop, nfft, f64, ctypes.byref(got)) == 0
                        assert got.value == 3 * -(-segments // r) * (nfft // 2 + 1) * (4 if ch == 2 else 1) * 8
                    assert lib.vnd_spectrum_run_length(nfft, nperseg, hop, f64, 0, ctypes.byref(run)) == 0
                    assert run.value == C.spectrum_run(nfft, nperseg, hop, 8 if f64 else 4, 0), (nfft, nperseg, hop)
                    tile = (nfft // 2 + 1) * (run.value | 1)
                    assert (2 * 2368 + (run.value - 1) * hop + nperseg + tile) * (8 if f64 else 4) <= 156 * 1024
    # the defaults own the longest run; the largest float64 segment still fits, alone
    assert spectral.run_length(256, 256, 224) == 32 and spectral.run_length(256, 256, 128, np.float32, 2) == 32
    assert spectral.run_length(4096, 4096, 4096, np.float64) == 2 and spectral.run_length(4096, 4096, 4096, np.float64, 2) == 1
    # the shortest runs of a float64 stereo pool, which the GPU tier's Welch replay must meet: 8, 4, 2, 1 - whole passes
    for (nfft, nperseg, hop), want in C.SHORTEST_RUNS.items():
        assert spectral.run_length(nfft, nperseg, hop, np.float64, 2) == want == 2048 // (nfft // 2), (nfft, nperseg, hop)
    assert all(shape in C.SHORTEST_RUNS for shape in C.WELCH_SHAPES[4:])
    # the one float32 spectrogram run that is neither 32 nor a few: 30 segments, tile pitch 31
    assert spectral.run_length(2048, 2048, 1) == 30
    for nfft, nperseg, hop in C.ODD_ROOM:                          # the right channel's staged frames start at an odd offset
        for dtype in (np.float32, np.float64):
            assert ((spectral.run_length(nfft, nperseg, hop, dtype, 2) - 1) * hop + nperseg) % 2 == 1
    assert _native.cross_spectra_work_bytes(2, 1000, 2, 256, 128, 256) == 2 * 1 * 129 * 4 * 8
    for bad in ((0, 1000, 2, 256, 128, 256), (1, 0, 2, 256, 128, 256), (1, 1000, 3, 256, 128, 256), (1, 1000, 2, 1, 1, 256),
                (1, 1000, 2, 256, 0, 256), (1, 255, 2, 256, 128, 256)):
        assert lib.vnd_cross_spectra_work_bytes(*bad, 0, ctypes.byref(got)) == INVALID and got.value == 0, bad
    assert lib.vnd_cross_spectra_work_bytes(1, 1000, 2, 256, 128, 256, 0, None) == INVALID
    for bad in ((65536, 1000, 2, 256, 128, 256), (1, 2 ** 31, 2, 256, 128, 256), (1, 1000, 2, 256, 128, 100),
                (1, 1000, 2, 256, 128, 8192), (1, 1000, 2, 300, 128, 256), (1, 1000, 2, 256, 257, 256)):
        assert lib.vnd_cross_spectra_work_bytes(*bad, 0, ctypes.byref(got)) == UNSUPPORTED and got.value == 0, bad
    assert lib.vnd_spectrum_run_length(256, 256, 128, 0, 3, ctypes.byref(run)) == INVALID and run.value == 0
    assert lib.vnd_spectrum_run_length(256, 1, 1, 0, 0, ctypes.byref(run)) == INVALID
    assert lib.vnd_spectrum_run_length(100, 64, 1, 0, 0, ctypes.byref(run)) == UNSUPPORTED
    assert lib.vnd_spectrum_run_length(256, 256, 128, 0, 0, None) == INVALID
