"""GPU tier of WhiteNoise on the device (vnd_white_noise_f32_dev): the dense float64 FIR against np.convolve under the
per-output bound of include/vnd_amd.h, the whole stage against NumPy's WhiteNoise, the batched call, the default policy
and a device-resident chain through the stage.  The reference for every number is NumPy itself."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS_SUM = 2.0 ** -40


@pytest.fixture(scope='module')
def vnd():
    import vndecorrelate_amd.decorrelation as d
    from vndecorrelate_amd import _native
    ctx = _native.default_context()
    assert 'gfx950' in ctx.info()['name']
    yield d
    d.set_white_noise_device(None)


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


def _device_white_noise(torch, x, h, *, width=None, normalize=0):
    """x float32 (B, n, Cx), h float64 (M, C) through the C ABI on torch buffers; float32 (B, n, C)."""
    from vndecorrelate_amd import _native
    ctx = _native.default_context()
    dev = torch.device('cuda', ctx.device)
    batch, n, cx = x.shape
    m, c = h.shape
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
    hd = torch.from_numpy(np.ascontiguousarray(h, np.float64)).to(dev)
    yd = torch.full((batch, n, c), float('nan'), dtype=torch.float32, device=dev)
    ws = _native.decorrelate_workspace_bytes(batch, n, c)
    work = torch.empty((ws,), dtype=torch.uint8, device=dev)
    _native.white_noise_device(ctx, xd.data_ptr(), hd.data_ptr(), yd.data_ptr(), batch, n, cx, c, m, width=width,
                               normalize=normalize, workspace_ptr=work.data_ptr(), workspace_bytes=ws,
                               stream=torch.cuda.current_stream(dev).cuda_stream)
    return yd.cpu().numpy()


def _numpy_conv(x, h):
    """np.convolve 'same' per channel, as WhiteNoise.decorrelate forms it (x (n, Cx), Cx = 1 fans out)."""
    out = np.zeros((x.shape[0], h.shape[1]), np.float32)
    for c in range(h.shape[1]):
        out[:, c] = np.convolve(x[:, c % x.shape[1]], h[:, c], mode='same')
    return out


def _abs_sums(x, h):
    return np.stack([np.convolve(np.abs(x[:, c % x.shape[1]].astype(np.float64)), np.abs(h[:, c]), mode='same')
                     for c in range(h.shape[1])], axis=1)


def _check_bound(got, want, x, h, what):
    """The per-output contract; returns the number of outputs that differ from NumPy's."""
    finite = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f'{what}: NaN pattern differs'
    assert np.array_equal(got[~finite & ~np.isnan(want)], want[~finite & ~np.isnan(want)]), f'{what}: infinities differ'
    g, w = got[finite].astype(np.float64), want[finite].astype(np.float64)
    bound = np.spacing(np.abs(want[finite])).astype(np.float64) + EPS_SUM * _abs_sums(x, h)[finite]
    err = np.abs(g - w)
    worst = float(np.max(err / bound)) if err.size else 0.0
    assert worst <= 1.0, f'{what}: {worst:.3f} of the bound'
    return int(np.count_nonzero(got[finite] != want[finite]))


def _signal(kind, n, c, rng):
    if kind == 'gaussian':
        return rng.standard_normal((n, c)).astype(np.float32)
    if kind == 'quantised':
        return (rng.integers(-32768, 32767, (n, c)) / 32768.0).astype(np.float32)
    if kind == 'sparse':
        x = np.zeros((n, c), np.float32)
        at = rng.integers(0, n, max(n // 200, 1))
        x[at] = rng.uniform(-1, 1, (len(at), c))
        return x
    if kind == 'silent':
        return np.zeros((n, c), np.float32)
    if kind == 'sine':
        t = np.arange(n)[:, None] / 44100.0
        return np.sin(2 * np.pi * (440.0 + 110.0 * np.arange(c))[None] * t).astype(np.float32)
    raise ValueError(kind)


def test_bare_convolution_against_np_convolve(vnd, torch):
    rng = np.random.default_rng(11)
    kinds = ['gaussian', 'quantised', 'sparse', 'silent', 'sine']
    mismatches = total = 0
    case = 0
    for m in (1, 2, 1323, 1440):
        lengths = [m, m + 1, 4096 + 3 * m + 5, 37_001]
        if m == 1323:
            lengths.append(441_000)                      # 10 s at 44.1 kHz
        for n in lengths:
            for c in (1, 2, 3, 8):
                if n > 100_000 and c != 2:
                    continue
                kind = kinds[case % len(kinds)]
                case += 1
                x = _signal(kind, n, c, rng)
                h = rng.standard_normal((m, c))
                got = _device_white_noise(torch, x[None], h)[0]
                mismatches += _check_bound(got, _numpy_conv(x, h), x, h, f'M={m} N={n} C={c} {kind}')
                total += got.size
            # mono fanned out to two channels
            x = _signal('gaussian', n, 1, rng)
            h = rng.standard_normal((m, 2))
            got = _device_white_noise(torch, x[None], h)[0]
            mismatches += _check_bound(got, _numpy_conv(x, h), x, h, f'M={m} N={n} mono->stereo')
            total += got.size
    print(f'\nbare convolution: {mismatches} of {total} float32 outputs differ from np.convolve (all within the bound)')


def test_non_finite_input_propagates_as_in_numpy(vnd, torch):
    rng = np.random.default_rng(12)
    n, m = 20_000, 1323
    x = rng.standard_normal((n, 2)).astype(np.float32)
    x[5000, 0] = np.inf
    x[9000, 1] = -np.inf
    x[15000, 0] = np.nan
    x[15010, 1] = np.nan
    h = rng.standard_normal((m, 2))
    got = _device_white_noise(torch, x[None], h)[0]
    mism = _check_bound(got, _numpy_conv(x, h), x, h, 'inf / nan')
    assert not np.isfinite(got[5000, 0]) and not np.isfinite(got[9000, 1]) and np.isnan(got[15000, 0])
    print(f'\nnon-finite input: {mism} finite outputs differ from np.convolve')


def test_impulse_reads_the_filter_back(vnd, torch):
    rng = np.random.default_rng(13)
    for m, n, p in ((1323, 9000, 4000), (1440, 6000, 0), (1440, 6000, 5999), (2, 10, 3), (1, 5, 2), (2049, 4100, 2050)):
        h = rng.standard_normal((m, 2))
        x = np.zeros((n, 2), np.float32)
        x[p] = 1.0
        got = _device_white_noise(torch, x[None], h)[0]
        o = (m - 1) // 2
        want = np.zeros((n, 2), np.float32)
        for nn in range(n):
            k = nn + o - p
            if 0 <= k < m:
                want[nn] = h[k].astype(np.float32)
        assert np.array_equal(got, want), (m, n, p)


def _stage_bound(got, want, x, wn, conv_dev, conv_ref):
    """The convolution's bound carried through width and the scale, plus a few ulp for the scale's own rounding."""
    h = wn.white_noise_filter[:, :wn.num_outs]
    xs = x if x.ndim == 2 else x[:, None]
    b = np.spacing(np.abs(conv_ref)).astype(np.float64) + EPS_SUM * _abs_sums(xs, h)
    if wn.width is not None:
        b = np.repeat(b.sum(axis=1, keepdims=True), 2, axis=1)
    scale = np.abs(want.astype(np.float64)).max(axis=0) / np.maximum(np.abs(conv_ref.astype(np.float64)).max(axis=0), 1e-30)
    tol = 8 * np.spacing(np.abs(want)).astype(np.float64) + 2 * scale[None] * b
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err <= tol), float(np.max(err / tol))


def test_whole_stage_against_numpy_white_noise(vnd, torch, golden):
    rng = np.random.default_rng(14)
    cases = []
    for fs in (44100, 48000, 96000):
        for seed in (1, 2):
            n = int(fs * 1.3) + seed
            cases += [(fs, seed, 2, w, _signal('gaussian', n, 2, rng)) for w in (None, 0.0, 0.5, 1.0)]
            cases.append((fs, seed, 2, 0.5, rng.uniform(-1, 1, n).astype(np.float32)))            # mono
            cases.append((fs, seed, 2, None, rng.uniform(-1, 1, n).astype(np.float32)))
            cases.append((fs, seed, 1, None, _signal('quantised', n, 1, rng)))
            cases.append((fs, seed, 8, None, _signal('sine', n, 8, rng)))
    viola = golden.arrays['viola_excerpt_in']
    cases += [(44100, 7, 2, None, viola), (44100, 8, 2, 0.7, viola)]
    exact = 0
    for fs, seed, outs, width, x in cases:
        wn = vnd.WhiteNoise(sample_rate_hz=fs, seed=seed, num_outs=outs, width=width)
        vnd.set_white_noise_device(False)
        want = wn.decorrelate(x.copy())
        vnd.set_white_noise_device(None)
        got = wn.decorrelate(x.copy())
        assert got.dtype == np.float32 and got.shape == want.shape
        xs = x.astype(np.float32)
        h = wn.white_noise_filter[:, :outs]
        conv_dev = _device_white_noise(torch, (xs if xs.ndim == 2 else xs[:, None])[None], h)[0]
        conv_ref = _numpy_conv(xs if xs.ndim == 2 else xs[:, None], h)
        if np.array_equal(conv_dev, conv_ref):
            assert np.array_equal(got, want), (fs, seed, outs, width, x.shape)
            exact += 1
        else:
            _stage_bound(got, want, xs, wn, conv_dev, conv_ref)
    print(f'\nwhole stage: {exact} of {len(cases)} cases had float32 convolutions identical to NumPy\'s and were bit-identical')


def test_batched_is_the_per_stream_loop(vnd, torch):
    rng = np.random.default_rng(15)
    wn = vnd.WhiteNoise(sample_rate_hz=44100, seed=5, width=0.3)
    for b, n in ((1, 6000), (3, 9001), (257, 3000)):
        xb = rng.standard_normal((b, n, 2)).astype(np.float32)
        got = wn.decorrelate_batched(xb)
        assert got.shape == (b, n, 2) and got.dtype == np.float32
        assert np.array_equal(got, np.stack([wn.decorrelate(s) for s in xb])), b
        assert np.array_equal(wn.decorrelate_batched(xb), got), b          # repeated calls
    mono = rng.standard_normal((3, 5000)).astype(np.float32)
    got = wn.decorrelate_batched(mono)
    assert np.array_equal(got, np.stack([wn.decorrelate(s) for s in mono]))
    # the device copy of the filter follows a reassignment
    before = wn.decorrelate(mono[0])
    wn.white_noise_filter = np.random.default_rng(99).normal(size=wn.white_noise_filter.shape)
    after = wn.decorrelate(mono[0])
    vnd.set_white_noise_device(False)
    try:
        numpy_after = wn.decorrelate(mono[0])
    finally:
        vnd.set_white_noise_device(None)
    assert not np.array_equal(after, before)
    np.testing.assert_allclose(after, numpy_after, rtol=1e-5, atol=1e-6 * float(np.max(np.abs(numpy_after))))


def test_default_policy_takes_the_device(vnd, torch, monkeypatch):
    rng = np.random.default_rng(16)
    wn = vnd.WhiteNoise(sample_rate_hz=48000, seed=3)
    x = rng.standard_normal((20_000, 2)).astype(np.float32)
    vnd.set_white_noise_device(False)
    numpy_out = wn.decorrelate(x)
    vnd.set_white_noise_device(None)

    def no_convolve(*a, **k):
        raise AssertionError('np.convolve called on a covered call')
    with monkeypatch.context() as mp:
        mp.setattr(np, 'convolve', no_convolve)
        dev = wn.decorrelate(x)
        vnd.set_white_noise_device(True)
        assert np.array_equal(wn.decorrelate(x), dev)
        vnd.set_white_noise_device(None)
    assert dev.shape == numpy_out.shape
    # False is NumPy's code, bit for bit
    from vndecorrelate_amd.utils.dsp import rms_normalize
    ref = np.zeros_like(numpy_out)
    for c in range(2):
        ref[:, c] = np.convolve(x[:, c], wn.white_noise_filter[:, c], mode='same')
    rms_normalize(x, ref)
    assert np.array_equal(numpy_out, ref)
    # uncovered shapes raise exactly what NumPy raises
    for sig, kw in ((x[:500], {}), (x[:, :1], {}), (x[:, 0], dict(num_outs=3)), (x, dict(num_outs=3)),
                    (np.zeros((20_000, 3), np.float32), dict(num_outs=3, width=0.5))):
        w = vnd.WhiteNoise(sample_rate_hz=48000, seed=3, **kw)
        errors = []
        for policy in (False, None):
            vnd.set_white_noise_device(policy)
            try:
                w.decorrelate(sig)
                errors.append(None)
            except Exception as exc:                     # noqa: BLE001 - the exact exception is what is compared
                errors.append((type(exc), str(exc)))
        vnd.set_white_noise_device(None)
        assert errors[0] is not None and errors[0] == errors[1], (sig.shape, kw, errors)


def test_resident_chain_through_white_noise(vnd, torch):
    from vndecorrelate_amd import resident
    rng = np.random.default_rng(17)
    x = rng.uniform(-1, 1, (30_000, 2)).astype(np.float32)

    def chain(device_resident):
        return (vnd.SignalChain(sample_rate_hz=44100, device_resident=device_resident)
                .velvet_noise(seed=1).haas_effect(delay_time_seconds=0.01, width=0.8)
                .white_noise(seed=2).velvet_noise(seed=3))
    plain = chain(False)(x)
    resident_chain = chain(True)
    got = resident_chain(x)
    assert resident.transfers == {'to_host': 1, 'to_device': 1}
    assert got.shape == plain.shape and got.dtype == plain.dtype
    assert np.array_equal(got, plain)
    assert np.array_equal(resident_chain(x), got)                   # the chain's buffers are reused
