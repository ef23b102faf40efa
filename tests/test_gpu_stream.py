"""GPU tier of the chunked stream (include/vnd_stream.h, vndecorrelate_amd/streaming.py): streamed under several schedules,
the concatenated output equals the reference's (sha256 of the goldens) and the one-shot calls, bit for bit in the exact
and fma modes."""
import ctypes
import hashlib
import json
import pathlib

import numpy as np
import pytest

from conftest import make_input
from oracle import c_oracle
from oracle import vnd_oracle as O

pytestmark = pytest.mark.gpu

TOL_PEAK = 1e-6
MANIFEST = json.loads((pathlib.Path(__file__).parent / 'golden' / 'manifest.json').read_text())
FN_CASES = sorted(n for n, m in MANIFEST['fn'].items()
                  if 'f64' not in n and m['input'].get('dtype', 'float32') == 'float32')


@pytest.fixture(scope='module')
def vnd():
    import vndecorrelate_amd.decorrelation as d
    from vndecorrelate_amd import _native
    ctx = _native.default_context()
    assert 'gfx950' in ctx.info()['name']
    yield d
    d.set_default_mode(d.MODE_EXACT)


def _kw(d):
    return {k: (tuple(v) if isinstance(v, list) else v) for k, v in d.items()}


def _sha(y):
    return hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest()


def _schedule(kind, n, latency, seed=0):
    if kind == 'whole':
        return [n]
    if kind == 'random':
        rng, out, left = np.random.default_rng(seed), [], n
        while left > 0:
            b = int(min(left, rng.choice([0, 0, 1, 17, 480, max(1, latency // 2), latency + 3, 3 * latency + 11])))
            out.append(b)
            left -= b
        return out
    step = int(kind)
    return [step] * (n // step) + ([n % step] if n % step else [])


def _run(stream, x, sched):
    """x: (n, Cx) / (n,) for a pool of one, (S, n, Cx) otherwise; returns the concatenation of every call's outputs."""
    outs, pos = [], 0
    for b in sched:
        outs.append(stream.process(x[..., pos:pos + b, :] if x.ndim == 3 else x[pos:pos + b]))
        pos += b
    assert pos == x.shape[-2 if x.ndim == 3 else 0]
    outs.append(stream.flush())
    return np.concatenate(outs, axis=-2)


def _kinds(n):
    return ['480', 'random', 'whole'] + (['1', '997'] if n <= 50000 else [])


# ---- 1. the function path against every float32 / int16 golden --------------------------
@pytest.mark.parametrize('name', FN_CASES)
def test_function_path_goldens(vnd, golden, name):
    from vndecorrelate_amd.streaming import convolve_velvet_noise_stream
    meta = golden.manifest['fn'][name]
    x = make_input(meta['input'])
    fir = golden.fir(meta['generator'])
    pool = x.ndim == 3
    n = x.shape[-2]
    cx = x.shape[-1]
    for kind in _kinds(n):
        probe = convolve_velvet_noise_stream(fir, in_channels=cx)
        sched = _schedule(kind, n, probe.latency_frames, seed=len(name))
        s = convolve_velvet_noise_stream(fir, num_streams=x.shape[0] if pool else 1, in_channels=cx,
                                         max_frames_per_call=max([1] + sched) + (1000 if kind == 'whole' else 0))
        y = _run(s, x, sched)
        assert y.dtype == np.float32 and list(y.shape) == meta['out']['shape'], (kind, y.shape)
        assert _sha(y) == meta['out']['sha256'], (name, kind)
        if pool:
            for b, want in enumerate(meta['per_stream_sha256']):
                assert _sha(y[b]) == want, (kind, b)


def test_direct_variant_long_fir(vnd):
    """A 2 s table's window does not fit LDS: the direct variant, against the C oracle (as test_long_fir_falls_back)."""
    from vndecorrelate_amd.streaming import convolve_velvet_noise_stream
    fir = vnd.generate_velvet_noise(duration_seconds=2.0, num_impulses=40, sample_rate_hz=48000, seed=4)
    x = make_input(dict(seed=2, shape=[150000, 2]))
    offs, idx, w = O.fir_to_taps(fir)
    want = c_oracle.convolve(x, offs, idx, w, threads=4)
    for kind in ('4800', 'random'):
        s = convolve_velvet_noise_stream(fir, max_frames_per_call=100000)
        assert s.latency_frames > 48000
        y = _run(s, x, _schedule(kind, len(x), s.latency_frames, seed=3))
        assert np.array_equal(y, want), kind


# ---- 2. VelvetNoise.decorrelate, every golden --------------------------------------------
@pytest.mark.parametrize('name', sorted(MANIFEST['cls_decorrelate']))
def test_class_decorrelate_goldens(vnd, golden, name):
    from vndecorrelate_amd.utils.dsp import mono_to_stereo, rms_normalize, to_float32
    meta = golden.manifest['cls_decorrelate'][name]
    kw = _kw(golden.manifest['class_taps'][meta['class']]['kwargs'])
    normalised = kw.pop('normalizer', 'default') is not None
    vn = vnd.VelvetNoise(normalizer=None, **kw)
    x = make_input(meta['input'])
    mono = x.ndim == 1
    n = len(x)
    for kind in ['480', 'random'] + (['1'] if n <= 5000 else []):
        s = vn.stream(in_channels=1 if mono else None, max_frames_per_call=480 if kind != 'random' else 16384)
        y = _run(s, x, _schedule(kind, n, s.latency_frames, seed=7))
        if normalised:
            xin = to_float32(x)
            rms_normalize(mono_to_stereo(xin) if mono else xin, y)
        assert list(y.shape) == meta['out']['shape']
        assert _sha(y) == meta['out']['sha256'], (name, kind)


# ---- 3. a pool of 64 different signals --------------------------------------------------
def _pool(seed=21, streams=64, n=30011):
    return np.random.default_rng(seed).uniform(-1, 1, (streams, n, 2)).astype(np.float32)


def test_pool_of_64_exact_and_fma(vnd):
    from vndecorrelate_amd.streaming import convolve_velvet_noise_stream
    fir = vnd.generate_velvet_noise(duration_seconds=0.03, num_impulses=30, sample_rate_hz=48000, seed=1)
    x = _pool()
    offs, idx, w = O.fir_to_taps(fir)
    ref = {vnd.MODE_EXACT: c_oracle.convolve(x, offs, idx, w, threads=8),
           vnd.MODE_FMA: c_oracle.convolve_fma(x, offs, idx, w, threads=8)}
    assert not np.array_equal(ref[vnd.MODE_FMA], ref[vnd.MODE_EXACT])
    for mode in (vnd.MODE_EXACT, vnd.MODE_FMA):
        s = convolve_velvet_noise_stream(fir, num_streams=64, mode=mode, max_frames_per_call=8192)
        y = _run(s, x, _schedule('random', x.shape[1], s.latency_frames, seed=mode))
        want = vnd.convolve_velvet_noise_batched(x, fir, mode=mode)
        for b in range(64):
            assert np.array_equal(y[b], want[b]), (mode, b)
            assert np.array_equal(y[b], ref[mode][b]), (mode, b)
    vn = vnd.VelvetNoise(sample_rate_hz=48000, seed=1, normalizer=None, width=0.3)
    s = vn.stream(num_streams=64, max_frames_per_call=8192)
    y = _run(s, x, _schedule('random', x.shape[1], s.latency_frames, seed=5))
    want = vn.decorrelate_batched(x)
    for b in range(64):
        assert np.array_equal(y[b], want[b]), b


# ---- 4. the fast mode -------------------------------------------------------------------
def test_fast_mode_tolerance_and_repeatability(vnd):
    from vndecorrelate_amd.streaming import convolve_velvet_noise_stream
    fir = vnd.generate_velvet_noise(duration_seconds=0.03, num_impulses=128, sample_rate_hz=48000, seed=1)
    x = _pool(seed=4, streams=8, n=40001)
    exact = vnd.convolve_velvet_noise_batched(x, fir, mode=vnd.MODE_EXACT)
    runs = []
    for _ in range(2):
        s = convolve_velvet_noise_stream(fir, num_streams=8, mode=vnd.MODE_FAST, max_frames_per_call=8192)
        runs.append(_run(s, x, _schedule('random', x.shape[1], s.latency_frames, seed=9)))
    assert np.array_equal(runs[0], runs[1])
    peak = float(np.max(np.abs(exact)))
    assert float(np.max(np.abs(runs[0].astype(np.float64) - exact))) <= TOL_PEAK * peak
    vn = vnd.VelvetNoise(sample_rate_hz=48000, seed=1, normalizer=None, mode='LR')      # a mono input fanned out
    s = vn.stream(num_streams=8, in_channels=1, mode=vnd.MODE_FAST, max_frames_per_call=8192)
    got = _run(s, x[:, :, :1], _schedule('480', x.shape[1], s.latency_frames))
    want = vn.decorrelate_batched(x[:, :, :1])
    assert float(np.max(np.abs(got.astype(np.float64) - want))) <= TOL_PEAK * float(np.max(np.abs(want)))


# ---- 5. torch device tensors ------------------------------------------------------------
def test_device_tensors_on_a_side_stream(vnd):
    import torch
    from vndecorrelate_amd import _native
    from vndecorrelate_amd.streaming import convolve_velvet_noise_stream
    fir = vnd.generate_velvet_noise(duration_seconds=0.03, num_impulses=30, sample_rate_hz=48000, seed=1)
    x = _pool(seed=6, streams=5, n=20001)
    sched = _schedule('random', x.shape[1], 1439, seed=2)
    s = convolve_velvet_noise_stream(fir, num_streams=5, max_frames_per_call=8192)
    want = _run(s, x, sched)
    dev = torch.device('cuda', _native.default_context().device)
    side = torch.cuda.Stream(dev)
    for offset in (0, 1):                     # 1: every chunk one float off 16-byte alignment
        s = convolve_velvet_noise_stream(fir, num_streams=5, max_frames_per_call=8192)
        outs, pos = [], 0
        with torch.cuda.stream(side):
            for b in sched:
                flat = torch.empty(5 * b * 2 + offset, dtype=torch.float32, device=dev)
                chunk = flat[offset:].view(5, b, 2)
                chunk.copy_(torch.from_numpy(np.ascontiguousarray(x[:, pos:pos + b])).to(dev))
                assert (chunk.data_ptr() % 16 == 0) == (offset == 0) or b == 0
                outs.append(s.process(chunk))
                pos += b
            outs.append(s.flush())
            got = torch.cat(outs, dim=1)
        side.synchronize()
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), want), offset


# ---- 6. the C ABI refuses before it enqueues ------------------------------------------------
def test_invalid_calls_write_nothing(vnd):
    import torch
    from vndecorrelate_amd import _native
    from vndecorrelate_amd.taps import function_path_arrays
    fir = vnd.generate_velvet_noise(duration_seconds=0.03, num_impulses=30, sample_rate_hz=48000, seed=1)
    ctx = _native.default_context()
    arr = function_path_arrays(fir)
    table = _native.TapTable.create(ctx, arr.tap_offsets, arr.tap_index, arr.tap_weight)
    lib = table._lib
    dev = torch.device('cuda', ctx.device)
    need = ctypes.c_int64()
    assert lib.vnd_stream_state_bytes(table.handle, 2, 2, 480, ctypes.byref(need)) == 0 and need.value > 0
    state = torch.full((need.value // 4,), 7.0, dtype=torch.float32, device=dev)
    x = torch.ones((2, 481, 2), dtype=torch.float32, device=dev)
    y = torch.full((2, 4000, 2), 5.0, dtype=torch.float32, device=dev)
    n_out = ctypes.c_int64(-1)

    def call(n_in, state_bytes, pos=3000):
        return lib.vnd_stream_f32_dev(ctx.handle, table.handle, ctypes.c_void_p(state.data_ptr()), state_bytes, 480,
                                      ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), 2, pos, n_in, 2, 0,
                                      vnd.MODE_EXACT, 0, 0, 0.0, ctypes.byref(n_out), ctypes.c_void_p(0))
    assert call(481, need.value) == 1                 # n_in > max_frames_per_call
    assert call(480, need.value - 4) == 1             # state too short
    assert call(480, need.value, pos=-1) == 1         # negative position
    assert call(480, need.value, pos=2 ** 60 + 1) == 1 and b'position' in lib.vnd_last_error()     # above the last one taken
    assert n_out.value == 0
    torch.cuda.synchronize(dev)
    assert bool((y == 5.0).all()) and bool((state == 7.0).all())
    assert call(480, need.value) == 0 and n_out.value == 480    # the same call, valid: it runs
    torch.cuda.synchronize(dev)
    assert not bool((y[:, :480] == 5.0).all())
    table.close()


# ---- 7. calls ordered across torch streams ----------------------------------------------------
SPIN_CYCLES = 1_000_000


@pytest.mark.parametrize('kind', ['velvet', 'haas', 'correlogram'])
def test_calls_on_alternating_torch_streams_stay_in_order(vnd, kind):
    """Every call runs on the other of two side streams, and each call on the first waits behind a spin there, so its
    state write lands late: the next call, on the second, must still read it.  Exact mode, bit for bit."""
    import torch
    from vndecorrelate_amd import _native, analysis
    from vndecorrelate_amd.streaming import convolve_velvet_noise_stream
    dev = torch.device('cuda', _native.default_context().device)
    S, n, top = 4, 6007, 480
    x = _pool(seed=31, streams=S, n=n)
    if kind == 'velvet':
        fir = vnd.generate_velvet_noise(duration_seconds=0.03, num_impulses=30, sample_rate_hz=48000, seed=1)
        s = convolve_velvet_noise_stream(fir, num_streams=S, max_frames_per_call=top)
        want = vnd.convolve_velvet_noise_batched(x, fir, mode=vnd.MODE_EXACT)
    elif kind == 'haas':
        stage = vnd.HaasEffect(sample_rate_hz=48000, delay_time_seconds=0.0125, delayed_channel=1, mode='MS', width=0.7)
        s = stage.stream(num_streams=S, max_frames_per_call=top)
        want = np.stack([stage.decorrelate(x[b]) for b in range(S)])
    else:
        s = analysis.cross_correlogram_stream(S, sample_rate_hz=48000, max_frames_per_call=top)
        want = analysis.correlogram_numpy_batch(x, None, s.window, s.hop, s.num_lags, s.epsilon)
    rng, sched, left = np.random.default_rng(8), [], n
    while left > 0:
        b = int(min(left, rng.choice([0, 1, 97, top, int(rng.integers(1, top + 1))])))
        sched.append(b)
        left -= b
    xt = torch.from_numpy(x).to(dev)
    sides = (torch.cuda.Stream(dev), torch.cuda.Stream(dev))
    for side in sides:
        side.wait_stream(torch.cuda.current_stream(dev))
    outs, pos = [], 0
    for k, b in enumerate(sched):
        with torch.cuda.stream(sides[k % 2]):
            if k % 2 == 0:
                torch.cuda._sleep(SPIN_CYCLES)
            outs.append(s.process(xt[:, pos:pos + b]))
        pos += b
    with torch.cuda.stream(sides[len(sched) % 2]):
        outs.append(s.flush())
    torch.cuda.synchronize(dev)
    got = torch.cat(outs, dim=1).cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape
    assert got.tobytes() == want.tobytes(), kind
