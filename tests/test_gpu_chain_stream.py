"""GPU tier of the Haas and chain streams (include/vnd_haas_stream.h, streaming.HaasStream / ChainStream): streamed under
several schedules, the concatenated output equals the reference's (sha256 of the Haas goldens), the one-shot chain and
the device-resident chain, bit for bit in the exact and fma modes."""
import ctypes
import hashlib

import numpy as np
import pytest

from conftest import make_input

pytestmark = pytest.mark.gpu

FS = 48000


@pytest.fixture(scope='module')
def vnd():
    import vndecorrelate_amd.decorrelation as d
    from vndecorrelate_amd import _native
    ctx = _native.default_context()
    assert 'gfx950' in ctx.info()['name']
    yield d
    d.set_default_mode(d.MODE_EXACT)


def _schedule(kind, n, seed=0, top=480):
    if kind == 'whole':
        return [n]
    if kind == 'random':
        rng, out, left = np.random.default_rng(seed), [], n
        while left > 0:
            b = int(min(left, rng.choice([0, 0, int(rng.integers(0, top + 1)), top])))
            out.append(b)
            left -= b
        return out
    step = int(kind)
    return [step] * (n // step) + ([n % step] if n % step else [])


def _run(stream, x, sched, axis):
    """x: the pool's whole signal, frames on ``axis``; the concatenation of every call's outputs."""
    outs, pos = [], 0
    for b in sched:
        outs.append(stream.process(np.take(x, np.arange(pos, pos + b), axis=axis)))
        pos += b
    assert pos == x.shape[axis]
    outs.append(stream.flush())
    return np.concatenate(outs, axis=-2)


# ---- 1. HaasEffect.stream against the reference's goldens ------------------------------------
@pytest.mark.parametrize('kind', ['whole', '1', '64', '480', 'random'])
def test_haas_goldens(vnd, golden, kind):
    for name, meta in golden.manifest['haas'].items():
        x = make_input(meta['input'])
        n = x.shape[0]
        stage = vnd.HaasEffect(**meta['kwargs'])
        top = max(n, 1) if kind == 'whole' else (480 if kind == 'random' else int(kind))
        s = stage.stream(in_channels=1 if x.ndim == 1 else 2, max_frames_per_call=top)
        for seed in (range(3) if kind == 'random' else [0]):
            s.reset()
            got = _run(s, x, _schedule(kind, n, seed, top), 0)
            assert got.dtype == np.float64 and list(got.shape) == meta['out_shape'], (name, kind)
            assert hashlib.sha256(got.tobytes()).hexdigest() == meta['out_sha256'], (name, kind, seed)


def test_haas_pool_and_torch_path(vnd):
    import torch
    stage = vnd.HaasEffect(sample_rate_hz=FS, delay_time_seconds=0.0125, delayed_channel=1, mode='MS', width=0.7)
    x = make_input(dict(seed=7, shape=[5, 3001, 2]))
    want = np.stack([stage.decorrelate(x[b]) for b in range(5)])
    s = stage.stream(num_streams=5, max_frames_per_call=480)
    assert np.array_equal(_run(s, x, _schedule('random', 3001, 3), 1), want)
    s.reset()
    xt = torch.from_numpy(x).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        outs, pos = [], 0
        for b in _schedule('random', 3001, 4):
            outs.append(s.process(xt[:, pos:pos + b]))
            pos += b
        outs.append(s.flush())
        got = torch.cat(outs, dim=1)
    side.synchronize()
    assert got.dtype == torch.float64 and np.array_equal(got.cpu().numpy(), want)


# ---- 2. chains ------------------------------------------------------------------------------
def _fir():
    import vndecorrelate_amd.decorrelation as d
    return d.generate_velvet_noise(duration_seconds=0.03, num_impulses=30, sample_rate_hz=FS, seed=3)


def _chains(vnd):
    sc = lambda: vnd.SignalChain(sample_rate_hz=FS)
    return {
        'vn>haas': lambda: (sc().velvet_noise(duration_seconds=0.02, seed=1, normalizer=None)
                            .haas_effect(delay_time_seconds=0.02, delayed_channel=1, mode='LR')),
        'vn_lr_width>haas_ms': lambda: (sc().velvet_noise(seed=2, mode='LR', width=0.4, normalizer=None)
                                        .haas_effect(delay_time_seconds=0.004, delayed_channel=0, mode='MS', width=0.6)),
        'haas>vn': lambda: (sc().haas_effect(delay_time_seconds=0.01, delayed_channel=1)
                            .velvet_noise(seed=4, normalizer=None)),
        'haas>haas': lambda: (sc().haas_effect(delay_time_seconds=0.003, delayed_channel=1, mode='MS', width=0.5)
                              .haas_effect(delay_time_seconds=0.011, delayed_channel=0)),
        'conv>haas': lambda: (sc().stateless(vnd.convolve_velvet_noise, velvet_noise_filters=_fir())
                              .haas_effect(delay_time_seconds=0.005, delayed_channel=1, mode='MS')),
    }


def _input(kind, S, n, seed):
    rng = np.random.default_rng(seed)
    if kind == 'int16':
        return rng.integers(-32768, 32767, (S, n, 2), dtype=np.int16)
    x = rng.uniform(-1, 1, (S, n) if kind == 'mono' else (S, n, 2)).astype(np.float32)
    return x


@pytest.mark.parametrize('pool', [1, 5, 64])
@pytest.mark.parametrize('kind', ['stereo', 'mono', 'int16'])
@pytest.mark.parametrize('name', ['vn>haas', 'vn_lr_width>haas_ms', 'haas>vn', 'haas>haas', 'conv>haas'])
def test_chain_exact(vnd, name, kind, pool):
    make = _chains(vnd)[name]
    n = 2500 if pool == 64 else 6000
    x = _input(kind, pool, n, seed=17 * pool + 3 * len(name) + len(kind))
    if name == 'conv>haas' and kind == 'mono':      # the one-shot call raises IndexError on a mono (n,) signal: refused
        with pytest.raises(IndexError):
            make()(x[0])
        with pytest.raises(ValueError, match='stage 0'):
            make().stream(num_streams=pool, in_channels=1)
        return
    cs = make().stream(num_streams=pool, in_channels=1 if kind == 'mono' else 2, max_frames_per_call=480)
    xin = x[..., None] if kind == 'mono' else x
    got = _run(cs, xin, _schedule('random', n, pool), 1)
    chain, resident = make(), make()
    resident.device_resident = True
    for b in range(pool):
        want = chain(x[b])
        assert got.dtype == want.dtype and got.shape[1:] == want.shape, (name, kind)
        assert np.array_equal(got[b], want), (name, kind, pool, b)
        if b in (0, pool - 1):
            assert np.array_equal(got[b], resident(x[b])), (name, kind, pool, b)
    assert got.shape[1] == n + cs.tail_frames


def test_chain_pool_of_one_shapes(vnd):
    chain = _chains(vnd)['vn>haas']()
    x = _input('stereo', 1, 3000, 11)[0]
    cs = chain.stream(max_frames_per_call=512)
    assert np.array_equal(_run(cs, x, _schedule('512', 3000), 0), chain(x))
    m = _input('mono', 1, 3000, 12)[0]
    cs = chain.stream(in_channels=1, max_frames_per_call=512)
    assert np.array_equal(_run(cs, m, _schedule('random', 3000, 5, 512), 0), chain(m))


def test_chain_fma_and_fast_modes(vnd):
    from oracle import c_oracle
    from oracle import vnd_oracle as O
    x = _input('stereo', 5, 5000, 21)
    offs, idx, w = O.fir_to_taps(_fir())
    conv_fma = c_oracle.convolve_fma(x, offs, idx, w, threads=4)
    assert not np.array_equal(conv_fma, c_oracle.convolve(x, offs, idx, w, threads=4))
    for name in ('vn>haas', 'conv>haas'):
        make = _chains(vnd)[name]
        cs = make().stream(num_streams=5, mode=vnd.MODE_FMA, max_frames_per_call=480)
        got = _run(cs, x, _schedule('random', 5000, 6), 1)
        vnd.set_default_mode(vnd.MODE_FMA)
        try:
            chain = make()
            for b in range(5):
                assert np.array_equal(got[b], chain(x[b])), (name, b)
                if name == 'conv>haas':      # the fma definition, then the reference's Haas stage
                    want = O.haas_effect(conv_fma[b], sample_rate_hz=FS, delay_time_seconds=0.005, delayed_channel=1, mode='MS')
                    assert np.array_equal(got[b], want), (name, b)
        finally:
            vnd.set_default_mode(vnd.MODE_EXACT)
        cs = make().stream(num_streams=5, mode=vnd.MODE_FAST, max_frames_per_call=480)
        got = _run(cs, x, _schedule('random', 5000, 7), 1)
        chain = make()
        for b in range(5):
            want = chain(x[b])
            assert np.max(np.abs(got[b] - want)) <= 1e-6 * np.max(np.abs(want)), (name, b)


def test_chain_torch_path_and_transfers(vnd):
    import torch
    make = _chains(vnd)['vn_lr_width>haas_ms']
    x = _input('stereo', 5, 4000, 31)
    cs = make().stream(num_streams=5, max_frames_per_call=480)
    sched = _schedule('random', 4000, 8)
    outs, pos = [], 0
    for b in sched:
        outs.append(cs.process(x[:, pos:pos + b]))
        assert cs.transfers == {'to_device': 1, 'to_host': 1}
        pos += b
    outs.append(cs.flush())
    assert cs.transfers == {'to_device': 0, 'to_host': 1}
    want = np.concatenate(outs, axis=1)
    cs.reset()
    xt = torch.from_numpy(x).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        outs, pos = [], 0
        for b in sched:
            outs.append(cs.process(xt[:, pos:pos + b]))
            assert cs.transfers == {'to_device': 0, 'to_host': 0}
            assert outs[-1].is_cuda
            pos += b
        outs.append(cs.flush())
        assert cs.transfers == {'to_device': 0, 'to_host': 0}
        got = torch.cat(outs, dim=1)
    side.synchronize()
    assert got.dtype == torch.float64 and np.array_equal(got.cpu().numpy(), want)
    chain = make()
    assert np.array_equal(want[3], chain(x[3]))


# ---- 3. invalid C-ABI calls -------------------------------------------------------------------
def test_invalid_calls_write_nothing(vnd):
    import torch
    from vndecorrelate_amd import _native
    lib, ctx = _native.load_library(), _native.default_context()
    S, M, d, cx = 3, 64, 100, 2
    stage = vnd.HaasEffect(sample_rate_hz=FS, delay_time_seconds=d / FS, delayed_channel=0, mode='MS', width=0.3)
    x = make_input(dict(seed=9, shape=[S, 700, cx]))
    need = ctypes.c_int64()
    assert lib.vnd_haas_stream_state_bytes(S, cx, d, M, ctypes.byref(need)) == 0
    state = torch.zeros(need.value, dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()                    # the host calls run on the library's own stream
    got = ctypes.c_int64()
    outs, pos = [], 0

    def call(chunk, final, *, batch=S, position=None, n_in=None, channels=cx, dch=0, bytes_=None, xp=True, cap=M):
        n = chunk.shape[1] if n_in is None else n_in
        y = np.full((S, chunk.shape[1] + (d if final else 0), 2), 12345.0)       # [batch][n_out][2] of the valid call
        xs = np.ascontiguousarray(chunk, np.float32)
        rc = lib.vnd_haas_stream_f64_host(ctx.handle, ctypes.c_void_p(state.data_ptr()),
                                          need.value if bytes_ is None else bytes_, cap,
                                          ctypes.c_void_p(xs.ctypes.data if xp else None), ctypes.c_void_p(y.ctypes.data),
                                          batch, pos if position is None else position, n, channels, int(final), d, dch,
                                          1, 1, 0.3, ctypes.byref(got))
        return rc, y

    for b in (50, 64, 30):
        rc, y = call(x[:, pos:pos + b], False)
        assert rc == 0 and got.value == b
        outs.append(y)
        pos += b
    before = state.cpu().clone()
    chunk = x[:, pos:pos + 40]
    for kw in (dict(n_in=M + 1), dict(bytes_=need.value - 1), dict(batch=65536), dict(channels=3), dict(dch=2),
               dict(position=-1), dict(position=2 ** 60 + 1), dict(n_in=-1), dict(xp=False)):
        rc, y = call(chunk, False, **kw)
        assert rc == 1, kw
        assert np.all(y == 12345.0), kw
    assert torch.equal(state.cpu(), before)
    rc, y = call(chunk, False)
    assert rc == 0
    outs.append(y)
    pos += 40
    rc, y = call(x[:, pos:pos + 0], True)
    assert rc == 0 and got.value == d
    outs.append(y)
    for b in range(S):
        assert np.array_equal(np.concatenate([o[b] for o in outs]), stage.decorrelate(x[b, :pos]))
