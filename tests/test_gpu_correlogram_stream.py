"""GPU tier of the streamed cross-correlogram (vnd_correlogram_stream_f32_dev, analysis.cross_correlogram_stream): under
many shapes and block schedules, for pools of 1 to 512 streams, in every input form, the concatenated rows equal
cross_correlogram_batched on the whole signal bit for bit; the reference's fixtures fed block by block stay within the
bound of DESIGN.md §3.8; reset() leaks nothing; a SignalChain stream can be metered as it runs; an output above 2^31
floats; a stream planted at a position a long-lived one reaches (2^31 .. 2^60), by the ring layout the header documents;
argument checks that write nothing."""
import ctypes
import json
import pathlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = pathlib.Path(__file__).resolve().parents[1]
GOLDEN = REPO / 'tests' / 'golden'
EPS = 1e-10


@pytest.fixture(scope='module')
def an():
    from vndecorrelate_amd import _native, analysis
    ctx = _native.default_context()
    assert 'gfx950' in ctx.info()['name']
    return analysis


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


@pytest.fixture(scope='module')
def dev(torch, an):
    from vndecorrelate_amd import _native
    return torch.device('cuda', _native.default_context().device)


def bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))


def one_shot(an, x, y, W, H, L):
    """The one-shot device call on the whole signal (what cross_correlogram_batched runs), float32 (S, windows, L)."""
    return an.correlogram_numpy_batch(np.ascontiguousarray(x, np.float32),
                                      None if y is None else np.ascontiguousarray(y, np.float32), W, H, L, EPS)


def schedule(kind, n, W, H, top, seed=0):
    if kind == 'whole':
        return [n]
    if kind == 'random':
        rng, out, left = np.random.default_rng(seed), [], n
        while left > 0:
            b = int(min(left, rng.choice([0, 1, int(rng.integers(0, top + 1)), top])))
            out.append(b)
            left -= b
        return out
    if kind == 'zeros':                         # blocks of 0 frames between blocks of H
        out, left = [0], n
        while left > 0:
            out += [min(left, H), 0, 0]
            left -= min(left, H)
        return out
    step = {'H': H, 'W-1': max(1, W - 1), 'top': top, '1': 1}[kind]
    return [step] * (n // step) + ([n % step] if n % step else [])


def feed(s, x, y, sched, to=None):
    """Push x (and y) frame blocks along axis 1 (axis 0 for the unbatched forms); concatenated rows + flush()."""
    axis = 1 if s.num_streams > 1 or x.ndim == (3 if y is None else 2) else 0
    outs, pos = [], 0
    for b in sched:
        sl = [slice(None)] * x.ndim
        sl[axis] = slice(pos, pos + b)
        xb = x[tuple(sl)]
        yb = None if y is None else y[tuple(sl)]
        if to is not None:
            xb = to(xb)
            yb = None if yb is None else to(yb)
        outs.append(s.process(xb, yb))
        assert s.position == pos + b
        pos += b
    outs.append(s.flush())
    if to is not None:
        outs = [o.cpu().numpy() for o in outs]
    return np.concatenate(outs, axis=-2)


def signal(S, n, seed, stereo=False):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (S, n)).astype(np.float32)
    y = (0.6 * x + 0.4 * rng.standard_normal((S, n))).astype(np.float32)
    if stereo:
        return np.stack([x, y], axis=2), None
    return x, y


SHAPES = [  # W, H, num_lags, n
    (882, 441, 1765, 5000),
    (320, 160, 641, 3000),
    (4800, 2400, 9601, 16000),
    (100, 250, 51, 2100),                       # H > W
    (64, 1, 200, 400),                          # H = 1, num_lags > 2W - 1
    (1000, 300, 11, 4200),                      # max_lag < W - 1
    (1, 1, 1, 50),
    (1, 3, 4, 50),
]


@pytest.mark.parametrize('W,H,L,n', SHAPES)
@pytest.mark.parametrize('kind', ['whole', 'H', 'W-1', 'top', 'zeros', 'random'])
def test_schedules_equal_the_one_shot(an, W, H, L, n, kind):
    top = max(700, W - 1, H) if kind != 'whole' else n          # room for blocks of H and of W - 1
    x, y = signal(3, n, W + H + L)
    want = one_shot(an, x, y, W, H, L)
    s = an.CorrelogramStream(3, window=W, hop=H, num_lags=L, epsilon=EPS, max_frames_per_call=top)
    for seed in (range(3) if kind == 'random' else [0]):
        s.reset()
        got = feed(s, x, y, schedule(kind, n, W, H, top, seed))
        assert bits_equal(got, want), (W, H, L, kind, seed)


@pytest.mark.parametrize('W,H,L,n', [(882, 441, 1765, 1800), (64, 1, 200, 150), (100, 250, 51, 600), (1, 1, 1, 20),
                                     (320, 160, 641, 700)])
def test_one_frame_blocks(an, W, H, L, n):
    x, y = signal(1, n, 7 * W + H)
    s = an.CorrelogramStream(1, window=W, hop=H, num_lags=L, epsilon=EPS, max_frames_per_call=1)
    got = feed(s, x[0], y[0], [1] * n)
    assert bits_equal(got, one_shot(an, x, y, W, H, L)[0])


def test_window_16384_once(an):
    W, H, L, n = 16384, 8192, 129, 16384 + 3 * 8192 + 100
    x, y = signal(2, n, 16384)
    s = an.CorrelogramStream(2, window=W, hop=H, num_lags=L, epsilon=EPS, max_frames_per_call=9000)
    got = feed(s, x, y, schedule('random', n, W, H, 9000, 3))
    assert got.shape == (2, 4, L) and bits_equal(got, one_shot(an, x, y, W, H, L))


@pytest.mark.parametrize('S', [1, 3, 512])
def test_pools_equal_single_streams(an, S):
    n = 3000 if S == 512 else 6000
    st, _ = signal(S, n, S, stereo=True)
    s = an.cross_correlogram_stream(S, max_frames_per_call=480)
    got = feed(s, st, None, schedule('random', n, 882, 441, 480, S))
    assert bits_equal(got, an.cross_correlogram_batched(st))
    one = an.cross_correlogram_stream(1, max_frames_per_call=480)
    for b in sorted({0, S // 2, S - 1}):
        one.reset()
        assert bits_equal(feed(one, st[b], None, schedule('random', n, 882, 441, 480, b + 1)), got[b]), b


def test_forms_agree(torch, an, dev):
    S, n = 3, 5000
    st, _ = signal(S, n, 21, stereo=True)
    want = an.cross_correlogram_batched(st)
    sched = schedule('random', n, 882, 441, 480, 21)
    mk = lambda: an.cross_correlogram_stream(S, max_frames_per_call=480)
    x, y = np.ascontiguousarray(st[:, :, 0]), np.ascontiguousarray(st[:, :, 1])
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    assert bits_equal(feed(mk(), st, None, sched), want)                        # (S, B, 2) NumPy
    assert bits_equal(feed(mk(), x, y, sched), want)                            # (x, y) NumPy
    assert bits_equal(feed(mk(), st, None, sched, to=to_dev), want)             # (S, B, 2) device
    assert bits_equal(feed(mk(), x, y, sched, to=to_dev), want)                 # (x, y) device
    # non-contiguous device tensors: channels 1..2 of a (S, n, 4) buffer (frame stride 4), and the two channel views
    # of a (S, n, 2) buffer as a pair (frame stride 2, x and y aliasing); a transposed block (channel-major)
    wide = torch.zeros((S, n, 4), dtype=torch.float32, device=dev)
    wide[:, :, 1:3] = to_dev(st)
    view = wide[:, :, 1:3]
    assert not view.is_contiguous()
    s, outs, pos = mk(), [], 0
    for b in sched:
        outs.append(s.process(view[:, pos:pos + b]))
        assert isinstance(outs[-1], torch.Tensor) and outs[-1].device == dev and outs[-1].dtype == torch.float32
        pos += b
    outs.append(s.flush())
    assert bits_equal(torch.cat(outs, dim=1).cpu().numpy(), want)
    full = to_dev(st)
    s, outs, pos = mk(), [], 0
    for b in sched:
        outs.append(s.process(full[:, pos:pos + b, 0], full[:, pos:pos + b, 1]))
        pos += b
    assert bits_equal(torch.cat(outs + [s.flush()], dim=1).cpu().numpy(), want)
    chan_major = to_dev(np.ascontiguousarray(st.transpose(0, 2, 1))).transpose(1, 2)
    assert chan_major.stride(2) != 1
    assert bits_equal(feed(mk(), chan_major, None, sched, to=lambda a: a), want)
    # the unbatched forms of a pool of one
    one = lambda: an.cross_correlogram_stream(1, max_frames_per_call=480)
    assert bits_equal(feed(one(), st[1], None, sched), want[1])
    assert bits_equal(feed(one(), x[1], y[1], sched), want[1])
    assert bits_equal(feed(one(), st[2], None, sched, to=to_dev), want[2])


def test_float64_blocks_equal_their_float32_casts(torch, an, dev):
    rng = np.random.default_rng(5)
    st = rng.uniform(-1, 1, (2, 4000, 2)) * np.array([1.0, 1e-3])          # float64, values between float32 ones
    want = an.cross_correlogram_batched(st.astype(np.float32))
    sched = schedule('random', 4000, 882, 441, 480, 5)
    mk = lambda: an.cross_correlogram_stream(2, max_frames_per_call=480)
    assert bits_equal(feed(mk(), st, None, sched), want)
    assert bits_equal(feed(mk(), st, None, sched, to=lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)), want)
    assert bits_equal(feed(mk(), st[:, :, 0], st[:, :, 1], sched), want)


def test_reference_fixtures_block_by_block(an):
    import importlib.util
    from vndecorrelate_amd.utils import dsp
    spec = importlib.util.spec_from_file_location('gen_correlogram_golden', REPO / 'tools' / 'gen_correlogram_golden.py')
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    g = np.load(GOLDEN / 'correlogram.npz')
    manifest = json.loads((GOLDEN / 'correlogram_manifest.json').read_text())
    for i, (name, case) in enumerate(manifest['cases'].items()):
        x, y = gen.fixture_inputs(case['input'], g)
        ref = g[name + '__out']
        kw = case['kwargs']
        s = an.cross_correlogram_stream(1, max_frames_per_call=256, **kw)
        got = feed(s, np.asarray(x), np.asarray(y), schedule('random', len(x), s.window, s.hop, 256, i))
        assert got.shape == ref.shape, name
        diff = np.abs(got.astype(np.float64) - ref)
        assert diff.max(initial=0) <= (2 * s.window + 4) * 2.0 ** -24, name
        want = an.cross_correlogram_batched(np.asarray(x)[None], np.asarray(y)[None], **kw)
        assert bits_equal(got, want[0]), name
        if name == 'huge_16k':
            assert not got.any()


@pytest.mark.parametrize('amplitude', [0.0, 1e17])
def test_silent_and_overflowing_windows_give_zero(an, amplitude):
    rng = np.random.default_rng(3)
    x = (rng.uniform(-1, 1, (2, 4000)) * amplitude).astype(np.float32)
    y = (rng.uniform(-1, 1, (2, 4000)) * amplitude).astype(np.float32)
    x[1, 1000:2500] = 0                                                     # silent stretches in a live stream too
    if amplitude == 0.0:
        x[1] = rng.uniform(-1, 1, 4000).astype(np.float32)
        x[1, 1000:2500] = 0
        y[1] = x[1]
    s = an.CorrelogramStream(2, window=320, hop=160, num_lags=641, epsilon=EPS, max_frames_per_call=333)
    got = feed(s, x, y, schedule('random', 4000, 320, 160, 333, 9))
    assert bits_equal(got, one_shot(an, x, y, 320, 160, 641))
    assert not got[0].any()
    if amplitude == 0.0:
        assert not got[1, 7:9].any() and got[1, 0].any()                  # windows inside the silence: 0


def test_reset_leaks_no_stale_frames(an):
    a, _ = signal(2, 6000, 31, stereo=True)
    b, _ = signal(2, 1500, 32, stereo=True)
    s = an.cross_correlogram_stream(2, max_frames_per_call=480)
    for i in range(0, 5000, 480):                                              # a signal cut off without flush
        s.process(a[:, i:i + 480])
    s.reset()
    got = feed(s, b, None, schedule('random', 1500, 882, 441, 480, 2))
    fresh = feed(an.cross_correlogram_stream(2, max_frames_per_call=480), b, None,
                 schedule('random', 1500, 882, 441, 480, 2))
    assert bits_equal(got, fresh) and bits_equal(got, an.cross_correlogram_batched(b))
    s.reset()
    assert s.process(b[:, :400]).shape == (2, 0, 1765)                        # n < W after a reset: no rows yet


def test_meter_of_a_chain_stream(torch, an, dev):
    import vndecorrelate_amd.decorrelation as vnd
    make = lambda: (vnd.SignalChain(sample_rate_hz=48000).velvet_noise(duration_seconds=0.02, seed=1, normalizer=None)
                    .haas_effect(delay_time_seconds=0.005, delayed_channel=1, mode='LR'))
    S, n = 4, 9000
    x = np.random.default_rng(41).uniform(-1, 1, (S, n, 2)).astype(np.float32)
    cs = make().stream(num_streams=S, max_frames_per_call=480)
    meter = an.cross_correlogram_stream(S, sample_rate_hz=48000, max_frames_per_call=4800)
    xd = torch.from_numpy(x).to(dev)
    rows, pos = [], 0
    for b in schedule('random', n, 0, 0, 480, 41):
        y = cs.process(xd[:, pos:pos + b])
        assert y.is_cuda and y.dtype == torch.float64
        rows.append(meter.process(y))
        pos += b
    rows.append(meter.process(cs.flush()))
    rows.append(meter.flush())
    got = torch.cat(rows, dim=1).cpu().numpy()
    chain = make()
    want = an.cross_correlogram_batched(np.stack([chain(x[b]) for b in range(S)]), sample_rate_hz=48000)
    assert got.shape == want.shape and bits_equal(got, want)


def test_output_above_2_to_31_floats(torch, an, dev):
    B, n0, n1, W, H, L = 4, 1000, 4_300_000, 64, 1, 127
    rows1 = (n0 + n1 - W) // H + 1 - ((n0 - W) // H + 1)
    assert B * rows1 * L > 2 ** 31
    rng = np.random.default_rng(14)
    x = rng.uniform(-1, 1, (B, n0 + n1)).astype(np.float32)
    y = rng.uniform(-1, 1, (B, n0 + n1)).astype(np.float32)
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    s = an.CorrelogramStream(B, window=W, hop=H, num_lags=L, epsilon=EPS, max_frames_per_call=n1)
    head = s.process(xd[:, :n0], yd[:, :n0])
    out = s.process(xd[:, n0:], yd[:, n0:])
    assert tuple(out.shape) == (B, rows1, L)
    first = out[0, :3].cpu().numpy()
    last = out[B - 1, -3:].cpu().numpy()
    del out
    torch.cuda.empty_cache()
    start = n0 - W + 1                                                         # the first row of the big call
    want_first = one_shot(an, x[:1, start:start + W + 2], y[:1, start:start + W + 2], W, H, L)[0]
    want_last = one_shot(an, x[B - 1:, -(W + 2):], y[B - 1:, -(W + 2):], W, H, L)[0]
    assert bits_equal(first, want_first) and bits_equal(last, want_last)
    assert bits_equal(head.cpu().numpy(), one_shot(an, x[:, :n0], y[:, :n0], W, H, L))


PLANTED = (2 ** 31 - 7, 2 ** 32 - 300, 2 ** 40 + 3, None)        # None: 2^60 less the frames pushed


@pytest.mark.parametrize('position', PLANTED, ids=['2^31-7', '2^32-300', '2^40+3', 'ends-at-2^60'])
def test_planted_position(torch, an, dev, position):
    """A stream at position P has wc(P) windows behind it; window wc(P) starts at frame A = wc(P) x hop, in (P - W, P].
    The signal starts at A: its frames below P go into the ring (slot = absolute frame mod (W - 1 + M)), the rest is
    pushed, and the rows are the one-shot call's on the signal.  The ring frames [P - W + 1, A) are within reach of P but
    belong to no window still to complete: they hold loud noise, everything else NaN, and no row may show either."""
    from vndecorrelate_amd import _native
    ctx = _native.default_context()
    S, W, H, L, M, n = 3, 320, 160, 641, 333, 1500
    P = 2 ** 60 - n if position is None else position
    w0 = (P - W) // H + 1
    A = w0 * H
    held, cap = P - A, W - 1 + M
    assert 0 < held < W - 1                                                    # there are frames of both kinds
    x, y = signal(S, held + n, 17 + P % 107)
    want = one_shot(an, x, y, W, H, L)
    need = _native.correlogram_stream_state_bytes(S, W, M)
    assert need == S * cap * 8
    state = torch.full((need // 4,), float('nan'), dtype=torch.float32, device=dev)
    history = np.random.default_rng(P % 109).uniform(-1e3, 1e3, (S, W - 1, 2)).astype(np.float32)
    history[:, W - 1 - held:, 0], history[:, W - 1 - held:, 1] = x[:, :held], y[:, :held]
    where = np.array([(P - (W - 1) + j) % cap for j in range(W - 1)], np.int64)  # Python integers: no wrap
    state.view(S, cap, 2)[:, torch.from_numpy(where).to(dev)] = torch.from_numpy(history).to(dev)
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    outs, pos = [], P
    for b in schedule('random', n, W, H, M, P % 113) + [0]:                    # the last call, of no frames, at P + n
        rows = ((pos + b - W) // H + 1) - ((pos - W) // H + 1)
        out = torch.full((S * rows * L + 64,), float('nan'), dtype=torch.float32, device=dev)
        first = held + pos - P
        xb, yb = xd[:, first:first + b].contiguous(), yd[:, first:first + b].contiguous()
        got = _native.correlogram_stream_device(ctx, state.data_ptr(), need, M, xb.data_ptr(), yb.data_ptr(), max(b, 1), 1,
                                                out.data_ptr(), S, pos, b, window=W, hop=H, num_lags=L, eps=EPS, stream=stream)
        assert got == rows, (pos, b)
        oh = out.cpu().numpy()
        assert np.isnan(oh[S * rows * L:]).all() and not np.isnan(oh[:S * rows * L]).any(), (pos, b)
        outs.append(oh[:S * rows * L].reshape(S, rows, L))
        pos += b
    assert pos == P + n and (position is not None or pos == 2 ** 60)
    got = np.concatenate(outs, axis=1)
    assert got.shape == want.shape and want.shape[1] == (held + n - W) // H + 1
    assert bits_equal(got, want), np.argwhere(got.view(np.int32) != want.view(np.int32))[:3]


def test_bad_arguments_write_nothing(torch, an, dev):
    from vndecorrelate_amd import _native
    ctx = _native.default_context()
    lib = ctx._lib
    S, W, H, L, M = 2, 20, 10, 21, 100
    need = _native.correlogram_stream_state_bytes(S, W, M)
    state = torch.full((need // 4,), float('nan'), dtype=torch.float32, device=dev)
    x = torch.ones((S, M), dtype=torch.float32, device=dev)
    out = torch.full((S, 9, L), float('nan'), dtype=torch.float32, device=dev)
    good = dict(state=state.data_ptr(), state_bytes=need, M=M, x=x.data_ptr(), y=x.data_ptr(), ss=M, fs=1,
                out=out.data_ptr(), batch=S, pos=0, n_in=M, W=W, H=H, L=L)

    def call(**kw):
        a = dict(good, **kw)
        rows = ctypes.c_int64(-7)
        rc = lib.vnd_correlogram_stream_f32_dev(
            ctx.handle, ctypes.c_void_p(a['state']), a['state_bytes'], a['M'], ctypes.c_void_p(a['x']),
            ctypes.c_void_p(a['y']), a['ss'], a['fs'], ctypes.c_void_p(a['out']), a['batch'], a['pos'], a['n_in'],
            a['W'], a['H'], a['L'], EPS, ctypes.byref(rows), ctypes.c_void_p(0))
        return rc, rows.value

    invalid = [dict(state_bytes=need - 1), dict(n_in=M + 1), dict(n_in=-1), dict(pos=-1), dict(pos=2 ** 60 + 1), dict(M=0),
               dict(batch=0),
               dict(ss=0), dict(fs=0), dict(W=0), dict(H=0), dict(L=0), dict(H=-3), dict(state=0), dict(x=0), dict(y=0),
               dict(out=0), dict(out=x.data_ptr()), dict(out=state.data_ptr()), dict(x=state.data_ptr()),
               dict(ss=2 ** 62)]
    for kw in invalid:
        assert call(**kw) == (1, 0), kw
    assert call(W=an.MAX_WINDOW + 1, M=10 ** 5)[0] == 4                       # VND_ERR_UNSUPPORTED
    rows = ctypes.c_int64()
    assert lib.vnd_correlogram_stream_f32_dev(None, None, 0, M, None, None, M, 1, None, S, 0, M, W, H, L, EPS,
                                              ctypes.byref(rows), None) == 1
    assert call(n_in=0, state=0, x=0, y=0, out=0) == (0, 0)                   # nothing to do: nothing used
    torch.cuda.synchronize(dev)
    assert torch.isnan(out).all() and torch.isnan(state).all()
    assert call() == (0, 9)                                                   # the good call writes
    torch.cuda.synchronize(dev)
    assert not torch.isnan(out).any()
