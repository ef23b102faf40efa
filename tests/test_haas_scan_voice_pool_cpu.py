"""CPU tier of the Haas-delay scan voice pool (include/vnd_haas_scan_voice_stream.h; optimization.HaasScanVoicePool,
haas_scan_voice_pool, haas_scan_voice_spans; _native_haas_scan_voice.py): the NumPy model of the slot rule against a list
that appends frames, keeps the last W and clears on START; the dict form's refusals and bookkeeping before any device call;
and what each wrapper of _native_haas_scan_voice.py hands to the C ABI, parameter by parameter, against the header's
prototypes (that the binding's types are the header's is tests/test_abi.py's, which globs the header by itself)."""
import inspect
import pathlib
import re

import numpy as np
import pytest

from test_native_marshalling_cpu import GEN

REPO = pathlib.Path(__file__).resolve().parents[1]
START, END, SWITCH = 1, 2, 4
HEADER = 'vnd_haas_scan_voice_stream.h'


# ---- the slot rule ------------------------------------------------------------------------------------------------------
class ListVoice:
    """One slot, brute force: the frames of the current voice in a list, of which the last W count; a START, or the
    first answered call after an END (the position is 0 again), begins with an empty list.  `ring` is the W entries as
    the device writes them, frame g at g mod W, never cleared."""

    def __init__(self, W):
        self.W, self.frames, self.pushed, self.ended = W, [], 0, True
        self.ring = [None] * W

    def call(self, names, flags):
        if flags & START or self.ended:
            self.frames, self.pushed = [], 0
        for name in names:
            self.ring[self.pushed % self.W] = name
            self.frames.append(name)
            self.pushed += 1
        self.frames = self.frames[-self.W:]
        self.ended = bool(flags & END)

    @property
    def position(self):
        return 0 if self.ended else self.pushed


@pytest.mark.parametrize('W, M', [(7, 7), (10, 4), (64, 9), (5, 1)])
def test_spans_against_the_list_model(W, M):
    from vndecorrelate_amd.optimization import haas_scan_voice_spans
    rng = np.random.default_rng(100 * W + M)
    S = 12
    voices = [ListVoice(W) for _ in range(S)]
    pos, fill, head = (np.zeros(S, np.int64) for _ in range(3))
    seen = dict(idle=0, bad=0, start=0, end=0, whole=0, wrapped=0, restart_full=0, end_twice=0)
    for call in range(300):
        counts = rng.integers(0, M + 1, S)
        counts[rng.random(S) < 0.3] = 0
        flags = rng.choice([0, 0, 0, 0, START, END, START | END, SWITCH, SWITCH | START], S)
        flags[:3] = START if call == 0 else 0                         # three voices that live long enough to wrap twice
        flags[3] = START if call % 50 == 49 else SWITCH               # ... and one that restarts over a full ring
        spoiled = rng.random(S) < 0.05
        counts[spoiled] = rng.choice([-1, M + 1, 2 ** 31 - 1, -2 ** 31], int(spoiled.sum()))
        valid, new_pos, new_fill, new_head = haas_scan_voice_spans(pos, fill, head, counts, flags, W, M)
        for b, v in enumerate(voices):
            bad = not 0 <= counts[b] <= M
            idle = not bad and counts[b] == 0 and not flags[b] & (START | END)
            assert valid[b] == (-1 if bad else 0 if idle else 1)
            if bad or idle:                                           # nothing of the slot moves
                assert (new_pos[b], new_fill[b], new_head[b]) == (pos[b], fill[b], head[b])
                seen['bad' if bad else 'idle'] += 1
                continue
            seen['restart_full'] += bool(flags[b] & START and fill[b] == W)
            seen['end_twice'] += bool(flags[b] & END and v.ended and not flags[b] & START)
            v.call([(b, call, j) for j in range(counts[b])], int(flags[b]))
            assert new_pos[b] == v.position and new_fill[b] == len(v.frames) == min(v.pushed, W)
            assert new_head[b] == v.pushed % W
            window = [v.ring[(new_head[b] - new_fill[b] + k) % W] for k in range(new_fill[b])]
            assert window == v.frames                                 # the ring entries name the model's frames, in order
            seen['start'] += bool(flags[b] & START)
            seen['end'] += bool(flags[b] & END)
            seen['whole'] += flags[b] & (START | END) == START | END
            seen['wrapped'] += v.pushed > 2 * W
        pos, fill, head = new_pos, new_fill, new_head
    assert all(seen.values()), seen


def test_spans_leave_a_never_reset_position_alone():
    from vndecorrelate_amd.optimization import haas_scan_voice_spans
    pos = np.array([2 ** 60 + 1, -5, 2 ** 60, 2 ** 60 + 1], np.int64)
    fill, head = np.array([3, 4, 5, 6]), np.array([1, 2, 3, 4])
    valid, new_pos, new_fill, new_head = haas_scan_voice_spans(pos, fill, head, [2, 2, 2, 2], [0, 0, 0, START], 8, 4)
    assert valid.tolist() == [-1, -1, 1, 1]
    assert new_pos.tolist() == [2 ** 60 + 1, -5, 2 ** 60 + 2, 2] and new_fill.tolist() == [3, 4, 8, 2]
    assert new_head.tolist() == [1, 2, (2 ** 60 + 2) % 8, 2]
    with pytest.raises(ValueError, match='window_frames'):
        haas_scan_voice_spans(pos, fill, head, [0] * 4, [0] * 4, 0, 4)


# ---- the dict form ------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    from vndecorrelate_amd import _native

    def refuse(*a, **k):
        raise AssertionError('the call reached the device')
    monkeypatch.setattr(_native, 'default_context', refuse)
    monkeypatch.setattr(_native, 'torch_module', refuse)


def _pool(**over):
    from vndecorrelate_amd import optimization
    settings = dict(in_channels=2, max_frames_per_call=100, window_frames=250, max_delay_seconds=0.02, sample_rate_hz=48000)
    settings.update(over)
    return optimization.haas_scan_voice_pool(4, **settings)


def test_the_factory_and_its_refusals(no_device):
    pool = _pool()
    assert (pool.slots, pool.in_channels, pool.max_frames_per_call, pool.window_frames) == (4, 2, 100, 250)
    assert pool.max_delay == 960 and pool.chunks_per_pair == 1 and not pool.ms_mode and pool.width is None
    assert _pool(max_delay_seconds=0.0125, sample_rate_hz=44100).max_delay == 551        # 551.25
    assert _pool(max_delay_seconds=2.5, sample_rate_hz=1).max_delay == 2                 # ties to even, as HaasEffect
    assert _pool(mode='MS', delayed_channel=1, width=0.3, in_channels=1).ms_mode
    with pytest.raises(ValueError, match='window_frames 99 below max_frames_per_call 100'):
        _pool(window_frames=99)
    for bad in (dict(in_channels=3), dict(delayed_channel=2), dict(mode='XY'), dict(max_frames_per_call=0),
                dict(sample_rate_hz=0), dict(max_delay_seconds=-1.0), dict(width=float('nan')),
                dict(window_frames=2 ** 31)):
        with pytest.raises(ValueError):
            _pool(**bad)
    from vndecorrelate_amd import optimization
    with pytest.raises(ValueError, match='split the pool'):
        optimization.haas_scan_voice_pool(65536, in_channels=2, max_frames_per_call=100, window_frames=250,
                                          max_delay_seconds=0.02, sample_rate_hz=48000)


def test_the_dict_form_refuses_before_the_device(no_device):
    pool = _pool()
    block = np.zeros((10, 2), np.float32)
    with pytest.raises(ValueError, match='slot 4 is outside the pool of 4 slots'):
        pool.process({4: block}, start=[4])
    with pytest.raises(ValueError, match='slot -1 is outside'):
        pool.process({}, end=[-1])
    with pytest.raises(ValueError, match='101 frames in one call, above max_frames_per_call=100'):
        pool.process({0: np.zeros((101, 2), np.float32)}, start=[0])
    with pytest.raises(ValueError, match='never started'):
        pool.process({1: block})
    with pytest.raises(ValueError, match='expected \\(frames, 2\\)'):
        pool.process({0: np.zeros((10,), np.float32)}, start=[0])
    with pytest.raises(TypeError, match='float32'):
        pool.process({0: np.zeros((10, 2), np.float64)}, start=[0])
    with pytest.raises(ValueError, match='named twice'):
        pool.process({}, start=[2, 2])
    assert pool.process({}) == {} and pool._form is None and not pool.positions.any()
    for delays in ([-1], [961], [], [[1, 2]], [0.5]):
        with pytest.raises(ValueError, match='delays'):
            pool.scan(np.asarray(delays))


@pytest.mark.parametrize('settings', [dict(mode='MS'), dict(delayed_channel=1), dict(width=0.5)])
def test_optimize_refuses_an_uncovered_configuration(no_device, settings):
    with pytest.raises(ValueError, match="optimize searches HaasEffect\\(mode='LR', delayed_channel=0, width=None\\)"):
        _pool(**settings).optimize()
    pool = _pool()
    with pytest.raises(ValueError, match='slot 9 is outside'):
        pool.optimize([0, 9])
    with pytest.raises(ValueError, match='grid_size'):
        pool.optimize(grid_size=0)
    assert pool.optimize([]).shape == (0,)


def test_the_dict_form_keeps_the_mirror(no_device):
    """The bookkeeping tests/test_meter_pool_dict_form_cpu.py holds the other meters to, over a stand-in for the push."""
    from vndecorrelate_amd import _native
    from vndecorrelate_amd.optimization import haas_scan_voice_spans
    pool = _pool(in_channels=1)
    S, M, W = pool.slots, pool.max_frames_per_call, pool.window_frames
    state = [np.zeros(S, np.int64) for _ in range(3)]
    calls = []

    def host(x, counts, flags, rows=True):
        assert x.shape == (S, M, 1) and x.dtype == np.float32 and counts.dtype == flags.dtype == np.int32 and rows is False
        calls.append((x.copy(), counts.copy(), flags.copy()))
        valid, *state[:] = haas_scan_voice_spans(*state, counts, flags, W, M)
        return None, valid.astype(np.int32)
    pool._call_host = host
    a = np.arange(M, dtype=np.float32)
    assert pool.process({0: a, 2: a[:7, None]}, start=[0, 2, 3]) == {0: None, 2: None, 3: None}
    x, counts, flags = calls[-1]
    assert counts.tolist() == [M, 0, 7, 0] and flags.tolist() == [START, 0, START, START]
    assert x[0, :, 0].tobytes() == a.tobytes() and x[2, :7, 0].tobytes() == a[:7].tobytes() and not x[2, 7:].any()
    for _ in range(3):
        assert pool.process({0: a}) == {0: None}
    assert pool.positions.tolist() == state[0].tolist() == [4 * M, 0, 7, 0] and state[1].tolist() == [W, 0, 7, 0]
    assert state[2].tolist() == [4 * M % W, 0, 7, 0]
    assert pool.process({0: a[:0]}) == {} and len(calls) == 4          # an empty block alone: no device call
    assert pool.process({2: a[:3]}, end=[0, 2]) == {0: None, 2: None}
    assert pool.positions.tolist() == [0, 0, 0, 0] and pool.live.tolist() == [False, False, False, True]
    assert state[1].tolist() == [W, 0, 10, 0]                           # an END leaves the window
    with pytest.raises(ValueError, match='slot 3 holds a live voice'):
        pool.process({}, start=[3])
    pool._call_host = lambda x, c, f, rows=True: (None, np.array([0, 0, 0, 0], np.int32))
    with pytest.raises(_native.NativeError, match='the voice pool answered .* the spans are'):
        pool.process({3: a[:1]})
    with pytest.raises(RuntimeError, match='runs through process\\(\\)'):
        pool.process_dev(None, None, None)


def test_scores_numpy_form_is_scores_from_moments(no_device):
    from vndecorrelate_amd.optimization import scores_from_moments
    rng = np.random.default_rng(5)
    m = np.abs(rng.normal(size=(3, 5, 8))) + 0.1
    weights = dict(angle_limit=0.7, lambda_mean=5.0, lambda_skew=2.0, lambda_correlation=15.0, lambda_penalty=1e3)
    got = _pool().scores(m, **weights)
    assert got.shape == (3, 5) and got.tobytes() == scores_from_moments(m.reshape(-1, 8), **weights).tobytes()
    with pytest.raises(ValueError, match='moments of shape'):
        _pool().scores(np.zeros((3, 7)))


# ---- marshalling: every wrapper of _native_haas_scan_voice.py against the header's prototype ----------------------------
WRAPPERS = {'haas_scan_voice_stream_state_bytes': 'vnd_haas_scan_voice_stream_state_bytes',
            'haas_scan_voice_stream_reset_device': 'vnd_haas_scan_voice_stream_reset_dev',
            'haas_scan_voice_stream_push_device': 'vnd_haas_scan_voice_stream_push_f32_dev',
            'haas_scan_voice_stream_workspace_bytes': 'vnd_haas_scan_voice_stream_workspace_bytes',
            'haas_scan_voice_stream_pairs_device': 'vnd_haas_scan_voice_stream_pairs_f64_dev'}
PYTHON_NAMES = {'in_channels': 'channels', 'hip_stream': 'stream', 'ms': 'ms_mode'}


def _prototype(function: str):
    """The parameter names of `function` in the header, in order."""
    text = re.sub(r'/\*.*?\*/', ' ', (REPO / 'include' / HEADER).read_text(), flags=re.S)
    match = re.search(r'\b' + function + r'\s*\(([^)]*)\)\s*;', text)
    assert match, function
    return [re.split(r'[\s\*]+', p.strip())[-1] for p in match.group(1).split(',')]


def test_every_public_wrapper_is_listed():
    from vndecorrelate_amd import _native, _native_haas_scan_voice
    public = [name for name, f in vars(_native_haas_scan_voice).items()
              if inspect.isfunction(f) and f.__module__ == _native_haas_scan_voice.__name__ and not name.startswith('_')]
    assert sorted(public) == sorted(WRAPPERS)
    assert _native.HEADERS[HEADER] is _native.HAAS_SCAN_VOICE_STREAM_SIGNATURES
    assert sorted(_native.HAAS_SCAN_VOICE_STREAM_SIGNATURES) == sorted(WRAPPERS.values())
    assert '_host' not in re.sub(r'/\*.*?\*/', ' ', (REPO / 'include' / HEADER).read_text(), flags=re.S)


@pytest.mark.parametrize('name', sorted(WRAPPERS))
@pytest.mark.parametrize('width, flag', [(None, False), (0.5, True)])
def test_wrapper_hands_each_parameter_to_its_place(name, width, flag, monkeypatch):
    from vndecorrelate_amd import _native, _native_haas_scan_voice
    function = WRAPPERS[name]
    c_names = _prototype(function)
    lib = GEN.RecordingLibrary(_native)
    monkeypatch.setattr(_native, '_lib', lib)
    fn = getattr(_native_haas_scan_voice, name)
    sent, expect = {}, {}
    for i, p in enumerate(inspect.signature(fn).parameters.values()):
        if p.name == 'ctx':
            sent[p.name], expect['ctx'] = GEN.Handle(lib, GEN.CTX_HANDLE), GEN.CTX_HANDLE
        elif p.name == 'width':
            sent[p.name] = width
            expect['use_width'], expect['width'] = int(width is not None), float(width or 0.0)
        elif p.name == 'ms_mode':
            sent[p.name], expect[p.name] = flag, int(flag)
        else:
            sent[p.name] = expect[p.name] = 1000 + 16 * i             # one sentinel per parameter
    returned = fn(**sent)
    (called, args), = lib.calls
    assert called == function and len(args) == len(c_names)
    for c_name, got in zip(c_names, args):
        if c_name == 'bytes':
            assert got == 'out' and returned == 4000                   # the stand-in's value for the first out-parameter
        else:
            python = PYTHON_NAMES.get(c_name, c_name[:-4] + '_ptr' if c_name.endswith('_dev') else c_name)
            assert got == expect[python], (function, c_name, got)
    numbers = [a for a in args if isinstance(a, (int, float)) and not isinstance(a, bool) and a not in (0, 1)]
    assert len(numbers) == len(set(numbers))                           # the sentinels tell the arguments apart
