"""CPU tier of the crossfading voice pool (include/vnd_voice_fade_stream.h; streaming.FadeVoicePool, voice_fade_spans,
fade_gains; _native_fade.py): the NumPy mirror against the header's block restated in Python integers, the reference
blend's own properties, the gains, every dict-form refusal before the device, the dispatch of decorrelate_voice_pool, and
what each wrapper of _native_fade.py hands to the C ABI, parameter by parameter, against the header's prototypes."""
import inspect
import pathlib
import re

import numpy as np
import pytest

from test_native_marshalling_cpu import GEN
from voice_fade_cases import END, MAX_POSITION, RAGGED, START, SWITCH, bank_latency, blend, one_slot, ragged_schedule

REPO = pathlib.Path(__file__).resolve().parents[1]


# ---- the spans mirror ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F', [0, 1, 200, 1500])
def test_spans_mirror_is_the_headers_block(F):
    from vndecorrelate_amd.streaming import voice_fade_spans
    rng = np.random.default_rng(10 + F)
    S, M, H, T = 16, 600, 319, 5
    pos = np.zeros(S, np.int64)
    rec = rng.integers(-2 ** 62, 2 ** 62, (S, 3))                     # never cleared: whatever the memory held
    pos[3], rec[3] = MAX_POSITION - 700, (MAX_POSITION - 3000, 1, 2)           # a long-lived voice, close to the limit
    pos[4], rec[4] = MAX_POSITION - 100, (MAX_POSITION - 100 - H - F // 2, 0, 4)
    pos[5] = MAX_POSITION + 1                                          # a state that was never reset
    seen = dict(accepted=0, refused=0, fresh_switch=0, bad=0, idle=0, whole=0, end_alone=0)
    for call in range(300):
        counts = rng.choice([0, 0, 1, 7, 64, 599, 600], S).astype(np.int64)
        flags = rng.choice([0, 0, 0, START, END, START | END, SWITCH, SWITCH, SWITCH | END, START | SWITCH], S).astype(np.int64)
        counts[rng.random(S) < 0.03] = rng.choice([-1, M + 1, 2 ** 31 - 1, -2 ** 31])
        tables = rng.integers(0, T, S).astype(np.int64)
        got = voice_fade_spans(pos, rec, counts, flags, tables, H, F, M)
        assert [g.dtype for g in got] == [np.int64] * 4 and got[2].shape == (S, 3)
        for b in range(S):
            n_out, new, record, left, E, accept = one_slot(pos[b], rec[b], counts[b], flags[b], tables[b], H, F, M)
            assert (int(got[0][b]), int(got[1][b]), tuple(int(v) for v in got[2][b]), int(got[3][b])) == \
                (n_out, new, record, left), (call, b, int(pos[b]), tuple(rec[b]), int(counts[b]), int(flags[b]))
            fresh = bool(flags[b] & START) or pos[b] == 0
            seen['bad'] += n_out < 0
            seen['accepted'] += accept
            seen['refused'] += bool(flags[b] & SWITCH) and not fresh and n_out >= 0 and not accept
            seen['fresh_switch'] += bool(flags[b] & SWITCH) and fresh
            seen['idle'] += counts[b] == 0 and flags[b] == 0
            seen['whole'] += flags[b] & (START | END) == START | END
            seen['end_alone'] += counts[b] == 0 and flags[b] == END
        _, pos, rec, _ = got
    if F == 0:                                                         # a hard switch is whole at once: none is ever refused
        assert seen.pop('refused') == 0
    assert all(seen.values()), seen


def test_spans_mirror_without_a_switch_is_voice_spans():
    from vndecorrelate_amd.streaming import voice_fade_spans, voice_spans
    rng = np.random.default_rng(3)
    S, M, H = 8, 600, 319
    pos, rec = np.zeros(S, np.int64), np.zeros((S, 3), np.int64)
    for _ in range(100):
        counts = rng.integers(-1, M + 2, S)
        flags = rng.choice([0, 0, START, END, START | END], S)
        tables = rng.integers(0, 5, S)
        out, new, rec, left = voice_fade_spans(pos, rec, counts, flags, tables, H, 200, M)
        want_out, want_new = voice_spans(pos, counts, flags, H, M)
        assert out.tolist() == want_out.tolist() and new.tolist() == want_new.tolist()
        assert set(left[out >= 0].tolist()) <= {0} and (left[out < 0] == -1).all()
        pos = new
    with pytest.raises(ValueError, match='records of shape'):
        voice_fade_spans(pos, rec[:, :2], counts, flags, tables, H, 200, M)


def test_the_ragged_schedule_meets_every_case():
    """The schedule the GPU tier runs, counted on the CPU with the restatement alone: none of the cases is missing."""
    H = bank_latency()
    assert 200 < H <= 319
    calls, voices, counted = ragged_schedule(RAGGED['seed'], H=H, **RAGGED['shape'])
    # at F = 200 no fade reaches frame 512 of a row (a fade's frames are a row's first): that case is test 3's, F = 1500
    assert counted['crosses_512'] == 0 and all(counted[case] for case in RAGGED['cases']), counted
    _, _, long_fade = ragged_schedule(RAGGED['lengths_seed'], H=H, **{**RAGGED['shape'], 'F': 1500})     # test_fade_lengths'
    assert all(long_fade[case] for case in RAGGED['long_cases']), long_fade
    for F in (0, 1):
        _, _, short = ragged_schedule(RAGGED['lengths_seed'], H=H, **{**RAGGED['shape'], 'F': F})
        assert short['accepted'] and short['switch_on_fresh'], (F, short)
    mono = ragged_schedule(RAGGED['seed'], H=H, **{**RAGGED['shape'], 'cx': 1})
    assert mono[2] == counted and [c[1].tolist() for c in mono[0]] == [c[1].tolist() for c in calls]
    switches = sorted({len(v.fades) for vs in voices.values() for v in vs})
    assert switches[0] == 0 and switches[-1] == 3, switches
    assert any(len(vs) > 1 for vs in voices.values())                  # a slot reused after END
    assert {int(c) for _, counts, _, _ in calls for c in counts} >= {0, 1, 7, 64, 599, 600}


# ---- the reference blend ------------------------------------------------------------------------------------------------
def test_reference_blend():
    rng = np.random.default_rng(5)
    N = 1000
    conv = {t: rng.uniform(-1, 1, (N, 2)).astype(np.float32) for t in range(3)}
    from vndecorrelate_amd.streaming import fade_gains
    hard = blend(conv, 0, [(300, 0, 2)], fade_gains(0), 0)             # F = 0: a hard switch
    assert hard[:300].tobytes() == conv[0][:300].tobytes() and hard[300:].tobytes() == conv[2][300:].tobytes()
    F = 200
    g = fade_gains(F, 'equal_power')
    fades = [(100, 0, 1), (450, 1, 1), (900, 1, 2)]                    # the last one is cut short by the voice's end
    out = blend(conv, 0, fades, g, F)
    for lo, hi, t in ((0, 100, 0), (300, 450, 1), (650, 900, 1)):      # outside every [s, s + F): one table's bytes
        assert out[lo:hi].tobytes() == conv[t][lo:hi].tobytes()
    j = 37
    for s, old, cur in fades:
        want = conv[old][s + j] * g[0][j] + conv[cur][s + j] * g[1][j]
        assert out[s + j].tobytes() == want.astype(np.float32).tobytes()
    same = conv[1][450:650] * g[0][:, None] + conv[1][450:650] * g[1][:, None]          # a fade to the table it has
    assert out[450:650].tobytes() == same.tobytes() and same.tobytes() != conv[1][450:650].tobytes()
    assert np.isnan(blend(conv, 0, [(100, 0, 7)], g, F)[100:]).all()   # a table outside the bank
    assert not np.isnan(blend(conv, 0, [(100, 0, 7)], g, F)[:100]).any()


# ---- the gains ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F', [0, 1, 200, 4097])
def test_named_gains(F):
    from vndecorrelate_amd.streaming import fade_gains
    lin, eq = fade_gains(F), fade_gains(F, 'equal_power')
    assert lin.dtype == eq.dtype == np.float32 and lin.shape == eq.shape == (2, F)
    for j in range(F):
        rise = np.float32((j + 1) / (F + 1))
        assert lin[1][j] == rise and lin[0][j] == np.float32(1) - rise
        angle = np.pi / 2 * (j + 1) / (F + 1)
        assert eq[1][j] == np.float32(np.sin(angle)) and eq[0][j] == np.float32(np.cos(angle))
    assert ((lin > 0) & (lin < 1)).all() and ((eq > 0) & (eq < 1)).all()


def test_custom_gains():
    from vndecorrelate_amd.streaming import VOICE_FADE_MAX_FRAMES, fade_gains
    out, rise = np.linspace(1, 0, 8, dtype=np.float32), np.linspace(0, 1, 8, dtype=np.float32)
    got = fade_gains(8, (out, rise))
    assert got.dtype == np.float32 and got[0].tobytes() == out.tobytes() and got[1].tobytes() == rise.tobytes()
    bad = rise.copy()
    bad[3] = np.inf
    nan = rise.copy()
    nan[0] = np.nan
    for pair in ((out[:7], rise), (out, rise[:7]), (out.astype(np.float64), rise), (out, list(rise)), (out, bad), (nan, rise),
                 (out,), 'cosine', None):
        with pytest.raises(ValueError):
            fade_gains(8, pair)
    for frames in (-1, VOICE_FADE_MAX_FRAMES + 1, 2.0, True, None):
        with pytest.raises(ValueError, match='fade_frames'):
            fade_gains(frames)


# ---- the dict form's refusals, and the dispatch ------------------------------------------------------------------------
def _velvets(dec, kappas, **kw):
    return [dec.VelvetNoise(sample_rate_hz=16000, duration_seconds=0.02, num_impulses=15, log_distribution_strength=k,
                            seed=1, normalizer=None, **kw) for k in kappas]


@pytest.fixture
def dec():
    import vndecorrelate_amd.decorrelation as decorrelation
    return decorrelation


def test_switch_refusals_come_before_the_device(dec, monkeypatch):
    from vndecorrelate_amd import streaming
    pool = dec.decorrelate_voice_pool(_velvets(dec, (0.0, 0.3, 0.8)), slots=4, max_frames_per_call=600, fade_frames=200)
    assert type(pool) is streaming.FadeVoicePool and pool.fade_frames == 200
    assert pool.fade_gains.tobytes() == streaming.fade_gains(200, 'linear').tobytes()
    assert pool.fade_left.tolist() == [0] * 4

    def reached(*args, **kwargs):
        pytest.fail('a refused call reached the device')
    monkeypatch.setattr(pool, '_call_host', reached)
    monkeypatch.setattr(pool, '_call_device', reached)
    monkeypatch.setattr(pool, '_ensure_state', reached)
    block = np.zeros((100, 2), np.float32)
    pool.live[:2] = True                                               # slots 0 and 1 hold live voices, as the mirror has it
    pool.positions[:2] = 1000
    pool.fade_left[1] = 50
    before = (pool.positions.copy(), pool.records.copy(), pool.fade_left.copy(), pool.live.copy(), pool.tables.copy())
    for kwargs, text in ((dict(switch={2: 1}), 'slot 2 holds no live voice'),
                         (dict(blocks={2: block}, start={2: 0}, switch={2: 1}), 'slot 2 starts with this call'),
                         (dict(start={0: 1}, switch={0: 2}, discard=True), 'slot 0 starts with this call'),
                         (dict(switch={0: 3}), 'bank index 3 of slot 0 is outside the bank of 3'),
                         (dict(switch={0: -1}), 'outside the bank'), (dict(switch={0: True}), 'outside the bank'),
                         (dict(switch={0: 1.0}), 'outside the bank'),
                         (dict(switch={4: 0}), 'slot 4 is outside the pool'), (dict(switch={-1: 0}), 'outside the pool'),
                         (dict(blocks={1: block}, switch={1: 2}), 'slot 1 has 50 frames of its fade left')):
        with pytest.raises(ValueError, match=text):
            pool.process(kwargs.pop('blocks', None), **kwargs)
        for kept, was in zip((pool.positions, pool.records, pool.fade_left, pool.live, pool.tables), before):
            assert kept.tolist() == was.tolist()
    with pytest.raises(RuntimeError, match='reset\\(\\) first'):
        pool.fade_left_dev


def test_dispatch_of_decorrelate_voice_pool(dec):
    from vndecorrelate_amd import streaming
    velvets = _velvets(dec, (0.0, 0.3))
    assert type(dec.decorrelate_voice_pool(velvets, slots=2)) is streaming.VoicePool
    assert type(dec.decorrelate_voice_pool(velvets, slots=2, fade_frames=None, fade='equal_power')) is streaming.VoicePool
    hard = dec.decorrelate_voice_pool(velvets, slots=2, fade_frames=0)
    assert type(hard) is streaming.FadeVoicePool and hard.fade_gains.shape == (2, 0)
    eq = dec.decorrelate_voice_pool(velvets, slots=2, fade_frames=64, fade='equal_power')
    assert eq.fade_gains.tobytes() == streaming.fade_gains(64, 'equal_power').tobytes()
    haas = [dec.HaasEffect(sample_rate_hz=16000, delay_time_seconds=0.01 * (i + 1)) for i in range(2)]
    chains = [dec.SignalChain(sample_rate_hz=16000).velvet_noise(duration_seconds=0.02, num_impulses=15, seed=3)
              .haas_effect(delay_time_seconds=0.01) for _ in range(2)]
    for bank in (haas, chains):
        with pytest.raises(ValueError, match='fade_frames is taken with a bank of plain VelvetNoise'):
            dec.decorrelate_voice_pool(bank, slots=2, fade_frames=64)
    assert type(dec.decorrelate_voice_pool(haas, slots=2)) is streaming.HaasVoicePool
    for frames in (-1, (1 << 20) + 1, 2.5):
        with pytest.raises(ValueError, match='fade_frames'):
            dec.decorrelate_voice_pool(velvets, slots=2, fade_frames=frames)
    with pytest.raises(ValueError, match='linear'):
        dec.decorrelate_voice_pool(velvets, slots=2, fade_frames=8, fade='cosine')


# ---- marshalling: every wrapper of _native_fade.py against the header's prototype ---------------------------------------
def _prototype(header: str, function: str):
    """The parameter names of `function` in include/<header>, in order."""
    text = re.sub(r'/\*.*?\*/', ' ', (REPO / 'include' / header).read_text(), flags=re.S)
    match = re.search(r'\b' + function + r'\s*\(([^)]*)\)\s*;', text)
    assert match, (header, function)
    return [re.split(r'[\s\*]+', p.strip())[-1] for p in match.group(1).split(',')]


# wrapper -> (header, C function, what follows the wrapper's own out-parameter or buffer in the C call)
WRAPPERS = {
    'voice_fade_stream_state_bytes': ('vnd_voice_fade_stream.h', 'vnd_voice_fade_stream_state_bytes'),
    'voice_fade_stream_reset_device': ('vnd_voice_fade_stream.h', 'vnd_voice_fade_stream_reset_dev'),
    'voice_fade_stream_device': ('vnd_voice_fade_stream.h', 'vnd_voice_fade_stream_f32_dev'),
    'describe_voice_fade_stream': ('vnd_amd_internal.h', 'vnd_describe_voice_fade_stream_launch'),
}


def _python_name(c_name: str) -> str:
    """The wrapper's parameter for a C parameter: addresses are `*_ptr`, the channel count and the stream are short."""
    if c_name in ('in_channels', 'hip_stream'):
        return {'in_channels': 'channels', 'hip_stream': 'stream'}[c_name]
    return c_name[:-4] + '_ptr' if c_name.endswith('_dev') else c_name


def test_every_public_wrapper_is_listed():
    from vndecorrelate_amd import _native_fade
    public = [name for name, f in vars(_native_fade).items()
              if inspect.isfunction(f) and f.__module__ == _native_fade.__name__ and not name.startswith('_')]
    assert sorted(public) == sorted(WRAPPERS)
    from vndecorrelate_amd import _native
    assert _native_fade.VOICE_SWITCH == _native.VOICE_SWITCH == SWITCH == 4
    assert _native.VOICE_FADE_MAX_FRAMES == 1 << 20
    text = (REPO / 'include' / 'vnd_voice_fade_stream.h').read_text()
    assert '#define VND_VOICE_SWITCH 4' in text and '#define VND_VOICE_FADE_MAX_FRAMES (1 << 20)' in text
    assert 'vnd_voice_fade_stream.h' in _native.HEADERS
    assert 'vnd_describe_voice_fade_stream_launch' in _native.INTERNAL_SIGNATURES


@pytest.mark.parametrize('name', sorted(WRAPPERS))
@pytest.mark.parametrize('width', [None, 0.5])
@pytest.mark.parametrize('flag', [False, True])
def test_wrapper_hands_each_parameter_to_its_place(name, width, flag, monkeypatch):
    from vndecorrelate_amd import _native, _native_fade
    header, function = WRAPPERS[name]
    c_names = _prototype(header, function)
    lib = GEN.RecordingLibrary(_native)
    monkeypatch.setattr(_native, '_lib', lib)
    fn = getattr(_native_fade, name)
    sent, expect = {}, {}
    for i, p in enumerate(inspect.signature(fn).parameters.values()):
        if p.name == 'ctx':
            sent[p.name], expect['ctx'] = GEN.Handle(lib, GEN.CTX_HANDLE), GEN.CTX_HANDLE
        elif p.name == 'bank':
            bank = GEN.Handle(lib, GEN.BANK_HANDLE)
            bank.ctx = GEN.Handle(lib, GEN.CTX_HANDLE)                 # (a table knows its context: the describe hook's)
            sent[p.name], expect['bank'] = bank, GEN.BANK_HANDLE
            expect.setdefault('ctx', GEN.CTX_HANDLE)
        elif p.name == 'width':
            sent[p.name] = width
            expect['use_width'], expect['width'] = int(width is not None), float(width or 0.0)
        elif p.name in ('ms_encode', 'epilogue'):
            sent[p.name], expect[p.name] = flag, int(flag)
        else:
            sent[p.name] = expect[p.name] = 1000 + 16 * i
    returned = fn(**sent)
    (called, args), = lib.calls
    assert called == function and len(args) == len(c_names)
    for c_name, got in zip(c_names, args):
        if c_name == 'bytes':
            assert got == 'out' and returned == 4000                   # the stand-in's value for the first out-parameter
        elif c_name == 'text':
            assert got == 512 and returned == 'launch 1'
        elif c_name == 'len':
            assert got == 512
        else:
            assert got == expect[_python_name(c_name)], (function, c_name, got)
    numbers = [a for a in args if isinstance(a, (int, float)) and not isinstance(a, bool) and a not in (0, 1, 512)]
    assert len(numbers) == len(set(numbers))                           # the sentinels tell the arguments apart


def test_a_null_gains_and_a_null_fade_left_go_down_as_null(monkeypatch):
    from vndecorrelate_amd import _native, _native_fade
    lib = GEN.RecordingLibrary(_native)
    ctx, bank = GEN.Handle(lib, GEN.CTX_HANDLE), GEN.Handle(lib, GEN.BANK_HANDLE)
    _native_fade.voice_fade_stream_device(ctx, bank, 16, 32, 48, 0, None, 64, 80, 96, 112, 128, 144, None, 6, 2,
                                          ms_encode=False, width=None, stream=7)
    (_, args), = lib.calls
    names = _prototype('vnd_voice_fade_stream.h', 'vnd_voice_fade_stream_f32_dev')
    assert args[names.index('gains_dev')] == 0 and args[names.index('fade_left_dev')] == 0
    assert args[names.index('mode')] == 0 and args[names.index('hip_stream')] == 7
