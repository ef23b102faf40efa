"""CPU tier of the crossfading Haas and chain voice pools (include/vnd_haas_voice_fade_stream.h; streaming.HaasFadeVoicePool,
ChainFadeVoicePool, haas_voice_fade_spans; decorrelation.decorrelate_fade_voice_pool; _native_haas_fade.py): the NumPy mirror
against the header's block restated in Python integers, the tail against a frame-by-frame count, the NumPy reference against
the oracle, every dict-form refusal before the device, the dispatch, and what each wrapper of _native_haas_fade.py hands to
the C ABI, parameter by parameter, against the header's prototypes."""
import inspect
import pathlib
import re

import numpy as np
import pytest

from haas_voice_fade_cases import (CHAIN, END, MAX_POSITION, RAGGED, START, SWITCH, chain_schedule, haas_fade, one_slot,
                                   ragged_schedule, tail_by_count)
from test_native_marshalling_cpu import GEN

REPO = pathlib.Path(__file__).resolve().parents[1]


# ---- the spans mirror ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F', [0, 1, 200, 1500])
def test_spans_mirror_is_the_headers_block(F):
    from vndecorrelate_amd.streaming import haas_voice_fade_spans
    rng = np.random.default_rng(20 + F)
    S, M, D = 16, 300, 400
    pos = np.zeros(S, np.int64)
    rec = rng.integers(-2 ** 62, 2 ** 62, (S, 3))                     # never cleared: whatever the memory held
    pos[3], rec[3] = MAX_POSITION - 700, (MAX_POSITION - 3000, 1, 400)         # a long-lived voice, close to the limit
    pos[4], rec[4] = MAX_POSITION - 100, (MAX_POSITION - 100 - F // 2, 0, 7)   # ... and one inside a fade there
    pos[5] = MAX_POSITION + 1                                          # a state that was never reset
    pos[6], rec[6] = 5000, (100, 3, D + 1)                             # a record no call of the pool wrote
    pos[7], rec[7] = 2 ** 32 - 50, (2 ** 62, 5, 9)                     # a planted s far ahead: no sum wraps
    seen = dict(accepted=0, refused=0, fresh_switch=0, switch_alone=0, bad_count=0, bad_delay_taken=0, bad_delay_unread=0,
                bad_record=0, idle=0, whole=0, end_alone=0, near_limit=0)
    for call in range(400):
        counts = rng.choice([0, 0, 1, 7, 64, 299, 300], S).astype(np.int64)
        flags = rng.choice([0, 0, 0, START, END, START | END, SWITCH, SWITCH, SWITCH | END, START | SWITCH], S).astype(np.int64)
        spoiled = rng.random(S) < 0.03
        counts[spoiled] = rng.choice([-1, M + 1, 2 ** 31 - 1, -2 ** 31])
        delays = rng.choice([0, 1, 7, 150, 399, 400], S).astype(np.int64)
        wrong = rng.random(S) < 0.1
        delays[wrong] = rng.choice([-1, D + 1, 2 ** 31 - 1, -2 ** 31])
        got = haas_voice_fade_spans(pos, rec, counts, flags, delays, D, F, M)
        assert [g.dtype for g in got] == [np.int64] * 4 and got[2].shape == (S, 3)
        for b in range(S):
            n_out, new, record, left, accept = one_slot(pos[b], rec[b], counts[b], flags[b], delays[b], D, F, M)
            assert (int(got[0][b]), int(got[1][b]), tuple(int(v) for v in got[2][b]), int(got[3][b])) == \
                (n_out, new, record, left), (call, b, int(pos[b]), tuple(rec[b]), int(counts[b]), int(flags[b]), int(delays[b]))
            fresh = bool(flags[b] & START) or pos[b] == 0
            work = counts[b] > 0 or flags[b] != 0
            count_ok = 0 <= counts[b] <= M
            seen['bad_count'] += not count_ok
            seen['bad_delay_taken'] += count_ok and n_out < 0 and wrong[b] and b not in (5, 6)
            seen['bad_delay_unread'] += wrong[b] and n_out >= 0
            seen['bad_record'] += b == 6 and n_out < 0 and count_ok and not fresh
            seen['accepted'] += accept
            seen['switch_alone'] += accept and counts[b] == 0 and flags[b] == SWITCH
            seen['refused'] += bool(flags[b] & SWITCH) and not fresh and n_out >= 0 and not accept
            seen['fresh_switch'] += bool(flags[b] & SWITCH) and fresh
            seen['idle'] += not work and n_out == 0
            seen['whole'] += flags[b] & (START | END) == START | END and n_out >= 0
            seen['end_alone'] += counts[b] == 0 and flags[b] == END and n_out >= 0
            seen['near_limit'] += n_out >= 0 and pos[b] > 2 ** 59
            if not work and count_ok and b != 5:                       # an idle slot: nothing changes, whatever the delay says
                assert (n_out, new, record) == (0, int(pos[b]), tuple(int(v) for v in rec[b]))
        _, pos, rec, _ = got
    if F == 0:                                                         # a hard switch is whole at once: none is ever refused
        assert seen.pop('refused') == 0
    assert all(seen.values()), seen


def test_spans_mirror_without_a_switch_is_haas_voice_spans():
    from vndecorrelate_amd.streaming import haas_voice_fade_spans, haas_voice_spans
    rng = np.random.default_rng(3)
    S, M, D = 8, 300, 400
    pos, rec = np.zeros(S, np.int64), np.zeros((S, 3), np.int64)
    delays = rng.integers(0, D + 1, S)                                 # a voice keeps its delay: the existing pool's contract
    for _ in range(200):
        counts = rng.integers(-1, M + 2, S)
        flags = rng.choice([0, 0, START, END, START | END], S)
        out, new, rec, left = haas_voice_fade_spans(pos, rec, counts, flags, delays, D, 200, M)
        want_out, want_new = haas_voice_spans(pos, counts, flags, delays, D, M)
        assert out.tolist() == want_out.tolist() and new.tolist() == want_new.tolist()
        assert set(left[out >= 0].tolist()) <= {0} and (left[out < 0] == -1).all()
        pos = new
    with pytest.raises(ValueError, match='records of shape'):
        haas_voice_fade_spans(pos, rec[:, :2], counts, flags, delays, D, 200, M)


def test_tail_is_the_frame_by_frame_count():
    """tail = max(cur, min(old, max(0, s + F - e))) against the count of tail_by_count, over random (F, old, cur, e, s) with
    s <= e - the state's invariant: a fade begins at a position, and positions only grow - and each of the formula's three
    branches met: cur largest, old smaller than s + F - e, s + F - e in between."""
    rng = np.random.default_rng(1)
    met = dict(cur=0, old=0, between=0, through=0)
    for _ in range(4000):
        F = int(rng.choice([0, 1, 50, 200, 700]))
        old, cur = (int(v) for v in rng.integers(0, 401, 2))
        e = int(rng.integers(0, 3000))
        s = e - int(rng.integers(0, F + 300)) if rng.random() < 0.9 else -F
        formula = max(cur, min(old, max(0, s + F - e)))
        assert formula == tail_by_count(F, old, cur, e, s), (F, old, cur, e, s)
        r = s + F - e
        met['through' if r <= 0 else ('cur' if cur >= min(old, r) else ('old' if old <= r else 'between'))] += 1
        if e:                                                          # ... and an END alone at position e returns exactly this tail
            n_out, new, _, left, _ = one_slot(e, (s, old, cur), 0, END, 0, 400, F, 300)
            assert (n_out, new, left) == (formula, 0, 0)
    assert all(met.values()), met


def test_the_ragged_schedule_meets_every_case():
    """The schedule the GPU tier runs, counted on the CPU with the restatement alone: none of the cases is missing."""
    shape = dict(RAGGED['shape'], delays=RAGGED['delays'])
    calls, voices, counted = ragged_schedule(RAGGED['seed'], **shape)
    assert all(counted[case] for case in RAGGED['cases']) and counted['crosses_tile'] == 0, counted
    mono = ragged_schedule(RAGGED['seed'], cx=1, **shape)
    assert mono[2] == counted and [c[1].tolist() for c in mono[0]] == [c[1].tolist() for c in calls]
    assert any(len(vs) > 1 for vs in voices.values())                  # a slot reused
    assert {len(v.fades) for vs in voices.values() for v in vs} >= {0, 1, 2}
    for F in (0, 1, 700):
        _, _, other = ragged_schedule(RAGGED['lengths_seed'], **dict(shape, F=F))
        assert other['accepted'] and other['switch_on_fresh'] and other['longer'] and other['shorter'], (F, other)
        assert F != 700 or all(other[case] for case in RAGGED['long_cases']), other


# ---- the NumPy reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cx', [1, 2])
@pytest.mark.parametrize('ms_mode, width', [(False, None), (True, 0.35)])
@pytest.mark.parametrize('delayed_channel', [0, 1])
def test_reference_without_a_switch_is_the_oracle(cx, ms_mode, width, delayed_channel):
    from oracle import vnd_oracle as O
    x = np.random.default_rng(cx).uniform(-1, 1, (500, cx)).astype(np.float32)
    for d in (0, 1, 150, 499, 500, 700):
        want = O.haas_effect(x[:, 0] if cx == 1 else x, sample_rate_hz=1, delay_time_seconds=float(d),
                             delayed_channel=delayed_channel, mode='MS' if ms_mode else 'LR', width=width)
        got = haas_fade(x, d, [], None, 200, 500 + d, delayed_channel=delayed_channel, ms_mode=ms_mode, width=width)
        assert got.dtype == np.float64 and got.tobytes() == want.tobytes(), d


def test_reference_blend():
    from vndecorrelate_amd.streaming import fade_gains
    x = np.random.default_rng(5).uniform(-1, 1, (1000, 2)).astype(np.float32)
    lr = dict(delayed_channel=1, ms_mode=False, width=None)
    pure = {d: haas_fade(x, d, [], None, 0, 1400, **lr) for d in (0, 150, 400)}
    hard = haas_fade(x, 150, [(300, 150, 400)], fade_gains(0), 0, 1400, **lr)           # F = 0: a hard switch
    assert hard[:300].tobytes() == pure[150][:300].tobytes() and hard[300:].tobytes() == pure[400][300:].tobytes()
    F, g = 200, fade_gains(200, 'equal_power')
    fades = [(100, 150, 0), (450, 0, 0), (900, 0, 400)]                # the last one runs on through the tail
    out = haas_fade(x, 150, fades, g, F, 1400, **lr)
    assert out[:, 0].tobytes() == pure[0][:, 0].tobytes()              # the undelayed channel
    for lo, hi, d in ((0, 100, 150), (300, 450, 0), (650, 900, 0), (1100, 1400, 400)):
        assert out[lo:hi].tobytes() == pure[d][lo:hi].tobytes()        # outside every [s, s + F): one delay's bytes
    for s, old, cur in fades:
        for j in (0, 37, 199):
            want = pure[old][s + j, 1] * np.float64(g[0][j]) + pure[cur][s + j, 1] * np.float64(g[1][j])
            assert out[s + j, 1] == want
    same = out[450:650, 1]                                             # a fade to the delay it has: a * g0 + a * g1
    assert same.tobytes() != pure[0][450:650, 1].tobytes() and np.allclose(same, pure[0][450:650, 1] * (g[0] + g[1]))


# ---- the dict form's refusals, and the dispatch ------------------------------------------------------------------------
@pytest.fixture
def dec():
    import vndecorrelate_amd.decorrelation as decorrelation
    return decorrelation


def _velvets(dec, kappas, **kw):
    return [dec.VelvetNoise(sample_rate_hz=16000, duration_seconds=0.02, num_impulses=15, log_distribution_strength=k,
                            seed=1, normalizer=None, **kw) for k in kappas]


def _haases(dec, delays=(0.0, 0.01, 0.02)):
    return [dec.HaasEffect(sample_rate_hz=16000, delay_time_seconds=d) for d in delays]


def _chains(dec, kappas=(0.0, 0.3, 0.8), delays=(0.0, 0.01, 0.02)):
    return [dec.SignalChain(sample_rate_hz=16000).velvet_noise(duration_seconds=0.02, num_impulses=15, seed=1, normalizer=None,
                                                               log_distribution_strength=k)
            .haas_effect(delay_time_seconds=d) for k, d in zip(kappas, delays)]


@pytest.mark.parametrize('kind', ['haas', 'chain'])
def test_switch_refusals_come_before_the_device(dec, monkeypatch, kind):
    from vndecorrelate_amd import streaming
    bank = _haases(dec) if kind == 'haas' else _chains(dec)
    pool = dec.decorrelate_fade_voice_pool(bank, slots=4, max_frames_per_call=300, fade_frames=200)
    assert type(pool) is (streaming.HaasFadeVoicePool if kind == 'haas' else streaming.ChainFadeVoicePool)
    assert pool.fade_frames == 200 and pool.fade_gains.tobytes() == streaming.fade_gains(200, 'linear').tobytes()
    assert pool.fade_left.tolist() == [0] * 4 and pool.records.shape == (4, 3)
    pools = [pool] + ([pool.haas] if kind == 'chain' else [])

    def reached(*args, **kwargs):
        pytest.fail('a refused call reached the device')
    for p in pools:
        for name in ('_call_host', '_call_device', '_ensure_state'):
            monkeypatch.setattr(p, name, reached)
    block = np.zeros((100, 2), np.float32)
    pool.live[:2] = True                                               # slots 0 and 1 hold live voices, as the mirror has it
    pool.positions[:2] = 1000
    pool.fade_left[1] = 50
    kept = lambda: [a.copy() for p in pools for a in (p.positions, p.records, p.fade_left, p.live, p.tables)]
    before = kept()
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
        for was, now in zip(before, kept()):
            assert now.tolist() == was.tolist()
    with pytest.raises(RuntimeError, match='reset\\(\\) first'):
        pool.fade_left_dev


def test_dispatch_of_decorrelate_fade_voice_pool(dec):
    from vndecorrelate_amd import streaming
    import vndecorrelate_amd
    assert vndecorrelate_amd.decorrelate_fade_voice_pool is dec.decorrelate_fade_voice_pool
    velvets, haases, chains = _velvets(dec, (0.0, 0.3)), _haases(dec), _chains(dec)
    v = dec.decorrelate_fade_voice_pool(velvets, slots=2, fade_frames=64, fade='equal_power')
    same = dec.decorrelate_voice_pool(velvets, slots=2, fade_frames=64, fade='equal_power')
    assert type(v) is type(same) is streaming.FadeVoicePool and v.fade_gains.tobytes() == same.fade_gains.tobytes()
    h = dec.decorrelate_fade_voice_pool(haases, slots=3, in_channels=1, max_frames_per_call=300, fade_frames=64, fade='equal_power')
    assert type(h) is streaming.HaasFadeVoicePool and isinstance(h, streaming.HaasVoicePool)
    assert h.bank_delays.tolist() == [0, 160, 320] and h.row_frames == 620 and h.in_channels == 1
    assert h.fade_gains.tobytes() == streaming.fade_gains(64, 'equal_power').tobytes()
    hard = dec.decorrelate_fade_voice_pool(haases, slots=2, fade_frames=0)
    assert hard.fade_frames == 0 and hard.fade_gains.shape == (2, 0)
    c = dec.decorrelate_fade_voice_pool(chains, slots=2, max_frames_per_call=300, fade_frames=64)
    assert type(c) is streaming.ChainFadeVoicePool and type(c.haas) is streaming.HaasFadeVoicePool
    H = c.latency_frames
    assert c.haas.max_frames_per_call == 300 + H and c.row_frames == 300 + H + 320 and c.haas.fade_frames == 64
    assert c.haas.fade_gains.tobytes() == c.fade_gains.tobytes() and c.bank_delays.tolist() == [0, 160, 320]
    for bank in ([velvets[0], haases[0]], [haases[0], chains[0]], [velvets[0], chains[0]]):    # mixed banks
        with pytest.raises(TypeError, match='takes a bank of'):
            dec.decorrelate_fade_voice_pool(bank, slots=2, fade_frames=64)
    with pytest.raises(ValueError, match='at least one'):
        dec.decorrelate_fade_voice_pool([], slots=2, fade_frames=64)
    for bank in (velvets, haases, chains):
        for frames in (-1, (1 << 20) + 1, 2.5, None):
            with pytest.raises(ValueError, match='fade_frames'):
                dec.decorrelate_fade_voice_pool(bank, slots=2, fade_frames=frames)
        with pytest.raises(ValueError, match='linear'):
            dec.decorrelate_fade_voice_pool(bank, slots=2, fade_frames=8, fade='cosine')
    # decorrelate_voice_pool keeps its pools and its refusal
    assert type(dec.decorrelate_voice_pool(haases, slots=2)) is streaming.HaasVoicePool
    assert type(dec.decorrelate_voice_pool(chains, slots=2)) is streaming.ChainVoicePool
    with pytest.raises(ValueError, match='fade_frames is taken with a bank of plain VelvetNoise'):
        dec.decorrelate_voice_pool(haases, slots=2, fade_frames=64)


def test_the_chain_mirror_is_the_composition(dec):
    """ChainFadeVoicePool._spans: stage 2's rule on stage 1's counts, the caller's flags to both, fade_left the maximum."""
    from vndecorrelate_amd.streaming import haas_voice_fade_spans, voice_fade_spans
    pool = dec.decorrelate_fade_voice_pool(_chains(dec), slots=3, max_frames_per_call=300, fade_frames=200)
    H, D = pool.latency_frames, pool.max_delay
    rng = np.random.default_rng(2)
    p1 = p2 = np.zeros(3, np.int64)
    r1 = r2 = np.zeros((3, 3), np.int64)
    fresh_corner = most_left = 0
    for call in range(60):
        counts = rng.choice([0, 7, 150, 300], 3)
        flags = rng.choice([0, 0, START, END, SWITCH, SWITCH], 3)
        entries = rng.integers(0, 3, 3)
        out, state = pool._spans(counts, flags, entries)
        mid, p1n, r1n, l1 = voice_fade_spans(p1, r1, counts, flags, pool.bank_tables[entries], H, 200, 300)
        want, p2n, r2n, l2 = haas_voice_fade_spans(p2, r2, mid, flags, pool.bank_delays[entries], D, 200, 300 + H)
        assert out.tolist() == want.tolist()
        assert [a.tolist() for a in state] == [a.tolist() for a in (p1n, r1n, p2n, r2n, np.maximum(l1, l2))]
        switched = ((flags & SWITCH) != 0) & ((flags & START) == 0) & (p1 != 0)
        fresh_corner += int((switched & (p2 == 0) & (r1n != r1).any(axis=1)).sum())     # stage 1 fades, stage 2 is fresh
        pool._commit(state)
        most_left = max(most_left, int(pool.fade_left.max()))
        p1, r1, p2, r2 = p1n, r1n, p2n, r2n
    assert fresh_corner and most_left > 0


def test_the_chain_schedule_meets_every_case(dec):
    """The chain schedule the GPU tier runs through the dict form, counted with the two restatements alone."""
    shape = RAGGED['shape']
    chains = _chains(dec, CHAIN['kappas'], [d / 16000 for d in CHAIN['delays']])
    pool = dec.decorrelate_fade_voice_pool(chains, slots=shape['slots'], max_frames_per_call=shape['M'], fade_frames=shape['F'])
    assert pool.bank_delays.tolist() == list(CHAIN['delays']) and pool.max_delay == shape['D'] and pool.latency_frames > shape['F']
    calls, voices, counted = chain_schedule(CHAIN['seed'], H=pool.latency_frames, tables=pool.bank_tables, delays=pool.bank_delays,
                                            **shape)
    assert all(counted[case] for case in CHAIN['cases']), counted
    assert sum(bool(v.fades1 and v.fades2) for v in voices) >= 5 and any(not v.fades1 and not v.fades2 for v in voices)
    assert all(v.pushed == len(v.x) and v.frames == len(v.x) + v.fades2[-1][2] if v.fades2 else True for v in voices)


# ---- marshalling: every wrapper of _native_haas_fade.py against the header's prototype ---------------------------------
HEADER = 'vnd_haas_voice_fade_stream.h'
WRAPPERS = {'haas_voice_fade_stream_state_bytes': 'vnd_haas_voice_fade_stream_state_bytes',
            'haas_voice_fade_stream_reset_device': 'vnd_haas_voice_fade_stream_reset_dev',
            'haas_voice_fade_stream_device': 'vnd_haas_voice_fade_stream_f64_dev'}


def _prototype(function: str):
    """The parameter names of `function` in the header, in order."""
    text = re.sub(r'/\*.*?\*/', ' ', (REPO / 'include' / HEADER).read_text(), flags=re.S)
    match = re.search(r'\b' + function + r'\s*\(([^)]*)\)\s*;', text)
    assert match, function
    return [re.split(r'[\s\*]+', p.strip())[-1] for p in match.group(1).split(',')]


def _python_name(c_name: str) -> str:
    """The wrapper's parameter for a C parameter: addresses are `*_ptr`, the channel count and the stream are short."""
    if c_name in ('in_channels', 'hip_stream'):
        return {'in_channels': 'channels', 'hip_stream': 'stream'}[c_name]
    return c_name[:-4] + '_ptr' if c_name.endswith('_dev') else c_name


def test_every_public_wrapper_is_listed():
    from vndecorrelate_amd import _native, _native_haas_fade
    public = [name for name, f in vars(_native_haas_fade).items()
              if inspect.isfunction(f) and f.__module__ == _native_haas_fade.__name__ and not name.startswith('_')]
    assert sorted(public) == sorted(WRAPPERS)
    assert _native_haas_fade.VOICE_SWITCH == _native.VOICE_SWITCH == SWITCH == 4
    assert _native.HEADERS[HEADER] is _native.HAAS_VOICE_FADE_STREAM_SIGNATURES
    assert sorted(_native.HAAS_VOICE_FADE_STREAM_SIGNATURES) == sorted(WRAPPERS.values())
    text = (REPO / 'include' / HEADER).read_text()
    assert '#include "vnd_voice_fade_stream.h"' in text and '_host' not in re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)


@pytest.mark.parametrize('name', sorted(WRAPPERS))
@pytest.mark.parametrize('width', [None, 0.5])
@pytest.mark.parametrize('flag', [False, True])
def test_wrapper_hands_each_parameter_to_its_place(name, width, flag, monkeypatch):
    from vndecorrelate_amd import _native, _native_haas_fade
    function = WRAPPERS[name]
    c_names = _prototype(function)
    lib = GEN.RecordingLibrary(_native)
    monkeypatch.setattr(_native, '_lib', lib)
    fn = getattr(_native_haas_fade, name)
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
            assert got == expect[_python_name(c_name)], (function, c_name, got)
    numbers = [a for a in args if isinstance(a, (int, float)) and not isinstance(a, bool) and a not in (0, 1)]
    assert len(numbers) == len(set(numbers))                           # the sentinels tell the arguments apart


def test_a_null_gains_and_a_null_fade_left_go_down_as_null():
    from vndecorrelate_amd import _native, _native_haas_fade
    lib = GEN.RecordingLibrary(_native)
    ctx = GEN.Handle(lib, GEN.CTX_HANDLE)
    _native_haas_fade.haas_voice_fade_stream_device(ctx, 16, 32, 48, 0, None, 64, 80, 96, 112, 128, 144, None, 6, 2,
                                                    max_delay=400, delayed_channel=1, ms_mode=False, width=None, stream=7)
    (_, args), = lib.calls
    names = _prototype('vnd_haas_voice_fade_stream_f64_dev')
    assert args[names.index('gains_dev')] == 0 and args[names.index('fade_left_dev')] == 0
    assert args[names.index('max_delay')] == 400 and args[names.index('delayed_channel')] == 1
    assert args[names.index('hip_stream')] == 7
