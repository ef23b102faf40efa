"""GPU tier of the chain voice pool (streaming.ChainVoicePool, decorrelate_voice_pool on a bank of SignalChains): a voice
goes through its velvet-noise filter (vnd_voice_stream_f32_dev) and then its Haas delay (vnd_haas_voice_stream_f64_dev,
whose counts are stage 1's out_counts in device memory) entirely on the device.  Every comparison is bit for bit.

The bank: four chains of a 15-tap velvet filter (16 kHz, 0.02 s: H <= 319) at four kappa values and the delays {0, 100,
441, 882}; the reference's example settings - velvet MS, Haas LR on channel 1 - and a second set, velvet LR + width 0.4,
Haas MS on channel 0 + width 0.6.  S = 6, M = 600.  A voice's concatenated outputs equal the oracle's
haas_effect(decorrelate(x, normalize=False)) on its whole signal, and the package's one-shot chain(x)."""
import numpy as np
import pytest

from oracle import vnd_oracle as O
from test_gpu_each_stream import _noise
from test_gpu_voice_pool import Voice

pytestmark = pytest.mark.gpu

S, M = 6, 600
FS, DURATION, IMPULSES, SEED = 16000, 0.02, 15, 1
KAPPAS = (0.0, 0.3, 0.55, 1.0)
DELAYS = (0, 100, 441, 882)
START, END = 1, 2
POISON = 0x7FF4A5A5A5A5A5A5                  # a signalling NaN: no kernel arithmetic yields it
SETTINGS = {'ms>lr-ch1': (dict(mode='MS', width=None), dict(delayed_channel=1, mode='LR', width=None)),
            'lr-width>ms-ch0-width': (dict(mode='LR', width=0.4), dict(delayed_channel=0, mode='MS', width=0.6))}


@pytest.fixture(scope='module')
def ctx():
    from vndecorrelate_amd import _native
    context = _native.default_context()
    assert 'gfx950' in context.info()['name']
    return context


@pytest.fixture
def dec(ctx):
    import vndecorrelate_amd.decorrelation as decorrelation
    return decorrelation


def _bank(dec, name, kappas=KAPPAS, delays=DELAYS):
    velvet, haas = SETTINGS[name]
    return [dec.SignalChain(sample_rate_hz=FS)
            .velvet_noise(duration_seconds=DURATION, num_impulses=IMPULSES, seed=SEED, normalizer=None,
                          log_distribution_strength=k, **velvet)
            .haas_effect(delay_time_seconds=d / FS, **haas) for k, d in zip(kappas, delays)]


def _oracle(x, entry, cx, name):
    velvet, haas = SETTINGS[name]
    mid = O.decorrelate(x[:, 0] if cx == 1 else x, sample_rate_hz=FS, duration_seconds=DURATION, num_impulses=IMPULSES,
                        log_distribution_strength=KAPPAS[entry], seed=SEED, normalize=False, **velvet)
    assert mid.shape == (len(x), 2)
    return O.haas_effect(mid, sample_rate_hz=FS, delay_time_seconds=DELAYS[entry] / FS, **haas)


def _same(got, want, where):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64, (where, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.int64) != want.view(np.int64))
        raise AssertionError((where, 'first (frame, channel)', tuple(bad[0]), len(bad), float(got[tuple(bad[0])]),
                              float(want[tuple(bad[0])])))


def _cat(rows):
    rows = [r for r in rows if len(r)]
    return np.concatenate(rows) if rows else np.zeros((0, 2), np.float64)


def _ragged_plan(cx, seed):
    """test_gpu_haas_voice_pool.py's schedule with bank entries for delays: voices of 1, 200 (both shorter than H), 255,
    257, 1300 and 2049 frames that start on different calls; slots 0 - 3 are reused after END by a voice of another entry;
    slot 5's first voice is discarded by a START without END; slot 0's first voice is one frame, START + END in one call."""
    sig = lambda n, k: _noise((n, cx), seed + k)
    return {0: [Voice(sig(1, 0), 3, 0, whole=True), Voice(sig(700, 1), 1, 4, end_with_last=False)],
            1: [Voice(sig(200, 2), 2, 1, end_with_last=False), Voice(sig(300, 8), 0, 0)],
            2: [Voice(sig(255, 3), 1, 0), Voice(sig(400, 9), 2, 3)],
            3: [Voice(sig(257, 4), 0, 2, end_with_last=False), Voice(sig(350, 10), 3, 0)],
            4: [Voice(sig(1300, 5), 2, 3, end_with_last=False)],
            5: [Voice(sig(900, 6), 1, 1, discard_after=450), Voice(sig(2049, 7), 3, 0)]}


def _drive_dict(pool, plan, rng):
    """The voices of `plan` ({slot: [Voice, ...]}, Voice.table = the bank entry) through the dict form on counts drawn from
    [0, M], zeros included.  A voice with discard_after is never ended: the next voice of its slot starts over it."""
    queue = {slot: list(voices) for slot, voices in plan.items()}
    active = {slot: None for slot in range(pool.slots)}
    call = 0
    while any(queue.values()) or any(v is not None for v in active.values()):
        assert call < 200
        blocks, start, end, discard = {}, {}, [], False
        for slot in range(pool.slots):
            v, force = active[slot], False
            if v is not None and v.discard_after is not None and v.pushed >= v.discard_after:
                v, active[slot], force = None, None, True
            if v is None and queue.get(slot) and (force or queue[slot][0].start_call <= call):
                v = active[slot] = queue[slot].pop(0)
                start[slot] = v.table
                discard = discard or force
            if v is None:
                continue
            limit = (len(v.x) if v.discard_after is None else v.discard_after) - v.pushed
            n = limit if v.whole else min(limit, 0 if rng.random() < 0.3 else int(rng.integers(1, M + 1)))
            blocks[slot] = v.x[v.pushed:v.pushed + n]
            v.pushed += n
            if v.discard_after is None and v.pushed == len(v.x):
                if v.end_with_last or v.done:
                    end.append(slot)
                v.done = True
        out = pool.process(blocks, start=start, end=end, discard=discard)
        assert sorted(out) == sorted(set(blocks) | set(end)), call
        for slot, rows in out.items():
            assert rows.dtype == np.float64 and rows.ndim == 2 and rows.shape[1] == 2
            active[slot].out.append(rows)
        for slot in end:
            active[slot] = None
        call += 1
    return call


# ---- 1. a ragged schedule through the dict form -----------------------------------------------------------------------
@pytest.mark.parametrize('cx', [2, 1], ids=['stereo', 'mono'])
@pytest.mark.parametrize('name', list(SETTINGS))
def test_ragged_schedule(dec, name, cx):
    bank = _bank(dec, name)
    pool = dec.decorrelate_voice_pool(bank, slots=S, in_channels=cx, max_frames_per_call=M)
    H = pool.latency_frames
    assert 200 < H <= 319 and pool.bank_delays.tolist() == list(DELAYS) and pool.row_frames == M + H + 882
    assert len(set(pool.bank_tables.tolist())) == 4
    plan = _ragged_plan(cx, 100 * cx)
    calls = _drive_dict(pool, plan, np.random.default_rng(7 + cx))
    assert calls > 8
    for slot, voices in plan.items():
        for i, v in enumerate(voices):
            want = _oracle(v.x, v.table, cx, name)
            got = _cat(v.out)
            where = (name, 'slot', slot, 'voice', i, 'entry', v.table)
            if v.discard_after is None:
                _same(got, want, where)
                _same(bank[v.table](v.x[:, 0] if cx == 1 else v.x), want, where + ('the one-shot chain',))
            else:                                       # what it returned before it was dropped is final all the same
                assert len(got) == max(0, v.discard_after - H)
                _same(got, want[:len(got)], where)
    assert not pool.positions.any() and not pool.haas_positions.any() and not pool.live.any()
    with pytest.raises(RuntimeError, match='runs through process\\(\\)'):
        pool.process_dev(None, None, None, None, None)


# ---- 2. lockstep ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cx', [2, 1], ids=['stereo', 'mono'])
def test_lockstep_equals_the_chain_stream_call_by_call(dec, cx):
    """A bank of one chain: the pool's latency is its bank's largest tap index, and the lockstep stream's its own chain's."""
    name, entry = 'ms>lr-ch1', 2
    pool = dec.decorrelate_voice_pool([_bank(dec, name)[entry]], slots=S, in_channels=cx, max_frames_per_call=M)
    lock = _bank(dec, name)[entry].stream(num_streams=S, in_channels=cx, max_frames_per_call=M)
    assert (lock.latency_frames, lock.tail_frames) == (pool.latency_frames, DELAYS[entry])
    sizes = [600, 0, 37, 263, 600, 1]
    x = _noise((S, sum(sizes), cx), 11 + cx)
    pos = 0
    for i, n in enumerate(sizes):
        block = x[:, pos:pos + n]
        want = lock.process(block)
        out = pool.process({b: block[b] for b in range(S)}, start={b: 0 for b in range(S)} if i == 0 else None)
        for b in range(S):
            assert out[b].tobytes() == want[b].tobytes() and out[b].shape == want[b].shape, (i, b)
        if i == 0:                                                             # one upload and one download for both stages
            assert pool.transfers == {'to_device': 1, 'to_host': 1}
        pos += n
    want = lock.flush()
    out = pool.process({}, end=list(range(S)))
    assert want.shape == (S, pool.latency_frames + DELAYS[entry], 2)
    for b in range(S):
        assert out[b].tobytes() == want[b].tobytes() and out[b].shape == want[b].shape, ('flush', b)


# ---- 3. the device form: a bad count, and graph replay ----------------------------------------------------------------
def _device_schedule(cx, seed):
    """8 calls of (blocks, counts, flags) over 6 slots as process_dev arrays, with a START and an END inside, a reused slot
    and idle calls; the bank entry is fixed per slot."""
    rng = np.random.default_rng(seed)
    calls = []
    for i in range(8):
        counts = rng.integers(0, M + 1, S).astype(np.int32)
        counts[rng.random(S) < 0.3] = 0
        flags = np.zeros(S, np.int32)
        if i == 0:
            flags[:4] = START
        if i == 2:
            flags[4] = START
            flags[1] = END
        if i == 3:
            flags[5] = START | END
        if i == 4:
            flags[1] = START
            flags[0] = END
            counts[0] = 0
        if i == 7:
            flags[:] |= END
        calls.append((rng.uniform(-1, 1, (S, M, cx)).astype(np.float32), counts, flags))
    return calls


ENTRIES = np.array([3, 0, 2, 1, 3, 2])


class DevicePool:
    """A chain pool run through process_dev on poisoned outputs, the uploads of one call at a time."""

    def __init__(self, dec, ctx, cx, replayed=False):
        import torch
        self.torch, self.dev = torch, torch.device('cuda', ctx.device)
        self.pool = pool = dec.decorrelate_voice_pool(_bank(dec, 'ms>lr-ch1'), slots=S, in_channels=cx, max_frames_per_call=M)
        dev = self.dev
        self.tables = torch.from_numpy(pool.bank_tables[ENTRIES].astype(np.int32)).to(dev)
        self.delays = torch.from_numpy(pool.bank_delays[ENTRIES].astype(np.int32)).to(dev)
        self.x = torch.empty((S, M, cx), dtype=torch.float32, device=dev)
        self.counts, self.flags, self.oc = (torch.empty(S, dtype=torch.int32, device=dev) for _ in range(3))
        self.y = torch.empty((S, pool.row_frames, 2), dtype=torch.int64, device=dev)
        self.out = (self.y.view(torch.float64), self.oc)
        pool.reset()                                  # allocates both states and the intermediate buffers: before a capture
        assert pool._mid is not None and tuple(pool._mid[0].shape) == (S, M + pool.latency_frames, 2)
        self.graph = None
        if replayed:
            self.graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
            with torch.cuda.graph(self.graph, stream=side):
                pool.process_dev(self.x, self.counts, self.flags, self.tables, self.delays, out=self.out)
            torch.cuda.synchronize(dev)

    def call(self, xh, counts, flags):
        torch = self.torch
        self.x.copy_(torch.from_numpy(xh))
        self.counts.copy_(torch.from_numpy(counts))
        self.flags.copy_(torch.from_numpy(flags))
        self.y.fill_(POISON)
        if self.graph is not None:
            self.graph.replay()
        else:
            self.pool.process_dev(self.x, self.counts, self.flags, self.tables, self.delays, out=self.out)
        torch.cuda.synchronize(self.dev)
        return self.y.cpu().numpy(), self.oc.cpu().numpy(), self.pool._mid[1].cpu().numpy()

    def positions(self):
        """(stage 1's, stage 2's): the first int64 words of the two states."""
        torch = self.torch
        return tuple(state[0][:S * 8].view(torch.int64).cpu().numpy().copy() for state in (self.pool._state, self.pool.haas._state))


def _chain_spans(pool, calls):
    """The mirror of every call of a device schedule: (stage 1's out_counts, stage 2's) per call."""
    from vndecorrelate_amd.streaming import haas_voice_spans, voice_spans
    p1, p2, spans = np.zeros(S, np.int64), np.zeros(S, np.int64), []
    for _, counts, flags in calls:
        mid, p1 = voice_spans(p1, counts, flags, pool.latency_frames, M)
        out, p2 = haas_voice_spans(p2, mid, flags, pool.bank_delays[ENTRIES], pool.tail_frames, M + pool.latency_frames)
        spans.append((mid, out))
    return spans


def test_graph_replay_equals_the_uncaptured_run(dec, ctx):
    cx = 2
    calls = _device_schedule(cx, 3)
    plain_pool = DevicePool(dec, ctx, cx)
    plain = [plain_pool.call(*c) for c in calls]                               # first: it loads the kernels
    with pytest.raises(RuntimeError, match='runs through process_dev'):
        plain_pool.pool.process({})
    replay_pool = DevicePool(dec, ctx, cx, replayed=True)
    replay = [replay_pool.call(*c) for c in calls]
    for i, ((y0, c0, m0), (y1, c1, m1), (mid, want)) in enumerate(zip(plain, replay, _chain_spans(plain_pool.pool, calls))):
        assert m0.tolist() == mid.tolist() == m1.tolist(), i
        assert c0.tolist() == want.tolist() == c1.tolist(), i
        assert y0.tobytes() == y1.tobytes(), i                                 # outputs and untouched frames alike
        for b, n in enumerate(want):
            assert not (y0[b, :n] == POISON).any() and (y0[b, n:] == POISON).all(), (i, b)
    assert any(0 < n for _, c, _ in plain for n in c)
    assert not any(p.any() for p in replay_pool.positions())                   # every voice ended


@pytest.mark.parametrize('bad_count', [M + 1, -1])
def test_a_bad_count_answers_minus_one_from_both_stages(dec, ctx, bad_count):
    cx = 2
    calls = _device_schedule(cx, 5)
    calls[0][1][2], calls[1][1][2] = 500, 300                                  # slot 2 is live and has a block on call 1
    clean_pool = DevicePool(dec, ctx, cx)
    clean = [clean_pool.call(*c) for c in calls]
    spoiled_pool = DevicePool(dec, ctx, cx)
    for i, (xh, counts, flags) in enumerate(calls):
        if i == 1:                                                             # slot 2, live since call 0, sends a bad count
            bad = counts.copy()
            bad[2] = bad_count
            before = spoiled_pool.positions()
            y, oc, mid = spoiled_pool.call(xh, bad, flags)
            assert mid[2] == -1 and oc[2] == -1 and (y[2] == POISON).all()
            after = spoiled_pool.positions()
            assert after[0][2] == before[0][2] > 0 and after[1][2] == before[1][2]
            for b in (0, 1, 3, 4, 5):
                assert oc[b] == clean[i][1][b] and y[b].tobytes() == clean[i][0][b].tobytes(), (i, b)
            only = np.zeros(S, np.int32)                                       # the voice goes on: the block it meant to push
            only[2] = counts[2]
            y, oc, mid = spoiled_pool.call(xh, only, np.zeros(S, np.int32))
            assert oc[2] == clean[i][1][2] and y[2].tobytes() == clean[i][0][2].tobytes()
        else:
            y, oc, mid = spoiled_pool.call(xh, counts, flags)
            assert oc.tolist() == clean[i][1].tolist() and y.tobytes() == clean[i][0].tobytes(), i
