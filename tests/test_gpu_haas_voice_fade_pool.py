"""GPU tier of the crossfading Haas and chain voice pools (vnd_haas_voice_fade_stream_f64_dev,
include/vnd_haas_voice_fade_stream.h; streaming.HaasFadeVoicePool, ChainFadeVoicePool): Haas voices that change their delay,
and chains that change filter and delay together.  Every comparison is of bytes.

The C ABI runs through the poisoned harness of test_gpu_haas_voice_pool.py with the pool's own state layout - positions,
records, ring, all NaN bits before the reset, which zeroes the positions alone - and a fifth output, fade_left, behind a
sentinel tail of its own.  After every call out_counts, fade_left, the positions and the records on the device equal
streaming.haas_voice_fade_spans', every frame below out_counts[b] was written and none at or past it.  S = 6, M = 300,
max_delay = 400: a row of 700 frames spans three 256-lane tiles.

The reference is haas_voice_fade_cases.haas_fade: NumPy float64 on the oracle's own steps, the blend between the shift and
the decode, from the switches the header's block - restated in Python integers there - accepts.  Without a switch it is
oracle.haas_effect bit for bit (tests/test_haas_voice_fade_pool_cpu.py, and test 1 here)."""
import ctypes

import numpy as np
import pytest

from haas_voice_fade_cases import (CHAIN, END, RAGGED, START, SWITCH, ChainVoice, chain_schedule, haas_fade,
                                   ragged_schedule)
from test_gpu_each_stream import _noise
from test_gpu_haas_voice_pool import (INVALID, NAN_BITS, POISON, SENTINEL, SENTINEL32, TAIL, UNSUPPORTED, Harness, _cat,
                                      _check_voices, _reference, _same, ctx, dec)  # noqa: F401  (fixtures)
from test_gpu_voice_pool import Voice, _drive

pytestmark = pytest.mark.gpu

S, M, D, F = (RAGGED['shape'][k] for k in ('slots', 'M', 'D', 'F'))
DELAYS = RAGGED['delays']
LR1 = dict(delayed_channel=1, ms_mode=False, width=None)
MS0 = dict(delayed_channel=0, ms_mode=True, width=0.35)
MS1 = dict(delayed_channel=1, ms_mode=True, width=0.35)


def _gains(frames, fade='linear'):
    from vndecorrelate_amd.streaming import fade_gains
    return fade_gains(frames, fade)


class FadeHarness(Harness):
    """test_gpu_haas_voice_pool.Harness on vnd_haas_voice_fade_stream_f64_dev: the records between positions and ring, the
    gains, fade_left, and the mirror of all of it."""

    def __init__(self, ctx, cx, settings, fade_frames, gains=None, max_delay=D, slots=S, max_frames=M):
        import torch
        from vndecorrelate_amd import _native, _native_haas_fade
        self.torch, self.ctx, self.lib, self.native = torch, ctx, ctx._lib, _native
        self.S, self.M, self.D, self.cx, self.settings, self.F = slots, max_frames, max_delay, cx, settings, fade_frames
        self.dev = torch.device('cuda', ctx.device)
        self.pos_bytes = (slots * 8 + 15) & ~15
        self.rec_bytes = 16 * slots
        self.state_bytes = _native_haas_fade.haas_voice_fade_stream_state_bytes(slots, cx, max_delay, max_frames, fade_frames)
        assert self.state_bytes == self.pos_bytes + self.rec_bytes + slots * (max_delay + max_frames) * cx * 4
        self.state = torch.full((self.state_bytes // 4,), float('nan'), dtype=torch.float32, device=self.dev)
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream
        _native_haas_fade.haas_voice_fade_stream_reset_device(ctx, self.state.data_ptr(), self.state_bytes, slots, cx, max_delay,
                                                              max_frames, fade_frames, stream=self.stream)
        words = self.state_words()
        assert not words[:self.pos_bytes // 4].any(), 'the reset leaves positions that are not 0'
        assert (words[self.pos_bytes // 4:] == NAN_BITS).all(), 'the reset cleared the records or the ring'
        self.gains_host = _gains(fade_frames) if gains is None else gains
        self.gains = torch.from_numpy(self.gains_host).to(self.dev) if fade_frames else None
        self.rows = max_frames + max_delay
        self.body = slots * self.rows * 2
        self.x = torch.empty((slots, max_frames, cx), dtype=torch.float32, device=self.dev)
        self.y = torch.empty((self.body + TAIL,), dtype=torch.int64, device=self.dev)
        self.ints = torch.empty((3, slots), dtype=torch.int32, device=self.dev)           # counts, flags, delays
        self.out_counts = torch.empty((slots + 8,), dtype=torch.int32, device=self.dev)
        self.fade_left = torch.empty((slots + 8,), dtype=torch.int32, device=self.dev)
        self.mirror = np.zeros(slots, np.int64)
        self.mirror_records = self.records()
        self.mirror_left = np.zeros(slots, np.int64)

    def _record_words(self):
        return self.state[self.pos_bytes // 4:(self.pos_bytes + self.rec_bytes) // 4].view(self.torch.int32).view(self.S, 4)

    def records(self):
        """The records on the device as int64 (S, 3): s, old, cur."""
        words = self._record_words().cpu().numpy()
        s = words[:, :2].copy().view(np.int64)[:, 0]
        return np.stack([s, words[:, 2].astype(np.int64), words[:, 3].astype(np.int64)], axis=1)

    def ring(self):
        return self.state_words()[(self.pos_bytes + self.rec_bytes) // 4:].reshape(self.S, self.D + self.M, self.cx)

    def plant(self, slot, position, history, record):
        """Harness.plant, by this pool's layout, with the slot's record (s, old, cur)."""
        torch, D_, cap = self.torch, self.D, self.D + self.M
        assert history.shape == (D_, self.cx) and history.dtype == np.float32
        ring = self.state[(self.pos_bytes + self.rec_bytes) // 4:].view(self.S, cap, self.cx)
        where = np.array([(position - D_ + j) % cap for j in range(D_)], np.int64)      # Python integers: no wrap
        ring[slot, torch.from_numpy(where).to(self.dev)] = torch.from_numpy(history).to(self.dev)
        rec = self._record_words()
        rec[slot, :2] = torch.from_numpy(np.array([record[0]], np.int64).view(np.int32)).to(self.dev)
        rec[slot, 2], rec[slot, 3] = int(record[1]), int(record[2])
        self.set_position(slot, position)
        self.mirror_records[slot] = record
        assert self.records()[slot].tolist() == list(record)

    def raw(self, blocks, counts, flags, delays, override=None):
        """One call on poisoned buffers: (status, out_counts, y as int64 (S, M + max_delay, 2), fade_left)."""
        torch = self.torch
        xh = np.full((self.S, self.M, self.cx), np.nan, np.float32)                       # NaN past counts[b]: never read
        for slot, block in blocks.items():
            xh[slot, :len(block)] = block
        self.x.copy_(torch.from_numpy(xh))
        self.ints.copy_(torch.from_numpy(np.stack([counts, flags, delays]).astype(np.int32)))
        self.y[:self.body] = POISON
        self.y[self.body:] = SENTINEL
        self.out_counts[:] = SENTINEL32
        self.fade_left[:] = SENTINEL32
        a = dict(ctx=self.ctx.handle, state=self.state.data_ptr(), state_bytes=self.state_bytes, M=self.M, F=self.F,
                 gains=self.gains.data_ptr() if self.F else 0, x=self.x.data_ptr(), counts=self.ints[0].data_ptr(),
                 flags=self.ints[1].data_ptr(), delays=self.ints[2].data_ptr(), y=self.y.data_ptr(),
                 out_counts=self.out_counts.data_ptr(), fade_left=self.fade_left.data_ptr(), slots=self.S, cx=self.cx,
                 max_delay=self.D, delayed_channel=self.settings['delayed_channel'])
        a.update(override or {})
        width, p = self.settings['width'], ctypes.c_void_p
        rc = self.lib.vnd_haas_voice_fade_stream_f64_dev(
            a['ctx'], p(a['state']), a['state_bytes'], a['M'], a['F'], p(a['gains']), p(a['x']), p(a['counts']), p(a['flags']),
            p(a['delays']), p(a['y']), p(a['out_counts']), p(a['fade_left']), a['slots'], a['cx'], a['max_delay'],
            a['delayed_channel'], int(self.settings['ms_mode']), int(width is not None), float(width or 0.0), p(self.stream))
        yh, oc, fl = self.y.cpu().numpy(), self.out_counts.cpu().numpy(), self.fade_left.cpu().numpy()
        assert (yh[self.body:] == SENTINEL).all(), 'the call wrote behind the last row'
        assert (oc[self.S:] == SENTINEL32).all() and (fl[self.S:] == SENTINEL32).all(), 'the call wrote behind its int32 outputs'
        return rc, oc[:self.S].copy(), yh[:self.body].reshape(self.S, self.rows, 2), fl[:self.S].copy()

    def call(self, blocks, counts, flags, delays, where=''):
        """A call that must succeed, held to haas_voice_fade_spans and to its footprint: the rows as float64, one per slot."""
        from vndecorrelate_amd.streaming import haas_voice_fade_spans
        rc, oc, yh, fl = self.raw(blocks, counts, flags, delays)
        assert rc == 0, self.lib.vnd_last_error()
        want, self.mirror, self.mirror_records, self.mirror_left = haas_voice_fade_spans(
            self.mirror, self.mirror_records, counts, flags, delays, self.D, self.F, self.M)
        assert oc.tolist() == want.tolist(), (where, counts, flags, delays)
        assert fl.tolist() == self.mirror_left.tolist(), (where, 'fade_left', counts, flags)
        assert self.positions().tolist() == self.mirror.tolist(), f'{where}: the positions on the device are not the mirror\'s'
        assert self.records().tolist() == self.mirror_records.tolist(), f'{where}: the records on the device are not the mirror\'s'
        rows = []
        for b, n in enumerate(np.maximum(want, 0)):
            hole = np.argwhere(yh[b, :n] == POISON)
            assert not len(hole), f'{where}: slot {b} left (frame, channel) {tuple(hole[0])} of its {n} frames unwritten'
            assert (yh[b, n:] == POISON).all(), f'{where}: slot {b} wrote at or past its {n} frames'
            rows.append(yh[b, :n].view(np.float64).copy())
        return rows


def _replay(h, calls):
    """Run `calls` ((blocks, counts, flags, delays), ...) and hand every slot's rows to the voice they belong to: returns
    {slot: [float64 (n, 2), ...]} per voice that began with a START, in order."""
    outs = {b: [] for b in range(h.S)}
    for i, (blocks, counts, flags, delays) in enumerate(calls):
        rows = h.call(blocks, counts, flags, delays, f'call {i}')
        for b in range(h.S):
            if flags[b] & START:
                outs[b].append([])
            if outs[b] and len(rows[b]):
                outs[b][-1].append(rows[b])
    return {b: [_cat(o) for o in per] for b, per in outs.items()}


def _check_schedule(h, calls, voices, settings):
    """Every voice of a haas_voice_fade_cases.ragged_schedule against the reference; returns the blended samples that are
    neither pure delay's bytes."""
    got = _replay(h, calls)
    mixed = 0
    for b, per in voices.items():
        assert len(per) == len(got[b])
        for i, v in enumerate(per):
            x = v.x[:v.pushed]                                         # (a voice that was started over: what it had pushed)
            assert v.dropped or v.pushed == len(v.x)
            want = haas_fade(x, v.delay, v.fades, h.gains_host, h.F, v.frames, **settings)
            _same(got[b][i], want, ('slot', b, 'voice', i, 'delay', v.delay, 'fades', v.fades))
            for s, old, cur in v.fades:
                k = min(h.F, v.frames - s)
                pure = [haas_fade(x, d, [], None, 0, v.frames, **settings)[s:s + k].view(np.int64) for d in (old, cur)]
                mine = want[s:s + k].view(np.int64)
                mixed += int(((mine != pure[0]) & (mine != pure[1])).sum())
    return mixed


# ---- 1. no switch: the existing pool's bytes --------------------------------------------------------------------------
def _plain_plan(cx, seed):
    """Voices of 1 to 1300 frames over every delay of the bank, slots reused, one voice discarded by a START."""
    sig = lambda n, k: _noise((n, cx), seed + k)
    return {0: [Voice(sig(1, 0), 400, 0, whole=True), Voice(sig(700, 1), 7, 4, end_with_last=False)],
            1: [Voice(sig(200, 2), 399, 1, end_with_last=False), Voice(sig(300, 8), 0, 0)],
            2: [Voice(sig(255, 3), 150, 0), Voice(sig(400, 9), 400, 3)],
            3: [Voice(sig(257, 4), 1, 2, end_with_last=False)],
            4: [Voice(sig(1300, 5), 150, 3, end_with_last=False)],
            5: [Voice(sig(900, 6), 399, 1, discard_after=450), Voice(sig(1025, 7), 400, 0)]}


@pytest.mark.parametrize('delayed_channel', [0, 1])
@pytest.mark.parametrize('ms_mode, width', [(False, None), (True, 0.35)], ids=['lr', 'ms-width'])
@pytest.mark.parametrize('cx', [1, 2])
def test_without_a_switch_it_is_the_haas_voice_pool(ctx, cx, ms_mode, width, delayed_channel):
    settings = dict(delayed_channel=delayed_channel, ms_mode=ms_mode, width=width)
    plan = _plain_plan(cx, 100 * cx)
    plain, log = Harness(ctx, cx, settings, max_delay=D, slots=S, max_frames=M), []
    inner = plain.call

    def recorded(blocks, counts, flags, delays, where=''):
        rows = inner(blocks, counts, flags, delays, where)
        log.append((dict(blocks), counts.copy(), flags.copy(), delays.copy(), rows))
        return rows
    plain.call = recorded
    assert _drive(plain, plan, np.random.default_rng(7 + cx)) > 8
    _check_voices(plan, cx, settings)                                  # the existing pool is the oracle's haas_effect ...
    for voices in plan.values():                                       # ... and so is the NumPy reference of the tests below
        for v in voices:
            if v.discard_after is None:
                want = _reference(v.x, v.table, cx, settings)
                assert haas_fade(v.x, v.table, [], None, F, len(want), **settings).tobytes() == want.tobytes()
    h = FadeHarness(ctx, cx, settings, F)
    for i, (blocks, counts, flags, delays, want) in enumerate(log):
        rows = h.call(blocks, counts, flags, delays, f'call {i}')      # out_counts = haas_voice_spans', as the plain call's were
        assert not h.mirror_left.any()
        for b in range(S):
            assert rows[b].tobytes() == want[b].tobytes(), (i, b)
    assert not h.positions().any()


# ---- 2. a ragged schedule with switches -------------------------------------------------------------------------------
@pytest.mark.parametrize('cx, settings', [(2, LR1), (2, MS0), (1, MS1)], ids=['lr-ch1', 'ms-width-ch0', 'mono-ms-width-ch1'])
def test_ragged_schedule_with_switches(ctx, cx, settings):
    calls, voices, counted = ragged_schedule(RAGGED['seed'], cx=cx, delays=DELAYS, **RAGGED['shape'])
    assert all(counted[case] for case in RAGGED['cases']), counted
    h = FadeHarness(ctx, cx, settings, F)
    mixed = _check_schedule(h, calls, voices, settings)
    assert mixed > 0, 'no blended sample differs from both pure delays'
    assert not h.positions().any()


# ---- 3. F = 0, 1 and a fade longer than a row -------------------------------------------------------------------------
@pytest.mark.parametrize('frames', [0, 1, 700])
def test_fade_lengths(ctx, frames):
    cx, settings = 2, MS1
    calls, voices, counted = ragged_schedule(RAGGED['lengths_seed'], delays=DELAYS, **dict(RAGGED['shape'], F=frames))
    assert counted['accepted'] and counted['switch_on_fresh']
    if frames == 700:                  # a fade crosses a 256-lane tile of a row and comes back over several calls
        assert all(counted[case] for case in RAGGED['long_cases']), counted
    h = FadeHarness(ctx, cx, settings, frames, _gains(frames, 'equal_power'))
    mixed = _check_schedule(h, calls, voices, settings)
    assert (mixed > 0) == (frames > 0)


# ---- 4. positions a long-lived voice reaches --------------------------------------------------------------------------
@pytest.mark.parametrize('cx', [2, 1])
def test_planted_positions_with_a_switch_in_the_first_call(ctx, cx):
    """No START: the slots go on from the position, history and record planted in their state, and switch at once.  The fade
    of the slot at 2^32 - 300 begins there and is 700 frames long: it straddles 2^32."""
    settings, frames = MS1, 700
    planted = {0: (2 ** 32 - 300, 150, 400), 3: (2 ** 53 + 1, 400, 7)}                  # position, delay before, delay after
    h = FadeHarness(ctx, cx, settings, frames)
    sigs = {b: _noise((D + 1400, cx), 900 + b + cx) for b in planted}
    for b, (P, old, _) in planted.items():
        h.plant(b, P, sigs[b][:D], (-frames, old, old))                # its delay since its start, never switched
    assert planted[0][0] < 2 ** 32 < planted[0][0] + frames
    outs, done = {b: [] for b in planted}, 0
    for i, n in enumerate((300, 0, 7, 299, 300, 300, 194)):
        counts, flags, delays = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32)
        for b, (P, old, cur) in planted.items():
            counts[b] = n
            flags[b] = (SWITCH if i in (0, 1) else 0) | (END if done + n == 1400 else 0)
            delays[b] = cur if i == 0 else D + 9                       # the switch of call 1 comes inside the fade: not read
        rows = h.call({b: sigs[b][D + done:D + done + n] for b in planted}, counts, flags, delays, f'call {i}')
        if i == 0:
            assert h.mirror_left[0] == frames - 300 and h.records()[0].tolist() == [planted[0][0], 150, 400]
        for b in planted:
            outs[b].append(rows[b])
        done += n
    assert done == 1400 and not h.positions().any()
    for b, (P, old, cur) in planted.items():
        got = _cat(outs[b])
        assert len(got) == 1400 + cur                                  # the fade was through: the new delay's tail
        want = haas_fade(sigs[b], old, [(D, old, cur)], h.gains_host, frames, D + len(got), **settings)[D:]
        _same(got, want, ('planted at', P))


# ---- 5. a bad delay ---------------------------------------------------------------------------------------------------
START_DELAYS = np.array([7, 400, 150, 399, 0, 1], np.int32)
NEXT_DELAYS = np.array([400, 0, 399, 150, 1, 7], np.int32)


@pytest.mark.parametrize('bad', [D + 1, -1, 2 ** 31 - 1, -2 ** 31])
def test_a_switch_to_a_bad_delay_leaves_the_slot_alone(ctx, bad):
    """Call 1 switches every slot; slot 2's delay is outside [0, max_delay]: -1 twice, its row, position, record and ring
    untouched, the neighbours' bytes as if nothing had happened; it then makes the call it meant to make.  Call 2 carries
    the same bad value on switches that are refused, slot 2's among them: it is not read."""
    cx, settings = 2, MS1
    x = _noise((S, 700, cx), 61)
    h = FadeHarness(ctx, cx, settings, F)
    outs = [[] for _ in range(S)]
    full = lambda n, flag: (np.full(S, n, np.int32), np.full(S, flag, np.int32))
    rows = h.call({b: x[b, :250] for b in range(S)}, *full(250, START), START_DELAYS, 'call 0')
    blocks = {b: x[b, 250:400] for b in range(S)}
    counts, flags = full(150, SWITCH)
    delays = NEXT_DELAYS.copy()
    delays[2] = bad
    before, state, records = h.positions(), h.state_words().copy(), h.records()
    rc, oc, yh, fl = h.raw(blocks, counts, flags, delays)
    assert rc == 0, h.lib.vnd_last_error()
    assert oc[2] == -1 and fl[2] == -1 and (yh[2] == POISON).all()
    assert h.positions()[2] == before[2] == 250 and h.records()[2].tolist() == records[2].tolist() == [-F, 150, 150]
    ring = lambda w: w[(h.pos_bytes + h.rec_bytes) // 4:].reshape(S, -1)[2]
    assert ring(h.state_words()).tobytes() == ring(state).tobytes()
    for b in (0, 1, 3, 4, 5):
        assert oc[b] == 150 and fl[b] == F - 150 and not (yh[b, :150] == POISON).any() and (yh[b, 150:] == POISON).all()
        outs[b] += [rows[b], yh[b, :150].view(np.float64).copy()]
    from vndecorrelate_amd.streaming import haas_voice_fade_spans
    good = np.where(np.arange(S) == 2, 0, counts)                      # the mirror of that call: slot 2 stood still
    _, h.mirror, h.mirror_records, h.mirror_left = haas_voice_fade_spans(
        h.mirror, h.mirror_records, good, np.where(np.arange(S) == 2, 0, flags), NEXT_DELAYS, D, F, M)
    only, switch = np.zeros(S, np.int32), np.zeros(S, np.int32)
    only[2], switch[2] = 150, SWITCH
    retry = h.call({2: x[2, 250:400]}, only, switch, NEXT_DELAYS, 'retry')
    outs[2] += [rows[2], retry[2]]
    assert h.mirror_left.tolist() == [F - 150] * S
    last = h.call({b: x[b, 400:] for b in range(S)}, *full(300, SWITCH | END), np.full(S, bad, np.int32), 'call 2')
    for b in range(S):
        got = _cat(outs[b] + [last[b]])
        fades = [(250, int(START_DELAYS[b]), int(NEXT_DELAYS[b]))]
        want = haas_fade(x[b], int(START_DELAYS[b]), fades, h.gains_host, F, len(got), **settings)
        assert len(got) == 700 + NEXT_DELAYS[b]                        # 250 + F <= 700: the old delay's reach is through
        _same(got, want, ('beside or after a bad switch', b))
    assert not h.positions().any()


# ---- 6. graph replay --------------------------------------------------------------------------------------------------
def _haas_bank(dec, delays=DELAYS, **kw):
    base = dict(sample_rate_hz=1000, delayed_channel=1, mode='MS', width=0.35)
    base.update(kw)
    return [dec.HaasEffect(delay_time_seconds=d / 1000, **base) for d in delays]


def _device_schedule(cx, seed, calls=9):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(calls):
        counts = rng.choice([0, 1, 7, 64, M - 1, M], S).astype(np.int32)
        flags = np.zeros(S, np.int32)
        delays = rng.choice(DELAYS, S).astype(np.int32)
        if i == 0:
            flags[:5] = START
        else:
            flags[rng.random(S) < 0.4] |= SWITCH
        if i == 3:
            flags[5] = START | END | SWITCH
            flags[1] |= END
        if i == 5:
            flags[1] = START
        if i == calls - 1:
            flags[:] |= END
        out.append((rng.uniform(-1, 1, (S, M, cx)).astype(np.float32), counts, flags, delays))
    return out


def test_graph_replay_equals_the_uncaptured_run(dec, ctx):
    import torch
    from vndecorrelate_amd.streaming import HaasFadeVoicePool, haas_voice_fade_spans
    cx = 2
    stages, calls = _haas_bank(dec), _device_schedule(cx, 4)
    dev = torch.device('cuda', ctx.device)

    def run(replayed):
        pool = dec.decorrelate_fade_voice_pool(stages, slots=S, in_channels=cx, max_frames_per_call=M, fade_frames=F)
        assert type(pool) is HaasFadeVoicePool and pool.row_frames == M + D
        x = torch.empty((S, M, cx), dtype=torch.float32, device=dev)
        counts, flags, delays, oc = (torch.empty(S, dtype=torch.int32, device=dev) for _ in range(4))
        y = torch.empty((S, pool.row_frames, 2), dtype=torch.int64, device=dev)
        out = (y.view(torch.float64), oc)
        pool.reset()                                                           # allocates state, gains, fade_left_dev
        left = pool.fade_left_dev
        if replayed:
            graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
            with torch.cuda.graph(graph, stream=side):
                pool.process_dev(x, counts, flags, delays, out=out)
            torch.cuda.synchronize(dev)
        results = []
        for xh, ch, fh, dh in calls:
            for t, v in ((x, xh), (counts, ch), (flags, fh), (delays, dh)):
                t.copy_(torch.from_numpy(v))
            y.fill_(POISON)
            if replayed:
                graph.replay()
            else:
                pool.process_dev(x, counts, flags, delays, out=out)
            torch.cuda.synchronize(dev)
            assert pool.fade_left_dev.data_ptr() == left.data_ptr()
            results.append((y.cpu().numpy(), oc.cpu().numpy(), left.cpu().numpy()))
        with pytest.raises(RuntimeError, match='runs through process_dev'):
            pool.process({})
        return results
    plain = run(False)                                                         # first: it loads the kernels
    replay = run(True)
    pos, rec, accepted, refused = np.zeros(S, np.int64), np.zeros((S, 3), np.int64), 0, 0
    for i, ((y0, c0, l0), (y1, c1, l1)) in enumerate(zip(plain, replay)):
        _, counts, flags, delays = calls[i]
        before, was = rec, pos
        want, pos, rec, left = haas_voice_fade_spans(pos, rec, counts, flags, delays, D, F, M)
        asked = ((flags & SWITCH) != 0) & ((flags & START) == 0) & (was != 0)
        changed = (rec != before).any(axis=1)
        accepted, refused = accepted + int((asked & changed).sum()), refused + int((asked & ~changed).sum())
        assert c0.tolist() == want.tolist() == c1.tolist(), i
        assert l0.tolist() == left.tolist() == l1.tolist(), i
        assert y0.tobytes() == y1.tobytes(), i                                 # outputs and untouched frames alike
        for b, n in enumerate(want):
            assert not (y0[b, :n] == POISON).any() and (y0[b, n:] == POISON).all(), (i, b)
    assert accepted and refused, (accepted, refused)


# ---- 7. the dict form -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cx', [1, 2])
def test_dict_form_with_switches(dec, cx):
    stages = _haas_bank(dec)
    settings = MS1
    pool = dec.decorrelate_fade_voice_pool(stages, slots=3, in_channels=cx, max_frames_per_call=M, fade_frames=F,
                                           fade='equal_power')
    assert pool.bank_delays.tolist() == list(DELAYS)
    a, b, c = (_noise((n, cx), 70 + n + cx) for n in (900, 700, 257))
    got = {name: [] for name in 'abc'}

    def take(out, **slots):
        assert sorted(out) == sorted(slots.values())
        for name, slot in slots.items():
            assert out[slot].dtype == np.float64
            got[name].append(out[slot])
    take(pool.process({0: a[:300], 1: b[:250]}, start={0: 3, 1: 5}), a=0, b=1)
    assert pool.transfers == {'to_device': 1, 'to_host': 1} and pool.fade_left.tolist() == [0, 0, 0]
    take(pool.process({0: a[300:600], 1: b[250:500], 2: c}, start={2: 4}, end=[2], switch={0: 5}), a=0, b=1, c=2)
    assert pool.fade_left.tolist() == [0, 0, 0]                                # 300 frames came back: the fade is through
    take(pool.process({0: a[600:700], 1: b[500:600]}, switch={0: 0, 1: 5}), a=0, b=1)
    assert pool.fade_left.tolist() == [100, 100, 0] and pool.records[:2].tolist() == [[600, 400, 0], [500, 400, 400]]
    with pytest.raises(ValueError, match='slot 1 has 100 frames of its fade left'):
        pool.process({1: b[600:]}, switch={1: 0})
    take(pool.process({0: a[700:], 1: b[600:]}, end=[0, 1]), a=0, b=1)         # a past its fade, b at its last frame
    assert not pool.positions.any() and not pool.live.any() and not pool.fade_left.any()
    assert pool.transfers == {'to_device': 1, 'to_host': 1}
    g = pool.fade_gains
    # a: 150 -> 400 at 300, -> 0 at 600, END at e = 900 with s + F - e = -100: the tail is the new delay's, none
    # b: 400 -> 400 at 500 (a * g0 + a * g1, and sin + cos is not 1), END at e = 700 = s + F: the tail is 400
    for name, x, first, fades, frames in (('a', a, 150, [(300, 150, 400), (600, 400, 0)], 900),
                                          ('b', b, 400, [(500, 400, 400)], 1100), ('c', c, 399, [], 257 + 399)):
        want = haas_fade(x, first, fades, g, F, frames, **settings)
        _same(_cat(got[name]), want, name)
    _same(_cat(got['c']), stages[4].decorrelate(c[:, 0] if cx == 1 else c), 'a voice that never switches')
    with pytest.raises(RuntimeError, match='runs through process\\(\\)'):
        pool.process_dev(None, None, None, None)


# ---- 8. the ABI's refusals --------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ctx):
    settings = LR1
    h = FadeHarness(ctx, 2, settings, F)
    x = _noise((S, 100, 2), 9)
    blocks = {b: x[b] for b in range(S)}
    counts, flags = np.full(S, 100, np.int32), np.full(S, START, np.int32)
    h.call(blocks, counts, flags, START_DELAYS, 'a good call')                 # positions 100: a refusal must keep them
    flags[:] = SWITCH
    before = h.state_words().copy()
    big = 1 << 40
    for override, status, text in (
            (dict(counts=0), INVALID, b'null'), (dict(flags=0), INVALID, b'null'), (dict(delays=0), INVALID, b'null'),
            (dict(x=0), INVALID, b'null'), (dict(y=0), INVALID, b'null'), (dict(out_counts=0), INVALID, b'null'),
            (dict(state=0), INVALID, b'null state'), (dict(ctx=None), INVALID, b'null context'),
            (dict(F=-1), INVALID, b'negative fade_frames'), (dict(F=(1 << 20) + 1), UNSUPPORTED, b'fade_frames'),
            (dict(gains=0), INVALID, b'null gains'),
            (dict(slots=-1), INVALID, b'negative'), (dict(M=-1), INVALID, b'max_frames_per_call'),
            (dict(max_delay=-1), INVALID, b'negative max_delay'),
            (dict(state_bytes=h.state_bytes - 4), INVALID, b'the crossfading Haas voice pool needs'),
            (dict(state=h.state.data_ptr() + 8), INVALID, b'16-byte aligned'),
            (dict(cx=3), INVALID, b'mono or stereo'), (dict(delayed_channel=2), INVALID, b'delayed_channel'),
            (dict(slots=65536, state_bytes=big), UNSUPPORTED, b'split the pool'),
            (dict(M=65535 * 256 - D + 1, state_bytes=big), UNSUPPORTED, b'one grid dimension')):
        rc, oc, yh, fl = h.raw(blocks, counts, flags, NEXT_DELAYS, override)
        message = h.lib.vnd_last_error()
        assert rc == status and text in message, (override, rc, message)
        assert (yh == POISON).all() and (oc == SENTINEL32).all() and (fl == SENTINEL32).all(), override
        assert h.state_words().tobytes() == before.tobytes(), override
    # the query and the reset check the same pool
    need = ctypes.c_int64(-1)
    query = h.lib.vnd_haas_voice_fade_stream_state_bytes
    assert query(S, 2, D, M, -1, ctypes.byref(need)) == INVALID and need.value == 0
    assert query(S, 2, D, M, (1 << 20) + 1, ctypes.byref(need)) == UNSUPPORTED and need.value == 0
    assert query(S, 3, D, M, F, ctypes.byref(need)) == INVALID and need.value == 0
    assert query(S, 2, D, M, 1 << 20, ctypes.byref(need)) == 0 and need.value == h.state_bytes
    rc = h.lib.vnd_haas_voice_fade_stream_reset_dev(ctx.handle, ctypes.c_void_p(h.state.data_ptr()), h.state_bytes - 4, S, 2, D,
                                                    M, F, ctypes.c_void_p(h.stream))
    assert rc == INVALID and b'the crossfading Haas voice pool needs' in h.lib.vnd_last_error()
    assert h.state_words().tobytes() == before.tobytes()
    # a null fade_left is taken, and F = 0 takes null gains: the voices of the first call switch hard and end
    hard = FadeHarness(ctx, 2, settings, 0)
    hard.call(blocks, counts, np.full(S, START, np.int32), START_DELAYS, 'F = 0: start')
    rc, oc, yh, fl = hard.raw({}, np.zeros(S, np.int32), np.full(S, SWITCH | END, np.int32), NEXT_DELAYS,
                              dict(gains=0, fade_left=0))
    assert rc == 0 and oc.tolist() == NEXT_DELAYS.tolist() and (fl == SENTINEL32).all()
    for b in range(S):
        d0, d1 = int(START_DELAYS[b]), int(NEXT_DELAYS[b])
        want = haas_fade(x[b], d0, [(100, d0, d1)], hard.gains_host, 0, 100 + d1, **settings)[100:]
        _same(yh[b, :d1].view(np.float64).copy(), want, ('a hard switch at the end', b))


# ---- 9. the chain pool ------------------------------------------------------------------------------------------------
CHAIN_HAAS = dict(delayed_channel=1, ms_mode=False, width=None)


def _chain_bank(dec):
    from test_gpu_each_stream import DURATION, FS, IMPULSES, SEED
    return [dec.SignalChain(sample_rate_hz=FS)
            .velvet_noise(duration_seconds=DURATION, num_impulses=IMPULSES, seed=SEED, normalizer=None, log_distribution_strength=k)
            .haas_effect(delay_time_seconds=d / FS, delayed_channel=1, mode='LR') for k, d in zip(CHAIN['kappas'], CHAIN['delays'])]


@pytest.fixture
def velvet_oracle(ctx):
    """The velvet stage's tables alone, for the C oracle's plain convolutions (test_gpu_voice_fade_pool._expected)."""
    from oracle import vnd_oracle as O
    from test_gpu_each_stream import Bank, _taps
    env = tuple(O.DEFAULT_ENVELOPE)
    bank = Bank.of_members(ctx, [(_taps(k, filtered=(0, 1)), env, True) for k in CHAIN['kappas']])
    yield bank
    bank.close()


def _chain_expected(velvet_oracle, v, gains, cx):
    """The composition: voice_fade_cases.blend on the C oracle's convolutions and the velvet stage's pointwise step
    (test_gpu_voice_fade_pool._expected), fed through the NumPy Haas fade."""
    from test_gpu_voice_fade_pool import _expected
    mid = _expected(velvet_oracle, v.x, v.table, v.fades1, gains, F, cx, (True, None))
    assert mid.dtype == np.float32 and mid.shape == (len(v.x), 2)
    return haas_fade(mid, v.delay, v.fades2, gains, F, v.frames, **CHAIN_HAAS)


@pytest.mark.parametrize('cx', [2, 1], ids=['stereo', 'mono'])
def test_chain_ragged_schedule_with_switches(dec, velvet_oracle, cx):
    """The dict form on a ragged schedule: blocks of every size, voices of 1 to 1500 frames, slots reused, a switch
    wherever fade_left allows one, among them switches inside a voice's first H frames - where stage 2 is fresh."""
    pool = dec.decorrelate_fade_voice_pool(_chain_bank(dec), slots=S, in_channels=cx, max_frames_per_call=M, fade_frames=F)
    H = pool.latency_frames
    assert H == velvet_oracle.H and pool.bank_tables.tolist() == [0, 1, 2, 3] and pool.bank_delays.tolist() == list(CHAIN['delays'])
    assert pool.row_frames == M + H + D
    calls, voices, counted = chain_schedule(CHAIN['seed'], slots=S, M=M, D=D, F=F, H=H, tables=pool.bank_tables,
                                            delays=pool.bank_delays, cx=cx)
    assert all(counted[case] for case in CHAIN['cases']), counted
    live, queue = {}, {b: iter([v for v in voices if v.slot == b]) for b in range(S)}
    for i, (blocks, start, end, switch, answers, left) in enumerate(calls):
        out = pool.process(blocks, start=start, end=end, switch=switch)
        assert pool.transfers == {'to_device': 1, 'to_host': 1}
        assert sorted(out) == sorted(answers) and pool.fade_left.tolist() == left, i
        for b in start:
            live[b] = next(queue[b])
        for b, rows in out.items():
            assert rows.shape == (answers[b], 2) and rows.dtype == np.float64, (i, b)
            live[b].out.append(rows)
    assert not pool.positions.any() and not pool.haas_positions.any() and not pool.live.any()
    switched = 0
    for v in voices:
        _same(_cat(v.out), _chain_expected(velvet_oracle, v, pool.fade_gains, cx),
              ('slot', v.slot, 'table', v.table, v.fades1, 'delay', v.delay, v.fades2))
        switched += bool(v.fades1 or v.fades2)
    assert switched >= 5 and len(voices) > 10, (switched, len(voices))


def test_chain_switch_inside_the_first_frames_is_fresh_in_stage_two(dec, velvet_oracle):
    """One voice switches after 100 frames, inside its first H: stage 1 has returned nothing, so stage 2 stands at position
    0 and takes the new delay without a fade, where stage 1 fades its filter from output frame 0."""
    cx = 2
    pool = dec.decorrelate_fade_voice_pool(_chain_bank(dec), slots=2, in_channels=cx, max_frames_per_call=M, fade_frames=F)
    H = pool.latency_frames
    assert 200 < H <= 319
    x = _noise((700, cx), 77)
    outs = [pool.process({1: x[:100]}, start={1: 3})[1]]
    assert len(outs[0]) == 0 and pool.fade_left.tolist() == [0, 0]
    outs.append(pool.process({1: x[100:400]}, switch={1: 1})[1])
    assert pool.records[1].tolist() == [0, 3, 1] and pool.haas_records[1].tolist() == [-F, 100, 100]
    assert len(outs[1]) == 400 - H and pool.fade_left[1] == max(0, F - (400 - H))
    outs.append(pool.process({1: x[400:]}, end=[1])[1])
    v = ChainVoice(x, 1, 1)
    v.table, v.fades1, v.delay, v.fades2, v.frames = 3, [(0, 3, 1)], 100, [], 700 + 100
    _same(_cat(outs), _chain_expected(velvet_oracle, v, pool.fade_gains, cx), 'the fresh corner')
    assert not pool.positions.any() and not pool.haas_positions.any()


def test_chain_and_a_meter_replay_in_one_graph(dec, ctx):
    """Velvet fade, Haas fade and a meter's process_dev captured in one graph: the replay equals the uncaptured run in
    every output - y, out_counts, both stages' fade_left through their maximum, the meter's moments and valid."""
    import torch
    from vndecorrelate_amd import analysis
    from vndecorrelate_amd.streaming import haas_voice_fade_spans, voice_fade_spans
    cx = 2
    dev = torch.device('cuda', ctx.device)
    calls = _device_schedule(cx, 8)
    rng = np.random.default_rng(6)
    entries = [rng.integers(0, 4, S) for _ in calls]

    def run(replayed):
        pool = dec.decorrelate_fade_voice_pool(_chain_bank(dec), slots=S, in_channels=cx, max_frames_per_call=M, fade_frames=F)
        meter = analysis.stereo_image_voice_pool(S, max_frames_per_call=pool.row_frames, dtype='float64')
        x = torch.empty((S, M, cx), dtype=torch.float32, device=dev)
        counts, flags, tables, delays, oc, valid = (torch.empty(S, dtype=torch.int32, device=dev) for _ in range(6))
        y = torch.empty((S, pool.row_frames, 2), dtype=torch.int64, device=dev)
        moments = torch.empty((S, 8), dtype=torch.int64, device=dev)
        pool.reset()
        meter.reset()
        left = pool.fade_left_dev

        def both():
            pool.process_dev(x, counts, flags, tables, delays, out=(y.view(torch.float64), oc))
            meter.process_dev(y.view(torch.float64), oc, flags, out=(moments.view(torch.float64), valid))
        if replayed:
            graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
            with torch.cuda.graph(graph, stream=side):
                both()
            torch.cuda.synchronize(dev)
        results = []
        for (xh, ch, fh, _), eh in zip(calls, entries):
            for t, v in ((x, xh), (counts, ch), (flags, fh), (tables, pool.bank_tables[eh].astype(np.int32)),
                         (delays, pool.bank_delays[eh].astype(np.int32))):
                t.copy_(torch.from_numpy(v))
            y.fill_(POISON)
            moments.fill_(POISON)
            graph.replay() if replayed else both()
            torch.cuda.synchronize(dev)
            assert pool.fade_left_dev.data_ptr() == left.data_ptr()
            results.append((y.cpu().numpy(), oc.cpu().numpy(), left.cpu().numpy(), moments.cpu().numpy(), valid.cpu().numpy(),
                            pool._mid[1].cpu().numpy()))
        return pool, results
    pool, plain = run(False)                                                   # first: it loads the kernels
    _, replay = run(True)
    H = pool.latency_frames
    p1, r1, p2, r2 = np.zeros(S, np.int64), np.zeros((S, 3), np.int64), np.zeros(S, np.int64), np.zeros((S, 3), np.int64)
    fading = 0
    for i, (a, b) in enumerate(zip(plain, replay)):
        _, counts, flags, _ = calls[i]
        mid, p1, r1, l1 = voice_fade_spans(p1, r1, counts, flags, pool.bank_tables[entries[i]], H, F, M)
        want, p2, r2, l2 = haas_voice_fade_spans(p2, r2, mid, flags, pool.bank_delays[entries[i]], D, F, M + H)
        assert a[5].tolist() == mid.tolist() and a[1].tolist() == want.tolist(), i
        assert a[2].tolist() == np.maximum(l1, l2).tolist(), i
        fading += int((a[2] > 0).sum())
        for k, (u, w) in enumerate(zip(a, b)):
            assert u.tobytes() == w.tobytes(), (i, k)                          # outputs and untouched frames alike
        for s, n in enumerate(want):
            assert not (a[0][s, :n] == POISON).any() and (a[0][s, n:] == POISON).all(), (i, s)
        work = (want > 0) | ((flags & (START | END)) != 0)                     # (a meter does not know the SWITCH bit)
        assert a[4].tolist() == work.astype(int).tolist(), i
    assert fading and not p1.any() and not p2.any()
