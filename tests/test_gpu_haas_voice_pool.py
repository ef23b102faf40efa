"""GPU tier of the Haas voice pool (vnd_haas_voice_stream_f64_*, include/vnd_haas_voice_stream.h; streaming.HaasVoicePool):
slots over a bank of delays whose voices start, end and bring their own block sizes call by call, the position of every
slot in the device state.  Every comparison is bit for bit.

The C ABI runs through a poisoned harness, as test_gpu_voice_pool.py's: the ring starts as NaN and is never cleared (the
positions start as NaN bits too, and vnd_haas_voice_stream_reset_dev zeroes them alone), the chunk rows are NaN past
counts[b], y is prefilled with a NaN no arithmetic produces and ends in a sentinel tail.  After each call out_counts is
streaming.haas_voice_spans', every frame below out_counts[b] was written, every frame at or past it was not, the tail is
intact and the positions on the device are the mirror's.  S = 6, M = 600 and the delays {0, 1, 7, 255, 256, 257, 599, 600,
601, 1300}: max_delay = 1300 is above M, so a delayed read reaches back across three calls and the ring wraps; a row is
1900 frames, eight workgroups.  A voice's concatenated outputs equal the oracle's haas_effect on its whole signal."""
import ctypes
import hashlib

import numpy as np
import pytest

from conftest import make_input
from oracle import vnd_oracle as O
from test_gpu_each_stream import PoisonedHaas, _calls, _noise
from test_gpu_voice_pool import Voice, _drive

pytestmark = pytest.mark.gpu

S, M = 6, 600
DELAYS = (0, 1, 7, 255, 256, 257, 599, 600, 601, 1300)
MAX_DELAY = max(DELAYS)
TAIL = 512                                   # int64 words of sentinel behind the last row
START, END = 1, 2
INVALID, UNSUPPORTED = 1, 4
NAN_BITS = 0x7FC00000                        # the ring's and the positions' first contents
POISON = 0x7FF4A5A5A5A5A5A5                  # a signalling NaN: no kernel arithmetic yields it
SENTINEL = 0x7FF5B0B0B0B0B0B0
SENTINEL32 = 0x7FB0B0B0
MAX_POSITION = 1 << 60
BIG_M = 2100
SETTINGS = {'lr-ch0': (2, dict(delayed_channel=0, ms_mode=False, width=None)),
            'lr-ch1': (2, dict(delayed_channel=1, ms_mode=False, width=None)),
            'ms-width-ch1': (2, dict(delayed_channel=1, ms_mode=True, width=0.35)),
            'ms-width-ch0': (2, dict(delayed_channel=0, ms_mode=True, width=0.35)),
            'mono-lr-ch1': (1, dict(delayed_channel=1, ms_mode=False, width=None)),
            'mono-ms-width-ch0': (1, dict(delayed_channel=0, ms_mode=True, width=0.35))}


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


_REFERENCES = {}


def _reference(x, d, cx, settings):
    """One voice alone through the oracle's haas_effect: float64 (n + d, 2), computed once per signal and form."""
    key = (x.tobytes(), int(d), cx, tuple(sorted(settings.items(), key=lambda kv: kv[0])))
    if key not in _REFERENCES:
        _REFERENCES[key] = O.haas_effect(x[:, 0] if cx == 1 else x, sample_rate_hz=1, delay_time_seconds=float(d),
                                         delayed_channel=settings['delayed_channel'],
                                         mode='MS' if settings['ms_mode'] else 'LR', width=settings['width'])
        assert _REFERENCES[key].shape == (len(x) + d, 2) and _REFERENCES[key].dtype == np.float64
    return _REFERENCES[key]


def _same(got, want, where):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64, (where, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.int64) != want.view(np.int64))
        raise AssertionError((where, 'first (frame, channel)', tuple(bad[0]), len(bad), float(got[tuple(bad[0])]),
                              float(want[tuple(bad[0])])))


def _cat(rows):
    rows = [r for r in rows if len(r)]
    return np.concatenate(rows) if rows else np.zeros((0, 2), np.float64)


class Harness:
    """One pool's poisoned state and buffers, the host's mirror of the positions, and the calls of
    vnd_haas_voice_stream_f64_dev on them."""

    def __init__(self, ctx, cx, settings, max_delay=MAX_DELAY, slots=S, max_frames=M):
        import torch
        from vndecorrelate_amd import _native
        self.torch, self.ctx, self.lib, self.native = torch, ctx, ctx._lib, _native
        self.S, self.M, self.D, self.cx, self.settings = slots, max_frames, max_delay, cx, settings
        self.dev = torch.device('cuda', ctx.device)
        self.pos_bytes = (slots * 8 + 15) & ~15
        self.state_bytes = _native.haas_voice_stream_state_bytes(slots, cx, max_delay, max_frames)
        assert self.state_bytes == self.pos_bytes + (slots * (max_delay + max_frames) * cx * 4 if max_delay else 0)
        self.state = torch.full((self.state_bytes // 4,), float('nan'), dtype=torch.float32, device=self.dev)
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream
        _native.haas_voice_stream_reset_device(ctx, self.state.data_ptr(), self.state_bytes, slots, cx, max_delay, max_frames,
                                               stream=self.stream)
        words = self.state_words()
        assert not words[:self.pos_bytes // 4].any(), 'the reset leaves positions that are not 0'
        assert (words[self.pos_bytes // 4:] == NAN_BITS).all(), 'the reset cleared the ring'
        self.rows = max_frames + max_delay
        self.body = slots * self.rows * 2
        self.x = torch.empty((slots, max_frames, cx), dtype=torch.float32, device=self.dev)
        self.y = torch.empty((self.body + TAIL,), dtype=torch.int64, device=self.dev)
        self.ints = torch.empty((3, slots), dtype=torch.int32, device=self.dev)           # counts, flags, delays
        self.out_counts = torch.empty((slots + 8,), dtype=torch.int32, device=self.dev)
        self.mirror = np.zeros(slots, np.int64)

    def state_words(self):
        return self.state.view(self.torch.int32).cpu().numpy()

    def positions(self):
        return self.state[:self.pos_bytes // 4].view(self.torch.int64).cpu().numpy()[:self.S].copy()

    def ring(self):
        """The ring as int32 words, (S, max_delay + M, cx)."""
        return self.state_words()[self.pos_bytes // 4:].reshape(self.S, self.D + self.M, self.cx)

    def plant(self, slot, position, history):
        """Put `slot` at `position` as the header lays the state out: the int64 position, and the max_delay frames below
        it - absolute frames [position - max_delay, position) - each in ring slot (absolute frame mod capacity).  Every
        other word of the slot's ring stays NaN."""
        torch, D, cap = self.torch, self.D, self.D + self.M
        assert history.shape == (D, self.cx) and history.dtype == np.float32
        ring = self.state[self.pos_bytes // 4:].view(self.S, cap, self.cx)
        where = np.array([(position - D + j) % cap for j in range(D)], np.int64)        # Python integers: no wrap
        ring[slot, torch.from_numpy(where).to(self.dev)] = torch.from_numpy(history).to(self.dev)
        self.set_position(slot, position)

    def set_position(self, slot, position):
        self.state[:self.pos_bytes // 4].view(self.torch.int64)[slot] = position
        self.mirror[slot] = position
        assert int(self.positions()[slot]) == position

    def raw(self, blocks, counts, flags, delays, override=None):
        """One call on poisoned buffers: (status, out_counts, y as int64 (S, M + max_delay, 2)); the tail is checked here."""
        torch = self.torch
        xh = np.full((self.S, self.M, self.cx), np.nan, np.float32)                       # NaN past counts[b]: never read
        for slot, block in blocks.items():
            xh[slot, :len(block)] = block
        self.x.copy_(torch.from_numpy(xh))
        self.ints.copy_(torch.from_numpy(np.stack([counts, flags, delays]).astype(np.int32)))
        self.y[:self.body] = POISON
        self.y[self.body:] = SENTINEL
        self.out_counts[:] = SENTINEL32
        a = dict(ctx=self.ctx.handle, state=self.state.data_ptr(), state_bytes=self.state_bytes, M=self.M,
                 x=self.x.data_ptr(), counts=self.ints[0].data_ptr(), flags=self.ints[1].data_ptr(),
                 delays=self.ints[2].data_ptr(), y=self.y.data_ptr(), out_counts=self.out_counts.data_ptr(), slots=self.S,
                 cx=self.cx, max_delay=self.D, delayed_channel=self.settings['delayed_channel'])
        a.update(override or {})
        width = self.settings['width']
        rc = self.lib.vnd_haas_voice_stream_f64_dev(
            a['ctx'], ctypes.c_void_p(a['state']), a['state_bytes'], a['M'], ctypes.c_void_p(a['x']),
            ctypes.c_void_p(a['counts']), ctypes.c_void_p(a['flags']), ctypes.c_void_p(a['delays']), ctypes.c_void_p(a['y']),
            ctypes.c_void_p(a['out_counts']), a['slots'], a['cx'], a['max_delay'], a['delayed_channel'],
            int(self.settings['ms_mode']), int(width is not None), float(width or 0.0), ctypes.c_void_p(self.stream))
        yh, oc = self.y.cpu().numpy(), self.out_counts.cpu().numpy()
        assert (yh[self.body:] == SENTINEL).all(), 'the call wrote behind the last row'
        assert (oc[self.S:] == SENTINEL32).all(), 'the call wrote behind out_counts'
        return rc, oc[:self.S].copy(), yh[:self.body].reshape(self.S, self.rows, 2)

    def call(self, blocks, counts, flags, delays, where=''):
        """A call that must succeed, held to haas_voice_spans and to its footprint: the rows as float64, one per slot."""
        from vndecorrelate_amd.streaming import haas_voice_spans
        rc, oc, yh = self.raw(blocks, counts, flags, delays)
        assert rc == 0, self.lib.vnd_last_error()
        want, self.mirror = haas_voice_spans(self.mirror, counts, flags, delays, self.D, self.M)
        assert oc.tolist() == want.tolist(), (where, counts, flags, delays)
        assert self.positions().tolist() == self.mirror.tolist(), f'{where}: the positions on the device are not the mirror\'s'
        rows = []
        for b, n in enumerate(np.maximum(want, 0)):
            hole = np.argwhere(yh[b, :n] == POISON)
            assert not len(hole), f'{where}: slot {b} left (frame, channel) {tuple(hole[0])} of its {n} frames unwritten'
            assert (yh[b, n:] == POISON).all(), f'{where}: slot {b} wrote at or past its {n} frames'
            rows.append(yh[b, :n].view(np.float64).copy())
        return rows


def _check_voices(plan, cx, settings):
    for slot, voices in plan.items():
        for i, v in enumerate(voices):
            want = _reference(v.x, v.table, cx, settings)                  # (Voice.table holds the voice's delay)
            got = _cat(v.out)
            if v.discard_after is None:
                _same(got, want, ('slot', slot, 'voice', i, 'delay', v.table))
            else:                                       # what it returned before it was dropped is final all the same
                assert len(got) == v.discard_after
                _same(got, want[:len(got)], ('slot', slot, 'discarded voice', i))


# ---- 1. a ragged schedule, and the footprint of every call ------------------------------------------------------------
def _ragged_plan(cx, seed):
    """Voices of 1, 200, 255, 257, 1300 and 2049 frames that start on different calls and meet every delay of the bank:
    slots 0 - 3 are reused after END by a voice with another delay; slot 5's first voice is discarded by a START without
    END; slot 0's first voice is one frame with d = 1300, START + END in one call."""
    sig = lambda n, k: _noise((n, cx), seed + k)
    return {0: [Voice(sig(1, 0), 1300, 0, whole=True), Voice(sig(700, 1), 7, 4, end_with_last=False)],
            1: [Voice(sig(200, 2), 599, 1, end_with_last=False), Voice(sig(300, 8), 0, 0)],
            2: [Voice(sig(255, 3), 256, 0), Voice(sig(400, 9), 600, 3)],
            3: [Voice(sig(257, 4), 255, 2, end_with_last=False), Voice(sig(350, 10), 601, 0)],
            4: [Voice(sig(1300, 5), 1, 3, end_with_last=False)],
            5: [Voice(sig(900, 6), 257, 1, discard_after=450), Voice(sig(2049, 7), 1300, 0)]}


@pytest.mark.parametrize('name', list(SETTINGS))
def test_ragged_schedule(ctx, name):
    cx, settings = SETTINGS[name]
    plan = _ragged_plan(cx, 100 * cx)
    assert sorted({v.table for voices in plan.values() for v in voices}) == sorted(DELAYS)
    h = Harness(ctx, cx, settings)
    calls = _drive(h, plan, np.random.default_rng(7 + cx))
    assert calls > 8
    _check_voices(plan, cx, settings)
    assert not h.positions().any() and not h.mirror.any()           # every voice ended: every slot is back at 0
    assert not np.isnan(_cat(plan[5][1].out)).any()                 # nothing of the discarded voice, no NaN from the ring
    # the ring was written by the calls alone: slot 4 pushed 1300 < max_delay + M frames and ended with an END alone (a
    # block that comes with END is not kept), the rest is still NaN
    ring = h.ring()
    assert (ring[4, 1300:] == NAN_BITS).all() and not (ring[4, :1300] == NAN_BITS).any()


# ---- 2. the reference's goldens, one voice each beside a neighbour ------------------------------------------------------
def _schedule(kind, n, seed=0, top=480):
    """test_gpu_chain_stream.py's schedules: blocks of 1, 64 or 480 frames, or random sizes in [0, 480] with idle calls."""
    if kind == 'random':
        rng, out, left = np.random.default_rng(seed), [], n
        while left > 0:
            b = int(min(left, rng.choice([0, 0, int(rng.integers(0, top + 1)), top])))
            out.append(b)
            left -= b
        return out
    step = int(kind)
    return [step] * (n // step) + ([n % step] if n % step else [])


@pytest.mark.parametrize('kind', ['1', '64', '480', 'random'])
def test_goldens_as_one_voice_beside_a_neighbour(dec, ctx, golden, kind):
    """Slot 0 is the golden's voice, ended by an END alone; slot 1 a neighbour with another delay that pushes a full block
    on every call and never ends.  The blocks and the results stay on the device: one download per golden."""
    import torch
    dev = torch.device('cuda', ctx.device)
    top = 480 if kind == 'random' else int(kind)
    for name, meta in golden.manifest['haas'].items():
        x = make_input(meta['input']).astype(np.float32)
        n, cx = x.shape[0], 1 if x.ndim == 1 else 2
        stage = dec.HaasEffect(**meta['kwargs'])
        d = round(meta['kwargs']['delay_time_seconds'] * meta['kwargs']['sample_rate_hz'])
        other = dec.HaasEffect(**dict(meta['kwargs'], delay_time_seconds=(d + 3) / meta['kwargs']['sample_rate_hz']))
        pool = dec.decorrelate_voice_pool([stage, other], slots=2, in_channels=cx, max_frames_per_call=top)
        assert pool.bank_delays.tolist() == [d, d + 3] and pool.row_frames == top + d + 3
        sched = _schedule(kind, n, 0, top) + [0]
        xd = torch.from_numpy(x.reshape(n, cx)).to(dev)
        noise = torch.from_numpy(_noise((top, cx), 5)).to(dev)
        block = torch.zeros((2, top, cx), dtype=torch.float32, device=dev)
        block[1] = noise
        ints = np.zeros((len(sched), 2, 2), np.int32)                 # per call: counts, flags
        ints[:, 0, 0], ints[:, 0, 1] = sched, top
        ints[0, 1, :] = START
        ints[-1, 1, 0] = END
        ints_dev = torch.from_numpy(ints).to(dev)
        delays = torch.from_numpy(pool.bank_delays.copy()).to(dev)
        out = torch.full((n + d, 2), float('nan'), dtype=torch.float64, device=dev)
        y = torch.empty((2, pool.row_frames, 2), dtype=torch.float64, device=dev)
        counts_out = torch.empty((len(sched), 2), dtype=torch.int32, device=dev)
        pool.reset()
        pos = 0
        for i, b in enumerate(sched):
            block[0, :b] = xd[pos:pos + b]
            y.view(torch.int64).fill_(POISON)
            pool.process_dev(block, ints_dev[i, 0], ints_dev[i, 1], delays, out=(y, counts_out[i]))
            k = b + (d if i == len(sched) - 1 else 0)
            out[pos:pos + k] = y[0, :k]
            pos += b
        got, oc = out.cpu().numpy(), counts_out.cpu().numpy()
        assert oc[:, 0].tolist() == sched[:-1] + [d] and (oc[:, 1] == top).all(), (name, kind)
        assert list(got.shape) == meta['out_shape'], (name, kind)
        assert hashlib.sha256(got.tobytes()).hexdigest() == meta['out_sha256'], (name, kind)


# ---- 3. edge calls ----------------------------------------------------------------------------------------------------
def test_edge_calls(ctx):
    """END alone; START with END (one shorter than its delay); START alone with n = 0; idle slots with any delay value."""
    cx, settings = SETTINGS['ms-width-ch1']
    h = Harness(ctx, cx, settings)
    xs = [_noise((n, cx), 40 + n) for n in (150, 600, 600, 5)]
    delays = np.array([599, 1300, 0, 257, 7, 2 ** 31 - 1], np.int32)      # slot 5 is idle throughout: its delay is not read
    zero = np.zeros(S, np.int32)
    counts = np.array([150, 600, 600, 5, 0, 0], np.int32)
    flags = np.array([START, START, START, START | END, START, 0], np.int32)
    r0 = h.call({b: xs[b] for b in range(4)}, counts, flags, delays, 'call 0')
    assert [len(r) for r in r0] == [150, 600, 600, 5 + 257, 0, 0]
    _same(r0[3], _reference(xs[3], 257, cx, settings), 'a whole voice of 5 frames with d = 257 in one call')
    # call 1: END alone everywhere: the d tail frames - none for d = 0; 7 for slot 4, at position 0 after its START; 1 for
    # slot 5, which never started
    delays[5] = 1
    r1 = h.call({}, zero, np.array([END, END, END, 0, END, END], np.int32), delays, 'call 1')
    assert [len(r) for r in r1] == [599, 1300, 0, 0, 7, 1]
    for b in range(3):
        _same(_cat([r0[b], r1[b]]), _reference(xs[b], delays[b], cx, settings), ('flushed', b))
    assert not np.concatenate([r1[4], r1[5]]).view(np.int64).any()     # a voice of no frames: d frames of +0.0
    # call 2: nothing anywhere, whatever the delays say
    bad = np.array([-1, MAX_DELAY + 1, 0, 0, -2 ** 31, 2 ** 31 - 1], np.int32)
    assert [len(r) for r in h.call({}, zero, zero, bad, 'call 2')] == [0] * S
    assert not h.positions().any()


def test_a_pool_without_delay_has_no_ring(ctx):
    cx, settings = SETTINGS['lr-ch0']
    h = Harness(ctx, cx, settings, max_delay=0, slots=3, max_frames=300)
    assert h.state_bytes == h.pos_bytes == 32 and h.rows == 300
    x = _noise((3, 700, cx), 3)
    outs, pos = [[] for _ in range(3)], 0
    for i, n in enumerate((300, 0, 299, 101)):
        flags = np.full(3, (START if i == 0 else 0) | (END if i == 3 else 0), np.int32)
        rows = h.call({b: x[b, pos:pos + n] for b in range(3)}, np.full(3, n, np.int32), flags, np.zeros(3, np.int32), f'call {i}')
        for b in range(3):
            outs[b].append(rows[b])
        pos += n
    for b in range(3):
        _same(_cat(outs[b]), _reference(x[b], 0, cx, settings), b)
    rc, oc, yh = h.raw({}, np.full(3, 1, np.int32), np.zeros(3, np.int32), np.array([0, 1, -1], np.int32))
    assert rc == 0 and oc.tolist() == [1, -1, -1]                     # a delay above max_delay = 0


# ---- 4. lockstep ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['ms-width-ch1', 'mono-lr-ch1'])
def test_lockstep_equals_haas_each_stream_call_by_call(ctx, name):
    cx, settings = SETTINGS[name]
    delays = np.array([0, 1, 257, 600, 601, 1300], np.int32)
    sizes = [600, 0, 37, 263, 600, 1]
    x = _noise((S, sum(sizes), cx), 11 + cx)
    lock = PoisonedHaas(ctx, delays, MAX_DELAY, cx, M, settings)
    whole = lock.signal(x, _calls(sizes, 'final'))                     # (S, n + max_delay, 2): every call's frames in order
    h = Harness(ctx, cx, settings)
    pos = 0
    for i, n in enumerate(sizes):
        final = i == len(sizes) - 1
        flags = np.full(S, (START if i == 0 else 0) | (END if final else 0), np.int32)
        rows = h.call({b: x[b, pos:pos + n] for b in range(S)}, np.full(S, n, np.int32), flags, delays, f'call {i}')
        for b in range(S):
            k = n + (int(delays[b]) if final else 0)                   # the lockstep pool pads the rest with +0.0
            assert rows[b].tobytes() == whole[b, pos:pos + k].tobytes(), (i, b)
        pos += n
    assert not h.positions().any()


# ---- 5. pools past one advance group ------------------------------------------------------------------------------------
def _pool_plan(slots, cx, delays, seed):
    """({slot: [Voice, ...]}, the slots never started): the first six slots hold the cases by name, the others draw from
    them - a tenth reused, a few END alone, a few discarded, some never started, the rest one voice."""
    rng = np.random.default_rng(seed)
    sig = lambda n, k: _noise((n, cx), 100003 * seed + k)
    D = max(delays)
    lengths = (1, 150, 255, 257, BIG_M, BIG_M + D + 1, 2 * BIG_M + 3)
    plan = {0: [Voice(sig(1, 0), D, 0, whole=True), Voice(sig(BIG_M + D + 1, 1), delays[1], 2, end_with_last=False)],
            1: [Voice(sig(150, 2), delays[2], 1, end_with_last=False)],
            2: [Voice(sig(255, 3), 0, 0)],
            3: [Voice(sig(BIG_M, 5), delays[1], 1, discard_after=900), Voice(sig(2 * BIG_M + 3, 6), D, 0)],
            4: [Voice(sig(257, 4), delays[3], 3)]}
    never = [5]
    for slot in range(6, slots):
        u, k = rng.random(), 10 + 2 * slot
        short = int(rng.choice(lengths[:6]))
        n = lengths[6] if rng.random() < 0.05 else short
        d, start = int(rng.choice(delays)), int(rng.integers(0, 4))
        if u < 0.08:
            never.append(slot)
        elif u < 0.18:
            plan[slot] = [Voice(sig(short, k), d, start % 2, end_with_last=bool(rng.random() < 0.5)),
                          Voice(sig(int(rng.choice(lengths[:6])), k + 1), int(rng.choice(delays)), 0)]
        elif u < 0.22:
            first = max(short, 255)
            plan[slot] = [Voice(sig(first, k), d, start % 2, discard_after=int(rng.integers(1, first))),
                          Voice(sig(int(rng.choice(lengths[:6])), k + 1), int(rng.choice(delays)), 0)]
        elif u < 0.27:
            plan[slot] = [Voice(sig(n, k), d, start, end_with_last=False)]
        else:
            plan[slot] = [Voice(sig(n, k), d, 0 if n == lengths[-1] else start)]
    return plan, never


@pytest.mark.parametrize('groups', [1, 3, 4])
def test_pool_sizes(ctx, groups):
    """7, 2 x CUs + 1 and 3 x CUs + 1 slots of M = 2100 frames: one, and on 256 CUs three and four advance workgroups, the
    last with one live lane.  h.call reads the positions back after every call and holds them to the mirror."""
    cus = ctx.info()['compute_units']
    slots = {1: 7, 3: 2 * cus + 1, 4: 3 * cus + 1}[groups]
    assert slots % 256 == 1 or groups == 1
    cx, settings = SETTINGS['ms-width-ch0'] if groups != 3 else SETTINGS['mono-lr-ch1']
    delays = (0, 1, 255, 256, 257, 700)
    plan, never = _pool_plan(slots, cx, delays, 10 * groups + cx)
    h = Harness(ctx, cx, settings, max_delay=700, slots=slots, max_frames=BIG_M)
    calls = _drive(h, plan, np.random.default_rng(3 + groups))
    assert calls >= 4, calls
    print(f'{calls} calls, {slots} slots, {sum(len(v) for v in plan.values())} voices')
    try:
        _check_voices(plan, cx, settings)
    finally:
        _REFERENCES.clear()
    assert not h.positions().any() and not h.mirror.any()
    assert (h.ring()[never] == NAN_BITS).all(), 'a slot that never started has frames in its ring'


# ---- 6. positions a long-lived voice reaches --------------------------------------------------------------------------
PLANTED = (2 ** 31 - 7, 2 ** 32 - 300, 2 ** 32 + 12345, 2 ** 40 + 3, 2 ** 53 + 1,
           None)               # 2^60 less the frames the slot pushes: its last call, an END alone, is at 2^60 exactly


@pytest.mark.parametrize('name', ['ms-width-ch1', 'mono-ms-width-ch0'])
def test_planted_positions(ctx, name):
    """No START anywhere: every slot goes on from the position and the max_delay frames of history planted in its state.
    The outputs from the planted position on are the oracle's on the signal that starts max_delay frames below it."""
    cx, settings = SETTINGS[name]
    h = Harness(ctx, cx, settings)
    D = MAX_DELAY
    delays = np.array([1300, 601, 257, 256, 1, 600], np.int32)
    rng = np.random.default_rng(50 + cx)
    pushed = [int(n) for n in rng.integers(900, 1900, S)]
    sigs = [_noise((D + n, cx), 300 + 10 * cx + b) for b, n in enumerate(pushed)]
    start = [MAX_POSITION - pushed[b] if P is None else P for b, P in enumerate(PLANTED)]
    for b in range(S):
        h.plant(b, start[b], sigs[b][:D])
    assert h.mirror.tolist() == start
    done, ended, outs = [0] * S, [False] * S, [[] for _ in range(S)]
    call = 0
    while not all(ended):
        assert call < 40
        blocks, counts, flags = {}, np.zeros(S, np.int32), np.zeros(S, np.int32)
        for b in range(S):
            if ended[b]:
                continue
            left = pushed[b] - done[b]
            n = min(left, 0 if rng.random() < 0.3 else int(rng.integers(1, M + 1)))
            if PLANTED[b] is None and left == 0:                       # the position is 2^60: the largest one taken
                assert int(h.mirror[b]) == MAX_POSITION
                flags[b], ended[b] = END, True
            elif n == left and PLANTED[b] is not None and left:
                flags[b], ended[b] = END, True                         # END on the last block
            if n:
                blocks[b] = sigs[b][D + done[b]:D + done[b] + n]
            counts[b] = n
            done[b] += n
        rows = h.call(blocks, counts, flags, delays, f'call {call}')
        for b in range(S):
            outs[b].append(rows[b])
        call += 1
    assert call > 3 and not h.positions().any()
    for b in range(S):
        _same(_cat(outs[b]), _reference(sigs[b], delays[b], cx, settings)[D:], ('planted at', start[b]))


def test_a_position_above_the_range_leaves_the_slot_alone(ctx):
    cx, settings = SETTINGS['lr-ch1']
    h = Harness(ctx, cx, settings)
    delays = np.array([0, 1, 257, 600, 601, 1300], np.int32)
    x = _noise((S, 1000, cx), 8)
    blocks = lambda first, n: {b: x[b, first:first + n] for b in range(S)}
    h.call(blocks(0, 400), np.full(S, 400, np.int32), np.full(S, START, np.int32), delays, 'call 0')
    h.state[:h.pos_bytes // 4].view(h.torch.int64)[3] = MAX_POSITION + 1
    before = h.state_words().copy()
    rc, oc, yh = h.raw(blocks(400, 600), np.full(S, 600, np.int32), np.full(S, END, np.int32), delays)
    assert rc == 0, h.lib.vnd_last_error()
    assert oc[3] == -1 and (yh[3] == POISON).all()
    assert int(h.positions()[3]) == MAX_POSITION + 1
    assert h.ring()[3].tobytes() == before[h.pos_bytes // 4:].reshape(S, -1)[3].tobytes()
    for b in (0, 1, 2, 4, 5):                                          # the neighbours end as if nothing had happened
        assert oc[b] == 600 + delays[b] and (yh[b, oc[b]:] == POISON).all()
        _same(yh[b, :oc[b]].view(np.float64), _reference(x[b], delays[b], cx, settings)[400:], ('beside a bad position', b))
    from vndecorrelate_amd.streaming import haas_voice_spans
    h.mirror[:] = 0
    h.mirror[3] = MAX_POSITION + 1
    counts, flags = np.zeros(S, np.int32), np.zeros(S, np.int32)
    counts[3] = 500
    out, new = haas_voice_spans(h.mirror, counts, flags, delays, MAX_DELAY, M)
    assert out[3] == -1 and new[3] == MAX_POSITION + 1
    flags[3] = START | END
    rows = h.call({3: x[3, :500]}, counts, flags, delays, 'restarted')
    _same(rows[3], _reference(x[3, :500], 600, cx, settings), 'START over a bad position')
    assert not h.positions().any()


# ---- 7. bad per-slot values ---------------------------------------------------------------------------------------------
BAD_DELAYS = np.array([7, 1300, 257, 600, 0, 601], np.int32)


def _bad_value_run(ctx, spoil):
    """Three calls of every slot; `spoil` = (counts[2], delays[2]) of the second call, or None.  The spoiled call is lost to
    slot 2, which pushes the block it meant to push on a call of its own afterwards."""
    cx, settings = SETTINGS['ms-width-ch1']
    x = _noise((S, 1500, cx), 5)
    sizes = [500, 400, 600]
    h = Harness(ctx, cx, settings)
    outs, pos = [[] for _ in range(S)], 0
    for i, n in enumerate(sizes):
        flags = np.full(S, (START if i == 0 else 0) | (END if i == 2 else 0), np.int32)
        blocks = {b: x[b, pos:pos + n] for b in range(S)}
        if spoil is not None and i == 1:
            counts, delays = np.full(S, n, np.int32), BAD_DELAYS.copy()
            counts[2] = n if spoil[0] is None else spoil[0]
            delays[2] = BAD_DELAYS[2] if spoil[1] is None else spoil[1]
            before, state = h.positions(), h.state_words().copy()
            rc, oc, yh = h.raw(blocks, counts, flags, delays)
            assert rc == 0, h.lib.vnd_last_error()
            assert oc[2] == -1 and (yh[2] == POISON).all()                   # the row is untouched
            assert h.positions()[2] == before[2] == 500                      # the position and the ring are unchanged
            ring = lambda w: w[h.pos_bytes // 4:].reshape(S, -1)[2]
            assert ring(h.state_words()).tobytes() == ring(state).tobytes()
            for b in (0, 1, 3, 4, 5):
                assert oc[b] == n and not (yh[b, :n] == POISON).any() and (yh[b, n:] == POISON).all()
                outs[b].append(yh[b, :n].view(np.float64).copy())
            h.mirror += np.where(np.arange(S) == 2, 0, n)
            one = np.zeros(S, np.int32)
            one[2] = n
            rows = h.call({2: x[2, pos:pos + n]}, one, np.zeros(S, np.int32), BAD_DELAYS, 'retry')
            outs[2].append(rows[2])
        else:
            rows = h.call(blocks, np.full(S, n, np.int32), flags, BAD_DELAYS, f'call {i}')
            for b in range(S):
                outs[b].append(rows[b])
        pos += n
    return x, [_cat(o) for o in outs]


@pytest.fixture(scope='module')
def clean_run(ctx):
    cx, settings = SETTINGS['ms-width-ch1']
    x, clean = _bad_value_run(ctx, None)
    for b in range(S):
        _same(clean[b], _reference(x[b], BAD_DELAYS[b], cx, settings), ('clean', b))
    return clean


@pytest.mark.parametrize('bad_count, bad_delay', [(M + 1, None), (-1, None), (2 ** 31 - 1, None), (-2 ** 31, None),
                                                  (None, -1), (None, MAX_DELAY + 1)])
def test_a_bad_count_or_delay_leaves_the_slot_alone(ctx, clean_run, bad_count, bad_delay):
    _, spoiled = _bad_value_run(ctx, (bad_count, bad_delay))
    for b in range(S):
        _same(spoiled[b], clean_run[b], ('beside or after a bad value', b))


# ---- 8. graph replay and the Python forms -----------------------------------------------------------------------------
def _haas_bank(dec, delays, **kw):
    base = dict(sample_rate_hz=1000, delayed_channel=1, mode='MS', width=0.35)
    base.update(kw)
    return [dec.HaasEffect(delay_time_seconds=d / 1000, **base) for d in delays]


def _python_schedule(cx, seed):
    """A ragged schedule as process_dev arrays: 8 calls of (blocks, counts, flags) over 6 slots, with a START and an END
    inside, a reused slot and idle calls; the delays are fixed per slot."""
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


def test_graph_replay_equals_the_uncaptured_run(dec, ctx):
    import torch
    from vndecorrelate_amd.streaming import haas_voice_spans
    cx = 2
    slot_delays = np.array([1300, 0, 257, 601, 1, 600], np.int32)
    stages = _haas_bank(dec, DELAYS)
    calls = _python_schedule(cx, 3)
    dev = torch.device('cuda', ctx.device)
    delays = torch.from_numpy(slot_delays).to(dev)

    def run(replayed):
        pool = dec.decorrelate_voice_pool(stages, slots=S, in_channels=cx, max_frames_per_call=M)
        assert pool.row_frames == M + MAX_DELAY and pool.latency_frames == 0 and pool.tail_frames == MAX_DELAY
        x = torch.empty((S, M, cx), dtype=torch.float32, device=dev)
        counts, flags, oc = (torch.empty(S, dtype=torch.int32, device=dev) for _ in range(3))
        y = torch.empty((S, pool.row_frames, 2), dtype=torch.int64, device=dev)
        out = (y.view(torch.float64), oc)
        pool.reset()                                                           # allocates and zeroes: before the capture
        if replayed:
            graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
            with torch.cuda.graph(graph, stream=side):
                pool.process_dev(x, counts, flags, delays, out=out)
            torch.cuda.synchronize(dev)
        results = []
        for xh, ch, fh in calls:
            x.copy_(torch.from_numpy(xh))
            counts.copy_(torch.from_numpy(ch))
            flags.copy_(torch.from_numpy(fh))
            y.fill_(POISON)
            if replayed:
                graph.replay()
            else:
                pool.process_dev(x, counts, flags, delays, out=out)
            torch.cuda.synchronize(dev)
            results.append((y.cpu().numpy(), oc.cpu().numpy()))
        with pytest.raises(RuntimeError, match='runs through process_dev'):
            pool.process({})
        return results
    plain = run(False)                                                         # first: it loads the kernels
    replay = run(True)
    pos = np.zeros(S, np.int64)
    for i, ((y0, c0), (y1, c1)) in enumerate(zip(plain, replay)):
        want, pos = haas_voice_spans(pos, calls[i][1], calls[i][2], slot_delays, MAX_DELAY, M)
        assert c0.tolist() == want.tolist() == c1.tolist(), i
        assert y0.tobytes() == y1.tobytes(), i                                 # outputs and untouched frames alike
        for b, n in enumerate(want):
            assert not (y0[b, :n] == POISON).any() and (y0[b, n:] == POISON).all(), (i, b)
    assert any(0 < n for _, c in plain for n in c)


@pytest.mark.parametrize('cx', [1, 2])
def test_dict_form_equals_decorrelate(dec, cx):
    stages = _haas_bank(dec, DELAYS)
    pool = dec.decorrelate_voice_pool(stages, slots=3, in_channels=cx, max_frames_per_call=M)
    assert pool.bank_delays.tolist() == list(DELAYS)
    a, b, c, d = (_noise((n, cx), 20 + n + cx) for n in (1000, 700, 5, 650))
    got = {name: [] for name in 'abcd'}

    def take(out, **slots):
        assert sorted(out) == sorted(slots.values()), (out.keys(), slots)
        for name, slot in slots.items():
            assert out[slot].dtype == np.float64 and out[slot].ndim == 2 and out[slot].shape[1] == 2
            got[name].append(out[slot])
    take(pool.process({0: a[:600], 1: b[:100]}, start={0: 9, 1: 3}), a=0, b=1)
    take(pool.process({0: a[600:], 2: c}, start={2: 8}, end=[2]), a=0, c=2)                 # c: a whole voice, 5 < d = 601
    take(pool.process({1: b[100:]}, end=[0]), a=0, b=1)
    take(pool.process({0: d[:300]}, start={0: 0}, end=[1]), d=0, b=1)                       # slot 0 reused, no delay now
    take(pool.process({0: d[300:]}, end=[0]), d=0)
    for name, x, t in (('a', a, 9), ('b', b, 3), ('c', c, 8), ('d', d, 0)):
        want = stages[t].decorrelate(x[:, 0] if cx == 1 else x)
        assert want.shape == (len(x) + DELAYS[t], 2)
        _same(_cat(got[name]), want, name)
    assert not pool.positions.any() and not pool.live.any()
    with pytest.raises(RuntimeError, match='runs through process\\(\\)'):
        pool.process_dev(None, None, None, None)


# ---- 9. the ABI's refusals ----------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ctx):
    from vndecorrelate_amd import _native
    cx, settings = SETTINGS['lr-ch0']
    h = Harness(ctx, cx, settings)
    delays = np.array([0, 1, 257, 600, 601, 1300], np.int32)
    x = _noise((S, 100, 2), 9)
    blocks = {b: x[b] for b in range(S)}
    counts, flags = np.full(S, 100, np.int32), np.full(S, START, np.int32)
    h.call(blocks, counts, flags, delays, 'a good call')                       # positions 100: a refusal must keep them
    flags[:] = 0
    before = h.state_words().copy()
    big = 1 << 40
    row_limit = 65535 * 256
    for override, status, text in (
            (dict(counts=0), INVALID, b'null'), (dict(flags=0), INVALID, b'null'), (dict(delays=0), INVALID, b'null'),
            (dict(x=0), INVALID, b'null'), (dict(y=0), INVALID, b'null'), (dict(out_counts=0), INVALID, b'null'),
            (dict(state=0), INVALID, b'null state'), (dict(ctx=None), INVALID, b'null context'),
            (dict(slots=-1), INVALID, b'negative'), (dict(M=-1), INVALID, b'max_frames_per_call'),
            (dict(max_delay=-1), INVALID, b'negative max_delay'),
            (dict(state_bytes=h.state_bytes - 4), INVALID, b'the Haas voice pool needs'),
            (dict(state=h.state.data_ptr() + 8), INVALID, b'16-byte aligned'),
            (dict(cx=3), INVALID, b'mono or stereo'), (dict(cx=0), INVALID, b'mono or stereo'),
            (dict(delayed_channel=2), INVALID, b'delayed_channel'), (dict(delayed_channel=-1), INVALID, b'delayed_channel'),
            (dict(slots=65536, state_bytes=big), UNSUPPORTED, b'split the pool'),
            (dict(M=row_limit - MAX_DELAY + 1, state_bytes=big), UNSUPPORTED, b'one grid dimension')):
        rc, oc, yh = h.raw(blocks, counts, flags, delays, override)
        message = h.lib.vnd_last_error()
        assert rc == status and text in message, (override, rc, message)
        assert (yh == POISON).all() and (oc == SENTINEL32).all(), override
        assert h.state_words().tobytes() == before.tobytes(), override
    # the reset and the query check the same pool
    need = ctypes.c_int64(-1)
    lib = h.lib
    assert lib.vnd_haas_voice_stream_state_bytes(S, 3, MAX_DELAY, M, ctypes.byref(need)) == INVALID and need.value == 0
    assert lib.vnd_haas_voice_stream_state_bytes(65536, 2, MAX_DELAY, M, ctypes.byref(need)) == UNSUPPORTED
    assert lib.vnd_haas_voice_stream_state_bytes(S, 2, MAX_DELAY, row_limit - MAX_DELAY + 1, ctypes.byref(need)) == UNSUPPORTED
    assert lib.vnd_haas_voice_stream_state_bytes(S, 2, MAX_DELAY, row_limit - MAX_DELAY, ctypes.byref(need)) == 0
    assert need.value == h.pos_bytes + S * row_limit * 2 * 4
    rc = lib.vnd_haas_voice_stream_reset_dev(ctx.handle, ctypes.c_void_p(h.state.data_ptr()), h.state_bytes - 4, S, 2,
                                             MAX_DELAY, M, ctypes.c_void_p(h.stream))
    assert rc == INVALID and b'the Haas voice pool needs' in lib.vnd_last_error()
    assert h.state_words().tobytes() == before.tobytes()
    # the host entry names the slot of a bad count or delay and writes nothing
    y = np.full((S, M + MAX_DELAY, 2), 7.0, np.float64)
    xh = np.zeros((S, M, 2), np.float32)
    for c, d, text in ((M + 1, 0, rf'count {M + 1} of slot 3 is outside \[0, {M}\]'), (-1, 0, 'count -1 of slot 3'),
                       (10, MAX_DELAY + 1, rf'delay {MAX_DELAY + 1} of slot 3 is outside \[0, {MAX_DELAY}\]'),
                       (10, -1, 'delay -1 of slot 3')):
        bad_c, bad_d = np.full(S, 10, np.int32), delays.copy()
        bad_c[3], bad_d[3] = c, d
        with pytest.raises(ValueError, match=text):
            _native.haas_voice_stream_host(ctx, h.state.data_ptr(), h.state_bytes, M, xh, bad_c, flags, bad_d, y,
                                           max_delay=MAX_DELAY, **settings)
        assert (y == 7.0).all() and h.state_words().tobytes() == before.tobytes()
    # ... and on good values it is the device entry's call: the voices of the first call go on and end
    xh[:, :50] = x[:, :50]
    got = _native.haas_voice_stream_host(ctx, h.state.data_ptr(), h.state_bytes, M, xh, np.full(S, 50, np.int32),
                                         np.full(S, END, np.int32), delays, y, max_delay=MAX_DELAY, **settings)
    assert got.tolist() == (50 + delays).tolist()
    signal = np.concatenate([x, x[:, :50]], axis=1)
    for b in range(S):
        assert (y[b, got[b]:] == 7.0).all()
        _same(y[b, :got[b]].copy(), _reference(signal[b], delays[b], 2, settings)[100:], ('host entry', b))
