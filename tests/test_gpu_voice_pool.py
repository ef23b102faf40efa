"""GPU tier of the voice pool (vnd_voice_stream_f32_*, include/vnd_voice_stream.h; streaming.VoicePool): slots over a bank
of velvet-noise filters whose voices start, end and bring their own block sizes call by call, the position of every slot
in the device state.  Every comparison is bit for bit.

The C ABI runs through the poisoned harness of test_gpu_each_stream.py: the ring starts as NaN and is never cleared (the
positions start as NaN bits too, and vnd_voice_stream_reset_dev zeroes them alone), the chunk rows are NaN past
counts[b], y is prefilled with a NaN no arithmetic produces and ends in a sentinel tail.  After each call out_counts is
streaming.voice_spans', every frame below out_counts[b] was written, every frame at or past it was not, and the tail is
intact.  The filter is that file's small one (16 kHz, 0.02 s, 15 taps, H <= 319, 5 tables); S = 6 and M = 600, so a row
of M + H frames spans two 512-frame tiles.  A voice's concatenated outputs equal the C oracle on its whole signal with
its own table alone, then encode_side and apply_stereo_width (O.decorrelate's order).

test_every_form runs all 24 voice_stream_kernel instantiations on pools of M = 2100 frames sized from the CU count, past
one advance group, each naming its plan through vnd_describe_voice_stream_launch.  The planted-position tests put a slot
at a position a long-lived voice reaches (2^31 .. 2^60) by the state layout the header documents - the int64 positions
first, then the ring, slot = absolute frame mod capacity - without pushing that many frames."""
import ctypes

import numpy as np
import pytest

from oracle import vnd_oracle as O
from test_gpu_each_stream import (KAPPAS, POISON, SENTINEL, TABLES, Bank, Poisoned, _function_bank, _members, _noise, _same,
                                  _velvets)

pytestmark = pytest.mark.gpu

S, M = 6, 600
TAIL = 1024                  # int32 words of sentinel behind the last row
START, END = 1, 2
INVALID, UNSUPPORTED = 1, 4
NAN_BITS = 0x7FC00000        # the ring's and the positions' first contents
BIG_M = 2100                 # test_every_form: a steady-state call is 2 tiles at r = 4, 3 at r = 2 and 5 at r = 1
MAX_POSITION = 1 << 60       # the largest position a call accepts (include/vnd_voice_stream.h)


@pytest.fixture(scope='module')
def ctx():
    from vndecorrelate_amd import _native
    context = _native.default_context()
    assert 'gfx950' in context.info()['name']
    return context


@pytest.fixture(scope='module')
def bank(ctx):
    b = Bank.of_members(ctx, _members(O.DEFAULT_ENVELOPE, (0,)))
    assert 200 < b.H <= 319 and (M + b.H) > 512                     # a row spans two tiles of the smallest kernel
    yield b
    b.close()


@pytest.fixture
def dec(ctx):
    import vndecorrelate_amd.decorrelation as decorrelation
    decorrelation.set_each_device(False)
    yield decorrelation
    decorrelation.set_each_device(None)
    decorrelation.set_device_epilogue(None)


@pytest.fixture(scope='module')
def function_bank(ctx):
    """test_gpu_each_stream.py's function-path bank: 3 tables whose weights carry the gains, so not +-1."""
    b = _function_bank(ctx)
    assert 200 < b.H <= 319
    yield b
    b.close()


_REFERENCES = {}


def _reference_key(bank, x, table, cx, epi):
    return (id(bank), x.tobytes(), int(table), cx, epi)


def _reference(bank, x, table, cx, epi):
    """One voice alone through its table by the C oracle: computed once per signal and form."""
    key = _reference_key(bank, x, table, cx, epi)
    if key not in _REFERENCES:
        _REFERENCES[key] = bank.reference(x[None], np.array([table], np.int32), cx, epi)[0]
    return _REFERENCES[key]


def _batch_references(bank, plan, cx, epi):
    """_reference for every voice of a large plan, one oracle call per (table, length); returns the keys it filled."""
    groups = {}
    for voices in plan.values():
        for v in voices:
            groups.setdefault((v.table, len(v.x)), []).append(v)
    keys = []
    for (table, _), voices in groups.items():
        want = bank.reference(np.stack([v.x for v in voices]), np.full(len(voices), table, np.int32), cx, epi)
        for v, w in zip(voices, want):
            keys.append(_reference_key(bank, v.x, table, cx, epi))
            _REFERENCES[keys[-1]] = w.copy()
    return keys


class Harness:
    """One pool's poisoned state and buffers, the host's mirror of the positions, and the calls of
    vnd_voice_stream_f32_dev on them."""

    def __init__(self, bank, cx, epi, slots=S, max_frames=M):
        import torch
        from vndecorrelate_amd import _native
        self.torch, self.bank, self.ctx, self.lib = torch, bank, bank.ctx, bank.ctx._lib
        self.S, self.M, self.H, self.cx = slots, max_frames, bank.H, cx
        self.ms, self.width = epi
        self.dev = torch.device('cuda', self.ctx.device)
        self.pos_bytes = (slots * 8 + 15) & ~15
        self.state_bytes = _native.voice_stream_state_bytes(bank.table, slots, cx, max_frames)
        assert self.state_bytes == self.pos_bytes + slots * (self.H + max_frames) * cx * 4
        self.state = torch.full((self.state_bytes // 4,), float('nan'), dtype=torch.float32, device=self.dev)
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream
        _native.voice_stream_reset_device(self.ctx, bank.table, self.state.data_ptr(), self.state_bytes, slots, cx, max_frames,
                                          stream=self.stream)
        words = self.state_words()
        assert not words[:self.pos_bytes // 4].any(), 'the reset leaves positions that are not 0'
        assert (words[self.pos_bytes // 4:] == NAN_BITS).all(), 'the reset cleared the ring'
        self.rows = max_frames + self.H
        self.body = slots * self.rows * 2
        self.x = torch.empty((slots, max_frames, cx), dtype=torch.float32, device=self.dev)
        self.y = torch.empty((self.body + TAIL,), dtype=torch.int32, device=self.dev)
        self.ints = torch.empty((3, slots), dtype=torch.int32, device=self.dev)           # counts, flags, tables
        self.out_counts = torch.empty((slots + 8,), dtype=torch.int32, device=self.dev)
        self.mirror = np.zeros(slots, np.int64)

    def state_words(self):
        return self.state.view(self.torch.int32).cpu().numpy()

    def positions(self):
        return self.state[:self.pos_bytes // 4].view(self.torch.int64).cpu().numpy()[:self.S].copy()

    def ring(self):
        """The ring as int32 words, (S, H + M, cx)."""
        return self.state_words()[self.pos_bytes // 4:].reshape(self.S, self.H + self.M, self.cx)

    def plant(self, slot, position, history):
        """Put `slot` at `position` as the header lays the state out: the int64 position, and the H frames below it -
        `history`, absolute frames [position - H, position) - each in ring slot (absolute frame mod capacity).  Every
        other word of the slot's ring stays NaN."""
        torch, H, cap = self.torch, self.H, self.H + self.M
        assert history.shape == (H, self.cx) and history.dtype == np.float32
        ring = self.state[self.pos_bytes // 4:].view(self.S, cap, self.cx)
        where = np.array([(position - H + j) % cap for j in range(H)], np.int64)        # Python integers: no wrap
        ring[slot, torch.from_numpy(where).to(self.dev)] = torch.from_numpy(history).to(self.dev)
        self.state[:self.pos_bytes // 4].view(torch.int64)[slot] = position
        self.mirror[slot] = position
        assert int(self.positions()[slot]) == position

    def raw(self, blocks, counts, flags, tables, override=None):
        """One call on poisoned buffers: (status, out_counts, y as int32 (S, M + H, 2)); the tail is checked here."""
        torch = self.torch
        xh = np.full((self.S, self.M, self.cx), np.nan, np.float32)                       # NaN past counts[b]: never read
        for slot, block in blocks.items():
            xh[slot, :len(block)] = block
        self.x.copy_(torch.from_numpy(xh))
        self.ints.copy_(torch.from_numpy(np.stack([counts, flags, tables]).astype(np.int32)))
        self.y[:self.body] = POISON
        self.y[self.body:] = SENTINEL
        self.out_counts[:] = SENTINEL
        a = dict(bank=self.bank.table.handle, state=self.state.data_ptr(), state_bytes=self.state_bytes, M=self.M,
                 x=self.x.data_ptr(), counts=self.ints[0].data_ptr(), flags=self.ints[1].data_ptr(),
                 tables=self.ints[2].data_ptr(), y=self.y.data_ptr(), out_counts=self.out_counts.data_ptr(), slots=self.S,
                 cx=self.cx, mode=0)
        a.update(override or {})
        rc = self.lib.vnd_voice_stream_f32_dev(
            self.ctx.handle, a['bank'], ctypes.c_void_p(a['state']), a['state_bytes'], a['M'], ctypes.c_void_p(a['x']),
            ctypes.c_void_p(a['counts']), ctypes.c_void_p(a['flags']), ctypes.c_void_p(a['tables']), ctypes.c_void_p(a['y']),
            ctypes.c_void_p(a['out_counts']), a['slots'], a['cx'], a['mode'], int(self.ms), int(self.width is not None),
            float(self.width or 0.0), ctypes.c_void_p(self.stream))
        yh, oc = self.y.cpu().numpy(), self.out_counts.cpu().numpy()
        assert (yh[self.body:] == SENTINEL).all(), 'the call wrote behind the last row'
        assert (oc[self.S:] == SENTINEL).all(), 'the call wrote behind out_counts'
        return rc, oc[:self.S].copy(), yh[:self.body].reshape(self.S, self.rows, 2)

    def call(self, blocks, counts, flags, tables, where=''):
        """A call that must succeed, held to voice_spans and to its footprint: the rows as float32, one per slot."""
        from vndecorrelate_amd.streaming import voice_spans
        rc, oc, yh = self.raw(blocks, counts, flags, tables)
        assert rc == 0, self.lib.vnd_last_error()
        want, self.mirror = voice_spans(self.mirror, counts, flags, self.H, self.M)
        assert oc.tolist() == want.tolist(), (where, counts, flags)
        assert self.positions().tolist() == self.mirror.tolist(), f'{where}: the positions on the device are not the mirror\'s'
        rows = []
        for b, n in enumerate(np.maximum(want, 0)):
            hole = np.argwhere(yh[b, :n] == POISON)
            assert not len(hole), f'{where}: slot {b} left (frame, channel) {tuple(hole[0])} of its {n} frames unwritten'
            assert (yh[b, n:] == POISON).all(), f'{where}: slot {b} wrote at or past its {n} frames'
            rows.append(yh[b, :n].view(np.float32).copy())
        return rows


class Voice:
    def __init__(self, x, table, start_call=0, *, end_with_last=True, whole=False, discard_after=None):
        self.x, self.table, self.start_call = x, int(table), start_call
        self.end_with_last, self.whole, self.discard_after = end_with_last, whole, discard_after
        self.pushed, self.done, self.out = 0, False, []

    def result(self):
        return np.concatenate(self.out) if self.out else np.zeros((0, 2), np.float32)


def _drive(h, plan, rng, hook=None):
    """Run the voices of `plan` ({slot: [Voice, ...]}, in order) through the pool on counts drawn from [0, M], zeros
    included.  A voice with discard_after is never ended: the next voice of its slot STARTs over it."""
    queue = {slot: list(voices) for slot, voices in plan.items()}
    active = {slot: None for slot in range(h.S)}
    tables = np.zeros(h.S, np.int32)
    call = 0
    while any(queue.values()) or any(v is not None for v in active.values()):
        assert call < 200
        blocks, counts, flags = {}, np.zeros(h.S, np.int32), np.zeros(h.S, np.int32)
        for slot in range(h.S):
            v, force = active[slot], False
            if v is not None and v.discard_after is not None and v.pushed >= v.discard_after:
                v, active[slot], force = None, None, True                      # dropped, unflushed
            if v is None and queue.get(slot) and (force or queue[slot][0].start_call <= call):
                v = active[slot] = queue[slot].pop(0)
                flags[slot] |= START
                tables[slot] = v.table
            if v is None:
                continue
            limit = (len(v.x) if v.discard_after is None else v.discard_after) - v.pushed
            n = limit if v.whole else min(limit, 0 if rng.random() < 0.3 else int(rng.integers(1, h.M + 1)))
            if n:
                blocks[slot] = v.x[v.pushed:v.pushed + n]
            counts[slot] = n
            v.pushed += n
            if v.discard_after is None and v.pushed == len(v.x):
                if v.end_with_last or v.done:
                    flags[slot] |= END
                v.done = True                                                  # (else END comes alone, with n = 0)
        if hook is not None:
            hook(call, blocks, counts, flags, tables)
        rows = h.call(blocks, counts, flags, tables.copy(), where=f'call {call}')
        for slot, v in active.items():
            if v is not None:
                v.out.append(rows[slot])
                if flags[slot] & END:
                    active[slot] = None
        call += 1
    return call


def _ragged_plan(cx, seed):
    """Voices of 1, 200 (shorter than H), 511, 513, 1300 and 2049 frames that start on different calls; slot 0 is reused
    after END by a second voice with another table; slot 5's first voice is discarded by a START without END."""
    sig = lambda n, k: _noise((n, cx), seed + k)
    return {0: [Voice(sig(1, 0), 0, 0, whole=True), Voice(sig(700, 1), 3, 4, end_with_last=False)],
            1: [Voice(sig(200, 2), 1, 1, end_with_last=False)],
            2: [Voice(sig(511, 3), 2, 0)],
            3: [Voice(sig(513, 4), 3, 2, end_with_last=False)],
            4: [Voice(sig(1300, 5), 4, 3)],
            5: [Voice(sig(900, 6), 1, 1, discard_after=450), Voice(sig(2049, 7), 2, 0)]}


def _check_voices(bank, plan, cx, epi):
    for slot, voices in plan.items():
        for i, v in enumerate(voices):
            want = _reference(bank, v.x, v.table, cx, epi)
            got = v.result()
            if v.discard_after is None:
                _same(got, want, ('slot', slot, 'voice', i))
            else:                                           # what it returned before it was dropped is final all the same
                assert len(got) == max(0, v.discard_after - bank.H)
                _same(got, want[:len(got)], ('slot', slot, 'discarded voice', i))


# ---- 1. a ragged schedule, and the footprint of every call ------------------------------------------------------------
@pytest.mark.parametrize('cx, epi', [(2, (False, None)), (2, (True, None)), (2, (True, 0.35)), (1, (True, 0.35))],
                         ids=['plain', 'ms_encode', 'ms_encode-width', 'mono-in'])
def test_ragged_schedule(bank, cx, epi):
    plan = _ragged_plan(cx, 100 * cx)
    h = Harness(bank, cx, epi)
    calls = _drive(h, plan, np.random.default_rng(7 + cx))
    assert calls > 8
    _check_voices(bank, plan, cx, epi)
    assert not h.positions().any() and not h.mirror.any()           # every voice ended: every slot is back at 0
    # the voice that follows the discarded one: nothing of it, and no NaN from the ring
    assert not np.isnan(plan[5][1].result()).any()
    # ... and the ring was written by the calls alone: still NaN where no voice reached (slot 1 pushed 200 < H + M frames)
    ring = h.state_words()[h.pos_bytes // 4:].reshape(S, bank.H + M, cx)
    assert (ring[1, 200:] == NAN_BITS).all() and not (ring[1, :200] == NAN_BITS).any()


def test_edge_calls(bank):
    """END with n = 0 at p = 0, at p < H and at p > H; START with END in one call; START alone with n = 0; idle slots."""
    cx, epi = 2, (True, 0.35)
    h = Harness(bank, cx, epi)
    H = bank.H
    xs = [_noise((n, cx), 40 + n) for n in (150, H + 90, 600, 600)]
    tables = np.array([0, 1, 2, 3, 4, 0], np.int32)
    zero = np.zeros(S, np.int32)
    # call 0: slots 0..2 start and push; slot 3 is a whole voice of M frames; slot 4 starts with no frames; slot 5 is idle
    counts = np.array([150, H + 90, 600, 600, 0, 0], np.int32)
    flags = np.array([START, START, START, START | END, START, 0], np.int32)
    r0 = h.call({b: xs[b] for b in range(4)}, counts, flags, tables, 'call 0')
    assert [len(r) for r in r0] == [0, 90, 600 - H, 600, 0, 0]
    _same(r0[3], _reference(bank, xs[3], 3, cx, epi), 'a whole voice in one call')
    # call 1: END alone everywhere: p < H (slot 0), p > H (slots 1, 2), p = 0 after START (slot 4), p = 0 never started (5)
    r1 = h.call({}, zero, np.array([END, END, END, 0, END, END], np.int32), tables, 'call 1')
    assert [len(r) for r in r1] == [150, H, H, 0, 0, 0]
    for b in range(3):
        _same(np.concatenate([r0[b], r1[b]]), _reference(bank, xs[b], b, cx, epi), ('flushed', b))
    # call 2: nothing anywhere
    assert [len(r) for r in h.call({}, zero, zero, tables, 'call 2')] == [0] * S
    assert not h.positions().any()


# ---- 2. lockstep -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cx, r', [pytest.param(1, None, id='1'), pytest.param(2, None, id='2'),
                                   pytest.param(2, 2, id='2-r2'), pytest.param(2, 4, id='2-r4')])
def test_lockstep_equals_each_stream_call_by_call(ctx, bank, cx, r):
    """r None: the file's 6 slots.  r = 2, 4: test_every_form's pools, whose voice kernel takes that tile on every call
    whatever tile the lockstep sibling takes for the call's own frames."""
    epi = (True, 0.35)
    if r is None:
        slots, max_frames, sizes = S, M, [600, 0, 37, 263, 600, 1]
        tables = TABLES
    else:
        slots, max_frames, sizes = _pool_slots(ctx, r), BIG_M, [BIG_M, 0, 700, BIG_M]
        tables = (np.arange(slots) % 5).astype(np.int32)
    x = _noise((slots, sum(sizes), cx), 11 + cx + (r or 0))
    lock = Poisoned(bank, tables, cx, max_frames, epi)
    h = Harness(bank, cx, epi, slots, max_frames)
    if r is not None:
        assert _voice_plan(bank, max_frames, slots, cx, epi)['r'] == r
    xd = h.torch.from_numpy(x).to(h.dev)
    pos = 0
    for i, n in enumerate(sizes):
        final = i == len(sizes) - 1
        rc, got, yh, n_out = lock.call(xd[:, pos:pos + n].contiguous(), pos, n, final)
        assert rc == 0 and got == n_out
        want = yh[:slots * n_out * 2].reshape(slots, n_out, 2)
        flags = np.full(slots, (START if i == 0 else 0) | (END if final else 0), np.int32)
        rows = h.call({b: x[b, pos:pos + n] for b in range(slots)}, np.full(slots, n, np.int32), flags, tables, f'call {i}')
        for b in range(slots):
            assert rows[b].view(np.int32).tobytes() == want[b].tobytes(), (i, b)
        pos += n
    assert not h.positions().any()


# ---- 2b. every instantiation, on pools past one advance group --------------------------------------------------------
def _pool_slots(ctx, r):
    """make_each_stream_plan takes the largest tile that leaves every CU six workgroups: a call of BIG_M frames is 2
    tiles at r = 4 and 3 at r = 2.  The one slot more leaves a last advance group of 256 lanes with one live lane."""
    cus = ctx.info()['compute_units']
    return {4: 3 * cus + 1, 2: 2 * cus + 1, 1: 7}[r]


def _voice_plan(bank, max_frames, slots, cx, epi):
    head, *fields = bank.table.describe_voice_stream(max_frames, slots, cx, 0, epi[0] or epi[1] is not None).split()
    assert head == 'voice_stream'
    return {k: int(v) for k, v in (f.split('=') for f in fields)}


def _pool_plan(slots, cx, H, T, seed):
    """({slot: [Voice, ...]}, the slots never started).  The first seven slots hold every length the kernel can go wrong
    at - 1, below H, 511, 513, M, M + H + 1, 3 M - a slot reused after END by a voice with another table, an END alone
    with n = 0, a voice discarded by a START without END, and a slot that never starts; the slots after them draw from
    the same cases: a tenth reused, a few END alone, a few discarded, some never started, the rest one voice."""
    rng = np.random.default_rng(seed)
    sig = lambda n, k: _noise((n, cx), 100003 * seed + k)
    lengths = (1, 150, 511, 513, BIG_M, BIG_M + H + 1, 3 * BIG_M)
    assert 150 < H
    plan = {0: [Voice(sig(1, 0), 0, 0, whole=True), Voice(sig(BIG_M + H + 1, 1), 1, 2, end_with_last=False)],
            1: [Voice(sig(150, 2), 1, 1, end_with_last=False)],
            2: [Voice(sig(511, 3), 2, 0)],
            3: [Voice(sig(513, 4), 0, 2)],
            4: [Voice(sig(BIG_M, 5), 1, 1, discard_after=900), Voice(sig(3 * BIG_M, 6), 2, 0)],
            5: [Voice(sig(BIG_M, 7), T - 1, 3)]}
    never = [6]
    for slot in range(7, slots):
        u, k = rng.random(), 10 + 2 * slot
        short = int(rng.choice(lengths[:6]))                           # two voices in a slot: neither is the longest
        n = lengths[6] if rng.random() < 0.05 else short               # (the longest sets the number of calls: a few)
        table, start = int(rng.integers(T)), int(rng.integers(0, 4))
        if u < 0.08:
            never.append(slot)
        elif u < 0.18:                                                 # reused after END, by another table
            plan[slot] = [Voice(sig(short, k), table, start % 2, end_with_last=bool(rng.random() < 0.5)),
                          Voice(sig(int(rng.choice(lengths[:6])), k + 1), (table + 1) % T, 0)]
        elif u < 0.22:                                                 # discarded by the START of the next voice
            first = max(short, 511)
            plan[slot] = [Voice(sig(first, k), table, start % 2, discard_after=int(rng.integers(1, first))),
                          Voice(sig(int(rng.choice(lengths[:6])), k + 1), (table + 1) % T, 0)]
        elif u < 0.27:                                                 # END alone, with n = 0
            plan[slot] = [Voice(sig(n, k), table, start, end_with_last=False)]
        else:
            plan[slot] = [Voice(sig(n, k), table, 0 if n == lengths[-1] else start)]
    return plan, never


@pytest.mark.parametrize('epi', [(False, None), (True, 0.35)], ids=['plain', 'ms_encode-width'])
@pytest.mark.parametrize('r', [1, 2, 4])
@pytest.mark.parametrize('path', ['class', 'function'])
@pytest.mark.parametrize('cx', [1, 2])
def test_every_form(ctx, bank, function_bank, cx, path, r, epi):
    """voice_stream_kernel<cx, MODE, r, EPI> for every cx, MODE (1: the class-path bank's +-1 weights, 0: the function-path
    bank's), r and EPI, the plan named by the hook before anything runs; 3 x CUs + 1 slots reach r = 4, 2 x CUs + 1
    reach r = 2 (four and three advance groups on 256 CUs, the last with one live lane), 7 slots plan r = 1.
    (With H <= 319 a row of M + H frames has as many tiles as a call of M frames at every r: the workgroups past a
    slot's n_out are those of the calls that push less than M.)"""
    bk = bank if path == 'class' else function_bank
    slots, T = _pool_slots(ctx, r), len(bk.alone)
    plan_text = _voice_plan(bk, BIG_M, slots, cx, epi)
    want = dict(r=r, fma=int(path == 'class'), epilogue=int(epi != (False, None)), tiles=-(-(BIG_M + bk.H) // (512 * r)),
                nblocks=slots * -(-(BIG_M + bk.H) // (512 * r)), advance_groups=-(-slots // 256))
    assert {k: plan_text[k] for k in want} == want, plan_text
    assert r == 1 or want['advance_groups'] >= 3
    plan, never = _pool_plan(slots, cx, bk.H, T, 1000 * cx + 10 * r + (path == 'class'))
    keys = _batch_references(bk, plan, cx, epi)
    try:
        h = Harness(bk, cx, epi, slots, BIG_M)
        calls = _drive(h, plan, np.random.default_rng(3 + cx + r))     # every call: out_counts, footprint, positions
        assert calls >= 8, calls
        print(f'{calls} calls, {slots} slots, {sum(len(v) for v in plan.values())} voices')
        _check_voices(bk, plan, cx, epi)
        assert not h.positions().any() and not h.mirror.any()         # every voice ended
        assert (h.ring()[never] == NAN_BITS).all(), 'a slot that never started has frames in its ring'
    finally:
        for key in keys:
            _REFERENCES.pop(key, None)


# ---- 2c. positions a long-lived voice reaches ------------------------------------------------------------------------
PLANTED = (2 ** 31 - 7,        # the first block crosses 2^31
           2 ** 32 - 300,      # p - H and p straddle 2^32 inside one staged window
           2 ** 32 + 12345, 2 ** 40 + 3,
           2 ** 53 + 1,        # no float64 holds it: a detour through doubles shows
           None)               # 2^60 less the frames the slot pushes: its last call, an END alone, is at 2^60 exactly


@pytest.mark.parametrize('cx, epi', [(2, (True, 0.35)), (1, (True, 0.35))], ids=['ms_encode-width', 'mono-in'])
def test_planted_positions(bank, cx, epi):
    """No START anywhere: every slot goes on from the position and the H frames of history planted in its state.  The
    tap sum reads x[n .. n + H], so the outputs from frame P - H on are the oracle's on the signal that starts there."""
    h = Harness(bank, cx, epi)
    H = bank.H
    rng = np.random.default_rng(50 + cx)
    pushed = [int(n) for n in rng.integers(900, 1900, S)]
    sigs = [_noise((H + n, cx), 300 + 10 * cx + b) for b, n in enumerate(pushed)]
    start = [MAX_POSITION - pushed[b] if P is None else P for b, P in enumerate(PLANTED)]
    for b in range(S):
        h.plant(b, start[b], sigs[b][:H])
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
                blocks[b] = sigs[b][H + done[b]:H + done[b] + n]
            counts[b] = n
            done[b] += n
        rows = h.call(blocks, counts, flags, TABLES, f'call {call}')   # out_counts and positions against the mirror
        for b in range(S):
            outs[b].append(rows[b])
        call += 1
    assert call > 3 and not h.positions().any()
    for b in range(S):
        _same(np.concatenate(outs[b]), _reference(bank, sigs[b], TABLES[b], cx, epi), ('planted at', start[b]))


def test_a_position_above_the_range_leaves_the_slot_alone(bank):
    cx, epi = 2, (True, 0.35)
    h = Harness(bank, cx, epi)
    H = bank.H
    x = _noise((S, 1000, cx), 8)
    blocks = lambda first, n: {b: x[b, first:first + n] for b in range(S)}
    h.call(blocks(0, 400), np.full(S, 400, np.int32), np.full(S, START, np.int32), TABLES, 'call 0')
    # slot 3's position becomes 2^60 + 1 (its ring keeps the frames of call 0): without START the slot is refused
    h.state[:h.pos_bytes // 4].view(h.torch.int64)[3] = MAX_POSITION + 1
    before = h.state_words().copy()
    rc, oc, yh = h.raw(blocks(400, 600), np.full(S, 600, np.int32), np.full(S, END, np.int32), TABLES)
    assert rc == 0, h.lib.vnd_last_error()
    assert oc[3] == -1 and (yh[3] == POISON).all()
    assert int(h.positions()[3]) == MAX_POSITION + 1
    assert h.ring()[3].tobytes() == before[h.pos_bytes // 4:].reshape(S, -1)[3].tobytes()
    for b in (0, 1, 2, 4, 5):                                          # the neighbours end as if nothing had happened
        assert oc[b] == 1000 - max(0, 400 - H) and (yh[b, oc[b]:] == POISON).all()
        want = _reference(bank, x[b], TABLES[b], cx, epi)
        _same(yh[b, :oc[b]].view(np.float32), want[max(0, 400 - H):], ('beside a bad position', b))
    # the mirror answers the same -1, and the slot works again with START
    from vndecorrelate_amd.streaming import voice_spans
    h.mirror[:] = 0
    h.mirror[3] = MAX_POSITION + 1
    counts, flags = np.zeros(S, np.int32), np.zeros(S, np.int32)
    counts[3] = 500
    out, new = voice_spans(h.mirror, counts, flags, H, M)
    assert out[3] == -1 and new[3] == MAX_POSITION + 1
    flags[3] = START | END
    rows = h.call({3: x[3, :500]}, counts, flags, TABLES, 'restarted')
    _same(rows[3], _reference(bank, x[3, :500], TABLES[3], cx, epi), 'START over a bad position')
    assert not h.positions().any()


# ---- 3. bad per-slot values ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad_count', [M + 1, -1, 2 ** 31 - 1, -2 ** 31])
def test_a_bad_count_leaves_the_slot_alone(bank, bad_count):
    cx, epi = 2, (True, None)
    x = _noise((S, 1500, cx), 5)
    sizes = [500, 400, 600]

    def run(spoil):
        h = Harness(bank, cx, epi)
        outs, pos = [[] for _ in range(S)], 0
        for i, n in enumerate(sizes):
            flags = np.full(S, (START if i == 0 else 0) | (END if i == 2 else 0), np.int32)
            blocks = {b: x[b, pos:pos + n] for b in range(S)}
            if spoil and i == 1:                                               # slot 2 sends a bad count: one call lost to it
                counts = np.full(S, n, np.int32)
                counts[2] = bad_count
                before, state = h.positions(), h.state_words().copy()
                rc, oc, yh = h.raw(blocks, counts, flags, TABLES)
                assert rc == 0, h.lib.vnd_last_error()
                assert oc[2] == -1 and (yh[2] == POISON).all()                   # the row is untouched
                assert h.positions()[2] == before[2] == 500                    # the position and the ring are unchanged
                ring = lambda w: w[h.pos_bytes // 4:].reshape(S, -1)[2]
                assert ring(h.state_words()).tobytes() == ring(state).tobytes()
                for b in (0, 1, 3, 4, 5):
                    assert oc[b] == n and not (yh[b, :n] == POISON).any() and (yh[b, n:] == POISON).all()
                    outs[b].append(yh[b, :n].view(np.float32).copy())
                h.mirror += np.where(np.arange(S) == 2, 0, n)
                # the voice continues on the next call with the block it meant to push
                one = np.zeros(S, np.int32)
                one[2] = n
                rows = h.call({2: x[2, pos:pos + n]}, one, np.zeros(S, np.int32), TABLES, 'retry')
                outs[2].append(rows[2])
            else:
                rows = h.call(blocks, np.full(S, n, np.int32), flags, TABLES, f'call {i}')
                for b in range(S):
                    outs[b].append(rows[b])
            pos += n
        return [np.concatenate(o) for o in outs]
    clean, spoiled = run(False), run(True)
    for b in range(S):
        _same(clean[b], _reference(bank, x[b], TABLES[b], cx, epi), ('clean', b))
        _same(spoiled[b], clean[b], ('beside or after a bad count', b))


def test_a_bad_table_is_nan_for_that_slot_alone(bank):
    cx, epi = 2, (True, 0.35)
    x = _noise((S, 1100, cx), 6)
    sizes = [600, 500]
    for bad_value in (5, -1, 2 ** 31 - 1):
        h = Harness(bank, cx, epi)
        tables = TABLES.copy()
        tables[4] = bad_value
        outs, pos = [[] for _ in range(S)], 0
        for i, n in enumerate(sizes):
            flags = np.full(S, (START if i == 0 else 0) | (END if i == 1 else 0), np.int32)
            rows = h.call({b: x[b, pos:pos + n] for b in range(S)}, np.full(S, n, np.int32), flags, tables, f'call {i}')
            if i == 0:
                assert h.positions()[4] == 600                                 # the position still advances
            for b in range(S):
                outs[b].append(rows[b])
            pos += n
        for b in range(S):
            got = np.concatenate(outs[b])
            if b == 4:
                assert got.shape == (1100, 2) and np.isnan(got).all(), bad_value
            else:
                _same(got, _reference(bank, x[b], TABLES[b], cx, epi), (bad_value, b))


# ---- 4. graph replay and the Python forms ----------------------------------------------------------------------------
def _python_schedule(cx, seed):
    """A ragged schedule as process_dev arrays: 8 calls of (blocks, counts, flags) over 6 slots, with a START and an END
    inside, a reused slot and idle calls; tables are fixed per slot (the reused slot keeps its table)."""
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
            flags[5] = START | END                                             # a whole voice
        if i == 4:
            flags[1] = START                                                   # the slot reused
            flags[0] = END
            counts[0] = 0
        if i == 7:
            flags[:] |= END
        x = rng.uniform(-1, 1, (S, M, cx)).astype(np.float32)
        calls.append((x, counts, flags))
    return calls


def test_graph_replay_equals_the_uncaptured_run(dec, ctx):
    import torch
    cx = 2
    stages = _velvets(dec, sorted(set(KAPPAS)), mode='LR', width=0.35)
    calls = _python_schedule(cx, 3)
    dev = torch.device('cuda', ctx.device)
    tables = torch.from_numpy(TABLES.copy()).to(dev)

    def run(replayed):
        pool = dec.decorrelate_voice_pool(stages, slots=S, in_channels=cx, max_frames_per_call=M)
        x = torch.empty((S, M, cx), dtype=torch.float32, device=dev)
        counts, flags, oc = (torch.empty(S, dtype=torch.int32, device=dev) for _ in range(3))
        y = torch.empty((S, pool.row_frames, 2), dtype=torch.int32, device=dev)
        out = (y.view(torch.float32), oc)
        pool.reset()                                                           # allocates and zeroes: before the capture
        if replayed:
            graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
            with torch.cuda.graph(graph, stream=side):
                pool.process_dev(x, counts, flags, tables, out=out)
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
                pool.process_dev(x, counts, flags, tables, out=out)
            torch.cuda.synchronize(dev)
            results.append((y.cpu().numpy(), oc.cpu().numpy()))
        with pytest.raises(RuntimeError, match='runs through process_dev'):
            pool.process({})
        return pool, results
    pool, plain = run(False)                                                   # first: it loads the kernels
    _, replay = run(True)
    from vndecorrelate_amd.streaming import voice_spans
    pos = np.zeros(S, np.int64)
    for i, ((y0, c0), (y1, c1)) in enumerate(zip(plain, replay)):
        want, pos = voice_spans(pos, calls[i][1], calls[i][2], pool.latency_frames, M)
        assert c0.tolist() == want.tolist() == c1.tolist(), i
        assert y0.tobytes() == y1.tobytes(), i                                 # outputs and untouched frames alike
        for b, n in enumerate(want):
            assert not (y0[b, :n] == POISON).any() and (y0[b, n:] == POISON).all(), (i, b)
    assert any(0 < n for _, c in plain for n in c)


@pytest.mark.parametrize('cx', [1, 2])
def test_dict_form_equals_decorrelate(dec, cx):
    stages = _velvets(dec, KAPPAS)                                             # 6 bank entries over 5 tables
    pool = dec.decorrelate_voice_pool(stages, slots=3, in_channels=cx, max_frames_per_call=M)
    assert pool.bank_tables.tolist() == TABLES.tolist() and 200 < pool.latency_frames <= 319
    a, b, c, d = (_noise((n, cx), 20 + n + cx) for n in (1000, 700, 513, 650))
    got = {name: [] for name in 'abcd'}

    def take(out, **slots):
        assert sorted(out) == sorted(slots.values()), (out.keys(), slots)
        for name, slot in slots.items():
            assert out[slot].dtype == np.float32 and out[slot].ndim == 2 and out[slot].shape[1] == 2
            got[name].append(out[slot])
    take(pool.process({0: a[:600], 1: b[:100]}, start={0: 2, 1: 3}), a=0, b=1)
    take(pool.process({0: a[600:], 2: c}, start={2: 5}, end=[2]), a=0, c=2)                 # c: a whole voice
    take(pool.process({1: b[100:]}, end=[0]), a=0, b=1)
    take(pool.process({0: d[:300]}, start={0: 0}, end=[1]), d=0, b=1)                       # slot 0 reused, another table
    take(pool.process({0: d[300:]}, end=[0]), d=0)
    for name, x, t in (('a', a, 2), ('b', b, 3), ('c', c, 5), ('d', d, 0)):
        want = stages[t].decorrelate(x[:, 0] if cx == 1 else x)
        _same(np.concatenate(got[name]), want, name)
    assert not pool.positions.any() and not pool.live.any()
    with pytest.raises(RuntimeError, match='runs through process\\(\\)'):
        pool.process_dev(None, None, None, None)
    # after reset() the other form may follow, and the slot's old frames do not show
    import torch
    pool.reset()
    dev = torch.device('cuda', pool._state[0].device.index)
    x = torch.zeros((3, M, cx), device=dev)
    x[1, :513] = torch.from_numpy(c).to(dev)
    counts = torch.tensor([0, 513, 0], dtype=torch.int32, device=dev)
    flags = torch.tensor([0, START | END, 0], dtype=torch.int32, device=dev)
    tables = torch.tensor([0, int(pool.bank_tables[5]), 0], dtype=torch.int32, device=dev)
    y, oc = pool.process_dev(x, counts, flags, tables)
    assert oc.tolist() == [0, 513, 0]
    _same(y[1, :513].cpu().numpy(), np.concatenate(got['c']), 'process_dev after reset')


# ---- 5. the ABI's refusals -------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ctx, bank):
    from vndecorrelate_amd import _native
    from vndecorrelate_amd.taps import class_path_bank_arrays, function_path_arrays
    h = Harness(bank, 2, (True, None))
    x = _noise((S, 100, 2), 9)
    blocks = {b: x[b] for b in range(S)}
    counts, flags = np.full(S, 100, np.int32), np.full(S, START, np.int32)
    h.call(blocks, counts, flags, TABLES, 'a good call')                       # positions 100: a refusal must keep them
    flags[:] = 0
    env = tuple(O.DEFAULT_ENVELOPE)
    far = class_path_bank_arrays([([[([7], [0, 4095])], None], env, True)])
    long_bank = _native.TapTable.create(ctx, far.tap_offsets, far.tap_index, far.tap_weight, **far.kwargs())
    fir = O.generate_velvet_noise(duration_seconds=0.02, num_impulses=15, num_outs=2, sample_rate_hz=16000, seed=3)
    arr = function_path_arrays(fir)
    weights = arr.tap_weight.copy()
    weights[0] = np.inf
    inf_bank = _native.TapTable.create(ctx, arr.tap_offsets, arr.tap_index, weights)
    odd = function_path_arrays(fir[:, :1])
    odd_bank = _native.TapTable.create(ctx, odd.tap_offsets, odd.tap_index, odd.tap_weight)
    try:
        before = h.state_words().copy()
        big = 1 << 40
        for override, status, text in (
                (dict(counts=0), INVALID, b'null'), (dict(flags=0), INVALID, b'null'), (dict(tables=0), INVALID, b'null'),
                (dict(x=0), INVALID, b'null'), (dict(y=0), INVALID, b'null'), (dict(out_counts=0), INVALID, b'null'),
                (dict(state=0), INVALID, b'null state'), (dict(bank=None), INVALID, b'null context or tap table'),
                (dict(slots=-1), INVALID, b'negative slots'), (dict(M=-1), INVALID, b'max_frames_per_call'),
                (dict(state_bytes=h.state_bytes - 4), INVALID, b'the voice pool needs'),
                (dict(state=h.state.data_ptr() + 8), INVALID, b'16-byte aligned'),
                (dict(cx=3), INVALID, b'mono or stereo'), (dict(cx=0), INVALID, b'mono or stereo'),
                (dict(bank=odd_bank.handle), INVALID, b'stereo pairs'),
                (dict(mode=1), UNSUPPORTED, b'VND_MODE_EXACT only'), (dict(mode=2), UNSUPPORTED, b'VND_MODE_EXACT only'),
                (dict(slots=65536, state_bytes=big), UNSUPPORTED, b'split the pool'),
                (dict(bank=long_bank.handle, state_bytes=big), UNSUPPORTED, b'4095'),
                (dict(bank=inf_bank.handle, state_bytes=big), UNSUPPORTED, b'not finite')):
            rc, oc, yh = h.raw(blocks, counts, flags, TABLES, override)
            message = h.lib.vnd_last_error()
            assert rc == status and text in message, (override, rc, message)
            assert (yh == POISON).all() and (oc == SENTINEL).all(), override
            assert h.state_words().tobytes() == before.tobytes(), override
        # the reset and the query check the same pool
        need = ctypes.c_int64(-1)
        assert h.lib.vnd_voice_stream_state_bytes(bank.table.handle, S, 3, M, ctypes.byref(need)) == INVALID and need.value == 0
        assert h.lib.vnd_voice_stream_state_bytes(bank.table.handle, 65536, 2, M, ctypes.byref(need)) == UNSUPPORTED
        assert h.lib.vnd_voice_stream_state_bytes(bank.table.handle, S, 2, (1 << 24) + 1, ctypes.byref(need)) == UNSUPPORTED
        rc = h.lib.vnd_voice_stream_reset_dev(ctx.handle, ctypes.c_void_p(h.state.data_ptr()), h.state_bytes - 4, S, 2,
                                              bank.table.handle, M, ctypes.c_void_p(h.stream))
        assert rc == INVALID and b'the voice pool needs' in h.lib.vnd_last_error()
        assert h.state_words().tobytes() == before.tobytes()
        # the host entry names the slot of a bad count or table and writes nothing
        y = np.full((S, M + bank.H, 2), 7.0, np.float32)
        xh = np.zeros((S, M, 2), np.float32)
        for c, t, text in ((M + 1, 0, rf'count {M + 1} of slot 3 is outside \[0, {M}\]'), (-1, 0, 'count -1 of slot 3'),
                           (10, 5, r'table 5 of slot 3 is outside \[0, 5\)'), (10, -1, 'table -1 of slot 3')):
            bad_c, bad_t = np.full(S, 10, np.int32), TABLES.copy()
            bad_c[3], bad_t[3] = c, t
            with pytest.raises(ValueError, match=text):
                _native.voice_stream_host(ctx, bank.table, h.state.data_ptr(), h.state_bytes, M, xh, bad_c, flags, bad_t, y,
                                          ms_encode=True, width=None)
            assert (y == 7.0).all() and h.state_words().tobytes() == before.tobytes()
        # ... and on good values it is the device entry's call: the voices of the first call go on and end
        xh[:, :50] = x[:, :50]
        got = _native.voice_stream_host(ctx, bank.table, h.state.data_ptr(), h.state_bytes, M, xh, np.full(S, 50, np.int32),
                                        np.full(S, END, np.int32), TABLES, y, ms_encode=True, width=None)
        assert got.tolist() == [150] * S and (y[:, 150:] == 7.0).all()
        signal = np.concatenate([x, x[:, :50]], axis=1)
        for b in range(S):
            _same(y[b, :150], _reference(bank, signal[b], TABLES[b], 2, (True, None)), ('host entry', b))
    finally:
        long_bank.close()
        inf_bank.close()
        odd_bank.close()
