"""GPU tier of the crossfading voice pool (vnd_voice_fade_stream_f32_dev, include/vnd_voice_fade_stream.h;
streaming.FadeVoicePool): the voice pool whose live voices change their filter.  Every comparison is of bytes.

The C ABI runs through the poisoned harness of test_gpu_voice_pool.py with the pool's own state layout - positions,
records, ring, all NaN bits before the reset, which zeroes the positions alone - and a fifth output, fade_left, behind a
sentinel tail of its own.  After every call out_counts, fade_left, the positions and the records on the device equal
streaming.voice_fade_spans', every frame below out_counts[b] was written and none at or past it.  The bank is that
file's (16 kHz, 15 taps, H <= 319, 5 tables), S = 6 and M = 600: a row spans two 512-frame tiles.

The reference is the C oracle's plain convolution of a voice's whole signal with each table alone, blended in NumPy float32
by voice_fade_cases.blend from the switches the header's block - restated in Python integers there - accepts, then
O.encode_side / O.apply_stereo_width in O.decorrelate's order."""
import ctypes

import numpy as np
import pytest

from oracle import vnd_oracle as O
from test_gpu_each_stream import KAPPAS, POISON, SENTINEL, TABLES, Bank, _noise, _same, _taps, _velvets
from test_gpu_voice_pool import (BIG_M, INVALID, M, NAN_BITS, S, TAIL, UNSUPPORTED, Harness, Voice, _drive, _pool_slots,
                                 _ragged_plan, bank, ctx, dec, function_bank)  # noqa: F401  (fixtures)
from voice_fade_cases import END, RAGGED, START, SWITCH, bank_latency, blend, ragged_schedule

pytestmark = pytest.mark.gpu

PLAIN, MS_WIDTH = (False, None), (True, 0.35)


def _gains(F, fade='linear'):
    from vndecorrelate_amd.streaming import fade_gains
    return fade_gains(F, fade)


class FadeHarness(Harness):
    """test_gpu_voice_pool.Harness on vnd_voice_fade_stream_f32_dev: the records between positions and ring, the gains,
    fade_left, the mirror of all of it, and per slot the voices the calls began with the switches that were accepted."""

    def __init__(self, bank, cx, epi, F, gains=None, slots=S, max_frames=M):
        import torch
        from vndecorrelate_amd import _native_fade
        self.torch, self.bank, self.ctx, self.lib = torch, bank, bank.ctx, bank.ctx._lib
        self.S, self.M, self.H, self.cx, self.F = slots, max_frames, bank.H, cx, F
        self.ms, self.width = epi
        self.dev = torch.device('cuda', self.ctx.device)
        self.pos_bytes = (slots * 8 + 15) & ~15
        self.rec_bytes = 16 * slots
        self.state_bytes = _native_fade.voice_fade_stream_state_bytes(bank.table, slots, cx, max_frames, F)
        assert self.state_bytes == self.pos_bytes + self.rec_bytes + slots * (self.H + max_frames) * cx * 4
        self.state = torch.full((self.state_bytes // 4,), float('nan'), dtype=torch.float32, device=self.dev)
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream
        _native_fade.voice_fade_stream_reset_device(self.ctx, bank.table, self.state.data_ptr(), self.state_bytes, slots, cx,
                                                    max_frames, F, stream=self.stream)
        words = self.state_words()
        assert not words[:self.pos_bytes // 4].any(), 'the reset leaves positions that are not 0'
        assert (words[self.pos_bytes // 4:] == NAN_BITS).all(), 'the reset cleared the records or the ring'
        self.gains_host = _gains(F) if gains is None else gains
        self.gains = torch.from_numpy(self.gains_host).to(self.dev) if F else None
        self.rows = max_frames + self.H
        self.body = slots * self.rows * 2
        self.x = torch.empty((slots, max_frames, cx), dtype=torch.float32, device=self.dev)
        self.y = torch.empty((self.body + TAIL,), dtype=torch.int32, device=self.dev)
        self.ints = torch.empty((3, slots), dtype=torch.int32, device=self.dev)           # counts, flags, tables
        self.out_counts = torch.empty((slots + 8,), dtype=torch.int32, device=self.dev)
        self.fade_left = torch.empty((slots + 8,), dtype=torch.int32, device=self.dev)
        self.mirror = np.zeros(slots, np.int64)
        self.mirror_records = self.records()
        self.mirror_left = np.zeros(slots, np.int64)
        self.lives = [[] for _ in range(slots)]                       # per slot: dict(table, fades, open, started)

    def records(self):
        """The records on the device as int64 (S, 3): s, old, cur."""
        words = self.state[self.pos_bytes // 4:(self.pos_bytes + self.rec_bytes) // 4].view(self.torch.int32).cpu().numpy()
        words = words.reshape(self.S, 4)
        s = words[:, :2].copy().view(np.int64)[:, 0]
        return np.stack([s, words[:, 2].astype(np.int64), words[:, 3].astype(np.int64)], axis=1)

    def ring(self):
        return self.state_words()[(self.pos_bytes + self.rec_bytes) // 4:].reshape(self.S, self.H + self.M, self.cx)

    def plant(self, slot, position, history, record):
        """Harness.plant, by this pool's layout, with the slot's record (s, old, cur)."""
        torch, H, cap = self.torch, self.H, self.H + self.M
        assert history.shape == (H, self.cx) and history.dtype == np.float32
        ring = self.state[(self.pos_bytes + self.rec_bytes) // 4:].view(self.S, cap, self.cx)
        where = np.array([(position - H + j) % cap for j in range(H)], np.int64)        # Python integers: no wrap
        ring[slot, torch.from_numpy(where).to(self.dev)] = torch.from_numpy(history).to(self.dev)
        self.state[:self.pos_bytes // 4].view(torch.int64)[slot] = position
        rec = self.state[self.pos_bytes // 4:(self.pos_bytes + self.rec_bytes) // 4].view(torch.int32).view(self.S, 4)
        rec[slot, :2] = torch.from_numpy(np.array([record[0]], np.int64).view(np.int32)).to(self.dev)
        rec[slot, 2], rec[slot, 3] = int(record[1]), int(record[2])
        self.mirror[slot] = position
        self.mirror_records[slot] = record
        self.lives[slot].append(dict(table=int(record[2]), fades=[], open=True, started=True))
        assert int(self.positions()[slot]) == position and self.records()[slot].tolist() == list(record)

    def raw(self, blocks, counts, flags, tables, override=None):
        """One call on poisoned buffers: (status, out_counts, y as int32 (S, M + H, 2), fade_left)."""
        torch = self.torch
        xh = np.full((self.S, self.M, self.cx), np.nan, np.float32)                       # NaN past counts[b]: never read
        for slot, block in blocks.items():
            xh[slot, :len(block)] = block
        self.x.copy_(torch.from_numpy(xh))
        self.ints.copy_(torch.from_numpy(np.stack([counts, flags, tables]).astype(np.int32)))
        self.y[:self.body] = POISON
        self.y[self.body:] = SENTINEL
        self.out_counts[:] = SENTINEL
        self.fade_left[:] = SENTINEL
        a = dict(ctx=self.ctx.handle, bank=self.bank.table.handle, state=self.state.data_ptr(), state_bytes=self.state_bytes,
                 M=self.M, F=self.F, gains=self.gains.data_ptr() if self.F else 0, x=self.x.data_ptr(),
                 counts=self.ints[0].data_ptr(), flags=self.ints[1].data_ptr(), tables=self.ints[2].data_ptr(),
                 y=self.y.data_ptr(), out_counts=self.out_counts.data_ptr(), fade_left=self.fade_left.data_ptr(), slots=self.S,
                 cx=self.cx, mode=0)
        a.update(override or {})
        p = ctypes.c_void_p
        rc = self.lib.vnd_voice_fade_stream_f32_dev(
            a['ctx'], a['bank'], p(a['state']), a['state_bytes'], a['M'], a['F'], p(a['gains']), p(a['x']), p(a['counts']),
            p(a['flags']), p(a['tables']), p(a['y']), p(a['out_counts']), p(a['fade_left']), a['slots'], a['cx'], a['mode'],
            int(self.ms), int(self.width is not None), float(self.width or 0.0), p(self.stream))
        yh, oc, fl = self.y.cpu().numpy(), self.out_counts.cpu().numpy(), self.fade_left.cpu().numpy()
        assert (yh[self.body:] == SENTINEL).all(), 'the call wrote behind the last row'
        assert (oc[self.S:] == SENTINEL).all() and (fl[self.S:] == SENTINEL).all(), 'the call wrote behind its int32 outputs'
        return rc, oc[:self.S].copy(), yh[:self.body].reshape(self.S, self.rows, 2), fl[:self.S].copy()

    def call(self, blocks, counts, flags, tables, where=''):
        """A call that must succeed, held to voice_fade_spans and to its footprint: the rows as float32, one per slot."""
        from vndecorrelate_amd.streaming import voice_fade_spans
        rc, oc, yh, fl = self.raw(blocks, counts, flags, tables)
        assert rc == 0, self.lib.vnd_last_error()
        before, fresh = self.mirror_records, ((np.asarray(flags) & START) != 0) | (self.mirror == 0)
        want, self.mirror, self.mirror_records, self.mirror_left = voice_fade_spans(
            self.mirror, before, counts, flags, tables, self.H, self.F, self.M)
        assert oc.tolist() == want.tolist(), (where, counts, flags)
        assert fl.tolist() == self.mirror_left.tolist(), (where, 'fade_left', counts, flags)
        assert self.positions().tolist() == self.mirror.tolist(), f'{where}: the positions on the device are not the mirror\'s'
        assert self.records().tolist() == self.mirror_records.tolist(), f'{where}: the records on the device are not the mirror\'s'
        for b in range(self.S):                                        # whose frames these are, and with which switches
            if want[b] < 0:
                continue
            lives = self.lives[b]
            if flags[b] & START or (fresh[b] and not (lives and lives[-1]['open'])):
                lives.append(dict(table=0, fades=[], open=True, started=bool(flags[b] & START)))
            if fresh[b]:
                lives[-1]['table'] = int(self.mirror_records[b][1])
            elif flags[b] & SWITCH and self.mirror_records[b].tolist() != before[b].tolist():
                lives[-1]['fades'].append(tuple(int(v) for v in self.mirror_records[b]))
            if flags[b] & END:
                lives[-1]['open'] = False
        rows = []
        for b, n in enumerate(np.maximum(want, 0)):
            hole = np.argwhere(yh[b, :n] == POISON)
            assert not len(hole), f'{where}: slot {b} left (frame, channel) {tuple(hole[0])} of its {n} frames unwritten'
            assert (yh[b, n:] == POISON).all(), f'{where}: slot {b} wrote at or past its {n} frames'
            rows.append(yh[b, :n].view(np.float32).copy())
        return rows

    def voices(self, slot):
        """The voices that began with a START in `slot`, in order: dict(table, fades)."""
        return [life for life in self.lives[slot] if life['started']]


def _expected(bank, x, table, fades, gains, F, cx, epi, first_frame=0):
    """A voice's whole output: plain convolutions by the C oracle, blended, then the pointwise steps.  `fades` hold
    absolute frames; the signal's frame 0 is absolute frame `first_frame`."""
    ms, width = epi
    involved = {table} | {t for _, old, cur in fades for t in (old, cur)}
    conv = {t: bank.reference(x[None], np.array([t], np.int32), cx, PLAIN)[0] for t in involved if 0 <= t < len(bank.alone)}
    if not conv:
        conv = {-1: np.full((len(x), 2), np.nan, np.float32)}
    y = blend(conv, table, [(s - first_frame, old, cur) for s, old, cur in fades], gains, F)
    xf = np.ascontiguousarray(x[..., np.arange(2) % cx])
    if ms:
        O.encode_side(xf, y)
    if width is not None:
        O.apply_stereo_width(y, width)
    return y


def _replay(h, calls):
    """Run `calls` ((blocks, counts, flags, tables), ...) and hand every slot's rows to the voice they belong to: returns
    {slot: [float32 (n, 2), ...]} per voice that began with a START, in order."""
    outs = {b: [] for b in range(h.S)}
    for i, (blocks, counts, flags, tables) in enumerate(calls):
        rows = h.call(blocks, counts, flags, tables, f'call {i}')
        for b in range(h.S):
            if flags[b] & START:
                outs[b].append([])
            if outs[b] and len(rows[b]):
                outs[b][-1].append(rows[b])
    return {b: [np.concatenate(o) if o else np.zeros((0, 2), np.float32) for o in per] for b, per in outs.items()}


def _check_schedule(h, bank, calls, voices, cx, epi):
    """Every voice of a voice_fade_cases.ragged_schedule against the reference; returns the blended samples that are
    neither pure table's bytes."""
    got = _replay(h, calls)
    mixed = 0
    for b, per in voices.items():
        lives = h.voices(b)
        assert len(lives) == len(per) == len(got[b])
        for i, (v, life) in enumerate(zip(per, lives)):
            assert (life['table'], life['fades']) == (v.table, v.fades), ('the harness and the restatement disagree', b, i)
            want = _expected(bank, v.x, v.table, v.fades, h.gains_host, h.F, cx, epi)
            _same(got[b][i], want, ('slot', b, 'voice', i, 'fades', v.fades))
            for s, old, cur in v.fades:
                k = min(h.F, len(v.x) - s)
                pure = [_expected(bank, v.x, t, [], h.gains_host, h.F, cx, epi)[s:s + k].view(np.int32) for t in (old, cur)]
                mine = want[s:s + k].view(np.int32)
                mixed += int(((mine != pure[0]) & (mine != pure[1])).sum())
    return mixed


# ---- 1. no switch: the existing pool's bytes --------------------------------------------------------------------------
@pytest.mark.parametrize('cx', [1, 2])
@pytest.mark.parametrize('epi', [PLAIN, MS_WIDTH], ids=['plain', 'ms_encode-width'])
def test_without_a_switch_it_is_the_voice_pool(bank, cx, epi):
    plan = _ragged_plan(cx, 100 * cx)
    plain, log = Harness(bank, cx, epi), []
    inner = plain.call

    def recorded(blocks, counts, flags, tables, where=''):
        rows = inner(blocks, counts, flags, tables, where)
        log.append((dict(blocks), counts.copy(), flags.copy(), tables.copy(), rows))
        return rows
    plain.call = recorded
    assert _drive(plain, plan, np.random.default_rng(7 + cx)) > 8
    h = FadeHarness(bank, cx, epi, 200)
    for i, (blocks, counts, flags, tables, want) in enumerate(log):
        rows = h.call(blocks, counts, flags, tables, f'call {i}')      # out_counts = voice_spans', as the plain call's were
        assert not h.mirror_left.any()
        for b in range(S):
            assert rows[b].tobytes() == want[b].tobytes(), (i, b)
    assert not h.positions().any()


# ---- 2. a ragged schedule with switches -------------------------------------------------------------------------------
@pytest.mark.parametrize('cx, epi', [(2, PLAIN), (2, MS_WIDTH), (1, MS_WIDTH)], ids=['plain', 'ms_encode-width', 'mono-in'])
def test_ragged_schedule_with_switches(bank, cx, epi):
    assert bank.H == bank_latency()
    shape = {**RAGGED['shape'], 'cx': cx}
    calls, voices, counted = ragged_schedule(RAGGED['seed'], H=bank.H, **shape)
    # (at F = 200 a fade's frames are a row's first 200: none reaches frame 512 - test_fade_lengths' F = 1500 does)
    assert counted['crosses_512'] == 0 and all(counted[case] for case in RAGGED['cases']), counted
    h = FadeHarness(bank, cx, epi, shape['F'])
    mixed = _check_schedule(h, bank, calls, voices, cx, epi)
    assert mixed > 0, 'no blended sample differs from both pure tables'
    assert not h.positions().any()


# ---- 3. F = 0, 1 and a fade longer than a row -------------------------------------------------------------------------
@pytest.mark.parametrize('F', [0, 1, 1500])
def test_fade_lengths(bank, F):
    cx, epi = 2, MS_WIDTH
    assert F in (0, 1) or F > M + bank.H
    calls, voices, counted = ragged_schedule(RAGGED['lengths_seed'], H=bank.H, **{**RAGGED['shape'], 'F': F})
    assert counted['accepted'] and counted['switch_on_fresh']
    if F == 1500:                      # a fade reaches frame 512 of a row, holds a whole tile, and comes back over three calls
        assert all(counted[case] for case in RAGGED['long_cases']), counted
    h = FadeHarness(bank, cx, epi, F, _gains(F, 'equal_power'))
    mixed = _check_schedule(h, bank, calls, voices, cx, epi)
    assert (mixed > 0) == (F > 0)


# ---- 4. every instantiation -------------------------------------------------------------------------------------------
def _fade_plan(bank, max_frames, slots, F, cx, epi):
    from vndecorrelate_amd import _native_fade
    head, *fields = _native_fade.describe_voice_fade_stream(bank.table, max_frames, F, slots, cx, 0,
                                                            epi[0] or epi[1] is not None).split()
    assert head == 'voice_fade_stream'
    return {k: int(v) for k, v in (f.split('=') for f in fields)}


def _long_pool_plan(slots, cx, H, T, seed):
    """{slot: [Voice, ...]}: mostly voices of several calls - M, M + H + 1, 3 M frames - that can switch, the short ones of
    test_gpu_voice_pool._pool_plan among them, a tenth of the slots reused after END, a few never started."""
    rng = np.random.default_rng(seed)
    sig = lambda n, k: _noise((n, cx), 100003 * seed + k)
    plan = {}
    for slot in range(slots):
        u, k = rng.random(), 2 * slot
        n = int(rng.choice([1, 150, 513, BIG_M, BIG_M + H + 1, 3 * BIG_M], p=[0.05, 0.05, 0.1, 0.3, 0.3, 0.2]))
        table = int(rng.integers(T))
        if u < 0.05:
            continue
        plan[slot] = [Voice(sig(n, k), table, int(rng.integers(0, 3)), end_with_last=bool(rng.random() < 0.7))]
        if u < 0.15:
            plan[slot].append(Voice(sig(int(rng.choice([513, BIG_M])), k + 1), (table + 1) % T, 0))
    return plan


@pytest.mark.parametrize('epi', [PLAIN, MS_WIDTH], ids=['plain', 'ms_encode-width'])
@pytest.mark.parametrize('r', [1, 2, 4])
@pytest.mark.parametrize('path', ['class', 'function'])
@pytest.mark.parametrize('cx', [1, 2])
def test_every_form(ctx, bank, function_bank, cx, path, r, epi):
    """voice_fade_stream_kernel<cx, MODE, r, EPI> for every cx, MODE, r and EPI, by test_gpu_voice_pool.test_every_form's
    recipe: the pools that plan r = 4, 2 and 1 at M = 2100, the plan named by the describe hook before anything runs.  F is
    longer than the tile of the form, so a fade has whole tiles inside it and tiles it ends in."""
    bk = bank if path == 'class' else function_bank
    slots, T = _pool_slots(ctx, r), len(bk.alone)
    F = {1: 700, 2: 1500, 4: 2300}[r]
    text = _fade_plan(bk, BIG_M, slots, F, cx, epi)
    tiles = -(-(BIG_M + bk.H) // (512 * r))
    want = dict(r=r, fma=int(path == 'class'), epilogue=int(epi != PLAIN), tiles=tiles, nblocks=slots * tiles,
                advance_groups=-(-slots // 256), fade_frames=F)
    assert {k: text[k] for k in want} == want, text
    plan = _long_pool_plan(slots, cx, bk.H, T, 1000 * cx + 10 * r + (path == 'class'))
    h = FadeHarness(bk, cx, epi, F, slots=slots, max_frames=BIG_M)
    rng = np.random.default_rng(17 + cx + r)

    def switches(call, blocks, counts, flags, tables):
        """Half of the live voices that are not starting ask for another table, whether their last fade is through or not."""
        for b in range(slots):
            live = h.lives[b] and h.lives[b][-1]['open']
            if live and not flags[b] & START and rng.random() < 0.5:
                flags[b] |= SWITCH
                tables[b] = int(rng.integers(T))
    calls = _drive(h, plan, np.random.default_rng(3 + cx + r), switches)
    assert calls >= 6, calls
    total = switched = 0
    for slot, per in plan.items():
        lives = h.voices(slot)
        assert len(lives) == len(per)
        for i, (v, life) in enumerate(zip(per, lives)):
            total += 1
            switched += bool(life['fades'])
            _same(v.result(), _expected(bk, v.x, life['table'], life['fades'], h.gains_host, F, cx, epi),
                  ('slot', slot, 'voice', i, life['fades']))
    print(f'{calls} calls, {slots} slots, {total} voices, {switched} switched')
    assert 3 * switched >= total, (switched, total)
    assert not h.positions().any()


# ---- 5. positions a long-lived voice reaches --------------------------------------------------------------------------
@pytest.mark.parametrize('cx', [2, 1])
def test_planted_positions_with_a_switch_in_the_first_call(bank, cx):
    """No START: the slots go on from the position, history and record planted in their state, and switch at once.  The fade
    of the slot at 2^32 - 300 begins at 2^32 - 300 - H and is 1500 frames long: it straddles 2^32."""
    epi, F, H = MS_WIDTH, 1500, bank.H
    planted = {0: 2 ** 32 - 300, 3: 2 ** 53 + 1}
    h = FadeHarness(bank, cx, epi, F)
    sigs = {b: _noise((H + 2600, cx), 900 + b + cx) for b in planted}
    for b, P in planted.items():
        h.plant(b, P, sigs[b][:H], (-F, 1, 1))                         # table 1 since its start, never switched
    assert planted[0] - H < 2 ** 32 < planted[0] - H + F
    outs, done = {b: [] for b in planted}, 0
    for i, n in enumerate((600, 0, 7, 599, 600, 600, 194)):
        counts, flags, tables = np.zeros(S, np.int32), np.zeros(S, np.int32), np.full(S, 1, np.int32)
        for b in planted:
            counts[b] = n
            flags[b] = (SWITCH if i in (0, 1) else 0) | (END if done + n == 2600 else 0)
            tables[b] = 3 if i == 0 else 4                             # the switch of call 1 comes inside the fade: ignored
        rows = h.call({b: sigs[b][H + done:H + done + n] for b in planted}, counts, flags, tables, f'call {i}')
        if i == 0:
            assert h.mirror_left[0] == F - 600 and h.records()[0].tolist() == [planted[0] - H, 1, 3]
        for b in planted:
            outs[b].append(rows[b])
        done += n
    assert done == 2600 and not h.positions().any()
    for b, P in planted.items():
        life, = h.voices(b)
        assert life['fades'] == [(P - H, 1, 3)]
        want = _expected(bank, sigs[b], 1, life['fades'], h.gains_host, F, cx, epi, first_frame=P - H)
        _same(np.concatenate(outs[b]), want, ('planted at', P))


# ---- 6. a bad table on SWITCH -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad', [5, -1, 2 ** 31 - 1])
def test_a_switch_to_a_bad_table_is_nan_from_the_fade_on(bank, bad):
    cx, epi, F, H = 2, MS_WIDTH, 200, bank.H
    h = FadeHarness(bank, cx, epi, F)
    x = _noise((S, 1700, cx), 61)
    outs, pos = [[] for _ in range(S)], 0
    for i, n in enumerate((600, 500, 600)):
        flags = np.full(S, (START if i == 0 else 0) | (END if i == 2 else 0), np.int32)
        tables = TABLES.copy()
        if i == 1:
            flags[4] |= SWITCH
            tables[4] = bad
        rows = h.call({b: x[b, pos:pos + n] for b in range(S)}, np.full(S, n, np.int32), flags, tables, f'call {i}')
        pos += n
        assert h.positions()[4] == (pos if i < 2 else 0)               # the position advances
        for b in range(S):
            outs[b].append(rows[b])
    s = 600 - H
    assert h.voices(4)[0]['fades'] == [(s, int(TABLES[4]), bad)]
    for b in range(S):
        got = np.concatenate(outs[b])
        want = _expected(bank, x[b], int(TABLES[b]), [], h.gains_host, F, cx, epi)
        if b == 4:
            _same(got[:s], want[:s], 'below s: the old table')
            assert got.shape == want.shape and np.isnan(got[s:]).all()
        else:
            _same(got, want, ('beside a bad switch', b))


# ---- 7. graph replay --------------------------------------------------------------------------------------------------
def test_graph_replay_equals_the_uncaptured_run(dec, ctx):
    import torch
    from vndecorrelate_amd.streaming import voice_fade_spans
    cx, F = 2, 200
    stages = _velvets(dec, sorted(set(KAPPAS)), mode='LR', width=0.35)
    rng = np.random.default_rng(4)
    calls = []
    for i in range(9):
        counts = rng.choice([0, 1, 7, 64, 599, 600], S).astype(np.int32)
        flags = np.zeros(S, np.int32)
        tables = rng.integers(0, 5, S).astype(np.int32)
        if i == 0:
            flags[:5] = START
        else:
            flags[rng.random(S) < 0.4] |= SWITCH
        if i == 3:
            flags[5] = START | END | SWITCH
            flags[1] |= END
        if i == 5:
            flags[1] = START
        if i == 8:
            flags[:] |= END
        calls.append((rng.uniform(-1, 1, (S, M, cx)).astype(np.float32), counts, flags, tables))
    dev = torch.device('cuda', ctx.device)

    def run(replayed):
        pool = dec.decorrelate_voice_pool(stages, slots=S, in_channels=cx, max_frames_per_call=M, fade_frames=F)
        x = torch.empty((S, M, cx), dtype=torch.float32, device=dev)
        counts, flags, tables, oc = (torch.empty(S, dtype=torch.int32, device=dev) for _ in range(4))
        y = torch.empty((S, pool.row_frames, 2), dtype=torch.int32, device=dev)
        out = (y.view(torch.float32), oc)
        pool.reset()                                                           # allocates state, gains, fade_left_dev
        left = pool.fade_left_dev
        if replayed:
            graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
            with torch.cuda.graph(graph, stream=side):
                pool.process_dev(x, counts, flags, tables, out=out)
            torch.cuda.synchronize(dev)
        results = []
        for xh, ch, fh, th in calls:
            x.copy_(torch.from_numpy(xh))
            counts.copy_(torch.from_numpy(ch))
            flags.copy_(torch.from_numpy(fh))
            tables.copy_(torch.from_numpy(th))
            y.fill_(POISON)
            if replayed:
                graph.replay()
            else:
                pool.process_dev(x, counts, flags, tables, out=out)
            torch.cuda.synchronize(dev)
            assert pool.fade_left_dev.data_ptr() == left.data_ptr()
            results.append((y.cpu().numpy(), oc.cpu().numpy(), left.cpu().numpy()))
        return pool, results
    pool, plain = run(False)                                                   # first: it loads the kernels
    _, replay = run(True)
    pos, rec, accepted, refused = np.zeros(S, np.int64), np.zeros((S, 3), np.int64), 0, 0
    for i, ((y0, c0, l0), (y1, c1, l1)) in enumerate(zip(plain, replay)):
        _, counts, flags, tables = calls[i]
        before, was = rec, pos
        want, pos, rec, left = voice_fade_spans(pos, rec, counts, flags, tables, pool.latency_frames, F, M)
        asked = ((flags & SWITCH) != 0) & ((flags & START) == 0) & (was != 0)
        changed = (rec != before).any(axis=1)
        accepted, refused = accepted + int((asked & changed).sum()), refused + int((asked & ~changed).sum())
        assert c0.tolist() == want.tolist() == c1.tolist(), i
        assert l0.tolist() == left.tolist() == l1.tolist(), i
        assert y0.tobytes() == y1.tobytes(), i                                 # outputs and untouched frames alike
        for b, n in enumerate(want):
            assert not (y0[b, :n] == POISON).any() and (y0[b, n:] == POISON).all(), (i, b)
    assert accepted and refused, (accepted, refused)


# ---- 8. the dict form -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cx', [1, 2])
def test_dict_form_with_switches(dec, ctx, cx):
    F = 200
    stages = _velvets(dec, KAPPAS)                                             # 6 bank entries over 5 tables, MS, two-sided
    env = tuple(O.DEFAULT_ENVELOPE)
    oracle_bank = Bank.of_members(ctx, [(_taps(k, filtered=(0, 1)), env, True) for k in sorted(set(KAPPAS))])
    try:
        pool = dec.decorrelate_voice_pool(stages, slots=3, in_channels=cx, max_frames_per_call=M, fade_frames=F,
                                          fade='equal_power')
        H = pool.latency_frames
        assert pool.bank_tables.tolist() == TABLES.tolist() and H == oracle_bank.H
        a, b, c = (_noise((n, cx), 70 + n + cx) for n in (1700, 1300, 513))
        got = {name: [] for name in 'abc'}

        def take(out, **slots):
            assert sorted(out) == sorted(slots.values())
            for name, slot in slots.items():
                got[name].append(out[slot])
        take(pool.process({0: a[:600], 1: b[:500]}, start={0: 2, 1: 3}), a=0, b=1)
        assert pool.fade_left.tolist() == [0, 0, 0]
        take(pool.process({0: a[600:1000], 1: b[500:900], 2: c}, start={2: 5}, end=[2], switch={0: 4}), a=0, b=1, c=2)
        assert pool.fade_left.tolist() == [0, 0, 0]                            # 400 frames came back: the fade is through
        take(pool.process({0: a[1000:1100], 1: b[900:1000]}, switch={0: 0, 1: 1}), a=0, b=1)
        assert pool.fade_left.tolist() == [100, 100, 0]
        with pytest.raises(ValueError, match='slot 1 has 100 frames of its fade left'):
            pool.process({1: b[1000:]}, switch={1: 0})
        take(pool.process({0: a[1100:], 1: b[1000:]}, end=[0, 1]), a=0, b=1)
        assert TABLES[3] == TABLES[1]               # b fades to the table it has: a * g0 + a * g1, and sin + cos is not 1
        assert not pool.positions.any() and not pool.live.any() and not pool.fade_left.any()
        assert pool.transfers == {'to_device': 1, 'to_host': 1}
        g, T = pool.fade_gains, [int(t) for t in TABLES]
        fades = {'a': [(600 - H, T[2], T[4]), (1000 - H, T[4], T[0])], 'b': [(900 - H, T[3], T[1])], 'c': []}
        for name, x, first in (('a', a, T[2]), ('b', b, T[3]), ('c', c, T[5])):
            want = _expected(oracle_bank, x, first, fades[name], g, F, cx, (True, None))
            _same(np.concatenate(got[name]), want, name)
        _same(np.concatenate(got['c']), stages[5].decorrelate(c[:, 0] if cx == 1 else c), 'a voice that never switches')
    finally:
        oracle_bank.close()


# ---- 9. the ABI's refusals --------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ctx, bank):
    from vndecorrelate_amd import _native_fade
    F = 200
    h = FadeHarness(bank, 2, (True, None), F)
    x = _noise((S, 100, 2), 9)
    blocks = {b: x[b] for b in range(S)}
    counts, flags = np.full(S, 100, np.int32), np.full(S, START, np.int32)
    h.call(blocks, counts, flags, TABLES, 'a good call')                       # positions 100: a refusal must keep them
    flags[:] = SWITCH
    before = h.state_words().copy()
    for override, status, text in (
            (dict(counts=0), INVALID, b'null'), (dict(flags=0), INVALID, b'null'), (dict(tables=0), INVALID, b'null'),
            (dict(x=0), INVALID, b'null'), (dict(y=0), INVALID, b'null'), (dict(out_counts=0), INVALID, b'null'),
            (dict(state=0), INVALID, b'null state'), (dict(bank=None), INVALID, b'null context or tap table'),
            (dict(ctx=None), INVALID, b'null context or tap table'),
            (dict(F=-1), INVALID, b'negative fade_frames'), (dict(F=(1 << 20) + 1), UNSUPPORTED, b'fade_frames'),
            (dict(gains=0), INVALID, b'null gains'),
            (dict(state_bytes=h.state_bytes - 4), INVALID, b'the crossfading voice pool needs'),
            (dict(state=h.state.data_ptr() + 8), INVALID, b'16-byte aligned'),
            (dict(slots=-1), INVALID, b'negative slots'), (dict(M=-1), INVALID, b'max_frames_per_call'),
            (dict(cx=3), INVALID, b'mono or stereo'), (dict(mode=2), UNSUPPORTED, b'VND_MODE_EXACT only')):
        rc, oc, yh, fl = h.raw(blocks, counts, flags, TABLES, override)
        message = h.lib.vnd_last_error()
        assert rc == status and text in message, (override, rc, message)
        assert (yh == POISON).all() and (oc == SENTINEL).all() and (fl == SENTINEL).all(), override
        assert h.state_words().tobytes() == before.tobytes(), override
    # the query and the reset check the same pool
    need = ctypes.c_int64(-1)
    query = h.lib.vnd_voice_fade_stream_state_bytes
    assert query(bank.table.handle, S, 2, M, -1, ctypes.byref(need)) == INVALID and need.value == 0
    assert query(bank.table.handle, S, 2, M, (1 << 20) + 1, ctypes.byref(need)) == UNSUPPORTED and need.value == 0
    assert query(bank.table.handle, S, 2, M, 1 << 20, ctypes.byref(need)) == 0 and need.value == h.state_bytes
    rc = h.lib.vnd_voice_fade_stream_reset_dev(ctx.handle, ctypes.c_void_p(h.state.data_ptr()), h.state_bytes - 4, S, 2,
                                               bank.table.handle, M, F, ctypes.c_void_p(h.stream))
    assert rc == INVALID and b'the crossfading voice pool needs' in h.lib.vnd_last_error()
    assert h.state_words().tobytes() == before.tobytes()
    with pytest.raises(ValueError, match='negative fade_frames'):
        _native_fade.describe_voice_fade_stream(bank.table, M, -1, S, 2)
    # a null fade_left is taken, and F = 0 takes null gains: the voices of the first call switch hard and end
    hard = FadeHarness(bank, 2, (True, None), 0)
    hard.call(blocks, counts, np.full(S, START, np.int32), TABLES, 'F = 0: start')
    rc, oc, yh, fl = hard.raw({}, np.zeros(S, np.int32), np.full(S, SWITCH | END, np.int32), TABLES[::-1].copy(),
                              dict(gains=0, fade_left=0))
    assert rc == 0 and oc.tolist() == [100] * S and (fl == SENTINEL).all()
    for b in range(S):
        want = _expected(bank, x[b], int(TABLES[::-1][b]), [], hard.gains_host, 0, 2, (True, None))
        _same(yh[b, :100].view(np.float32), want, ('a hard switch before anything came back', b))
