"""GPU tier of the level-envelope voice pool (vnd_polar_level_voice_stream_*, include/vnd_polar_level_voice_stream.h;
vectorscope.LevelVoicePool).  Every comparison is of bytes: after EVERY call the levels and the slice counts of EVERY slot
against the one-shot device entry (vnd_polar_level_*_dev, n_each) on the frames of the slot's window.

The harness drives the C ABI on poisoned memory: the state is NaN bytes until the reset, every ring entry starts as slice 0
with a key above every real one and is never cleared - a stale read shows up as a count and as a level - the chunk rows past
counts[b] are NaN, levels, bin_counts and valid have guards on both sides and the state has a poisoned tail.  After every
call valid, the device's positions and its fills equal the mirror (vectorscope.scope_voice_spans / scope_voice_window), and
the ring rows of slots that did not answer 1, every guard and the tail are unchanged."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

START, END = 1, 2
GUARD = 5                                    # values before and after levels, bin_counts and valid
TAIL = 256                                   # poisoned bytes past the state
INVALID, UNSUPPORTED = 1, 4
STALE_KEY = {4: 0x7F000000, 8: 0x7FE0000000000000}      # 2^127 and 2^1023: finite, above every radius of the tests
LEVEL_POISON, COUNT_POISON = -7.5, 0x5A5A5A5A


@pytest.fixture(scope='module')
def ctx():
    from vndecorrelate_amd import _native
    context = _native.default_context()
    assert 'gfx950' in context.info()['name']
    return context


@pytest.fixture(scope='module')
def vs(ctx):
    from vndecorrelate_amd import vectorscope
    return vectorscope


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


def pad16(v):
    return (v + 15) // 16 * 16


def one_shot(torch, ctx, windows, edges_dev, bins, ps, *, dtype, ms=True, fold=True, scale=1.0):
    """vnd_polar_level_*_dev on a list of (n, 2) windows, one signal each (n_each: a window of no frames is a row of zeros):
    (levels (B, P, bins) of dtype, bin_counts uint32 (B, bins))."""
    from vndecorrelate_amd import _native
    dev = torch.device('cuda', ctx.device)
    dtype = np.dtype(dtype)
    B, n = len(windows), max([1] + [len(w) for w in windows])
    host = np.zeros((B, n, 2), dtype)
    for b, w in enumerate(windows):
        host[b, :len(w)] = w
    x = torch.from_numpy(host).to(dev)
    each = torch.from_numpy(np.array([len(w) for w in windows], np.int32)).to(dev)
    levels = torch.full((B, len(ps), bins), 3.25, dtype=x.dtype, device=dev)
    counts = torch.full((B, bins), 7, dtype=torch.int32, device=dev)
    is64 = dtype == np.float64
    need = _native.polar_level_work_bytes(B, n, bins, len(ps), is64)
    work = torch.empty(((need + 7) // 8,), dtype=torch.int64, device=dev)
    e = dtype.itemsize
    _native.polar_level_device(ctx, x.data_ptr(), x.data_ptr() + e, B, n, 2 * n, 2, edges_dev.data_ptr(), bins, ps,
                               levels.data_ptr(), counts.data_ptr(), work_ptr=work.data_ptr(), work_bytes=need, ms_mode=ms,
                               semicircular=fold, radius_scale=scale, n_each_ptr=each.data_ptr(), float64=is64,
                               stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return levels.cpu().numpy(), counts.cpu().numpy().view(np.uint32)


class Harness:
    """One pool at the C ABI on poisoned memory.  planar: L and R as two (S, M) arrays; else channels of one (S, M, 2)."""

    def __init__(self, torch, ctx, vs, S, M, W, bins=8, ps=(95.0, 50.0), *, dtype=np.float32, planar=False, ms=True, fold=True,
                 scale=1.0, reset=True):
        from vndecorrelate_amd import _native
        self.torch, self.ctx, self.native, self.vs = torch, ctx, _native, vs
        self.dev = torch.device('cuda', ctx.device)
        self.S, self.M, self.W, self.bins, self.ps = S, M, W, bins, [float(p) for p in ps]
        self.P = len(self.ps)
        self.ms, self.fold, self.scale = ms, fold, scale
        self.dtype, self.planar = np.dtype(dtype), planar
        self.e = self.dtype.itemsize
        self.is64 = self.e == 8
        self.edges = torch.from_numpy(vs.level_edges(bins)[0].copy()).to(self.dev)
        self.need = _native.level_voice_stream_state_bytes(S, M, W, self.is64)
        self.fill_at = pad16(8 * S)
        self.keys_at = self.fill_at + pad16(4 * S)
        self.bins_at = self.keys_at + pad16(S * W * self.e)
        assert self.need == self.bins_at + pad16(S * W * 2)
        self.raw_state = torch.full(((self.need + TAIL) // 4,), float('nan'), dtype=torch.float32, device=self.dev)
        self.state_bytes = self.raw_state.view(torch.uint8)
        self.state = self.state_bytes[:self.need]
        self.keys_view().fill_(STALE_KEY[self.e])
        self.slices_view().fill_(0)
        self.tdt = torch.float32 if self.e == 4 else torch.float64
        self.chunk = torch.empty((2, S, M) if planar else (S, M, 2), dtype=self.tdt, device=self.dev)
        self.counts, self.flags = (torch.empty(S, dtype=torch.int32, device=self.dev) for _ in range(2))
        self.levels = torch.full((S * self.P * bins + 2 * GUARD,), LEVEL_POISON, dtype=self.tdt, device=self.dev)
        self.bin_counts = torch.full((S * bins + 2 * GUARD,), COUNT_POISON, dtype=torch.int32, device=self.dev)
        self.val = torch.empty((S + 2 * GUARD,), dtype=torch.int32, device=self.dev)
        self.work_need = _native.level_voice_stream_work_bytes(S, W, bins, self.P, self.is64)
        self.work = torch.full(((self.work_need + 7) // 8,), -1, dtype=torch.int64, device=self.dev)
        self.window = [np.zeros((0, 2), self.dtype) for _ in range(S)]       # the frames the slot's ring holds, oldest first
        self.mirror = self.fills = None                      # the positions and fills, once they are known
        self.checked = self.slid = 0
        if reset:
            self.reset()

    def stream(self):
        return self.torch.cuda.current_stream(self.dev).cuda_stream

    def reset(self):
        self.native.level_voice_stream_reset_device(self.ctx, self.state.data_ptr(), self.need, self.S, self.M, self.W,
                                                    float64=self.is64, stream=self.stream())
        self.mirror, self.fills = np.zeros(self.S, np.int64), np.zeros(self.S, np.int64)
        self.window = [np.zeros((0, 2), self.dtype) for _ in range(self.S)]

    # ---- the parts of the state ---------------------------------------------------------------------------------------
    def positions_view(self):
        return self.state[:8 * self.S].view(self.torch.int64)

    def fill_view(self):
        return self.state[self.fill_at:self.fill_at + 4 * self.S].view(self.torch.int32)

    def keys_view(self):
        t = self.torch.int32 if self.e == 4 else self.torch.int64
        return self.state[self.keys_at:self.keys_at + self.S * self.W * self.e].view(t).view(self.S, self.W)

    def slices_view(self):
        return self.state[self.bins_at:self.bins_at + self.S * self.W * 2].view(self.torch.int16).view(self.S, self.W)

    def rings(self):
        return self.keys_view().cpu().numpy().copy(), self.slices_view().cpu().numpy().copy()

    def rest_is_poison(self):
        """The padding behind each ring and the tail past the state (the reset's one memset runs from the first position to
        the first key, padding included): the gaps that are not poison any more, none if all is well."""
        S, W, host = self.S, self.W, self.state_bytes.cpu().numpy()
        gaps = [(self.keys_at + S * W * self.e, self.bins_at), (self.bins_at + S * W * 2, len(host))]
        nan = np.full(len(host) // 4, np.nan, np.float32).view(np.uint8)
        return [(lo, hi) for lo, hi in gaps if host[lo:hi].tobytes() != nan[lo:hi].tobytes()]

    def plant(self, b, position, like):
        """Slot b as slot `like` would be at `position` (its rings, its fill and its window); the residues must agree."""
        assert position % self.W == int(self.mirror[like]) % self.W
        self.positions_view()[b] = position
        self.fill_view()[b] = self.fill_view()[like]
        self.keys_view()[b] = self.keys_view()[like]
        self.slices_view()[b] = self.slices_view()[like]
        self.window[b] = self.window[like].copy()
        self.mirror[b], self.fills[b] = position, self.fills[like]

    # ---- calls ------------------------------------------------------------------------------------------------------
    def raw_push(self, **kw):
        """The C push with pointers and scalars replaced by name; returns the status."""
        if self.planar:
            l, r, ss, fs = self.chunk[0].data_ptr(), self.chunk[1].data_ptr(), self.M, 1
        else:
            l, r, ss, fs = self.chunk.data_ptr(), self.chunk.data_ptr() + self.e, 2 * self.M, 2
        a = dict(state=self.state.data_ptr(), state_bytes=self.need, M=self.M, W=self.W, l=l, r=r, ss=ss, fs=fs,
                 counts=self.counts.data_ptr(), flags=self.flags.data_ptr(), ms=int(self.ms), fold=int(self.fold),
                 scale=self.scale, edges=self.edges.data_ptr(), bins=self.bins, val=self.val.data_ptr() + 4 * GUARD, S=self.S,
                 ctx=self.ctx.handle)
        a.update(kw)
        p = ctypes.c_void_p
        fn = getattr(self.ctx._lib, f"vnd_polar_level_voice_stream_push_{'f64' if self.is64 else 'f32'}_dev")
        return fn(a['ctx'], p(a['state']), a['state_bytes'], a['M'], a['W'], p(a['l']), p(a['r']), a['ss'], a['fs'],
                  p(a['counts']), p(a['flags']), a['ms'], a['fold'], ctypes.c_double(a['scale']), p(a['edges']), a['bins'],
                  p(a['val']), a['S'], p(self.stream()))

    def raw_levels(self, **kw):
        a = dict(state=self.state.data_ptr(), state_bytes=self.need, M=self.M, W=self.W, bins=self.bins, ps=self.ps,
                 levels=self.levels.data_ptr() + self.e * GUARD, bin_counts=self.bin_counts.data_ptr() + 4 * GUARD,
                 work=self.work.data_ptr(), work_bytes=self.work_need, S=self.S, ctx=self.ctx.handle)
        a.update(kw)
        p = ctypes.c_void_p
        ps = (ctypes.c_double * max(1, len(a['ps'])))(*a['ps']) if a['ps'] is not None else None
        fn = getattr(self.ctx._lib, f"vnd_polar_level_voice_stream_levels_{'f64' if self.is64 else 'f32'}_dev")
        return fn(a['ctx'], p(a['state']), a['state_bytes'], a['M'], a['W'], a['bins'], ps, a.get('P', len(a['ps'] or ())),
                  p(a['levels']), p(a['bin_counts']), p(a['work']), a['work_bytes'], a['S'], p(self.stream()))

    def upload(self, blocks, counts, flags):
        torch = self.torch
        host = np.full((self.S, self.M, 2), np.nan, self.dtype)
        for b, block in enumerate(blocks):
            if block is not None and len(block):
                host[b, :len(block)] = block
        if self.planar:
            host = np.ascontiguousarray(host.transpose(2, 0, 1))
        self.chunk.copy_(torch.from_numpy(host))
        self.counts.copy_(torch.from_numpy(np.asarray(counts, np.int64).astype(np.int32)))
        self.flags.copy_(torch.from_numpy(np.asarray(flags, np.int32)))
        self.val.fill_(-77)

    def push(self, blocks, counts, flags):
        """One push; checks valid, the positions, the fills, the untouched ring rows and the poison; returns valid."""
        from vndecorrelate_amd.vectorscope import scope_voice_spans, scope_voice_window
        self.upload(blocks, counts, flags)
        keys_before, slices_before = self.rings()
        assert self.raw_push() == 0, self.ctx._lib.vnd_last_error()
        self.torch.cuda.synchronize(self.dev)
        want, new = scope_voice_spans(self.mirror, counts, flags, self.M)
        val = self.val.cpu().numpy()
        assert (val[:GUARD] == -77).all() and (val[GUARD + self.S:] == -77).all()
        assert val[GUARD:GUARD + self.S].tolist() == want.tolist(), (counts, flags, self.mirror)
        assert self.positions_view().cpu().numpy().tolist() == new.tolist()
        keys_after, slices_after = self.rings()
        for b in range(self.S):
            if want[b] != 1:
                assert keys_after[b].tobytes() == keys_before[b].tobytes(), b
                assert slices_after[b].tobytes() == slices_before[b].tobytes(), b
                continue
            p = 0 if int(flags[b]) & START else int(self.mirror[b])
            block = np.asarray(blocks[b], self.dtype).reshape(-1, 2) if blocks[b] is not None else np.zeros((0, 2), self.dtype)
            assert len(block) == counts[b]
            self.window[b] = np.concatenate([self.window[b][:0] if p == 0 else self.window[b], block])[-self.W:]
            lo, hi = scope_voice_window(p + len(block), self.W)
            assert hi - lo == len(self.window[b])
            self.fills[b] = hi - lo
            self.slid += lo > 0
        assert self.fill_view().cpu().numpy().tolist() == self.fills.tolist()
        assert self.rest_is_poison() == []
        self.mirror = new
        return want

    def read(self):
        """The levels entry; checks every slot's rows against the one-shot entry on its window, byte for byte, and the
        guards; the state is not written.  Returns (levels (S, P, bins), bin_counts (S, bins))."""
        state_before = self.state_bytes.clone()
        self.levels.fill_(LEVEL_POISON)
        self.bin_counts.fill_(COUNT_POISON)
        assert self.raw_levels() == 0, self.ctx._lib.vnd_last_error()
        self.torch.cuda.synchronize(self.dev)
        assert bool((self.state_bytes == state_before).all())
        got, cnt = self.levels.cpu().numpy(), self.bin_counts.cpu().numpy().view(np.uint32)
        assert (got[:GUARD] == LEVEL_POISON).all() and (got[-GUARD:] == LEVEL_POISON).all()
        assert (cnt[:GUARD] == COUNT_POISON).all() and (cnt[-GUARD:] == COUNT_POISON).all()
        got = got[GUARD:-GUARD].reshape(self.S, self.P, self.bins)
        cnt = cnt[GUARD:-GUARD].reshape(self.S, self.bins)
        want, want_cnt = one_shot(self.torch, self.ctx, self.window, self.edges, self.bins, self.ps, dtype=self.dtype,
                                  ms=self.ms, fold=self.fold, scale=self.scale)
        for b in range(self.S):
            assert cnt[b].tobytes() == want_cnt[b].tobytes(), (b, cnt[b], want_cnt[b], self.mirror, self.fills)
            assert got[b].tobytes() == want[b].tobytes(), (b, got[b], want[b], self.mirror, self.fills)
            assert int(cnt[b].sum()) <= len(self.window[b])
        self.checked += self.S
        return got, cnt

    def call(self, blocks, counts, flags):
        valid = self.push(blocks, counts, flags)
        levels, cnt = self.read()
        return levels, cnt, valid


def frames(rng, n, dtype):
    """Gaussian frames, sigma 0.5; half of the longer blocks carry the frames the mask treats specially."""
    x = rng.normal(0.0, 0.5, (n, 2))
    if np.dtype(dtype) == np.float64:
        x = x * (1 + 1e-9)                                            # values between float32 ones
    x = x.astype(dtype)
    if n > 4 and rng.random() < 0.5:
        x[0] = (0.25, -0.25)                                          # R = -L, L > 0: +90 degrees, the last edge: no slice
        x[1] = (-0.25, 0.25)                                          # -90 degrees: slice 0
        x[2] = (0.5, 0.5)                                             # mono: 0 degrees, an inner edge
        x[3] = (0.0, 0.0)
        x[4] = x[2]                                                   # an equal key in one slice
    return x


def fuzz_schedule(S, M, seed, dtype, calls=60):
    """(blocks, counts, flags) per call.  Slot 0: END, a new voice with START, END, a voice from position 0 without START;
    slot 1: a discard-START mid-voice; slot 2: whole voices in one call; the last slot is fed M + 1 and -1 and starts late;
    call 9 is idle for every slot; the last call ENDs every voice."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(calls):
        counts = np.array([int(rng.choice([0, 1, M - 1, M, int(rng.integers(0, M + 1))])) for _ in range(S)], np.int64)
        flags = np.zeros(S, np.int32)
        if i == 0:
            flags[:S - 1] = START
        if i < 3:
            counts[S - 1], flags[S - 1] = 0, 0                            # never started so far
        if i == 3:
            flags[S - 1] = START
        if i == 9:
            counts[:] = 0
        if i in (12, 25, 40):
            flags[0] |= END
        if i in (13, 26):
            counts[0] = 0
        if i == 14:
            flags[0] |= START
        if i in (15, 44):
            flags[1] |= START
        if i in (5, 6, 33):
            flags[2] |= START | END
        if i == 7:
            counts[S - 1] = M + 1
        if i == 16:
            counts[S - 1] = -1
        if i == 30:
            counts[S - 1], flags[S - 1] = M + 1, START
        if i == calls - 1:
            flags[:] |= END
        blocks = [frames(rng, int(c), dtype) if 0 <= c <= M else None for c in counts]
        out.append((blocks, counts, flags))
    return out


# ---- 1. the schedule fuzz -----------------------------------------------------------------------------------------------
# W in {64, 67} x M in {1, 23, W} x {float32, float64}; slices, percentiles, chunk layout and mode rotate through the twelve.
FUZZ = [(W, M, dtype) for W in (64, 67) for M in (1, 23, 'W') for dtype in (np.float32, np.float64)]


def _rotating(index):
    """(slices, percentiles, planar, (ms, fold), radius_scale) of fuzz case `index`."""
    return ((8, 360)[index % 2 ^ (index // 2) % 2], ((95.0, 50.0), (0.0, 37.5, 50.0, 100.0))[(index // 2) % 2],
            bool((index // 4) % 2) ^ bool(index % 2), ((True, True), (False, False), (True, False), (False, True))[index % 4],
            (1.0, 0.75)[index % 2])


# every value of every rotating setting appears among the twelve
assert [len({_rotating(i)[k] for i in range(len(FUZZ))}) for k in range(5)] == [2, 2, 2, 4, 2]


@pytest.mark.parametrize('index', range(len(FUZZ)), ids=[f"W{W}-M{M}-{np.dtype(d).name}" for W, M, d in FUZZ])
def test_schedule_fuzz(torch, ctx, vs, index):
    W, M, dtype = FUZZ[index]
    M = W if M == 'W' else M
    bins, ps, planar, ms_fold, scale = _rotating(index)
    h = Harness(torch, ctx, vs, 4, M, W, bins, ps, dtype=dtype, planar=planar, ms=ms_fold[0], fold=ms_fold[1], scale=scale)
    seen = set()
    for blocks, counts, flags in fuzz_schedule(4, M, 100 + index, dtype):
        _, _, valid = h.call(blocks, counts, flags)
        seen |= set(valid.tolist())
    assert seen == {-1, 0, 1} and h.checked == 240
    assert h.slid > 20 or M == 1


# ---- 2. the named cases ---------------------------------------------------------------------------------------------------
def _slot_blocks(S, b, block, M):
    blocks, counts = [None] * S, np.zeros(S, np.int64)
    blocks[b], counts[b] = block, len(block)
    return blocks, counts


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_the_window_fills_wraps_and_is_replaced(torch, ctx, vs, dtype):
    S, M, W = 4, 23, 64
    rng = np.random.default_rng(3)
    h = Harness(torch, ctx, vs, S, M, W, 8, (95.0, 50.0), dtype=dtype)
    levels, cnt = h.read()                                            # 12. never started: zeros, whatever the rings hold
    assert not levels.any() and not cnt.any()
    flags = np.zeros(S, np.int32)
    flags[0] = START
    _, cnt, _ = h.call(*_slot_blocks(S, 0, frames(rng, 23, dtype), M), flags)           # 1. a window not yet full
    assert h.fills.tolist() == [23, 0, 0, 0] and 0 < cnt[0].sum() <= 23 and not cnt[1:].any()
    flags[0] = 0
    h.call(*_slot_blocks(S, 0, frames(rng, 23, dtype), M), flags)
    h.call(*_slot_blocks(S, 0, frames(rng, 18, dtype), M), flags)                       # 2. exactly full: 64 frames
    assert h.fills[0] == W and h.mirror[0] == W and h.slid == 0
    while h.mirror[0] < 3 * W + 10:                                                     # 3. wrapped three times
        h.call(*_slot_blocks(S, 0, frames(rng, int(rng.integers(1, M + 1)), dtype), M), flags)
    assert h.mirror[0] >= 3 * W + 10 and h.slid > 6
    # 5. START of a 5-frame voice over the full ring: the 59 stale entries beyond fill must not count
    flags[0] = START
    _, cnt, _ = h.call(*_slot_blocks(S, 0, rng.normal(0, 0.3, (5, 2)).astype(dtype), M), flags)
    assert h.fills[0] == 5 and cnt[0].sum() == 5
    # 6. END keeps the levels ...
    flags[0] = END
    kept, kept_cnt, _ = h.call(*_slot_blocks(S, 0, rng.normal(0, 0.3, (7, 2)).astype(dtype), M), flags)
    assert h.mirror[0] == 0 and h.fills[0] == 12 and kept_cnt[0].sum() == 12 and kept[0].any()
    idle = np.zeros(S, np.int32)
    again, again_cnt, valid = h.call([None] * S, np.zeros(S, np.int64), idle)
    assert valid.tolist() == [0] * S and again.tobytes() == kept.tobytes() and again_cnt.tobytes() == kept_cnt.tobytes()
    # ... and the next START drops them
    flags[0] = START
    dropped, dropped_cnt, _ = h.call([None] * S, np.zeros(S, np.int64), flags)
    assert h.fills[0] == 0 and not dropped[0].any() and not dropped_cnt[0].any()


@pytest.mark.parametrize('W', [64, 67])
def test_one_block_of_w_frames_replaces_the_window(torch, ctx, vs, W):
    S = 4
    rng = np.random.default_rng(W)
    h = Harness(torch, ctx, vs, S, W, W, 8, (0.0, 37.5, 50.0, 100.0), planar=True)
    flags = np.full(S, START, np.int32)
    h.call([frames(rng, W, np.float32) for _ in range(S)], [W] * S, flags)              # 4. each call is a whole window
    first = h.window[1].copy()
    flags[:] = 0
    h.call([frames(rng, W, np.float32) for _ in range(S)], [W] * S, flags)
    assert h.fills.tolist() == [W] * S and not np.array_equal(first, h.window[1])
    h.call([frames(rng, 3, np.float32) for _ in range(S)], [3] * S, flags)
    assert h.mirror.tolist() == [2 * W + 3] * S


def test_pushes_without_levels_then_one_read(torch, ctx, vs):
    S, M, W = 4, 23, 67
    rng = np.random.default_rng(8)
    h = Harness(torch, ctx, vs, S, M, W, 360, (95.0, 50.0), dtype=np.float64)
    flags = np.full(S, START, np.int32)
    for i in range(9):                                                # 7. nine pushes, no select in between
        counts = rng.integers(0, M + 1, S)
        h.push([frames(rng, int(c), np.float64) for c in counts], counts, flags)
        flags[:] = 0
    levels, cnt = h.read()
    assert (cnt.sum(axis=1) > 0).all() and h.checked == S and h.slid > 0
    again, again_cnt = h.read()                                       # a pure function of the state
    assert again.tobytes() == levels.tobytes() and again_cnt.tobytes() == cnt.tobytes()


def test_bad_counts_pass_through_as_minus_one(torch, ctx, vs):
    S, M, W = 4, 23, 64
    rng = np.random.default_rng(11)
    h = Harness(torch, ctx, vs, S, M, W)
    h.call([frames(rng, M, np.float32) for _ in range(S)], [M] * S, np.full(S, START, np.int32))
    before, before_cnt = h.read()
    blocks = [frames(rng, 4, np.float32), None, None, frames(rng, 2, np.float32)]
    levels, cnt, valid = h.call(blocks, [4, -1, M + 1, 2], np.array([0, 0, START, 0], np.int32))     # 8.
    assert valid.tolist() == [1, -1, -1, 1] and h.mirror.tolist() == [M + 4, M, M, M + 2]
    assert levels[1:3].tobytes() == before[1:3].tobytes() and cnt[1:3].tobytes() == before_cnt[1:3].tobytes()


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_mono_voice_single_frames_and_the_last_edge(torch, ctx, vs, dtype):
    S, M, W = 4, 23, 64
    h = Harness(torch, ctx, vs, S, M, W, 8, (0.0, 37.5, 50.0, 95.0), dtype=dtype)
    mono = np.full((M, 2), 0.3, dtype)                                # 9. a mono voice: every key of its slice is equal
    lone = np.zeros((M, 2), dtype)
    lone[:, 0] = np.linspace(0.1, 0.9, M)                             # left, R = L / 10: about +39.3 degrees, inside a slice
    lone[:, 1] = lone[:, 0] / 10
    lone[5] = (0.04, 0.4)                                             # 10. ... and one frame alone at about -39.3 degrees
    edge = np.tile(np.array([[0.25, -0.25]], dtype), (M, 1))          # 11. anti-phase, exactly +90 degrees: no slice
    edge[3] = (-0.25, 0.25)                                           # (-90 degrees is slice 0)
    two = np.zeros((2, 2), dtype)
    two[:, 1] = (0.2, 0.6)                                            # two frames in one slice: the lerp between them
    two[:, 0] = two[:, 1] / 10
    levels, cnt, _ = h.call([mono, lone, edge, two], [M, M, M, 2], np.full(S, START, np.int32))
    assert cnt[0].tolist().count(M) == 1 and cnt[0].sum() == M
    slice_of_mono = int(np.argmax(cnt[0]))
    assert len(set(levels[0][:, slice_of_mono].tolist())) == 1 and levels[0][0, slice_of_mono] > 0
    assert sorted(c for c in cnt[1].tolist() if c) == [1, M - 1]
    alone = cnt[1].tolist().index(1)
    assert len(set(levels[1][:, alone].tolist())) == 1                # one frame: every percentile is its radius
    assert cnt[2].sum() == 1 and cnt[2][0] == 1                       # 22 frames at the last edge fall in no slice
    assert cnt[3].sum() == 2 and cnt[3].max() == 2
    for _ in range(4):                                                # the same frames again, past the wrap
        h.call([mono, lone, edge, two], [M, M, M, 2], np.zeros(S, np.int32))
    assert h.slid > 0


@pytest.mark.parametrize('W', [64, 67])
def test_a_planted_position_past_2_to_40_continues_as_the_voice_would(torch, ctx, vs, W):
    S, M = 4, 23
    rng = np.random.default_rng(40 + W)
    P = 2 ** 40 + 3                                                   # 13.
    h = Harness(torch, ctx, vs, S, M, W)
    target = W + P % W                                                # slot 0 up to a position of the same residue
    flags = np.zeros(S, np.int32)
    flags[0] = START
    while h.mirror[0] < target:
        n = int(min(M, target - h.mirror[0]))
        h.push(*_slot_blocks(S, 0, frames(rng, n, np.float32), M), flags)
        flags[0] = 0
    assert h.mirror[0] == target and h.fills[0] == W
    h.plant(1, P, like=0)
    h.read()
    for n in (7, M, 1, M, M, M):                                      # on past another wrap, the two slots apart
        blocks = [frames(rng, 3, np.float32), frames(rng, n, np.float32), None, None]
        _, _, valid = h.call(blocks, [3, n, 0, 0], flags)
        assert valid.tolist() == [1, 1, 0, 0]
    assert h.mirror[1] == P + 8 + 4 * M and h.mirror[1] > 2 ** 40 + W
    assert not np.array_equal(h.window[0], h.window[1])


def test_two_workgroups_a_slot_in_the_select(torch, ctx, vs):
    S, W = 2, vs.LEVEL_SPAN_FRAMES + 5
    rng = np.random.default_rng(77)
    h = Harness(torch, ctx, vs, S, W, W, 360, (95.0, 50.0))
    flags = np.full(S, START, np.int32)
    whole = [rng.normal(0, 0.5, (W, 2)).astype(np.float32), rng.normal(0, 0.2, (W - 9, 2)).astype(np.float32)]
    _, cnt, _ = h.call(whole, [W, W - 9], flags)
    assert h.fills.tolist() == [W, W - 9] and cnt[0].sum() > vs.LEVEL_SPAN_FRAMES
    flags[:] = 0
    h.call([frames(rng, 1000, np.float32), frames(rng, 20, np.float32)], [1000, 20], flags)
    assert h.fills.tolist() == [W, W] and h.slid == 2


def test_a_state_that_was_never_reset(torch, ctx, vs):
    S, M, W = 4, 23, 64
    rng = np.random.default_rng(5)
    h = Harness(torch, ctx, vs, S, M, W, reset=False)
    h.mirror, h.fills = np.full(S, 0x7FC000007FC00000, np.int64), np.full(S, 0x7FC00000, np.int64)     # the NaN bytes
    levels, cnt = h.read()                                            # fills outside [0, W]: no frame
    assert not levels.any() and not cnt.any()
    blocks = [frames(rng, 5, np.float32), frames(rng, 5, np.float32), None, None]
    h.upload(blocks, [5, 5, 0, 0], [START, 0, 0, START | END])
    assert h.raw_push() == 0
    torch.cuda.synchronize(h.dev)
    assert h.val.cpu().numpy()[GUARD:GUARD + S].tolist() == [1, -1, -1, 1]      # (a bad position answers -1 even when idle)
    assert h.positions_view().cpu().numpy().tolist() == [5, 0x7FC000007FC00000, 0x7FC000007FC00000, 0]
    assert h.fill_view().cpu().numpy().tolist() == [5, 0x7FC00000, 0x7FC00000, 0]
    h.window[0], h.mirror, h.fills = blocks[0], np.array([5, -1, -1, 0]), np.array([5, -1, -1, 0])
    _, cnt = h.read()
    assert cnt[0].sum() == 5 and not cnt[1:].any()


# ---- 3. refusals --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_bad_arguments_write_nothing(torch, ctx, vs, dtype):
    lib = ctx._lib
    S, M, W = 2, 100, 128
    h = Harness(torch, ctx, vs, S, M, W, 12, (95.0, 50.0), dtype=dtype, planar=True, reset=False)
    h.upload([np.full((M, 2), 0.25, dtype)] * S, [M] * S, [START] * S)
    state, val, l = h.state.data_ptr(), h.val.data_ptr() + 4 * GUARD, h.chunk.data_ptr()
    levels, cnt, work = h.levels.data_ptr() + h.e * GUARD, h.bin_counts.data_ptr() + 4 * GUARD, h.work.data_ptr()
    snapshot = h.raw_state.clone()
    invalid = [dict(state_bytes=h.need - 1), dict(M=0), dict(M=-5), dict(S=0), dict(S=-1), dict(ss=0), dict(fs=0), dict(fs=-2),
               dict(bins=0), dict(bins=-1), dict(W=-1), dict(W=0), dict(W=M - 1), dict(W=1), dict(M=W + 1, state_bytes=2 ** 40),
               dict(state=0), dict(state=state + 8), dict(l=0), dict(r=0), dict(val=0), dict(counts=0), dict(flags=0),
               dict(edges=0), dict(val=l), dict(val=state + h.need - 4), dict(l=state), dict(r=state),
               dict(val=h.edges.data_ptr()), dict(val=h.counts.data_ptr()), dict(val=h.flags.data_ptr()),
               dict(edges=state + 16), dict(counts=state), dict(ss=2 ** 62), dict(M=2 ** 31, W=2 ** 31), dict(ctx=None),
               dict(scale=0.0), dict(scale=-1.0), dict(scale=float('nan')), dict(scale=float('inf'))]
    invalid += [dict(scale=1e-50), dict(scale=1e39)] if dtype == np.float32 else []       # zero, infinite as float32
    for kw in invalid:
        assert h.raw_push(**kw) == INVALID, kw
        assert lib.vnd_last_error()
    wide = torch.zeros(2048, dtype=torch.float64, device=h.dev)
    unsupported = [dict(S=65536, state_bytes=2 ** 50), dict(W=2 ** 31, state_bytes=2 ** 50), dict(bins=1025, edges=wide.data_ptr()),
                   dict(M=1024 * 129, W=1024 * 129, S=65535, state_bytes=2 ** 50)]        # 129 x 65535 > 2^23 workgroups
    for kw in unsupported:
        assert h.raw_push(**kw) == UNSUPPORTED, (kw, lib.vnd_last_error())
    invalid = [dict(state_bytes=h.need - 1), dict(M=0), dict(S=0), dict(S=-1), dict(bins=0), dict(ps=[]), dict(ps=[50.0], P=0),
               dict(ps=[50.0], P=-1), dict(W=M - 1), dict(W=0), dict(M=2 ** 31, W=2 ** 31), dict(state=0), dict(state=state + 8),
               dict(ps=None, P=2), dict(levels=0), dict(bin_counts=0), dict(work=0), dict(work=work + 4),
               dict(work_bytes=h.work_need - 1), dict(work_bytes=0), dict(ps=[95.0, 100.5]), dict(ps=[-0.1]),
               dict(ps=[float('nan'), 50.0]), dict(levels=state), dict(bin_counts=state + h.need - 4), dict(work=state + 16),
               dict(levels=work), dict(bin_counts=work + h.work_need - 4), dict(bin_counts=levels + 8),
               dict(levels=cnt - 8 * h.e), dict(ctx=None)]
    for kw in invalid:
        assert h.raw_levels(**kw) == INVALID, kw
        assert lib.vnd_last_error()
    big = torch.zeros(2 ** 16, dtype=torch.float64, device=h.dev)
    unsupported = [dict(S=65536, state_bytes=2 ** 50, work_bytes=2 ** 50), dict(W=2 ** 31, state_bytes=2 ** 50, work_bytes=2 ** 50),
                   dict(bins=1025, levels=big.data_ptr(), work_bytes=2 ** 50), dict(ps=[1.0, 2.0, 3.0, 4.0, 5.0], work_bytes=2 ** 50),
                   dict(M=1, W=32768 * 129, S=65535, state_bytes=2 ** 50, work_bytes=2 ** 50)]
    for kw in unsupported:
        assert h.raw_levels(**kw) == UNSUPPORTED, (kw, lib.vnd_last_error())
    null = ctypes.c_void_p(None)
    reset = lib.vnd_polar_level_voice_stream_reset_dev
    is64 = int(h.is64)
    assert reset(ctx.handle, null, h.need, S, M, W, is64, null) == INVALID
    assert reset(ctx.handle, ctypes.c_void_p(state), h.need - 1, S, M, W, is64, null) == INVALID
    assert reset(ctx.handle, ctypes.c_void_p(state + 4), h.need, S, M, W, is64, null) == INVALID
    assert reset(ctx.handle, ctypes.c_void_p(state), h.need, 0, M, W, is64, null) == INVALID
    assert reset(ctx.handle, ctypes.c_void_p(state), h.need, S, M, M - 1, is64, null) == INVALID
    assert reset(null, ctypes.c_void_p(state), h.need, S, M, W, is64, null) == INVALID
    assert reset(ctx.handle, ctypes.c_void_p(state), 2 ** 50, 65536, M, W, is64, null) == UNSUPPORTED
    if not h.is64:                                                    # a float32 state is too small for float64 keys
        assert reset(ctx.handle, ctypes.c_void_p(state), h.need, S, M, W, 1, null) == INVALID
    torch.cuda.synchronize(h.dev)
    assert bool((h.levels == LEVEL_POISON).all()) and bool((h.bin_counts == COUNT_POISON).all()) and bool((h.val == -77).all())
    assert bool((h.work == -1).all())
    assert h.raw_state.cpu().numpy().tobytes() == snapshot.cpu().numpy().tobytes()
    h.reset()
    levels, cnt, valid = h.call([np.full((M, 2), 0.25, dtype)] * S, [M] * S, [START] * S)      # the good call writes
    assert valid.tolist() == [1, 1] and cnt.sum(axis=1).tolist() == [M, M] and (cnt.max(axis=1) == M).all()


# ---- 4. the Python pool behind a decorrelating pool, eager and captured -------------------------------------------------
def _noise(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, n)
    return np.stack([x, 0.6 * x + 0.4 * rng.standard_normal(n)], axis=1).astype(np.float32)


def _pool_and_meter(vs, kind, S, M, W):
    import vndecorrelate_amd.decorrelation as dec
    if kind == 'velvet':
        bank = [dec.VelvetNoise(sample_rate_hz=16000, duration_seconds=0.02, num_impulses=15, seed=1, normalizer=None,
                                log_distribution_strength=k) for k in (0.0, 0.3, 0.55, 1.0)]
    else:
        bank = [dec.HaasEffect(delay_time_seconds=d / 1000, sample_rate_hz=1000, delayed_channel=1, mode='MS', width=0.35)
                for d in (0, 100, 441, 882)]
    pool = dec.decorrelate_voice_pool(bank, slots=S, in_channels=2, max_frames_per_call=M)
    meter = vs.polar_level_voice_pool(S, max_frames_per_call=pool.row_frames, window_frames=W, radius_scale=2.0, num_bins=24,
                                      dtype='float32' if kind == 'velvet' else 'float64')
    per_voice = pool.bank_tables if kind == 'velvet' else pool.bank_delays
    return pool, meter, per_voice


def _pool_schedule(S, M, seed, calls):
    """Every slot starts on call 0 with a voice of its own length, ENDs with its last block and starts the next voice two
    calls later; (x (S, M, 2), counts, flags) per call."""
    rng = np.random.default_rng(seed)
    left, wait, out = [int(v) for v in rng.integers(900, 2200, S)], [0] * S, []
    for i in range(calls):
        x, counts, flags = np.zeros((S, M, 2), np.float32), np.zeros(S, np.int32), np.zeros(S, np.int32)
        for b in range(S):
            if wait[b] > 0:
                wait[b] -= 1
                continue
            if left[b] is None:
                left[b], flags[b] = int(rng.integers(300, 1500)), START
            elif i == 0:
                flags[b] = START
            n = int(min(left[b], rng.choice([0, 1, M, M, int(rng.integers(0, M + 1))])))
            x[b, :n], counts[b] = _noise(n, 1000 * i + b), n
            left[b] -= n
            if left[b] == 0:
                flags[b] |= END
                left[b], wait[b] = None, 2
        out.append((x, counts, flags))
    return out


@pytest.mark.parametrize('kind', ['velvet', 'haas'])
def test_metering_a_decorrelating_pool_with_no_host_read_between(torch, ctx, vs, kind):
    S, M, W = 4, 300, 1200
    pool, meter, per_voice = _pool_and_meter(vs, kind, S, M, W)
    assert W >= pool.row_frames
    dev = torch.device('cuda', ctx.device)
    extra = torch.from_numpy(per_voice[np.array([3, 0, 2, 1])].astype(np.int32)).to(dev)
    pool.reset()
    meter.reset()
    tdt = torch.float32 if kind == 'velvet' else torch.float64
    assert meter.levels.shape == (S, 2, 24) and meter.levels.dtype == tdt and not bool(meter.levels.any())
    assert meter.bin_counts.shape == (S, 24) and meter.bin_counts.dtype == torch.int32
    assert np.array_equal(meter.bin_edges, np.linspace(-90.0, 90.0, 25)) and meter.bin_centers.shape == (24,)
    address = meter.levels.data_ptr()
    positions, voice = np.zeros(S, np.int64), [np.zeros((0, 2), meter.dtype) for _ in range(S)]
    checked = slid = 0
    for i, (xh, c, f) in enumerate(_pool_schedule(S, M, 6, 24)):
        calls = [(xh, c, f)]
        if i == 2:                                                    # a bad count for slot 2: -1 from the pool, -1 here
            bad = np.zeros(S, np.int32)
            bad[2] = M + 1
            calls.insert(0, (xh, bad, np.zeros(S, np.int32)))
        for xh, c, f in calls:
            y, mid = pool.process_dev(torch.from_numpy(xh).to(dev), torch.from_numpy(c).to(dev), torch.from_numpy(f).to(dev),
                                      extra)
            with_levels = i % 3 != 1                                  # every third call pushes only ...
            levels, valid = meter.process_dev(y, mid, torch.from_numpy(f).to(dev), levels=with_levels)
            if not with_levels:
                assert meter.read_dev() is levels                     # ... and reads behind it
            torch.cuda.synchronize(dev)
            assert levels.data_ptr() == address and levels is meter.levels
            given, yh = mid.cpu().numpy(), y.cpu().numpy()
            want, new = vs.scope_voice_spans(positions, given, f, pool.row_frames)
            assert valid.cpu().numpy().tolist() == want.tolist()
            if c[2] == M + 1:
                assert given[2] == -1 and want.tolist() == [0, 0, -1, 0]
            for b in range(S):
                if want[b] == 1:
                    begins = bool(f[b] & START) or positions[b] == 0
                    voice[b] = np.concatenate([voice[b][:0] if begins else voice[b], yh[b, :given[b]]])
                lo, hi = vs.scope_voice_window(len(voice[b]), W)
                if hi > lo:
                    ref, ref_cnt, _, _ = vs.polar_level_batched(torch.from_numpy(voice[b][lo:hi]).to(dev), 24, radius_scale=2.0)
                    assert bool((levels[b] == ref).all()) and bool((meter.bin_counts[b] == ref_cnt).all()), (i, b, lo, hi)
                else:
                    assert not bool(levels[b].any()) and not bool(meter.bin_counts[b].any())
                checked += 1
                slid += lo > 0
            positions = new
    assert checked > 60 and slid > 5
    with pytest.raises(RuntimeError, match='runs through process_dev'):
        meter.process({})


@pytest.mark.parametrize('kind', ['velvet', 'haas'])
def test_graph_replay_equals_the_eager_run(torch, ctx, vs, kind):
    S, M, W = 4, 600, 1500
    dev = torch.device('cuda', ctx.device)
    schedule = _pool_schedule(S, M, 9, 6)
    results = []
    for replayed in (False, True):
        pool, meter, per_voice = _pool_and_meter(vs, kind, S, M, W)
        extra = torch.from_numpy(per_voice[np.array([1, 2, 0, 3])].astype(np.int32)).to(dev)
        x = torch.zeros((S, M, 2), dtype=torch.float32, device=dev)
        counts, flags = (torch.zeros(S, dtype=torch.int32, device=dev) for _ in range(2))
        pool.reset()
        meter.reset()
        graph = None
        if replayed:                                                  # one chain: pool, push, levels - no parallel branches
            graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
            torch.cuda.synchronize(dev)
            with torch.cuda.graph(graph, stream=side):
                y, mid = pool.process_dev(x, counts, flags, extra)
                levels, valid = meter.process_dev(y, mid, flags)
            torch.cuda.synchronize(dev)
            pool.reset()                                              # the capture ran nothing; start both from 0 all the same
            meter.reset()
        got = []
        for xh, c, f in schedule:
            x.copy_(torch.from_numpy(xh))
            counts.copy_(torch.from_numpy(c))
            flags.copy_(torch.from_numpy(f))
            if graph is not None:
                graph.replay()
            else:
                y, mid = pool.process_dev(x, counts, flags, extra)
                levels, valid = meter.process_dev(y, mid, flags)
            torch.cuda.synchronize(dev)
            got.append((levels.cpu().numpy().tobytes(), meter.bin_counts.cpu().numpy().tobytes(), valid.cpu().numpy().tolist(),
                        mid.cpu().numpy().tolist()))
        results.append(got)
    assert results[0] == results[1]
    assert len({g[0] for g in results[1]}) >= 3                       # at least three different inputs and envelopes
    assert all(np.frombuffer(g[1], np.int32).any() for g in results[1])


# ---- 5. the dict form ---------------------------------------------------------------------------------------------------
def test_dict_form_equals_the_batched_levels_of_the_window(torch, ctx, vs):
    S, M, W = 3, 100, 250
    meter = vs.polar_level_voice_pool(S, max_frames_per_call=M, window_frames=W, radius_scale=1.5, num_bins=24,
                                      percentiles=(95.0, 50.0, 5.0))
    rng = np.random.default_rng(12)
    sigs = {0: _noise(730, 1), 2: _noise(411, 2)}
    pushed, first = {s: 0 for s in sigs}, True
    while pushed:
        blocks, end = {}, []
        for s in list(pushed):
            n = int(min(len(sigs[s]) - pushed[s], rng.choice([0, 1, M, int(rng.integers(0, M + 1))])))
            blocks[s] = sigs[s][pushed[s]:pushed[s] + n]
            pushed[s] += n
            if pushed[s] == len(sigs[s]):
                end.append(s)
        out = meter.process(blocks, start=list(sigs) if first else [], end=end)
        assert meter.transfers == {'to_device': 1, 'to_host': 1}
        first = False
        for s, levels in out.items():
            lo, hi = vs.scope_voice_window(pushed[s], W)
            if hi == lo:
                assert not levels.any()
                continue
            want, _, _, _ = vs.polar_level_batched(sigs[s][lo:hi], 24, (95.0, 50.0, 5.0), radius_scale=1.5)
            assert levels.dtype == want.dtype == np.float64 and levels.shape == want.shape == (3, 24)
            assert np.array_equal(levels, want), (s, lo, hi)
        for s in end:
            del pushed[s]
    assert not meter.positions.any() and not meter.live.any()
    only = meter.process({1: sigs[0][:100]}, start=[1], end=[1], levels=False)
    assert only == {1: None} and meter.transfers == {'to_device': 1, 'to_host': 1}
    want, want_cnt, _, _ = vs.polar_level_batched(sigs[0][:100], 24, (95.0, 50.0, 5.0), radius_scale=1.5)
    assert np.array_equal(meter.read_dev()[1].cpu().numpy().astype(np.float64), want)
    assert np.array_equal(meter.bin_counts[1].cpu().numpy().astype(np.int64), want_cnt)
    with pytest.raises(RuntimeError, match='runs through process\\(\\)'):
        meter.process_dev(None, None, None)


# ---- 6. three workgroups a slot -------------------------------------------------------------------------------------------
def span_schedule(M, seed, dtype):
    """Eight calls of three slots with M = 2 spans + 3.  Slot 0 pushes M, M, span, span + 1, span - 1, M, 1, M; slot 1 a
    permutation of these, ENDs on call 3 and STARTs again on call 4; slot 2 a random count in [0, M].  START on call 0, END on
    the last call: whole workgroups leave past n, and the wrap of a ring falls into the first, second and third workgroup."""
    span = (M - 3) // 2
    rng = np.random.default_rng(seed)
    first = [M, M, span, span + 1, span - 1, M, 1, M]
    second = [span + 1, M, 1, M, span - 1, M, span, M]
    assert sorted(first) == sorted(second)
    out = []
    for i in range(8):
        counts = np.array([first[i], second[i], int(rng.integers(0, M + 1))], np.int64)
        flags = np.array([START if i == 0 else 0, START if i in (0, 4) else (END if i == 3 else 0), START if i == 0 else 0],
                         np.int32)
        if i == 7:
            flags |= END
        out.append(([frames(rng, int(c), dtype) for c in counts], counts, flags))
    return out


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('window', ['M', 'M+span+1'])
def test_three_workgroups_a_slot_wrap_an_odd_ring(torch, ctx, vs, window, dtype):
    from vndecorrelate_amd import _native
    span = _native.SCOPE_VOICE_SPAN_FRAMES
    S, M = 3, 2 * span + 3
    assert span == 1024 and -(-M // span) == 3 and M % span == 3
    W = {'M': M, 'M+span+1': M + span + 1}[window]
    h = Harness(torch, ctx, vs, S, M, W, 8, (95.0, 50.0), dtype=dtype)
    for blocks, counts, flags in span_schedule(M, 41 + W, dtype):
        _, _, valid = h.call(blocks, counts, flags)
        assert valid[:2].tolist() == [1, 1] and valid[2] >= 0
    assert h.checked == 8 * S and not h.mirror.any()
    assert h.slid >= 8                                                # the window slid: ring entries were written over
    assert 4 * M + 3 * span + 1 > 2 * W                               # slot 0 went over its ring more than twice
