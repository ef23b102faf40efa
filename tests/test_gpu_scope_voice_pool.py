"""GPU tier of the count-grid voice pool (vnd_polar_hist_voice_stream_* / vnd_lissajous_hist_voice_stream_*,
include/vnd_scope_voice_stream.h; vectorscope.ScopeVoicePool).  Every comparison is of bytes: after EVERY call the grid row of
a slot that answered 1 against the one-shot device entry (vnd_polar_hist_*_dev / vnd_lissajous_hist_*_dev, accumulate = 0) on
the frames of the voice's window.

The harness drives the C ABI on poisoned memory: the positions are NaN bytes until the reset, every ring entry starts as a
VALID cell index (cells - 1) and is never cleared - a stale read shows up as a wrong count and cannot leave the grid - the
chunk rows past counts[b] are NaN, the grid starts as a pattern no voice leaves behind and is never initialised, grid and
valid have guards on both sides (of a size that leaves the rows off 16-byte boundaries) and the state has a poisoned tail.
After every call valid and the device's positions equal the mirror (vectorscope.scope_voice_spans), and the rows and ring
rows of slots that did not answer 1, every guard and the tail are unchanged."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

START, END = 1, 2
GRID_POISON = 0xA5A5A5A5
GUARD = 5                                    # 4-byte values before and after grid and valid: rows begin 4 bytes off
TAIL = 256                                   # poisoned bytes past the state
INVALID, UNSUPPORTED = 1, 4


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


def one_shot(torch, ctx, windows, e0_dev, e1_dev, bins, *, polar, dtype, ms=True, fold=True, scale=1.0):
    """The one-shot device entry with accumulate = 0 on a list of (n, 2) windows, one signal each (n_each: a window of no
    frames is a row of zeros): uint32 (len(windows), cells)."""
    from vndecorrelate_amd import _native
    dev = torch.device('cuda', ctx.device)
    B, n = len(windows), max([1] + [len(w) for w in windows])
    host = np.zeros((B, n, 2), dtype)
    for b, w in enumerate(windows):
        host[b, :len(w)] = w
    x = torch.from_numpy(host).to(dev)
    each = torch.from_numpy(np.array([len(w) for w in windows], np.int32)).to(dev)
    out = torch.full((B, bins[0] * bins[1]), 7, dtype=torch.int32, device=dev)
    e = host.dtype.itemsize
    kw = dict(n_each_ptr=each.data_ptr(), accumulate=False, float64=host.dtype == np.float64,
              stream=torch.cuda.current_stream(dev).cuda_stream)
    args = (ctx, x.data_ptr(), x.data_ptr() + e, B, n, 2 * n, 2, e0_dev.data_ptr(), bins[0], e1_dev.data_ptr(), bins[1],
            out.data_ptr())
    if polar:
        _native.polar_hist_device(*args, ms_mode=ms, semicircular=fold, radius_scale=scale, **kw)
    else:
        _native.lissajous_hist_device(*args, **kw)
    torch.cuda.synchronize(dev)
    return out.cpu().numpy().view(np.uint32)


class Harness:
    """One pool at the C ABI on poisoned memory.  planar: L and R as two (S, M) arrays; else channels of one (S, M, 2)."""

    def __init__(self, torch, ctx, S, M, W, e0, e1, *, polar=True, dtype=np.float32, planar=False, ms=True, fold=True,
                 scale=1.0, reset=True):
        from vndecorrelate_amd import _native
        self.torch, self.ctx, self.native = torch, ctx, _native
        self.dev = torch.device('cuda', ctx.device)
        self.S, self.M, self.W = S, M, W
        self.polar, self.ms, self.fold, self.scale = polar, ms, fold, scale
        self.dtype, self.planar = np.dtype(dtype), planar
        self.e = self.dtype.itemsize
        self.bins = (len(e0) - 1, len(e1) - 1)
        self.cells = self.bins[0] * self.bins[1]
        self.e0 = torch.from_numpy(np.asarray(e0, np.float64).copy()).to(self.dev)
        self.e1 = torch.from_numpy(np.asarray(e1, np.float64).copy()).to(self.dev)
        self.need = _native.scope_voice_stream_state_bytes(S, M, W)
        self.pos_bytes = (8 * S + 15) // 16 * 16
        assert self.need == self.pos_bytes + (S * W * 4 + 15) // 16 * 16
        self.raw_state = torch.full(((self.need + TAIL) // 4,), float('nan'), dtype=torch.float32, device=self.dev)
        self.state = self.raw_state[:self.need // 4]
        if W:
            self.ring_view().fill_(self.cells - 1)
        self.tdt = torch.float32 if self.dtype == np.float32 else torch.float64
        self.chunk = torch.empty((2, S, M) if planar else (S, M, 2), dtype=self.tdt, device=self.dev)
        self.counts, self.flags = (torch.empty(S, dtype=torch.int32, device=self.dev) for _ in range(2))
        self.grid = torch.from_numpy(np.full(S * self.cells + 2 * GUARD, GRID_POISON, np.uint32).view(np.int32)).to(self.dev)
        self.val = torch.empty((S + 2 * GUARD,), dtype=torch.int32, device=self.dev)
        self.expect = np.full(S * self.cells + 2 * GUARD, GRID_POISON, np.uint32)     # what the grid memory must hold
        self.frames = [np.zeros((0, 2), self.dtype) for _ in range(S)]                # the frames of the slot's voice ...
        self.origin = [0] * S                                                         # ... from this absolute position on
        self.mirror = None                                   # the positions, once they are known
        self.checked = self.slid = 0
        if reset:
            self.reset()

    def stream(self):
        return self.torch.cuda.current_stream(self.dev).cuda_stream

    def reset(self):
        self.native.scope_voice_stream_reset_device(self.ctx, self.state.data_ptr(), self.need, self.S, self.M, self.W,
                                                    stream=self.stream())
        self.mirror = np.zeros(self.S, np.int64)

    # ---- the parts of the state ---------------------------------------------------------------------------------------
    def positions_view(self):
        return self.state[:2 * self.S].view(self.torch.int64)

    def ring_view(self):
        at = self.pos_bytes // 4
        return self.state[at:at + self.S * self.W].view(self.torch.int32).view(self.S, self.W)

    def positions(self):
        return self.positions_view().cpu().numpy().copy()

    def ring(self):
        return self.ring_view().cpu().numpy().copy() if self.W else np.zeros((self.S, 0), np.int32)

    def rest_is_poison(self):
        """The ring's padding and the tail past the state."""
        return bool(self.torch.isnan(self.raw_state[(self.pos_bytes + 4 * self.S * self.W) // 4:]).all())

    def rows(self):
        return self.grid.cpu().numpy().view(np.uint32)[GUARD:GUARD + self.S * self.cells].reshape(self.S, self.cells).copy()

    def plant(self, b, position, like):
        """Slot b as slot `like` would be at `position`: its ring row, its grid row and its voice's frames."""
        self.positions_view()[b] = position
        self.ring_view()[b] = self.ring_view()[like]
        lo = GUARD + self.cells * np.array([b, like])
        self.grid[lo[0]:lo[0] + self.cells] = self.grid[lo[1]:lo[1] + self.cells]
        self.expect[lo[0]:lo[0] + self.cells] = self.expect[lo[1]:lo[1] + self.cells]
        self.frames[b], self.origin[b] = self.frames[like].copy(), position - len(self.frames[like])
        self.mirror[b] = position

    # ---- calls ------------------------------------------------------------------------------------------------------
    def raw(self, **kw):
        """The C call with pointers and scalars replaced by name; returns the status."""
        lib = self.ctx._lib
        if self.planar:
            l, r, ss, fs = self.chunk[0].data_ptr(), self.chunk[1].data_ptr(), self.M, 1
        else:
            l, r, ss, fs = self.chunk.data_ptr(), self.chunk.data_ptr() + self.e, 2 * self.M, 2
        a = dict(state=self.state.data_ptr(), state_bytes=self.need, M=self.M, W=self.W, l=l, r=r, ss=ss, fs=fs,
                 counts=self.counts.data_ptr(), flags=self.flags.data_ptr(), ms=int(self.ms), fold=int(self.fold),
                 scale=self.scale, e0=self.e0.data_ptr(), b0=self.bins[0], e1=self.e1.data_ptr(), b1=self.bins[1],
                 grid=self.grid.data_ptr() + 4 * GUARD, val=self.val.data_ptr() + 4 * GUARD, S=self.S, ctx=self.ctx.handle)
        a.update(kw)
        name = f"vnd_{'polar' if self.polar else 'lissajous'}_hist_voice_stream_{'f64' if self.e == 8 else 'f32'}_dev"
        p = ctypes.c_void_p
        head = (a['ctx'], p(a['state']), a['state_bytes'], a['M'], a['W'], p(a['l']), p(a['r']), a['ss'], a['fs'],
                p(a['counts']), p(a['flags']))
        mode = (a['ms'], a['fold'], ctypes.c_double(a['scale'])) if self.polar else ()
        return getattr(lib, name)(*head, *mode, p(a['e0']), a['b0'], p(a['e1']), a['b1'], p(a['grid']), p(a['val']), a['S'],
                                  p(self.stream()))

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

    def call(self, blocks, counts, flags):
        """One call; checks valid, the positions, every answered row against the one-shot entry on its window and the rest
        of the memory against what it held; returns (rows (S, cells) uint32, valid)."""
        from vndecorrelate_amd.vectorscope import scope_voice_spans, scope_voice_window
        self.upload(blocks, counts, flags)
        ring_before = self.ring()
        assert self.raw() == 0, self.ctx._lib.vnd_last_error()
        self.torch.cuda.synchronize(self.dev)
        want, new = scope_voice_spans(self.mirror, counts, flags, self.M)
        val = self.val.cpu().numpy()
        assert (val[:GUARD] == -77).all() and (val[GUARD + self.S:] == -77).all()
        assert val[GUARD:GUARD + self.S].tolist() == want.tolist(), (counts, flags, self.mirror)
        assert self.positions().tolist() == new.tolist()
        answered, windows = [], []
        for b in range(self.S):
            if want[b] != 1:
                continue
            p = 0 if int(flags[b]) & START else int(self.mirror[b])
            block = np.asarray(blocks[b], self.dtype).reshape(-1, 2) if blocks[b] is not None else np.zeros((0, 2), self.dtype)
            assert len(block) == counts[b]
            if p == 0:
                self.frames[b], self.origin[b] = block.copy(), 0
            else:
                self.frames[b] = np.concatenate([self.frames[b], block])
            lo, hi = scope_voice_window(p + len(block), self.W)
            assert hi - self.origin[b] == len(self.frames[b]) and lo >= self.origin[b]
            if self.W and lo > self.origin[b] + 2 * self.W:                          # keep what a later window can need
                cut = lo - self.origin[b] - self.W
                self.frames[b], self.origin[b] = self.frames[b][cut:], self.origin[b] + cut
            answered.append(b)
            windows.append(self.frames[b][lo - self.origin[b]:])
            self.slid += lo > 0
        if answered:
            ref = one_shot(self.torch, self.ctx, windows, self.e0, self.e1, self.bins, polar=self.polar, dtype=self.dtype,
                           ms=self.ms, fold=self.fold, scale=self.scale)
            for b, row in zip(answered, ref):
                self.expect[GUARD + b * self.cells:GUARD + (b + 1) * self.cells] = row
            self.checked += len(answered)
        got = self.grid.cpu().numpy().view(np.uint32)
        if got.tobytes() != self.expect.tobytes():
            wrong = np.flatnonzero(got != self.expect)
            raise AssertionError(f'grid memory differs at {wrong[:8]} (slot {(wrong[0] - GUARD) // self.cells}): '
                                 f'{got[wrong[:8]]} != {self.expect[wrong[:8]]}; counts {counts}, flags {flags}, '
                                 f'positions {self.mirror}')
        ring_after = self.ring()
        for b in range(self.S):
            if want[b] != 1:
                assert ring_after[b].tobytes() == ring_before[b].tobytes(), b
        assert self.rest_is_poison()
        self.mirror = new
        return got[GUARD:GUARD + self.S * self.cells].reshape(self.S, self.cells).copy(), want


def frames(rng, n, dtype):
    """Gaussian frames with sigma 0.5: with radius_scale 1 about e^-2 of them lie past the radius range and are dropped."""
    x = rng.normal(0.0, 0.5, (n, 2))
    if np.dtype(dtype) == np.float64:
        x = x * (1 + 1e-9)                                            # values between float32 ones
    x = x.astype(dtype)
    if n > 4 and rng.random() < 0.5:                                  # frames the binning rule drops, and exact edges
        x[0, 0] = np.nan
        x[1] = (np.inf, 1.0)
        x[2] = (0.5, -np.inf)
        x[3] = (0.25, -0.25)                                          # R = -L, L > 0: +90 degrees, the last edge
        x[4] = (0.0, 0.0)
    return x


def fuzz_schedule(S, M, seed, dtype, calls=40):
    """(blocks, counts, flags) per call.  Slot 0: END, a new voice with START, END, a voice from position 0 without START;
    slot 1: a discard-START mid-voice; slot 2: whole voices in one call; slot 4 (if any) starts late and ENDs with no
    frames; the last slot is fed M + 1 and -1; call 9 is idle for every slot; the last call ENDs every voice."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(calls):
        counts = np.array([int(rng.choice([0, 1, M - 1, M, int(rng.integers(0, M + 1))])) for _ in range(S)], np.int64)
        flags = np.zeros(S, np.int32)
        if i == 0:
            flags[:] = START
        if i == 9:
            counts[:] = 0
        if i in (12, 25):
            flags[0] |= END
        if i in (13, 26):
            counts[0] = 0
        if i == 14:
            flags[0] |= START
        if i == 15:
            flags[1] |= START
        if i in (5, 6):
            flags[2] |= START | END
        if S > 4:
            if i < 3 or 18 <= i < 22:
                counts[4], flags[4] = 0, 0
            if i == 3:
                flags[4] = START
            if i == 18:
                flags[4] = END
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


def run_schedule(h, schedule):
    seen = []
    for blocks, counts, flags in schedule:
        rows, valid = h.call(blocks, counts, flags)
        seen.append((rows.tobytes(), valid.tolist()))
    return seen


UNEVEN = (np.array([-90.0, -80.0, -45.0, -44.0, -10.0, 0.0, 0.5, 7.0, 30.0, 31.0, 60.0, 89.0, 90.0]),
          np.array([0.0, 0.01, 0.1, 0.3, 0.35, 0.6, 0.9, 1.0]))


def polar_12x7(vs):
    return vs.polar_edges(12, 7)


# ---- 1. the schedule fuzz ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ms_fold', [(True, True), (False, False)], ids=['MS-fold', 'LR-nofold'])
@pytest.mark.parametrize('planar', [False, True], ids=['channels', 'planar'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('W', [0, 37, 64, 1000])
def test_schedule_fuzz(torch, ctx, vs, W, dtype, planar, ms_fold):
    S, M = 6, 37
    h = Harness(torch, ctx, S, M, W, *polar_12x7(vs), dtype=dtype, planar=planar, ms=ms_fold[0], fold=ms_fold[1])
    seen = run_schedule(h, fuzz_schedule(S, M, 11 + W, dtype))
    valid = np.array([v for _, v in seen])
    assert (valid[:, S - 1] == -1).sum() == 3 and (valid[:, :S - 1] >= 0).all()
    assert (valid[9] == 0).all() and h.checked > 120
    assert W == 0 or W == 1000 or h.slid > 40                        # the window slid
    assert not W or (h.ring() == -1).any()                           # dropped frames went through the ring
    assert not h.positions().any()


def test_schedule_fuzz_uneven_edges(torch, ctx, vs):
    S, M = 6, 37
    h = Harness(torch, ctx, S, M, 64, *UNEVEN)
    run_schedule(h, fuzz_schedule(S, M, 5, np.float32))
    assert h.checked > 120 and h.slid > 40


# ---- 2. Lissajous -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bins', [(16, 16), (5, 3)], ids=['16x16', '5x3'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_lissajous_schedule_fuzz(torch, ctx, vs, dtype, bins):
    S, M = 4, 37
    h = Harness(torch, ctx, S, M, 64, *vs.lissajous_edges(bins, ((-1.1, 1.1), (-1.0, 0.9))), polar=False, dtype=dtype)
    run_schedule(h, fuzz_schedule(S, M, 21, dtype))
    assert h.checked > 80 and h.slid > 30
    whole = Harness(torch, ctx, S, M, 0, *vs.lissajous_edges(bins), polar=False, dtype=dtype, planar=True)
    run_schedule(whole, fuzz_schedule(S, M, 22, dtype, calls=20))


def test_lissajous_512x512(torch, ctx, vs):
    S, M, W = 2, 64, 128
    h = Harness(torch, ctx, S, M, W, *vs.lissajous_edges(512), polar=False)
    rng = np.random.default_rng(3)
    for i in range(9):
        counts = [M, int(rng.integers(0, M + 1))]
        flags = [(START if i in (0, 6) else 0) | (END if i == 8 else 0), START if i == 0 else (END if i == 4 else 0)]
        h.call([frames(rng, c, np.float32) for c in counts], counts, flags)
    assert h.slid >= 4


# ---- 3. the default grid ------------------------------------------------------------------------------------------------
def test_default_grid_window_slides_over_the_ring_twice(torch, ctx, vs):
    S, M, W = 3, 480, 4800
    h = Harness(torch, ctx, S, M, W, *vs.polar_edges())
    rng = np.random.default_rng(8)
    for i in range(25):
        counts = [M, int(rng.choice([M, M - 1, 0, int(rng.integers(0, M + 1))])), M]
        flags = [START if i == 0 else 0, START if i == 0 else 0, START if i in (0, 13) else 0]
        h.call([frames(rng, c, np.float32) for c in counts], counts, flags)
    assert h.mirror[0] == 25 * M > 2 * W and h.slid >= 15


# ---- 4. positions past 2^32 ---------------------------------------------------------------------------------------------
def test_a_planted_position_past_2_to_32_continues_as_the_voice_would(torch, ctx, vs):
    S, M, W = 2, 37, 64
    h = Harness(torch, ctx, S, M, W, *polar_12x7(vs))
    rng = np.random.default_rng(4)
    for i in range(3):
        h.call([frames(rng, M, np.float32), None], [M, 0], [START if i == 0 else 0, 0])
    q, far = 3 * M, 3 * M + 2 ** 34 * W
    assert q >= W
    h.plant(1, far, like=0)
    for i in range(10):
        n = int(rng.choice([M, 1, M - 1, int(rng.integers(0, M + 1))]))
        block = frames(rng, n, np.float32)
        rows, valid = h.call([block, block], [n, n], [0, 0])
        q += n
        assert rows[0].tobytes() == rows[1].tobytes(), i
        pos = h.positions()
        assert pos.tolist() == [q, q + 2 ** 34 * W] and valid.tolist() == [1 if n else 0] * 2
    assert h.ring()[0].tobytes() == h.ring()[1].tobytes()


# ---- 5. determinism -----------------------------------------------------------------------------------------------------
def test_two_runs_of_the_fuzz_schedule_are_byte_equal(torch, ctx, vs):
    S, M = 6, 37
    runs = []
    for _ in range(2):
        h = Harness(torch, ctx, S, M, 64, *polar_12x7(vs))
        runs.append(run_schedule(h, fuzz_schedule(S, M, 77, np.float32)))
    assert runs[0] == runs[1]


# ---- 6. behind a decorrelating pool, eager and captured -----------------------------------------------------------------
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
    meter = vs.polar_histogram_voice_pool(S, max_frames_per_call=pool.row_frames, radius_scale=2.0, num_angle_bins=24,
                                          num_radius_bins=10, window_frames=W,
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
    assert meter.grid.shape == (S, 24, 10) and meter.grid.dtype == torch.int32 and not bool(meter.grid.any())
    address = meter.grid.data_ptr()
    positions, voice = np.zeros(S, np.int64), [np.zeros((0, 2), meter.dtype) for _ in range(S)]
    schedule = _pool_schedule(S, M, 6, 30)
    checked = slid = 0
    for i, (xh, c, f) in enumerate(schedule):
        calls = [(xh, c, f)]
        if i == 2:                                                    # a bad count for slot 2: -1 from the pool, -1 here
            bad = np.zeros(S, np.int32)
            bad[2] = M + 1
            calls.insert(0, (xh, bad, np.zeros(S, np.int32)))
        for xh, c, f in calls:
            before = meter.grid.clone()
            y, mid = pool.process_dev(torch.from_numpy(xh).to(dev), torch.from_numpy(c).to(dev), torch.from_numpy(f).to(dev),
                                      extra)
            grid, valid = meter.process_dev(y, mid, torch.from_numpy(f).to(dev))
            torch.cuda.synchronize(dev)
            assert grid.data_ptr() == address
            given, yh = mid.cpu().numpy(), y.cpu().numpy()
            want, new = vs.scope_voice_spans(positions, given, f, pool.row_frames)
            assert valid.cpu().numpy().tolist() == want.tolist()
            if c[2] == M + 1:
                assert given[2] == -1 and want.tolist() == [0, 0, -1, 0] and bool((grid == before).all())
            for b in range(S):
                if want[b] != 1:
                    assert bool((grid[b] == before[b]).all())
                    continue
                begins = bool(f[b] & START) or positions[b] == 0
                voice[b] = np.concatenate([voice[b][:0] if begins else voice[b], yh[b, :given[b]]])
                lo, hi = vs.scope_voice_window(len(voice[b]), W)
                if hi > lo:
                    ref, _, _ = vs.polar_histogram_batched(torch.from_numpy(voice[b][lo:hi]).to(dev), 24, 10, radius_scale=2.0)
                    assert bool((grid[b] == ref).all()), (i, b, lo, hi)
                else:
                    assert not bool(grid[b].any())
                checked += 1
                slid += lo > 0
            positions = new
    assert checked > 30 and slid > 5
    with pytest.raises(RuntimeError, match='runs through process_dev'):
        meter.process({})


def test_graph_replay_equals_the_eager_run(torch, ctx, vs):
    S, M, W = 4, 600, 1500
    dev = torch.device('cuda', ctx.device)
    schedule = _pool_schedule(S, M, 9, 6)
    results = []
    for replayed in (False, True):
        pool, meter, per_voice = _pool_and_meter(vs, 'velvet', S, M, W)
        extra = torch.from_numpy(per_voice[np.array([1, 2, 0, 3])].astype(np.int32)).to(dev)
        x = torch.zeros((S, M, 2), dtype=torch.float32, device=dev)
        counts, flags = (torch.zeros(S, dtype=torch.int32, device=dev) for _ in range(2))
        pool.reset()
        meter.reset()
        graph = None
        if replayed:                                                  # one chain: pool, then meter, no parallel branches
            graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
            torch.cuda.synchronize(dev)
            with torch.cuda.graph(graph, stream=side):
                y, mid = pool.process_dev(x, counts, flags, extra)
                grid, valid = meter.process_dev(y, mid, flags)
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
                grid, valid = meter.process_dev(y, mid, flags)
            torch.cuda.synchronize(dev)
            got.append((grid.cpu().numpy().tobytes(), valid.cpu().numpy().tolist(), mid.cpu().numpy().tolist()))
        results.append(got)
    assert len(results[1]) >= 5 and results[0] == results[1]
    assert any(np.frombuffer(g, np.int32).any() for g, _, _ in results[1])


# ---- 7. the dict form ---------------------------------------------------------------------------------------------------
def test_dict_form_equals_the_batched_histogram_of_the_window(torch, ctx, vs):
    S, M, W = 3, 100, 250
    meter = vs.polar_histogram_voice_pool(S, max_frames_per_call=M, radius_scale=1.5, num_angle_bins=24, num_radius_bins=10,
                                          window_frames=W)
    rng = np.random.default_rng(12)
    sigs = {0: _noise(730, 1), 2: _noise(411, 2)}
    pushed, first = {s: 0 for s in sigs}, True
    vs.set_scope_device(False)                                        # the reference below: the NumPy route
    try:
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
            for s, grid in out.items():
                lo, hi = vs.scope_voice_window(pushed[s], W)
                want, _, _ = vs.polar_histogram_batched(sigs[s][lo:hi], 24, 10, radius_scale=1.5)
                assert grid.dtype == want.dtype == np.float64 and grid.shape == want.shape == (24, 10)
                assert np.array_equal(grid, want), (s, lo, hi, int(np.abs(grid - want).sum()))
            for s in end:
                del pushed[s]
    finally:
        vs.set_scope_device(None)
    assert not meter.positions.any() and not meter.live.any()
    only = meter.process({1: sigs[0][:100]}, start=[1], end=[1], grids=False)
    assert only == {1: None} and meter.transfers == {'to_device': 1, 'to_host': 1}
    assert int(meter.grid[1].sum()) <= 100 and bool(meter.grid[1].any())
    with pytest.raises(RuntimeError, match='runs through process\\(\\)'):
        meter.process_dev(None, None, None)


# ---- 8. refusals --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('polar', [True, False], ids=['polar', 'lissajous'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_bad_arguments_write_nothing(torch, ctx, vs, dtype, polar):
    lib = ctx._lib
    S, M, W = 2, 100, 128
    edges = polar_12x7(vs) if polar else vs.lissajous_edges((12, 7))
    h = Harness(torch, ctx, S, M, W, *edges, polar=polar, dtype=dtype, planar=True, reset=False)
    h.upload([np.full((M, 2), 0.25, dtype)] * S, [M] * S, [START] * S)
    state, grid, val, l = h.state.data_ptr(), h.grid.data_ptr() + 4 * GUARD, h.val.data_ptr() + 4 * GUARD, h.chunk.data_ptr()
    snapshot = h.raw_state.clone()
    invalid = [dict(state_bytes=h.need - 1), dict(M=0), dict(M=-5), dict(S=0), dict(S=-1), dict(ss=0), dict(fs=0), dict(fs=-2),
               dict(b0=0), dict(b1=-1), dict(W=-1), dict(W=M - 1), dict(W=1), dict(M=W + 1, state_bytes=2 ** 40),
               dict(state=0), dict(state=state + 8), dict(l=0), dict(r=0), dict(grid=0), dict(val=0), dict(counts=0),
               dict(flags=0), dict(e0=0), dict(e1=0), dict(grid=grid + 2), dict(grid=l), dict(val=l), dict(grid=state),
               dict(val=state + h.need - 4), dict(l=state), dict(r=state), dict(val=grid + 8), dict(grid=val - 60),
               dict(grid=h.e0.data_ptr()), dict(val=h.e1.data_ptr()), dict(grid=h.counts.data_ptr()),
               dict(val=h.flags.data_ptr()), dict(ss=2 ** 62), dict(M=2 ** 31, W=2 ** 31), dict(ctx=None)]
    if polar:
        invalid += [dict(scale=0.0), dict(scale=-1.0), dict(scale=float('nan')), dict(scale=float('inf'))]
        invalid += [dict(scale=1e-50), dict(scale=1e39)] if dtype == np.float32 else []       # zero, infinite as float32
    for kw in invalid:
        assert h.raw(**kw) == INVALID, kw
        assert lib.vnd_last_error()
    # (a grid and edges of 4097 bins reach past the harness's: memory of their own, so that nothing overlaps)
    big, wide = (torch.zeros(2 ** 18, dtype=dt, device=h.dev) for dt in (torch.int32, torch.float64))
    unsupported = [dict(S=65536, state_bytes=2 ** 50), dict(W=2 ** 31, state_bytes=2 ** 50),
                   dict(b0=4097, grid=big.data_ptr(), e0=wide.data_ptr()), dict(b1=4097, grid=big.data_ptr(), e1=wide.data_ptr()),
                   dict(M=1024 * 129, W=1024 * 129, S=65535, state_bytes=2 ** 50)]        # 129 x 65535 > 2^23 workgroups
    for kw in unsupported:
        assert h.raw(**kw) == UNSUPPORTED, (kw, lib.vnd_last_error())
    null = ctypes.c_void_p(None)
    reset = lib.vnd_scope_voice_stream_reset_dev
    assert reset(ctx.handle, null, h.need, S, M, W, null) == INVALID
    assert reset(ctx.handle, ctypes.c_void_p(state), h.need - 1, S, M, W, null) == INVALID
    assert reset(ctx.handle, ctypes.c_void_p(state + 4), h.need, S, M, W, null) == INVALID
    assert reset(ctx.handle, ctypes.c_void_p(state), h.need, 0, M, W, null) == INVALID
    assert reset(ctx.handle, ctypes.c_void_p(state), h.need, S, M, M - 1, null) == INVALID
    assert reset(null, ctypes.c_void_p(state), h.need, S, M, W, null) == INVALID
    assert reset(ctx.handle, ctypes.c_void_p(state), 2 ** 50, 65536, M, W, null) == UNSUPPORTED
    torch.cuda.synchronize(h.dev)
    assert h.grid.cpu().numpy().view(np.uint32).tobytes() == h.expect.tobytes() and bool((h.val == -77).all())
    assert h.raw_state.cpu().numpy().tobytes() == snapshot.cpu().numpy().tobytes()
    h.reset()
    rows, valid = h.call([np.full((M, 2), 0.25, dtype)] * S, [M] * S, [START] * S)       # the good call writes
    assert valid.tolist() == [1, 1] and rows.sum(axis=1).tolist() == [M, M] and (rows.max(axis=1) == M).all()


# ---- 9. three workgroups a slot -------------------------------------------------------------------------------------------
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
@pytest.mark.parametrize('window', ['M', 'M+span+1', 'whole'])
def test_three_workgroups_a_slot_wrap_an_odd_ring(torch, ctx, vs, window, dtype):
    from vndecorrelate_amd import _native
    span = _native.SCOPE_VOICE_SPAN_FRAMES
    S, M = 3, 2 * span + 3
    assert span == 1024 and -(-M // span) == 3 and M % span == 3
    W = {'M': M, 'M+span+1': M + span + 1, 'whole': 0}[window]
    h = Harness(torch, ctx, S, M, W, *polar_12x7(vs), dtype=dtype)
    seen = run_schedule(h, span_schedule(M, 31 + W, dtype))
    assert all(v[:2] == [1, 1] and v[2] >= 0 for _, v in seen) and h.checked >= 16
    assert not h.positions().any()
    if W:
        assert h.slid >= 8                                            # the window slid: frames left through the ring
        assert 4 * M + 3 * span + 1 > 2 * W                           # slot 0 went over its ring more than twice
