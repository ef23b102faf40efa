"""GPU tier of the polar-moments voice pool (vnd_polar_voice_stream_f32_dev / _f64_dev, include/vnd_polar_voice_stream.h;
analysis.PolarVoicePool).  The float32 comparisons are of the float64 bits of the eight moments, against the one-shot
device call vnd_polar_moments_f32_dev with one pair on each voice's frames so far, after EVERY call.

The harness drives the C ABI on poisoned memory: ring, lane sums and partials are NaN and are never cleared, the positions
are NaN bytes until the reset, the chunk rows past counts[b] are NaN, `moments` and `valid` hold patterns no kernel writes
with guards on both sides, and the state has a poisoned tail.  After every call valid and the device's positions equal the
mirror (analysis.polar_voice_spans), the rows of slots that did not answer 1 are untouched and so is every guard."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

START, END = 1, 2
POISON = 0x7FF4A5A5A5A5A5A5                  # a signalling NaN: no kernel arithmetic yields it
GUARD = 16                                   # values before and after moments and valid
TAIL = 256                                   # poisoned bytes past the state
INVALID, UNSUPPORTED = 1, 4
SUM_REL = 1e-12             # tests/test_gpu_haas_scan.py: a float64 moment sum against NumPy's, relative to sum |term|
THETA_ABS = 4e-15           # tests/test_gpu_haas_scan.py: max |theta| in float64, a few ulps of pi/2
F32_SUM_REL = 3e-8          # tests/test_gpu_optimization.py::test_moments_kernel_against_numpy: on the scale of the terms
F32_THETA_ABS = 2.4e-7      # ... and one float32 ulp on max |theta|
SCORE_TOL = 2e-4            # tests/test_gpu_optimization.py's constant, what grid_scan is held to
WEIGHTS = dict(angle_limit=np.pi / 4, lambda_mean=5.0, lambda_skew=2.0, lambda_correlation=15.0, lambda_penalty=1e3)


@pytest.fixture(scope='module')
def ctx():
    from vndecorrelate_amd import _native
    context = _native.default_context()
    assert 'gfx950' in context.info()['name']
    return context


@pytest.fixture(scope='module')
def an(ctx):
    from vndecorrelate_amd import analysis
    return analysis


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float64 and a.tobytes() == b.tobytes()


_one_shot_cache = {}


def one_shot(ctx, x):
    """vnd_polar_moments_f32_dev with n_pairs = 1 on a float32 (n, 2) signal: float64 (8,)."""
    import torch
    from vndecorrelate_amd import _native
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 2)
    key = x.tobytes()
    if key not in _one_shot_cache:
        dev = torch.device('cuda', ctx.device)
        n = len(x)
        y = torch.from_numpy(x if n else np.zeros((1, 2), np.float32)).to(dev)
        ws = _native.polar_moments_workspace_bytes(n, 1)
        work = torch.empty(ws, dtype=torch.uint8, device=dev)
        out = torch.full((8,), -1.0, dtype=torch.float64, device=dev)
        _native.polar_moments_device(ctx, y.data_ptr(), n, 1, out.data_ptr(), work.data_ptr(), ws,
                                     torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        _one_shot_cache[key] = out.cpu().numpy()
    return _one_shot_cache[key]


def check_f64_against_numpy(row, y, what):
    """tests/test_gpu_haas_scan.py's check_row: float64 NumPy terms as the reference's polar_coordinates computes them."""
    l, r = y[:, 0], y[:, 1]
    th = np.arctan2(l - r, l + r)
    th = np.where(th < -np.pi / 2, th + np.pi, np.where(th > np.pi / 2, th - np.pi, th))
    rad = np.sqrt(l ** 2 + r ** 2)
    for k, t in enumerate([rad, rad * th, rad * th * th, rad * th * th * th, None, l * r, l * l, r * r]):
        if t is None:
            want = float(np.max(np.abs(th))) if th.size else 0.0
            assert abs(row[4] - want) <= THETA_ABS, (what, k, row[4], want)
            continue
        bound = SUM_REL * float(np.sum(np.abs(t))) + 1e-300
        assert abs(row[k] - float(np.sum(t))) <= bound, (what, k, row[k], float(np.sum(t)), bound)


def _moments64(y):
    """tests/test_gpu_optimization.py's: float32 element maths as NumPy, float64 sums."""
    left, right = y[:, 0], y[:, 1]
    th = np.arctan2(left - right, left + right)
    th = np.where(th < -np.pi / 2, th + np.pi, np.where(th > np.pi / 2, th - np.pi, th))
    r = np.sqrt(left**2 + right**2)
    assert th.dtype == np.float32 and r.dtype == np.float32
    d = np.float64
    return np.array([r.sum(dtype=d), (r * th).sum(dtype=d), (r * th**2).sum(dtype=d), (r * (th**2 * th)).sum(dtype=d),
                     np.max(np.abs(th)) if len(th) else 0.0, (left * right).sum(dtype=d), (left * left).sum(dtype=d),
                     (right * right).sum(dtype=d)])


def check_f32_against_numpy(row, y, what):
    """The bars of tests/test_gpu_optimization.py::test_moments_kernel_against_numpy, as that test forms them."""
    want = _moments64(y)
    scale = _moments64(np.abs(y) * np.array([1.0, 0.5], np.float32))
    scale[1:4] = want[0] * np.array([np.pi / 2, (np.pi / 2) ** 2, (np.pi / 2) ** 3])
    assert np.all(np.abs(row - want) <= F32_SUM_REL * np.maximum(scale, 1.0)), (what, row, want)
    assert row[4] == want[4] or abs(row[4] - want[4]) <= F32_THETA_ABS, (what, row[4], want[4])


class Harness:
    """One pool at the C ABI on poisoned memory.  planar: L and R as two (S, M) arrays; else channels of one (S, M, 2)."""

    def __init__(self, torch, ctx, S, M, dtype=np.float32, planar=False, reset=True):
        from vndecorrelate_amd import _native
        self.torch, self.ctx, self.native = torch, ctx, _native
        self.dev = torch.device('cuda', ctx.device)
        self.S, self.M = S, M
        self.dtype, self.planar = np.dtype(dtype), planar
        self.e = self.dtype.itemsize
        self.G = -(-M // 512) + 1
        self.cap = 511 + M
        self.need = _native.polar_voice_stream_state_bytes(S, M, self.e)
        self.pos_bytes = (8 * S + 15) // 16 * 16
        self.sums_at = self.pos_bytes
        self.partials_at = self.sums_at + S * 256 * 64
        self.ring_at = self.partials_at + S * self.G * 64
        assert self.need == self.ring_at + S * self.cap * 2 * self.e and self.need % 8 == 0
        plan = dict(f.split('=') for f in _native.describe_polar_voice_stream(S, M, self.e).split()[1:])
        assert (int(plan['groups']), int(plan['nblocks']), int(plan['finish_groups']), int(plan['state_bytes'])) == \
            (self.G, S * self.G, S, self.need)
        self.raw_state = torch.full(((self.need + TAIL) // 4,), float('nan'), dtype=torch.float32, device=self.dev)
        self.state = self.raw_state[:self.need // 4]
        self.tdt = torch.float32 if self.dtype == np.float32 else torch.float64
        self.chunk = torch.empty((2, S, M) if planar else (S, M, 2), dtype=self.tdt, device=self.dev)
        self.counts, self.flags = (torch.empty(S, dtype=torch.int32, device=self.dev) for _ in range(2))
        self.mom = torch.empty((S * 8 + 2 * GUARD,), dtype=torch.int64, device=self.dev)
        self.val = torch.empty((S + 2 * GUARD,), dtype=torch.int32, device=self.dev)
        self.mirror = None                                   # the positions, once they are known
        if reset:
            self.reset()

    def stream(self):
        return self.torch.cuda.current_stream(self.dev).cuda_stream

    def reset(self):
        self.native.polar_voice_stream_reset_device(self.ctx, self.state.data_ptr(), self.need, self.S, self.M, self.e,
                                                    stream=self.stream())
        self.mirror = np.zeros(self.S, np.int64)

    # ---- the parts of the state ---------------------------------------------------------------------------------------
    def positions_view(self):
        return self.state[:2 * self.S].view(self.torch.int64)

    def sums_view(self):
        return self.state[self.sums_at // 4:self.partials_at // 4].view(self.torch.float64).view(self.S, 256, 8)

    def ring_view(self):
        return self.state[self.ring_at // 4:].view(self.tdt).view(self.S, self.cap, 2)

    def positions(self):
        return self.positions_view().cpu().numpy().copy()

    def slot_state(self, b):
        """The bytes of slot b's position, lane sums and ring."""
        return (self.positions_view()[b:b + 1].cpu().numpy().tobytes(), self.sums_view()[b].cpu().numpy().tobytes(),
                self.ring_view()[b].cpu().numpy().tobytes())

    def plant(self, b, position, lanes=None, pending=None):
        """Slot b at `position` with these lane sums and the frames [position - len(pending), position) in their ring
        slots (Python integers)."""
        torch = self.torch
        self.positions_view()[b] = position
        if lanes is not None:
            self.sums_view()[b] = torch.from_numpy(np.asarray(lanes, np.float64)).to(self.dev)
        if pending is not None and len(pending):
            where = np.array([(position - len(pending) + j) % self.cap for j in range(len(pending))], np.int64)
            self.ring_view()[b, torch.from_numpy(where).to(self.dev)] = torch.from_numpy(np.asarray(pending, self.dtype)).to(self.dev)
        self.mirror[b] = position

    def pending(self, b):
        """The frames of slot b's incomplete chunk, read from the ring at the device's own position."""
        p = int(self.positions()[b])
        where = np.array([(p - p % 512 + j) % self.cap for j in range(p % 512)], np.int64)
        return self.ring_view()[b].cpu().numpy()[where]

    # ---- calls ------------------------------------------------------------------------------------------------------
    def raw(self, **kw):
        """The C call with pointers and scalars replaced by name; returns the status."""
        lib = self.ctx._lib
        if self.planar:
            l, r, ss, fs = self.chunk[0].data_ptr(), self.chunk[1].data_ptr(), self.M, 1
        else:
            l, r, ss, fs = self.chunk.data_ptr(), self.chunk.data_ptr() + self.e, 2 * self.M, 2
        a = dict(state=self.state.data_ptr(), state_bytes=self.need, M=self.M, l=l, r=r, ss=ss, fs=fs,
                 counts=self.counts.data_ptr(), flags=self.flags.data_ptr(), mom=self.mom.data_ptr() + 8 * GUARD,
                 val=self.val.data_ptr() + 4 * GUARD, S=self.S, ctx=self.ctx.handle)
        a.update(kw)
        fn = lib.vnd_polar_voice_stream_f64_dev if self.dtype == np.float64 else lib.vnd_polar_voice_stream_f32_dev
        p = ctypes.c_void_p
        return fn(a['ctx'], p(a['state']), a['state_bytes'], a['M'], p(a['l']), p(a['r']), a['ss'], a['fs'], p(a['counts']),
                  p(a['flags']), p(a['mom']), p(a['val']), a['S'], p(self.stream()))

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
        self.mom.fill_(POISON)
        self.val.fill_(-77)

    def untouched(self):
        """Nothing was written: moments, valid, the state's tail."""
        return bool((self.mom == POISON).all()) and bool((self.val == -77).all()) and \
            bool(self.torch.isnan(self.raw_state[self.need // 4:]).all())

    def call(self, blocks, counts, flags):
        """One call; checks valid, the positions and the written / untouched split; returns (moments (S, 8), valid)."""
        from vndecorrelate_amd.analysis import polar_voice_spans
        self.upload(blocks, counts, flags)
        assert self.raw() == 0, self.ctx._lib.vnd_last_error()
        self.torch.cuda.synchronize(self.dev)
        want, new = polar_voice_spans(self.mirror, counts, flags, self.M)
        val = self.val.cpu().numpy()
        assert (val[:GUARD] == -77).all() and (val[GUARD + self.S:] == -77).all()
        assert val[GUARD:GUARD + self.S].tolist() == want.tolist(), (counts, flags, self.mirror)
        assert self.positions().tolist() == new.tolist()
        self.mirror = new
        mom = self.mom.cpu().numpy()
        assert (mom[:GUARD] == POISON).all() and (mom[GUARD + 8 * self.S:] == POISON).all()
        body = mom[GUARD:GUARD + 8 * self.S].reshape(self.S, 8)
        for b, v in enumerate(want):
            assert (body[b] == POISON).all() if v != 1 else not (body[b] == POISON).any(), (b, v)
        assert bool(self.torch.isnan(self.raw_state[self.need // 4:]).all())           # the footprint of the state
        return body.view(np.float64).copy(), want


class Voice:
    def __init__(self, x, start_call=0, whole=False, end_with_last=True, discard_after=None):
        self.x, self.start_call, self.whole, self.end_with_last = x, start_call, whole, end_with_last
        self.discard_after = discard_after
        self.pushed, self.done, self.ended, self.last = 0, False, False, None


def noise(n, seed, amplitude=1.0, dtype=np.float32):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, n)
    y = 0.6 * x + 0.4 * rng.standard_normal(n)
    if dtype == np.float64:                                   # values between float32 ones
        x, y = x * (1 + 1e-9), y * (1 - 1e-9)
    return (np.stack([x, y], axis=1) * amplitude).astype(dtype)


def drive(h, plan, rng, menu, after_call):
    """The voices of `plan` ({slot: [Voice, ...]}) through the harness on counts drawn from `menu` and from [0, M]; a voice
    with discard_after is never ended: the next voice of its slot STARTs over it.  after_call(call, moments, active) sees
    every call's rows and the voice of every slot that answered."""
    queue = {slot: list(voices) for slot, voices in plan.items()}
    active = {slot: None for slot in range(h.S)}
    call = 0
    while any(queue.values()) or any(v is not None for v in active.values()):
        assert call < 400
        blocks, counts, flags, ended = [None] * h.S, np.zeros(h.S, np.int32), np.zeros(h.S, np.int32), []
        for slot in range(h.S):
            v, force = active[slot], False
            if v is not None and v.discard_after is not None and v.pushed >= v.discard_after:
                v, active[slot], force = None, None, True
            if v is None and queue.get(slot) and (force or queue[slot][0].start_call <= call):
                v = active[slot] = queue[slot].pop(0)
                flags[slot] |= START
            if v is None:
                continue
            limit = (len(v.x) if v.discard_after is None else v.discard_after) - v.pushed
            pick = int(rng.choice(menu)) if rng.random() < 0.6 else int(rng.integers(0, h.M + 1))
            n = limit if v.whole else min(limit, h.M, pick)
            blocks[slot], counts[slot] = v.x[v.pushed:v.pushed + n], n
            v.pushed += n
            if v.discard_after is None and v.pushed == len(v.x):
                if v.end_with_last or v.done:
                    flags[slot] |= END
                    ended.append(slot)
                v.done = True
        moments, valid = h.call(blocks, counts, flags)
        answered = {}
        for slot in range(h.S):
            if valid[slot] == 1:
                assert active[slot] is not None
                answered[slot] = active[slot]
                active[slot].last = moments[slot]
            else:
                assert valid[slot] == 0
        after_call(call, moments, answered)
        for slot in ended:
            active[slot].ended = True
            active[slot] = None
        call += 1
    return call


# ---- 1. a ragged schedule ---------------------------------------------------------------------------------------------
def ragged_plan(dtype, seed):
    sig = lambda n, k, amp=1.0: noise(n, seed + k, amp, dtype)
    long = sig(2049, 11)
    long[100] = 0.0                                           # a silent frame: r = 0, theta = 0
    long[3, 0] = -long[3, 1]                                  # L + R == 0: theta = +-pi/2
    long[1500, 1] = -long[1500, 0]
    return {0: [Voice(sig(0, 0), whole=True), Voice(sig(1300, 1), start_call=2, end_with_last=False)],
            1: [Voice(sig(1, 2)), Voice(sig(255, 3), start_call=3), Voice(sig(256, 12))],
            2: [Voice(sig(257, 4), whole=True), Voice(sig(511, 5), start_call=1), Voice(sig(512, 13))],
            3: [Voice(sig(2049, 6, 1e3)), Voice(sig(513, 7, 1e-3))],          # a loud voice, then a quiet one in its slot
            4: [Voice(sig(1025, 8), discard_after=450), Voice(sig(600, 9), whole=True)],      # dropped by a START
            5: [Voice(sig(1025, 10), start_call=1, end_with_last=False), Voice(long)]}


MENU = [0, 0, 1, 600, 511, 512, 513, 89]


@pytest.mark.parametrize('planar', [False, True], ids=['channels', 'planar'])
def test_ragged_schedule_float32_bit_for_bit(torch, ctx, an, planar):
    h = Harness(torch, ctx, 6, 600, planar=planar)
    plan = ragged_plan(np.float32, 100)
    seen = []

    def after_call(call, moments, answered):
        for slot, v in answered.items():
            assert same_bits(moments[slot], one_shot(ctx, v.x[:v.pushed])), (call, slot, v.pushed)
            seen.append(v.pushed)
    calls = drive(h, plan, np.random.default_rng(7 + planar), MENU, after_call)
    assert calls > 10 and len(seen) >= 30
    for slot, voices in plan.items():
        for v in voices:
            assert v.last is not None and (v.ended or v.discard_after is not None)
            if v.ended:                                               # the float32 bars against NumPy, at END
                assert same_bits(v.last, one_shot(ctx, v.x))
                check_f32_against_numpy(v.last, v.x, (slot, len(v.x)))
    assert not h.positions().any()
    assert plan[5][1].last[4] == np.float64(np.float32(np.pi / 2))    # the frame with L + R = 0


# ---- 2. the lane wrap, many chunks per call, M below a chunk ------------------------------------------------------------
def test_a_voice_that_wraps_the_reduce_lanes(torch, ctx, an):
    S, M, n = 2, 4800, 131585
    h = Harness(torch, ctx, S, M)
    x, other = noise(n, 31), noise(3 * M + 11, 32)
    look = {5, 13, 27 - 1}                                            # 27 full blocks = 129600; the wrap is at 131072
    p, call = 0, 0
    while p < n:
        k = min(M, n - p)
        q = min(call * 700, len(other))
        k2 = min(700, len(other) - q)
        flags = [(START if p == 0 else 0) | (END if p + k == n else 0), (START if call == 0 else 0)]
        moments, valid = h.call([x[p:p + k], other[q:q + k2]], [k, k2], flags)
        p += k
        if call in look or p == n or 131072 <= p < 131072 + M:
            assert same_bits(moments[0], one_shot(ctx, x[:p])), (call, p)
        if k2:
            assert same_bits(moments[1], one_shot(ctx, other[:q + k2])), call
        call += 1
    assert call == 28 and h.positions().tolist() == [0, len(other)]


def test_many_chunks_in_one_call(torch, ctx, an):
    S, M = 2, 132096                                                  # 258 chunks a call: lanes 0 and 1 take two of them
    h = Harness(torch, ctx, S, M)
    assert h.G == 259
    x = [noise(2 * M + 7, 41), noise(2 * M + 7, 42)]
    sizes = [(M, M, 7), (7, M, M)]
    p = [0, 0]
    for i in range(3):
        blocks = [x[b][p[b]:p[b] + sizes[b][i]] for b in range(S)]
        moments, valid = h.call(blocks, [sizes[b][i] for b in range(S)], [(START if i == 0 else 0) | (END if i == 2 else 0)] * S)
        for b in range(S):
            p[b] += sizes[b][i]
            assert same_bits(moments[b], one_shot(ctx, x[b][:p[b]])), (i, b)


def test_a_block_size_below_a_chunk(torch, ctx, an):
    S, M = 3, 100
    h = Harness(torch, ctx, S, M)
    assert h.G == 2
    plan = {0: [Voice(noise(513, 51))], 1: [Voice(noise(1025, 52), start_call=1)], 2: [Voice(noise(513, 53), whole=False)]}

    def after_call(call, moments, answered):
        for slot, v in answered.items():
            assert same_bits(moments[slot], one_shot(ctx, v.x[:v.pushed])), (call, slot, v.pushed)
    drive(h, plan, np.random.default_rng(5), [0, 1, 100, 100, 99, 12], after_call)
    assert all(v.ended for voices in plan.values() for v in voices)


# ---- 3. float64 --------------------------------------------------------------------------------------------------------
def test_ragged_schedule_float64(torch, ctx, an):
    S, M = 6, 600
    h = Harness(torch, ctx, S, M, dtype=np.float64)
    ref = Harness(torch, ctx, S, M, dtype=np.float64, planar=True)
    plan = ragged_plan(np.float64, 200)

    def whole_blocks(answered):
        """The same voices' frames so far, fed to the second pool in whole blocks of M."""
        p, out, first = {s: 0 for s in answered}, {}, True
        while p:
            blocks, counts, flags = [None] * S, np.zeros(S, np.int32), np.zeros(S, np.int32)
            for s in list(p):
                v = answered[s]
                k = min(M, v.pushed - p[s])
                blocks[s], counts[s] = v.x[p[s]:p[s] + k], k
                p[s] += k
                flags[s] = (START if first else 0) | (END if p[s] == v.pushed else 0)
            moments, _ = ref.call(blocks, counts, flags)
            for s in list(p):
                if p[s] == answered[s].pushed:
                    out[s] = moments[s]
                    del p[s]
            first = False
        return out

    def after_call(call, moments, answered):
        want = whole_blocks(answered)
        for slot, v in answered.items():
            assert same_bits(moments[slot], want[slot]), (call, slot, v.pushed)
    drive(h, plan, np.random.default_rng(17), MENU, after_call)
    for slot, voices in plan.items():
        for v in voices:
            if v.ended:
                check_f64_against_numpy(v.last, v.x, (slot, len(v.x)))
    assert sum(v.ended for voices in plan.values() for v in voices) == 13


# ---- 4. wide pools -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', [7, 257, 513])
def test_every_slot_live(torch, ctx, an, S):
    M = 600
    h = Harness(torch, ctx, S, M)
    rng = np.random.default_rng(S)
    sizes = rng.integers(1, M + 1, (3, S))
    sizes[1, ::5] = 0                                                 # idle in the middle call
    sizes[0, 1::7], sizes[2, 2::9] = M, M
    x = [noise(int(sizes[:, b].sum()), 1000 + b) for b in range(S)]
    p = np.zeros(S, np.int64)
    for i in range(3):
        blocks = [x[b][p[b]:p[b] + sizes[i, b]] for b in range(S)]
        moments, valid = h.call(blocks, sizes[i], np.full(S, (START if i == 0 else 0) | (END if i == 2 else 0), np.int32))
        p += sizes[i]
        for b in (range(S) if i == 2 else range(0, S, 37)):
            if valid[b] == 1:
                assert same_bits(moments[b], one_shot(ctx, x[b][:p[b]])), (i, b)
        assert (valid == 1).sum() == (S if i != 1 else S - len(range(0, S, 5)))


# ---- 5. positions of a long-lived voice -------------------------------------------------------------------------------
def test_planted_positions_continue_as_the_voice_would(torch, ctx, an):
    """A slot's answer depends on its position through floor(p / 512) mod 256 and p mod 512 alone once every lane has a
    chunk (tests/test_polar_voice_pool_cpu.py holds the mirror to that in Python integers).  So an honest voice is run to
    p' = P mod 131072 + 131072 on one pool; its lane sums and pending frames are planted at P on a second pool, and both
    go on with the same blocks: the same bits after every call, the positions the mirror's, and the honest voice the
    one-shot call's at its END."""
    targets = [2 ** 31 - 7, 2 ** 32 - 300, 2 ** 40 + 3]
    S, M = 3, 6000
    honest, planted = Harness(torch, ctx, S, M), Harness(torch, ctx, S, M)
    small = [t % 131072 + 131072 for t in targets]
    tail = [1, 600, 0, 511, 6000, 513, 77]
    x = [noise(small[b] + sum(tail), 60 + b) for b in range(S)]
    p, first = [0] * S, True
    while any(p[b] < small[b] for b in range(S)):
        k = [min(M, small[b] - p[b]) for b in range(S)]
        honest.call([x[b][p[b]:p[b] + k[b]] for b in range(S)], k, [START if first else 0] * S)
        p, first = [p[b] + k[b] for b in range(S)], False
    assert honest.positions().tolist() == small
    sums = honest.sums_view().cpu().numpy()
    for b in range(S):
        pend = honest.pending(b)
        assert pend.tobytes() == x[b][small[b] - small[b] % 512:small[b]].tobytes()      # the ring holds the open chunk
        planted.plant(b, targets[b], sums[b], pend)
    for i, k in enumerate(tail):
        blocks = [x[b][p[b]:p[b] + k] for b in range(S)]
        flags = [END if i == len(tail) - 1 else 0] * S
        a, _ = honest.call(blocks, [k] * S, flags)
        c, valid = planted.call(blocks, [k] * S, flags)              # (the harness holds the positions to the mirror)
        p = [p[b] + k for b in range(S)]
        for b in range(S):
            if valid[b] == 1:
                assert same_bits(a[b], c[b]), (i, b)
    for b in range(S):
        assert same_bits(a[b], one_shot(ctx, x[b])), b
    assert not planted.positions().any()


def exact_frames(n, seed):
    """Frames whose theta is exact on any atan2 - L = R > 0 (theta = 0) and L = -R (theta = +-pi/2) - so that every term is
    a few IEEE float32 operations (multiply, add, a correctly rounded square root) and NumPy has the device's bits."""
    rng = np.random.default_rng(seed)
    a = (rng.integers(1, 4096, n) * 2.0 ** rng.integers(-12, 4, n)).astype(np.float32)
    sign = np.where(rng.random(n) < 0.5, 1, -1).astype(np.float32)
    side = rng.random(n) < 0.5
    return np.stack([np.where(side, a, sign * a), np.where(side, a, -sign * a)], axis=1).astype(np.float32)


def float32_terms(y):
    """The eight per-frame terms as the float32 kernel forms them (csrc/vnd_polar.hpp), in NumPy float32, as float64."""
    left, right = y[:, 0], y[:, 1]
    th = np.arctan2(left - right, left + right)
    assert th.dtype == np.float32 and np.isin(np.abs(th), [0.0, np.float32(np.pi / 2)]).all()
    r = np.sqrt(left * left + right * right)
    t2 = th * th
    terms = np.stack([r, r * th, r * t2, r * (t2 * th), np.abs(th), left * right, left * left, right * right], axis=1)
    assert terms.dtype == np.float32
    return terms.astype(np.float64)


def test_planted_lane_sums_from_the_mirror(torch, ctx, an):
    """Positions 2^31 - 7, 2^32 - 300 and 2^40 + 3 planted with lane sums and pending frames that the mirror
    (analysis.polar_moments_ordered's streamed form) holds as well, then continued: the device's moments are the mirror's
    bit for bit after every call.  Slot 3 is an honest voice from a START beside them."""
    targets = [2 ** 31 - 7, 2 ** 32 - 300, 2 ** 40 + 3]
    S, M = 4, 600
    h = Harness(torch, ctx, S, M)
    rng = np.random.default_rng(77)
    states = []
    for b, p in enumerate(targets):
        lanes = rng.standard_normal((256, 8)) * 1e3
        lanes[:, 4] = rng.uniform(0, np.pi / 2, 256)
        pend = exact_frames(p % 512, 80 + b)
        h.plant(b, p, lanes, pend)
        states.append(an.PolarMomentsState(p, lanes, float32_terms(pend)))
    states.append(an.PolarMomentsState())
    sizes = [(1, 600, 0, 511, 600, 513, 77), (600, 600, 600, 0, 1, 300, 512), (0, 7, 600, 600, 89, 0, 600),
             (511, 600, 1, 0, 600, 600, 3)]
    for i in range(7):
        blocks = [exact_frames(sizes[b][i], 1000 + 10 * i + b) for b in range(S)]
        flags = [(START if (i == 0 and b == 3) else 0) | (END if i == 6 else 0) for b in range(S)]
        moments, valid = h.call(blocks, [sizes[b][i] for b in range(S)], flags)       # (positions: the harness's check)
        for b in range(S):
            want = an.polar_moments_ordered(float32_terms(blocks[b]), states[b])
            if valid[b] == 1:
                assert same_bits(moments[b], want), (i, b)
                if b == 3:
                    sofar = np.concatenate([exact_frames(sizes[3][k], 1000 + 10 * k + 3) for k in range(i + 1)])
                    assert same_bits(moments[b], one_shot(ctx, sofar)), i
    assert [st.position for st in states[:3]] == [t + sum(sizes[b]) for b, t in enumerate(targets)]
    assert not h.positions().any()


def test_a_position_past_2_to_60_answers_minus_one_until_a_start(torch, ctx, an):
    S, M = 3, 100
    h = Harness(torch, ctx, S, M)
    x = noise(300, 8)
    h.call([x[:100], None, x[:100]], [100, 0, 100], [START, 0, START])
    h.plant(1, 2 ** 60 + 1)
    before = h.slot_state(1)
    b, valid = h.call([x[100:200], x[:100], x[100:200]], [100, 100, 100], [0, 0, 0])
    assert valid.tolist() == [1, -1, 1] and h.positions()[1] == 2 ** 60 + 1 and h.slot_state(1) == before
    h.call([x[200:], x[:100], x[200:]], [100, 100, 100], [END, START, END])          # the slot works again with START
    h.call([None, x[100:200], None], [0, 100, 0], [0, 0, 0])
    e, _ = h.call([None, x[200:], None], [0, 100, 0], [0, END, 0])
    assert same_bits(e[1], one_shot(ctx, x))
    h.plant(0, 2 ** 60)                                               # the last position a call goes on from
    f, valid = h.call([x[:7], None, None], [7, 0, 0], [0, 0, 0])
    assert valid[0] == 1 and h.positions()[0] == 2 ** 60 + 7


# ---- 6. bad counts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad_count', [101, -1, 2 ** 31 - 1, -2 ** 31])
def test_a_bad_count_leaves_the_slot_and_its_neighbours_alone(torch, ctx, an, bad_count):
    S, M = 4, 100
    x = [noise(300, 20 + b) for b in range(S)]
    h = Harness(torch, ctx, S, M)
    for i in range(3):
        blocks = [x[b][100 * i:100 * i + 100] for b in range(S)]
        counts = np.full(S, 100, np.int64)
        flags = np.full(S, (START if i == 0 else 0) | (END if i == 2 else 0), np.int32)
        if i == 1:                                               # slot 2, live since call 0, sends a bad count
            bad = counts.copy()
            bad[2] = bad_count
            before = h.slot_state(2)
            moments, valid = h.call(blocks, bad, flags)          # (the harness holds its moments row to the poison)
            assert valid.tolist() == [1, 1, -1, 1] and h.slot_state(2) == before and h.positions()[2] == 100
            for b in (0, 1, 3):
                assert same_bits(moments[b], one_shot(ctx, x[b][:200])), b
            only = np.zeros(S, np.int64)                         # the voice goes on: the block it meant to push
            only[2] = 100
            moments, valid = h.call(blocks, only, np.zeros(S, np.int32))
            assert valid.tolist() == [0, 0, 1, 0] and same_bits(moments[2], one_shot(ctx, x[2][:200]))
        else:
            moments, valid = h.call(blocks, counts, flags)
            for b in range(S):
                assert same_bits(moments[b], one_shot(ctx, x[b][:100 * i + 100])), (i, b)
    # a bad count with START or END changes nothing either
    h.call([x[0][:50]] * S, [50] * S, [START] * S)
    before = [h.slot_state(b) for b in range(S)]
    _, valid = h.call([None] * S, [bad_count] * S, [START, END, START | END, 0])
    assert valid.tolist() == [-1] * S and [h.slot_state(b) for b in range(S)] == before


# ---- 7. the Python pool: capture, metering a decorrelating pool, the dict form ----------------------------------------
def device_schedule(S, M, seed, dtype=np.float32):
    rng = np.random.default_rng(seed)
    calls = []
    for i in range(8):
        counts = rng.integers(0, M + 1, S).astype(np.int32)
        counts[rng.random(S) < 0.3] = 0
        flags = np.zeros(S, np.int32)
        if i == 0:
            flags[:4] = START
        if i == 2:
            flags[4], flags[1] = START, END
        if i == 3:
            flags[5] = START | END
        if i == 4:
            flags[1], flags[0], counts[0] = START, END, 0
        if i == 7:
            flags[:] |= END
        calls.append((rng.uniform(-1, 1, (S, M, 2)).astype(dtype), counts, flags))
    return calls


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_graph_replay_equals_the_uncaptured_run(torch, ctx, an, dtype):
    S, M = 6, 600
    dev = torch.device('cuda', ctx.device)
    calls = device_schedule(S, M, 3, np.dtype(dtype))
    results = []
    for replayed in (False, True):
        pool = an.stereo_image_voice_pool(S, max_frames_per_call=M, dtype=dtype)
        y = torch.empty((S, M, 2), dtype=getattr(torch, dtype), device=dev)
        counts, flags, valid = (torch.empty(S, dtype=torch.int32, device=dev) for _ in range(3))
        moments = torch.empty((S, 8), dtype=torch.int64, device=dev)
        out = (moments.view(torch.float64), valid)
        pool.reset()
        graph = None
        if replayed:
            graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
            with torch.cuda.graph(graph, stream=side):
                pool.process_dev(y, counts, flags, out=out)
            torch.cuda.synchronize(dev)
        got = []
        for yh, c, f in calls:
            y.copy_(torch.from_numpy(yh))
            counts.copy_(torch.from_numpy(c))
            flags.copy_(torch.from_numpy(f))
            moments.fill_(POISON)
            if graph is not None:
                graph.replay()
            else:
                pool.process_dev(y, counts, flags, out=out)
            torch.cuda.synchronize(dev)
            got.append((moments.cpu().numpy(), valid.cpu().numpy()))
        with pytest.raises(RuntimeError, match='runs through process_dev'):
            pool.process({})
        results.append(got)
    pos = np.zeros(S, np.int64)
    sofar = [np.zeros((0, 2), np.dtype(dtype)) for _ in range(S)]
    for i, ((m0, v0), (m1, v1)) in enumerate(zip(*results)):
        want, pos = an.polar_voice_spans(pos, calls[i][1], calls[i][2], M)
        assert v0.tolist() == want.tolist() == v1.tolist(), i
        assert m0.tobytes() == m1.tobytes(), i
        for b, v in enumerate(want):
            if calls[i][2][b] & START or (i and calls[i - 1][2][b] & END):        # after an END a voice begins at 0 by itself
                sofar[b] = sofar[b][:0]
            sofar[b] = np.concatenate([sofar[b], calls[i][0][b, :calls[i][1][b]]])
            assert (m0[b] == POISON).all() if v != 1 else not (m0[b] == POISON).any(), (i, b)
            if v == 1 and dtype == 'float32':
                assert same_bits(m0[b].view(np.float64), one_shot(ctx, sofar[b])), (i, b)
            elif v == 1:
                check_f64_against_numpy(m0[b].view(np.float64), sofar[b], (i, b))
    assert len(results[1]) == 8 and not pos.any()


def _meter_run(torch, ctx, pool, meter, extra, voices, stage_counts):
    """`pool` and `meter` captured together in one graph; voices: per slot (signal, bank entry).  Every slot starts on call
    0 and pushes blocks of its own sizes, END with its last block.  After call 0 a replay carries a bad count for slot 2
    and nothing for the others: every stage's out_counts and the meter's valid must answer -1 for it, and the voice goes
    on.  Returns the moments per slot at its END."""
    S, M = pool.slots, pool.max_frames_per_call
    dev = torch.device('cuda', ctx.device)
    x = torch.empty((S, M, 2), dtype=torch.float32, device=dev)
    counts, flags, valid = (torch.empty(S, dtype=torch.int32, device=dev) for _ in range(3))
    moments = torch.empty((S, 8), dtype=torch.int64, device=dev)
    pool.reset()
    meter.reset()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
    with torch.cuda.graph(graph, stream=side):
        y, mid = pool.process_dev(x, counts, flags, *extra)
        meter.process_dev(y, mid, flags, out=(moments.view(torch.float64), valid))
    torch.cuda.synchronize(dev)

    def replay(xh, c, f):
        for t, v in ((x, xh), (counts, c), (flags, f)):
            t.copy_(torch.from_numpy(v))
        moments.fill_(POISON)
        graph.replay()
        torch.cuda.synchronize(dev)
        return moments.cpu().numpy(), valid.cpu().numpy()
    rng = np.random.default_rng(S)
    pushed, started, final, call = [0] * S, [False] * S, [None] * S, 0
    while any(p is not None for p in pushed):
        assert call < 80
        xh, c, f = np.zeros((S, M, 2), np.float32), np.zeros(S, np.int32), np.zeros(S, np.int32)
        for b, (sig, _) in enumerate(voices):
            if pushed[b] is None:
                continue
            n = int(min(len(sig) - pushed[b], rng.choice([0, 1, M, int(rng.integers(0, M + 1))])))
            xh[b, :n], c[b] = sig[pushed[b]:pushed[b] + n], n
            f[b] = (0 if started[b] else START) | (END if pushed[b] + n == len(sig) else 0)
            started[b] = True
            pushed[b] = None if pushed[b] + n == len(sig) else pushed[b] + n
        mh, vh = replay(xh, c, f)
        given = mid.cpu().numpy()                                     # what the decorrelating pool handed the meter
        for b in range(S):
            work = given[b] > 0 or f[b] != 0
            assert vh[b] == (1 if work else 0) and (mh[b] == POISON).any() == (not work), (call, b)
            if f[b] & END:
                final[b] = mh[b].view(np.float64).copy()
        if call == 0:
            assert pushed[2] is not None
            bad = np.zeros(S, np.int32)
            bad[2] = M + 1
            mh, vh = replay(xh, bad, np.zeros(S, np.int32))
            assert [int(t.cpu()[2]) for t in stage_counts(mid)] + [int(vh[2])] == [-1] * (len(stage_counts(mid)) + 1)
            assert (mh == POISON).all() and [int(v) for v in vh[[0, 1, 3]]] == [0, 0, 0]
        call += 1
    return final


def test_metering_a_velvet_voice_pool_in_one_graph(torch, ctx, an):
    import vndecorrelate_amd.decorrelation as dec
    from test_gpu_chain_voice_pool import DURATION, FS, IMPULSES, KAPPAS, SEED
    S, M = 4, 600
    bank = [dec.VelvetNoise(sample_rate_hz=FS, duration_seconds=DURATION, num_impulses=IMPULSES, seed=SEED, normalizer=None,
                            log_distribution_strength=k) for k in KAPPAS]
    pool = dec.decorrelate_voice_pool(bank, slots=S, in_channels=2, max_frames_per_call=M)
    meter = an.stereo_image_voice_pool(S, max_frames_per_call=pool.row_frames)
    dev = torch.device('cuda', ctx.device)
    entries = np.array([3, 0, 2, 1])
    extra = (torch.from_numpy(pool.bank_tables[entries].astype(np.int32)).to(dev),)
    voices = [(noise(n, 70 + b), int(entries[b])) for b, n in enumerate((1700, 1900, 2300, 2201))]
    got = _meter_run(torch, ctx, pool, meter, extra, voices, lambda mid: (mid,))          # a VoicePool's -1 passes through
    for b, (sig, entry) in enumerate(voices):
        want = bank[entry].decorrelate(sig)
        assert want.dtype == np.float32 and len(want) >= len(sig)
        assert same_bits(got[b], one_shot(ctx, want)), b


def test_metering_a_chain_voice_pool_in_one_graph(torch, ctx, an):
    import vndecorrelate_amd.decorrelation as dec
    from test_gpu_chain_voice_pool import _bank
    S, M = 4, 600
    bank = _bank(dec, 'ms>lr-ch1')
    pool = dec.decorrelate_voice_pool(bank, slots=S, in_channels=2, max_frames_per_call=M)
    meter = an.stereo_image_voice_pool(S, max_frames_per_call=pool.row_frames, dtype='float64')
    dev = torch.device('cuda', ctx.device)
    entries = np.array([3, 0, 2, 1])
    extra = (torch.from_numpy(pool.bank_tables[entries].astype(np.int32)).to(dev),
             torch.from_numpy(pool.bank_delays[entries].astype(np.int32)).to(dev))
    voices = [(noise(n, 60 + b), int(entries[b])) for b, n in enumerate((1700, 1900, 2300, 2201))]
    got = _meter_run(torch, ctx, pool, meter, extra, voices, lambda mid: (pool._mid[1], mid))     # -1 from all three stages
    for b, (sig, entry) in enumerate(voices):
        want = np.asarray(bank[entry](sig))
        assert want.dtype == np.float64 and len(want) >= len(sig)
        check_f64_against_numpy(got[b], want, b)


def test_dict_form_scores_equal_the_objective(torch, ctx, an):
    import vndecorrelate_amd.decorrelation as dec
    from vndecorrelate_amd import optimization
    from test_gpu_chain_voice_pool import DURATION, FS, IMPULSES, KAPPAS, SEED
    S, M = 3, 480
    bank = [dec.VelvetNoise(sample_rate_hz=FS, duration_seconds=DURATION, num_impulses=IMPULSES, seed=SEED, normalizer=None,
                            log_distribution_strength=k) for k in KAPPAS]
    pool = dec.decorrelate_voice_pool(bank, slots=S, in_channels=2, max_frames_per_call=M)
    meter = an.stereo_image_voice_pool(S, max_frames_per_call=pool.row_frames)
    rng = np.random.default_rng(9)
    sigs = {0: noise(1500, 1), 1: noise(2000, 2), 2: noise(961, 3)}
    entry = {0: 2, 1: 0, 2: 3}
    pushed, final, first = {s: 0 for s in sigs}, {}, True
    while pushed:
        blocks, end = {}, []
        for s in list(pushed):
            n = int(min(len(sigs[s]) - pushed[s], rng.choice([0, 1, M, int(rng.integers(0, M + 1))])))
            blocks[s] = sigs[s][pushed[s]:pushed[s] + n]
            pushed[s] += n
            if pushed[s] == len(sigs[s]):
                end.append(s)
                del pushed[s]
        y = pool.process(blocks, start=entry if first else None, end=end)
        out = meter.process(y, start=list(sigs) if first else [], end=end)
        if first:
            assert meter.transfers == {'to_device': 1, 'to_host': 1}
        first = False
        for s, m in out.items():
            assert m.shape == (8,) and m.dtype == np.float64
        for s in end:
            final[s] = out[s]
    for s, sig in sigs.items():
        assert same_bits(final[s], one_shot(ctx, bank[entry[s]].decorrelate(sig))), s
        want = optimization.symmetry_aware_objective(sig, bank[entry[s]], **WEIGHTS)
        assert abs(meter.scores(final[s], **WEIGHTS) - want) <= SCORE_TOL, (s, want)
    scores = meter.scores(np.stack([final[s] for s in sigs]), **WEIGHTS)
    assert scores.shape == (3,) and len(set(scores.tolist())) == 3
    assert not meter.positions.any() and not meter.live.any()
    again = meter.process({2: sigs[0][:480]}, start=[2], end=[2])                     # a reused slot, a whole voice in one block
    assert same_bits(again[2], one_shot(ctx, sigs[0][:480]))
    with pytest.raises(RuntimeError, match='runs through process\\(\\)'):
        meter.process_dev(None, None, None)


# ---- 8. refusals -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_bad_arguments_write_nothing(torch, ctx, an, dtype):
    lib = ctx._lib
    S, M = 2, 100
    h = Harness(torch, ctx, S, M, dtype=dtype, planar=True, reset=False)
    h.upload([np.ones((M, 2), dtype)] * S, [M] * S, [START] * S)
    state, mom, val, l = h.state.data_ptr(), h.mom.data_ptr() + 8 * GUARD, h.val.data_ptr() + 4 * GUARD, h.chunk.data_ptr()
    invalid = [dict(state_bytes=h.need - 1), dict(M=0), dict(M=-5), dict(S=0), dict(S=-1), dict(ss=0), dict(fs=0), dict(fs=-2),
               dict(state=0), dict(state=state + 8), dict(l=0), dict(r=0), dict(mom=0), dict(val=0), dict(counts=0),
               dict(flags=0), dict(mom=l), dict(val=l), dict(mom=state), dict(val=state + h.need - 4), dict(l=state),
               dict(r=state), dict(val=mom + 8), dict(mom=val - 60), dict(ss=2 ** 62), dict(M=2 ** 31), dict(ctx=None)]
    for kw in invalid:
        assert h.raw(**kw) == INVALID, kw
        assert lib.vnd_last_error()
    unsupported = [dict(S=65536, state_bytes=2 ** 50), dict(M=512 * 65535, state_bytes=2 ** 50),    # 65536 workgroups a slot
                   dict(M=512 * 256, S=40000, state_bytes=2 ** 50)]                                 # 257 x 40000 > 2^23
    for kw in unsupported:
        assert h.raw(**kw) == UNSUPPORTED, (kw, lib.vnd_last_error())
    null = ctypes.c_void_p(None)
    e = h.e
    assert lib.vnd_polar_voice_stream_reset_dev(ctx.handle, null, h.need, S, M, e, null) == INVALID
    assert lib.vnd_polar_voice_stream_reset_dev(ctx.handle, ctypes.c_void_p(state), h.need - 1, S, M, e, null) == INVALID
    assert lib.vnd_polar_voice_stream_reset_dev(ctx.handle, ctypes.c_void_p(state + 4), h.need, S, M, e, null) == INVALID
    assert lib.vnd_polar_voice_stream_reset_dev(ctx.handle, ctypes.c_void_p(state), h.need, 0, M, e, null) == INVALID
    assert lib.vnd_polar_voice_stream_reset_dev(ctx.handle, ctypes.c_void_p(state), h.need, S, M, 2, null) == INVALID
    assert lib.vnd_polar_voice_stream_reset_dev(null, ctypes.c_void_p(state), h.need, S, M, e, null) == INVALID
    assert lib.vnd_polar_voice_stream_reset_dev(ctx.handle, ctypes.c_void_p(state), 2 ** 50, 65536, M, e, null) == UNSUPPORTED
    torch.cuda.synchronize(h.dev)
    assert h.untouched() and bool(torch.isnan(h.state).all())
    h.reset()
    moments, valid = h.call([np.ones((M, 2), dtype)] * S, [M] * S, [START] * S)       # the good call writes
    assert valid.tolist() == [1, 1] and abs(moments[0, 0] - M * float(np.sqrt(dtype(2)))) <= 1e-10 and moments[0, 4] == 0.0
