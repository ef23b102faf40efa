"""GPU tier of the correlogram voice pool (vnd_correlogram_voice_stream_f32_dev / _f64_dev,
include/vnd_correlogram_voice_stream.h; analysis.CorrelogramVoicePool).  Every comparison is of the float32 bits, against
the one-shot device call vnd_correlogram_f32_dev on each voice's whole signal.

The harness drives the C ABI on poisoned memory: the ring is NaN, the positions are NaN bytes until the reset, the chunk
rows past counts[b] are NaN, `out` holds a signalling NaN no arithmetic yields, with a sentinel tail.  After every call
out_counts and the device's positions equal the mirror (analysis.correlogram_voice_spans), every row below out_counts[b]
is written and every value at or past it is untouched."""
import ctypes
import importlib.util
import json
import pathlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = pathlib.Path(__file__).resolve().parents[1]
GOLDEN = REPO / 'tests' / 'golden'
EPS = 1e-10
START, END = 1, 2
POISON = 0x7FA5A5A5                          # a signalling NaN: no kernel arithmetic yields it
TAIL = 64
INVALID, UNSUPPORTED = 1, 4


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


def bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))


_one_shot_cache = {}


def one_shot(an, x, W, H, L):
    """vnd_correlogram_f32_dev on one voice's whole (n, 2) signal, cast to float32 as astype does: float32 (windows, L)."""
    x32 = np.ascontiguousarray(x).astype(np.float32)
    if len(x32) < W:
        return np.zeros((0, L), np.float32)
    key = (x32.tobytes(), W, H, L)
    if key not in _one_shot_cache:
        _one_shot_cache[key] = np.array(an.correlogram_numpy_batch(x32[None], None, W, H, L, EPS)[0])
    return _one_shot_cache[key]


def plan_of(ctx, S, W, H, L, M):
    from vndecorrelate_amd import _native
    text = _native.describe_correlogram_voice_stream(S, W, H, L, M)
    assert text.startswith('correlogram_voice_stream ')
    return {k: int(v) for k, v in (f.split('=') for f in text.split()[1:])}


class Harness:
    """One pool at the C ABI on poisoned memory.  planar: x and y as two (S, M) arrays; else channels of one (S, M, 2)."""

    def __init__(self, torch, ctx, S, M, W, H, L, dtype=np.float32, planar=False, reset=True):
        from vndecorrelate_amd import _native
        self.torch, self.ctx, self.native = torch, ctx, _native
        self.dev = torch.device('cuda', ctx.device)
        self.S, self.M, self.W, self.H, self.L = S, M, W, H, L
        self.dtype, self.planar = np.dtype(dtype), planar
        self.rc = -(-M // H)
        self.cap = W - 1 + M
        self.need = _native.correlogram_voice_stream_state_bytes(S, W, M)
        self.pos_bytes = (8 * S + 15) // 16 * 16
        assert self.need == self.pos_bytes + S * self.cap * 8
        self.state = torch.full((self.need // 4,), float('nan'), dtype=torch.float32, device=self.dev)
        tdt = torch.float32 if self.dtype == np.float32 else torch.float64
        self.chunk = torch.empty((2, S, M) if planar else (S, M, 2), dtype=tdt, device=self.dev)
        self.counts, self.flags, self.oc = (torch.empty(S, dtype=torch.int32, device=self.dev) for _ in range(3))
        self.out = torch.empty((S * self.rc * L + TAIL,), dtype=torch.int32, device=self.dev)
        self.mirror = None                                   # the positions, once they are known
        if reset:
            self.reset()

    def stream(self):
        return self.torch.cuda.current_stream(self.dev).cuda_stream

    def reset(self):
        self.native.correlogram_voice_stream_reset_device(self.ctx, self.state.data_ptr(), self.need, self.S, self.W, self.M,
                                                          stream=self.stream())
        self.mirror = np.zeros(self.S, np.int64)

    def positions(self):
        return self.state[:2 * self.S].view(self.torch.int64).cpu().numpy().copy()

    def ring(self):
        return self.state[self.pos_bytes // 4:].view(self.torch.int32).cpu().numpy().copy().reshape(self.S, self.cap, 2)

    def plant(self, b, position, history):
        """Slot b at `position`, the frames [position - len(history), position) in their ring slots."""
        torch = self.torch
        self.state[:2 * self.S].view(torch.int64)[b] = position
        where = np.array([(position - len(history) + j) % self.cap for j in range(len(history))], np.int64)   # Python ints
        if len(history):
            ring = self.state[self.pos_bytes // 4:].view(self.S, self.cap, 2)
            ring[b, torch.from_numpy(where).to(self.dev)] = torch.from_numpy(np.asarray(history, np.float32)).to(self.dev)
        self.mirror[b] = position

    def raw(self, **kw):
        """The C call with pointers and scalars replaced by name; returns the status."""
        lib = self.ctx._lib
        e = self.chunk.element_size()
        if self.planar:
            x, y, ss, fs = self.chunk[0].data_ptr(), self.chunk[1].data_ptr(), self.M, 1
        else:
            x, y, ss, fs = self.chunk.data_ptr(), self.chunk.data_ptr() + e, 2 * self.M, 2
        a = dict(state=self.state.data_ptr(), state_bytes=self.need, M=self.M, x=x, y=y, ss=ss, fs=fs,
                 counts=self.counts.data_ptr(), flags=self.flags.data_ptr(), out=self.out.data_ptr(), oc=self.oc.data_ptr(),
                 S=self.S, W=self.W, H=self.H, L=self.L, ctx=self.ctx.handle)
        a.update(kw)
        fn = lib.vnd_correlogram_voice_stream_f64_dev if self.dtype == np.float64 else lib.vnd_correlogram_voice_stream_f32_dev
        p = ctypes.c_void_p
        return fn(a['ctx'], p(a['state']), a['state_bytes'], a['M'], p(a['x']), p(a['y']), a['ss'], a['fs'], p(a['counts']),
                  p(a['flags']), p(a['out']), p(a['oc']), a['S'], a['W'], a['H'], a['L'], EPS, p(self.stream()))

    def upload(self, blocks, counts, flags):
        torch = self.torch
        host = np.full((self.S, self.M, 2), np.nan, self.dtype)
        for b, block in enumerate(blocks):
            if block is not None and len(block):
                host[b, :len(block)] = block
        if self.planar:
            host = np.ascontiguousarray(host.transpose(2, 0, 1))
        self.chunk.copy_(torch.from_numpy(host))
        self.counts.copy_(torch.from_numpy(np.asarray(counts, np.int32)))
        self.flags.copy_(torch.from_numpy(np.asarray(flags, np.int32)))
        self.out.fill_(POISON)
        self.oc.fill_(-77)

    def call(self, blocks, counts, flags):
        """One call; checks the counts, the positions and the written / untouched split; returns the rows per slot."""
        from vndecorrelate_amd.analysis import correlogram_voice_spans
        self.upload(blocks, counts, flags)
        assert self.raw() == 0, self.ctx._lib.vnd_last_error()
        self.torch.cuda.synchronize(self.dev)
        want, new = correlogram_voice_spans(self.mirror, counts, flags, self.W, self.H, self.M)
        oc = self.oc.cpu().numpy()
        assert oc.tolist() == want.tolist(), (counts, flags, self.mirror)
        assert (want <= self.rc).all()
        assert self.positions().tolist() == new.tolist()
        self.mirror = new
        out = self.out.cpu().numpy()
        assert (out[self.S * self.rc * self.L:] == POISON).all()
        body = out[:self.S * self.rc * self.L].reshape(self.S, self.rc, self.L)
        rows = []
        for b, n in enumerate(want):
            n = max(int(n), 0)
            assert not (body[b, :n] == POISON).any() and (body[b, n:] == POISON).all(), (b, n)
            rows.append(body[b, :n].view(np.float32).copy())
        return rows


class Voice:
    def __init__(self, x, start_call=0, whole=False, end_with_last=True, discard_after=None):
        self.x, self.start_call, self.whole, self.end_with_last = x, start_call, whole, end_with_last
        self.discard_after = discard_after
        self.pushed, self.done, self.out = 0, False, []


def noise(n, seed, amplitude=1.0, dtype=np.float32):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, n)
    y = 0.6 * x + 0.4 * rng.standard_normal(n)
    if dtype == np.float64:                                   # values between float32 ones
        x, y = x * (1 + 1e-9), y * (1 - 1e-9)
    return (np.stack([x, y], axis=1) * amplitude).astype(dtype)


def drive(h, plan, rng, menu):
    """The voices of `plan` ({slot: [Voice, ...]}) through the harness on counts drawn from `menu` and from [0, M]; a voice
    with discard_after is never ended: the next voice of its slot STARTs over it."""
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
        rows = h.call(blocks, counts, flags)
        for slot in range(h.S):
            if active[slot] is not None:
                active[slot].out.append(rows[slot])
            else:
                assert len(rows[slot]) == 0
        for slot in ended:
            active[slot] = None
        call += 1
    return call


def check_voices(an, plan, W, H, L):
    for slot, voices in plan.items():
        for i, v in enumerate(voices):
            want = one_shot(an, v.x, W, H, L)
            got = np.concatenate([r.reshape(-1, L) for r in v.out]) if v.out else np.zeros((0, L), np.float32)
            if v.discard_after is None:
                assert bits_equal(got, want), (slot, i, got.shape, want.shape)
            else:                                            # what it returned before it was dropped is final all the same
                assert len(got) == (max(0, (v.discard_after - W) // H + 1) if v.discard_after >= W else 0)
                assert bits_equal(got, want[:len(got)]), (slot, i)


# ---- 1. a ragged schedule ---------------------------------------------------------------------------------------------
RAGGED = [(64, 24, 127), (64, 1, 200), (100, 250, 51), (1, 1, 1), (64, 24, 1100), (882, 441, 1765)]


def ragged_plan(dtype, seed):
    sig = lambda n, k, amp=1.0: noise(n, seed + k, amp, dtype)
    return {0: [Voice(sig(1, 0), whole=True), Voice(sig(1300, 1), start_call=2, end_with_last=False)],
            1: [Voice(sig(63, 2)), Voice(sig(65, 3), start_call=3)],
            2: [Voice(sig(64, 4), whole=True), Voice(sig(200, 5), start_call=1)],
            3: [Voice(sig(2049, 6, 1e3)), Voice(sig(700, 7, 1e-3))],          # a loud voice, then a quiet one in its slot
            4: [Voice(sig(900, 8), discard_after=450), Voice(sig(600, 9), whole=True)],       # dropped by a START
            5: [Voice(sig(30, 10), start_call=1, end_with_last=False), Voice(sig(2049, 11))]}


@pytest.mark.parametrize('planar', [False, True], ids=['channels', 'planar'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('W,H,L', RAGGED)
def test_ragged_schedule(torch, ctx, an, W, H, L, dtype, planar):
    S, M = 6, 600
    plan = plan_of(ctx, S, W, H, L, M)
    rc = -(-M // H)
    assert plan == dict(rows_per_call=rc, groups=-(-rc // 4), tiles=-(-L // 1024), nblocks=S * -(-rc // 4) * -(-L // 1024),
                        threads=256, advance_groups=1)
    h = Harness(torch, ctx, S, M, W, H, L, dtype, planar, reset=False)
    assert (np.abs(h.positions()) > 2 ** 60).all()          # NaN bytes until the reset
    h.reset()
    voices = ragged_plan(dtype, 1000 * W + H)
    menu = [0, 1, min(H, M), min(max(W - 1, 0), M), M]
    calls = drive(h, voices, np.random.default_rng(W + H + L), menu)
    assert calls > 6
    check_voices(an, voices, W, H, L)
    assert not h.positions().any()                           # every voice ended
    if W >= 64:                                              # the voice shorter than W returned nothing, END included
        assert sum(len(r) for r in voices[5][0].out) == 0 and len(voices[5][0].out) >= 2


# ---- 2. the reference's goldens ---------------------------------------------------------------------------------------
def test_reference_fixtures_beside_a_neighbour(torch, ctx, an):
    from vndecorrelate_amd.utils.dsp import correlogram_sizes, to_float32
    spec = importlib.util.spec_from_file_location('gen_correlogram_golden', REPO / 'tools' / 'gen_correlogram_golden.py')
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    g = np.load(GOLDEN / 'correlogram.npz')
    manifest = json.loads((GOLDEN / 'correlogram_manifest.json').read_text())
    M, seen = 256, 0
    for i, (name, case) in enumerate(manifest['cases'].items()):
        x, y = gen.fixture_inputs(case['input'], g)
        ref = g[name + '__out']
        kw = dict(sample_rate_hz=44100, max_lag_seconds=0.02, window_size_seconds=0.02, stride_seconds=0.01)
        kw.update(case['kwargs'])
        W, H, max_lag = correlogram_sizes(kw['sample_rate_hz'], kw['max_lag_seconds'], kw['window_size_seconds'],
                                          kw['stride_seconds'])
        L = 2 * max_lag + 1
        sig = np.stack([to_float32(np.asarray(x)), to_float32(np.asarray(y))], axis=1)
        h = Harness(torch, ctx, 2, M, W, H, L)
        voices = {0: [Voice(sig, start_call=1)], 1: [Voice(noise(len(sig) + 333, i, 10.0))]}
        drive(h, voices, np.random.default_rng(i), [0, 1, M])
        check_voices(an, voices, W, H, L)
        got = np.concatenate(voices[0][0].out)
        assert got.shape == ref.shape, name
        assert np.abs(got.astype(np.float64) - ref).max(initial=0) <= (2 * W + 4) * 2.0 ** -24, name
        if name in ('huge_16k',):
            assert len(got) and not got.any()
        if name == 'silent_16k':
            assert not got[5].any()                          # a window inside the silence
        seen += 1
    assert seen == len(manifest['cases']) >= 11


# ---- 3. lockstep ------------------------------------------------------------------------------------------------------
def test_lockstep_equals_the_lockstep_stream_call_by_call(torch, ctx, an):
    from vndecorrelate_amd import _native
    S, M, W, H, L = 5, 300, 64, 24, 127
    h = Harness(torch, ctx, S, M, W, H, L, planar=True)
    dev = h.dev
    need = _native.correlogram_stream_state_bytes(S, W, M)
    lock_state = torch.full((need // 4,), float('nan'), dtype=torch.float32, device=dev)
    sizes = [300, 0, 37, 63, 24, 1, 300, 100]
    x = np.stack([noise(sum(sizes), 50 + b) for b in range(S)])
    pos = 0
    for i, n in enumerate(sizes):
        block = x[:, pos:pos + n]
        flags = np.full(S, START if i == 0 else 0, np.int32)
        rows = h.call(list(block), np.full(S, n, np.int32), flags)
        rc = an.stream_rows(pos, n, W, H)
        out = torch.full((S, rc[1] - rc[0], L), float('nan'), dtype=torch.float32, device=dev)
        got = _native.correlogram_stream_device(ctx, lock_state.data_ptr(), need, M, h.chunk[0].data_ptr(), h.chunk[1].data_ptr(),
                                                M, 1, out.data_ptr(), S, pos, n, window=W, hop=H, num_lags=L, eps=EPS,
                                                stream=h.stream())
        assert got == rc[1] - rc[0]
        want = out.cpu().numpy()
        for b in range(S):
            assert bits_equal(rows[b], want[b]), (i, b)
        pos += n
    assert pos > 10 * W


# ---- 4. every grid form -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S,groups', [(7, 1), (257, 2), (513, 3)])
def test_pools_of_one_two_and_three_advance_groups(torch, ctx, an, S, groups):
    W, H, L, M = 64, 24, 127, 100
    plan = plan_of(ctx, S, W, H, L, M)
    assert plan['advance_groups'] == groups and plan['rows_per_call'] == 5 and plan['groups'] == 2   # RC no multiple of 4
    assert plan['nblocks'] == S * 2 and (S - 1) % 256 == (0 if groups > 1 else 6)
    h = Harness(torch, ctx, S, M, W, H, L)
    rng = np.random.default_rng(S)
    x = noise(260, S)
    sizes = [100, 100, 60]
    late = rng.random(S) < 0.3                               # these slots start one call later, on the same signal
    late[-1] = False
    got = [[] for _ in range(S)]
    for i in range(len(sizes) + 1):
        counts, flags, blocks = np.zeros(S, np.int32), np.zeros(S, np.int32), [None] * S
        for b in range(S):
            k = i - int(late[b])
            if 0 <= k < len(sizes):
                p = sum(sizes[:k])
                blocks[b], counts[b] = x[p:p + sizes[k]], sizes[k]
                flags[b] = (START if k == 0 else 0) | (END if k == len(sizes) - 1 else 0)
        for b, r in enumerate(h.call(blocks, counts, flags)):
            got[b].append(r)
    want = one_shot(an, x, W, H, L)
    assert len(want) == 9
    for b in range(S):
        assert bits_equal(np.concatenate(got[b]), want), b
    assert not h.positions().any()


def test_full_blocks_beside_single_frames(torch, ctx, an):
    """RC a multiple of 4 (M = 768, H = 24: 32 rows, 8 window groups), and workgroups past out_counts[b]: slots 0, 2, 4 push
    M frames a call, the others 63 frames and then one frame a call."""
    S, W, H, L, M = 6, 64, 24, 127, 768
    plan = plan_of(ctx, S, W, H, L, M)
    assert plan['rows_per_call'] == 32 and plan['groups'] == 8 and plan['nblocks'] == 48
    h = Harness(torch, ctx, S, M, W, H, L)
    full, single = noise(3 * M, 3), noise(63 + 3, 4)
    got = [[] for _ in range(S)]
    for i in range(4):
        small = single[:63] if i == 0 else single[62 + i:63 + i]
        blocks = [(full[i * M:(i + 1) * M] if i < 3 else None) if b % 2 == 0 else small for b in range(S)]
        counts = np.array([0 if blk is None else len(blk) for blk in blocks], np.int32)
        flags = np.full(S, (START if i == 0 else 0) | (END if i == 3 else 0), np.int32)
        for b, r in enumerate(h.call(blocks, counts, flags)):
            got[b].append(r)
    for b in range(S):
        want = one_shot(an, full if b % 2 == 0 else single, W, H, L)
        assert len(want) == ((3 * M - W) // H + 1 if b % 2 == 0 else 1) and bits_equal(np.concatenate(got[b]), want), b


# ---- 5. positions -----------------------------------------------------------------------------------------------------
PLANTED = (2 ** 31 - 7, 2 ** 32 - 300, 2 ** 40 + 3, None)        # None: 2^60 less the frames pushed


@pytest.mark.parametrize('position', PLANTED, ids=['2^31-7', '2^32-300', '2^40+3', 'ends-at-2^60'])
def test_planted_position(torch, ctx, an, position):
    """Slot 1 at position P has wc(P) windows behind it; window wc(P) starts at frame A = wc(P) x hop, in (P - W, P].  The
    signal starts at A: its frames below P go into the ring, the rest is pushed.  The ring frames [P - W + 1, A) are within
    reach of P but belong to no pending window: they hold loud noise, everything else NaN, and no row may show either."""
    S, W, H, L, M, n = 3, 320, 160, 641, 333, 1500
    P = 2 ** 60 - n if position is None else position
    A = ((P - W) // H + 1) * H
    held = P - A
    assert 0 < held < W - 1
    x = noise(held + n, 17 + P % 107)
    h = Harness(torch, ctx, S, M, W, H, L)
    history = np.random.default_rng(P % 109).uniform(-1e3, 1e3, (W - 1, 2)).astype(np.float32)
    history[W - 1 - held:] = x[:held]
    h.plant(1, P, history)
    other = noise(n, 5)
    rng = np.random.default_rng(P % 113)
    got, mine, pushed, first = [], [], 0, True
    while pushed < n:
        b = int(min(n - pushed, rng.choice([0, 1, int(rng.integers(0, M + 1)), M])))
        blocks = [other[pushed:pushed + b], x[held + pushed:held + pushed + b], None]
        flags = np.array([START if first else 0, END if pushed + b == n else 0, 0], np.int32)
        rows = h.call(blocks, np.array([b, b, 0], np.int32), flags)
        mine.append(rows[0])
        got.append(rows[1])
        pushed, first = pushed + b, False
    if position is None:
        assert P + n == 2 ** 60
    want = one_shot(an, x, W, H, L)
    assert bits_equal(np.concatenate(got), want) and len(want) == (held + n - W) // H + 1
    assert bits_equal(np.concatenate(mine), one_shot(an, other, W, H, L))
    assert h.positions().tolist() == [n, 0, 0]


def test_a_position_past_2_to_60_answers_minus_one_until_a_start(torch, ctx, an):
    S, W, H, L, M = 3, 64, 24, 127, 100
    h = Harness(torch, ctx, S, M, W, H, L)
    x = noise(300, 8)
    a = h.call([x[:100], None, x[:100]], [100, 0, 100], [START, 0, START])
    h.plant(1, 2 ** 60 + 1, np.zeros((0, 2), np.float32))
    ring = h.ring()
    b = h.call([x[100:200], x[:100], x[100:200]], [100, 100, 100], [0, 0, 0])         # the harness holds oc[1] to the mirror: -1
    assert h.oc.cpu().numpy()[1] == -1 and h.positions()[1] == 2 ** 60 + 1
    assert np.array_equal(h.ring()[1], ring[1])                                       # the slot's ring is untouched
    c = h.call([x[200:], x[:100], x[200:]], [100, 100, 100], [END, START, END])       # the slot works again with START
    d = h.call([None, x[100:200], None], [0, 100, 0], [0, 0, 0])
    e = h.call([None, x[200:], None], [0, 100, 0], [0, END, 0])
    want = one_shot(an, x, W, H, L)
    assert bits_equal(np.concatenate([c[1], d[1], e[1]]), want)
    for slot in (0, 2):
        assert bits_equal(np.concatenate([a[slot], b[slot], c[slot]]), want), slot


@pytest.mark.parametrize('bad_count', [101, -1, 2 ** 31 - 1, -2 ** 31])
def test_a_bad_count_leaves_the_slot_and_its_neighbours_alone(torch, ctx, an, bad_count):
    S, W, H, L, M = 4, 64, 24, 127, 100
    x = [noise(300, 20 + b) for b in range(S)]
    clean = Harness(torch, ctx, S, M, W, H, L)
    spoiled = Harness(torch, ctx, S, M, W, H, L)
    got = [[] for _ in range(S)]
    for i in range(3):
        blocks = [x[b][100 * i:100 * i + 100] for b in range(S)]
        counts = np.full(S, 100, np.int32)
        flags = np.full(S, (START if i == 0 else 0) | (END if i == 2 else 0), np.int32)
        want = clean.call(blocks, counts, flags)
        if i == 1:                                               # slot 2, live since call 0, sends a bad count
            bad = counts.copy()
            bad[2] = bad_count
            before, ring = spoiled.positions(), spoiled.ring()
            rows = spoiled.call(blocks, bad, flags)
            assert spoiled.oc.cpu().numpy()[2] == -1 and spoiled.positions()[2] == before[2] == 100
            assert np.array_equal(spoiled.ring()[2], ring[2])
            for b in (0, 1, 3):
                assert bits_equal(rows[b], want[b]), b
                got[b].append(rows[b])
            only = np.zeros(S, np.int32)                         # the voice goes on: the block it meant to push
            only[2] = 100
            got[2].append(spoiled.call(blocks, only, np.zeros(S, np.int32))[2])
            assert bits_equal(got[2][-1], want[2])
        else:
            rows = spoiled.call(blocks, counts, flags)
            for b in range(S):
                assert bits_equal(rows[b], want[b]), (i, b)
                got[b].append(rows[b])
    for b in range(S):
        assert bits_equal(np.concatenate(got[b]), one_shot(an, x[b], W, H, L)), b


# ---- 6. the Python pool: capture, metering a decorrelating pool, the dict form --------------------------------------
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


def test_graph_replay_equals_the_uncaptured_run(torch, ctx, an):
    S, M = 6, 600
    dev = torch.device('cuda', ctx.device)
    calls = device_schedule(S, M, 3)
    results = []
    for replayed in (False, True):
        pool = an.cross_correlogram_voice_pool(S, sample_rate_hz=16000, max_frames_per_call=M)
        assert (pool.window, pool.hop, pool.num_lags, pool.rows_per_call) == (320, 160, 641, 4)
        x = torch.empty((S, M, 2), dtype=torch.float32, device=dev)
        counts, flags, oc = (torch.empty(S, dtype=torch.int32, device=dev) for _ in range(3))
        rows = torch.empty((S, pool.rows_per_call, pool.num_lags), dtype=torch.int32, device=dev)
        out = (rows.view(torch.float32), oc)
        pool.reset()
        graph = None
        if replayed:
            graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
            with torch.cuda.graph(graph, stream=side):
                pool.process_dev(x, counts, flags, out=out)
            torch.cuda.synchronize(dev)
        got = []
        for xh, c, f in calls:
            x.copy_(torch.from_numpy(xh))
            counts.copy_(torch.from_numpy(c))
            flags.copy_(torch.from_numpy(f))
            rows.fill_(POISON)
            if graph is not None:
                graph.replay()
            else:
                pool.process_dev(x, counts, flags, out=out)
            torch.cuda.synchronize(dev)
            got.append((rows.cpu().numpy(), oc.cpu().numpy()))
        with pytest.raises(RuntimeError, match='runs through process_dev'):
            pool.process({})
        results.append(got)
    pos = np.zeros(S, np.int64)
    for i, ((r0, c0), (r1, c1)) in enumerate(zip(*results)):
        want, pos = an.correlogram_voice_spans(pos, calls[i][1], calls[i][2], 320, 160, M)
        assert c0.tolist() == want.tolist() == c1.tolist(), i
        assert r0.tobytes() == r1.tobytes(), i
        for b, n in enumerate(want):
            assert not (r0[b, :n] == POISON).any() and (r0[b, n:] == POISON).all(), (i, b)
    assert any(n > 0 for _, c in results[0] for n in c) and not pos.any()


def _meter_run(torch, ctx, an, pool, meter, extra, voices, stage_counts):
    """`pool` and `meter` captured together in one graph; voices: per slot (signal, bank entry).  Every slot starts on call
    0 and pushes blocks of its own sizes, END with its last block.  After call 0 a replay carries a bad count for slot 2
    and nothing for the others: stage_counts() - every stage's out_counts - must answer -1 for it, and the voice goes on.
    Returns the rows per slot."""
    S, M = pool.slots, pool.max_frames_per_call
    dev = torch.device('cuda', ctx.device)
    x = torch.empty((S, M, 2), dtype=torch.float32, device=dev)
    counts, flags, oc = (torch.empty(S, dtype=torch.int32, device=dev) for _ in range(3))
    rows = torch.empty((S, meter.rows_per_call, meter.num_lags), dtype=torch.int32, device=dev)
    pool.reset()
    meter.reset()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
    with torch.cuda.graph(graph, stream=side):
        y, mid = pool.process_dev(x, counts, flags, *extra)
        meter.process_dev(y, mid, flags, out=(rows.view(torch.float32), oc))
    torch.cuda.synchronize(dev)

    def replay(xh, c, f):
        for t, v in ((x, xh), (counts, c), (flags, f)):
            t.copy_(torch.from_numpy(v))
        rows.fill_(POISON)
        graph.replay()
        torch.cuda.synchronize(dev)
        return rows.cpu().numpy(), oc.cpu().numpy()
    rng = np.random.default_rng(S)
    pushed, started, got, call = [0] * S, [False] * S, [[] for _ in range(S)], 0
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
        rh, ch = replay(xh, c, f)
        for b in range(S):
            n = int(ch[b])
            assert n >= 0 and not (rh[b, :n] == POISON).any() and (rh[b, n:] == POISON).all(), (call, b)
            got[b].append(rh[b, :n].view(np.float32).copy())
        if call == 0:
            assert pushed[2] is not None
            bad = np.zeros(S, np.int32)
            bad[2] = M + 1
            rh, ch = replay(xh, bad, np.zeros(S, np.int32))
            assert [int(t.cpu()[2]) for t in stage_counts(mid)] + [int(ch[2])] == [-1] * (len(stage_counts(mid)) + 1)
            assert (rh == POISON).all() and [int(v) for v in ch[[0, 1, 3]]] == [0, 0, 0]
        call += 1
    return [np.concatenate(g) for g in got]


def test_metering_a_chain_voice_pool_in_one_graph(torch, ctx, an):
    import vndecorrelate_amd.decorrelation as dec
    from test_gpu_chain_voice_pool import FS, _bank
    S, M = 4, 600
    bank = _bank(dec, 'ms>lr-ch1')
    pool = dec.decorrelate_voice_pool(bank, slots=S, in_channels=2, max_frames_per_call=M)
    meter = an.cross_correlogram_voice_pool(S, sample_rate_hz=FS, max_frames_per_call=pool.row_frames, dtype='float64')
    dev = torch.device('cuda', ctx.device)
    entries = np.array([3, 0, 2, 1])
    extra = (torch.from_numpy(pool.bank_tables[entries].astype(np.int32)).to(dev),
             torch.from_numpy(pool.bank_delays[entries].astype(np.int32)).to(dev))
    voices = [(noise(n, 60 + b), int(entries[b])) for b, n in enumerate((1700, 1900, 2300, 2201))]
    got = _meter_run(torch, ctx, an, pool, meter, extra, voices, lambda mid: (pool._mid[1], mid))    # -1 from all three stages
    for b, (sig, entry) in enumerate(voices):
        want = an.cross_correlogram_batched(bank[entry](sig)[None], sample_rate_hz=FS)[0]
        assert len(want) > 8 and bits_equal(got[b], np.asarray(want)), b


def test_metering_a_velvet_voice_pool_in_one_graph(torch, ctx, an):
    import vndecorrelate_amd.decorrelation as dec
    from test_gpu_chain_voice_pool import DURATION, FS, IMPULSES, KAPPAS, SEED
    S, M = 4, 600
    bank = [dec.VelvetNoise(sample_rate_hz=FS, duration_seconds=DURATION, num_impulses=IMPULSES, seed=SEED, normalizer=None,
                            log_distribution_strength=k) for k in KAPPAS]
    pool = dec.decorrelate_voice_pool(bank, slots=S, in_channels=2, max_frames_per_call=M)
    meter = an.cross_correlogram_voice_pool(S, sample_rate_hz=FS, max_frames_per_call=pool.row_frames)
    dev = torch.device('cuda', ctx.device)
    entries = np.array([3, 0, 2, 1])
    extra = (torch.from_numpy(pool.bank_tables[entries].astype(np.int32)).to(dev),)
    voices = [(noise(n, 70 + b), int(entries[b])) for b, n in enumerate((1700, 1900, 2300, 2201))]
    got = _meter_run(torch, ctx, an, pool, meter, extra, voices, lambda mid: (mid,))
    for b, (sig, entry) in enumerate(voices):
        want = an.cross_correlogram_batched(bank[entry].decorrelate(sig)[None], sample_rate_hz=FS)[0]
        assert len(want) > 8 and bits_equal(got[b], np.asarray(want)), b


def test_dict_form_equals_the_batched_call_per_voice(an):
    S, M = 4, 480
    pool = an.cross_correlogram_voice_pool(S, sample_rate_hz=16000, max_frames_per_call=M)
    rng = np.random.default_rng(9)
    sigs = {0: noise(1500, 1), 1: noise(2000, 2, dtype=np.float64), 2: noise(300, 3), 3: noise(961, 4)}
    got, pushed = {s: [] for s in sigs}, {s: 0 for s in sigs}
    first = True
    while pushed:
        blocks, end = {}, []
        for s in list(pushed):
            n = int(min(len(sigs[s]) - pushed[s], rng.choice([0, 1, M, int(rng.integers(0, M + 1))])))
            blocks[s] = sigs[s][pushed[s]:pushed[s] + n]
            pushed[s] += n
            if pushed[s] == len(sigs[s]):
                end.append(s)
                del pushed[s]
        out = pool.process(blocks, start=list(sigs) if first else [], end=end)
        if first:
            assert pool.transfers == {'to_device': 1, 'to_host': 1}
        first = False
        assert sorted(out) == sorted(blocks)
        for s, r in out.items():
            assert r.dtype == np.float32 and r.ndim == 2 and r.shape[1] == pool.num_lags
            got[s].append(r)
    for s, sig in sigs.items():
        want = an.cross_correlogram_batched(sig[None], sample_rate_hz=16000)[0]
        assert bits_equal(np.concatenate(got[s]), np.asarray(want)), s
    assert not pool.positions.any() and not pool.live.any()
    again = pool.process({2: sigs[0][:480]}, start=[2], end=[2])                      # a reused slot, a whole voice in one block
    assert bits_equal(again[2], np.asarray(an.cross_correlogram_batched(sigs[0][None, :480], sample_rate_hz=16000)[0]))
    with pytest.raises(RuntimeError, match='runs through process\\(\\)'):
        pool.process_dev(None, None, None)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------
def test_bad_arguments_write_nothing(torch, ctx, an):
    from vndecorrelate_amd import _native
    lib = ctx._lib
    S, W, H, L, M = 2, 20, 10, 21, 100
    h = Harness(torch, ctx, S, M, W, H, L, planar=True, reset=False)
    h.upload([np.ones((M, 2), np.float32)] * S, [M] * S, [START] * S)
    state, out, x = h.state.data_ptr(), h.out.data_ptr(), h.chunk.data_ptr()
    invalid = [dict(state_bytes=h.need - 1), dict(M=0), dict(S=0), dict(S=-1), dict(ss=0), dict(fs=0), dict(W=0), dict(H=0),
               dict(L=0), dict(H=-3), dict(state=0), dict(state=state + 8), dict(x=0), dict(y=0), dict(out=0), dict(counts=0),
               dict(flags=0), dict(oc=0), dict(out=x), dict(out=state), dict(x=state), dict(y=state), dict(ss=2 ** 62),
               dict(M=2 ** 31), dict(ctx=None)]
    for kw in invalid:
        assert h.raw(**kw) == INVALID, kw
        assert lib.vnd_last_error()
    unsupported = [dict(W=an.MAX_WINDOW + 1, state_bytes=2 ** 40), dict(S=65536, state_bytes=2 ** 40),
                   dict(M=2 ** 20, H=1, state_bytes=2 ** 40),                       # 2^18 window groups per slot
                   dict(M=2 ** 18, H=8, S=40000, state_bytes=2 ** 50),              # 2^13 groups x 40000 slots > 2^23
                   dict(M=2 ** 24, H=2 ** 10, L=2 ** 22, S=60000, state_bytes=2 ** 50)]  # out above 2^40 values
    for kw in unsupported:
        assert h.raw(**kw) == UNSUPPORTED, (kw, lib.vnd_last_error())
    assert b'values' in lib.vnd_last_error()
    null = ctypes.c_void_p(None)
    need = ctypes.c_int64(-7)
    assert lib.vnd_correlogram_voice_stream_state_bytes(S, W, 0, ctypes.byref(need)) == INVALID and need.value == 0
    assert lib.vnd_correlogram_voice_stream_state_bytes(S, an.MAX_WINDOW + 1, M, ctypes.byref(need)) == UNSUPPORTED
    assert lib.vnd_correlogram_voice_stream_reset_dev(ctx.handle, null, h.need, S, W, M, null) == INVALID
    assert lib.vnd_correlogram_voice_stream_reset_dev(ctx.handle, ctypes.c_void_p(state), h.need - 1, S, W, M, null) == INVALID
    assert lib.vnd_correlogram_voice_stream_reset_dev(ctx.handle, ctypes.c_void_p(state + 4), h.need, S, W, M, null) == INVALID
    text = ctypes.create_string_buffer(256)
    assert lib.vnd_describe_correlogram_voice_stream_launch(S, W, H, L, 2 ** 20 * H, text, 256) == UNSUPPORTED
    assert not text.value
    torch.cuda.synchronize(h.dev)
    assert (h.out == POISON).all() and torch.isnan(h.state).all() and (h.oc == -77).all()
    h.reset()
    h.mirror = np.zeros(S, np.int64)
    rows = h.call([np.ones((M, 2), np.float32)] * S, [M] * S, [START] * S)            # the good call writes
    assert all(len(r) == 9 for r in rows)
