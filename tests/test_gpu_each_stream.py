"""GPU tier of decorrelate_each_stream (vnd_each_stream_f32_*, vnd_haas_each_stream_f64_*, include/vnd_each_stream.h):
a pool streamed block by block with its own filter or delay per stream.  Every comparison is bit for bit.

The C ABI runs on torch device buffers through a poisoned harness, after test_gpu_stream_plans.py: the ring state starts
as NaN, every call's output starts as a NaN no arithmetic produces and ends in a sentinel tail of one r = 4 tile; after
each call *n_out is streaming.output_span's at the BANK's latency, every output frame was written and the tail was not.
The concatenated outputs of stream b equal the C oracle on the whole signal with that stream's own table, then
encode_side and apply_stereo_width (O.decorrelate's order).  Each case names the tile (r) the planner must report
(vnd_describe_each_stream_launch); the pools that reach r = 2 and r = 4 are sized from the device's CU count.

The planted-position cases start a stream at a position a long-lived one reaches (2^31 .. 2^60) without pushing that
many frames: the header documents the ring - slot = absolute frame mod capacity - so the frames below the position are
written there by that rule and everything else stays NaN."""
import contextlib
import ctypes
import io
import itertools

import numpy as np
import pytest

from oracle import c_oracle
from oracle import vnd_oracle as O

pytestmark = pytest.mark.gpu

FS, DURATION, IMPULSES, SEED = 16000, 0.02, 15, 1        # a small filter: 320 frames, 15 taps
POISON = 0x7FA5A5A5          # a signalling NaN: no kernel arithmetic yields it, so it marks frames nobody wrote
SENTINEL = 0x7FB0B0B0        # the tail behind n_out
TAIL = 2048                  # frames of sentinel per call: one tile at r = 4
THREADS = 16                 # C-oracle threads
SIZES = (1, 200, 511, 512, 513, 2049, 5000)               # 200: shorter than H
KAPPAS = (0.0, 0.3, 0.55, 0.3, 0.8, 1.0)                  # streams 1 and 3 share a kappa: 5 tables serve 6 streams
INVALID, UNSUPPORTED = 1, 4
MAX_POSITION = 1 << 60       # the largest position every block stream takes
# 2^31 - 7: the first block crosses 2^31; 2^32 - 300: pos - reach and pos straddle 2^32; None: 2^60 less the frames pushed
PLANTED = (2 ** 31 - 7, 2 ** 32 - 300, 2 ** 40 + 3, None)
PLANTED_IDS = ['2^31-7', '2^32-300', '2^40+3', 'ends-at-2^60']


@pytest.fixture(scope='module')
def ctx():
    from vndecorrelate_amd import _native
    context = _native.default_context()
    assert 'gfx950' in context.info()['name']
    return context


@pytest.fixture
def dec(ctx):
    import vndecorrelate_amd.decorrelation as decorrelation
    decorrelation.set_each_device(False)
    yield decorrelation
    decorrelation.set_each_device(None)
    decorrelation.set_device_epilogue(None)


def _taps(kappa, *, filtered=(0,), envelope=O.DEFAULT_ENVELOPE, seed=SEED):
    return O.generate_class_taps(sample_rate_hz=FS, duration_seconds=DURATION, num_impulses=IMPULSES,
                                 segment_envelope=envelope, log_distribution_strength=kappa,
                                 filtered_channels=filtered, seed=seed)


def _members(envelope, filtered):
    """The file's bank of 5 distinct kappas (one- or two-sided members), as class_path_bank_arrays triples."""
    env = tuple(envelope)
    return [(_taps(k, filtered=filtered, envelope=env, seed=SEED + i), env, env != (1.0,))
            for i, k in enumerate(sorted(set(KAPPAS)))]


TABLES = np.array([sorted(set(KAPPAS)).index(k) for k in KAPPAS], np.int32)


def _noise(shape, seed):
    return np.random.default_rng(seed).uniform(-1, 1, shape).astype(np.float32)


class Bank:
    """A bank on the device, the arrays of each of its candidates alone (the oracle's tables), and its latency."""

    def __init__(self, ctx, arrays, alone):
        from vndecorrelate_amd import _native
        self.ctx, self.arrays, self.alone = ctx, arrays, alone
        self.table = _native.TapTable.create(ctx, arrays.tap_offsets, arrays.tap_index, arrays.tap_weight, **arrays.kwargs())
        self.H = int(arrays.tap_index.max())
        assert self.table.max_index == self.H

    @classmethod
    def of_members(cls, ctx, members):
        from vndecorrelate_amd.taps import class_path_arrays, class_path_bank_arrays
        return cls(ctx, class_path_bank_arrays(members), [class_path_arrays(*m) for m in members])

    def close(self):
        self.table.close()

    def reference(self, x, tables, cx, epi):
        """(S, n, 2): stream b through candidate tables[b] alone by the C oracle, then the pointwise epilogue."""
        ms, width = epi
        xf = np.ascontiguousarray(x[..., np.arange(2) % cx])
        want = np.empty(x.shape[:2] + (2,), np.float32)
        for t in np.unique(tables):
            rows = np.flatnonzero(tables == t)
            a = self.alone[int(t)]
            want[rows] = c_oracle.convolve(xf[rows], a.tap_offsets, a.tap_index, a.tap_weight, seg_off=a.seg_offsets,
                                           seg_end=a.seg_end, seg_gain=a.seg_gain, chan_flags=a.chan_flags,
                                           apply_gain=a.apply_gain, threads=THREADS)
        for b in range(len(want)):
            if ms:
                O.encode_side(xf[b], want[b])
            if width is not None:
                O.apply_stereo_width(want[b], width)
        return want


def _function_bank(ctx):
    """A bank whose weights are not +-1 (a function-path table: the gains folded into the weights), 3 candidates."""
    from vndecorrelate_amd.taps import function_path_arrays
    fir = O.generate_velvet_noise(duration_seconds=DURATION, num_impulses=IMPULSES, num_outs=6, sample_rate_hz=FS,
                                  segment_envelope=(1.0, 0.5, 0.25), log_distribution_strength=0.6, seed=3)
    bank = Bank(ctx, function_path_arrays(fir), [function_path_arrays(fir[:, 2 * c:2 * c + 2]) for c in range(3)])
    bank.fir = fir
    return bank


def _ring_slots(position, reach, cap):
    """The ring slots of the absolute frames [position - reach, position): Python integers, so nothing wraps."""
    return np.array([(position - reach + j) % cap for j in range(reach)], np.int64)


class Poisoned:
    """One pool's state (NaN-filled once, at construction) and the calls of vnd_each_stream_f32_dev on it."""

    def __init__(self, bank, tables, cx, M, epi):
        import torch
        from vndecorrelate_amd import _native
        self.torch, self.bank, self.ctx = torch, bank, bank.ctx
        self.tables, self.S, self.cx, self.M = np.asarray(tables, np.int32), len(tables), cx, M
        self.ms, self.width = epi
        self.dev = torch.device('cuda', self.ctx.device)
        self.state_bytes = _native.each_stream_state_bytes(bank.table, self.S, cx, M)
        assert self.state_bytes == self.S * (bank.H + M) * cx * 4
        self.state = torch.full((max(self.state_bytes // 4, 1),), float('nan'), dtype=torch.float32, device=self.dev)
        self.index = torch.from_numpy(self.tables).to(self.dev)
        self.plans = []                       # (n_out, {field: value}) of every frame-computing call

    def describe(self, pos, n_in, final):
        text = self.bank.table.describe_each_stream(self.M, self.S, pos, n_in, self.cx, final, 0,
                                                    self.ms or self.width is not None)
        head, *fields = text.split()
        assert head == 'each_stream'
        return {k: int(v) for k, v in (f.split('=') for f in fields)}

    def call(self, chunk, pos, n_in, final, *, mode=0, state_bytes=None, M=None):
        """One raw call on a poisoned output: (status, *n_out, the output buffer as int32 on the host)."""
        from vndecorrelate_amd.streaming import output_span
        torch = self.torch
        first, end = output_span(pos, n_in, self.bank.H, final)
        body = self.S * (end - first) * 2
        y = torch.full((body + TAIL * 2,), SENTINEL, dtype=torch.int32, device=self.dev)
        y[:body] = POISON
        got = ctypes.c_int64(-1)
        rc = self.ctx._lib.vnd_each_stream_f32_dev(
            self.ctx.handle, self.bank.table.handle, ctypes.c_void_p(self.index.data_ptr()),
            ctypes.c_void_p(self.state.data_ptr()), self.state_bytes if state_bytes is None else state_bytes,
            self.M if M is None else M, ctypes.c_void_p(chunk.data_ptr()), ctypes.c_void_p(y.data_ptr()), self.S, pos, n_in,
            self.cx, int(final), mode, int(self.ms), int(self.width is not None), float(self.width or 0.0),
            ctypes.byref(got), ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream))
        return rc, got.value, y.cpu().numpy(), end - first

    def plant(self, position, history):
        """The H frames below `position` of every stream, (S, H, cx), into the ring slots the header names."""
        H, cap = self.bank.H, self.bank.H + self.M
        assert history.shape == (self.S, H, self.cx) and history.dtype == np.float32
        where = self.torch.from_numpy(_ring_slots(position, H, cap)).to(self.dev)
        self.state.view(self.S, cap, self.cx)[:, where] = self.torch.from_numpy(history).to(self.dev)

    def signal(self, x, calls, start=0):
        """x (S, n, cx); calls [(n_in, final)], the last one final: the concatenation of every call's outputs.  The
        first frame of x is absolute frame `start`."""
        xd = self.torch.from_numpy(np.ascontiguousarray(x)).to(self.dev)
        outs, pos = [], start
        for i, (n_in, final) in enumerate(calls):
            chunk = xd[:, pos - start:pos - start + n_in].contiguous()
            rc, got, yh, n_out = self.call(chunk, pos, n_in, final)
            assert rc == 0, self.ctx._lib.vnd_last_error()
            assert got == n_out, (i, got, n_out)
            body = self.S * n_out * 2
            assert (yh[body:] == SENTINEL).all(), f'call {i} (pos {pos}, n_in {n_in}) wrote past its {n_out} frames'
            hole = np.argwhere((yh[:body] == POISON).reshape(self.S, n_out, 2))
            assert not len(hole), f'call {i} (pos {pos}, n_in {n_in}) left (stream, frame, channel) {tuple(hole[0])} unwritten'
            if n_out:
                plan = self.describe(pos, n_in, final)
                assert plan['n_out'] == n_out and plan['nblocks'] == self.S * plan['tiles']
                assert plan['tiles'] == -(-n_out // (512 * plan['r']))
                self.plans.append((n_out, plan))
            outs.append(yh[:body].view(np.float32).reshape(self.S, n_out, 2))
            pos += n_in
        assert pos - start == x.shape[1] and calls[-1][1]
        return np.concatenate(outs, axis=1)


def _sizes(n, H, M, rng):
    """Block sizes summing to n, none above M: first calls that only fill the ring (pos + n_in <= H), then 0, 1, H, H + 1,
    M and random sizes in a shuffled order (test_gpu_stream_plans.py's)."""
    out, pos = [], 0
    for b in (1, 0, (H - 1) // 2, H):
        b = max(0, min(b, n - pos, M, H - pos))
        out.append(b)
        pos += b
    menu = [0, 1, H, H + 1, M, 17]
    order = [menu[i] for i in rng.permutation(len(menu))]
    while pos < n:
        b = min(order.pop() if order else int(rng.choice(menu + [int(rng.integers(1, M + 1))])), n - pos, M)
        out.append(b)
        pos += b
    return out


def _calls(sizes, ending):
    if ending == 'flush':
        return [(b, False) for b in sizes] + [(0, True)]
    return [(b, False) for b in sizes[:-1]] + [(sizes[-1], True)]


def _blocks(n, B):
    return [B] * (n // B) + ([n % B] if n % B else [])


def _same(got, want, where):
    assert got.shape == want.shape, (where, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
        raise AssertionError((where, 'first (stream, frame, channel)', tuple(bad[0]), len(bad),
                              float(got[tuple(bad[0])]), float(want[tuple(bad[0])])))


# ---- 1. frames, in every schedule ------------------------------------------------------------------------------------
@pytest.mark.parametrize('cx', [1, 2])
@pytest.mark.parametrize('envelope, filtered, epi', [
    (O.DEFAULT_ENVELOPE, (0,), (True, None)),             # the VelvetNoise defaults: one-sided, MS
    (O.DEFAULT_ENVELOPE, (0, 1), (False, 0.35)),          # two-sided, LR, width
    ((1.0,), (0,), (True, 0.35)),                         # the identity envelope: no gains
    ((1.0,), (0, 1), (False, None)),                      # ... and no pointwise steps at all
])
def test_frames_in_every_schedule(ctx, cx, envelope, filtered, epi):
    bank = Bank.of_members(ctx, _members(envelope, filtered))
    try:
        H, M = bank.H, 600
        assert 200 < H < 320
        for i, n in enumerate(SIZES):
            seed = 1000 * cx + 10 * i + len(envelope) + len(filtered)
            x = _noise((6, n, cx), seed)
            tables = np.roll(TABLES, i)
            want = bank.reference(x, tables, cx, epi)
            whole = Poisoned(bank, tables, cx, max(n, 1), epi)
            _same(whole.signal(x, [(n, True)]), want, ('whole', n))
            assert all(p['r'] == 1 for _, p in whole.plans)           # a small pool: the smallest tile
            _same(Poisoned(bank, tables, cx, 480, epi).signal(x, _calls(_blocks(n, 480) or [0], 'flush')), want,
                  ('480-frame blocks', n))
            rng = np.random.default_rng(seed)
            sizes = _sizes(n, H, M, rng)
            for ending in ('flush', 'final'):
                p = Poisoned(bank, tables, cx, M, epi)
                _same(p.signal(x, _calls(sizes, ending)), want, (ending, n, sizes))
            # a second, shorter signal on the same state after the final block: its ring still holds the first one's frames
            n2 = n // 2 + 1
            x2 = _noise((6, n2, cx), seed + 1)
            _same(p.signal(x2, _calls(_sizes(n2, H, M, rng), 'flush')), bank.reference(x2, tables, cx, epi),
                  ('second signal', n2))
    finally:
        bank.close()


@pytest.mark.parametrize('cx', [1, 2])
def test_function_path_bank_takes_the_exact_instantiation(ctx, cx):
    """A bank whose weights are not +-1 (a function-path table: the gains folded into the weights) runs the separate
    multiply and add; the plan says so."""
    bank = _function_bank(ctx)
    fir = bank.fir
    try:
        tables = np.array([2, 0, 1, 2], np.int32)
        for n, epi in ((513, (True, 0.35)), (2049, (False, None))):
            x = _noise((4, n, cx), 40 + n + cx)
            want = bank.reference(x, tables, cx, epi)
            for b, c in enumerate(tables):                         # ... which is the reference's own convolution
                conv = O.convolve_velvet_noise(np.ascontiguousarray(x[b][:, np.arange(2) % cx]), fir[:, 2 * c:2 * c + 2])
                if epi == (False, None):
                    assert conv.tobytes() == want[b].tobytes()
            p = Poisoned(bank, tables, cx, 700, epi)
            _same(p.signal(x, _calls(_sizes(n, bank.H, 700, np.random.default_rng(n)), 'final')), want, ('function path', n))
            assert p.plans and all(plan['fma'] == 0 for _, plan in p.plans)
    finally:
        bank.close()


# ---- 2. every tile ---------------------------------------------------------------------------------------------------
def _tile_cases():
    """each_stream_kernel<cx, MODE, r, EPI> in its 24 forms; the three cases that were here first keep their names."""
    cases = []
    for r, cx, path, epi in itertools.product((1, 2, 4), (2, 1), ('class', 'function'), ((True, 0.35), (False, None))):
        first = (cx, path, epi) == (2, 'class', (True, 0.35))
        cases.append(pytest.param(r, cx, path, epi, id=str(r) if first else f'{r}-cx{cx}-{path}-{"epi" if epi[0] else "plain"}'))
    return cases


@pytest.mark.parametrize('r, cx, path, epi', _tile_cases())
def test_every_tile(ctx, r, cx, path, epi):
    """The planner's rule, the largest tile that still leaves every CU six workgroups: a call of 2100 output frames is
    2 tiles at r = 4, 3 at r = 2 and 5 at r = 1, so pools of 3, 2 and (a few) x CU count streams reach each.  The
    class-path bank's +-1 weights take the fma instantiation, the function-path bank's the separate multiply and add."""
    cus = ctx.info()['compute_units']
    S = {4: 3 * cus, 2: 2 * cus, 1: 7}[r]
    bank = Bank.of_members(ctx, _members(O.DEFAULT_ENVELOPE, (0,))) if path == 'class' else _function_bank(ctx)
    try:
        H = bank.H
        first, last = H + 2100, 700                      # a call of 2100 outputs that fills the ring, then the final block
        tables = (np.arange(S) % len(bank.alone)).astype(np.int32)
        x = _noise((S, first + last, cx), 77 + r)
        want = bank.reference(x, tables, cx, epi)
        p = Poisoned(bank, tables, cx, first, epi)
        got = p.signal(x, [(first, False), (last, True)])
        assert [n_out for n_out, _ in p.plans] == [2100, last + H]
        assert p.plans[0][1]['r'] == r, p.plans
        assert p.plans[0][1]['tiles'] == {4: 2, 2: 3, 1: 5}[r]
        assert p.plans[0][1]['fma'] == int(path == 'class') and p.plans[0][1]['epilogue'] == int(epi[0])
        _same(got, want, ('tile', r))
        # a tile the call does not fill past half is never taken, however many streams there are
        assert p.describe(first, 480, False)['r'] == 1 and p.describe(first, 512, False)['r'] == 1
    finally:
        bank.close()


# ---- 2b. a stream that has been running for a day --------------------------------------------------------------------
@pytest.mark.parametrize('position', PLANTED, ids=PLANTED_IDS)
def test_planted_position(ctx, position):
    """The tap sum reads x[n .. n + H]: with the H frames below P in the ring, the outputs from frame P - H on are the
    oracle's on the signal that starts there, whole."""
    bank = Bank.of_members(ctx, _members(O.DEFAULT_ENVELOPE, (0,)))
    try:
        H, M, cx, epi = bank.H, 480, 2, (True, 0.35)
        n = 1700
        start = MAX_POSITION - n if position is None else position
        sig = _noise((6, H + n, cx), 90 + start % 97)
        rng = np.random.default_rng(start % 1009)
        sizes = [int(b) for b in rng.permutation([0, 1, 17, H, H + 1, M, M])]
        sizes.append(n - sum(sizes))
        assert 0 < sizes[-1] <= M
        p = Poisoned(bank, TABLES, cx, M, epi)
        p.plant(start, sig[:, :H])
        got = p.signal(sig[:, H:], _calls(sizes, 'flush' if position is None else 'final'), start=start)
        _same(got, bank.reference(sig, TABLES, cx, epi), ('planted at', start))
    finally:
        bank.close()


# ---- 3. the Python route ---------------------------------------------------------------------------------------------
def _velvets(dec, kappas, **kw):
    base = dict(sample_rate_hz=FS, duration_seconds=DURATION, num_impulses=IMPULSES, seed=SEED, normalizer=None)
    base.update(kw)
    return [dec.VelvetNoise(log_distribution_strength=k, **base) for k in kappas]


@pytest.mark.parametrize('cx', [1, 2])
@pytest.mark.parametrize('kw', [dict(), dict(mode='LR', width=0.35), dict(segment_envelope=(), filtered_channels=(0, 1))])
def test_python_route_equals_the_loop(dec, cx, kw):
    stages = _velvets(dec, KAPPAS, **kw)
    n, M = 2049, 600
    pool = np.random.default_rng(5 + cx).uniform(-1, 1, (6, n, cx))               # float64: cast as decorrelate casts it
    want = np.stack([d.decorrelate(pool[b, :, 0] if cx == 1 else pool[b]) for b, d in enumerate(stages)])
    s = dec.decorrelate_each_stream(stages, in_channels=cx, max_frames_per_call=M)
    assert s.latency_frames > 200
    rng = np.random.default_rng(9)
    for ending in ('flush', 'final'):
        sizes = _sizes(n, s.latency_frames, M, rng)
        outs, pos = [], 0
        for i, b in enumerate(sizes):
            final = ending == 'final' and i == len(sizes) - 1
            out = s.process(pool[:, pos:pos + b], final=final)
            assert isinstance(out, np.ndarray) and out.dtype == np.float32
            outs.append(out)
            pos += b
        if ending == 'flush':
            outs.append(s.flush())
        _same(np.concatenate(outs, axis=1), want, (ending, sizes))
        s.reset()


def test_device_blocks_on_a_side_stream_call_no_host_entry(dec, ctx, monkeypatch):
    import torch
    from vndecorrelate_amd import _native
    stages = _velvets(dec, KAPPAS)
    haas = [dec.HaasEffect(sample_rate_hz=FS, delay_time_seconds=d / FS, mode='MS', width=0.3) for d in (0, 3, 300, 77)]
    n = 1500
    pool = _noise((6, n, 2), 3)
    want = np.stack([d.decorrelate(pool[b]) for b, d in enumerate(stages)])
    want_h = [d.decorrelate(pool[b]) for b, d in enumerate(haas)]
    s = dec.decorrelate_each_stream(stages, max_frames_per_call=480)
    h = dec.decorrelate_each_stream(haas, max_frames_per_call=480)

    def refuse(*args, **kwargs):
        raise AssertionError('a host entry was called for a device block')
    lib = ctx._lib
    names = [n_ for n_ in _native.EACH_STREAM_SIGNATURES if n_.endswith('_host')] + ['vnd_stream_f32_host', 'vnd_haas_stream_f64_host']
    saved = {n_: getattr(lib, n_) for n_ in names}
    dev = torch.device('cuda', ctx.device)
    side = torch.cuda.Stream(dev)
    xd = torch.from_numpy(pool).to(dev)
    try:
        for n_ in names:
            setattr(lib, n_, refuse)
        outs, outs_h = [], []
        for i, first in enumerate(range(0, n, 480)):
            block = xd[:, first:first + 480]
            if i % 2:                                   # alternate streams: every call is ordered after the previous one
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    outs.append(s.process(block))
                    outs_h.append(h.process(block[:4]))
            else:
                outs.append(s.process(block))
                outs_h.append(h.process(block[:4]))
        outs.append(s.flush())
        outs_h.append(h.flush())
        assert all(isinstance(o, torch.Tensor) and o.is_cuda for o in outs + outs_h)
        torch.cuda.synchronize(dev)
    finally:
        for n_, fn in saved.items():
            setattr(lib, n_, fn)
    _same(torch.cat(outs, dim=1).cpu().numpy(), want, 'device blocks')
    got_h = torch.cat(outs_h, dim=1).cpu().numpy()
    for b, w in enumerate(want_h):
        assert got_h[b, :len(w)].tobytes() == w.tobytes(), b
        assert not got_h[b, len(w):].view(np.int64).any(), b


# ---- 4. independence -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cx', [1, 2])
def test_rows_depend_on_signal_and_table_only(ctx, cx):
    a, b, c = _taps(0.1), _taps(0.6), _taps(0.9, filtered=(0, 1), seed=2)
    env = tuple(O.DEFAULT_ENVELOPE)
    bank = Bank.of_members(ctx, [(m, env, True) for m in (a, b, c, a, b)])          # one table at two bank positions
    try:
        n, M, epi = 2049, 600, (True, 0.3)
        x = _noise((4, n, cx), 50 + cx)
        x[3] = x[0]                                                                # one signal at two stream indices
        calls = _calls(_sizes(n, bank.H, M, np.random.default_rng(1)), 'flush')
        rows = Poisoned(bank, [0, 1, 2, 3], cx, M, epi).signal(x, calls)
        assert rows[0].tobytes() == rows[3].tobytes()                              # tables 0 and 3 are the same table
        moved = Poisoned(bank, [3, 4, 2, 0], cx, M, epi).signal(x, calls)
        _same(moved, rows, 'the candidate\'s place in the bank')
        # the pool streamed whole and in two halves
        halves = [Poisoned(bank, [0, 1], cx, M, epi).signal(x[:2], calls), Poisoned(bank, [2, 3], cx, M, epi).signal(x[2:], calls)]
        _same(np.concatenate(halves), rows, 'two halves')
        # and another schedule of the same signal
        _same(Poisoned(bank, [0, 1, 2, 3], cx, n, epi).signal(x, [(n, True)]), rows, 'another schedule')
    finally:
        bank.close()


# ---- 5. bounds -------------------------------------------------------------------------------------------------------
def test_largest_index_4094_runs_and_4095_is_refused(ctx):
    from vndecorrelate_amd.taps import class_path_arrays, class_path_bank_arrays
    env = tuple(O.DEFAULT_ENVELOPE)

    def members(last):
        far = [[([7], [0, last])], None]                  # one segment: taps at 7 (negative), 0 and `last`
        return [(_taps(0.4), env, True), (far, env, True)]
    bank = Bank.of_members(ctx, members(4094))
    try:
        assert bank.H == 4094
        n, M = 4094 + 700, 480
        x = _noise((3, n, 2), 8)
        tables = np.array([1, 0, 1], np.int32)
        p = Poisoned(bank, tables, 2, M, (True, None))
        got = p.signal(x, _calls(_blocks(n, M), 'flush'))
        _same(got, bank.reference(x, tables, 2, (True, None)), 'index 4094')
        assert all(plan['W'] == 512 * plan['r'] + 4096 and plan['lds_bytes'] <= 48 * 1024 for _, plan in p.plans)
    finally:
        bank.close()
    from vndecorrelate_amd import _native
    arrays = class_path_bank_arrays(members(4095))
    table = _native.TapTable.create(ctx, arrays.tap_offsets, arrays.tap_index, arrays.tap_weight, **arrays.kwargs())
    try:
        import torch
        dev = torch.device('cuda', ctx.device)
        need = _native.each_stream_state_bytes(table, 1, 2, 480)
        state = torch.zeros(need // 4, dtype=torch.float32, device=dev)
        xd, yd, td = torch.zeros((1, 480, 2), device=dev), torch.full((1, 480, 2), 7.0, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        got = ctypes.c_int64(-1)
        rc = ctx._lib.vnd_each_stream_f32_dev(ctx.handle, table.handle, ctypes.c_void_p(td.data_ptr()),
                                              ctypes.c_void_p(state.data_ptr()), need, 480, ctypes.c_void_p(xd.data_ptr()),
                                              ctypes.c_void_p(yd.data_ptr()), 1, 0, 480, 2, 1, 0, 0, 0, 0.0, ctypes.byref(got), None)
        assert rc == UNSUPPORTED and b'4095' in ctx._lib.vnd_last_error() and got.value == 0
        torch.cuda.synchronize(dev)
        assert bool((yd == 7.0).all()) and not bool(state.any())
        with pytest.raises(_native.NativeError, match='4095'):
            table.describe_each_stream(480, 1, 0, 480, 2)
    finally:
        table.close()
    assert class_path_arrays(*members(4095)[1]).tap_index.max() == 4095


def test_a_bad_table_index_is_nan_for_that_stream_alone(ctx):
    from vndecorrelate_amd import _native
    bank = Bank.of_members(ctx, _members(O.DEFAULT_ENVELOPE, (0,)))
    try:
        n, M, epi = 1300, 480, (True, 0.35)
        x = _noise((5, n, 2), 21)
        good = np.array([0, 1, 2, 3, 4], np.int32)
        calls = _calls(_blocks(n, M), 'flush')
        want = Poisoned(bank, good, 2, M, epi).signal(x, calls)
        for bad_value in (5, -1, 2 ** 31 - 1):
            bad = good.copy()
            bad[2] = bad_value
            got = Poisoned(bank, bad, 2, M, epi).signal(x, calls)            # every frame written, none past n_out
            assert np.isnan(got[2]).all(), bad_value
            keep = [0, 1, 3, 4]
            assert got[keep].tobytes() == want[keep].tobytes(), bad_value
            # the host entry names the stream and writes nothing
            p = Poisoned(bank, bad, 2, M, epi)
            state_before = p.state.clone()
            with pytest.raises(ValueError, match=rf'table {bad_value} of stream 2 is outside \[0, 5\)'):
                _native.each_stream_host(ctx, bank.table, bad, p.state.data_ptr(), p.state_bytes, M, x[:, :M].copy(),
                                         M - bank.H, 0, final=False, ms_encode=True, width=0.35)
            assert p.state.view(p.torch.int32).equal(state_before.view(p.torch.int32))
        # the host entry on a good pool is the device entry's
        p = Poisoned(bank, good, 2, M, epi)
        outs, pos = [], 0
        for n_in, final in calls:
            from vndecorrelate_amd.streaming import output_span
            first, end = output_span(pos, n_in, bank.H, final)
            outs.append(_native.each_stream_host(ctx, bank.table, good, p.state.data_ptr(), p.state_bytes, M,
                                                 np.ascontiguousarray(x[:, pos:pos + n_in]), end - first, pos, final=final,
                                                 ms_encode=True, width=0.35))
            pos += n_in
        _same(np.concatenate(outs, axis=1), want, 'host entry')
    finally:
        bank.close()


def test_an_invalid_call_leaves_output_and_ring_untouched(ctx):
    bank = Bank.of_members(ctx, _members(O.DEFAULT_ENVELOPE, (0,)))
    try:
        M = 480
        p = Poisoned(bank, TABLES, 2, M, (True, None))
        torch = p.torch
        chunk = torch.from_numpy(_noise((6, M + 1, 2), 4)).to(p.dev)
        before = p.state.clone()
        for kwargs, status, text in ((dict(n_in=M + 1), INVALID, b'above max_frames_per_call'),
                                     (dict(n_in=M, state_bytes=p.state_bytes - 4), INVALID, b'the stream needs'),
                                     (dict(n_in=M, mode=1), UNSUPPORTED, b'VND_MODE_EXACT only'),
                                     (dict(n_in=M, mode=2), UNSUPPORTED, b'VND_MODE_EXACT only'),
                                     (dict(n_in=M, pos=-1), INVALID, b'position'),
                                     (dict(n_in=M, pos=MAX_POSITION + 1), INVALID, b'position')):
            n_in = kwargs.pop('n_in')
            pos = kwargs.pop('pos', 0)
            rc, got, yh, n_out = p.call(chunk[:, :n_in].contiguous(), pos, n_in, True, **kwargs)
            assert rc == status and text in p.ctx._lib.vnd_last_error(), (kwargs, rc, p.ctx._lib.vnd_last_error())
            assert got == 0
            body = p.S * n_out * 2
            assert (yh[:body] == POISON).all() and (yh[body:] == SENTINEL).all()
            torch.cuda.synchronize(p.dev)
            assert p.state.view(torch.int32).equal(before.view(torch.int32))
    finally:
        bank.close()


# ---- 6. Haas ---------------------------------------------------------------------------------------------------------
class PoisonedHaas:
    """vnd_haas_each_stream_f64_dev on a NaN-filled ring and poisoned outputs."""

    def __init__(self, ctx, delays, max_delay, cx, M, settings):
        import torch
        from vndecorrelate_amd import _native
        self.torch, self.native, self.ctx = torch, _native, ctx
        self.delays, self.max_delay, self.S, self.cx, self.M = np.asarray(delays, np.int32), max_delay, len(delays), cx, M
        self.settings = settings
        self.dev = torch.device('cuda', ctx.device)
        self.state_bytes = _native.haas_each_stream_state_bytes(self.S, cx, max_delay, M)
        assert self.state_bytes == (self.S * (max_delay + M) * cx * 4 if max_delay else 0)
        self.state = torch.full((max(self.state_bytes // 4, 1),), float('nan'), dtype=torch.float32, device=self.dev)
        self.frames = torch.from_numpy(self.delays).to(self.dev)

    def plant(self, position, history):
        """The max_delay frames below `position` of every stream, (S, max_delay, cx), into the ring slots the header names."""
        D, cap = self.max_delay, self.max_delay + self.M
        assert history.shape == (self.S, D, self.cx) and history.dtype == np.float32
        where = self.torch.from_numpy(_ring_slots(position, D, cap)).to(self.dev)
        self.state.view(self.S, cap, self.cx)[:, where] = self.torch.from_numpy(history).to(self.dev)

    def signal(self, x, calls, start=0):
        torch = self.torch
        xd = torch.from_numpy(np.ascontiguousarray(x)).to(self.dev)
        poison = np.array([0x7FF4A5A5A5A5A5A5], np.int64)[0]
        sentinel = np.array([0x7FF5B0B0B0B0B0B0], np.int64)[0]
        outs, pos = [], start
        for i, (n_in, final) in enumerate(calls):
            n_out = n_in + (self.max_delay if final else 0)
            body = self.S * n_out * 2
            y = torch.full((body + 512,), int(sentinel), dtype=torch.int64, device=self.dev)
            y[:body] = int(poison)
            chunk = xd[:, pos - start:pos - start + n_in].contiguous()
            got = self.native.haas_each_stream_device(
                self.ctx, self.state.data_ptr(), self.state_bytes, self.M, chunk.data_ptr(), y.data_ptr(), self.S, pos, n_in,
                self.cx, self.frames.data_ptr(), final=final, max_delay=self.max_delay,
                stream=torch.cuda.current_stream(self.dev).cuda_stream, **self.settings)
            assert got == n_out, (i, got, n_out)
            yh = y.cpu().numpy()
            assert (yh[body:] == sentinel).all(), f'call {i} wrote past its {n_out} frames'
            assert not (yh[:body] == poison).any(), f'call {i} left frames unwritten'
            outs.append(yh[:body].view(np.float64).reshape(self.S, n_out, 2))
            pos += n_in
        assert pos - start == x.shape[1] and calls[-1][1]
        return np.concatenate(outs, axis=1)


def _check_haas(dec, got, x, delays, cx, settings, skip=0):
    """`got` against HaasEffect.decorrelate of x, from x's frame `skip` on (a stream that started there)."""
    n = x.shape[1]
    for b, d in enumerate(delays):
        stage = dec.HaasEffect(sample_rate_hz=1, delay_time_seconds=float(d), delayed_channel=settings['delayed_channel'],
                               mode='MS' if settings['ms_mode'] else 'LR', width=settings['width'])
        want = stage.decorrelate(x[b, :, 0] if cx == 1 else x[b])
        assert want.shape == (n + d, 2) and want.dtype == np.float64
        assert got[b, :n + d - skip].tobytes() == want[skip:].tobytes(), (b, d)
        assert not got[b, n + d - skip:].view(np.int64).any(), (b, d)            # +0.0, bit for bit


@pytest.mark.parametrize('cx', [1, 2])
@pytest.mark.parametrize('ms_mode, delayed_channel, width', [(False, 0, None), (True, 1, 0.3), (True, 0, None), (False, 1, 0.3)])
def test_haas_rows_are_numpys(dec, ctx, cx, ms_mode, delayed_channel, width):
    n = 600
    delays = [0, 1, 255, 256, 257, n - 1, n, n + 5]
    settings = dict(delayed_channel=delayed_channel, ms_mode=ms_mode, width=width)
    x = _noise((len(delays), n, cx), 60 + cx + 2 * ms_mode)
    rng = np.random.default_rng(cx)
    schedules = [_calls(_blocks(n, 1), 'final')] if (cx, ms_mode, delayed_channel) == (2, False, 0) else []
    schedules += [_calls(_blocks(n, 256), 'flush'), _calls(_blocks(n, 257), 'final'), [(n, True)],
                  _calls(_sizes(n, 256, 300, rng), 'flush'), _calls(_sizes(n, 257, 300, rng), 'final')]
    p = PoisonedHaas(ctx, delays, n + 5, cx, 600, settings)
    for calls in schedules:                               # one state for all of them: no clearing between signals
        _check_haas(dec, p.signal(x, calls), x, delays, cx, settings)
    # a max_delay above every stream's own: more padding, the same rows
    wide = PoisonedHaas(ctx, delays[:5], 300, cx, 256, settings)
    _check_haas(dec, wide.signal(x[:5], _calls(_blocks(n, 256), 'flush')), x[:5], delays[:5], cx, settings)
    # no delay anywhere: no state
    none = PoisonedHaas(ctx, [0, 0], 0, cx, 256, settings)
    _check_haas(dec, none.signal(x[:2], _calls(_blocks(n, 256), 'flush')), x[:2], [0, 0], cx, settings)


@pytest.mark.parametrize('position', PLANTED, ids=PLANTED_IDS)
def test_haas_planted_position(dec, ctx, position):
    """A delay reads x[f - d]: with the max_delay frames below P in the ring, the outputs from P on are NumPy's on the
    signal that starts at P - max_delay, from its frame max_delay on."""
    M, D, cx = 256, 300, 2
    delays = [0, 1, 255, 256, 257, D]
    settings = dict(delayed_channel=1, ms_mode=True, width=0.3)
    n = 700
    start = MAX_POSITION - n if position is None else position
    sig = _noise((len(delays), D + n, cx), 31 + start % 89)
    rng = np.random.default_rng(start % 1013)
    sizes = [int(b) for b in rng.permutation([0, 1, 17, M, M])]
    sizes.append(n - sum(sizes))
    assert 0 < sizes[-1] <= M
    p = PoisonedHaas(ctx, delays, D, cx, M, settings)
    p.plant(start, sig[:, :D])
    got = p.signal(sig[:, D:], _calls(sizes, 'flush' if position is None else 'final'), start=start)
    assert got.shape == (len(delays), n + D, 2)
    _check_haas(dec, got, sig, delays, cx, settings, skip=D)
    # one frame further the position is out of range: refused, and the ring keeps its bits
    before = p.state.clone()
    y = p.torch.full((len(delays) * M * 2,), 7.0, dtype=p.torch.float64, device=p.dev)
    chunk = p.torch.zeros((len(delays), M, cx), dtype=p.torch.float32, device=p.dev)
    with pytest.raises(ValueError, match='position'):
        p.native.haas_each_stream_device(ctx, p.state.data_ptr(), p.state_bytes, M, chunk.data_ptr(), y.data_ptr(), len(delays),
                                         MAX_POSITION + 1, M, cx, p.frames.data_ptr(), final=False, max_delay=D, **settings)
    p.torch.cuda.synchronize(p.dev)
    assert bool((y == 7.0).all()) and p.state.view(p.torch.int32).equal(before.view(p.torch.int32))


def test_a_bad_delay_is_nan_for_that_stream_alone(dec, ctx):
    from vndecorrelate_amd import _native
    n, M = 500, 256
    settings = dict(delayed_channel=0, ms_mode=False, width=None)
    x = _noise((4, n, 2), 13)
    calls = _calls(_blocks(n, M), 'flush')
    want = PoisonedHaas(ctx, [3, 40, 7, 0], 40, 2, M, settings).signal(x, calls)
    for bad_value in (41, -1, 2 ** 31 - 1):
        p = PoisonedHaas(ctx, [3, 40, bad_value, 0], 40, 2, M, settings)
        got = p.signal(x, calls)
        assert np.isnan(got[2]).all()
        assert got[[0, 1, 3]].tobytes() == want[[0, 1, 3]].tobytes()
        before = p.state.clone()
        with pytest.raises(ValueError, match=rf'delay {bad_value} of stream 2 is outside \[0, 40\]'):
            _native.haas_each_stream_host(ctx, p.state.data_ptr(), p.state_bytes, M, x[:, :M].copy(), [3, 40, bad_value, 0], 0,
                                          final=False, max_delay=40, **settings)
        assert p.state.view(p.torch.int32).equal(before.view(p.torch.int32))
    # the host entry on good delays is the device entry's
    p = PoisonedHaas(ctx, [3, 40, 7, 0], 40, 2, M, settings)
    outs, pos = [], 0
    for n_in, final in calls:
        outs.append(_native.haas_each_stream_host(ctx, p.state.data_ptr(), p.state_bytes, M,
                                                  np.ascontiguousarray(x[:, pos:pos + n_in]), [3, 40, 7, 0], pos, final=final,
                                                  max_delay=40, **settings))
        pos += n_in
    assert np.concatenate(outs, axis=1).tobytes() == want.tobytes()
    _check_haas(dec, want, x, [3, 40, 7, 0], 2, settings)


def test_haas_python_route(dec):
    n, M = 700, 256
    delays = (0, 1, 255, 256, 257, n + 5)
    stages = [dec.HaasEffect(sample_rate_hz=1, delay_time_seconds=float(d), mode='MS', width=0.3) for d in delays]
    pool = np.random.default_rng(2).uniform(-1, 1, (len(delays), n))               # mono, float64
    s = dec.decorrelate_each_stream(stages, in_channels=1, max_frames_per_call=M)
    assert s.tail_frames == n + 5 and s.tail_frames_each.tolist() == list(delays)
    outs = [s.process(pool[:, first:first + M, None]) for first in range(0, n, M)] + [s.flush()]
    got = np.concatenate(outs, axis=1)
    assert got.shape == (len(delays), n + s.tail_frames, 2) and got.dtype == np.float64
    for b, d in enumerate(stages):
        want = d.decorrelate(pool[b])
        assert got[b, :n + s.tail_frames_each[b]].tobytes() == want.tobytes(), b
        assert not got[b, n + s.tail_frames_each[b]:].view(np.int64).any(), b


def test_one_delay_and_a_delay_per_stream_agree_on_every_call(dec, ctx):
    """HaasStream with delay d and HaasEachStream with every delay d run one kernel (haas_stream_kernel<EACH>): call by
    call they return the same float64 bits, on the host and on the device entries, and their concatenation is
    HaasEffect.decorrelate of the whole signal.  The schedule 0, 1, 5, 7, 2, flush puts the first d output frames -
    whose delayed column reads frames below 0 - into the second and third calls, and holds a block of exactly d = 7
    frames and one shorter than d."""
    import torch
    from vndecorrelate_amd.streaming import HaasEachStream, HaasStream
    schedule, S = (0, 1, 5, 7, 2), 3
    n, M = sum(schedule), max(schedule)
    device = torch.device('cuda', ctx.device)
    for d, cx, delayed_channel, ms_mode, width in itertools.product((0, 1, 7), (1, 2), (0, 1), (False, True), (None, 0.3)):
        x = _noise((S, n, cx), 70 + 10 * d + cx)
        stage = dec.HaasEffect(sample_rate_hz=1, delay_time_seconds=float(d), delayed_channel=delayed_channel,
                               mode='MS' if ms_mode else 'LR', width=width)
        want = np.stack([stage.decorrelate(x[b, :, 0] if cx == 1 else x[b]) for b in range(S)])
        assert want.shape == (S, n + d, 2) and want.dtype == np.float64
        kw = dict(in_channels=cx, max_frames_per_call=M, delayed_channel=delayed_channel, ms_mode=ms_mode, width=width)
        for on_device in (False, True):
            where = (d, cx, delayed_channel, ms_mode, width, 'device' if on_device else 'host')
            one, each = HaasStream(num_streams=S, delay=d, **kw), HaasEachStream([d] * S, **kw)
            outs, first = [], 0
            for call, B in enumerate(schedule + (None,)):
                if B is None:
                    a, b, frames = one.flush(), each.flush(), d
                else:
                    block = np.ascontiguousarray(x[:, first:first + B])
                    if on_device:
                        block = torch.from_numpy(block).to(device)
                    a, b, frames = one.process(block), each.process(block), B
                    first += B
                if on_device:
                    a, b = a.cpu().numpy(), b.cpu().numpy()
                assert a.shape == b.shape == (S, frames, 2) and a.dtype == b.dtype == np.float64, (where, call)
                assert a.tobytes() == b.tobytes(), (where, call)
                outs.append(a)
            assert np.concatenate(outs, axis=1).tobytes() == want.tobytes(), where


# ---- 7. the optimisers' results, streamed ----------------------------------------------------------------------------
def test_optimisers_results_streamed(dec):
    from vndecorrelate_amd import optimization as opt
    rng = np.random.default_rng(6)
    n, M = 4000, 480
    base = rng.uniform(-1, 1, (4, n, 1))
    pool = (base * np.array([1.0, 0.6]) + 0.4 * rng.uniform(-1, 1, (4, n, 2))).astype(np.float32)
    kw = dict(sample_rate_hz=FS, duration_seconds=DURATION, num_impulses=IMPULSES, seed=SEED)
    with contextlib.redirect_stdout(io.StringIO()):
        kappas = opt.optimize_velvet_noise_batched(input_signals=pool, grid_size=9, **kw)
        taus = opt.optimize_haas_delay_batched(input_signals=pool, sample_rate_hz=FS, max_delay_seconds=0.01, grid_size=9)
    velvets = [dec.VelvetNoise(log_distribution_strength=float(k), normalizer=None, **kw) for k in kappas]
    haas = [dec.HaasEffect(sample_rate_hz=FS, delay_time_seconds=float(t)) for t in taus]
    dec.set_each_device(True)
    for stages in (velvets, haas):
        want = dec.decorrelate_each(pool, stages)
        assert dec.last_each.route == 'device'
        s = dec.decorrelate_each_stream(stages, max_frames_per_call=M)
        got = np.concatenate([s.process(pool[:, first:first + M]) for first in range(0, n, M)] + [s.flush()], axis=1)
        if isinstance(want, list):
            for b, w in enumerate(want):
                assert got[b, :len(w)].tobytes() == w.tobytes(), b
                assert not got[b, len(w):].view(np.int64).any(), b
        else:
            _same(got, want, 'velvet optimiser')
