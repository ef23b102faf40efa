"""GPU tier of the chunked stream (include/vnd_stream.h) at its C ABI, in every launch plan make_stream_plan can take.

Each case names the plan it must take (vnd_describe_stream_launch, the planner vnd_stream_f32_dev calls) and runs on torch
device buffers through a poisoned harness: the ring state starts as NaN, every call's output buffer starts as a NaN no
arithmetic produces and ends in a sentinel tail of one r = 4 tile.  After each call: *n_out is streaming.output_span's,
every output frame was written, the tail was not.  The concatenated outputs equal the C oracle on the whole signal (input
channel c % in_channels; then encode_side and apply_stereo_width, O.decorrelate's order), bit for bit in the exact and fma
modes; the fast mode is within the one-shot fuzz's bar and bit-identical from run to run of one schedule.  Schedules: the
whole signal in one final call; random ones with 0- and 1-frame calls, calls that only fill the ring, calls of H, H + 1
and max_frames_per_call frames, ending with a flush or with a final block; then a second, shorter signal on the same
state, whose ring still holds the first one's frames.  The Haas stream (include/vnd_haas_stream.h) goes through the same
harness at the end.  The planted-position cases start a stream at a position a long-lived one reaches (2^31 .. 2^60): the
frames below it go into the ring by the header's rule, slot = absolute frame mod capacity, and the rest stays NaN."""
import collections
import ctypes

import numpy as np
import pytest
from hypothesis import given, strategies as st

from oracle import c_oracle
from oracle import vnd_oracle as O
from test_gpu_fuzz_hypothesis import SET, _term_scale
from test_properties_cpu import class_table, sparse_fir
from vndecorrelate_amd.taps import TapArrays, class_path_arrays, function_path_arrays

pytestmark = pytest.mark.gpu

EXACT, FMA, FAST = 0, 1, 2
MODES = (EXACT, FMA, FAST)
POISON = 0x7FA5A5A5          # a signalling NaN: no kernel arithmetic yields it, so it marks frames nobody wrote
SENTINEL = 0x7FB0B0B0        # the tail behind n_out
TAIL = 2048                  # frames of sentinel per call: one tile at r = 4
THREADS = 16                 # C-oracle threads
EPI = (True, 0.35)           # ms_encode plus width, for the stereo cases
MAX_POSITION = 1 << 60       # the largest position a call takes
# 2^31 - 7: the first block crosses 2^31; 2^32 - 300: pos - reach and pos straddle 2^32; None: 2^60 less the frames pushed
PLANTED = (2 ** 31 - 7, 2 ** 32 - 300, 2 ** 40 + 3, None)
PLANTED_IDS = ['2^31-7', '2^32-300', '2^40+3', 'ends-at-2^60']
PLANS = collections.defaultdict(set)      # mode -> every distinct plan the file reached (printed at the end, -s)


@pytest.fixture(scope='module')
def ctx():
    from vndecorrelate_amd import _native
    c = _native.default_context()
    assert 'gfx950' in c.info()['name']
    yield c
    for mode in sorted(PLANS):
        print(f'\nstream plans reached, mode {mode}:')
        for text in sorted(PLANS[mode]):
            print('   ', text)


def _plan(text):
    head, *fields = text.split()
    p = {k: int(v) for k, v in (f.split('=') for f in fields)}
    p['kernel'] = head
    return p


def _record(text):
    PLANS[_plan(text)['mode']].add(' '.join(f for f in text.split() if not f.startswith(('tiles=', 'nblocks='))))


def _latency(arr):
    return int(arr.tap_index.max()) if len(arr.tap_index) else 0


def _table(ctx, arr):
    from vndecorrelate_amd import _native
    return _native.TapTable.create(ctx, arr.tap_offsets, arr.tap_index, arr.tap_weight, **arr.kwargs())


# ---- references on the whole signal ----------------------------------------------------------------------------------
def _oracle(arr, x, cx, mode, epi):
    """(S, n, C): mode EXACT or FMA, x[..., c % cx] through the table, then the pointwise epilogue."""
    C = arr.num_channels
    xf = np.ascontiguousarray(x[..., np.arange(C) % cx])
    fn = c_oracle.convolve_fma if mode == FMA else c_oracle.convolve
    with np.errstate(all='ignore'):
        y = fn(xf, arr.tap_offsets, arr.tap_index, arr.tap_weight, seg_off=arr.seg_offsets, seg_end=arr.seg_end,
               seg_gain=arr.seg_gain, chan_flags=arr.chan_flags, apply_gain=arr.apply_gain, threads=THREADS)
        conv = y.copy()
        ms, width = epi
        if ms or width is not None:
            for b in range(len(y)):
                if ms:
                    O.encode_side(xf[b], y[b])
                if width is not None:
                    O.apply_stereo_width(y[b], width)
    return y, conv, xf


def _compare(got, arr, x, cx, mode, epi, where):
    want, conv, xf = _oracle(arr, x, cx, EXACT if mode == FAST else mode, epi)
    assert got.shape == want.shape, (where, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), where
    assert np.array_equal(np.isinf(got), np.isinf(want)), where
    if mode != FAST:
        assert np.array_equal(got, want, equal_nan=True), (where, _first_diff(got, want))
        return
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), where
    if not fin.any():
        return
    finite_conv = conv[np.isfinite(conv)]
    peak = max(float(np.max(np.abs(want[fin]))), float(np.max(np.abs(finite_conv))) if finite_conv.size else 0.0)
    finite_w = TapArrays(arr.tap_offsets, arr.tap_index, np.nan_to_num(arr.tap_weight, nan=0.0, posinf=0.0, neginf=0.0),
                         **arr.kwargs())
    bar = 1e-6 * peak + 2.0 ** -24 * _term_scale(finite_w, xf) + 1e-30
    err = float(np.max(np.abs(got[fin].astype(np.float64) - want[fin])))
    assert err <= bar, (where, err, bar)


def _first_diff(got, want):
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    return None if not len(bad) else (tuple(bad[0]), len(bad), float(got[tuple(bad[0])]), float(want[tuple(bad[0])]))


# ---- the poisoned harness --------------------------------------------------------------------------------------------
class Poisoned:
    """One pool's state (NaN-filled once, at construction) and the calls of vnd_stream_f32_dev on it."""

    def __init__(self, ctx, table, arr, S, cx, M, mode, epi):
        import torch
        self.torch, self.ctx, self.table, self.arr = torch, ctx, table, arr
        self.S, self.cx, self.M, self.mode = S, cx, M, mode
        self.ms, self.width = epi
        self.C, self.H = arr.num_channels, _latency(arr)
        self.dev = torch.device('cuda', ctx.device)
        need = ctypes.c_int64()
        assert table._lib.vnd_stream_state_bytes(table.handle, S, cx, M, ctypes.byref(need)) == 0
        assert need.value % 4 == 0
        self.state_bytes = need.value
        self.state = torch.full((max(need.value // 4, 1),), float('nan'), dtype=torch.float32, device=self.dev)
        self.plans = []

    def plant(self, position, history):
        """The H frames below `position` of every stream, (S, H, cx), into the ring slots the header names."""
        H, cap = self.H, self.H + self.M
        assert history.shape == (self.S, H, self.cx) and history.dtype == np.float32 and H > 0
        where = np.array([(position - H + j) % cap for j in range(H)], np.int64)         # Python integers: no wrap
        ring = self.state.view(self.S, cap, self.cx)
        ring[:, self.torch.from_numpy(where).to(self.dev)] = self.torch.from_numpy(history).to(self.dev)

    def signal(self, x, calls, start=0):
        """x (S, n, cx); calls [(n_in, final)], the last one final: the concatenation of every call's outputs.  The
        first frame of x is absolute frame `start`."""
        from vndecorrelate_amd.streaming import output_span
        torch = self.torch
        S, C = self.S, self.C
        xd = torch.from_numpy(np.ascontiguousarray(x)).to(self.dev)
        stream = torch.cuda.current_stream(self.dev)
        epi = self.ms or self.width is not None
        outs, pos = [], start
        for i, (n_in, final) in enumerate(calls):
            first, end = output_span(pos, n_in, self.H, final)
            n_out = end - first
            chunk = xd[:, pos - start:pos - start + n_in].contiguous()
            body = S * n_out * C
            y = torch.full((body + TAIL * C,), SENTINEL, dtype=torch.int32, device=self.dev)
            y[:body] = POISON
            if n_out:
                text = self.table.describe_stream(S, n_out, self.cx, self.mode, epi)
                _record(text)
                self.plans.append((n_out, _plan(text)))
            got = ctypes.c_int64(-1)
            rc = self.table._lib.vnd_stream_f32_dev(
                self.ctx.handle, self.table.handle, ctypes.c_void_p(self.state.data_ptr()), self.state_bytes, self.M,
                ctypes.c_void_p(chunk.data_ptr()), ctypes.c_void_p(y.data_ptr()), S, pos, n_in, self.cx, int(final),
                self.mode, int(self.ms), int(self.width is not None), float(self.width or 0.0), ctypes.byref(got),
                ctypes.c_void_p(stream.cuda_stream))
            assert rc == 0, self.table._lib.vnd_last_error()
            assert got.value == n_out, (i, got.value, n_out)
            yh = y.cpu().numpy()
            assert (yh[body:] == SENTINEL).all(), f'call {i} (pos {pos}, n_in {n_in}) wrote past its {n_out} frames'
            hole = np.argwhere((yh[:body] == POISON).reshape(S, n_out, C))
            assert not len(hole), f'call {i} (pos {pos}, n_in {n_in}) left (stream, frame, channel) {tuple(hole[0])} unwritten'
            outs.append(yh[:body].view(np.float32).reshape(S, n_out, C))
            pos += n_in
        assert pos - start == x.shape[1] and calls[-1][1]
        return np.concatenate(outs, axis=1)


def _sizes(n, H, M, rng):
    """Block sizes summing to n, none above M: first calls that only fill the ring (pos + n_in <= H), then 0, 1, H, H + 1,
    M and random sizes in a shuffled order."""
    out, pos = [], 0
    for b in (1, 0, (H - 1) // 2, H):                            # the last one fills the ring up to H
        b = max(0, min(b, n - pos, M, H - pos))
        out.append(b)
        pos += b
    menu = [0, 1, H, H + 1, M, 17]
    order = [menu[i] for i in rng.permutation(len(menu))]       # every size of the menu first, then any
    while pos < n:
        b = min(order.pop() if order else int(rng.choice(menu + [int(rng.integers(1, M + 1))])), n - pos, M)
        out.append(b)
        pos += b
    return out


def _calls(sizes, ending):
    if ending == 'flush':
        return [(b, False) for b in sizes] + [(0, True)]
    return [(b, False) for b in sizes[:-1]] + [(sizes[-1], True)]


def _signal(S, n, cx, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (S, n, cx)).astype(np.float32)


def _stream_case(ctx, arr, S, cx, n, M, mode, epi, seed, check_plan=None):
    """Every schedule of the file on one table, pool and mode; returns the (n_out, plan) of every frame-computing call."""
    table = _table(ctx, arr)
    H = _latency(arr)
    plans = []
    try:
        x = _signal(S, n, cx, seed)
        # the whole signal in one final call
        p = Poisoned(ctx, table, arr, S, cx, max(n, 1), mode, epi)
        got = p.signal(x, [(n, True)])
        _compare(got, arr, x, cx, mode, epi, 'whole')
        plans += p.plans
        rng = np.random.default_rng(seed + 1)
        sizes = _sizes(n, H, M, rng)
        for ending in ('flush', 'final'):
            p = Poisoned(ctx, table, arr, S, cx, M, mode, epi)
            got = p.signal(x, _calls(sizes, ending))
            _compare(got, arr, x, cx, mode, epi, ending)
            if mode == FAST and ending == 'flush':         # the same schedule again: the same bits
                again = Poisoned(ctx, table, arr, S, cx, M, mode, epi).signal(x, _calls(sizes, ending))
                assert np.array_equal(got.view(np.int32), again.view(np.int32)), 'fast mode not repeatable'
            if ending == 'final':                          # a second, shorter signal on the same state
                n2 = n // 2 + 1
                x2 = _signal(S, n2, cx, seed + 2)
                got2 = p.signal(x2, _calls(_sizes(n2, H, M, rng), 'flush'))
                _compare(got2, arr, x2, cx, mode, epi, 'second signal')
            plans += p.plans
    finally:
        table.close()
    for n_out, plan in plans:
        if check_plan is not None:
            check_plan(plan, n_out)
    return plans


# ---- tables ----------------------------------------------------------------------------------------------------------
def _csr(per_channel, seed=0):
    """per_channel: a list of index lists; weights irregular (the modes differ), none zero unless given."""
    rng = np.random.default_rng(seed)
    offs = np.zeros(len(per_channel) + 1, np.int32)
    idx, w = [], []
    for c, ch in enumerate(per_channel):
        idx += list(ch)
        w += list(rng.choice([-1, 1], len(ch)) * rng.uniform(0.05, 0.95, len(ch)))
        offs[c + 1] = len(idx)
    return TapArrays(offs, np.asarray(idx, np.int32), np.asarray(w, np.float32))


def _random_table(C, H, k, seed):
    """C channels of k taps in [0, H] (ascending), H reached by channel 0."""
    rng = np.random.default_rng(seed)
    chans = []
    for c in range(C):
        pick = rng.choice(np.arange(1, H), size=min(k, max(H - 1, 0)), replace=False) if H > 1 else np.array([], int)
        pick = np.sort(np.concatenate([[0] if c % 2 else [], pick, [H] if c == 0 else []]).astype(int))
        chans.append(sorted(set(pick.tolist())))
    return _csr(chans, seed)


def _class_table(seed):
    """VelvetNoise's class path: segments with gains, a pass-through channel, duplicate indices across segments."""
    rng = np.random.default_rng(seed)
    env = (1.0, 0.85, 0.5, 0.25)
    segs = [(sorted(rng.integers(0, 1400, 4).tolist()), sorted(rng.integers(0, 1439, 3).tolist())) for _ in env]
    segs[1][0].append(segs[0][0][0])
    return class_path_arrays([segs, None], env, True)


def _with_weights(arr, repl):
    w = arr.tap_weight.copy()
    for k, v in repl.items():
        w[k] = v
    return TapArrays(arr.tap_offsets, arr.tap_index, w)


def _probe_table(ctx, C, H):
    return _table(ctx, _csr([[0, H]] * C))


_BAND = {}


def _band_index(ctx, mode, cx=2):
    """The smallest max_index at which a stereo table's stream leaves its first plan, found through the hook: cg = 2 for
    a stereo input, the broadcast plane for a mono one."""
    if (mode, cx) in _BAND:
        return _BAND[mode, cx]

    def keeps(H):
        t = _probe_table(ctx, 2, H)
        try:
            p = _plan(t.describe_stream(1, 8192, cx, mode))
        finally:
            t.close()
        return not p['direct'] and (p['bc'] == 1 if cx == 1 else p['cg'] == 2)
    lo, hi = 64, 1 << 17
    assert keeps(lo) and not keeps(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if keeps(mid) else (lo, mid)
    _BAND[mode, cx] = hi
    return hi


def _calls_for_r(ctx, arr, S, cx, mode, epi, r):
    """The shortest call (a multiple of 1024 frames) whose plan takes r frame pairs per lane, found through the hook."""
    t = _table(ctx, arr)
    try:
        for k in range(1, 257):
            if _plan(t.describe_stream(S, 1024 * k, cx, mode, epi[0] or epi[1] is not None))['r'] == r:
                return 1024 * k
    finally:
        t.close()
    raise AssertionError(f'no call length up to 256 Ki frames takes r = {r}')


# ---- 1-6: the plan matrix --------------------------------------------------------------------------------------------
def _every(**want):
    def check(plan, n_out):
        assert all(plan[k] == v for k, v in want.items()), (want, n_out, plan)
    return check


NO_EPI = (False, None)
STEREO = [NO_EPI, EPI]
T30 = 1439                   # a 30 ms table at 48 kHz


def _matrix():
    cases = []

    def case(name, make, S, cx, n, M, want, epis=(NO_EPI,), reach_r=None):
        for e in epis:
            tag = '-'.join(t for t in ('ms' if e[0] else '', '' if e[1] is None else f'w{e[1]}') if t) or 'plain'
            for mode in MODES:
                cases.append(pytest.param(make, S, cx, n, M, mode, e, want, reach_r, id=f'{name}-{tag}-m{mode}'))

    st30 = lambda ctx, mode: _random_table(2, T30, 30, 1)
    case('r1-stereo', st30, 3, 2, 9001, 2500, dict(direct=0, cg=2, bc=0, r=1), STEREO)
    case('r2-stereo-pool64', st30, 64, 2, None, None, dict(direct=0, cg=2, bc=0), STEREO, reach_r=2)
    case('r4-stereo-pool64', st30, 64, 2, None, None, dict(direct=0, cg=2, bc=0), STEREO, reach_r=4)
    case('r4-mono-fanout-pool64', st30, 64, 1, None, None, dict(direct=0, cg=2, bc=1), reach_r=4)
    case('cg1-mono', lambda ctx, mode: _random_table(1, 700, 20, 2), 2, 1, 6001, 1500, dict(direct=0, cg=1, bc=0, r=1))
    case('cg1-C3', lambda ctx, mode: _random_table(3, 900, 25, 3), 2, 3, 6001, 1500, dict(direct=0, cg=1, bc=0, r=1))
    case('cg1-C3-from-mono', lambda ctx, mode: _random_table(3, 900, 25, 3), 2, 1, 6001, 1500, dict(direct=0, cg=1, bc=0))
    case('cg1-C6-from-Cx3', lambda ctx, mode: _random_table(6, 600, 12, 4), 2, 3, 5001, 1200, dict(direct=0, cg=1, bc=0))
    case('bc-C2-from-mono', st30, 3, 1, 9001, 2500, dict(direct=0, cg=2, bc=1), STEREO)
    case('bc-C4-from-mono', lambda ctx, mode: _random_table(4, 800, 16, 5), 2, 1, 6001, 1700, dict(direct=0, cg=2, bc=1))
    case('cg2-C4-from-Cx2', lambda ctx, mode: _random_table(4, 800, 16, 6), 2, 2, 6001, 1700, dict(direct=0, cg=2, bc=0))
    case('cg2-C8-from-Cx2', lambda ctx, mode: _random_table(8, 500, 10, 7), 2, 2, 4001, 1100, dict(direct=0, cg=2, bc=0))
    case('cg2-C8-from-Cx4', lambda ctx, mode: _random_table(8, 500, 10, 8), 2, 4, 4001, 1100, dict(direct=0, cg=2, bc=0))
    band = lambda ctx, mode: _random_table(2, _band_index(ctx, EXACT) + 64, 40, 9)
    case('band-stereo', band, 2, 2, 90001, None, dict(direct=0, cg=1, bc=0))
    case('band-stereo', band, 2, 2, 90001, None, dict(direct=1), (EPI, (False, 0.6), (True, None)))
    # one plane still holds a mono input's window in the stereo band: the broadcast plane goes further, to where one plane
    # stops fitting; there the fast mode (whose exchange buffer shrinks with cg) takes cg = 1, the others go direct
    case('band-mono-fanout', lambda ctx, mode: _random_table(2, _band_index(ctx, mode, 1), 40, 9), 2, 1, 180001, None,
         lambda mode: dict(bc=0, direct=int(mode != FAST)))
    case('direct-halo', lambda ctx, mode: _random_table(2, 48000, 40, 10), 2, 2, 180001, None, dict(direct=1), STEREO)
    case('direct-nonfinite', lambda ctx, mode: _with_weights(_csr([[1, 3, 5, 9, 40, 44], [0, 2, 17, 30, 33]], 11),
                                                       {2: np.inf, 8: np.nan}), 2, 2, 3001, 500, dict(direct=1))
    case('direct-huge-index', lambda ctx, mode: _csr([[3, (1 << 24) + 3], [0, 7]], 12), 2, 2, 3001, 1024, dict(direct=1))
    case('edge-H0', lambda ctx, mode: _csr([[0, 0], [0]], 13), 2, 2, 3001, 700, dict(direct=0))
    case('edge-empty-channel-dups-zeros', lambda ctx, mode: _with_weights(_csr([[0, 5, 5, 37, 300], [], [2, 2, 2]], 14),
                                                                    {1: 0.0, 5: -0.0}), 2, 3, 3001, 700, dict(direct=0))
    case('edge-shorter-than-H', lambda ctx, mode: _random_table(2, 5000, 20, 15), 2, 2, 3001, 5001, dict(direct=0), STEREO)
    case('class-path', lambda ctx, mode: _class_table(16), 2, 2, 7001, 2000, dict(direct=0, cg=2), STEREO)
    case('class-path-from-mono', lambda ctx, mode: _class_table(17), 2, 1, 7001, 2000, dict(direct=0, bc=1), STEREO)
    return cases


@pytest.mark.parametrize('make, S, cx, n, M, mode, epi, want, reach_r', _matrix())
def test_stream_plan_matrix(ctx, make, S, cx, n, M, mode, epi, want, reach_r):
    arr = make(ctx, mode)
    H = _latency(arr)
    if reach_r is not None:                      # the pool's calls of M frames take r = reach_r (M found by the hook)
        M = _calls_for_r(ctx, arr, S, cx, mode, epi, reach_r)
        n = 2 * M + 2 * H + 3001
    M = M or H + 4096
    plans = _stream_case(ctx, arr, S, cx, n, M, mode, epi, 11 + mode, _every(**(want(mode) if callable(want) else want)))
    assert plans, 'no call computed frames'
    if reach_r is not None:
        assert any(p['r'] == reach_r and n_out == M for n_out, p in plans), (reach_r, M, sorted({p['r'] for _, p in plans}))
    if H == 0:
        assert all(p['W'] == 2 * 256 * p['r'] + 16 for _, p in plans)


# ---- a stream that has been running for a day -------------------------------------------------------------------------
@pytest.mark.parametrize('position', PLANTED, ids=PLANTED_IDS)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('kernel', ['conv_stream', 'conv_stream_direct'])
def test_planted_position(ctx, kernel, mode, position):
    """The tap sum reads x[n .. n + H]: with the H frames below P in the ring, the outputs from frame P - H on are the
    oracle's on the signal that starts there, whole - bit for bit in the exact and fma modes; the fast mode's even / odd
    chains follow E = P - H, so it is held to the file's bar for that mode."""
    H, M, n = (T30, 700, 2900) if kernel == 'conv_stream' else (48000, 3000, 7000)
    arr = _random_table(2, H, 30, 21)
    S, cx = 2, 2
    start = MAX_POSITION - n if position is None else position
    table = _table(ctx, arr)
    try:
        sig = _signal(S, H + n, cx, 500 + mode + start % 101)
        sizes = _sizes(n, H, M, np.random.default_rng(start % 1021))
        p = Poisoned(ctx, table, arr, S, cx, M, mode, EPI)
        p.plant(start, sig[:, :H])
        got = p.signal(sig[:, H:], _calls(sizes, 'flush' if position is None else 'final'), start=start)
        assert p.plans and all(plan['kernel'] == kernel for _, plan in p.plans), p.plans
        _compare(got, arr, sig, cx, mode, EPI, ('planted at', start))
    finally:
        table.close()


def test_band_is_where_the_issue_puts_it(ctx):
    """The fallback band starts where one stereo plane pair stops fitting: about 19.8 k frames with 160 KiB of LDS."""
    lo = _band_index(ctx, EXACT)
    assert 15000 < lo < 40000, lo
    t = _probe_table(ctx, 2, lo - 1)
    try:
        assert _plan(t.describe_stream(1, 8192, 2, EXACT))['cg'] == 2
    finally:
        t.close()
    for H, want in ((lo + 64, dict(direct=0, cg=1)), (48000, dict(direct=1))):
        t = _probe_table(ctx, 2, H)
        try:
            for mode in MODES:
                _every(**want)(_plan(t.describe_stream(1, 8192, 2, mode)), 8192)
                assert _plan(t.describe_stream(1, 8192, 2, mode, True))['direct'] == (1 if H > lo else 0)
        finally:
            t.close()


def test_describe_stream_refuses_bad_shapes(ctx):
    from vndecorrelate_amd import _native
    t = _table(ctx, _random_table(4, 300, 5, 1))
    try:
        with pytest.raises(ValueError):
            t.describe_stream(1, 100, 3, EXACT)          # 3 input channels into 4
        with pytest.raises(ValueError):
            t.describe_stream(1, 100, 4, EXACT, True)    # the epilogue needs 2 output channels
        with pytest.raises(ValueError):
            t.describe_stream(1, 100, 4, 7)
        with pytest.raises(ValueError):
            t.describe_stream(_native.MAX_STREAMS_PER_CALL + 1, 100, 4, EXACT)
    finally:
        t.close()


# ---- property test ---------------------------------------------------------------------------------------------------
@st.composite
def _stream_draw(draw):
    if draw(st.booleans()):
        arr = function_path_arrays(draw(sparse_fir()))
    else:
        chans, env = draw(class_table())
        arr = class_path_arrays(chans, env, env != (1.0,))
    C = arr.num_channels
    cx = draw(st.sampled_from([d for d in range(1, C + 1) if C % d == 0]))
    H = _latency(arr)
    S = draw(st.integers(1, 3))
    n = draw(st.integers(1, 5000))
    M = draw(st.integers(1, 2 * H + 600))
    epi = draw(st.sampled_from([NO_EPI, (True, None), (False, 0.25), EPI])) if C == 2 else NO_EPI
    return arr, S, cx, n, M, epi, draw(st.sampled_from(['flush', 'final'])), draw(st.integers(0, 2**31 - 1))


@SET
@given(case=_stream_draw(), mode=st.sampled_from(MODES))
def test_random_tables_and_schedules(ctx, case, mode):
    arr, S, cx, n, M, epi, ending, seed = case
    H = _latency(arr)
    table = _table(ctx, arr)
    try:
        rng = np.random.default_rng(seed)
        x = _signal(S, n, cx, seed)
        p = Poisoned(ctx, table, arr, S, cx, M, mode, epi)
        _compare(p.signal(x, _calls(_sizes(n, H, M, rng), ending)), arr, x, cx, mode, epi, ending)
        n2 = int(rng.integers(1, n + 1))
        x2 = _signal(S, n2, cx, seed + 1)
        _compare(p.signal(x2, _calls(_sizes(n2, H, M, rng), 'flush')), arr, x2, cx, mode, epi, 'second signal')
    finally:
        table.close()


# ---- 7. the Haas stream: the same poisoned ring and sentinel -------------------------------------------------------------
POISON64 = 0x7FF4A5A5A5A5A5A5
SENTINEL64 = 0x7FF5B0B0B0B0B0B0
FS = 48000


def _haas_signal(ctx, state, state_bytes, M, x, calls, d, dc, ms, width, start=0):
    import torch
    from vndecorrelate_amd import _native
    from vndecorrelate_amd.streaming import haas_output_span
    lib = _native.load_library()
    dev = torch.device('cuda', ctx.device)
    S, n, cx = x.shape
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    stream = torch.cuda.current_stream(dev)
    outs, pos = [], start
    for i, (n_in, final) in enumerate(calls):
        first, end = haas_output_span(pos, n_in, d, final)
        n_out = end - first
        chunk = xd[:, pos - start:pos - start + n_in].contiguous()
        body = S * n_out * 2
        y = torch.full((body + TAIL * 2,), SENTINEL64, dtype=torch.int64, device=dev)
        y[:body] = POISON64
        got = ctypes.c_int64(-1)
        rc = lib.vnd_haas_stream_f64_dev(ctx.handle, ctypes.c_void_p(state.data_ptr() if state is not None else 0),
                                         state_bytes, M, ctypes.c_void_p(chunk.data_ptr()), ctypes.c_void_p(y.data_ptr()),
                                         S, pos, n_in, cx, int(final), d, dc, int(ms), int(width is not None),
                                         float(width or 0.0), ctypes.byref(got), ctypes.c_void_p(stream.cuda_stream))
        assert rc == 0, lib.vnd_last_error()
        assert got.value == n_out, (i, got.value, n_out)
        yh = y.cpu().numpy()
        assert (yh[body:] == SENTINEL64).all(), f'call {i} (pos {pos}) wrote past its {n_out} frames'
        assert not (yh[:body] == POISON64).any(), f'call {i} (pos {pos}) left frames unwritten'
        outs.append(yh[:body].view(np.float64).reshape(S, n_out, 2))
        pos += n_in
    assert pos - start == n and calls[-1][1]
    return np.concatenate(outs, axis=1)


@pytest.mark.parametrize('cx', [1, 2])
@pytest.mark.parametrize('d, dc, mode, width', [(1, 0, 'LR', None), (100, 1, 'MS', None), (479, 0, 'LR', 0.3),
                                                 (480, 1, 'MS', 0.6), (481, 0, 'MS', None), (1700, 1, 'LR', 0.8)])
def test_haas_stream_poisoned(ctx, cx, d, dc, mode, width):
    """Blocks of up to M = 480 frames, delays below, at and above it; the first call at position 0, a reset, a second signal."""
    import torch
    from vndecorrelate_amd import _native
    M, S = 480, 3
    need = ctypes.c_int64()
    assert _native.load_library().vnd_haas_stream_state_bytes(S, cx, d, M, ctypes.byref(need)) == 0
    dev = torch.device('cuda', ctx.device)
    state = torch.full((max(need.value // 4, 1),), float('nan'), dtype=torch.float32, device=dev)
    rng = np.random.default_rng(d * 7 + cx)
    ms = mode == 'MS'

    def want(x):
        out = []
        for b in range(S):
            xb = x[b, :, 0] if cx == 1 else x[b]
            out.append(O.haas_effect(xb, sample_rate_hz=FS, delay_time_seconds=d / FS, delayed_channel=dc, mode=mode,
                                     width=width))
        return np.stack(out)

    for n, ending in ((5000, 'final'), (2500, 'flush'), (d // 2 + 1, 'final')):     # one state: each signal after a reset
        x = rng.uniform(-1, 1, (S, n, cx)).astype(np.float32)
        sizes = [int(b) for b in _sizes(n, d, M, rng)]
        got = _haas_signal(ctx, state, need.value, M, x, _calls(sizes, ending), d, dc, ms, width)
        assert got.shape == (S, n + d, 2)
        assert np.array_equal(got, want(x)), (n, ending, _first_diff(got, want(x)))


@pytest.mark.parametrize('position', PLANTED, ids=PLANTED_IDS)
def test_haas_stream_planted_position(ctx, position):
    """A delay reads x[f - d]: with the d frames below P in the ring (slot = absolute frame mod (d + M)), the outputs
    from P on are the reference's on the signal that starts at P - d, from its frame d on."""
    import torch
    from vndecorrelate_amd import _native
    M, S, cx, d, dc, mode, width = 480, 3, 2, 481, 1, 'MS', 0.6
    n = 1500
    start = MAX_POSITION - n if position is None else position
    lib = _native.load_library()
    need = ctypes.c_int64()
    assert lib.vnd_haas_stream_state_bytes(S, cx, d, M, ctypes.byref(need)) == 0 and need.value == S * (d + M) * cx * 4
    dev = torch.device('cuda', ctx.device)
    state = torch.full((need.value // 4,), float('nan'), dtype=torch.float32, device=dev)
    sig = _signal(S, d + n, cx, 700 + start % 103)
    where = np.array([(start - d + j) % (d + M) for j in range(d)], np.int64)
    state.view(S, d + M, cx)[:, torch.from_numpy(where).to(dev)] = torch.from_numpy(sig[:, :d]).to(dev)
    sizes = [int(b) for b in _sizes(n, d, M, np.random.default_rng(start % 1031))]
    got = _haas_signal(ctx, state, need.value, M, sig[:, d:], _calls(sizes, 'flush' if position is None else 'final'),
                       d, dc, True, width, start=start)
    want = np.stack([O.haas_effect(sig[b], sample_rate_hz=FS, delay_time_seconds=d / FS, delayed_channel=dc, mode=mode,
                                   width=width) for b in range(S)])
    assert want.shape == (S, d + n + d, 2) and got.shape == (S, n + d, 2)
    assert np.array_equal(got, want[:, d:]), _first_diff(got, want[:, d:])
    # one frame further the position is out of range: refused, nothing written
    before = state.clone()
    y = torch.full((S, M, 2), 7.0, dtype=torch.float64, device=dev)
    chunk = torch.zeros((S, M, cx), dtype=torch.float32, device=dev)
    rows = ctypes.c_int64(-1)
    rc = lib.vnd_haas_stream_f64_dev(ctx.handle, ctypes.c_void_p(state.data_ptr()), need.value, M, ctypes.c_void_p(chunk.data_ptr()),
                                     ctypes.c_void_p(y.data_ptr()), S, MAX_POSITION + 1, M, cx, 0, d, dc, 1, 1, width,
                                     ctypes.byref(rows), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 1 and b'position' in lib.vnd_last_error() and rows.value == 0
    torch.cuda.synchronize(dev)
    assert bool((y == 7.0).all()) and state.view(torch.int32).equal(before.view(torch.int32))
