"""GPU tier of the spectrum voice pool (vnd_spectrum_voice_stream_f32_dev / _f64_dev, include/vnd_spectrum_voice_stream.h;
spectral.SpectrumVoicePool).  Every comparison is of the bits, against the one-shot device calls: vnd_spectrogram_*_dev on
each voice's whole signal for the columns, vnd_cross_spectra_*_dev on the frames pushed so far for the means after every call.

The harness drives the C ABI on poisoned memory: the ring, the sums and the work are NaN, the positions are NaN bytes until
the reset, the chunk rows past counts[b] are NaN, every output holds a signalling NaN no arithmetic yields, with a sentinel
tail.  After every call out_counts, segments and the device's positions equal the mirror (spectral.spectrum_voice_spans),
every row below out_counts[b] is written and every value at or past it is untouched, and the means of a bad or idle slot
are what they were."""
import ctypes

import numpy as np
import pytest

import spectrum_voice_cases as sv
from spectrum_voice_cases import END, INVALID, START, UNSUPPORTED

pytestmark = pytest.mark.gpu

POISON32, POISON64 = 0x7FA5A5A5, 0x7FF4A5A5A5A5A5A5      # signalling NaNs: no kernel arithmetic yields them
TAIL = 64


@pytest.fixture(scope='module')
def ctx():
    from vndecorrelate_amd import _native
    context = _native.default_context()
    assert 'gfx950' in context.info()['name']
    return context


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def noise(n, seed, amplitude=1.0, dtype=np.float32):
    """(n, 2): a partly coherent pair, so that the mean cross spectrum does not cancel."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, n)
    y = 0.6 * x + 0.4 * rng.standard_normal(n)
    if dtype == np.float64:                                   # values between float32 ones
        x, y = x * (1 + 1e-9), y * (1 - 1e-9)
    return (np.stack([x, y], axis=1) * amplitude).astype(dtype)


class Harness:
    """One pool at the C ABI on poisoned memory.  layout: 'stereo' - both channels of one (S, M, 2) block; 'mono' - an
    (S, M, 1) block; 'strided' - channel 1 of an (S, M, 2) block as a mono view (frame_stride 2)."""

    def __init__(self, torch, ctx, S, M, W, H, nfft, dtype=np.float32, layout='stereo', detrend=True, reset=True, columns=True,
                 means=True):
        from scipy.signal import get_window
        from vndecorrelate_amd import _native, spectral
        self.torch, self.ctx, self.native = torch, ctx, _native
        self.dev = torch.device('cuda', ctx.device)
        self.S, self.M, self.W, self.H, self.nfft = S, M, W, H, nfft
        self.dtype, self.layout, self.detrend = np.dtype(dtype), layout, detrend
        self.f64 = self.dtype == np.float64
        self.C = 2 if layout == 'stereo' else 1
        self.width = 1 if layout == 'mono' else 2                # channels of the chunk block
        self.pick = slice(None) if layout == 'stereo' else slice(0, 1) if layout == 'mono' else slice(1, 2)
        self.R = _native.spectrum_run_length(nfft, W, H, self.f64, self.C)
        self.lay = sv.layout(S, self.C, W, H, nfft, M, self.dtype.itemsize, self.R)
        self.F, self.Q, self.rc, self.cap, self.need = (self.lay[k] for k in ('F', 'Q', 'rc', 'cap', 'need'))
        assert self.need == _native.spectrum_voice_stream_state_bytes(S, self.C, W, H, nfft, M, self.f64)
        win64 = np.asarray(get_window('hann', W), np.float64)
        self.scale = spectral.spectrum_scale(win64, 1.0, 'density')
        self.win = torch.from_numpy(win64.astype(self.dtype)).to(self.dev)
        self.tw = torch.from_numpy(spectral.twiddle_table(nfft, self.dtype)).to(self.dev)
        self.tdt = torch.float64 if self.f64 else torch.float32
        self.idt = torch.int64 if self.f64 else torch.int32
        self.poison = POISON64 if self.f64 else POISON32
        self.state = torch.full((self.need // 4,), float('nan'), dtype=torch.float32, device=self.dev)
        self.chunk = torch.empty((S, M, self.width), dtype=self.tdt, device=self.dev)
        self.counts, self.flags, self.oc = (torch.empty(S, dtype=torch.int32, device=self.dev) for _ in range(3))
        F, C = self.F, self.C
        self.cols = torch.empty((S * self.rc * C * F + TAIL,), dtype=self.idt, device=self.dev) if columns else None
        self.has_means = means
        self.pxx, self.pyy, self.pxy = (torch.full((S * F * k + TAIL,), self.poison, dtype=self.idt, device=self.dev) for k in (1, 1, 2))
        self.segments = torch.full((S + TAIL,), -77, dtype=torch.int64, device=self.dev)
        self.mirror = None                                   # the positions, once they are known
        if reset:
            self.reset()

    def stream(self):
        return self.torch.cuda.current_stream(self.dev).cuda_stream

    def reset(self):
        self.native.spectrum_voice_stream_reset_device(self.ctx, self.state.data_ptr(), self.need, self.S, self.C, self.W, self.H,
                                                       self.nfft, self.M, self.f64, stream=self.stream())
        self.mirror = np.zeros(self.S, np.int64)

    def positions(self):
        return self.state[:2 * self.S].view(self.torch.int64).cpu().numpy().copy()

    def part(self, name):
        """'sums' (S, F, Q, 2), 'work' or 'ring' (S, cap, C) of the state as a torch view."""
        lay, t = self.lay, self.torch
        if name == 'sums':
            return self.state[lay['sums_at'] // 4:lay['work_at'] // 4].view(t.float64).view(self.S, self.F, self.Q, 2)
        if name == 'work':
            return self.state[lay['work_at'] // 4:lay['ring_at'] // 4].view(t.int32)
        count = self.S * self.cap * self.C
        return self.state[lay['ring_at'] // 4:].view(self.tdt)[:count].view(self.S, self.cap, self.C)

    def plant(self, b, position, history, total=None, partial=None):
        """Slot b at `position`, the frames [position - len(history), position) in their ring slots, and its sums."""
        torch = self.torch
        self.state[:2 * self.S].view(torch.int64)[b] = position
        if len(history):
            where = np.array([(position - len(history) + j) % self.cap for j in range(len(history))], np.int64)    # Python ints
            self.part('ring')[b, torch.from_numpy(where).to(self.dev)] = torch.from_numpy(np.asarray(history, self.dtype)).to(self.dev)
        if total is not None:
            self.part('sums')[b, :, :, 0] = torch.from_numpy(np.asarray(total, np.float64)).to(self.dev)
            self.part('sums')[b, :, :, 1] = torch.from_numpy(np.asarray(partial, np.float64)).to(self.dev)
        self.mirror[b] = position

    def args(self):
        e = self.chunk.element_size()
        stereo = self.C == 2
        return dict(ctx=self.ctx.handle, state=self.state.data_ptr(), state_bytes=self.need, M=self.M,
                    x=self.chunk.data_ptr() + (e if self.layout == 'strided' else 0), ss=self.M * self.width, fs=self.width, C=self.C,
                    counts=self.counts.data_ptr(), flags=self.flags.data_ptr(), win=self.win.data_ptr(), tw=self.tw.data_ptr(),
                    W=self.W, H=self.H, nfft=self.nfft, detrend=int(self.detrend), scale=self.scale,
                    cols=self.cols.data_ptr() if self.cols is not None else 0, oc=self.oc.data_ptr(),
                    pxx=self.pxx.data_ptr() if self.has_means else 0, pyy=self.pyy.data_ptr() if self.has_means and stereo else 0,
                    pxy=self.pxy.data_ptr() if self.has_means and stereo else 0,
                    segments=self.segments.data_ptr() if self.has_means else 0, S=self.S, stream=self.stream())

    def raw(self, **kw):
        """The C call with pointers and scalars replaced by name; returns the status."""
        return sv.raw_call(self.ctx._lib, self.f64, dict(self.args(), **kw))

    def upload(self, blocks, counts, flags):
        torch = self.torch
        host = np.full((self.S, self.M, self.width), np.nan, self.dtype)
        for b, block in enumerate(blocks):
            if block is not None and len(block):
                host[b, :len(block), -self.C:] = np.asarray(block)[:, self.pick]
        self.chunk.copy_(torch.from_numpy(host))
        self.counts.copy_(torch.from_numpy(np.asarray(counts, np.int32)))
        self.flags.copy_(torch.from_numpy(np.asarray(flags, np.int32)))
        if self.cols is not None:
            self.cols.fill_(self.poison)
        self.oc.fill_(-77)

    def means_host(self):
        return [t.cpu().numpy() for t in (self.pxx, self.pyy, self.pxy, self.segments)]

    def call(self, blocks, counts, flags):
        """One call; checks the counts, the segments, the positions and the written / untouched split; returns, per slot,
        the columns (n, C, F) and the means (segments, pxx, pyy, pxy - None for a slot whose means the call left alone)."""
        from vndecorrelate_amd.spectral import spectrum_voice_spans
        S, F, C, rc = self.S, self.F, self.C, self.rc
        self.upload(blocks, counts, flags)
        before = self.means_host()
        assert self.raw() == 0, self.ctx._lib.vnd_last_error()
        self.torch.cuda.synchronize(self.dev)
        want, segs, new = spectrum_voice_spans(self.mirror, counts, flags, self.W, self.H, self.M)
        assert self.oc.cpu().numpy().tolist() == want.tolist(), (counts, flags, self.mirror)
        assert (want <= rc).all()
        assert self.positions().tolist() == new.tolist()
        self.mirror = new
        rows = [np.zeros((0, C, F), self.dtype) for _ in want]
        if self.cols is not None:
            out = self.cols.cpu().numpy()
            assert (out[S * rc * C * F:] == self.poison).all()
            body = out[:S * rc * C * F].reshape(S, rc, C, F)
            for b, n in enumerate(want):
                n = max(int(n), 0)
                assert not (body[b, :n] == self.poison).any() and (body[b, n:] == self.poison).all(), (b, n)
                rows[b] = body[b, :n].view(self.dtype).copy()
        means = [None] * S
        if self.has_means:
            after = self.means_host()
            for k, name in enumerate(('pxx', 'pyy', 'pxy')):
                width = F * (2 if name == 'pxy' else 1)
                assert (after[k][S * width:] == self.poison).all(), name
                touched = C == 2 or name == 'pxx'
                a, z = after[k][:S * width].reshape(S, width), before[k][:S * width].reshape(S, width)
                for b in range(S):
                    if segs[b] < 0 or not touched:
                        assert np.array_equal(a[b], z[b]), (name, b)
                    else:
                        assert not (a[b] == self.poison).any(), (name, b)
            assert (after[3][S:] == -77).all()
            for b in range(S):
                assert after[3][b] == (before[3][b] if segs[b] < 0 else segs[b]), b
                if segs[b] >= 0:
                    view = lambda k, shape: after[k][:S * F * (2 if k == 2 else 1)].view(self.dtype).reshape((S,) + shape)[b].copy()
                    means[b] = (int(segs[b]), view(0, (F,)), view(1, (F,)) if C == 2 else None, view(2, (F, 2)) if C == 2 else None)
        return rows, means


# ---- the one-shot references -------------------------------------------------------------------------------------------
def _pool_of(h, signals):
    """(B, n, C) of the harness's dtype and channels, zero padded, n >= W, and the int32 lengths."""
    n = max([h.W] + [len(x) for x in signals])
    pool = np.zeros((len(signals), n, h.C), h.dtype)
    for i, x in enumerate(signals):
        pool[i, :len(x)] = np.asarray(x)[:, h.pick]
    return pool, np.array([len(x) for x in signals], np.int32)


def one_shot_columns(h, signals):
    """vnd_spectrogram_*_dev on every signal ((n, 2) arrays, the harness's channels taken): a list of (T, C, F)."""
    torch = h.torch
    pool, each = _pool_of(h, signals)
    B, n, C = pool.shape
    T = (n - h.W) // h.H + 1
    x, e = torch.from_numpy(pool).to(h.dev), torch.from_numpy(each).to(h.dev)
    sxx = torch.empty((B, C, h.F, T), dtype=h.tdt, device=h.dev)
    h.native.spectrogram_device(h.ctx, x.data_ptr(), B, n, n * C, C, C, h.win.data_ptr(), h.tw.data_ptr(), h.W, h.H, h.nfft,
                                sxx.data_ptr(), detrend=h.detrend, scale=h.scale, n_each_ptr=e.data_ptr(), float64=h.f64,
                                stream=h.stream())
    got = sxx.cpu().numpy()
    return [np.ascontiguousarray(got[i, :, :, :sv.complete(int(m), h.W, h.H)].transpose(2, 0, 1)) for i, m in enumerate(each)]


def one_shot_means(h, signals):
    """vnd_cross_spectra_*_dev on every signal: a list of (segments, pxx, pyy, pxy)."""
    torch = h.torch
    pool, each = _pool_of(h, signals)
    B, n, C = pool.shape
    x, e = torch.from_numpy(pool).to(h.dev), torch.from_numpy(each).to(h.dev)
    pxx, pyy = (torch.full((B, h.F), float('nan'), dtype=h.tdt, device=h.dev) for _ in range(2))
    pxy = torch.full((B, h.F, 2), float('nan'), dtype=h.tdt, device=h.dev)
    wb = h.native.cross_spectra_work_bytes(B, n, C, h.W, h.H, h.nfft, h.f64)
    work = torch.full((max(1, wb // 8),), float('nan'), dtype=torch.float64, device=h.dev)
    h.native.cross_spectra_device(h.ctx, x.data_ptr(), B, n, n * C, C, C, h.win.data_ptr(), h.tw.data_ptr(), h.W, h.H, h.nfft,
                                  pxx.data_ptr(), pyy.data_ptr() if C == 2 else 0, pxy.data_ptr() if C == 2 else 0,
                                  work_ptr=work.data_ptr(), work_bytes=wb, detrend=h.detrend, scale=h.scale, n_each_ptr=e.data_ptr(),
                                  float64=h.f64, stream=h.stream())
    a, b, c = pxx.cpu().numpy(), pyy.cpu().numpy(), pxy.cpu().numpy()
    return [(sv.complete(int(m), h.W, h.H), a[i], b[i] if C == 2 else None, c[i] if C == 2 else None) for i, m in enumerate(each)]


def same_means(got, want):
    if got[0] != want[0]:
        return False
    return all((g is None and w is None) or same_bits(g, w) for g, w in zip(got[1:], want[1:]))


class Voice:
    def __init__(self, x, start_call=0, whole=False, end_with_last=True, discard_after=None):
        self.x, self.start_call, self.whole, self.end_with_last = x, start_call, whole, end_with_last
        self.discard_after = discard_after
        self.pushed, self.done, self.out, self.means = 0, False, [], []      # means: (frames pushed, what the call left)


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
        rows, means = h.call(blocks, counts, flags)
        for slot in range(h.S):
            if active[slot] is not None:
                active[slot].out.append(rows[slot])
                if means[slot] is not None:
                    active[slot].means.append((active[slot].pushed, means[slot]))
            else:
                assert len(rows[slot]) == 0 and means[slot] is None
        for slot in ended:
            active[slot] = None
        call += 1
    return call


def check_voices(h, plan):
    """Every voice's columns against the one-shot spectrogram, and its means after every call against the one-shot cross
    spectra of the frames pushed so far: two reference calls for the whole plan."""
    voices = [v for vs in plan.values() for v in vs]
    want = one_shot_columns(h, [v.x for v in voices])
    records = [(v, pushed, m) for v in voices for pushed, m in v.means]
    refs = one_shot_means(h, [v.x[:pushed] for v, pushed, _ in records]) if records and h.has_means else []
    for i, v in enumerate(voices):
        got = np.concatenate(v.out) if v.out else np.zeros((0, h.C, h.F), h.dtype)
        if v.discard_after is None:
            assert same_bits(got, want[i]) or h.cols is None, (i, got.shape, want[i].shape)
        else:                                                # what it returned before it was dropped is final all the same
            assert len(got) == sv.complete(v.discard_after, h.W, h.H) or h.cols is None
            assert same_bits(got, want[i][:len(got)]) or h.cols is None, i
    for (v, pushed, got), ref in zip(records, refs):
        assert same_means(got, ref), (voices.index(v), pushed, got[0], ref[0])
    return len(records)


# ---- 1. a ragged schedule ----------------------------------------------------------------------------------------------
RAGGED = [(64, 64, 32, 600), (64, 63, 63, 600), (128, 99, 1, 600), (256, 256, 128, 600), (1024, 513, 256, 600), (4096, 4096, 2048, 5000)]


def ragged_plan(W, M, dtype, seed):
    sig = lambda n, k, amp=1.0: noise(n, seed + k, amp, dtype)
    long = max(2049, 2 * W + 901)
    return {0: [Voice(sig(1, 0), whole=True), Voice(sig(long - 700, 1), start_call=2, end_with_last=False)],
            1: [Voice(sig(W - 1, 2)), Voice(sig(W + 1, 3), start_call=3)],
            2: [Voice(sig(W, 4), whole=W <= M), Voice(sig(W // 2 + 1, 5), start_call=1)],      # the second: shorter than nperseg
            3: [Voice(sig(long, 6, 1e3)), Voice(sig(W + 700, 7, 1e-3))],          # a loud voice, then a quiet one in its slot
            4: [Voice(sig(long, 8), discard_after=W + 450), Voice(sig(min(M, W + 333), 9), whole=True)],   # dropped by a START
            5: [Voice(sig(30, 10), start_call=1, end_with_last=False), Voice(sig(long + 13, 11))]}


@pytest.mark.parametrize('detrend', [True, False], ids=['detrend', 'plain'])
@pytest.mark.parametrize('layout', ['stereo', 'mono', 'strided'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('nfft,W,H,M', RAGGED, ids=['%d-%d-%d' % s[:3] for s in RAGGED])
def test_ragged_schedule(torch, ctx, nfft, W, H, M, dtype, layout, detrend):
    S = 6
    h = Harness(torch, ctx, S, M, W, H, nfft, dtype, layout, detrend, reset=False)
    text = h.native.describe_spectrum_voice_stream(S, h.C, W, H, nfft, M, h.f64)
    G = -(-h.rc // h.R) + 1
    assert text == (f'spectrum_voice_stream rows_per_call={h.rc} run={h.R} groups={G} nblocks={S * G} threads=256 '
                    f'advance_groups={S} state_bytes={h.need}')
    assert (np.abs(h.positions()) > 2 ** 60).all()          # NaN bytes until the reset
    h.reset()
    plan = ragged_plan(W, M, dtype, 1000 * W + H)
    menu = [0, 1, min(H, M), max(H - 1, 0), min(W - 1, M), M]     # idle calls, calls below the hop, calls that complete nothing
    calls = drive(h, plan, np.random.default_rng(W + H + nfft), menu)
    assert calls > 6
    assert check_voices(h, plan) > 12
    assert not h.positions().any()                           # every voice ended
    assert sum(len(r) for r in plan[5][0].out) == 0 and len(plan[5][0].out) >= 2      # shorter than nperseg: nothing, END included
    assert plan[5][0].means[-1][1][0] == 0 and not plan[5][0].means[-1][1][1].any()   # ... and its means are zeros over 0 segments


# ---- 2. run boundaries -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nfft,W,H,dtype,layout', [(256, 256, 128, np.float32, 'stereo'), (64, 63, 32, np.float64, 'mono'),
                                                   (2048, 2048, 1792, np.float64, 'stereo'), (4096, 4096, 2048, np.float64, 'stereo')],
                         ids=['256-f32-R32', '64-f64-mono-R32', '2048-f64-R2', '4096-f64-R1'])
def test_calls_that_end_at_run_boundaries(torch, ctx, nfft, W, H, dtype, layout):
    """Slot 1's calls end at R - 1, R, R + 1, 2 R and 2 R + 1 segments, then one call adds 2 R + 1 segments: the rest of run
    2, the whole of run 3 and a part of run 4.  Slot 0 pushes one hop a call beside it; slot 2 is idle."""
    from vndecorrelate_amd import _native
    R = _native.spectrum_run_length(nfft, W, H, dtype == np.float64, 2 if layout == 'stereo' else 1)
    assert R == {256: 32, 64: 32, 2048: 2, 4096: 1}[nfft]
    targets = sorted({R - 1, R, R + 1, 2 * R, 2 * R + 1}) + [4 * R + 2]
    frames = [W + (t - 1) * H if t > 0 else W - 1 for t in targets]
    M = max(np.diff([0] + frames))
    h = Harness(torch, ctx, 3, int(M), W, H, nfft, dtype, layout)
    assert -(-h.rc // R) + 1 >= 4                                # G: a call can touch run 2, 3, 4 and one more
    a, b = noise(frames[-1], 5, dtype=dtype), noise(H * len(frames), 6, dtype=dtype)
    va, vb = Voice(a), Voice(b)
    for i, q in enumerate(frames):
        last = i == len(frames) - 1
        blocks = [b[i * H:(i + 1) * H], a[va.pushed:q], None]
        flags = [(START if i == 0 else 0) | (END if last else 0)] * 2 + [0]
        rows, means = h.call(blocks, [H, q - va.pushed, 0], flags)
        va.pushed, vb.pushed = q, (i + 1) * H
        assert means[1][0] == targets[i] and means[2] is None
        for v, k in ((vb, 0), (va, 1)):
            v.out.append(rows[k])
            v.means.append((v.pushed, means[k]))
    assert check_voices(h, {0: [vb], 1: [va]}) == 2 * len(frames)


# ---- 3. every grid form ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', [7, 257, 513])
def test_pools_of_many_slots(torch, ctx, S):
    """Half the slots push M frames a call and half push one (S = 257); the others start one call late at random."""
    nfft, W, H, M = 64, 64, 32, 100
    h = Harness(torch, ctx, S, M, W, H, nfft)
    assert h.rc == 4 and h.R == 32 and h.lay['G'] == 2
    rng = np.random.default_rng(S)
    x, single = noise(260, S), noise(W + 3, S + 1)
    sizes = [100, 100, 60]
    late = rng.random(S) < 0.3
    slow = np.arange(S) % 2 == 1 if S == 257 else np.zeros(S, bool)
    got = [[] for _ in range(S)]
    final = [None] * S
    for i in range(len(sizes) + 1):
        counts, flags, blocks = np.zeros(S, np.int32), np.zeros(S, np.int32), [None] * S
        for b in range(S):
            k = i - int(late[b] and not slow[b])
            if slow[b]:                                        # W frames, then one frame a call
                blocks[b] = single[:W] if i == 0 else single[W - 1 + i:W + i]
                counts[b], flags[b] = len(blocks[b]), (START if i == 0 else 0) | (END if i == len(sizes) else 0)
            elif 0 <= k < len(sizes):
                p = sum(sizes[:k])
                blocks[b], counts[b] = x[p:p + sizes[k]], sizes[k]
                flags[b] = (START if k == 0 else 0) | (END if k == len(sizes) - 1 else 0)
        rows, means = h.call(blocks, counts, flags)
        for b in range(S):
            got[b].append(rows[b])
            final[b] = means[b] if means[b] is not None else final[b]
    cols, ref = one_shot_columns(h, [x, single]), one_shot_means(h, [x, single])
    assert len(cols[0]) == 7 and len(cols[1]) == 1
    for b in range(S):
        assert same_bits(np.concatenate(got[b]), cols[int(slow[b])]), b
        assert same_means(final[b], ref[int(slow[b])]), b
    assert not h.positions().any()


# ---- 4. positions ------------------------------------------------------------------------------------------------------
def per_segment_values(h, x, first, count):
    """The (Pxx, Pyy, re Pxy, im Pxy) values of segments first .. first + count - 1 of x, each (F, Q): the one-shot cross
    spectra of every segment alone - its mean over one segment is the segment's value."""
    segs = one_shot_means(h, [x[(first + t) * h.H:(first + t) * h.H + h.W] for t in range(count)])
    out = []
    for _, pxx, pyy, pxy in segs:
        out.append(pxx[:, None] if h.C == 1 else np.stack([pxx, pyy, pxy[:, 0], pxy[:, 1]], axis=1))
    return out


@pytest.mark.parametrize('layout,dtype', [('stereo', np.float32), ('mono', np.float64)], ids=['stereo-f32', 'mono-f64'])
@pytest.mark.parametrize('position', [2 ** 31 - 7, 2 ** 32 - 300, 2 ** 40 + 3], ids=['2^31-7', '2^32-300', '2^40+3'])
def test_planted_position(torch, ctx, position, layout, dtype):
    """Slot 1 at position P has sc(P) segments behind it; segment sc(P) starts at frame A = sc(P) x hop, in (P - W, P].  The
    signal starts at A: its frames below P go into the ring, the rest is pushed.  The ring frames [P - W + 1, A) are within
    reach of P but belong to no pending segment: they hold loud noise, everything else NaN.  total and partial are planted
    too, and the voice goes on as the documented order says: the host fold of the per-segment values."""
    S, nfft, W, H, M, n = 3, 256, 256, 128, 333, 10000
    P = position
    w0 = sv.complete(P, W, H)
    A = w0 * H
    held = P - A
    assert 0 < held < W - 1
    h = Harness(torch, ctx, S, M, W, H, nfft, dtype, layout)
    R = h.R
    assert R == 32 and w0 >= R and w0 % R != 0                   # both total and partial are read
    x = noise(held + n, 17 + P % 107, dtype=dtype)
    history = np.random.default_rng(P % 109).uniform(-1e3, 1e3, (W - 1, 2)).astype(dtype)
    history[W - 1 - held:] = x[:held]
    rng = np.random.default_rng(P % 113)
    total = rng.uniform(0.5, 1.5, (h.F, h.Q)) * 1e-2 * w0
    partial = rng.uniform(0.5, 1.5, (h.F, h.Q)) * 1e-2 * (w0 % R)
    h.plant(1, P, history[:, h.pick], total, partial)
    count = sv.complete(held + n, W, H)
    values = per_segment_values(h, x, 0, count)
    want_cols = one_shot_columns(h, [x])[0]
    fold = sv.Fold(R, (h.F, h.Q), total, partial, w0)
    other = Voice(noise(n, 5, dtype=dtype))
    got, pushed, first, done = [], 0, True, 0
    while pushed < n:
        b = int(min(n - pushed, rng.choice([0, 1, int(rng.integers(0, M + 1)), M])))
        blocks = [other.x[pushed:pushed + b], x[held + pushed:held + pushed + b], None]
        flags = np.array([START if first else 0, END if pushed + b == n else 0, 0], np.int32)
        rows, means = h.call(blocks, np.array([b, b, 0], np.int32), flags)
        pushed, first = pushed + b, False
        other.pushed = pushed
        other.out.append(rows[0])
        if means[0] is not None:
            other.means.append((pushed, means[0]))
        got.append(rows[1])
        for t in range(done, done + len(rows[1])):
            fold.push(values[t])
        done += len(rows[1])
        if means[1] is not None:
            want = fold.mean(dtype)
            assert means[1][0] == w0 + done == fold.count
            assert same_bits(means[1][1], want[:, 0]), (pushed, 'pxx')
            if h.C == 2:
                assert same_bits(means[1][2], want[:, 1]) and same_bits(means[1][3], want[:, 2:]), pushed
    assert done == count > 2 * R and same_bits(np.concatenate(got), want_cols)
    check_voices(h, {0: [other]})
    assert h.positions().tolist() == [n, 0, 0]


def test_a_position_past_2_to_60_answers_minus_one_until_a_start(torch, ctx):
    S, nfft, W, H, M = 3, 64, 64, 32, 100
    h = Harness(torch, ctx, S, M, W, H, nfft)
    x = noise(300, 8)
    vs = [Voice(x) for _ in range(S)]

    def step(blocks, counts, flags, who):
        rows, means = h.call(blocks, counts, flags)
        for b, pushed in who:
            vs[b].out.append(rows[b])
            vs[b].means.append((pushed, means[b]))
        return rows, means
    step([x[:100], None, x[:100]], [100, 0, 100], [START, 0, START], [(0, 100), (2, 100)])
    h.plant(1, 2 ** 60 + 1, np.zeros((0, 2), np.float32))
    ring, sums = h.part('ring').cpu().numpy().copy(), h.part('sums').cpu().numpy().copy()
    rows, means = step([x[100:200], x[:100], x[100:200]], [100, 100, 100], [0, 0, 0], [(0, 200), (2, 200)])
    assert h.oc.cpu().numpy()[1] == -1 and h.positions()[1] == 2 ** 60 + 1 and means[1] is None    # (the harness held them to the mirror)
    assert same_bits(h.part('ring').cpu().numpy()[1], ring[1]) and same_bits(h.part('sums').cpu().numpy()[1], sums[1])
    step([x[200:], x[:100], x[200:]], [100, 100, 100], [END, START, END], [(0, 300), (1, 100), (2, 300)])     # works again with START
    step([None, x[100:200], None], [0, 100, 0], [0, 0, 0], [(1, 200)])
    step([None, x[200:], None], [0, 100, 0], [0, END, 0], [(1, 300)])
    assert check_voices(h, {b: [vs[b]] for b in range(S)}) == 9


@pytest.mark.parametrize('bad_count', [101, -1, 2 ** 31 - 1, -2 ** 31])
def test_a_bad_count_leaves_the_slot_and_its_neighbours_alone(torch, ctx, bad_count):
    S, nfft, W, H, M = 4, 64, 64, 32, 100
    x = [noise(300, 20 + b) for b in range(S)]
    h = Harness(torch, ctx, S, M, W, H, nfft)
    vs = [Voice(x[b]) for b in range(S)]
    for i in range(3):
        blocks = [x[b][100 * i:100 * i + 100] for b in range(S)]
        counts = np.full(S, 100, np.int32)
        flags = np.full(S, (START if i == 0 else 0) | (END if i == 2 else 0), np.int32)
        if i == 1:                                               # slot 2, live since call 0, sends a bad count
            counts[2] = bad_count
            ring, sums = h.part('ring').cpu().numpy().copy(), h.part('sums').cpu().numpy().copy()
        rows, means = h.call(blocks, counts, flags)
        for b in range(S):
            if i == 1 and b == 2:
                assert h.oc.cpu().numpy()[2] == -1 and h.positions()[2] == 100 and means[2] is None and len(rows[2]) == 0
                assert same_bits(h.part('ring').cpu().numpy()[2], ring[2]) and same_bits(h.part('sums').cpu().numpy()[2], sums[2])
                continue
            vs[b].out.append(rows[b])
            vs[b].means.append((100 * (i + 1), means[b]))
        if i == 1:                                               # the voice goes on: the block it meant to push
            only = np.zeros(S, np.int32)
            only[2] = 100
            rows, means = h.call(blocks, only, np.zeros(S, np.int32))
            vs[2].out.append(rows[2])
            vs[2].means.append((200, means[2]))
            assert all(m is None for b, m in enumerate(means) if b != 2)
    assert check_voices(h, {b: [vs[b]] for b in range(S)}) == 3 * S


def test_without_columns_and_without_means(torch, ctx):
    """A null cols_dev gives the same means; null means give the same columns."""
    S, nfft, W, H, M = 3, 128, 99, 40, 300
    x = [noise(1000, 40 + b) for b in range(S)]
    kinds = dict(both=Harness(torch, ctx, S, M, W, H, nfft), means=Harness(torch, ctx, S, M, W, H, nfft, columns=False),
                 cols=Harness(torch, ctx, S, M, W, H, nfft, means=False))
    rng = np.random.default_rng(4)
    pushed = 0
    while pushed < 1000:
        n = int(min(1000 - pushed, rng.integers(0, M + 1)))
        flags = [(START if pushed == 0 else 0) | (END if pushed + n == 1000 else 0)] * S
        got = {k: h.call([s[pushed:pushed + n] for s in x], [n] * S, flags) for k, h in kinds.items()}
        pushed += n
        for b in range(S):
            assert same_bits(got['both'][0][b], got['cols'][0][b]) and got['cols'][1][b] is None and not len(got['means'][0][b])
            if got['both'][1][b] is None:                        # an idle call
                assert got['means'][1][b] is None and n == 0
            else:
                assert same_means(got['both'][1][b], got['means'][1][b])
    ref = one_shot_means(kinds['both'], x)
    assert all(same_means(got['means'][1][b], ref[b]) for b in range(S)) and ref[0][0] == 23


# ---- 5. the Python pool: capture, metering a decorrelating pool, the dict form ---------------------------------------
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


def test_graph_replay_equals_the_uncaptured_run(torch, ctx):
    from vndecorrelate_amd import spectral
    S, M = 6, 600
    dev = torch.device('cuda', ctx.device)
    calls = device_schedule(S, M, 3)
    results = []
    for replayed in (False, True):
        pool = spectral.spectrum_voice_pool(S, M)
        assert (pool.nperseg, pool.hop, pool.bins, pool.rows_per_call, pool.run) == (256, 128, 129, 5, 32)
        x = torch.empty((S, M, 2), dtype=torch.float32, device=dev)
        counts, flags, oc = (torch.empty(S, dtype=torch.int32, device=dev) for _ in range(3))
        cols = torch.empty((S, pool.rows_per_call, 2, pool.bins), dtype=torch.int32, device=dev)
        out = (cols.view(torch.float32), oc)
        pool.reset()
        where = (pool.pxx.data_ptr(), pool.pyy.data_ptr(), pool.pxy.data_ptr(), pool.segments.data_ptr())
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
            cols.fill_(POISON32)
            if graph is not None:
                graph.replay()
            else:
                pool.process_dev(x, counts, flags, out=out)
            torch.cuda.synchronize(dev)
            got.append((cols.cpu().numpy(), oc.cpu().numpy(), pool.pxx.cpu().numpy(), pool.pyy.cpu().numpy(),
                        pool.pxy.cpu().numpy(), pool.segments.cpu().numpy(), pool.coherence().cpu().numpy()))
        assert where == (pool.pxx.data_ptr(), pool.pyy.data_ptr(), pool.pxy.data_ptr(), pool.segments.data_ptr())
        with pytest.raises(RuntimeError, match='runs through process_dev'):
            pool.process({})
        results.append(got)
    pos = np.zeros(S, np.int64)
    for i, (plain, again) in enumerate(zip(*results)):
        want, segs, pos = spectral.spectrum_voice_spans(pos, calls[i][1], calls[i][2], 256, 128, M)
        assert plain[1].tolist() == want.tolist() == again[1].tolist(), i
        assert all(a.tobytes() == b.tobytes() for a, b in zip(plain, again)), i
        for b, n in enumerate(want):
            assert not (plain[0][b, :n] == POISON32).any() and (plain[0][b, n:] == POISON32).all(), (i, b)
            assert segs[b] < 0 or plain[5][b] == segs[b]
    assert any(n > 0 for r in results[0] for n in r[1]) and not pos.any()


def _meter_run(torch, ctx, pool, meter, extra, voices, stage_counts):
    """`pool` and `meter` captured together in one graph; voices: per slot (signal, bank entry).  Every slot starts on call
    0 and pushes blocks of its own sizes, END with its last block.  After call 0 a replay carries a bad count for slot 2
    and nothing for the others: stage_counts() - every stage's out_counts - must answer -1 for it, and the voice goes on.
    Returns the columns per slot and, per slot, the means and the coherence its END call left."""
    S, M = pool.slots, pool.max_frames_per_call
    dev = torch.device('cuda', ctx.device)
    x = torch.empty((S, M, 2), dtype=torch.float32, device=dev)
    counts, flags, oc = (torch.empty(S, dtype=torch.int32, device=dev) for _ in range(3))
    idt, poison = (torch.int64, POISON64) if meter.dtype == np.float64 else (torch.int32, POISON32)
    cols = torch.empty((S, meter.rows_per_call, 2, meter.bins), dtype=idt, device=dev)
    pool.reset()
    meter.reset()
    coherence = torch.empty((S, meter.bins), dtype=meter.pxx.dtype, device=dev)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
    with torch.cuda.graph(graph, stream=side):
        y, mid = pool.process_dev(x, counts, flags, *extra)
        meter.process_dev(y, mid, flags, out=(cols.view(meter.pxx.dtype), oc))
        coherence.copy_(meter.coherence())
    torch.cuda.synchronize(dev)

    def replay(xh, c, f):
        for t, v in ((x, xh), (counts, c), (flags, f)):
            t.copy_(torch.from_numpy(v))
        cols.fill_(poison)
        graph.replay()
        torch.cuda.synchronize(dev)
        return cols.cpu().numpy(), oc.cpu().numpy()
    rng = np.random.default_rng(S)
    pushed, started, got, final, call = [0] * S, [False] * S, [[] for _ in range(S)], [None] * S, 0
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
            assert n >= 0 and not (rh[b, :n] == poison).any() and (rh[b, n:] == poison).all(), (call, b)
            got[b].append(rh[b, :n].view(meter.dtype).copy())
            if f[b] & END:
                final[b] = (int(meter.segments[b].cpu()), meter.pxx[b].cpu().numpy(), meter.pyy[b].cpu().numpy(),
                            meter.pxy[b].cpu().numpy(), coherence[b].cpu().numpy())
        if call == 0:
            assert pushed[2] is not None
            bad = np.zeros(S, np.int32)
            bad[2] = M + 1
            before = meter.pxx.cpu().numpy()
            rh, ch = replay(xh, bad, np.zeros(S, np.int32))
            assert [int(t.cpu()[2]) for t in stage_counts(mid)] + [int(ch[2])] == [-1] * (len(stage_counts(mid)) + 1)
            assert (rh == poison).all() and [int(v) for v in ch[[0, 1, 3]]] == [0, 0, 0]
            assert same_bits(meter.pxx.cpu().numpy(), before)    # a bad slot and idle ones: the means stay
        call += 1
    return [np.concatenate(g) for g in got], final


def _check_metered(torch, ctx, got, final, outputs, dtype):
    """Per voice against spectrogram_batched and coherence_batched of the one-shot output (device tensors in, so that the
    ratio is formed by the same torch operations)."""
    from vndecorrelate_amd import spectral
    dev = torch.device('cuda', ctx.device)
    kw = dict(window='hann', nperseg=256, noverlap=128)
    for b, out in enumerate(outputs):
        out = np.ascontiguousarray(out)
        assert out.dtype == dtype and out.ndim == 2 and out.shape[1] == 2
        t = torch.from_numpy(out[None]).to(dev)
        sxx = spectral.spectrogram_batched(t, **kw)[2][0].cpu().numpy()                # (C, F, T)
        assert sxx.shape[2] > 8 and same_bits(got[b], np.ascontiguousarray(sxx.transpose(2, 0, 1))), b
        segments, pxx, pyy, pxy, coherence = final[b]
        assert segments == sxx.shape[2]
        want = spectral.welch_batched(t, **kw)[1][0].cpu().numpy()
        assert same_bits(pxx, want[0]) and same_bits(pyy, want[1]), b
        assert same_bits(pxy, torch.view_as_real(spectral.csd_batched(t, **kw)[1][0]).cpu().numpy()), b
        assert same_bits(coherence, spectral.coherence_batched(t, **kw)[1][0].cpu().numpy()), b
        assert np.isfinite(coherence).all() and 0 <= coherence.min() and coherence.max() <= 1 + 1e-5


def test_metering_a_velvet_voice_pool_in_one_graph(torch, ctx):
    import vndecorrelate_amd.decorrelation as dec
    from test_gpu_chain_voice_pool import DURATION, FS, IMPULSES, KAPPAS, SEED
    from vndecorrelate_amd import spectral
    S, M = 4, 600
    bank = [dec.VelvetNoise(sample_rate_hz=FS, duration_seconds=DURATION, num_impulses=IMPULSES, seed=SEED, normalizer=None,
                            log_distribution_strength=k) for k in KAPPAS]
    pool = dec.decorrelate_voice_pool(bank, slots=S, in_channels=2, max_frames_per_call=M)
    meter = spectral.spectrum_voice_pool(S, pool.row_frames)
    dev = torch.device('cuda', ctx.device)
    entries = np.array([3, 0, 2, 1])
    extra = (torch.from_numpy(pool.bank_tables[entries].astype(np.int32)).to(dev),)
    voices = [(noise(n, 70 + b), int(entries[b])) for b, n in enumerate((1700, 1900, 2300, 2201))]
    got, final = _meter_run(torch, ctx, pool, meter, extra, voices, lambda mid: (mid,))
    _check_metered(torch, ctx, got, final, [bank[e].decorrelate(sig) for sig, e in voices], np.float32)


def test_metering_a_chain_voice_pool_in_one_graph(torch, ctx):
    import vndecorrelate_amd.decorrelation as dec
    from test_gpu_chain_voice_pool import _bank
    from vndecorrelate_amd import spectral
    S, M = 4, 600
    bank = _bank(dec, 'ms>lr-ch1')
    pool = dec.decorrelate_voice_pool(bank, slots=S, in_channels=2, max_frames_per_call=M)
    meter = spectral.spectrum_voice_pool(S, pool.row_frames, dtype='float64')
    dev = torch.device('cuda', ctx.device)
    entries = np.array([3, 0, 2, 1])
    extra = (torch.from_numpy(pool.bank_tables[entries].astype(np.int32)).to(dev),
             torch.from_numpy(pool.bank_delays[entries].astype(np.int32)).to(dev))
    voices = [(noise(n, 60 + b), int(entries[b])) for b, n in enumerate((1700, 1900, 2300, 2201))]
    got, final = _meter_run(torch, ctx, pool, meter, extra, voices, lambda mid: (pool._mid[1], mid))    # -1 from all three stages
    _check_metered(torch, ctx, got, final, [bank[e](sig) for sig, e in voices], np.float64)


def test_dict_form_equals_the_batched_calls_per_voice(torch, ctx):
    from vndecorrelate_amd import spectral
    S, M = 4, 480
    kw = dict(window='hann', nperseg=256, noverlap=128)
    for dtype, channels in ((np.float32, 2), (np.float64, 1)):
        pool = spectral.spectrum_voice_pool(S, M, dtype=dtype, channels=channels)
        rng = np.random.default_rng(9)
        sigs = {s: noise(n, s + 1, dtype=dtype)[:, :channels] for s, n in enumerate((1500, 2000, 300, 961))}
        got, pushed, means = {s: [] for s in sigs}, {s: 0 for s in sigs}, {}
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
                assert r.dtype == dtype and r.shape[1:] == (channels, 129)
                got[s].append(r)
            for s in end:
                means[s] = pool.welch(s)
        for s, sig in sigs.items():
            sxx = spectral.spectrogram_batched(sig[None], **kw)[2][0]
            assert same_bits(np.concatenate(got[s]), np.ascontiguousarray(sxx.transpose(2, 0, 1))), s
            segments, pxx, pyy, pxy = means[s]
            assert segments == sxx.shape[2] == (len(sig) - 256) // 128 + 1
            want = spectral.welch_batched(sig[None], **kw)[1][0]
            assert same_bits(pxx, want[0])
            if channels == 2:
                assert same_bits(pyy, want[1]) and same_bits(pxy, spectral.csd_batched(sig[None], **kw)[1][0])
            else:
                assert pyy is None and pxy is None
        assert not pool.positions.any() and not pool.live.any()
        again = pool.process({2: sigs[0][:480]}, start=[2], end=[2])                  # a reused slot, a whole voice in one block
        assert same_bits(again[2], np.ascontiguousarray(spectral.spectrogram_batched(sigs[0][None, :480], **kw)[2][0].transpose(2, 0, 1)))
        with pytest.raises(RuntimeError, match='runs through process\\(\\)'):
            pool.process_dev(None, None, None)
        if channels == 2:
            assert pool.coherence().shape == (S, 129)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_bad_arguments_write_nothing(torch, ctx, dtype):
    lib = ctx._lib
    S, nfft, W, H, M = 3, 64, 64, 32, 100
    h = Harness(torch, ctx, S, M, W, H, nfft, dtype, reset=False)
    h.upload([np.ones((M, 2), dtype)] * S, [M] * S, [START] * S)
    cases = sv.refusals(h.args(), h.dtype.itemsize) + [(dict(ctx=None), INVALID)]
    for kw, status in cases:
        assert h.raw(**kw) == status, (kw, lib.vnd_last_error())
        assert lib.vnd_last_error()
    assert b'null context' in lib.vnd_last_error()
    null = ctypes.c_void_p(None)
    reset = lib.vnd_spectrum_voice_stream_reset_dev
    state = ctypes.c_void_p(h.state.data_ptr())
    assert reset(ctx.handle, null, h.need, S, 2, W, H, nfft, M, int(h.f64), null) == INVALID
    assert reset(ctx.handle, state, h.need - 1, S, 2, W, H, nfft, M, int(h.f64), null) == INVALID
    assert reset(ctx.handle, ctypes.c_void_p(h.state.data_ptr() + 4), h.need, S, 2, W, H, nfft, M, int(h.f64), null) == INVALID
    assert reset(ctx.handle, state, h.need, S, 2, W, H, 100, M, int(h.f64), null) == UNSUPPORTED
    torch.cuda.synchronize(h.dev)
    assert (h.cols == h.poison).all() and torch.isnan(h.state).all() and (h.oc == -77).all()
    assert all((t == h.poison).all() for t in (h.pxx, h.pyy, h.pxy)) and (h.segments == -77).all()
    h.reset()
    rows, means = h.call([np.ones((M, 2), dtype)] * S, [M] * S, [START] * S)          # the good call writes
    assert all(len(r) == 2 and m[0] == 2 for r, m in zip(rows, means))
